"""Golden records for the sparse-layout edge files (tests/sparse_cases.py):
exit code and hole-aware digest of the file that the reference CLI's own
`main sparsify` (oracle/_ref/main, compiled from the reference's sources by
oracle/Makefile; sparsify_file, src/sparse.cpp:290-580) leaves for every
disk-bound case of pos_forms, adjacent, err_order and tail_bad, for block_edge
at n = 257 with each defect, and for the header-only file.  Run in the build
container (needs the reference build and a filesystem with holes); writes
sparse_edge_cases.json.

The inputs are not stored: the tests regenerate them from sparse_cases.py
and check their sha256 against the one recorded here.  The reference writes
with one syscall per byte and no buffer of its own, so the file it leaves
behind a throw is fixed; each case runs twice to check that, and a case whose
two files differ gets its rc only ("digest": null, "note")."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF_MAIN = os.path.join(REPO, "oracle", "_ref", "main")
sys.path[:0] = [os.path.join(REPO, "tests"), HERE]

import sparse_cases as C  # noqa: E402
import sparse_digest  # noqa: E402


def run_ref(wd, v):
    vp, sp = os.path.join(wd, "in.vcfc"), os.path.join(wd, "out.sparse")
    with open(vp, "wb") as f:
        f.write(v)
    if os.path.exists(sp):
        os.unlink(sp)
    r = subprocess.run([REF_MAIN, "sparsify", vp, sp], cwd=wd, capture_output=True, timeout=600)
    return r.returncode, sparse_digest.digest(sp) if os.path.exists(sp) else None


def main():
    if not os.path.exists(REF_MAIN):
        sys.exit("build the reference first: make -C oracle")
    cases = {}
    with tempfile.TemporaryDirectory(dir="/tmp") as wd:
        for name, v in C.golden_cases():
            rc, dg = run_ref(wd, v)
            rc2, dg2 = run_ref(wd, v)
            assert rc == rc2, (name, rc, rc2)
            c = {"input_sha256": C.sha(v), "rc": rc, "digest": dg}
            if dg != dg2:
                c["digest"] = None
                c["note"] = "the partial file differs between two runs of the reference: rc only"
            cases[name] = c
    with open(os.path.join(HERE, "sparse_edge_cases.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_sparse_edge_golden.py (reference: oracle/_ref/main sparsify)",
                   "cases": cases}, f, indent=1)
    print(len(cases), "cases,", sum(c["rc"] != 0 for c in cases.values()), "with a non-zero rc,",
          sum(c["digest"] is None for c in cases.values()), "without a digest")


if __name__ == "__main__":
    main()
