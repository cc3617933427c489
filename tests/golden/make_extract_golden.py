"""Regenerates tests/golden/extract_cases.json: size and sha256 of what the
reference CLI (oracle/_ref/main, built by `make -C oracle`) writes for
`compress` of column cuts of random_100x10000.vcf.  Data only: the column
sets are named by a range or by a seeded sample (extract_cases.golden_columns).

    python tests/golden/make_extract_golden.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))

import extract_cases as EC   # noqa: E402
import golden_io as G        # noqa: E402
import subset_cases as SC    # noqa: E402

REF_MAIN = os.path.join(REPO, "oracle", "_ref", "main")
NAME = "random_100x10000"
SETS = [{"range": [0, 100, 1]}, {"range": [99, -1, -1]}, {"range": [0, 100, 2]}, {"range": [17, 18, 1]},
        {"range": [30, 95, 1]}, {"sample": [1, 3]}, {"sample": [2, 64]}, {"sample": [3, 99]}]


def main():
    assert os.path.exists(REF_MAIN), "build oracle/_ref first (make -C oracle)"
    vcf = G.gz(NAME + ".vcf.gz")
    S = SC.parse_header(G.gz(NAME + ".vcfc.gz"))[1]
    cases = []
    with tempfile.TemporaryDirectory() as wd:
        for spec in SETS:
            ip, op = os.path.join(wd, "cut.vcf"), os.path.join(wd, "cut.vcfc")
            with open(ip, "wb") as f:
                f.write(SC.cut_vcf(vcf, EC.golden_columns(spec, S)))
            r = subprocess.run([REF_MAIN, "compress", ip, op], capture_output=True)
            assert r.returncode == 0, r.stderr
            with open(op, "rb") as f:
                out = f.read()
            cases.append({"cols": spec, "size": len(out), "sha256": hashlib.sha256(out).hexdigest()})
    with open(os.path.join(HERE, "extract_cases.json"), "w") as f:
        json.dump({"file": NAME + ".vcfc.gz", "generator": "tests/golden/make_extract_golden.py (oracle/_ref/main compress)",
                   "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
