"""Golden vectors for region-list queries: the reference CLI's
`main query <file.vcfc> <region>` (oracle/_ref/main, compiled from the
reference's sources by oracle/Makefile) once per region over
random_100x10000.vcfc.gz (one CHROM "1", POS 10000..29998 in steps of 2, every
line unique: checked here), and the union of its outputs in file order, each
line once -- what `query-regions` has to write.  Run where the reference build
exists; writes regions_cases.json."""
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF_MAIN = os.path.join(REPO, "oracle", "_ref", "main")
FILE = "random_100x10000.vcfc.gz"
REGIONS = ["1:10000-10100", "1:15000-15999", "1:15500-16500", "1:29998-40000", "2", "1:20001-20001", "1:20002-20002"]


def gz(name):
    with gzip.open(os.path.join(HERE, name), "rb") as f:
        return f.read()


def main():
    if not os.path.exists(REF_MAIN):
        sys.exit("build the reference first: make -C oracle")
    lines = [l for l in gz(FILE.replace(".vcfc", ".vcf")).split(b"\n")[:-1] if not l.startswith(b"#")]
    assert len(set(lines)) == len(lines), "the file's lines are not unique"
    order = {l: i for i, l in enumerate(lines)}
    assert [int(l.split(b"\t")[1]) for l in lines] == list(range(10000, 30000, 2))
    assert all(l.startswith(b"1\t") for l in lines)
    union, counts = set(), []
    with tempfile.TemporaryDirectory() as wd:
        path = os.path.join(wd, "q.vcfc")
        with open(path, "wb") as f:
            f.write(gz(FILE))
        for region in REGIONS:
            r = subprocess.run([REF_MAIN, "query", path, region], cwd=wd, capture_output=True, timeout=300)
            assert r.returncode == 0, (region, r.returncode)
            got = r.stdout.split(b"\n")[:-1]
            assert all(l in order for l in got), region
            counts.append(len(got))
            union.update(got)
    out = b"".join(l + b"\n" for l in sorted(union, key=order.get))
    with open(os.path.join(HERE, "regions_cases.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_regions_golden.py (reference: oracle/_ref/main)", "file": FILE,
                   "regions": "".join(r + "\n" for r in REGIONS), "region_lines": counts,
                   "union_lines": out.count(b"\n"), "union_sha256": hashlib.sha256(out).hexdigest()}, f, indent=1)
        f.write("\n")
    print(counts, out.count(b"\n"))


if __name__ == "__main__":
    main()
