"""Golden vectors for the binned external index: exit code, <file>.vcfci bytes
and stdout of the reference CLI's `main create-binned-index <bin> <file.vcfc>`
and `main query-binned-index <file.vcfc> <region>` (oracle/_ref/main, compiled
from the reference's sources by oracle/Makefile), over the committed
random_100x10000 fixture, a small seeded file of edge records and three files
the reference throws on.  Run where the reference build exists; writes
binned_index_cases.json (data only).

edge_cases(): the same two actions over the hand-built edge files of
tests/index_edge_cases.py whose records all hold their TABs (pinned_files());
make_sparse_index_golden.py --edge records them, with its own, into
index_edge_cases.json."""
import hashlib
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF_MAIN = os.path.join(REPO, "oracle", "_ref", "main")
sys.path.insert(0, os.path.join(REPO, "tests"))
import golden_io as G          # noqa: E402
import index_cases as X        # noqa: E402

BINS = [1, 2, 7, 100]
HDR = X.header(3)


def run(args, cwd):
    r = subprocess.run([REF_MAIN] + args, cwd=cwd, capture_output=True, timeout=300)
    return r.returncode, r.stdout


def row(chrom, pos, k, ref, alt, info, rnd):
    gts = b"\t".join(rnd.choice([b"0|0", b"0|1", b"1|1"]) for _ in range(3))
    return b"%s\t%d\trs%d\t%s\t%s\t50\tPASS\t%s\tGT\t%s\n" % (chrom, pos, k, ref, alt, info, gts)


def index_edge_vcf():
    """~100 records x 3 samples: CHROM 1, 2, chrZ, X with POS restarting on
    each, equal POS values, long-REF deletions overlapping later records,
    multi-ALT, <DEL> with END, <CN0>,<CN2> with negative and multiple SVLEN,
    <INS:...> with neither, INFO holding ';;', 'X==' and a flag key, and
    END=5,<big>,7;SVLEN=9."""
    rnd = random.Random(20261019)
    body, k = [], 0
    for chrom in (b"1", b"2", b"chrZ", b"X"):
        pos = 100
        for j in range(25):
            pos += rnd.choice([0, 1, 3, 10, 50])
            ref, alt, info = bytes([rnd.choice(b"ACGT")]), bytes([rnd.choice(b"ACGT")]), b"AC=%d;AF=0.25" % (1 + j % 5)
            if j == 3:
                ref = b"A" + b"CGT" * 13
            elif j == 7:
                alt = b"G,GTTTT,C"
            elif j == 9:
                alt = b"A,,TTT"
            elif j == 10:
                alt, info = b"<DEL>", b"SVTYPE=DEL;END=%d" % (pos + 500)
            elif j == 12:
                alt, info = b"<CN0>,<CN2>", b"SVTYPE=CNV;SVLEN=-300,120"
            elif j == 15:
                alt, info = b"<INS:ME:ALU>", b"SVTYPE=ALU;TSD=null"
            elif j == 17:
                alt, info = b"<DUP>", b"DB;;X==;SVLEN=50;;"
            elif j == 20 and chrom == b"1":
                alt, info = b"<DEL>", b"END=5,%d,7;SVLEN=9" % (pos + 2000)
            elif j == 20:
                alt, info = b"<DEL>", b"SVLEN=9;END=5"
            elif j == 22:
                alt = b"."
            body.append(row(chrom, pos, k, ref, alt, info, rnd))
            k += 1
    return HDR + b"".join(body)


def throw_vcfs():
    """A good base of 10 rows, and three files that continue it with one row
    the reference throws on (bad POS; a pair A=B=C on a structural record;
    END=12x) and two more rows.  The base's index is valid for their first
    records, so a query can walk into the bad row."""
    rnd = random.Random(7)
    base = b"".join(row(b"1", 100 + 10 * j, j, b"A", b"G", b"AC=1", rnd) for j in range(10))
    tail = row(b"1", 300, 11, b"A", b"T", b"AC=2", rnd) + row(b"1", 310, 12, b"C", b"T", b"AC=3", rnd)
    bad = {"throw_pos": row(b"1", 200, 10, b"A", b"G", b"AC=1", rnd).replace(b"\t200\t", b"\t20x\t"),
           "throw_kvp": row(b"1", 200, 10, b"A", b"<DEL>", b"SVTYPE=DEL;A=B=C;END=250", rnd),
           "throw_end": row(b"1", 200, 10, b"A", b"<DEL>", b"SVTYPE=DEL;END=12x", rnd)}
    out = {"throw_base": HDR + base}
    for name, r in bad.items():
        out[name] = HDR + base + r + tail
    return out


QUERIES = {
    "random_100x10000.vcfc.gz": ["1:10100-10104", "1:5-9999", "1:30000-40000", "foo:1-9", "2:1-100", "1:100-50", "1",
                                 "1:29990-30010", "1:20001-20001", "1:10000-10000", "1:19999-20405", "X:1-10",
                                 "1:10198-10200", "1:10199-10199", "1:25000-25001"],
    "index_edge": ["1:100-200", "1:1-50", "1:300-100", "1", "1:150-100000", "2:100-150", "2:120-4000",
                   "chrZ:1-100000", "foo:1-9", "foo:200-300", "X:100-400", "X:100000-200000", "3:1-1000", "1:600-2700",
                   "2:580-640", "X:560-561"],
}


def main():
    if not os.path.exists(REF_MAIN):
        sys.exit("build the reference first: make -C oracle")
    files = {"random_100x10000.vcfc.gz": G.gz("random_100x10000.vcfc.gz")}
    index_cases, query_cases, cli_cases = [], [], []
    with tempfile.TemporaryDirectory() as wd:
        vcfs = {"index_edge": index_edge_vcf()}
        vcfs.update(throw_vcfs())
        for name, vcf in vcfs.items():
            src = os.path.join(wd, name + ".vcf")
            with open(src, "wb") as f:
                f.write(vcf)
            rc, _ = run(["compress", src, src + "c"], wd)
            assert rc == 0, (name, rc)
            files[name] = open(src + "c", "rb").read()
        path = os.path.join(wd, "f.vcfc")
        indexes = {}
        for name, data in files.items():
            with open(path, "wb") as f:
                f.write(data)
            for b in BINS:
                if os.path.exists(path + ".vcfci"):
                    os.unlink(path + ".vcfci")
                rc, out = run(["create-binned-index", str(b), path], wd)
                idx = open(path + ".vcfci", "rb").read()
                indexes[(name, b)] = idx
                c = {"file": name, "bin": b, "rc": rc, "index_len": len(idx),
                     "index_sha256": hashlib.sha256(idx).hexdigest()}
                if len(idx) <= 4096:
                    c["index_hex"] = idx.hex()
                if name.startswith("throw_") and name != "throw_base":
                    assert rc not in (0, 1) and idx == b"", (name, rc)
                else:
                    assert rc == 0 and out == b"", (name, rc, out)
                index_cases.append(c)

        def query_case(name, index_file, b, region):
            idx = indexes[(index_file, b)]
            with open(path, "wb") as f:
                f.write(files[name])
            with open(path + ".vcfci", "wb") as f:
                f.write(idx)
            rc, out = run(["query-binned-index", path, region], wd)
            return {"file": name, "index_file": index_file, "bin": b, "region": region, "rc": rc,
                    "stdout_len": len(out), "stdout_sha256": hashlib.sha256(out).hexdigest()}

        backed = set()
        for name, regions in QUERIES.items():
            for b in BINS:
                idx = indexes[(name, b)]
                if len(idx) // 13 < 2:
                    continue   # (the reference reads an uninitialised entry there)
                for region in regions:
                    c = query_case(name, name, b, region)
                    assert c["rc"] == 0, c
                    ref, hr, a, e = G.oracle_parse_query(region.encode())
                    if X.search(idx, X.ref_idx(ref), a if hr else 0)[1]:
                        backed.add((name, b))
                    query_cases.append(c)
        assert ("random_100x10000.vcfc.gz", 100) in backed and any(n == "index_edge" for n, _ in backed), backed
        for name in ("throw_pos", "throw_kvp", "throw_end"):
            assert len(indexes[("throw_base", 2)]) // 13 >= 2
            for region in ("1:100-1000", "1:305-400", "1:100-150"):
                c = query_case(name, "throw_base", 2, region)
                assert (c["rc"] == 0) == (region == "1:100-150"), c
                query_cases.append(c)
        used = {(c["index_file"], c["bin"]) for c in query_cases}
        assert all(len(indexes[k]) // 13 >= 2 for k in used)
        # argv checks and messages (src/main.cpp:4097-4143); {f}: an existing .vcfc with its index, {m}: a missing file
        with open(path, "wb") as f:
            f.write(files["index_edge"])
        with open(path + ".vcfci", "wb") as f:
            f.write(indexes[("index_edge", 2)])
        noidx = os.path.join(wd, "noidx.vcfc")
        with open(noidx, "wb") as f:
            f.write(files["index_edge"])
        sub = {"{f}": path, "{m}": os.path.join(wd, "missing.vcfc"), "{n}": noidx}
        for argv in (["create-binned-index"], ["create-binned-index", "2"], ["create-binned-index", "2", "{f}", "x"],
                     ["create-binned-index", "abc", "{f}"], ["create-binned-index", "2x", "{f}"],
                     ["query-binned-index"], ["query-binned-index", "{f}"], ["query-binned-index", "{m}", "1:1-2"],
                     ["query-binned-index", "{n}", "1:1-2"], ["query-binned-index", "{f}", "1:5"],
                     ["query-binned-index", "{f}", "1:a-5"], ["query-binned-index", "{f}", "1:5-x"]):
            rc, out = run([sub.get(a, a) for a in argv], wd)
            for k, v in sub.items():
                out = out.replace(v.encode(), k.encode())
            assert rc == 1, (argv, rc)
            cli_cases.append({"argv": argv, "rc": rc, "stdout": out.decode()})
    inline = {k: v.hex() for k, v in files.items() if not k.endswith(".gz")}
    with open(os.path.join(HERE, "binned_index_cases.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_binned_index_golden.py (reference: oracle/_ref/main)",
                   "inline_files": inline, "index_cases": index_cases, "query_cases": query_cases,
                   "cli_cases": cli_cases}, f, indent=1)
    print(len(index_cases), "index cases,", len(query_cases), "query cases,", len(cli_cases), "cli cases; backed up:",
          sorted(backed))
    for (name, b), idx in sorted(indexes.items()):
        print(name, b, len(idx) // 13, "entries")


EDGE_BINS = [1, 2, 64]


def edge_cases(wd, files, queries):
    """(index cases, query cases) of the reference over `files` {name: .vcfc
    bytes}: the index at bins 1, 2 and 64 as its length and digest, and for
    queries[name] = (bin, regions) the stdout of each region against the
    reference's own index."""
    index_cases, query_cases = [], []
    path = os.path.join(wd, "e.vcfc")
    for name, data in files.items():
        with open(path, "wb") as f:
            f.write(data)
        for b in EDGE_BINS:
            if os.path.exists(path + ".vcfci"):
                os.unlink(path + ".vcfci")
            rc, out = run(["create-binned-index", str(b), path], wd)
            idx = open(path + ".vcfci", "rb").read() if os.path.exists(path + ".vcfci") else b""
            index_cases.append({"file": name, "bin": b, "rc": rc, "index_len": len(idx),
                                "index_sha256": hashlib.sha256(idx).hexdigest()})
            if name in queries and queries[name][0] == b:
                assert rc == 0 and len(idx) // 13 >= 2, (name, b, rc)
                for region in queries[name][1]:
                    rc, out = run(["query-binned-index", path, region], wd)
                    query_cases.append({"file": name, "bin": b, "region": region, "rc": rc, "stdout_len": len(out),
                                        "stdout_sha256": hashlib.sha256(out).hexdigest()})
    return index_cases, query_cases


if __name__ == "__main__":
    main()
