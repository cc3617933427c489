"""Golden vectors for the sparse external index and gap-analysis: exit code,
<file>.vcfci-sparse contents, stdout and stderr of the reference CLI's
`main create-sparse-index <file.vcfc>`, `main query-sparse-index <file.vcfc>
<region>` and `main gap-analysis <file.vcfc>` (oracle/_ref/main, compiled from
the reference's sources by oracle/Makefile).  An index is recorded as its
apparent size and the (offset, 13 bytes) of its non-zero slots, read through
SEEK_DATA / SEEK_HOLE.  Run where the reference build exists, on a file
system with sparse files; writes sparse_index_cases.json (data only).

--edge: instead, the three actions (and make_binned_index_golden.edge_cases)
over the hand-built edge files of tests/index_edge_cases.py whose records all
hold their TABs, recorded as lengths, digests and exit codes with the digest
of each input file into index_edge_cases.json (data only)."""
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
sys.path.insert(0, HERE)
import golden_io as G                    # noqa: E402
import index_cases as X                  # noqa: E402
import sparse_index_cases as SX          # noqa: E402
import make_binned_index_golden as MB    # noqa: E402

HDR = X.header(3)


def run(args, cwd):
    r = subprocess.run([REF_MAIN] + args, cwd=cwd, capture_output=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def rows(spec, seed):
    """Data lines from (CHROM, POS) pairs, SNVs with three samples."""
    rnd = random.Random(seed)
    return b"".join(MB.row(c, p, k, b"A", b"G", b"AC=%d" % (1 + k % 4), rnd) for k, (c, p) in enumerate(spec))


def vcfs():
    out = {"index_edge": MB.index_edge_vcf()}
    out.update({k: v for k, v in MB.throw_vcfs().items() if k != "throw_base"})
    # shared POS values across chromosomes: `2 100` takes over the slot of `1 100`; `1 200` twice
    out["multi_chrom"] = HDR + rows([(b"1", 100), (b"1", 150), (b"1", 200), (b"1", 200), (b"1", 300), (b"2", 100),
                                     (b"2", 250), (b"22", 500), (b"22", 700), (b"X", 600), (b"X", 900), (b"Y", 50)], 11)
    out["unsorted"] = HDR + rows([(b"1", 500), (b"1", 100), (b"1", 300), (b"1", 100), (b"1", 700)], 12)
    # POS >= 2^32: the entry's u32 position is truncated, the offset is not
    out["pos_2_32"] = HDR + rows([(b"1", 100), (b"1", (1 << 32) + 5), (b"1", (1 << 32) + 9)], 13)
    # (300000000 + 2^55) * 256 >= 2^63: negative as off_t, lseek fails on every file system
    out["seek_fails"] = HDR + rows([(b"1", 100), (b"1", 200), (b"1", 1 << 55), (b"1", 300)], 14)
    return out


QUERIES = {
    "random_100x10000.vcfc.gz": ["1:10100-10104", "1:10101-10101", "1:10100-10100", "1:5-9999", "1:5-10010",
                                 "1:30000-40000", "foo:1-9", "2:1-100", "1:10200-10100", "1", "1:29990-30010",
                                 "X:1-10", "1:20001-20001", "1:19999-20405"],
    "index_edge": ["1:100-200", "1:1-50", "1:300-100", "1", "1:150-100000", "2:100-150", "2:120-4000",
                   "chrZ:1-100000", "foo:1-9", "foo:200-300", "X:100-400", "X:100000-200000", "3:1-1000", "1:600-2700",
                   "2:580-640", "X:560-561"],
    "multi_chrom": ["1:100-100", "1:150-150", "1:120-400", "1:200-200", "2:100-100", "2:100-250", "X:1-1000",
                    "22:500-500", "22:1-1000", "Y:50-50", "Y:1-60", "foo:100-100", "1", "1:300-100", "1:1-50",
                    "1:1000-2000", "1:800-850", "1:901-950"],
    "unsorted": ["1:100-400", "1:300-800", "1:500-500", "1:100-100", "1:1-1000", "1:600-650"],
    "pos_2_32": ["1:100-100", "1:4294967301-4294967301", "1:4294967300-4294967400", "1:5-5", "1:101-4294967305"],
    "seek_fails": ["1:100-300", "1:200-200", "1:300-300", "1:36028797018963968-36028797018963968"],
    "throw_pos": ["1:100-1000", "1:305-400", "1:100-150"],
    "throw_kvp": ["1:100-1000", "1:305-400", "1:100-150", "1:200-200"],
    "throw_end": ["1:100-1000", "1:190-310"],
    "header_only": ["1:100-200", "1"],
}


def main():
    if not os.path.exists(REF_MAIN):
        sys.exit("build the reference first: make -C oracle")
    files = {"random_100x10000.vcfc.gz": G.gz("random_100x10000.vcfc.gz")}
    create_cases, query_cases, gap_cases, cli_cases = [], [], [], []
    with tempfile.TemporaryDirectory(dir=os.environ.get("SPARSE_GOLDEN_TMP")) as wd:
        for name, vcf in vcfs().items():
            src = os.path.join(wd, name + ".vcf")
            with open(src, "wb") as f:
                f.write(vcf)
            rc, _, _ = run(["compress", src, src + "c"], wd)
            assert rc == 0, (name, rc)
            files[name] = open(src + "c", "rb").read()
        files["header_only"] = HDR
        path = os.path.join(wd, "f.vcfc")
        index = path + ".vcfci-sparse"
        for name, data in files.items():
            with open(path, "wb") as f:
                f.write(data)
            if os.path.exists(index):
                os.unlink(index)
            rc, out, err = run(["create-sparse-index", path], wd)
            slots, size = SX.read_sparse_file(index)
            c = {"file": name, "rc": rc, "stdout": out.decode(), "size": size, "n_slots": len(slots),
                 "slots_sha256": SX.slots_digest(slots)}
            if rc == 0:
                c["stderr"] = err.decode()
            if len(slots) <= 200:
                c["slots"] = [[o, slots[o].hex()] for o in sorted(slots)]
            create_cases.append(c)
            for region in QUERIES[name]:
                rc, out, err = run(["query-sparse-index", path, region], wd)
                q = {"file": name, "region": region, "rc": rc, "stdout_len": len(out),
                     "stdout_sha256": hashlib.sha256(out).hexdigest()}
                if rc == 0:
                    q["stderr"] = err.decode()
                query_cases.append(q)
            sp = os.path.join(wd, "start-positions.txt")
            if os.path.exists(sp):
                os.unlink(sp)
            rc, out, _ = run(["gap-analysis", path], wd)
            txt = open(sp, "rb").read() if os.path.exists(sp) else b""
            g = {"file": name, "rc": rc, "stdout": out.decode(), "txt_len": len(txt),
                 "txt_sha256": hashlib.sha256(txt).hexdigest()}
            if len(txt) <= 8192:
                g["txt"] = txt.decode()
            gap_cases.append(g)
        # argv checks and messages (src/main.cpp:4144-4178); {f}: a .vcfc with its index, {m}: a missing
        # file, {n}: a .vcfc without an index
        with open(path, "wb") as f:
            f.write(files["index_edge"])
        assert run(["create-sparse-index", path], wd)[0] == 0
        noidx = os.path.join(wd, "noidx.vcfc")
        with open(noidx, "wb") as f:
            f.write(files["index_edge"])
        sub = {"{f}": path, "{m}": os.path.join(wd, "missing.vcfc"), "{n}": noidx}
        for argv in (["create-sparse-index"], ["create-sparse-index", "{f}", "x"], ["create-sparse-index", "{m}"],
                     ["query-sparse-index"], ["query-sparse-index", "{f}"], ["query-sparse-index", "{f}", "1:1-2", "x"],
                     ["query-sparse-index", "{m}", "1:1-2"], ["query-sparse-index", "{n}", "1:1-2"],
                     ["query-sparse-index", "{f}", "1:5"], ["query-sparse-index", "{f}", "1:a-5"],
                     ["query-sparse-index", "{f}", "1:5-x"], ["gap-analysis", "{m}"]):
            rc, out, err = run([sub.get(a, a) for a in argv], wd)
            for k, v in sub.items():
                out, err = out.replace(v.encode(), k.encode()), err.replace(v.encode(), k.encode())
            c = {"argv": argv, "rc": rc, "stdout": out.decode()}
            if rc == 0:
                c["stderr"] = err.decode()
            cli_cases.append(c)
    inline = {k: v.hex() for k, v in files.items() if not k.endswith(".gz")}
    with open(os.path.join(HERE, "sparse_index_cases.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_sparse_index_golden.py (reference: oracle/_ref/main)",
                   "inline_files": inline, "create_cases": create_cases, "query_cases": query_cases,
                   "gap_cases": gap_cases, "cli_cases": cli_cases}, f, indent=1)
    print(len(create_cases), "create cases,", len(query_cases), "query cases,", len(gap_cases), "gap cases,",
          len(cli_cases), "cli cases")
    for c in create_cases:
        print(c["file"], c["rc"], c["size"], c["n_slots"])
    for q in query_cases:
        print(q["file"], q["region"], q["rc"], q["stdout_len"], repr(q.get("stderr", ""))[:60])


def edge_main():
    import index_edge_cases as EC
    if not os.path.exists(REF_MAIN):
        sys.exit("build the reference first: make -C oracle")
    files = EC.pinned_files()
    create_cases, gap_cases, query_cases = [], [], []
    with tempfile.TemporaryDirectory(dir=os.environ.get("SPARSE_GOLDEN_TMP")) as wd:
        index_cases, binned_query_cases = MB.edge_cases(wd, files, EC.PINNED_BINNED_QUERIES)
        path = os.path.join(wd, "f.vcfc")
        index = path + ".vcfci-sparse"
        sp = os.path.join(wd, "start-positions.txt")
        for name, data in files.items():
            with open(path, "wb") as f:
                f.write(data)
            for p in (index, sp):
                if os.path.exists(p):
                    os.unlink(p)
            rc, out, err = run(["create-sparse-index", path], wd)
            slots, size = SX.read_sparse_file(index)
            create_cases.append({"file": name, "rc": rc, "size": size, "n_slots": len(slots),
                                 "slots_sha256": SX.slots_digest(slots), "seek_failed": int(b"lseek" in err)})
            for region in EC.PINNED_SPARSE_QUERIES.get(name, ()):
                rc, out, err = run(["query-sparse-index", path, region], wd)
                query_cases.append({"file": name, "region": region, "rc": rc, "stdout_len": len(out),
                                    "stdout_sha256": hashlib.sha256(out).hexdigest()})
            if name in EC.PINNED_NO_GAP:
                continue
            rc, out, _ = run(["gap-analysis", path], wd)
            txt = open(sp, "rb").read() if os.path.exists(sp) else b""
            gap_cases.append({"file": name, "rc": rc, "txt_len": len(txt), "txt_sha256": hashlib.sha256(txt).hexdigest()})
    meta = {k: {"len": len(v), "sha256": hashlib.sha256(v).hexdigest()} for k, v in files.items()}
    with open(os.path.join(HERE, "index_edge_cases.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_sparse_index_golden.py --edge (reference: oracle/_ref/main)",
                   "files": meta, "index_cases": index_cases, "binned_query_cases": binned_query_cases,
                   "create_cases": create_cases, "sparse_query_cases": query_cases, "gap_cases": gap_cases}, f,
                  separators=(",", ":"))
    print(len(files), "files,", len(index_cases), "index cases,", len(create_cases), "create cases,", len(gap_cases),
          "gap cases,", len(binned_query_cases) + len(query_cases), "query cases")


if __name__ == "__main__":
    edge_main() if "--edge" in sys.argv[1:] else main()
