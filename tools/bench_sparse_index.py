#!/usr/bin/env python3
"""Measurements of the sparse external index (report only; DESIGN.md cites the
lines, raw copies go under profiles/sparse_index/).

  1. device: vcfc_sparse_index_device over the headline batch (2504 samples x
     1M chr22-shaped rows, encoded in HBM), timed with HIP events and
     alternating, in one process, with the two yardsticks on the same records:
     vcfc_binned_index_device (E = 1000) and vcfc_query_match_device;
  2. host files (2504 x --file-rows, written to --dir): create_sparse_index
     against the reference CLI's create-sparse-index (oracle/_ref/main, when
     built) with the index contents compared, the 4 KiB blocks written (one
     pwrite each; the traced count goes to stderr), and
     one indexed query of ~1 % of the file against query_file's full scan and
     query_binned_index_file.

One JSON line per measurement on stdout."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_index import encode, stats   # noqa: E402


def device_part(args, torch, vcfc, workload, dev):
    n, S = args.rows, args.samples
    rows, recs, rec, rec_bytes = encode(torch, vcfc, workload, n, S, dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    swsb, iwsb = vcfc.sparse_index_workspace_size(n), vcfc.index_workspace_size(n)
    sws = torch.empty(swsb, dtype=torch.uint8, device=dev)
    iws = torch.empty(iwsb, dtype=torch.uint8, device=dev)
    ent = torch.empty(13 * n + 16, dtype=torch.uint8, device=dev)
    fo = torch.empty(n + 2, dtype=torch.int64, device=dev)
    words = torch.empty(4, dtype=torch.int64, device=dev)
    err = torch.empty(1, dtype=torch.int64, device=dev)
    flag = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    ref = rows.chrom.encode()
    d_ref = torch.tensor(list(ref), dtype=torch.uint8, device=dev)
    qs, qe = int(rows.pos[n // 2]), int(rows.pos[n // 2 + n // 100])

    def sparse():
        vcfc.sparse_index_device(recs.data_ptr(), rec.data_ptr(), n, 0, ent.data_ptr(), fo.data_ptr(), words.data_ptr(),
                                 words.data_ptr() + 8, sws.data_ptr(), swsb, err.data_ptr(), s)

    def binned():
        vcfc.binned_index_device(recs.data_ptr(), rec.data_ptr(), n, 0, 1000, ent.data_ptr(), n, words.data_ptr(),
                                 words.data_ptr() + 8, iws.data_ptr(), iwsb, err.data_ptr(), s)

    def match():
        vcfc.raise_for(vcfc.query_match_device(recs.data_ptr(), rec.data_ptr(), n, d_ref.data_ptr(), len(ref), True,
                                               qs, qe, flag.data_ptr(), err.data_ptr(), s))

    runs = [("sparse", sparse), ("binned", binned), ("match", match)]
    times = {k: [] for k, _ in runs}
    for it in range(args.warmup + args.reps):
        for k, f in runs:   # alternating in one process
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            if it >= args.warmup:
                times[k].append(a.elapsed_time(b))
    sparse()
    torch.cuda.synchronize(dev)
    assert int(err.item()) == -1
    w = words.cpu().tolist()
    m, bi = statistics.median(times["match"]), statistics.median(times["binned"])
    r = stats(times["sparse"])
    r.update({"what": "vcfc_sparse_index_device", "records": n, "samples": S, "record_bytes": rec_bytes,
              "kept_entries": w[0], "out_of_order": w[2], "ratio_to_query_match": round(r["median_ms"] / m, 3),
              "ratio_to_binned_index": round(r["median_ms"] / bi, 3)})
    print(json.dumps(r), flush=True)
    r = stats(times["binned"])
    r.update({"what": "vcfc_binned_index_device (yardstick, E = 1000)", "records": n, "samples": S})
    print(json.dumps(r), flush=True)
    r = stats(times["match"])
    r.update({"what": "vcfc_query_match_device (yardstick)", "records": n, "samples": S})
    print(json.dumps(r), flush=True)


def index_digest(path):
    """(sha256 over (offset, 13 bytes) of the non-zero slots, their count, the
    4 KiB blocks that hold them, the apparent size)."""
    d = hashlib.sha256()
    fd = os.open(path, os.O_RDONLY)
    n = blocks = 0
    try:
        size = os.fstat(fd).st_size
        p = 0
        while p < size:
            try:
                a = os.lseek(fd, p, os.SEEK_DATA)
            except OSError:
                break
            b = os.lseek(fd, a, os.SEEK_HOLE)
            a -= a % 4096
            data = os.pread(fd, b - a, a)
            for blk in range(0, len(data), 4096):
                hit = False
                for o in range(blk, min(blk + 4096, len(data)), 256):
                    e = data[o:o + 13]
                    if e.strip(b"\0"):
                        d.update((a + o).to_bytes(8, "little") + e)
                        n += 1
                        hit = True
                blocks += hit
            p = b
    finally:
        os.close(fd)
    return d.hexdigest(), n, blocks, size


def file_part(args, torch, vcfc, workload, dev):
    n, S = args.file_rows, args.samples
    rows, recs, rec, rec_bytes = encode(torch, vcfc, workload, n, S, dev)
    hdr = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + \
        b"".join(b"\tS%d" % i for i in range(S)) + b"\n"
    with tempfile.TemporaryDirectory(dir=args.dir) as wd:
        path = os.path.join(wd, "b.vcfc")
        with open(path, "wb") as f:
            f.write(hdr)
            f.write(recs[:rec_bytes].cpu().numpy().tobytes())
        size = os.path.getsize(path)
        index = path + ".vcfci-sparse"
        with vcfc.Context(0) as ctx:
            ctx.set_trace(vcfc.TRACE_INDEX)   # the pwrite count goes to stderr
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                seek_failed = ctx.create_sparse_index(path)
                ts.append(time.perf_counter() - t0)
            ctx.set_trace(0)
            ours = index_digest(index)
            print(json.dumps({"what": "create_sparse_index", "file_bytes": size, "records": n,
                              "wall_s": [round(t, 4) for t in ts], "entries": ours[1], "blocks_4k": ours[2],
                              "index_apparent_bytes": ours[3], "seek_failed": seek_failed}), flush=True)
            ref_main = os.path.join(REPO, "oracle", "_ref", "main")
            if os.path.exists(ref_main):
                t0 = time.perf_counter()
                rc = subprocess.run([ref_main, "create-sparse-index", path], stdout=subprocess.DEVNULL).returncode
                t = time.perf_counter() - t0
                theirs = index_digest(index)
                print(json.dumps({"what": "reference CLI create-sparse-index", "rc": rc, "wall_s": round(t, 4),
                                  "entry_writes": n, "index_identical": theirs == ours}), flush=True)
            else:
                print(json.dumps({"what": "reference CLI create-sparse-index", "skipped": "oracle/_ref/main not built"}))
            ctx.create_binned_index_file(path, args.bin)
            a = n // 2
            q = "%s:%d-%d" % (rows.chrom, int(rows.pos[a]), int(rows.pos[a + max(1, n // 100) - 1]))
            null = os.open(os.devnull, os.O_WRONLY)
            for name, f in (("query_sparse_index", lambda: ctx.query_sparse_index(path, q, null)),
                            ("query_binned_index_file", lambda: ctx.query_binned_index_file(path, q, null)),
                            ("query_file (full scan)", lambda: ctx.query_file(path, q, null))):
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    f()
                    ts.append(time.perf_counter() - t0)
                print(json.dumps({"what": name, "region": q, "file_bytes": size,
                                  "wall_s": [round(t, 4) for t in ts]}), flush=True)
            os.close(null)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--file-rows", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--bin", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dir", default=None, help="where the host files are written (default: the temp dir)")
    ap.add_argument("--skip-files", action="store_true")
    ap.add_argument("--skip-device", action="store_true")
    args = ap.parse_args()
    import torch   # before libvcfc: one HIP runtime in the process
    import vcfc
    import workload
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if not args.skip_device:
        device_part(args, torch, vcfc, workload, dev)
        torch.cuda.empty_cache()
    if not args.skip_files:
        file_part(args, torch, vcfc, workload, dev)


if __name__ == "__main__":
    main()
