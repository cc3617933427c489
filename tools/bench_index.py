#!/usr/bin/env python3
"""Measurements of the binned external index (report only; DESIGN.md cites the
lines, raw copies go under profiles/).

  1. device: vcfc_binned_index_device at E = 1 and E = 1000 over the headline
     batch (2504 samples x 1M chr22-shaped rows, encoded in HBM), timed with
     HIP events and alternating, in one process, with vcfc_query_match_device
     on the same records (the yardstick: one lane per record over the same
     record prefixes);
  2. host files (2504 x --file-rows, written to --dir): create_binned_index_file
     against the reference CLI's create-binned-index (oracle/_ref/main, when
     built), and one indexed query of ~1 % of the file against query_file.

One JSON line per measurement on stdout."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))


def encode(torch, vcfc, workload, n, S, dev):
    rows = workload.DeviceRows(torch, vcfc, n, S, 1, seed=1000, device=dev)
    cap = vcfc.encode_bound(n, rows.line_bytes)
    wsb = vcfc.workspace_size(n, rows.line_bytes)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    rec = torch.empty(n + 1, dtype=torch.int64, device=dev)
    err = torch.empty(1, dtype=torch.int64, device=dev)
    vcfc.encode_rows_device(rows.buf.data_ptr(), rows.line_off.data_ptr(), rows.line_len.data_ptr(), n, rows.line_bytes,
                            out.data_ptr(), cap, rec.data_ptr(), ws.data_ptr(), wsb, err.data_ptr(),
                            torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert int(err.item()) == -1
    del ws
    return rows, out, rec, int(rec[n].item())


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def device_part(args, torch, vcfc, workload, dev):
    n, S = args.rows, args.samples
    rows, recs, rec, rec_bytes = encode(torch, vcfc, workload, n, S, dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    iwsb = vcfc.index_workspace_size(n)
    iws = torch.empty(iwsb, dtype=torch.uint8, device=dev)
    ent = torch.empty(13 * n + 16, dtype=torch.uint8, device=dev)
    words = torch.empty(2, dtype=torch.int64, device=dev)
    err = torch.empty(1, dtype=torch.int64, device=dev)
    flag = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    ref = rows.chrom.encode()
    d_ref = torch.tensor(list(ref), dtype=torch.uint8, device=dev)
    qs, qe = int(rows.pos[n // 2]), int(rows.pos[n // 2 + n // 100])

    def index(E):
        vcfc.binned_index_device(recs.data_ptr(), rec.data_ptr(), n, 0, E, ent.data_ptr(), n, words.data_ptr(),
                                 words.data_ptr() + 8, iws.data_ptr(), iwsb, err.data_ptr(), s)

    def match():
        vcfc.raise_for(vcfc.query_match_device(recs.data_ptr(), rec.data_ptr(), n, d_ref.data_ptr(), len(ref), True,
                                               qs, qe, flag.data_ptr(), err.data_ptr(), s))

    runs = [("index_E1", lambda: index(1)), ("match_a", match), ("index_E1000", lambda: index(1000)),
            ("match_b", match)]
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
    count = {}
    for E in (1, 1000):
        index(E)
        torch.cuda.synchronize(dev)
        assert int(err.item()) == -1
        count[E] = int(words[0].item())
    m = statistics.median(times["match_a"] + times["match_b"])
    for k, E in (("index_E1", 1), ("index_E1000", 1000)):
        r = stats(times[k])
        r.update({"what": "vcfc_binned_index_device", "entries_per_bin": E, "records": n, "samples": S,
                  "record_bytes": rec_bytes, "entries": count[E],
                  "ratio_to_query_match": round(r["median_ms"] / m, 3)})
        print(json.dumps(r), flush=True)
    r = stats(times["match_a"] + times["match_b"])
    r.update({"what": "vcfc_query_match_device (yardstick, unchanged kernel)", "records": n, "samples": S})
    print(json.dumps(r), flush=True)


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
        with vcfc.Context(0) as ctx:
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                ctx.create_binned_index_file(path, args.bin)
                ts.append(time.perf_counter() - t0)
            ours = open(path + ".vcfci", "rb").read()
            print(json.dumps({"what": "create_binned_index_file", "file_bytes": size, "records": n, "bin": args.bin,
                              "wall_s": [round(t, 4) for t in ts], "index_bytes": len(ours)}), flush=True)
            ref_main = os.path.join(REPO, "oracle", "_ref", "main")
            if os.path.exists(ref_main):
                t0 = time.perf_counter()
                rc = subprocess.run([ref_main, "create-binned-index", str(args.bin), path],
                                    stdout=subprocess.DEVNULL).returncode
                t = time.perf_counter() - t0
                same = open(path + ".vcfci", "rb").read() == ours
                print(json.dumps({"what": "reference CLI create-binned-index", "rc": rc, "wall_s": round(t, 4),
                                  "index_identical": same}), flush=True)
            else:
                print(json.dumps({"what": "reference CLI create-binned-index", "skipped": "oracle/_ref/main not built"}))
            a = n // 2
            q = "%s:%d-%d" % (rows.chrom, int(rows.pos[a]), int(rows.pos[a + max(1, n // 100) - 1]))
            null = os.open(os.devnull, os.O_WRONLY)
            for name, f in (("query_binned_index_file", lambda: ctx.query_binned_index_file(path, q, null)),
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
    args = ap.parse_args()
    import torch   # before libvcfc: one HIP runtime in the process
    import vcfc
    import workload
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    device_part(args, torch, vcfc, workload, dev)
    torch.cuda.empty_cache()
    if not args.skip_files:
        file_part(args, torch, vcfc, workload, dev)


if __name__ == "__main__":
    main()
