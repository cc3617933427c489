#!/usr/bin/env python3
"""Measurements of the sample-subset decode (report only; DESIGN.md §4i cites
the lines, raw copies go under profiles/subset/).

Over the headline batch (2504 samples x 1M chr22-shaped rows, encoded in HBM),
timed with HIP events, alternating, in one process:

  vcfc_decode_samples_device for K = 1, 8, 64, 512 and 2504 random columns and
  for 64 contiguous columns, against three yardsticks: vcfc_decode_records_device
  on the same records (the full decode: what the subset replaces), a device
  copy of the record bytes (the read floor) and vcfc_query_match_device;

  a query line: the middle --query-frac of the rows (bench.py --mode query's
  window), match + subset decode with K = 8 against bench.py's own step (match
  + vcfc_decode_selected_device).

Before timing, the K = 2504 identity subset is checked against the source
rows byte for byte.  One JSON line per measurement on stdout."""
import argparse
import json
import os
import random
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_index import encode, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--query-frac", type=float, default=0.125)
    ap.add_argument("--only", default=None, help="comma-separated run names (for a profiler run)")
    args = ap.parse_args()
    import numpy as np
    import torch   # before libvcfc: one HIP runtime in the process
    import vcfc
    import workload
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, S = args.rows, args.samples
    rows, recs, rec, rec_bytes = encode(torch, vcfc, workload, n, S, dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    rnd = random.Random(7)
    colsets = {"K%d" % K: (rnd.sample(range(S), K) if K < S else list(range(S))) for K in (1, 8, 64, 512, S) if K <= S}
    if S >= 64:
        colsets["K64_contiguous"] = list(range(S // 2, S // 2 + 64))
    wsb = max(vcfc.subset_workspace_size(n, len(c)) for c in colsets.values())
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    dwsb = vcfc.decode_workspace_size(n)
    dws = torch.empty(dwsb, dtype=torch.uint8, device=dev)
    out_cap = rows.total_bytes + 64
    out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    loff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    err = torch.empty(1, dtype=torch.int64, device=dev)
    merr = torch.empty(1, dtype=torch.int64, device=dev)
    flag = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    copy_dst = torch.empty(rec_bytes, dtype=torch.uint8, device=dev)
    ref = rows.chrom.encode()
    d_ref = torch.tensor(list(ref), dtype=torch.uint8, device=dev)
    a = int(n * (0.5 - args.query_frac / 2))
    b = min(n - 1, a + max(1, int(n * args.query_frac)) - 1)
    qs, qe = int(rows.pos[a]), int(rows.pos[b])

    def noerr(e):
        return int(e.cpu().numpy().view(np.uint64)[0]) == vcfc.NO_ERROR

    def subset(cols, sel=None):
        vcfc.raise_for(vcfc.decode_samples_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), sel, n, S, cols,
                                                  out.data_ptr(), out_cap, loff.data_ptr(), ws.data_ptr(), wsb,
                                                  err.data_ptr(), s))

    def full():
        vcfc.decode_records_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), n, S, out.data_ptr(), out_cap,
                                   loff.data_ptr(), dws.data_ptr(), dwsb, err.data_ptr(), s)

    def match():
        vcfc.raise_for(vcfc.query_match_device(recs.data_ptr(), rec.data_ptr(), n, d_ref.data_ptr(), len(ref), True,
                                               qs, qe, flag.data_ptr(), merr.data_ptr(), s))

    def query_subset():
        match()
        subset(colsets.get("K8", [0]), flag.data_ptr())

    def query_full():
        match()
        vcfc.decode_selected_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), flag.data_ptr(), n, S, out.data_ptr(),
                                    out_cap, loff.data_ptr(), dws.data_ptr(), dwsb, err.data_ptr(), s)

    # the identity subset is the full decode: the source rows, byte for byte
    subset(list(range(S)))
    torch.cuda.synchronize(dev)
    ok = noerr(err) and int(loff[n].item()) == rows.total_bytes and \
        bool(torch.equal(out[:rows.total_bytes], rows.buf[:rows.total_bytes]))
    print(json.dumps({"what": "check: all columns == the source rows", "identical": ok, "records": n, "samples": S,
                      "record_bytes": rec_bytes, "line_bytes": rows.total_bytes}), flush=True)
    assert ok

    runs = [(k, (lambda c=c: subset(c))) for k, c in colsets.items()]
    runs += [("full_decode", full), ("copy_records", lambda: copy_dst.copy_(recs[:rec_bytes])), ("query_match", match),
             ("query_subset_K8", query_subset), ("query_full_decode", query_full)]
    if args.only:
        runs = [r for r in runs if r[0] in args.only.split(",")]
    times = {k: [] for k, _ in runs}
    outb = {}
    for it in range(args.warmup + args.reps):
        for k, f in runs:   # alternating in one process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if it >= args.warmup:
                times[k].append(e0.elapsed_time(e1))
            if it == 0 and k not in ("copy_records", "query_match"):
                assert noerr(err), k
                outb[k] = int(loff[n].item())
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, _ in runs:
        r = stats(times[k])
        r.update({"what": k, "records": n, "samples": S, "record_bytes": rec_bytes})
        if k in colsets:
            r["columns"] = len(colsets[k])
        if k in outb:
            r["output_bytes"] = outb[k]
        if k.startswith("query"):
            r["region"] = "%s:%d-%d" % (rows.chrom, qs, qe)
        for y in ("full_decode", "copy_records", "query_match"):
            if y in med and k in colsets:
                r["ratio_to_" + y] = round(r["median_ms"] / med[y], 3)
        if k == "query_subset_K8" and "query_full_decode" in med:
            r["ratio_to_query_full_decode"] = round(r["median_ms"] / med["query_full_decode"], 3)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
