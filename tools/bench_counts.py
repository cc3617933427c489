#!/usr/bin/env python3
"""Measurements of genotype-counts (report only; DESIGN.md §4j cites the
lines, raw copies go under profiles/counts/).

Over the headline batch (2504 samples x 1M chr22-shaped rows, encoded in HBM),
timed with HIP events, alternating, in one process:

  vcfc_genotype_counts_device for the rows only, the sample table only and
  both, against three yardsticks measured in the same run: a device copy of
  the record bytes (the read floor), vcfc_decode_records_device (what one pays
  today before one can count at all) and vcfc_decode_samples_device at K = 1
  (the same scan made twice: an exact sizing pass, then the write pass);

  a query line: the middle --query-frac of the rows (bench.py --mode query's
  window), match + both tables through d_select.

Before timing, the rows and the table are checked against a tally of the
source rows made with torch on the device.  One JSON line per measurement on
stdout; every counts line carries its ratios to the copy and the full decode."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_index import encode, stats  # noqa: E402


def tally(torch, rows, n, S, chunk=16384):
    """Class counters per row and per sample of the source rows (fixed-width
    3-byte tokens), on the device: class = 0..3 for 0|0 0|1 1|0 1|1, else 4."""
    dev = rows.buf.device
    per_row = torch.zeros((n, 5), dtype=torch.int64, device=dev)
    per_sample = torch.zeros((S, 5), dtype=torch.int64, device=dev)
    ar = torch.arange(S, device=dev, dtype=torch.int64) * 4
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        # a row's genotype region is its last 4 S bytes (3-byte tokens, TAB / LF)
        ends = (rows.line_off[i0:i1] + rows.line_len[i0:i1].to(torch.int64)).unsqueeze(1)
        base = ends + 1 - 4 * S + ar.unsqueeze(0)
        a, bar, b = rows.buf[base].to(torch.int64), rows.buf[base + 1], rows.buf[base + 2].to(torch.int64)
        x, y = a - 48, b - 48
        cls = torch.where((bar == 124) & (x >= 0) & (x < 2) & (y >= 0) & (y < 2), 2 * x + y, torch.full_like(x, 4))
        for k in range(5):
            m = cls == k
            per_row[i0:i1, k] = m.sum(1)
            per_sample[:, k] += m.sum(0)
    return per_row, per_sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--query-frac", type=float, default=0.125)
    ap.add_argument("--only", default=None, help="comma-separated run names (for a profiler run)")
    ap.add_argument("--no-check", action="store_true", help="skip the tally of the source rows")
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
    cwsb = vcfc.counts_workspace_size(n, S)
    cws = torch.empty(cwsb, dtype=torch.uint8, device=dev)
    swsb = vcfc.subset_workspace_size(n, 1)
    sws = torch.empty(swsb, dtype=torch.uint8, device=dev)
    dwsb = vcfc.decode_workspace_size(n)
    dws = torch.empty(dwsb, dtype=torch.uint8, device=dev)
    out_cap = rows.total_bytes + 64
    out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    loff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    err = torch.empty(1, dtype=torch.int64, device=dev)
    merr = torch.empty(1, dtype=torch.int64, device=dev)
    flag = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    copy_dst = torch.empty(rec_bytes, dtype=torch.uint8, device=dev)
    variant = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    table = torch.zeros((S, 5), dtype=torch.int64, device=dev)
    ref = rows.chrom.encode()
    d_ref = torch.tensor(list(ref), dtype=torch.uint8, device=dev)
    a = int(n * (0.5 - args.query_frac / 2))
    b = min(n - 1, a + max(1, int(n * args.query_frac)) - 1)
    qs, qe = int(rows.pos[a]), int(rows.pos[b])

    def noerr(e):
        return int(e.cpu().numpy().view(np.uint64)[0]) == vcfc.NO_ERROR

    def counts(v=True, t=True, sel=None):
        vcfc.raise_for(vcfc.genotype_counts_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), sel, n, S,
                                                   variant.data_ptr() if v else None, table.data_ptr() if t else None,
                                                   cws.data_ptr(), cwsb, err.data_ptr(), s))

    def subset1():
        vcfc.raise_for(vcfc.decode_samples_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), None, n, S, [S // 2],
                                                  out.data_ptr(), out_cap, loff.data_ptr(), sws.data_ptr(), swsb,
                                                  err.data_ptr(), s))

    def full():
        vcfc.decode_records_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), n, S, out.data_ptr(), out_cap,
                                   loff.data_ptr(), dws.data_ptr(), dwsb, err.data_ptr(), s)

    def match():
        vcfc.raise_for(vcfc.query_match_device(recs.data_ptr(), rec.data_ptr(), n, d_ref.data_ptr(), len(ref), True,
                                               qs, qe, flag.data_ptr(), merr.data_ptr(), s))

    def query_counts():
        match()
        counts(True, True, flag.data_ptr())

    if not args.no_check:
        counts()
        torch.cuda.synchronize(dev)
        per_row, per_sample = tally(torch, rows, n, S)
        ok = noerr(err) and bool(torch.equal(variant[:, :5].to(torch.int64), per_row)) and bool(torch.equal(table, per_sample))
        nonref = int(per_row[:, 1:].sum().item())
        print(json.dumps({"what": "check: rows and table == a tally of the source rows", "identical": ok, "records": n,
                          "samples": S, "record_bytes": rec_bytes, "line_bytes": rows.total_bytes,
                          "non_reference_tokens": nonref, "other_tokens": int(per_row[:, 4].sum().item())}), flush=True)
        assert ok

    runs = [("counts_variant", lambda: counts(True, False)), ("counts_sample", lambda: counts(False, True)),
            ("counts_both", lambda: counts(True, True)), ("copy_records", lambda: copy_dst.copy_(recs[:rec_bytes])),
            ("full_decode", full), ("subset_K1", subset1), ("query_counts_both", query_counts)]
    if args.only:
        runs = [r for r in runs if r[0] in args.only.split(",")]
    times = {k: [] for k, _ in runs}
    for it in range(args.warmup + args.reps):
        for k, f in runs:   # alternating in one process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if it >= args.warmup:
                times[k].append(e0.elapsed_time(e1))
            if it == 0 and k != "copy_records":
                assert noerr(err), k
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, _ in runs:
        r = stats(times[k])
        r.update({"what": k, "records": n, "samples": S, "record_bytes": rec_bytes})
        if k.startswith("query"):
            r["region"] = "%s:%d-%d" % (rows.chrom, qs, qe)
            r["selected_records"] = b - a + 1
        for y in ("copy_records", "full_decode", "subset_K1"):
            if y in med and k.startswith(("counts", "query")):
                r["ratio_to_" + y] = round(r["median_ms"] / med[y], 3)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
