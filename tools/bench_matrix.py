#!/usr/bin/env python3
"""Measurements of genotype-matrix (report only; DESIGN.md §4l cites the
lines, raw copies go under profiles/matrix/).

Over the headline batch (2504 samples x 1M chr22-shaped rows, encoded in HBM),
timed with HIP events, alternating, in one process:

  vcfc_genotype_matrix_device for each layout (dosage, hap, bed), and dosage
  for the middle --query-frac of the rows through d_select (match + matrix),
  against yardsticks measured in the same run: a device fill of each layout's
  output bytes (the write floor), a device copy of the record bytes (the read
  floor), vcfc_decode_records_device (what one pays today before one can
  parse and pack) and genotype-counts rows-only (the same scan, no rows out).

Before timing, the three matrices are checked against the source rows, token
by token, with torch on the device (the tokens that are one of 0|0 0|1 1|0
1|1; .bed on the rows that hold no other token).  One JSON line per
measurement on stdout; every matrix line carries its ratios to the yardsticks."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_index import encode, stats  # noqa: E402

NAMES = ("dosage", "hap", "bed")


def check(torch, rows, n, S, mats, chunk=8192):
    """The three matrices against the source rows (fixed-width 3-byte tokens)."""
    dev = rows.buf.device
    ar = torch.arange(S, device=dev, dtype=torch.int64) * 4
    S4 = (S + 3) // 4 * 4
    w = torch.tensor([1, 4, 16, 64], dtype=torch.int64, device=dev)
    ok, classed, plain_rows = True, 0, 0
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        ends = (rows.line_off[i0:i1] + rows.line_len[i0:i1].to(torch.int64)).unsqueeze(1)
        base = ends + 1 - 4 * S + ar.unsqueeze(0)
        x, bar, y = rows.buf[base].to(torch.int64) - 48, rows.buf[base + 1], rows.buf[base + 2].to(torch.int64) - 48
        m = (bar == 124) & (x >= 0) & (x < 2) & (y >= 0) & (y < 2)
        classed += int(m.sum().item())
        ok &= bool(torch.equal(mats[0][i0:i1].to(torch.int64)[m], (x + y)[m]))
        hap = mats[1][i0:i1].to(torch.int64).view(i1 - i0, S, 2)
        ok &= bool(torch.equal(hap[:, :, 0][m], x[m])) and bool(torch.equal(hap[:, :, 1][m], y[m]))
        code = torch.zeros((i1 - i0, S4), dtype=torch.int64, device=dev)
        code[:, :S] = torch.where(x + y == 0, 3, torch.where(x + y == 1, 2, 0))
        packed = (code.view(i1 - i0, S4 // 4, 4) * w).sum(2)
        full = m.all(1)
        plain_rows += int(full.sum().item())
        ok &= bool(torch.equal(mats[2][i0:i1].to(torch.int64)[full], packed[full]))
    return ok, classed, plain_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--query-frac", type=float, default=0.125)
    ap.add_argument("--only", default=None, help="comma-separated run names (for a profiler run)")
    ap.add_argument("--no-check", action="store_true", help="skip the check against the source rows")
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
    rb = [vcfc.matrix_row_bytes(k, S) for k in range(3)]
    mats = [torch.empty((n, rb[0]), dtype=torch.int8, device=dev), torch.empty((n, rb[1]), dtype=torch.int8, device=dev),
            torch.empty((n, rb[2]), dtype=torch.uint8, device=dev)]
    row_of = torch.empty(n + 1, dtype=torch.int64, device=dev)
    mwsb = vcfc.matrix_workspace_size(n, S, 0)
    mws = torch.empty(mwsb, dtype=torch.uint8, device=dev)
    cwsb = vcfc.counts_workspace_size(n, S)
    cws = torch.empty(cwsb, dtype=torch.uint8, device=dev)
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
    ref = rows.chrom.encode()
    d_ref = torch.tensor(list(ref), dtype=torch.uint8, device=dev)
    a = int(n * (0.5 - args.query_frac / 2))
    b = min(n - 1, a + max(1, int(n * args.query_frac)) - 1)
    qs, qe = int(rows.pos[a]), int(rows.pos[b])

    def noerr(e):
        return int(e.cpu().numpy().view(np.uint64)[0]) == vcfc.NO_ERROR

    def matrix(k, sel=None):
        vcfc.raise_for(vcfc.genotype_matrix_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), sel, n, S, k, mats[k].data_ptr(),
                                                   n * rb[k], rb[k], row_of.data_ptr(), mws.data_ptr(), mwsb, err.data_ptr(), s))

    def counts():
        vcfc.raise_for(vcfc.genotype_counts_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), None, n, S, variant.data_ptr(),
                                                   None, cws.data_ptr(), cwsb, err.data_ptr(), s))

    def full():
        vcfc.decode_records_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), n, S, out.data_ptr(), out_cap,
                                   loff.data_ptr(), dws.data_ptr(), dwsb, err.data_ptr(), s)

    def query_dosage():
        vcfc.raise_for(vcfc.query_match_device(recs.data_ptr(), rec.data_ptr(), n, d_ref.data_ptr(), len(ref), True,
                                               qs, qe, flag.data_ptr(), merr.data_ptr(), s))
        matrix(0, flag.data_ptr())

    if not args.no_check:
        for k in range(3):
            matrix(k)
            torch.cuda.synchronize(dev)
            assert noerr(err), NAMES[k]
        ok, classed, plain_rows = check(torch, rows, n, S, mats)
        print(json.dumps({"what": "check: the three matrices == the source rows' tokens", "identical": ok, "records": n,
                          "samples": S, "record_bytes": rec_bytes, "line_bytes": rows.total_bytes, "class_tokens": classed,
                          "rows_of_class_tokens_only": plain_rows, "row_bytes": rb}), flush=True)
        assert ok

    runs = [("matrix_" + NAMES[k], (lambda k=k: matrix(k))) for k in range(3)]
    runs += [("fill_" + NAMES[k], (lambda k=k: mats[k].fill_(1))) for k in range(3)]
    runs += [("copy_records", lambda: copy_dst.copy_(recs[:rec_bytes])), ("full_decode", full), ("counts_variant", counts),
             ("query_matrix_dosage", query_dosage)]
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
            if it == 0 and not k.startswith(("copy", "fill")):
                assert noerr(err), k
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, _ in runs:
        r = stats(times[k])
        r.update({"what": k, "records": n, "samples": S, "record_bytes": rec_bytes})
        if k.startswith(("matrix", "fill")):
            r["out_bytes"] = n * rb[NAMES.index(k.split("_")[1])]
        if k.startswith("query"):
            r["region"] = "%s:%d-%d" % (rows.chrom, qs, qe)
            r["selected_records"] = b - a + 1
        if k.startswith(("matrix", "query")):
            ys = ["copy_records", "full_decode", "counts_variant"] + (["fill_" + k.split("_")[1]] if k.startswith("matrix") else [])
            for y in ys:
                if y in med:
                    r["ratio_to_" + y] = round(r["median_ms"] / med[y], 3)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
