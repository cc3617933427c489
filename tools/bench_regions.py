#!/usr/bin/env python3
"""Measurements of the region-list match (report only; DESIGN.md §4k cites the
lines, raw copies go under profiles/regions/).

Over the headline batch (2504 samples x 1M chr22-shaped rows, encoded in HBM),
timed with HIP events, alternating, in one process:

  vcfc_regions_match_device for R = 1, 1 000 and 200 000 disjoint intervals
  over the middle --query-frac of the rows (R = 1 is bench.py --mode query's
  window; the larger tables split that window evenly, with gaps), each next to
  vcfc_query_match_device on the same records;

  the whole step, match + vcfc_decode_selected_device, for each R, next to the
  single-region step; for R = 1 000 also what the same answer costs today:
  R single-region steps, computed.

Every timed call follows an untimed vcfc_query_match_device on the same
records, so all of them start from the same cache state: without it the run
that follows a decode reads the records cold and the one after it warm, and
the order of the runs decides the ratio.

Before timing the flags are checked on the device: R = 1 must equal
vcfc_query_match_device's flags, the split tables' flags must be a subset of
them with the count a host search of the rows' POS expects.  One JSON line per
measurement on stdout."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_index import encode, stats  # noqa: E402


def split_window(qs, qe, R):
    """R disjoint intervals splitting [qs, qe] evenly, a gap after each
    (a quarter of its share, one position at least)."""
    if R == 1:
        return [(qs, qe)]
    span = qe - qs + 1
    out = []
    for g in range(R):
        lo, hi = qs + g * span // R, qs + (g + 1) * span // R - 1
        out.append((lo, hi - max(1, (hi - lo + 1) // 4)))
    assert all(a <= b for a, b in out), "the window is too narrow for %d intervals" % R
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--query-frac", type=float, default=0.125)
    ap.add_argument("--regions", default="1,1000,200000", help="comma-separated interval counts")
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
    dwsb = vcfc.decode_workspace_size(n)
    dws = torch.empty(dwsb, dtype=torch.uint8, device=dev)
    out_cap = rows.total_bytes + 64
    out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    loff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    derr = torch.empty(1, dtype=torch.int64, device=dev)
    merr = torch.empty(1, dtype=torch.int64, device=dev)
    flag = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    flag1 = torch.empty(n + 64, dtype=torch.uint8, device=dev)
    ref = rows.chrom.encode()
    d_ref = torch.tensor(list(ref), dtype=torch.uint8, device=dev)
    a = int(n * (0.5 - args.query_frac / 2))
    b = min(n - 1, a + max(1, int(n * args.query_frac)) - 1)
    qs, qe = int(rows.pos[a]), int(rows.pos[b])
    pos = np.asarray(rows.pos, dtype=np.int64)

    def noerr(e):
        return int(e.cpu().numpy().view(np.uint64)[0]) == vcfc.NO_ERROR

    def match1(f=flag):
        vcfc.raise_for(vcfc.query_match_device(recs.data_ptr(), rec.data_ptr(), n, d_ref.data_ptr(), len(ref), True, qs, qe,
                                               f.data_ptr(), merr.data_ptr(), s))

    def decode():
        vcfc.decode_selected_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), flag.data_ptr(), n, S, out.data_ptr(),
                                    out_cap, loff.data_ptr(), dws.data_ptr(), dwsb, derr.data_ptr(), s)

    tables = {}
    for R in [int(x) for x in args.regions.split(",")]:
        iv = split_window(qs, qe, R)
        table = vcfc.regions_build("".join("%s:%d-%d\n" % (rows.chrom, lo, hi) for lo, hi in iv))
        wsb = vcfc.regions_workspace_size(len(table))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        vcfc.raise_for(vcfc.regions_upload(table, ws.data_ptr(), wsb, s))
        st = np.array([x[0] for x in iv], dtype=np.int64)
        en = np.array([x[1] for x in iv], dtype=np.int64)
        k = np.searchsorted(st, pos, side="right") - 1
        want = int(((k >= 0) & (pos <= en[np.maximum(k, 0)])).sum())
        tables[R] = (ws, wsb, len(table), want)

    def matchR(R):
        ws, wsb = tables[R][:2]
        vcfc.raise_for(vcfc.regions_match_device(recs.data_ptr(), rec.data_ptr(), n, ws.data_ptr(), wsb, flag.data_ptr(),
                                                 merr.data_ptr(), s))

    # the flags, checked on the device
    match1(flag1)
    torch.cuda.synchronize(dev)
    assert noerr(merr)
    sel1 = int(flag1[:n].sum().item())
    for R, (ws, wsb, tb, want) in tables.items():
        matchR(R)
        torch.cuda.synchronize(dev)
        got = int(flag[:n].sum().item())
        subset = bool(((flag[:n] & ~flag1[:n]) == 0).all().item())
        same = bool(torch.equal(flag[:n], flag1[:n]))
        ok = noerr(merr) and subset and got == want and (R != 1 or same)
        print(json.dumps({"what": "check: flags of R=%d" % R, "ok": ok, "selected": got, "expected": want,
                          "single_region_selected": sel1, "subset_of_single_region": subset, "table_bytes": tb,
                          "records": n, "samples": S}), flush=True)
        assert ok

    runs = [("query_match", match1)]
    for R in tables:
        runs.append(("regions_match_R%d" % R, lambda R=R: matchR(R)))
    runs.append(("query_step", lambda: (match1(), decode())))
    for R in tables:
        runs.append(("regions_step_R%d" % R, lambda R=R: (matchR(R), decode())))
    times = {k: [] for k, _ in runs}
    for it in range(args.warmup + args.reps):
        for k, f in runs:   # alternating in one process
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            match1(flag1)   # untimed: every run starts from the cache state a match of these records leaves
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if it >= args.warmup:
                times[k].append(e0.elapsed_time(e1))
            if it == 0:
                assert noerr(merr) and ("step" not in k or noerr(derr)), k
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, _ in runs:
        r = stats(times[k])
        r.update({"what": k, "records": n, "samples": S, "record_bytes": rec_bytes,
                  "window": "%s:%d-%d" % (rows.chrom, qs, qe)})
        if "_R" in k:
            R = int(k.rsplit("_R", 1)[1])
            r.update({"regions": R, "table_bytes": tables[R][2], "selected_records": tables[R][3]})
        yard = "query_match" if k.endswith(tuple("match_R%d" % R for R in tables)) else "query_step"
        if k not in ("query_match", "query_step"):
            r["ratio_to_" + yard] = round(r["median_ms"] / med[yard], 3)
        if k == "regions_step_R1000":
            r["R_single_region_steps_ms_computed"] = round(1000 * med["query_step"], 2)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
