#!/usr/bin/env python3
"""Measurements of extract (report only; DESIGN.md §4m cites the lines, raw
copies go under profiles/extract/).

Over the headline batch (2504 samples x 1M chr22-shaped rows, encoded in HBM),
timed with HIP events, alternating, in one process:

  vcfc_extract_samples_device for K = 1, 8, 64, 512 random columns, 64
  contiguous columns and all 2504, and for all columns of the middle
  --query-frac of the rows (match + extract), against three yardsticks at the
  same K: a device copy of the record bytes (the read floor),
  vcfc_decode_samples_device (the cut as text), and the through-text path a
  user takes without extract: vcfc_decode_samples_device, then
  vcfc_encode_rows_device on its lines.

Before timing, the K = 2504 and one random-K output are verified on the
device: their records, decoded by vcfc_decode_records_device, equal the subset
decode's lines by vcfc_record_hash_device digest; the all-columns output also
equals the input records byte for byte.  One JSON line per measurement on
stdout."""
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
    colsets = {"K%d" % K: (rnd.sample(range(S), K) if K < S else None) for K in (1, 8, 64, 512, S) if K <= S}
    if S >= 64:
        colsets["K64_contiguous"] = list(range(S // 2, S // 2 + 64))
    width = {k: (S if c is None else len(c)) for k, c in colsets.items()}
    xwsb = max(vcfc.extract_workspace_size(n, w) for w in width.values())
    xws = torch.empty(xwsb, dtype=torch.uint8, device=dev)
    swsb = max(vcfc.subset_workspace_size(n, w) for w in width.values())
    sws = torch.empty(swsb, dtype=torch.uint8, device=dev)
    dwsb = vcfc.decode_workspace_size(n)
    dws = torch.empty(dwsb, dtype=torch.uint8, device=dev)
    xcap = vcfc.extract_bound(rec_bytes, n, S)
    xout = torch.empty(xcap + 64, dtype=torch.uint8, device=dev)
    xoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    tcap = rows.total_bytes + 64
    text = torch.empty(tcap, dtype=torch.uint8, device=dev)
    loff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ewsb = vcfc.workspace_size(n, rows.line_bytes)
    ews = torch.empty(ewsb, dtype=torch.uint8, device=dev)
    ecap = vcfc.encode_bound(n, rows.line_bytes)
    eout = torch.empty(ecap, dtype=torch.uint8, device=dev)
    eoff = torch.empty(n + 1, dtype=torch.int64, device=dev)
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

    def cols_of(k):
        return list(range(S)) if colsets[k] is None else colsets[k]

    def extract(k, sel=None):
        vcfc.raise_for(vcfc.extract_samples_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), sel, n, S, colsets[k],
                                                   xout.data_ptr(), xcap, xoff.data_ptr(), xws.data_ptr(), xwsb,
                                                   err.data_ptr(), s))

    def subset(k):
        vcfc.raise_for(vcfc.decode_samples_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), None, n, S, cols_of(k),
                                                  text.data_ptr(), tcap, loff.data_ptr(), sws.data_ptr(), swsb,
                                                  err.data_ptr(), s))

    def through_text(k):
        subset(k)
        llen = (loff[1:] - loff[:-1] - 1).to(torch.int32)
        vcfc.encode_rows_device(text.data_ptr(), loff.data_ptr(), llen.data_ptr(), n, rows.line_bytes, eout.data_ptr(),
                                ecap, eoff.data_ptr(), ews.data_ptr(), ewsb, err.data_ptr(), s)

    def match():
        vcfc.raise_for(vcfc.query_match_device(recs.data_ptr(), rec.data_ptr(), n, d_ref.data_ptr(), len(ref), True,
                                               qs, qe, flag.data_ptr(), merr.data_ptr(), s))

    def region_extract():
        match()
        extract("K%d" % S, flag.data_ptr())

    # verification before timing
    def digests(buf, off):
        h = torch.empty(n, dtype=torch.int64, device=dev)
        vcfc.record_hash_device(buf.data_ptr(), off.data_ptr(), n, h.data_ptr(), s)
        return h

    for k in ("K%d" % S, "K64" if "K64" in colsets else "K1"):
        subset(k)
        want = digests(text, loff)
        torch.cuda.synchronize(dev)
        ok = noerr(err)
        extract(k)
        torch.cuda.synchronize(dev)
        ok = ok and noerr(err)
        xbytes = int(xoff[n].item())
        dec = torch.empty(int(loff[n].item()) + 64, dtype=torch.uint8, device=dev)
        doff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        vcfc.decode_records_device(xout.data_ptr(), xbytes, xoff.data_ptr(), n, width[k], dec.data_ptr(), dec.numel(),
                                   doff.data_ptr(), dws.data_ptr(), dwsb, err.data_ptr(), s)
        got = digests(dec, doff)
        torch.cuda.synchronize(dev)
        ok = ok and noerr(err) and bool(torch.equal(doff, loff)) and bool(torch.equal(got, want))
        if colsets[k] is None:   # all columns: the input records themselves
            ok = ok and xbytes == rec_bytes and bool(torch.equal(xout[:xbytes], recs[:rec_bytes]))
        through_text(k)
        torch.cuda.synchronize(dev)
        ebytes = int(eoff[n].item())
        same = ebytes == xbytes and bool(torch.equal(eout[:ebytes], xout[:xbytes]))
        print(json.dumps({"what": "check: decode(extract) == subset decode, by record digest", "run": k, "identical": ok,
                          "equals_through_text_bytes": same, "records": n, "samples": S, "record_bytes": rec_bytes,
                          "output_bytes": xbytes}), flush=True)
        assert ok and same
        del dec, doff

    runs = []
    for k in colsets:
        runs += [("extract_" + k, (lambda k=k: extract(k))), ("subset_" + k, (lambda k=k: subset(k))),
                 ("through_text_" + k, (lambda k=k: through_text(k)))]
    runs += [("copy_records", lambda: copy_dst.copy_(recs[:rec_bytes])), ("region_extract_all", region_extract)]
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
            if it == 0 and k != "copy_records":
                assert noerr(err), k
                if k.startswith(("extract_", "region_")):
                    outb[k] = int(xoff[n].item())
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, _ in runs:
        r = stats(times[k])
        r.update({"what": k, "records": n, "samples": S, "record_bytes": rec_bytes})
        if k in outb:
            r["output_bytes"] = outb[k]
        if k.startswith("extract_"):
            cs = k[len("extract_"):]
            r["columns"] = width[cs]
            for y in ("copy_records", "subset_" + cs, "through_text_" + cs):
                if y in med:
                    r["ratio_to_" + y.replace("_" + cs, "")] = round(r["median_ms"] / med[y], 3)
        if k == "region_extract_all":
            r["region"] = "%s:%d-%d" % (rows.chrom, qs, qe)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
