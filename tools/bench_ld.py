#!/usr/bin/env python3
"""Measurements of ld-window (report only; DESIGN.md §4n cites the lines, raw
copies go under profiles/ld/).

Over the headline batch (2504 samples x 1M chr22-shaped rows, encoded in HBM),
timed with HIP events, alternating, in one process, for W = 16 and W = 64:

  vcfc_ld_window_device (the composed call: .bed rows, bit planes, pairs) and
  vcfc_ld_tables_device on the .bed matrix (planes and pairs alone), against
  yardsticks measured in the same run: (a) the .bed matrix call alone on the
  same records, (b) a device fill of the band's bytes (the write floor), (c)
  what a user has without the feature: for a block of --block rows the three
  genotype indicators unpacked from the .bed rows to float32 and float16, and
  the one stacked [3 B, S] x [S, 3 B] torch.matmul that holds every table of
  the block, reported per useful (in-band) pair.

Before timing, the band of both windows is checked on a sample of rows
against a straightforward count with torch on the unpacked .bed matrix.  One
JSON line per measurement on stdout."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_index import encode, stats  # noqa: E402


def unpack(torch, bed, S):
    """int8[rows, S] genotypes of .bed rows: 0, 1, 2, -1 missing."""
    sh = torch.tensor([0, 2, 4, 6], dtype=torch.uint8, device=bed.device)
    code = ((bed.unsqueeze(2) >> sh) & 3).reshape(bed.shape[0], -1)[:, :S]
    lut = torch.tensor([2, -1, 1, 0], dtype=torch.int8, device=bed.device)   # 00 -> 2, 01 -> missing, 10 -> 1, 11 -> 0
    return lut[code.long()]


def band_pairs(n, W):
    """Pairs (i, i + k), k = 1..W, among n rows."""
    return sum(min(W, n - 1 - i) for i in range(n)) if n <= W else (n - W) * W + W * (W - 1) // 2


def check(torch, bed, tables, n, S, W, starts, span=96):
    """Rows [i0, i0 + span) of the band against a count over the unpacked rows."""
    ok, pairs = True, 0
    for i0 in starts:
        hi = min(n, i0 + span + W)
        g = unpack(torch, bed[i0:hi], S)
        ind = torch.stack([(g == a) for a in range(3)], 1).to(torch.float32)   # [rows, 3, S]
        for i in range(i0, min(n, i0 + span)):
            k = min(W, n - 1 - i)
            want = torch.zeros((W, 3, 3), dtype=torch.int64, device=bed.device)
            if k > 0:
                want[:k] = torch.einsum("as,kbs->kab", ind[i - i0], ind[i - i0 + 1:i - i0 + 1 + k]).round().long()
            ok &= bool(torch.equal(tables[i].long(), want))
            pairs += k
    return ok, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--windows", default="16,64")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--block", type=int, default=4096, help="rows of the torch.matmul yardstick")
    ap.add_argument("--only", default=None, help="comma-separated run names (for a profiler run)")
    ap.add_argument("--no-check", action="store_true", help="skip the check against the straightforward count")
    args = ap.parse_args()
    import numpy as np
    import torch   # before libvcfc: one HIP runtime in the process
    import vcfc
    import workload
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    n, S = args.rows, args.samples
    Ws = [int(w) for w in args.windows.split(",")]
    rows, recs, rec, rec_bytes = encode(torch, vcfc, workload, n, S, dev)
    del rows
    torch.cuda.empty_cache()
    s = torch.cuda.current_stream(dev).cuda_stream
    rb = vcfc.matrix_row_bytes(vcfc.GM_BED, S)
    bed = torch.empty((n, rb), dtype=torch.uint8, device=dev)
    row_of = torch.empty(n + 1, dtype=torch.int64, device=dev)
    mwsb = vcfc.matrix_workspace_size(n, S, vcfc.GM_BED)
    mws = torch.empty(mwsb, dtype=torch.uint8, device=dev)
    wsb = vcfc.ld_workspace_size(n, S, max(Ws))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    tables = {W: torch.empty((n, W, 3, 3), dtype=torch.int32, device=dev) for W in Ws}
    err = torch.empty(1, dtype=torch.int64, device=dev)

    def noerr():
        return int(err.cpu().numpy().view(np.uint64)[0]) == vcfc.NO_ERROR

    def matrix_bed():
        vcfc.raise_for(vcfc.genotype_matrix_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), None, n, S, vcfc.GM_BED,
                                                   bed.data_ptr(), n * rb, rb, row_of.data_ptr(), mws.data_ptr(), mwsb,
                                                   err.data_ptr(), s))

    def window(W):
        vcfc.raise_for(vcfc.ld_window_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), None, n, S, W, tables[W].data_ptr(),
                                             n * W, row_of.data_ptr(), ws.data_ptr(), wsb, err.data_ptr(), s))

    def pair_step(W):
        vcfc.raise_for(vcfc.ld_tables_device(bed.data_ptr(), n, rb, S, W, tables[W].data_ptr(), n * W, ws.data_ptr(), wsb,
                                             err.data_ptr(), s))

    matrix_bed()
    torch.cuda.synchronize(dev)
    assert noerr()
    if not args.no_check:
        starts = sorted({0, 4093, n // 2 + 7, max(0, n - 200), max(0, n - 96)})
        for W in Ws:
            for name, f in (("ld_window", window), ("ld_tables", pair_step)):
                tables[W].fill_(-1)
                f(W)
                torch.cuda.synchronize(dev)
                assert noerr(), (name, W)
                ok, pairs = check(torch, bed, tables[W], n, S, W, starts)
                print(json.dumps({"what": "check: %s == a straightforward count" % name, "window": W, "identical": ok,
                                  "rows": n, "samples": S, "pairs_checked": pairs}), flush=True)
                assert ok

    # yardstick (c): one block of rows, every table of the block by one stacked matmul
    B = min(args.block, n)
    ind = {}

    def unpack_block(dtype):
        g = unpack(torch, bed[:B], S)
        ind[dtype] = torch.cat([(g == a) for a in range(3)], 0).to(dtype)   # [3 B, S]

    def matmul_block(dtype):
        return torch.matmul(ind[dtype], ind[dtype].t())

    runs = [("matrix_bed", matrix_bed)]
    for W in Ws:
        runs += [("ld_window_W%d" % W, (lambda W=W: window(W))), ("ld_tables_W%d" % W, (lambda W=W: pair_step(W))),
                 ("fill_band_W%d" % W, (lambda W=W: tables[W].fill_(1)))]
    for dt, nm in ((torch.float32, "f32"), (torch.float16, "f16")):
        unpack_block(dt)
        runs += [("torch_unpack_%s" % nm, (lambda dt=dt: unpack_block(dt))), ("torch_matmul_%s" % nm, (lambda dt=dt: matmul_block(dt)))]
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
            if it == 0 and k.startswith(("matrix", "ld_")):
                assert noerr(), k
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, _ in runs:
        r = stats(times[k])
        r.update({"what": k, "rows": n, "samples": S})
        if "_W" in k:
            W = int(k.rsplit("_W", 1)[1])
            pairs = band_pairs(n, W)
            r.update({"window": W, "pairs": pairs, "band_bytes": 36 * n * W})
            if k.startswith("ld_"):
                r["pairs_per_s"] = round(pairs / (r["median_ms"] * 1e-3))
                r["band_GBps"] = round(36 * n * W / (r["median_ms"] * 1e6), 1)
                for y in ("matrix_bed", "fill_band_W%d" % W):
                    if y in med:
                        r["ratio_to_" + y] = round(r["median_ms"] / med[y], 3)
        if k.startswith("torch_matmul"):
            r["block_rows"] = B
            for W in Ws:
                useful = band_pairs(B, W)
                r["ns_per_useful_pair_W%d" % W] = round(r["median_ms"] * 1e6 / useful, 2)
                if "ld_window_W%d" % W in med:
                    r["ld_window_ns_per_pair_W%d" % W] = round(med["ld_window_W%d" % W] * 1e6 / (n * W), 4)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
