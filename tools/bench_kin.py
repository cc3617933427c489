#!/usr/bin/env python3
"""Measurements of kinship (report only; DESIGN.md §4o cites the lines, raw
copies go under profiles/kin/).

Over the headline batch (2504 samples x 1M chr22-shaped rows, encoded in HBM),
timed with HIP events, alternating, in one process:

  vcfc_kin_records_device (the composed call: .bed rows, sample-major bit
  planes, pairs) and vcfc_kin_tables_device on the .bed matrix (planes and
  pairs alone), against yardsticks measured in the same run: (a) the .bed
  matrix call alone on the same records, (b) a device fill of the square's
  bytes (the write floor), (c) what a user has without the feature: for a
  block of --block rows the three genotype indicators unpacked from the .bed
  rows to float32 (exact counts) and float16 (the rate only), and the stacked
  [3 S, B] x [B, 3 S] torch.matmul that holds the block's share of every
  table, added into an int32 square; (c) is timed on one block and scaled to
  the rows.

Before timing, two slabs of the square are checked against a straightforward
count with torch on the unpacked .bed matrix.  One JSON line per measurement
on stdout."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_index import encode, stats  # noqa: E402
from bench_ld import unpack  # noqa: E402


def slab_count(torch, bed, S, s0, s1, block=65536):
    """int64[s1 - s0, S, 3, 3]: the tables of samples [s0, s1) against all, over every row of bed."""
    want = torch.zeros(((s1 - s0) * 3, S * 3), dtype=torch.int64, device=bed.device)
    for r0 in range(0, bed.shape[0], block):
        g = unpack(torch, bed[r0:r0 + block], S)
        ind = torch.stack([(g == a) for a in range(3)], 2).to(torch.float32)   # [rows, S, 3]; a block's counts < 2^24
        want += (ind[:, s0:s1].reshape(g.shape[0], -1).t() @ ind.reshape(g.shape[0], -1)).round().long()
    return want.view(s1 - s0, 3, S, 3).permute(0, 2, 1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--samples", type=int, default=2504)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--block", type=int, default=16384, help="rows of the torch.matmul yardstick")
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
    rows, recs, rec, rec_bytes = encode(torch, vcfc, workload, n, S, dev)
    del rows
    torch.cuda.empty_cache()
    s = torch.cuda.current_stream(dev).cuda_stream
    rb = vcfc.matrix_row_bytes(vcfc.GM_BED, S)
    bed = torch.empty((n, rb), dtype=torch.uint8, device=dev)
    row_of = torch.empty(n + 1, dtype=torch.int64, device=dev)
    mwsb = vcfc.matrix_workspace_size(n, S, vcfc.GM_BED)
    mws = torch.empty(mwsb, dtype=torch.uint8, device=dev)
    wsb = vcfc.kin_workspace_size(n, S)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    tables = torch.empty((S, S, 3, 3), dtype=torch.int32, device=dev)
    err = torch.empty(1, dtype=torch.int64, device=dev)

    def noerr():
        return int(err.cpu().numpy().view(np.uint64)[0]) == vcfc.NO_ERROR

    def matrix_bed():
        vcfc.raise_for(vcfc.genotype_matrix_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), None, n, S, vcfc.GM_BED,
                                                   bed.data_ptr(), n * rb, rb, row_of.data_ptr(), mws.data_ptr(), mwsb,
                                                   err.data_ptr(), s))

    def composed():
        vcfc.raise_for(vcfc.kin_records_device(recs.data_ptr(), rec_bytes, rec.data_ptr(), None, n, S, tables.data_ptr(), S * S, 0,
                                               row_of.data_ptr(), ws.data_ptr(), wsb, err.data_ptr(), s))

    def pair_step():
        vcfc.raise_for(vcfc.kin_tables_device(bed.data_ptr(), n, rb, S, tables.data_ptr(), S * S, 0, ws.data_ptr(), wsb,
                                              err.data_ptr(), s))

    matrix_bed()
    torch.cuda.synchronize(dev)
    assert noerr()
    if not args.no_check:
        slabs = [(0, min(S, 48)), (max(0, S - 40), S)]
        want = [slab_count(torch, bed, S, s0, s1) for s0, s1 in slabs]
        for name, f in (("kin_records", composed), ("kin_tables", pair_step)):
            tables.fill_(-1)
            f()
            torch.cuda.synchronize(dev)
            assert noerr(), name
            ok = all(bool(torch.equal(tables[s0:s1].long(), w)) for (s0, s1), w in zip(slabs, want))
            sym = bool(torch.equal(tables[:64, S - 64:], tables[S - 64:, :64].permute(1, 0, 3, 2)))
            print(json.dumps({"what": "check: %s == a straightforward count" % name, "identical": ok, "transpose_identity": sym,
                              "rows": n, "samples": S, "tables_checked": sum((s1 - s0) * S for s0, s1 in slabs)}), flush=True)
            assert ok and sym
        del want

    # yardstick (c): one block of rows, its share of every table by one stacked matmul, added into an int32 square
    B = min(args.block, n)
    acc = torch.zeros((3 * S, 3 * S), dtype=torch.int32, device=dev)
    ind = {}

    def unpack_block(dtype):
        g = unpack(torch, bed[:B], S)
        ind[dtype] = torch.cat([(g == a) for a in range(3)], 1).to(dtype)   # [B, 3 S]

    def matmul_block(dtype):
        acc.add_(torch.matmul(ind[dtype].t(), ind[dtype]).to(torch.int32))

    runs = [("matrix_bed", matrix_bed), ("kin_records", composed), ("kin_tables", pair_step), ("fill_square", lambda: tables.fill_(1))]
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
            if it == 0 and k.startswith(("matrix", "kin_")):
                assert noerr(), k
    med = {k: statistics.median(v) for k, v in times.items()}
    pairs = S * (S + 1) // 2
    words = (n + 31) // 32
    floor_ms = pairs * words * 18 / 64 * 4 / (1024 * 2.4e9) * 1e3   # 18 VALU a pair and word, a wave64 instruction per 4 cycles
    for k, _ in runs:
        r = stats(times[k])
        r.update({"what": k, "rows": n, "samples": S})
        if k.startswith("kin_"):
            r.update({"pairs": pairs, "square_bytes": 36 * S * S, "arithmetic_floor_ms": round(floor_ms, 2),
                      "ratio_to_floor": round(r["median_ms"] / floor_ms, 2),
                      "pair_words_per_s": round(pairs * words / (r["median_ms"] * 1e-3))})
            for y in ("matrix_bed", "fill_square"):
                if y in med:
                    r["ratio_to_" + y] = round(r["median_ms"] / med[y], 3)
        if k.startswith("torch_"):
            r["block_rows"] = B
            r["scaled_to_rows_ms"] = round(r["median_ms"] * n / B, 1)
        if k.startswith("torch_matmul"):
            nm = k.rsplit("_", 1)[1]
            whole = (med[k] + med.get("torch_unpack_" + nm, 0.0)) * n / B
            r["unpack_and_matmul_scaled_ms"] = round(whole, 1)
            r["tflops"] = round(2 * (3 * S) ** 2 * B / (r["median_ms"] * 1e-3) / 1e12, 1)
            if "kin_records" in med:
                r["ratio_to_kin_records"] = round(whole / med["kin_records"], 2)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
