#!/usr/bin/env python3
"""Time one buffer call each through the C ABI of the library VCFC_LIB names,
over a .vcfc of the benchmark's shape (chr22-shaped rows, 2504 samples) held in
host memory.  One JSON line: median / min / max ms per path."""
import ctypes
import json
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    rows_n = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    S = 2504
    import numpy as np
    import torch
    import vcfc
    import workload
    from bench_index import encode
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rows, recs, rec, rec_bytes = encode(torch, vcfc, workload, rows_n, S, dev)
    header = ("##fileformat=VCFv4.2\n##source=host_paths\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"
              + "".join("\ts%d" % i for i in range(S)) + "\n").encode()
    data = header + recs[:rec_bytes].cpu().numpy().tobytes()
    line_bytes = int(rows.line_bytes)
    a, b = int(rows_n * 0.4375), int(rows_n * 0.5625)
    qs, qe = int(rows.pos[a]), int(rows.pos[b])
    ref = rows.chrom.encode()
    del rows, recs, rec
    torch.cuda.empty_cache()
    src = np.frombuffer(data, dtype=np.uint8)
    cap = len(header) + line_bytes + rows_n + 4096
    out = np.empty(cap, dtype=np.uint8)
    n = ctypes.c_uint64(0)
    cols = np.array(sorted(random.Random(7).sample(range(S), 64)), dtype=np.uint32)
    L = vcfc.lib()
    ctx = vcfc.Context(0)
    h = ctx._h
    res = {}

    def check(st, what):
        assert st == 0, (what, st)
        res.setdefault(what + "_bytes", n.value)

    def full_decode():
        check(L.vcfc_decompress_buffer(h, src.ctypes.data, len(data), out.ctypes.data, cap, ctypes.byref(n)), "full_decode")

    def range_query():
        check(L.vcfc_query_buffer(h, src.ctypes.data, len(data), ref, len(ref), 1, qs, qe, out.ctypes.data, cap,
                                  ctypes.byref(n)), "range_query")

    def samples_k64():
        check(L.vcfc_decompress_samples_buffer(h, src.ctypes.data, len(data), cols.ctypes.data, len(cols), out.ctypes.data,
                                               cap, ctypes.byref(n)), "decompress_samples_k64")

    def extract_k64():
        check(L.vcfc_extract_buffer(h, src.ctypes.data, len(data), cols.ctypes.data, len(cols), 0, None, 0, 0, 0, 0,
                                    out.ctypes.data, cap, ctypes.byref(n)), "extract_k64")

    def counts():
        r = ctx.genotype_counts_buffer(data)
        assert r[0] == 0, ("genotype_counts", r[0])

    def matrix():
        r = ctx.genotype_matrix_buffer(data, vcfc.GM_DOSAGE)
        assert r[0] == 0, ("genotype_matrix", r[0])

    paths = [("full_decode", full_decode), ("range_query", range_query), ("decompress_samples_k64", samples_k64),
             ("extract_k64", extract_k64), ("genotype_counts", counts), ("genotype_matrix_dosage", matrix)]
    times = {k: [] for k, _ in paths}
    for it in range(1 + reps):
        for k, f in paths:
            t0 = time.perf_counter()
            f()
            if it:
                times[k].append((time.perf_counter() - t0) * 1e3)
    for k, v in times.items():
        res[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    res.update({"lib": os.environ.get("VCFC_LIB", "build/libvcfc.so"), "rows": rows_n, "samples": S, "file_bytes": len(data),
                "reps": reps})
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
