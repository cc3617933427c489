"""k_sparse_plan (csrc/vcfc_sparse.hip) on the CPU emulator: the planned
offsets/prefixes, applied with the reference's write order, reproduce the
reference's sparse file (hole-aware digest); and the kernel against the plain
statement of tests/sparse_cases.py on its edge families, that statement
against the oracle restatement and the reference's recorded files."""
import os
import struct
import tempfile

import numpy as np
import pytest

import emu_io as E
import golden_io as G
import sparse_cases as C
import sparse_digest


def materialise(v, path):
    """vcfc_sparsify_file's write loop (csrc/vcfc_api.cpp) over the emulated
    plan: the records before the first unparsable one, each behind its planned
    prefix with one write, or -- where the plan flags an anomaly -- in the
    reference's order with dist_to_next written as 0 and patched by the next
    record's step.  Returns (status, replay)."""
    hdr, recs, tail_ok = C.split(v)
    data_start = len(hdr) + 8
    fo, pf, st = E.emu_sparse_plan(b"".join(recs), C.rec_offsets(recs), data_start, fill=0xAB)
    upto = len(recs) if st[0] == C.NONE or not recs else int(st[0]) >> 8
    replay = bool(st[1] != 0)
    fd = os.open(path, os.O_CREAT | os.O_TRUNC | os.O_RDWR, 0o600)
    os.pwrite(fd, hdr + b"\0" * 8, 0)
    for i in range(upto):
        pre = bytearray(pf[16 * i:16 * i + 16])
        if i == 0:
            os.pwrite(fd, struct.pack("<Q", (int(fo[0]) - data_start) & C.M64), data_start - 8)
        elif replay:
            os.pwrite(fd, struct.pack(">Q", (int(fo[i]) - int(fo[i - 1])) & C.M64), int(fo[i - 1]) + 8)
        if replay:
            pre[8:16] = b"\0" * 8
        os.pwrite(fd, bytes(pre) + recs[i], int(fo[i]))
    os.close(fd)
    return (C.E_FORMAT if upto < len(recs) or not tail_ok else C.OK), replay


def test_plan_random_100x10000():
    v = G.gz("random_100x10000.vcfc.gz")
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "o.sparse")
        assert materialise(v, p) == (C.OK, False)
        assert sparse_digest.digest(p) == G.manifest()["sparse_100x10000"]


def test_plan_edge_overlap_replay():
    v = G.gz("sparse_edge.vcfc.gz")
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "o.sparse")
        assert materialise(v, p) == (C.OK, True)
        assert sparse_digest.digest(p) == G.manifest()["sparse_edge"]


def test_sparse_query_driver_matches_oracle_and_reference():
    """vcfc_dec::sparse_query (product driver + decode kernels, emulated) on
    every golden sparse-query case: byte-identical to the oracle restatement
    (including every line before a throw) and consistent with the reference
    CLI's recorded stdout / exit status."""
    d = G.sparse_query_cases()
    with tempfile.TemporaryDirectory(dir="/tmp") as wd:
        built = set()
        for c in d["cases"]:
            path = os.path.join(wd, c["file"] + ".sparse")
            if c["file"] not in built:
                G.build_sparse_file(d, c["file"], path, G.oracle_sparsify)
                built.add(c["file"])
            q = c["query"].encode()
            want = G.oracle_sparse_query(path, q)
            ref, hr, a, b = G.oracle_parse_query(q)
            got = E.emu_sparse_query(path, ref, hr, a, b)
            assert got == want, (c, got[0], want[0], len(got[1]), len(want[1]))
            assert G.check_sparse_case(c, *got), c


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_sparse_query_driver_on_mutated_files(seed):
    """Random byte patches in the distance prefixes, record headers and
    bodies of a sparse file (walk errors, off-hop parses, bad POS fields):
    the product driver against the oracle restatement."""
    d = G.sparse_query_cases()
    with tempfile.TemporaryDirectory(dir="/tmp") as wd:
        path = os.path.join(wd, "m.sparse")
        G.build_sparse_file(d, "random_100x10000", path, G.oracle_sparsify)
        C.mutate_random_sparse(path, seed)
        for q in C.MUTATED_QUERIES:
            want = G.oracle_sparse_query(path, q)
            ref, hr, a, b = G.oracle_parse_query(q)
            got = E.emu_sparse_query(path, ref, hr, a, b)
            assert got == want, (seed, q, got[0], want[0], len(got[1]), len(want[1]))


# ---- the edge families of sparse_cases.py -----------------------------------

def emu_plan(v):
    _, recs, _ = C.split(v)
    return E.emu_sparse_plan(b"".join(recs), C.rec_offsets(recs), C.data_start_of(v), fill=0xAB)


@pytest.mark.parametrize("family", sorted(C.FAMILIES))
def test_plan_contract(family):
    """k_sparse_plan against the plain statement on every case of a family,
    plan-only cases included, under the contract of sparse_cases.check_plan
    (outputs prefilled with 0xAB: a record the kernel skipped shows)."""
    ran = 0
    for name, v, _ in C.all_cases():
        if name.startswith(family + "/"):
            C.check_plan(name, v, *emu_plan(v))
            ran += 1
    assert ran == len(C.FAMILIES[family]())


def test_plan_only_cases():
    """POS -1, POS 2^64 - 1 and an offset that wraps below data_start never
    reach a file: the plan alone, with what the statement says of each."""
    cases = {name: v for name, v, disk in C.all_cases() if not disk}
    for name, pos in (("pos_forms/huge_neg1", C.M64), ("pos_forms/huge_18446744073709551615", C.M64),
                      ("pos_forms/huge_18446744073709551616", C.M64)):
        v = cases[name]
        _, recs, _ = C.split(v)
        assert C.pos_of(recs[1][8:]) == pos
        fo, pf, st = emu_plan(v)
        C.check_plan(name, v, fo, pf, st)
        # (L - 1) slots from data_start: below record 0's offset, so out of order
        assert int(fo[1]) == C.data_start_of(v) + (C.SPARSE_L - 1) * C.STRIDE and st[1] != 0
    for name in ("pos_forms/wrap_alone", "pos_forms/wrap_first"):
        v = cases[name]
        fo, pf, st = emu_plan(v)
        C.check_plan(name, v, fo, pf, st)
        ds = C.data_start_of(v)
        assert ds > C.STRIDE and int(fo[0]) == ds - C.STRIDE and st[0] == C.NONE and st[1] != 0


def test_image_equals_oracle_and_reference():
    """The plain statement's file against vcfo_sparsify (status and digest) on
    every disk-bound case, and against the reference's own recorded
    `main sparsify` (tests/golden/sparse_edge_cases.json) where it is recorded."""
    gold = C.golden()
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        p = os.path.join(d, "o.sparse")
        for name, v in C.disk_cases():
            st = G.oracle().vcfo_sparsify(v, len(v), p.encode())
            assert C.same_as_image(v, st, p), (name, st, C.image_digest(v)[0])
            if name in gold:
                C.check_golden(name, v, *C.image_digest(v))
    assert sum(c["rc"] != 0 for c in gold.values()) >= 10 and sum(c["rc"] == 0 for c in gold.values()) >= 10


def test_write_loop_over_emulated_plan():
    """The driver's write loop over the kernel's own plan, garbage
    dist_to_next of the last written record included, leaves the statement's
    file on every disk-bound case."""
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        p = os.path.join(d, "o.sparse")
        for name, v in C.disk_cases():
            if len(v) == C.header_end(v):
                continue   # the header reader throws: no plan is made
            st, _ = materialise(v, p)
            assert C.same_as_image(v, st, p), (name, st)


def test_sparse_query_over_adjacent_files():
    """Queries at every record's POS and over the whole span of the adjacent
    files, whose overlapping records leave later writes on top of earlier
    ones: the product driver against the oracle restatement."""
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        p = os.path.join(d, "a.sparse")
        outcomes = set()
        for name, v in C.adjacent():
            assert G.oracle().vcfo_sparsify(v, len(v), p.encode()) == C.OK
            for q in C.span_queries(v):
                want = G.oracle_sparse_query(p, q)
                ref, hr, a, b = G.oracle_parse_query(q)
                got = E.emu_sparse_query(p, ref, hr, a, b)
                assert got == want, (name, q, got[0], want[0], len(got[1]), len(want[1]))
                outcomes.add((want[0], bool(want[1])))
        assert {(C.OK, True), (C.E_FORMAT, False)} <= outcomes


def test_shard_slices():
    """The plan of every rank's slice (its records and one halo record each
    side, worlds 2, 3 and 5) of the 257-record shard files, a defect on and
    next to every halo record: first error and anomaly flag as the slice
    plan's, which is what vcfc_sparsify_shard reports."""
    flagged = clean = 0
    for name, v in C.shard_files():
        _, recs, _ = C.split(v)
        n = len(recs)
        if n != 257:
            continue
        for world in C.SHARD_WORLDS:
            for rank in range(world):
                lo, hi = n * rank // world, n * (rank + 1) // world
                a, b = max(lo - 1, 0), min(hi + 1, n)
                _, _, st = E.emu_sparse_plan(b"".join(recs[a:b]), C.rec_offsets(recs[a:b]), C.data_start_of(v))
                info = [lo, hi, None if st[0] == C.NONE else a + (int(st[0]) >> 8), int(st[1] != 0)]
                assert int(st[0]) == C.NONE or int(st[0]) & 0xFF == C.E_FORMAT
                assert info == C.shard_info(recs, rank, world, C.data_start_of(v)), (name, world, rank, info)
                flagged += info[2] is not None or info[3]
                clean += info[2] is None and not info[3]
    assert flagged >= 100 and clean >= 100
