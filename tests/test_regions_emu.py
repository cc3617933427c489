"""Region-list queries on the CPU: the Python restatement
(regions_cases.py) pinned to the reference CLI's own per-region output
(tests/golden/regions_cases.json), then the product kernel
(csrc/vcfc_regions.hip), the table builder and validator
(csrc/vcfc_regions_driver.h) and the three host drivers compiled against the
fiber SIMT emulator, held to the restatement: table bytes, flags, error word,
status and output bytes, all exact.  test_gpu_regions.py repeats it on the
GPU."""
import ctypes
import hashlib
import struct

import numpy as np

import emu_io as E
import golden_io as G
import regions_cases as RC
import subset_cases as SC

OK, E_NOSPACE, E_ARG, E_FORMAT = RC.OK, RC.E_NOSPACE, RC.E_ARG, RC.E_FORMAT
_lib = None


def lib():
    """The emulator build of the region kernel and the drivers (flags as tests/simt_emu/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    L = E.build_emu_lib("regions", ("vcfc_regions.hip", "vcfc_decode.hip", "vcfc_subset.hip", "vcfc_counts.hip",
                        "vcfc_encode.hip"), "emu_regions_api.cpp")
    vp, u64, cp, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int
    pu64 = ctypes.POINTER(u64)
    L.emu_regions_build.argtypes = [cp, u64, vp, u64, pu64, pu64, pu64]
    L.emu_regions_workspace_size.restype = u64
    L.emu_regions_workspace_size.argtypes = [u64]
    L.emu_regions_upload.argtypes = [cp, u64, vp, u64]
    L.emu_regions_match.argtypes = [cp, vp, u64, vp, u64, vp, vp]
    L.emu_regions_query_match.argtypes = [cp, vp, u64, cp, u64, ci, u64, u64, vp, vp]
    L.emu_regions_query.argtypes = [cp, u64, cp, u64, vp, u64, pu64, u64]
    L.emu_regions_query_samples.argtypes = [cp, u64, cp, u64, vp, u64, vp, u64, pu64, u64]
    L.emu_regions_counts.argtypes = [cp, u64, cp, u64, u64, vp, vp, u64, pu64, vp, pu64, pu64]
    _lib = L
    return L


def build_status(text, cap=None):
    """emu_regions_build: (status, table bytes, regions, bad line, size needed)."""
    nb, nr, bad = (ctypes.c_uint64(0) for _ in range(3))
    st = lib().emu_regions_build(text, len(text), None, 0, ctypes.byref(nb), ctypes.byref(nr), ctypes.byref(bad))
    if st != E_NOSPACE:
        return st, b"", nr.value, bad.value, nb.value
    need = nb.value
    cap = need if cap is None else cap
    out = np.full(cap + 8, 0xEE, dtype=np.uint8)
    st = lib().emu_regions_build(text, len(text), out.ctypes.data, cap, ctypes.byref(nb), ctypes.byref(nr), ctypes.byref(bad))
    assert (out[cap:] == 0xEE).all(), "bytes written past table_cap"
    return st, out[:nb.value].tobytes() if st == OK else b"", nr.value, bad.value, nb.value


def build(text):
    st, table, nr, bad, need = build_status(text)
    if st == E_ARG and bad:
        raise RC.RegionError(bad)
    assert st == OK and len(table) == need, st
    return table


def upload(table, extra=0):
    """emu_regions_upload into a fresh workspace: (status, workspace, ws_bytes)."""
    wsb = lib().emu_regions_workspace_size(len(table)) + extra
    ws = np.full(wsb + 64, 0xCD, dtype=np.uint8)
    st = lib().emu_regions_upload(table, len(table), ws.ctypes.data, wsb)
    assert (ws[wsb:] == 0xCD).all(), "bytes written past ws_bytes"
    return st, ws, wsb


def flags(body, rec, table):
    st, ws, wsb = upload(table)
    assert st == OK
    n = len(rec) - 1
    r = np.array(rec, dtype=np.uint64)
    f = np.full(n + 64, 0xEE, dtype=np.uint8)
    err = np.zeros(1, dtype=np.uint64)
    for _ in range(2):   # twice on one workspace: the error word is reset, the table is not consumed
        st = lib().emu_regions_match(body, r.ctypes.data, n, ws.ctypes.data, wsb, f.ctypes.data, err.ctypes.data)
        assert st == OK
    assert (f[n:] == 0xEE).all() and (ws[wsb:] == 0xCD).all(), "bytes written past the flags / the workspace"
    return [int(x) for x in f[:n]], int(err[0])


def single(body, rec, q):
    n = len(rec) - 1
    r = np.array(rec, dtype=np.uint64)
    f = np.full(n + 64, 0xEE, dtype=np.uint8)
    err = np.zeros(1, dtype=np.uint64)
    st = lib().emu_regions_query_match(body, r.ctypes.data, n, q[0], len(q[0]), int(q[1]), q[2], q[3], f.ctypes.data,
                                       err.ctypes.data)
    assert st == OK
    return [int(x) for x in f[:n]], int(err[0])


def emu_qry(data, text, out_batch=1 << 12):
    table = build(text)
    cap = len(data) * 8 + 4096
    out = np.zeros(cap, dtype=np.uint8)
    n = ctypes.c_uint64(0)
    st = lib().emu_regions_query(data, len(data), table, len(table), out.ctypes.data, cap, ctypes.byref(n), out_batch)
    return st, out[:n.value].tobytes()


def emu_qsam(data, text, cols, out_batch=1 << 12):
    table = build(text)
    c = np.array(cols, dtype=np.uint32)
    cap = len(data) * 8 + 4096
    out = np.zeros(cap, dtype=np.uint8)
    n = ctypes.c_uint64(0)
    st = lib().emu_regions_query_samples(data, len(data), table, len(table), c.ctypes.data, len(cols), out.ctypes.data, cap,
                                         ctypes.byref(n), out_batch)
    return st, out[:n.value].tobytes()


def emu_cnt(data, text, rec_batch=16):
    table = build(text)
    h = SC.parse_header(data)
    S = h[1] if h else 1
    cap = len(SC.hop(data[h[0]:])[0]) if h else 1
    idx = np.zeros(cap + 1, dtype=np.uint64)
    rows = np.zeros((cap + 1, 8), dtype=np.uint32)
    samples = np.zeros((max(S, 1), 5), dtype=np.uint64)
    n, ns, bad = (ctypes.c_uint64(0) for _ in range(3))
    st = lib().emu_regions_counts(data, len(data), table, len(table), rec_batch, idx.ctypes.data, rows.ctypes.data, cap + 1,
                                  ctypes.byref(n), samples.ctypes.data, ctypes.byref(ns), ctypes.byref(bad))
    return st, [int(x) for x in idx[:n.value]], rows[:n.value].tolist(), samples.tolist() if st == OK else None, bad.value


# ---- the restatement alone (no kernel) ----------------------------------------

def test_restatement_set_counts_and_the_oracle_query():
    """A..E match 33, 21, 13, 0 and 1 of the 60 records, and a one-region
    set is the oracle's query."""
    name, data = SC.query_files(1)[0]
    body, rec, S = RC.records_of(data)
    for key, text in RC.SETS.items():
        want = RC.expected(body, rec, RC.parse_text(text))
        assert (sum(want[0]), want[1]) == (RC.SET_MATCHES[key], RC.NO_ERROR), key
    for q in SC.QUERIES:
        st, want = G.oracle_query(data, SC.query_string(q))
        region = (q[0], q[2], q[3]) if q[1] else (q[0], 0, RC.U64)   # (the bare wildcard is an empty line: no text)
        assert st == 0 and RC.query_regions(data, [region]) == (OK, want), q
        if SC.query_string(q):
            assert RC.parse_text(SC.query_string(q) + b"\n") == [region]


def test_restatement_outcomes_on_mutated_files():
    """Over no_lf / nul_req x A..C: 8 (file, set) pairs stop, 16 run through."""
    stopped = through = 0
    for name, data in SC.query_files(1):
        if name.startswith(("no_lf", "nul_req")):
            for key in "ABC":
                st = RC.query_samples_regions(data, RC.parse_text(RC.SETS[key]), [0])[0]
                assert RC.counts_regions(data, RC.parse_text(RC.SETS[key]))[0] == st
                stopped += st == E_FORMAT
                through += st == OK
    assert (stopped, through) == (8, 16)


def test_restatement_reproduces_the_reference_cli():
    RC.check_golden(lambda data, text: RC.query_regions(data, RC.parse_text(text)))


# ---- the table ---------------------------------------------------------------------

def test_region_text():
    RC.check_text(build)
    st, table, nr, bad, need = build_status(RC.SETS["A"])
    assert (st, nr, bad) == (OK, 6, 0)   # the empty region 1:500-400 counts as parsed
    assert build_status(b"")[:4] == (OK, build(b"#\n"), 0, 0) and len(build(b"")) == 48
    # a short table buffer: the size needed, nothing written past the cap
    st, _, nr, bad, got = build_status(RC.SETS["A"], cap=need - 1)
    assert (st, got, nr) == (E_NOSPACE, need, 6)


def test_table_layout():
    """Names sorted by (length, bytes) with the wildcard first; starts and
    ends as two arrays; a name's intervals merged and disjoint."""
    table = build(b"chr1:5-9\n1:30-40\n:7-7\n11\n1:10-19\n1:20-25\n2:1-1\n1:35-50\n")
    magic, ver, n_names, n_iv, o_names, o_st, o_en, o_by, total, n_by = struct.unpack_from("<10I", table)
    assert (magic, ver, n_names, n_iv, total) == (0x47524356, 1, 5, 6, len(table))
    names = [struct.unpack_from("<4I", table, o_names + 16 * k) for k in range(n_names)]
    got = [(table[o_by + bo:o_by + bo + ln], [(struct.unpack_from("<Q", table, o_st + 8 * j)[0],
                                               struct.unpack_from("<Q", table, o_en + 8 * j)[0]) for j in range(f, f + c)])
           for bo, ln, f, c in names]
    assert got == [(b"", [(7, 7)]), (b"1", [(10, 25), (30, 50)]), (b"2", [(1, 1)]), (b"11", [(0, RC.U64)]),
                   (b"chr1", [(5, 9)])]
    # adjacent to an interval that ends at 2^64 - 1: end + 1 must not wrap
    t = build(b"1:5-18446744073709551615\n1:0-3\n1:9-10\n")
    assert struct.unpack_from("<4I", t)[3] == 2


def test_upload_validation():
    table = bytearray(build(b"1:10-19\n1:30-40\n2:5-6\nchrX\n"))   # names "1" (two intervals), "2", "chrX"
    assert upload(bytes(table))[0] == OK
    assert upload(bytes(table), extra=-256)[0] == E_ARG                      # a short workspace
    magic, ver, n_names, n_iv, o_names, o_st, o_en, o_by, total, n_by = struct.unpack_from("<10I", table)

    def corrupt(off, fmt, value):
        t = bytearray(table)
        struct.pack_into(fmt, t, off, value)
        return bytes(t)
    bad = {"magic": corrupt(0, "<I", 0x12345678), "version": corrupt(4, "<I", 2),
           "names past the end": corrupt(8, "<I", 1 << 20), "intervals past the end": corrupt(12, "<I", 1 << 24),
           "offset past the end": corrupt(20, "<I", total), "odd offset": corrupt(20, "<I", o_st + 4),
           "bytes offset past the end": corrupt(28, "<I", total + 8), "size": corrupt(32, "<I", total + 8),
           "name bytes past the end": corrupt(o_names + 16 + 4, "<I", n_by + 1),
           "interval range past the end": corrupt(o_names + 16 + 12, "<I", n_iv + 1),
           "unsorted names": corrupt(o_names + 4, "<I", 4),
           "unsorted starts": corrupt(o_st + 8, "<Q", 0),
           "start past end": corrupt(o_en, "<Q", 0),
           "truncated": bytes(table[:-8]), "header only": bytes(table[:40]), "empty": b""}
    for why, t in bad.items():
        assert upload(t)[0] == E_ARG, why
    data = SC.query_files(1)[0][1]   # the host entries refuse such a table too
    out = np.zeros(64, dtype=np.uint8)
    n = ctypes.c_uint64(0)
    t = bad["unsorted starts"]
    assert lib().emu_regions_query(data, len(data), t, len(t), out.ctypes.data, 64, ctypes.byref(n), 1 << 12) == E_ARG


# ---- flags and error word ------------------------------------------------------------

def test_sets_on_query_files():
    RC.check_sets(flags, build, 1)


def test_invariant_or_of_single_region_flags():
    RC.check_invariant(flags, single, build, 1)


def test_table_shapes_and_record_counts():
    RC.check_shapes(flags, build)


# ---- the three drivers ------------------------------------------------------------------

def test_drivers():
    assert RC.check_drivers(emu_qry, emu_qsam, emu_cnt, 1) == (8, 16)


def test_drivers_small_batches_and_arguments():
    name, data = SC.query_files(1)[0]
    regions = RC.parse_text(RC.SETS["A"])
    assert emu_qry(data, RC.SETS["A"], out_batch=64) == RC.query_regions(data, regions)
    assert emu_qsam(data, RC.SETS["A"], [3, 1], out_batch=16) == RC.query_samples_regions(data, regions, [3, 1])
    assert emu_cnt(data, RC.SETS["A"], rec_batch=7) == RC.counts_regions(data, regions)
    for cols in ([], [40], [2, 2]):
        assert emu_qsam(data, RC.SETS["A"], cols) == (E_ARG, b"")
    assert emu_qry(data[1:], RC.SETS["A"]) == (E_FORMAT, b"")
    # an empty set matches nothing and is no error; a file without records neither
    assert emu_qry(data, b"") == (OK, b"") and emu_cnt(data, b"# none\n")[:3] == (OK, [], [])
    hdr = data[:SC.parse_header(data)[0]]
    assert emu_qry(hdr + b"x", RC.SETS["B"]) == (OK, b"") and emu_qry(hdr + b"x" * 8, RC.SETS["B"]) == (E_FORMAT, b"")


def test_driver_reproduces_the_reference_cli():
    g = RC.golden()
    data = G.gz(g["file"])
    st, out = emu_qry(data, g["regions"].encode(), out_batch=1 << 20)
    assert st == OK and out.count(b"\n") == g["union_lines"] and hashlib.sha256(out).hexdigest() == g["union_sha256"]
