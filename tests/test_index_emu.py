"""Binned external index on the CPU: the Python restatement (index_cases.py)
against the reference CLI's recorded results
(tests/golden/binned_index_cases.json), then the product kernels
(csrc/vcfc_index.hip) and host drivers (csrc/vcfc_index_driver.h) compiled
against the fiber SIMT emulator, against the goldens and the restatement, and
the hand-built edge families of index_edge_cases.py.  test_gpu_index.py
repeats the generated inputs and the edge families on the GPU."""
import ctypes
import random

import numpy as np
import pytest

import emu_io
import golden_io as G
import index_cases as X
import index_edge_cases as EC

OK, E_ARG, E_FORMAT = 0, 5, 8
NO_ERROR = (1 << 64) - 1
_lib = None


def lib():
    """The emulator build of the index kernels and drivers (flags as tests/simt_emu/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    L = emu_io.build_emu_lib("index", ("vcfc_index.hip", "vcfc_decode.hip", "vcfc_encode.hip"), "emu_index_api.cpp")
    vp, u64, cp = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p
    pu64 = ctypes.POINTER(u64)
    L.emu_index_create.argtypes = [cp, u64, u64, vp, u64, pu64, ctypes.POINTER(ctypes.c_int64)]
    L.emu_index_query.argtypes = [cp, u64, cp, u64, cp, u64, ctypes.c_int, u64, u64, vp, u64, pu64, u64, u64, vp, u64,
                                  pu64]
    L.emu_index_device.argtypes = [cp, vp, u64, u64, u64, vp, u64, vp]
    L.emu_record_span.argtypes = [cp, vp, u64, vp, vp, vp, vp]
    L.emu_index_compare.argtypes = [vp, vp, vp, u64, ctypes.c_uint32, u64, u64, vp, vp]
    _lib = L
    return L


def emu_create(data, E):
    cap = 13 * (len(data) // 12 + 1)
    out = np.zeros(cap, dtype=np.uint8)
    n, er = ctypes.c_uint64(0), ctypes.c_int64(-1)
    st = lib().emu_index_create(data, len(data), E, out.ctypes.data, cap, ctypes.byref(n), ctypes.byref(er))
    return st, out[:n.value].tobytes(), er.value


def emu_query(data, index, q, window=1 << 16, out_batch=1 << 14, log=None):
    name, hr, a, b = G.oracle_parse_query(q.encode() if isinstance(q, str) else q)
    cap = len(data) * 40 + 4096
    out = np.zeros(cap, dtype=np.uint8)
    n, ln = ctypes.c_uint64(0), ctypes.c_uint64(0)
    lg = np.zeros(2 * 4096, dtype=np.uint64)
    st = lib().emu_index_query(data, len(data), index, len(index), name, len(name), int(hr), a, b, out.ctypes.data, cap,
                               ctypes.byref(n), window, out_batch, lg.ctypes.data, 4096, ctypes.byref(ln))
    if log is not None:
        assert ln.value <= 4096
        log.extend((int(lg[2 * i]), int(lg[2 * i + 1])) for i in range(ln.value))
    return st, out[:n.value].tobytes()


def rec_offsets(v):
    """(header end, record offsets relative to it, + end) of a well-formed .vcfc."""
    h = X.header_end(v)
    ro, p = [], h
    while p < len(v):
        ro.append(p - h)
        p += X.record_at(v, p)
    ro.append(p - h)
    return h, ro


def emu_device(v, E, cap=None):
    h, ro = rec_offsets(v)
    n = len(ro) - 1
    r = np.array(ro, dtype=np.uint64)
    cap = n if cap is None else cap
    ent = np.full(13 * max(cap, 1) + 16, 0xEE, dtype=np.uint8)
    words = np.zeros(3, dtype=np.uint64)
    assert lib().emu_index_device(v[h:], r.ctypes.data, n, h, E, ent.ctypes.data, cap, words.ctypes.data) == 0
    assert (ent[13 * cap:] == 0xEE).all(), "entries written past entries_cap"
    return [int(w) for w in words], ent[:13 * min(int(words[1]), cap)].tobytes()


def emu_span(v):
    h, ro = rec_offsets(v)
    n = len(ro) - 1
    r = np.array(ro, dtype=np.uint64)
    ref, pos, end = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    err = np.zeros(1, np.uint64)
    assert lib().emu_record_span(v[h:], r.ctypes.data, n, ref.ctypes.data, pos.ctypes.data, end.ctypes.data,
                                 err.ctypes.data) == 0
    return int(err[0]), ref.tolist(), pos.tolist(), end.tolist()


# ---- the restatement against the reference ---------------------------------------

def test_restatement_matches_reference_index_cases():
    n = 0
    for c in X.cases()["index_cases"]:
        st, idx, bad = X.build_index(X.file_bytes(c["file"]), c["bin"])
        if c["rc"] == 0:
            assert st == OK and len(idx) == c["index_len"] and X.sha(idx) == c["index_sha256"], c["file"]
            if "index_hex" in c:
                assert idx.hex() == c["index_hex"]
            sp, _ = X.spans_of(X.file_bytes(c["file"]))
            assert X.pack(X.parallel_entries(sp, c["bin"])) == idx   # every end < 2^32 here
        else:
            assert st == E_FORMAT and idx == b"" and bad == 10 and c["index_len"] == 0, c
        n += 1
    assert n == 24


def test_restatement_matches_reference_query_cases():
    n = 0
    for c in X.cases()["query_cases"]:
        idx = X.build_index(X.file_bytes(c["index_file"]), c["bin"])[1]
        assert len(idx) >= 26
        st, out = X.query(X.file_bytes(c["file"]), idx, c["region"])
        assert X.check_query_case(c, st, out), (c, st, len(out))
        n += 1
    assert n >= 100
    c = [c for c in X.cases()["query_cases"] if c["region"] == "1:10100-10104" and c["bin"] == 100][0]
    assert c["stdout_len"] > 0 and X.query(X.file_bytes(c["file"]), X.build_index(X.file_bytes(c["file"]), 100)[1],
                                           c["region"])[1].count(b"\n") == 3


# ---- the product kernels and drivers on the emulator --------------------------

def test_emu_golden_index_cases():
    for c in X.cases()["index_cases"]:
        st, idx, bad = emu_create(X.file_bytes(c["file"]), c["bin"])
        if c["rc"] == 0:
            assert st == OK and X.sha(idx) == c["index_sha256"] and len(idx) == c["index_len"], (c["file"], c["bin"])
        else:
            assert st == E_FORMAT and idx == b"" and bad == 10, (c["file"], c["bin"], st, bad)


def test_emu_golden_query_cases():
    built = {}
    for c in X.cases()["query_cases"]:
        key = (c["index_file"], c["bin"])
        if key not in built:
            built[key] = X.build_index(X.file_bytes(c["index_file"]), c["bin"])[1]
        data = X.file_bytes(c["file"])
        st, out = emu_query(data, built[key], c["region"])
        assert X.check_query_case(c, st, out), (c, st, len(out))
        assert (st, out) == X.query(data, built[key], c["region"])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_emu_generated_records(n):
    v = X.gen_vcfc(n, 100 + n)
    sp, bad = X.spans_of(v)
    assert bad is None and len(sp) == n
    err, ref, pos, end = emu_span(v)
    assert err == NO_ERROR
    assert (ref, pos, end) == ([s[1] for s in sp], [s[2] for s in sp], [s[3] for s in sp])
    for E in (1, 3, 64, 1000):
        want = X.build_index(v, E)
        assert emu_create(v, E) == want, (n, E)
        words, ent = emu_device(v, E)
        assert words[0] == NO_ERROR and words[1] == len(want[1]) // 13 and words[2] == max(end) and ent == want[1]
    if n >= 64:   # a short entries_cap: code 0xFF, the count still whole, nothing past the cap
        want = X.build_index(v, 1)[1]
        words, ent = emu_device(v, 1, cap=5)
        assert words[0] & 0xFF == 0xFF and words[1] == len(want) // 13 and ent == want[:13 * 5]


def test_emu_no_records():
    words = np.zeros(3, dtype=np.uint64)
    r = np.zeros(1, dtype=np.uint64)
    ent = np.zeros(16, dtype=np.uint8)
    assert lib().emu_index_device(b"", r.ctypes.data, 0, 0, 3, ent.ctypes.data, 0, words.ctypes.data) == 0
    assert [int(w) for w in words] == [NO_ERROR, 0, 0]
    st, idx, _ = emu_create(X.header(2), 3)   # no data line: the header parse throws
    assert st == E_FORMAT and idx == b""
    assert emu_create(X.gen_vcfc(5, 1), 0)[0] == E_ARG


def test_emu_end_past_2_32_replays_on_the_host():
    v = X.gen_vcfc(300, 9, big_end=True)
    sp, _ = X.spans_of(v)
    assert max(s[3] for s in sp) >= 1 << 32
    differ = False
    for E in (1, 3, 64):
        want = X.build_index(v, E)
        assert emu_create(v, E) == want, E
        differ = differ or X.pack(X.parallel_entries(sp, E)) != want[1]
        words, _ = emu_device(v, E)
        assert words[2] == max(s[3] for s in sp)
    assert differ   # the parallel form alone would be wrong here


def test_restatement_matches_reference_edge_cases():
    EC.check_pinned_binned()


class EMU:
    """The callables index_edge_cases.py checks, on the emulator."""
    span = staticmethod(emu_span)
    device = staticmethod(lambda v, E, cap: emu_device(v, E, cap))
    create = staticmethod(emu_create)
    query = staticmethod(emu_query)


def test_emu_odd_fields():
    EC.check_odd_fields(EMU)


@pytest.mark.parametrize("family", sorted(EC.BINNED))
def test_emu_edge_family(family):
    EC.BINNED[family](EMU)


@pytest.mark.parametrize("n", EC.NS)
def test_emu_edge_prefix_max(n):
    EC.binned_prefix_max(EMU, n)


def test_emu_index_edge_rules():
    v = X.file_bytes("index_edge")
    good = X.build_index(v, 1)[1]
    assert emu_query(v, good[:-1], "1:100-200")[0] == E_FORMAT            # not a multiple of 13
    assert emu_query(v, b"", "1:100-200") == (OK, b"")                     # no entries
    one = good[:13]
    assert emu_query(v, one, "1:100-200") == X.query(v, one, "1:100-200")  # one entry: entry 0
    assert emu_query(v, one, "1:100-200")[1].count(b"\n") > 0
    past = X.pack([(1, 100, len(v)), (1, 200, len(v) + 50)])
    assert emu_query(v, past, "1:100-200") == (OK, b"")                     # byte_offset at / past EOF
    h = X.header_end(v)
    mid = X.pack([(1, 0, h + 3), (1, 0, h + 3)])
    assert emu_query(v, mid, "1:100-200") == (E_FORMAT, b"")                # not a record start
    assert emu_query(v, X.pack([(1, 0, 2), (1, 0, 2)]), "1:100-200")[0] == E_FORMAT   # inside the header


@pytest.mark.parametrize("seed", EC.MUTATE_SEEDS)
def test_emu_mutated_files(seed):
    EC.check_mutated_binned(EMU, seed, window=4096)


def test_mutated_files_floor():
    """Over the seeds the restatement takes at least 5 files whole and refuses at least 5 under each of codes 2 and 3."""
    assert min(EC.mutated_floor(False)) >= 5, EC.mutated_floor(False)


def test_emu_query_reads_only_its_windows():
    """window_bytes = 4096, a region near the end of the 10000-record file at
    bin 100: no byte before the chosen entry's byte_offset is read, apart from
    the header, and at most one window past the first record after the query."""
    v = X.file_bytes("random_100x10000.vcfc.gz")
    idx = X.build_index(v, 100)[1]
    q = "1:29000-29010"
    ent, _ = X.search(idx, 1, 29000)
    h = X.header_end(v)
    assert ent[2] > h + (len(v) - h) * 9 // 10
    log = []
    st, out = emu_query(v, idx, q, window=4096, log=log)
    assert (st, out) == X.query(v, idx, q) and out.count(b"\n") == 6
    data_reads = [(o, k) for o, k in log if o != 0]
    assert log and all(o == 0 and o + k <= 1 << 16 for o, k in log if o == 0)   # the header prefix
    assert data_reads and min(o for o, _ in data_reads) == ent[2]
    # the first record after the query
    sp, _ = X.spans_of(v)
    after = min(o for o, r, pos, end in sp if o >= ent[2] and pos > 29010)
    assert all(k <= 4096 for _, k in data_reads)
    assert sum(1 for o, _ in data_reads if o > after) <= 1
    assert max(o + k for o, k in data_reads) <= after + 2 * 4096
    assert sum(k for _, k in data_reads) < (len(v) - h) // 10


def test_emu_compare_kernel():
    rnd = random.Random(5)
    n = 700
    ref = np.array([rnd.choice([0, 1, 2, 23]) for _ in range(n)], dtype=np.uint8)
    pos = np.array([rnd.randrange(1000) for _ in range(n)], dtype=np.uint64)
    end = pos + np.array([rnd.randrange(50) for _ in range(n)], dtype=np.uint64)
    for qidx, a, b in ((1, 100, 300), (0, 0, 0), (2, 990, 2000), (25, 0, 5), (1, 500, 100)):
        flag = np.zeros(n, dtype=np.uint8)
        fa = np.zeros(1, dtype=np.uint64)
        assert lib().emu_index_compare(ref.ctypes.data, pos.ctypes.data, end.ctypes.data, n, qidx, a, b,
                                       flag.ctypes.data, fa.ctypes.data) == 0
        want, first = [], NO_ERROR
        for i in range(n):
            before = ref[i] < qidx or (ref[i] == qidx and end[i] < a)
            aft = not before and (ref[i] > qidx or (ref[i] == qidx and pos[i] > b))
            want.append(int(not before and not aft))
            if aft and first == NO_ERROR:
                first = i
        assert flag.tolist() == want and int(fa[0]) == first
