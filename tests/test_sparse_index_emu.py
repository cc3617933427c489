"""Sparse external index on the CPU: the Python restatement
(sparse_index_cases.py) against the reference CLI's recorded results
(tests/golden/sparse_index_cases.json), then the product kernels
(csrc/vcfc_sparse_index.hip) and host drivers
(csrc/vcfc_sparse_index_driver.h) compiled against the fiber SIMT emulator,
against the goldens and the restatement, and the hand-built edge families of
index_edge_cases.py.  test_gpu_sparse_index.py repeats the generated inputs
and the edge families on the GPU."""
import ctypes
import struct

import numpy as np
import pytest

import emu_io as E
import golden_io as G
import index_cases as X
import index_edge_cases as EC
import sparse_index_cases as SX

OK, E_FORMAT = 0, 8
NO_ERROR = (1 << 64) - 1
_lib = None


def lib():
    """The emulator build of the sparse-index kernels and drivers (flags as tests/simt_emu/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    L = E.build_emu_lib("sparse_index", ("vcfc_sparse_index.hip", "vcfc_index.hip", "vcfc_decode.hip",
                        "vcfc_encode.hip"), "emu_sparse_index_api.cpp")
    vp, u64, cp = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p
    pu64, pint = ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_int)
    L.emu_spx_create.argtypes = [cp, u64, u64, vp, vp, u64, vp, ctypes.POINTER(ctypes.c_int64), pint]
    L.emu_spx_query.argtypes = [cp, u64, vp, vp, u64, u64, cp, u64, ctypes.c_int, u64, u64, vp, u64, pu64, u64, u64, vp,
                                u64, pu64, vp]
    L.emu_spx_device.argtypes = [cp, vp, u64, u64, vp, vp, vp]
    L.emu_spx_span.argtypes = [cp, vp, u64, ctypes.c_int, vp, vp, vp]
    L.emu_spx_gap.argtypes = [cp, u64, vp, u64, pu64, ctypes.POINTER(ctypes.c_int64)]
    _lib = L
    return L


def emu_create(data, limit=1 << 63):
    """(status, slots, failing record, seek_failed, info) with info =
    {size, pwrites, in_order, entries}."""
    cap = len(data) // 12 + 1
    so, se = np.zeros(cap, dtype=np.uint64), np.zeros(13 * cap, dtype=np.uint8)
    info = np.zeros(5, dtype=np.uint64)
    er, sf = ctypes.c_int64(-1), ctypes.c_int(0)
    st = lib().emu_spx_create(data, len(data), limit, so.ctypes.data, se.ctypes.data, cap, info.ctypes.data,
                              ctypes.byref(er), ctypes.byref(sf))
    k = int(info[0])
    slots = {int(so[j]): se[13 * j:13 * j + 13].tobytes() for j in range(k)}
    return st, slots, er.value, sf.value, {"size": int(info[1]), "pwrites": int(info[2]), "in_order": int(info[3]),
                                           "entries": int(info[4])}


def emu_query(data, slots, q, size=None, window=1 << 16, out_batch=1 << 14, log=None, idx_io=None):
    name, hr, a, b = G.oracle_parse_query(q.encode() if isinstance(q, str) else q)
    cap = len(data) * 40 + 4096
    out = np.zeros(cap, dtype=np.uint8)
    n, ln = ctypes.c_uint64(0), ctypes.c_uint64(0)
    lg = np.zeros(2 * 4096, dtype=np.uint64)
    io = np.zeros(2, dtype=np.uint64)
    offs = sorted(slots)
    so = np.array(offs, dtype=np.uint64)
    se = np.frombuffer(b"".join(slots[o] for o in offs) + b"\0", dtype=np.uint8).copy()
    size = SX.apparent_size(slots) if size is None else size
    st = lib().emu_spx_query(data, len(data), so.ctypes.data, se.ctypes.data, len(offs), size, name, len(name), int(hr),
                             a, b, out.ctypes.data, cap, ctypes.byref(n), window, out_batch, lg.ctypes.data, 4096,
                             ctypes.byref(ln), io.ctypes.data)
    if log is not None:
        assert ln.value <= 4096
        log.extend((int(lg[2 * i]), int(lg[2 * i + 1])) for i in range(ln.value))
    if idx_io is not None:
        idx_io.extend(int(x) for x in io)
    return st, out[:n.value].tobytes()


def emu_gap(data):
    cap = 64 * (len(data) // 12 + 1)
    out = np.zeros(cap, dtype=np.uint8)
    n, er = ctypes.c_uint64(0), ctypes.c_int64(-1)
    st = lib().emu_spx_gap(data, len(data), out.ctypes.data, cap, ctypes.byref(n), ctypes.byref(er))
    return st, out[:n.value].tobytes(), er.value


def rec_offsets(v):
    """(header end, record offsets relative to it, + end) of a well-formed .vcfc."""
    h = X.header_end(v)
    ro, p = [], h
    while p < len(v):
        ro.append(p - h)
        p += X.record_at(v, p)
    ro.append(p - h)
    return h, ro


def emu_device(v):
    """words {err, count, status[0..2]}, the kept entries and their offsets."""
    h, ro = rec_offsets(v)
    n = len(ro) - 1
    r = np.array(ro, dtype=np.uint64)
    ent = np.full(13 * n + 16, 0xEE, dtype=np.uint8)
    fo = np.full(n + 2, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    words = np.zeros(5, dtype=np.uint64)
    assert lib().emu_spx_device(v[h:], r.ctypes.data, n, h, ent.ctypes.data, fo.ctypes.data, words.ctypes.data) == 0
    cnt = int(words[1])
    assert cnt <= n and (ent[13 * cnt:] == 0xEE).all() and (fo[cnt:] == 0xEEEEEEEEEEEEEEEE).all()
    return [int(w) for w in words], ent[:13 * cnt].tobytes(), fo[:cnt].tolist()


def emu_span(v, walk):
    h, ro = rec_offsets(v)
    n = len(ro) - 1
    r = np.array(ro, dtype=np.uint64)
    ref, pos = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    err = np.zeros(1, np.uint64)
    assert lib().emu_spx_span(v[h:], r.ctypes.data, n, walk, ref.ctypes.data, pos.ctypes.data, err.ctypes.data) == 0
    return int(err[0]), ref.tolist(), pos.tolist()


def fields_of(v, walk):
    """[(ref_idx, pos)] by the restatement (well-formed files)."""
    h, ro = rec_offsets(v)
    f = SX.walk_fields if walk else SX.create_fields
    return [f(v[h + ro[i]:h + ro[i + 1]]) for i in range(len(ro) - 1)]


def kept(v):
    """The kept entries and offsets the device pass must give for a file whose offsets never decrease."""
    h, ro = rec_offsets(v)
    fl = fields_of(v, 0)
    ent, off = [], []
    for i, (ref, pos) in enumerate(fl):
        o = SX.slot_offset(pos)
        if i + 1 == len(fl) or SX.slot_offset(fl[i + 1][1]) != o:
            ent.append(SX.entry(ref, pos, h + ro[i]))
            off.append(o)
    return b"".join(ent), off


# ---- the restatement against the reference ---------------------------------------

def test_restatement_matches_reference_create_cases():
    n = 0
    for c in SX.cases()["create_cases"]:
        st, slots, bad, sf = SX.create(SX.file_bytes(c["file"]))
        assert SX.check_create_case(c, slots, SX.apparent_size(slots)), c["file"]
        assert (st == OK) == (c["rc"] == 0), c["file"]
        assert sf == (1 if c.get("stderr") == "lseek: Invalid argument\n" else 0), c["file"]
        n += 1
    assert n == 10
    by = {c["file"]: c for c in SX.cases()["create_cases"]}
    assert by["header_only"]["size"] == 0 and by["seek_fails"]["n_slots"] == 2 and by["throw_kvp"]["n_slots"] == 10
    assert SX.create(SX.file_bytes("throw_pos"))[2] == 10 and SX.create(SX.file_bytes("header_only"))[2] == -1
    assert by["multi_chrom"]["n_slots"] == 10 and by["unsorted"]["n_slots"] == 4   # shared slots: the last record wins


def test_restatement_matches_reference_query_cases():
    n = 0
    for c in SX.cases()["query_cases"]:
        v = SX.file_bytes(c["file"])
        slots = SX.create(v)[1]
        if not slots:   # the header-only index: the SEEK_DATA probe fails
            assert c["stderr"] == "fseek: No such device or address\n"
        st, out = SX.query(v, slots, c["region"])
        assert X.check_query_case(c, st, out), (c, st, len(out))
        n += 1
    assert n >= 70


def test_restatement_matches_reference_gap_cases():
    n = 0
    for c in SX.cases()["gap_cases"]:
        st, txt, bad = SX.gap_analysis(SX.file_bytes(c["file"]))
        assert (st == OK) == (c["rc"] == 0) and len(txt) == c["txt_len"] and X.sha(txt) == c["txt_sha256"], c["file"]
        assert "txt" not in c or txt.decode() == c["txt"]
        n += 1
    assert n == 10


# ---- the product kernels and drivers on the emulator --------------------------

def test_emu_golden_gap_cases():
    for c in SX.cases()["gap_cases"]:
        v = SX.file_bytes(c["file"])
        st, txt, bad = emu_gap(v)
        assert (st == OK) == (c["rc"] == 0) and len(txt) == c["txt_len"] and X.sha(txt) == c["txt_sha256"], c["file"]
        assert (st, txt, bad) == SX.gap_analysis(v)


def test_emu_gap_uncompressed_last_column():
    """Where the last sample column is an uncompressed one its LF is counted:
    the count equals the record's size in the file, else it is one less; a
    POS with a blank is written verbatim; a record the decoder refuses ends
    the text after the lines before it."""
    rows = [b"1\t7\t.\tA\tC\t1\tPASS\t.\tGT\t0|1\t0|0\t0/1", b"1\t 9\t.\tA\tC\t1\tPASS\t.\tGT\t0|1\t./.\t1|1",
            b"2\t12\t.\tA\tC\t1\tPASS\t.\tGT\t0/0\t0/1\t1/1", b"2\t15\t.\tA\tC\t1\tPASS\t.\tGT\t0|0\t0|0\t0|0"]
    st, v, _ = G.oracle_compress(X.header(3) + b"".join(r + b"\n" for r in rows))
    assert st == 0
    h, ro = rec_offsets(v)
    want = SX.gap_analysis(v)
    sizes = [ro[i + 1] - ro[i] for i in range(4)]
    assert want[1] == b"".join(b"%s %d %d\n" % (r.split(b"\t")[1], len(r) + 1, sizes[i] - (0 if i in (0, 2) else 1))
                               for i, r in enumerate(rows))
    assert emu_gap(v) == want
    cut = bytearray(v)
    cut[h + ro[2] + 4] ^= 0x40   # the REQ header's extension bits: record 2 is refused
    got = emu_gap(bytes(cut))
    assert got[0] == E_FORMAT and got[2] == 2 and got[1] == want[1][:len(b"".join(want[1].split(b"\n")[:2])) + 2]


@pytest.mark.parametrize("n", [1, 64, 257, 4097])
def test_emu_gap_generated_records(n):
    v = SX.gen_vcfc(n, 500 + n)
    want = SX.gap_analysis(v)
    assert want[0] == OK and want[1].count(b"\n") == n
    assert emu_gap(v) == want

def test_emu_golden_create_cases():
    for c in SX.cases()["create_cases"]:
        v = SX.file_bytes(c["file"])
        st, slots, bad, sf, info = emu_create(v)
        assert SX.check_create_case(c, slots, info["size"]), (c["file"], len(slots), info)
        assert (st, slots, bad, sf) == SX.create(v), c["file"]
        assert (st == OK) == (c["rc"] == 0)


def test_emu_golden_query_cases():
    for c in SX.cases()["query_cases"]:
        v = SX.file_bytes(c["file"])
        slots = SX.create(v)[1]
        st, out = emu_query(v, slots, c["region"])
        assert X.check_query_case(c, st, out), (c, st, len(out))
        assert (st, out) == SX.query(v, slots, c["region"])


# equal POS pairs across the wave (63/64) and block (255/256) boundaries, and inside a wave
PAIRS = {1: (), 2: (0,), 63: (5,), 64: (62,), 65: (63,), 255: (63, 100), 256: (63, 254), 257: (63, 255),
         4097: (63, 255, 256, 4095)}


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_emu_generated_records(n):
    v = SX.gen_vcfc(n, 300 + n, pairs=PAIRS[n])
    for walk in (0, 1):
        err, ref, pos = emu_span(v, walk)
        assert err == NO_ERROR and list(zip(ref, pos)) == fields_of(v, walk)
    words, ent, off = emu_device(v)
    want_ent, want_off = kept(v)
    assert words == [NO_ERROR, n - len(PAIRS[n]), 0, 0, NO_ERROR]
    assert (ent, off) == (want_ent, want_off)
    want = SX.create(v)
    st, slots, bad, sf, info = emu_create(v)
    assert (st, slots, bad, sf) == want and info["size"] == SX.apparent_size(want[1])
    assert info["in_order"] == 0 and info["entries"] == n - len(PAIRS[n]) and info["pwrites"] <= info["entries"]
    if n >= 63:   # POS steps of 1 and 2 put several slots in one 4 KiB block
        assert info["pwrites"] < info["entries"]
    for q in ("1:%d-%d" % (p, p + 30) for p in (1, 60, 90, 10**6)):
        assert emu_query(v, slots, q) == SX.query(v, slots, q)


def test_restatement_matches_reference_edge_cases():
    EC.check_pinned_sparse()


def _create(v):
    st, slots, bad, sf, info = emu_create(v)
    return st, slots, bad, sf, info["size"]


class EMU:
    """The callables index_edge_cases.py checks, on the emulator."""
    device = staticmethod(emu_device)
    create = staticmethod(_create)
    query = staticmethod(emu_query)
    span = staticmethod(emu_span)
    gap = staticmethod(emu_gap)


def test_emu_unsorted_falls_back_to_record_order():
    EC.check_unsorted(EMU)
    st, slots, bad, sf, info = emu_create(SX.gen_vcfc(300, 17, pairs=(63, 255), unsorted=True))
    assert info["in_order"] == 1 and info["pwrites"] == 300
    assert emu_create(SX.file_bytes("unsorted"))[4]["in_order"] == 1


@pytest.mark.parametrize("family", sorted(EC.SPARSE))
def test_emu_edge_family(family):
    EC.SPARSE[family](EMU)


def test_emu_no_records():
    words = np.zeros(5, dtype=np.uint64)
    r = np.zeros(1, dtype=np.uint64)
    ent, fo = np.zeros(16, dtype=np.uint8), np.zeros(2, dtype=np.uint64)
    assert lib().emu_spx_device(b"", r.ctypes.data, 0, 0, ent.ctypes.data, fo.ctypes.data, words.ctypes.data) == 0
    assert [int(w) for w in words] == [NO_ERROR, 0, 0, 0, NO_ERROR]
    st, slots, bad, sf, info = emu_create(X.header(2))   # no data line: the header parse throws
    assert (st, slots, bad, sf, info["size"]) == (E_FORMAT, {}, -1, 0, 0)


def test_emu_short_and_structural_records():
    EC.check_short_and_structural(EMU)


def test_emu_refused_offset_stops_the_run():
    """A file system that refuses offsets from `limit` on: the reference's
    lseek fails at the first such record, earlier entries stay."""
    v = SX.gen_vcfc(200, 5)
    pos = [p for _, p in fields_of(v, 0)]
    limit = SX.slot_offset(pos[120]) & ~4095   # (a file system's limit is a multiple of its block size)
    want = SX.create(v, limit=limit)
    assert want[3] == 1 and 100 < len(want[1]) <= 120
    assert emu_create(v, limit=limit)[:4] == want
    u = SX.gen_vcfc(200, 5, unsorted=True)   # record 0 holds the POS of record 100
    limit = SX.slot_offset(pos[50]) & ~4095
    want = SX.create(u, limit=limit)
    assert want[3] == 1 and len(want[1]) == 0
    assert emu_create(u, limit=limit)[:4] == want


def test_emu_lookup_rules():
    v = SX.file_bytes("multi_chrom")
    slots = SX.create(v)[1]
    size = SX.apparent_size(slots)
    assert emu_query(v, {}, "1:100-200", size=0) == (OK, b"")                      # an empty index
    assert emu_query(v, slots, "1:100-200", size=size - 1)[0] == OK                # (a cut last entry is never reached)
    first = SX.slot_offset(100)
    only_last = {max(slots): slots[max(slots)]}
    io = []
    st, out = emu_query(v, only_last, "1:1-2", idx_io=io)                          # across one long hole
    zeros = max(slots) % 4096 // 256   # SEEK_DATA lands on the block's start: its zero slots are stepped over
    assert (st, out) == SX.query(v, only_last, "1:1-2") and io == [2 + zeros, 2 + zeros]
    io = []
    assert emu_query(v, slots, "1:1-1", idx_io=io) == (OK, b"") and io == [1, 1]   # start == end in a hole
    past = {first: SX.entry(1, 100, len(v))}
    assert emu_query(v, past, "1:100-100") == (OK, b"")                            # byte_offset at EOF
    h = X.header_end(v)
    assert emu_query(v, {first: SX.entry(1, 100, h + 3)}, "1:100-100") == (E_FORMAT, b"")   # not a record start
    assert emu_query(v, {first: SX.entry(1, 100, 2)}, "1:100-100")[0] == E_FORMAT           # inside the header
    # zero slots inside a data block are stepped over 256 bytes at a time
    a, b = SX.slot_offset(100), SX.slot_offset(107)
    two = {a: slots[a], b: SX.entry(1, 107, struct.unpack("<BIQ", slots[SX.slot_offset(150)])[2])}
    io = []
    st, out = emu_query(v, two, "1:101-160", idx_io=io)
    assert (st, out) == SX.query(v, two, "1:101-160") and out.count(b"\n") == 1 and io == [8, 8]


@pytest.mark.parametrize("seed", EC.MUTATE_SEEDS)
def test_emu_mutated_files(seed):
    EC.check_mutated_sparse(EMU, seed, window=4096)


def test_mutated_files_floor():
    """Over the seeds the restatement takes at least 5 files whole and refuses at least 5 under each of codes 2 and 3."""
    assert min(EC.mutated_floor(True)) >= 5, EC.mutated_floor(True)


def test_emu_query_reads_only_its_windows():
    """window_bytes = 4096, a region near the end of the 10000-record file:
    the index is touched at the slot of `start` only, and no byte of the .vcfc
    before the entry's byte_offset is read, apart from the header, and at most
    one window past the first record after the query."""
    v = SX.file_bytes("random_100x10000.vcfc.gz")
    slots = SX.create(v)[1]
    q = "1:29000-29010"
    ent = struct.unpack("<BIQ", SX.lookup(slots, 29000, 29010))
    h = X.header_end(v)
    assert ent[2] > h + (len(v) - h) * 9 // 10
    log, io = [], []
    st, out = emu_query(v, slots, q, window=4096, log=log, idx_io=io)
    assert (st, out) == SX.query(v, slots, q) and out.count(b"\n") == 6
    assert io == [1, 1]   # the slot of `start`, and the SEEK_DATA probe
    data_reads = [(o, k) for o, k in log if o != 0]
    assert log and all(o == 0 and o + k <= 1 << 16 for o, k in log if o == 0)   # the header prefix
    assert data_reads and min(o for o, _ in data_reads) == ent[2]
    hh, ro = rec_offsets(v)
    fl = fields_of(v, 1)
    after = min(hh + ro[i] for i, (r, p) in enumerate(fl) if hh + ro[i] >= ent[2] and p > 29010)
    assert all(k <= 4096 for _, k in data_reads)
    assert sum(1 for o, _ in data_reads if o > after) <= 1
    assert max(o + k for o, k in data_reads) <= after + 2 * 4096
    assert sum(k for _, k in data_reads) < (len(v) - h) // 10
