"""The device entries on records that lie around byte offsets 2^31 and 2^32
(far_cases.py) on the CPU: the product kernels and host code
compiled against the fiber SIMT emulator, on a lazily mapped arena of
FAR + SLACK bytes of which only the pages written are touched.  From 2 GiB up
the emulator's entries read the caller's memory in place
(tests/simt_emu/host_buffers.h HostInput).  test_gpu_far.py repeats every
check on the GPU.  Where a suite's own helper takes (body, rec) it is used as
it is, with the arena's base for the body."""
import ctypes

import numpy as np
import pytest

import emu_io as E
import far_cases as F
import test_counts_emu as TC
import test_extract_emu as TX
import test_index_emu as TI
import test_ld_emu as TL
import test_matrix_emu as TM
import test_regions_emu as TR
import test_sparse_index_emu as TSX
import test_subset_emu as TS
from test_record_hash import py_hash64

OK = 0


@pytest.fixture(scope="module")
def arena():
    return F.host_arena()


def base(P):
    """The arena's base as the `recs` argument (a char pointer to ctypes)."""
    return ctypes.cast(P.ptr, ctypes.c_char_p)


def u64s(x):
    return np.array(x, dtype=np.uint64)


def sel_of(select):
    return None if select is None else np.array(select, dtype=np.uint8)


def ptr(a):
    return None if a is None else a.ctypes.data


def test_builder_assertions():
    F.check_builder()
    # the arena is lazy: two pages written 4 GiB apart read back
    a = F.host_arena()
    a.write(F.FAR + F.SLACK - 3, b"far")
    assert a.read(F.FAR + F.SLACK - 3, 3) == b"far"


# ---- matching ---------------------------------------------------------------------

def test_query_match(arena):
    def match(P, q):
        flags, err = TR.single(base(P), P.rec, q)
        return OK, err, flags
    F.check_match(arena, match)


def test_regions_match(arena):
    def regions(P, text):
        flags, err = TR.flags(base(P), P.rec, TR.build(text))
        return OK, err, flags
    F.check_regions(arena, regions)


# ---- decode -------------------------------------------------------------------------

def test_decode_sizes(arena):
    L = TSX.lib()
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.emu_decode_sizes.argtypes = [ctypes.c_char_p, u64, vp, u64, u64, vp, vp, vp, vp, vp]

    def sizes(P):
        r = u64s(P.rec)
        lo, po, cc = (np.full(P.n + 1, 0xEE, dtype=np.uint64) for _ in range(3))
        pl = np.full(P.n + 1, 0xEE, dtype=np.uint32)
        err = np.zeros(1, dtype=np.uint64)
        st = L.emu_decode_sizes(base(P), P.in_bytes, r.ctypes.data, P.n, P.S, lo.ctypes.data, po.ctypes.data,
                                pl.ctypes.data, cc.ctypes.data, err.ctypes.data)
        return st, int(err[0]), lo.tolist(), po[:P.n].tolist(), pl[:P.n].tolist(), cc[:P.n].tolist()
    F.check_sizes(arena, sizes)


def test_decode_records_and_selected(arena):
    L = E.lib()
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.emu_decode_device.argtypes = [ctypes.c_char_p, u64, vp, vp, u64, u64, vp, u64, vp, vp, ctypes.c_int]

    def decode(P, select, exact):
        r = u64s(P.rec)
        sel = sel_of(select)
        cap = 8 * len(P.f.body) + 4 * P.S * P.n + 4096
        out = np.full(cap + 64, 0xEE, dtype=np.uint8)
        lo = np.zeros(P.n + 1, dtype=np.uint64)
        err = np.zeros(1, dtype=np.uint64)
        st = L.emu_decode_device(base(P), P.in_bytes, r.ctypes.data, ptr(sel), P.n, P.S, out.ctypes.data,
                                 cap, lo.ctypes.data, err.ctypes.data, int(exact))
        assert (out[cap:] == 0xEE).all(), "bytes written past out_cap"
        ok = int(err[0]) == F.NO_ERROR
        return st, int(err[0]), lo.tolist() if ok else [], out[:int(lo[P.n])].tobytes() if ok else b""
    F.check_decode(arena, decode)


# ---- the readers ------------------------------------------------------------------------

def test_decode_samples(arena):
    L = TS.lib()

    def subset(P, cols, select):
        r = u64s(P.rec)
        sel = sel_of(select)
        c = np.array(cols, dtype=np.uint32)
        cap = 8 * len(P.f.body) + 4 * P.S * P.n + 64
        out = np.full(cap + 64, 0xEE, dtype=np.uint8)
        lo = np.zeros(P.n + 1, dtype=np.uint64)
        err = np.zeros(1, dtype=np.uint64)
        st = L.emu_subset_device(base(P), r.ctypes.data, ptr(sel), P.n, P.S, c.ctypes.data, len(cols),
                                 out.ctypes.data, cap, lo.ctypes.data, err.ctypes.data)
        assert (out[cap:] == 0xEE).all(), "bytes written past out_cap"
        return st, int(err[0]), lo.tolist(), out[:int(lo[P.n])].tobytes()
    F.check_subset(arena, subset)


def test_genotype_counts(arena):
    def counts(P, select):
        st, err, rows, tab = TC.emu_device_records(base(P), u64s(P.rec), P.S, sel_of(select), True, True, 1)
        return st, err, rows.tolist(), tab.tolist()
    F.check_counts(arena, counts)


def test_genotype_matrix(arena):
    F.check_matrix(arena, lambda P, layout, select, stride, cap, alloc:
                   TM.emu_device(base(P), P.rec, P.S, layout, select, stride, cap, alloc))


def test_extract_samples(arena):
    L = TX.lib()

    def extract(P, cols, select):
        r = u64s(P.rec)
        sel = sel_of(select)
        c = None if cols is None else np.array(cols, dtype=np.uint32)
        cap = L.emu_extract_bound(len(P.f.body), P.n, P.S if cols is None else len(cols))
        out = np.full(cap + 64, 0xEE, dtype=np.uint8)
        ro = np.zeros(P.n + 1, dtype=np.uint64)
        err = np.zeros(1, dtype=np.uint64)
        st = L.emu_extract_device(base(P), r.ctypes.data, ptr(sel), P.n, P.S, ptr(c),
                                  0 if cols is None else len(cols), out.ctypes.data, cap, ro.ctypes.data, err.ctypes.data)
        assert (out[cap:] == 0xEE).all(), "bytes written past out_cap"
        return st, int(err[0]), ro.tolist(), out[:int(ro[P.n])].tobytes()
    F.check_extract(arena, extract)


def test_ld_window(arena):
    F.check_ld_window(arena, lambda P, W, select, cap, slots: TL.emu_window(base(P), P.rec, P.S, W, select, cap, slots))


# ---- the indexes --------------------------------------------------------------------------

def test_binned_index(arena):
    L = TI.lib()

    def binned(P, base_offset, Eb):
        r = u64s(P.rec)
        ent = np.full(13 * P.n + 16, 0xEE, dtype=np.uint8)
        words = np.zeros(3, dtype=np.uint64)
        assert L.emu_index_device(base(P), r.ctypes.data, P.n, base_offset, Eb, ent.ctypes.data, P.n,
                                  words.ctypes.data) == 0
        assert (ent[13 * int(words[1]):] == 0xEE).all(), "entries written past the count"
        return [int(w) for w in words], ent[:13 * int(words[1])].tobytes()
    F.check_binned(arena, binned)


def test_record_span(arena):
    L = TI.lib()

    def span(P):
        r = u64s(P.rec)
        ref, pos, end = np.zeros(P.n, np.uint8), np.zeros(P.n, np.uint64), np.zeros(P.n, np.uint64)
        err = np.zeros(1, np.uint64)
        assert L.emu_record_span(base(P), r.ctypes.data, P.n, ref.ctypes.data, pos.ctypes.data, end.ctypes.data,
                                 err.ctypes.data) == 0
        return int(err[0]), ref.tolist(), pos.tolist(), end.tolist()
    F.check_span(arena, span)


def test_sparse_index(arena):
    L = TSX.lib()

    def spx(P, base_offset):
        r = u64s(P.rec)
        ent = np.full(13 * P.n + 16, 0xEE, dtype=np.uint8)
        fo = np.full(P.n + 2, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
        words = np.zeros(5, dtype=np.uint64)
        assert L.emu_spx_device(base(P), r.ctypes.data, P.n, base_offset, ent.ctypes.data, fo.ctypes.data,
                                words.ctypes.data) == 0
        cnt = int(words[1])
        assert cnt <= P.n and (ent[13 * cnt:] == 0xEE).all() and (fo[cnt:] == 0xEEEEEEEEEEEEEEEE).all()
        return [int(w) for w in words], ent[:13 * cnt].tobytes(), fo[:cnt].tolist()
    F.check_sparse_index(arena, spx)


def test_sparse_plan(arena):
    def splan(P, data_start):
        r = u64s(P.rec)
        fo = np.full(P.n, 0xEE, dtype=np.uint64)
        pf = np.full(16 * P.n, 0xEE, dtype=np.uint8)
        st = np.full(2, 0xEE, dtype=np.uint64)
        E.lib().emu_sparse_plan(P.ptr, r.ctypes.data, P.n, data_start, fo.ctypes.data, pf.ctypes.data, st.ctypes.data)
        return fo.tolist(), pf.tobytes(), st.tolist()
    F.check_sparse_plan(arena, splan)


# ---- the digest and the encoder's input -----------------------------------------------------

def test_record_hash(arena):
    def rhash(P):
        r = u64s(P.rec)
        out = np.zeros(P.n, dtype=np.uint64)
        assert E.lib().emu_record_hash(P.ptr, r.ctypes.data, P.n, out.ctypes.data) == 0
        return out.tolist()
    F.check_record_hash(arena, rhash, py_hash64)


def emu_encode_at(ptr_, offs, lens):
    n = len(offs)
    cap = sum(x * 3 // 2 + 32 for x in lens) + 64
    out = np.full(cap + 64, 0xEE, dtype=np.uint8)
    ro = np.zeros(n + 1, dtype=np.uint64)
    err, sw, rt = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    lo, ll = u64s(offs), np.array(lens, dtype=np.uint32)
    st = E.lib().emu_encode_rows(ptr_, lo.ctypes.data, ll.ctypes.data, n, out.ctypes.data,
                                 cap, ro.ctypes.data, ctypes.byref(err), ctypes.byref(sw), ctypes.byref(rt))
    assert st == 0 and (out[cap:] == 0xEE).all()
    return err.value, ro.tolist(), out[:int(ro[n])].tobytes()


@pytest.mark.parametrize("name", [b[0] for b in F.encode_batches()])
def test_encode_rows(arena, name):
    F.check_encode(arena, emu_encode_at, (name,))
    if name == "gdg_batch":
        assert E.last_deferred() > 0, "the GT:DP:GQ rows were not deferred"


# ---- strides ----------------------------------------------------------------------------------

def test_matrix_row_stride_above_2_30():
    """(the output, 5 GiB + 80 bytes, is a lazy mapping as the arena is)"""
    import mmap
    L = TM.lib()
    m = mmap.mmap(-1, F.STRIDE_ROWS * F.MATRIX_STRIDE, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | 0x4000)
    out = np.frombuffer(m, dtype=np.uint8)

    def matrix_rows(P, layout, stride, cap):
        r = u64s(P.rec)
        row_of = np.zeros(P.n + 1, dtype=np.uint64)
        wsb = L.emu_matrix_workspace_size(P.n, P.S, layout)
        ws = np.full(wsb + 64, 0xCD, dtype=np.uint8)
        err = np.zeros(1, dtype=np.uint64)
        st = L.emu_matrix_device(base(P), r.ctypes.data, None, P.n, P.S, layout, out.ctypes.data, cap, stride,
                                 row_of.ctypes.data, ws.ctypes.data, wsb, err.ctypes.data)
        return st, int(err[0]), row_of.tolist()

    def poke(off, data):
        out[off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)
    F.check_matrix_stride(F.host_arena(), matrix_rows, lambda off, n: out[off:off + n].tobytes(), poke)


def test_ld_tables_row_stride_above_2_30(arena):
    L = TL.lib()

    def tables(bed, n_rows, stride, S, W, pairs_cap):
        out = np.full(9 * pairs_cap + 16, 0xEEEEEEEE, dtype=np.uint32)
        wsb = L.emu_ld_workspace_size(n_rows, S, W)
        ws = np.full(wsb + 64, 0xCD, dtype=np.uint8)
        err = np.full(1, 0x1111, dtype=np.uint64)
        st = L.emu_ld_tables_device(bed, n_rows, stride, S, W, out.ctypes.data, pairs_cap, ws.ctypes.data, wsb, err.ctypes.data)
        assert (out[9 * pairs_cap:] == 0xEEEEEEEE).all() and (ws[wsb:] == 0xCD).all()
        return st, int(err[0]), out[:9 * pairs_cap].reshape(n_rows, W, 9)
    F.check_bed_stride(arena, tables)
