"""The device entries on records that lie around byte offsets 2^31 and 2^32
of one device allocation (far_cases.py), through the C ABI
(libvcfc.so) on the GPU; test_far_emu.py runs the same checks on the CPU
emulator.  The arena (FAR + SLACK bytes, uninitialised) and the strided
matrix output (5 rows of 2^30 + 16 bytes) are allocated once per process;
every kernel call is on kilobytes of records, the encoder's on a megabyte of
lines.  Then k_record_hash, the judge of the full-size parity tests and of
bench.py's output check, against its plain statement and for its sensitivity
to every bit of a record."""
import functools
import os
import random
import sys

import numpy as np
import pytest

import far_cases as F
import golden_io as G
import ld_cases as LC
import matrix_cases as MC
from test_record_hash import py_hash64

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(G.REPO, "vcf-compression_amd"))
DEV = "cuda:0"
OK = 0


class GpuArena:
    def __init__(self):
        import torch
        assert torch.cuda.is_available(), "GPU tests need a GPU"
        try:
            self.t = torch.empty(F.FAR + F.SLACK, dtype=torch.uint8, device=DEV)
        except RuntimeError as e:
            raise AssertionError("the far arena (%d bytes of device memory) could not be allocated: %s" % (F.FAR + F.SLACK, e))
        self.ptr = self.t.data_ptr()

    def write(self, off, data):
        import torch
        assert 0 <= off and off + len(data) <= F.FAR + F.SLACK
        self.t[off:off + len(data)] = torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).to(DEV)

    def read(self, off, n):
        return self.t[off:off + n].cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def gpu_arena():
    return GpuArena()


@functools.lru_cache(maxsize=None)
def strided_output():
    import torch
    try:
        return torch.empty(F.STRIDE_ROWS * F.MATRIX_STRIDE, dtype=torch.uint8, device=DEV)
    except RuntimeError as e:
        raise AssertionError("the strided matrix output (%d bytes of device memory) could not be allocated: %s"
                             % (F.STRIDE_ROWS * F.MATRIX_STRIDE, e))


@pytest.fixture(scope="module")
def arena():
    return gpu_arena()


@pytest.fixture(scope="module")
def vcfc():
    import torch   # before libvcfc: one HIP runtime in the process
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import vcfc
    return vcfc


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(DEV)


def filled(n, byte=0xEE):
    import torch
    return torch.full((n,), byte, dtype=torch.uint8, device=DEV)


def words(n):
    import torch
    return torch.zeros(n, dtype=torch.int64, device=DEV)


def u64(t):
    return [int(x) for x in t.cpu().numpy().view(np.uint64)]


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def sync():
    import torch
    torch.cuda.synchronize()


def recs_of(P):
    return dev(np.array(P.rec, dtype=np.uint64))


def sel_of(select):
    return None if select is None else dev(np.array(select, dtype=np.uint8))


def p(t):
    return None if t is None else t.data_ptr()


# ---- matching ---------------------------------------------------------------------

def test_query_match(arena, vcfc):
    def match(P, q):
        r, ref = recs_of(P), dev(np.array(list(q[0]) + [0], dtype=np.uint8))
        flag, err = filled(P.n + 64), words(1)
        st = vcfc.query_match_device(P.ptr, p(r), P.n, p(ref), len(q[0]), q[1], q[2], q[3], p(flag), p(err), stream())
        sync()
        assert bool((flag[P.n:] == 0xEE).all()), "flags written past n"
        return st, u64(err)[0], flag[:P.n].cpu().tolist()
    F.check_match(arena, match)


def test_regions_match(arena, vcfc):
    def regions(P, text):
        table = vcfc.regions_build(text)
        wsb = vcfc.regions_workspace_size(len(table))
        ws = filled(wsb + 64, 0xCD)
        assert vcfc.regions_upload(table, p(ws), wsb, stream()) == OK
        r, flag, err = recs_of(P), filled(P.n + 64), words(1)
        st = vcfc.regions_match_device(P.ptr, p(r), P.n, p(ws), wsb, p(flag), p(err), stream())
        sync()
        assert bool((flag[P.n:] == 0xEE).all()) and bool((ws[wsb:] == 0xCD).all()), "written past the flags / the workspace"
        return st, u64(err)[0], flag[:P.n].cpu().tolist()
    F.check_regions(arena, regions)


# ---- decode -------------------------------------------------------------------------

def test_decode_sizes(arena, vcfc):
    import torch

    def sizes(P):
        r, lo, po, cc, err = recs_of(P), words(P.n + 1), words(P.n), words(P.n), words(1)
        pl = torch.zeros(P.n, dtype=torch.int32, device=DEV)
        wsb = vcfc.decode_sizes_workspace_size(P.n)
        ws = filled(wsb)
        vcfc.decode_sizes_device(P.ptr, P.in_bytes, p(r), P.n, P.S, p(lo), p(po), p(pl), p(cc), p(ws), wsb, p(err), stream())
        sync()
        return OK, u64(err)[0], u64(lo), u64(po), pl.cpu().tolist(), u64(cc)
    F.check_sizes(arena, sizes)


def test_decode_records_and_selected(arena, vcfc):
    def decode(P, select, exact):
        cap = 8 * len(P.f.body) + 4 * P.S * P.n + 4096
        r, sel, out, lo, err = recs_of(P), sel_of(select), filled(cap + 64), words(P.n + 1), words(1)
        wsb = vcfc.decode_workspace_size(P.n)
        ws = filled(wsb)
        if select is None:
            vcfc.decode_records_device(P.ptr, P.in_bytes, p(r), P.n, P.S, p(out), cap, p(lo), p(ws), wsb, p(err), stream(), exact)
        else:
            vcfc.decode_selected_device(P.ptr, P.in_bytes, p(r), p(sel), P.n, P.S, p(out), cap, p(lo), p(ws), wsb, p(err),
                                        stream(), exact)
        sync()
        assert bool((out[cap:] == 0xEE).all()), "bytes written past out_cap"
        e, lo = u64(err)[0], u64(lo)
        ok = e == F.NO_ERROR
        return OK, e, lo if ok else [], out[:lo[P.n]].cpu().numpy().tobytes() if ok else b""
    F.check_decode(arena, decode)


# ---- the readers ------------------------------------------------------------------------

def test_decode_samples(arena, vcfc):
    def subset(P, cols, select):
        cap = 8 * len(P.f.body) + 4 * P.S * P.n + 64
        r, sel, out, lo, err = recs_of(P), sel_of(select), filled(cap + 64), words(P.n + 1), words(1)
        wsb = vcfc.subset_workspace_size(P.n, len(cols))
        ws = filled(wsb)
        st = vcfc.decode_samples_device(P.ptr, P.in_bytes, p(r), p(sel), P.n, P.S, cols, p(out), cap, p(lo), p(ws), wsb, p(err),
                                        stream())
        sync()
        assert bool((out[cap:] == 0xEE).all()), "bytes written past out_cap"
        lo = u64(lo)
        return st, u64(err)[0], lo, out[:min(lo[P.n], cap)].cpu().numpy().tobytes()
    F.check_subset(arena, subset)


def test_genotype_counts(arena, vcfc):
    import torch

    def counts(P, select):
        r, sel, err = recs_of(P), sel_of(select), words(1)
        rows = torch.full((P.n + 1, 8), 0x6E6E6E6E, dtype=torch.int32, device=DEV)
        tab = words((P.S + 1) * 5)
        wsb = vcfc.counts_workspace_size(P.n, P.S)
        ws = filled(wsb + 64, 0xCD)
        st = vcfc.genotype_counts_device(P.ptr, P.in_bytes, p(r), p(sel), P.n, P.S, p(rows), p(tab), p(ws), wsb, p(err), stream())
        sync()
        assert bool((rows[P.n] == 0x6E6E6E6E).all()) and not bool(tab[5 * P.S:].any()) and bool((ws[wsb:] == 0xCD).all())
        return st, u64(err)[0], rows[:P.n].cpu().numpy().view(np.uint32).tolist(), np.array(u64(tab[:5 * P.S])).reshape(P.S, 5).tolist()
    F.check_counts(arena, counts)


def test_genotype_matrix(arena, vcfc):
    def matrix(P, layout, select, stride, cap, alloc):
        r, sel, err = recs_of(P), sel_of(select), words(1)
        out, row_of = filled(alloc + MC.CANARY, MC.FILL), words(P.n + 1)
        wsb = vcfc.matrix_workspace_size(P.n, P.S, layout)
        ws = filled(wsb + 64, 0xCD)
        st = vcfc.genotype_matrix_device(P.ptr, P.in_bytes, p(r), p(sel), P.n, P.S, layout, p(out), cap, stride, p(row_of),
                                         p(ws), wsb, p(err), stream())
        sync()
        assert bool((ws[wsb:] == 0xCD).all()), "written past the workspace"
        return st, u64(err)[0], out.cpu().numpy().tobytes(), u64(row_of)
    F.check_matrix(arena, matrix)


def test_extract_samples(arena, vcfc):
    def extract(P, cols, select):
        K = P.S if cols is None else len(cols)
        cap = vcfc.extract_bound(len(P.f.body), P.n, K)
        r, sel, out, ro, err = recs_of(P), sel_of(select), filled(cap + 64), words(P.n + 1), words(1)
        wsb = vcfc.extract_workspace_size(P.n, K)
        ws = filled(wsb)
        st = vcfc.extract_samples_device(P.ptr, P.in_bytes, p(r), p(sel), P.n, P.S, cols, p(out), cap, p(ro), p(ws), wsb, p(err),
                                         stream())
        sync()
        assert bool((out[cap:] == 0xEE).all()), "bytes written past out_cap"
        ro = u64(ro)
        return st, u64(err)[0], ro, out[:min(ro[P.n], cap)].cpu().numpy().tobytes()
    F.check_extract(arena, extract)


def test_ld_window(arena, vcfc):
    def ldwin(P, W, select, cap, slots):
        r, sel, err = recs_of(P), sel_of(select), words(1)
        out, row_of = filled(36 * slots + LC.CANARY, LC.FILL), words(P.n + 1)
        wsb = vcfc.ld_workspace_size(P.n, P.S, W)
        ws = filled(wsb + 64, 0xCD)
        st = vcfc.ld_window_device(P.ptr, P.in_bytes, p(r), p(sel), P.n, P.S, W, p(out), cap, p(row_of), p(ws), wsb, p(err),
                                   stream())
        sync()
        assert bool((ws[wsb:] == 0xCD).all()), "written past the workspace"
        return st, u64(err)[0], out.cpu().numpy().tobytes(), u64(row_of)
    F.check_ld_window(arena, ldwin)


# ---- the indexes --------------------------------------------------------------------------

def test_binned_index(arena, vcfc):
    def binned(P, base_offset, E):
        r, ent, w, err = recs_of(P), filled(13 * P.n + 16), words(2), words(1)
        wsb = vcfc.index_workspace_size(P.n)
        ws = filled(wsb)
        vcfc.binned_index_device(P.ptr, p(r), P.n, base_offset, E, p(ent), P.n, p(w), p(w) + 8, p(ws), wsb, p(err), stream())
        sync()
        w = u64(w)
        assert w[0] <= P.n and bool((ent[13 * w[0]:] == 0xEE).all()), "entries written past the count"
        return [u64(err)[0], w[0], w[1]], ent[:13 * w[0]].cpu().numpy().tobytes()
    F.check_binned(arena, binned)


def test_record_span(arena, vcfc):
    def span(P):
        r, ref, pos, end, err = recs_of(P), filled(P.n), words(P.n), words(P.n), words(1)
        vcfc.record_span_device(P.ptr, p(r), P.n, p(ref), p(pos), p(end), p(err), stream())
        sync()
        return u64(err)[0], ref.cpu().tolist(), u64(pos), u64(end)
    F.check_span(arena, span)


def test_sparse_index(arena, vcfc):
    def spx(P, base_offset):
        r, ent, fo, cnt, status, err = recs_of(P), filled(13 * P.n + 16), words(P.n), words(1), words(3), words(1)
        wsb = vcfc.sparse_index_workspace_size(P.n)
        ws = filled(wsb)
        vcfc.sparse_index_device(P.ptr, p(r), P.n, base_offset, p(ent), p(fo), p(cnt), p(status), p(ws), wsb, p(err), stream())
        sync()
        c = u64(cnt)[0]
        assert c <= P.n and bool((ent[13 * c:] == 0xEE).all()), "entries written past the count"
        return [u64(err)[0], c] + u64(status), ent[:13 * c].cpu().numpy().tobytes(), u64(fo)[:c]
    F.check_sparse_index(arena, spx)


def test_sparse_plan(arena, vcfc):
    def splan(P, data_start):
        r, fo, pf, status = recs_of(P), words(P.n), filled(16 * P.n), words(2)
        vcfc.sparse_plan_device(P.ptr, p(r), P.n, data_start, p(fo), p(pf), p(status), stream())
        sync()
        return u64(fo), pf.cpu().numpy().tobytes(), u64(status)
    F.check_sparse_plan(arena, splan)


# ---- the digest with far offsets, and the encoder's input ------------------------------------

def test_record_hash_far(arena, vcfc):
    def rhash(P):
        r, out = recs_of(P), words(P.n)
        vcfc.record_hash_device(P.ptr, p(r), P.n, p(out), stream())
        sync()
        return u64(out)
    F.check_record_hash(arena, rhash, py_hash64)


@pytest.mark.parametrize("name", [b[0] for b in F.encode_batches()])
def test_encode_rows(arena, vcfc, name):
    def encode(ptr, offs, lens):
        n, total = len(offs), sum(lens)
        lo, ll = dev(np.array(offs, dtype=np.uint64)), dev(np.array(lens, dtype=np.uint32))
        cap, wsb = vcfc.encode_bound(n, total), vcfc.workspace_size(n, total)
        out, ws, rec, err = filled(cap + 64), filled(wsb), words(n + 1), words(1)
        vcfc.encode_rows_device(ptr, p(lo), p(ll), n, total, p(out), cap, p(rec), p(ws), wsb, p(err), stream())
        sync()
        assert bool((out[cap:] == 0xEE).all()), "bytes written past out_cap"
        rec = u64(rec)
        if name == "gdg_batch":
            assert vcfc.encode_deferred_rows(p(ws), n, total, stream()) > 0, "the GT:DP:GQ rows were not deferred"
        return u64(err)[0], rec, out[:min(rec[n], cap)].cpu().numpy().tobytes()
    F.check_encode(arena, encode, (name,))


# ---- strides ----------------------------------------------------------------------------------

def test_matrix_row_stride_above_2_30(arena, vcfc):
    import torch
    out = strided_output()

    def matrix_rows(P, layout, stride, cap):
        assert cap <= out.numel()
        r, row_of, err = recs_of(P), words(P.n + 1), words(1)
        wsb = vcfc.matrix_workspace_size(P.n, P.S, layout)
        ws = filled(wsb)
        st = vcfc.genotype_matrix_device(P.ptr, P.in_bytes, p(r), None, P.n, P.S, layout, p(out), cap, stride, p(row_of), p(ws),
                                         wsb, p(err), stream())
        sync()
        return st, u64(err)[0], u64(row_of)

    def poke(off, data):
        assert 0 <= off and off + len(data) <= out.numel()
        out[off:off + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(DEV)
    F.check_matrix_stride(arena, matrix_rows, lambda off, n: out[off:off + n].cpu().numpy().tobytes(), poke)


def test_ld_tables_row_stride_above_2_30(arena, vcfc):
    import torch

    def tables(bed, n_rows, stride, S, W, pairs_cap):
        assert arena.ptr <= bed and bed + (n_rows - 1) * stride + MC.row_bytes(MC.BED, S) + 64 <= arena.ptr + F.FAR + F.SLACK
        out = torch.full((9 * pairs_cap + 16,), 0x6E6E6E6E, dtype=torch.int32, device=DEV)
        err = words(1)
        wsb = vcfc.ld_workspace_size(n_rows, S, W)
        ws = filled(wsb + 64, 0xCD)
        st = vcfc.ld_tables_device(bed, n_rows, stride, S, W, p(out), pairs_cap, p(ws), wsb, p(err), stream())
        sync()
        assert bool((out[9 * pairs_cap:] == 0x6E6E6E6E).all()) and bool((ws[wsb:] == 0xCD).all())
        return st, u64(err)[0], out[:9 * pairs_cap].cpu().numpy().view(np.uint32).reshape(n_rows, W, 9)
    F.check_bed_stride(arena, tables)


def test_device_memory_held(arena):
    """The two allocations the far tests keep: the arena and the strided output, 9.008 GiB."""
    import torch
    print("device memory held by the far tests: %d bytes allocated, %d reserved" % (torch.cuda.memory_allocated(), torch.cuda.memory_reserved()))
    assert arena.t.numel() + strided_output().numel() == F.FAR + F.SLACK + F.STRIDE_ROWS * F.MATRIX_STRIDE == 9672065104


# ---- k_record_hash against its plain statement ------------------------------------------------

def gpu_hashes(vcfc, blob, off):
    d, o, out = dev(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8)), dev(np.asarray(off, dtype=np.uint64)), words(len(off) - 1)
    vcfc.record_hash_device(p(d), p(o), len(off) - 1, p(out), stream())
    sync()
    return u64(out)


def test_kernel_digest_every_alignment(vcfc):
    """test_record_hash.test_emulated_kernel_digest_every_alignment on the
    GPU: records of 0..1100 bytes packed back to back behind 0..3 bytes."""
    rnd = random.Random(2)
    lens = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 520, 1100] + [rnd.randrange(0, 300) for _ in range(40)]
    assert set(range(0, 4)) | {15, 16, 17, 63, 64, 65, 511, 512, 513, 520, 1100} <= set(lens)
    recs = [bytes(rnd.randrange(256) for _ in range(n)) for n in lens]
    want = [py_hash64(r) for r in recs]
    for lead in range(4):
        off = np.zeros(len(recs) + 1, dtype=np.uint64)
        np.cumsum([len(r) for r in recs], out=off[1:])
        off += np.uint64(lead)
        assert gpu_hashes(vcfc, b"\xAB" * lead + b"".join(recs), off) == want, lead
    rnd = random.Random(3)   # every length 0 .. 17 at every lead
    recs = [bytes(rnd.randrange(256) for _ in range(n)) for n in range(18)]
    for lead in range(4):
        off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64) + np.uint64(lead)
        assert gpu_hashes(vcfc, b"\xAB" * lead + b"".join(recs), off) == [py_hash64(r) for r in recs], lead


@pytest.mark.parametrize("lead", [0, 3])
def test_kernel_digest_sees_every_bit_and_nothing_else(vcfc, lead):
    """Per length class a record in 8 L + 3 copies, one byte apart: the record
    as it is, each of its bits flipped in turn, the byte before it changed,
    the byte behind it changed.  Every flip changes the digest; the two
    neighbours do not."""
    rnd = random.Random(11 + lead)
    for L in (0, 1, 7, 8, 9, 17, 64, 65, 512, 513, 1100):
        rec = np.frombuffer(bytes(rnd.randrange(256) for _ in range(L)), dtype=np.uint8)
        copies = 8 * L + 3
        a = np.full((copies, L + 2), 0x5A, dtype=np.uint8)
        a[:, 1:L + 1] = rec
        for b in range(8 * L):
            a[1 + b, 1 + b // 8] ^= 1 << (b % 8)
        a[8 * L + 1, 0] ^= 0xFF
        a[8 * L + 2, L + 1] ^= 0xFF
        # the copies and the two bytes between them, as alternating records
        off = np.empty(2 * copies, dtype=np.uint64)
        off[0::2] = np.arange(copies, dtype=np.uint64) * np.uint64(L + 2) + np.uint64(1 + lead)
        off[1::2] = off[0::2] + np.uint64(L)
        h = gpu_hashes(vcfc, b"\xAB" * lead + a.tobytes(), off)[0::2]
        assert h[0] == py_hash64(rec.tobytes()), L
        same = [b for b in range(8 * L) if h[1 + b] == h[0]]
        assert not same, (L, "bit flips the digest does not see", same[:8])
        assert h[8 * L + 1] == h[0] and h[8 * L + 2] == h[0], (L, "a neighbouring byte changes the digest")
