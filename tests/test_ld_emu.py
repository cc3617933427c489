"""ld-window on the CPU: the Python restatement (ld_cases.py)
pinned to a hand-written known answer, to genotype-counts and to its own
symmetries, then the product kernels (csrc/vcfc_ld.hip) and host driver
(csrc/vcfc_ld_driver.h) compiled against the fiber SIMT emulator, held to the
restatement: status, failing record, indices, every table of the band, the
text file, and every byte of the band's allocation outside the slots that
are due.  No tolerance anywhere.  test_gpu_ld.py repeats it on the GPU."""
import ctypes

import numpy as np
import pytest

import counts_cases as CC
import decode_cases as D
import emu_io as E
import ld_cases as LC
import matrix_cases as MC
import subset_cases as SC

OK, E_ARG, E_FORMAT = LC.OK, LC.E_ARG, LC.E_FORMAT
_lib = None


def lib():
    """The emulator build of the ld kernels and driver (flags as tests/simt_emu/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    L = E.build_emu_lib("ld", ("vcfc_ld.hip", "vcfc_matrix.hip", "vcfc_regions.hip", "vcfc_decode.hip", "vcfc_encode.hip"),
                        "emu_ld_api.cpp")
    vp, u64, cp, ci, dbl = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int, ctypes.c_double
    pu64 = ctypes.POINTER(u64)
    for f in (L.emu_ld_workspace_size, L.emu_ld_tile_rows, L.emu_ld_tile_partners, L.emu_ld_chunk_samples,
              L.emu_ld_matrix_lds_samples):
        f.restype = u64
    L.emu_ld_workspace_size.argtypes = [u64, u64, u64]
    L.emu_ld_file.argtypes = [cp, u64, u64, ci, cp, u64, ci, u64, u64, cp, u64, u64, vp, vp, u64, u64, pu64, pu64, dbl, vp,
                              pu64, u64]
    L.emu_ld_tables_device.argtypes = [vp, u64, u64, u64, u64, vp, u64, vp, u64, vp]
    L.emu_ld_window_device.argtypes = [cp, vp, vp, u64, u64, u64, vp, u64, vp, vp, u64, vp]
    _lib = L
    return L


def emu_run(data, W, query=None, regions=None, band_bound=0, min_r2=None):
    """emu_ld_file: (status, indices, band, failing record, the file entry's text)."""
    h = SC.parse_header(data)
    cap = len(SC.hop(data[h[0]:])[0]) if h else 1
    Wc = W if LC.window_ok(W) else 1
    idx = np.zeros(cap + 1, dtype=np.uint64)
    tables = np.zeros((cap + 1) * Wc * 9, dtype=np.uint32)
    tcap = len(LC.TSV_HEAD) + (cap + 1) * Wc * (len(data) // max(cap, 1) + 64) + 256
    text = np.zeros(tcap, dtype=np.uint8)
    n, bad, tl = (ctypes.c_uint64(0) for _ in range(3))
    q = query or (b"", False, 0, 0)
    mode = 2 if regions is not None else 1 if query is not None else 0
    st = lib().emu_ld_file(data, len(data), W, mode, q[0], len(q[0]), int(q[1]), q[2], q[3], regions or b"",
                           len(regions or b""), band_bound, idx.ctypes.data, tables.ctypes.data, cap + 1, (cap + 1) * Wc,
                           ctypes.byref(n), ctypes.byref(bad), min_r2 or 0.0, text.ctypes.data, ctypes.byref(tl), tcap)
    band = tables[:n.value * Wc * 9].reshape(n.value, Wc, 9)
    return st, [int(x) for x in idx[:n.value]], band, bad.value, text[:tl.value].tobytes()


def _alloc(slots):
    return np.full(36 * slots + LC.CANARY, LC.FILL, dtype=np.uint8)


def emu_tables(bed, n_rows, row_stride, S, W, pairs_cap, alloc_slots, offset=0, ws_short=0, null=None, n_override=None):
    base = np.zeros(len(bed) + 48, dtype=np.uint8)
    shift = (-base.ctypes.data) % 16 + offset   # d_bed's alignment is `offset`, whatever the allocator gave
    base[shift:shift + len(bed)] = np.frombuffer(bed, dtype=np.uint8)
    out = _alloc(alloc_slots)
    n = n_rows if n_override is None else n_override
    wsb = lib().emu_ld_workspace_size(n_rows, S if 0 < S < 1 << 30 else 1, W) - ws_short
    ws = np.full(wsb + 64, 0xCD, dtype=np.uint8)
    err = np.full(1, 0x1111, dtype=np.uint64)
    st = lib().emu_ld_tables_device(base.ctypes.data + shift, n, row_stride, S, W, None if null == "tables" else out.ctypes.data,
                                    pairs_cap, None if null == "ws" else ws.ctypes.data, wsb,
                                    None if null == "err" else err.ctypes.data)
    assert (ws[wsb:] == 0xCD).all(), "written past the workspace"
    return st, int(err[0]), out.tobytes()


def emu_window(body, rec, S, W, select, pairs_cap, alloc_slots, ws_short=0, null=None, n_override=None):
    n = len(rec) - 1
    r = np.array(rec, dtype=np.uint64)
    sel = None if select is None else np.array(select, dtype=np.uint8)
    out = _alloc(alloc_slots)
    row_of = np.full(n + 2, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    wsb = lib().emu_ld_workspace_size(n, S if 0 < S < 1 << 30 else 1, W) - ws_short
    ws = np.full(wsb + 64, 0xCD, dtype=np.uint8)
    err = np.full(1, 0x1111, dtype=np.uint64)
    st = lib().emu_ld_window_device(body, r.ctypes.data, None if sel is None else sel.ctypes.data,
                                    n if n_override is None else n_override, S, W,
                                    None if null == "tables" else out.ctypes.data, pairs_cap,
                                    None if null == "row_of" else row_of.ctypes.data, None if null == "ws" else ws.ctypes.data,
                                    wsb, None if null == "err" else err.ctypes.data)
    assert (ws[wsb:] == 0xCD).all(), "written past the workspace"
    assert row_of[n + 1] == 0xEEEEEEEEEEEEEEEE
    return st, int(err[0]), out.tobytes(), [int(x) for x in row_of[:n + 1]]


def lds_bed():
    return lib().emu_ld_matrix_lds_samples()


# ---- the restatement, before any kernel runs -----------------------------------

def test_known_answer():
    data = LC.kat_file()
    st, idx, band, bad = LC.ld(data, LC.KAT_W)
    assert (st, idx, bad) == (OK, [0, 1, 2], LC.NO_RECORD)
    assert band.tolist() == LC.KAT_BAND
    assert [[LC.r2(t)[0] for t in row] for row in band] == LC.KAT_N
    assert [[LC.r2_text(LC.r2(t)[1]) for t in row] for row in band] == LC.KAT_R2
    assert LC.r2(band[0, 0])[1] == 16.0 / 88.0 and LC.r2(band[0, 1])[1] == 0.5 and LC.r2(band[1, 0])[1] == 100.0 / 280.0
    assert LC.tsv(data, idx, band, LC.KAT_W, 0.0) == LC.KAT_TSV
    assert LC.tsv(data, idx, band, LC.KAT_W, 0.5).split(b"\n")[1:-1] == [b"1\t100\trs0\t1\t102\trs2\t4\t0.5"]
    assert LC.genotypes(bytes([0x4B, 0x02]), 5) == [0, 1, 2, None, 1]   # matrix_cases' literal .bed row


def test_restatement_agrees_with_counts_and_itself():
    checked = 0
    files = D.valid_files(1)[:5] + [("ld%d" % S, LC.ld_file(S, 7, 0.1)) for S in (5, 33, 129)]
    for name, data in files:
        st, idx, crow, samples = CC.counts(data)
        rows = MC.matrix(data, MC.BED)[2]
        S = SC.parse_header(data)[1]
        g = [LC.genotypes(r, S) for r in rows[:12]]
        for i in range(len(g)):
            for j in range(i + 1, len(g)):
                t = LC.table(g[i], g[j])
                assert sum(t) <= S
                assert LC.table(g[j], g[i]) == [t[3 * b + a] for a in range(3) for b in range(3)]   # the transpose
                if crow[i][4] == 0 and crow[j][4] == 0:   # n_other == 0: every sample called in both
                    ci, cj = crow[i], crow[j]
                    assert [sum(t[3 * a:3 * a + 3]) for a in range(3)] == [ci[0], ci[1] + ci[2], ci[3]], (name, i, j)
                    assert [sum(t[b::3]) for b in range(3)] == [cj[0], cj[1] + cj[2], cj[3]], (name, i, j)
                    checked += 1
    assert checked >= 50, checked


# ---- the kernels and driver on the emulator --------------------------------------

def test_constants():
    L = lib()
    assert (L.emu_ld_tile_rows(), L.emu_ld_tile_partners(), L.emu_ld_chunk_samples()) == \
        (LC.TILE_ROWS, LC.TILE_PARTNERS, LC.CHUNK_SAMPLES)


def test_known_answer_on_the_kernels():
    got = emu_run(LC.kat_file(), LC.KAT_W)
    assert got[0] == OK and got[2].tolist() == LC.KAT_BAND and got[4] == LC.KAT_TSV


def test_sample_counts():
    LC.check_sizes(emu_run, lds_bed())


def test_rows_and_windows():
    LC.check_shapes(emu_run)


def test_batches():
    LC.check_batches(emu_run)


def test_tables_device():
    LC.check_tables_device(emu_tables)


def test_tables_device_arguments():
    LC.check_tables_args(emu_tables, lib().emu_ld_workspace_size)


def test_window_device():
    LC.check_window_device(emu_window)


def test_window_device_arguments():
    LC.check_window_args(emu_window, lib().emu_ld_workspace_size)


@pytest.mark.parametrize("seed", [1])
def test_query_files(seed):
    LC.check_queries(emu_run, seed)


def test_region_tables():
    LC.check_regions(emu_run)


@pytest.mark.parametrize("seed", [3])
def test_mutated_files(seed):
    LC.check_mutated(emu_run, seed)


def test_irregular_records():
    LC.check_irregular(emu_run)


def test_bad_headers_and_windows():
    data = D.valid_files(1)[2][1]
    for W in (0, 1 << 16):
        assert emu_run(data, W)[0] == E_ARG == LC.ld(data, W)[0]
    got = emu_run(data[1:], 2)
    assert (got[0], got[1], got[3], got[4]) == (E_FORMAT, [], LC.NO_RECORD, b"") and LC.ld(data[1:], 2)[0] == E_FORMAT
    s0 = next(d for n, d in D.mutated_files(3) if n == "S0_row")
    assert emu_run(s0, 2)[0] == E_ARG == LC.ld(s0, 2)[0]


def test_text_file():
    LC.check_tsv(emu_run)
