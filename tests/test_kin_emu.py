"""kinship on the CPU: the Python restatement (kin_cases.py)
pinned to a hand-written known answer, to genotype-counts and to its own
symmetries, then the product kernels (csrc/vcfc_kin.hip) and host driver
(csrc/vcfc_kin_driver.h) compiled against the fiber SIMT emulator, held to the
restatement: status, failing record, indices, every table of the square, the
text file, and every byte of the square's allocation outside it.  No tolerance
anywhere.  test_gpu_kin.py repeats it on the GPU."""
import ctypes

import numpy as np
import pytest

import counts_cases as CC
import decode_cases as D
import emu_io as E
import kin_cases as KC
import matrix_cases as MC
import subset_cases as SC

OK, E_ARG, E_FORMAT = KC.OK, KC.E_ARG, KC.E_FORMAT
_lib = None


def lib():
    """The emulator build of the kinship kernels and driver (flags as tests/simt_emu/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    L = E.build_emu_lib("kin", ("vcfc_kin.hip", "vcfc_matrix.hip", "vcfc_regions.hip", "vcfc_decode.hip", "vcfc_encode.hip"),
                        "emu_kin_api.cpp")
    vp, u64, cp, ci, dbl = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int, ctypes.c_double
    pu64 = ctypes.POINTER(u64)
    for f in (L.emu_kin_workspace_size, L.emu_kin_tile_samples, L.emu_kin_chunk_words, L.emu_kin_plane_rows,
              L.emu_kin_batch_records, L.emu_kin_batch_need):
        f.restype = u64
    L.emu_kin_workspace_size.argtypes = [u64, u64]
    L.emu_kin_batch_records.argtypes = [u64, u64]
    L.emu_kin_batch_need.argtypes = [u64, u64]
    L.emu_kin_file.argtypes = [cp, u64, ci, cp, u64, ci, u64, u64, cp, u64, u64, vp, vp, u64, u64, pu64, pu64, pu64, ci, dbl,
                               vp, pu64, u64]
    L.emu_kin_tables_device.argtypes = [vp, u64, u64, u64, vp, u64, ci, vp, u64, vp]
    L.emu_kin_records_device.argtypes = [cp, vp, vp, u64, u64, vp, u64, ci, vp, vp, u64, vp]
    _lib = L
    return L


def emu_run(data, query=None, regions=None, batch=0, text=None):
    """emu_kin_file: (status, indices, square, failing record, the file entry's text or None)."""
    h = SC.parse_header(data)
    S = h[1] if h and 0 < h[1] < 1 << 30 else 0
    cap = len(SC.hop(data[h[0]:])[0]) if h else 1
    idx = np.zeros(cap + 1, dtype=np.uint64)
    tables = np.zeros(max(S * S, 1) * 9, dtype=np.uint32)
    tcap = (len(KC.TSV_HEAD) + S * S * 80 + 256) if text is not None else 0
    out = np.zeros(max(tcap, 1), dtype=np.uint8)
    n, ns, bad, tl = (ctypes.c_uint64(0) for _ in range(4))
    q = query or (b"", False, 0, 0)
    mode = 2 if regions is not None else 1 if query is not None else 0
    bound = lib().emu_kin_batch_need(batch, S) if batch and S else 0   # the bound that gives `batch` records a batch
    if bound:
        assert lib().emu_kin_batch_records(S, bound) == batch and lib().emu_kin_batch_records(S, bound - 1) == max(batch - 1, 1)
    st = lib().emu_kin_file(data, len(data), mode, q[0], len(q[0]), int(q[1]), q[2], q[3], regions or b"", len(regions or b""),
                            bound, idx.ctypes.data, tables.ctypes.data, cap + 1, S * S, ctypes.byref(n), ctypes.byref(ns),
                            ctypes.byref(bad), int(text not in (None, "all")), 0.0 if text in (None, "all") else text,
                            out.ctypes.data, ctypes.byref(tl), tcap)
    sq = tables[:ns.value * ns.value * 9].reshape(ns.value, ns.value, 9)
    return st, [int(x) for x in idx[:n.value]], sq, bad.value, out[:tl.value].tobytes() if text is not None else None


def _alloc(alloc_tables, prefill):
    out = np.full(36 * alloc_tables + KC.CANARY, KC.FILL, dtype=np.uint8)
    if prefill is not None:
        out[:len(prefill)] = np.frombuffer(prefill, dtype=np.uint8)
    return out


def emu_tables(bed, n_rows, row_stride, S, tables_cap, alloc_tables, accumulate=0, prefill=None, offset=0, ws_short=0, null=None,
               n_override=None):
    base = np.zeros(len(bed) + 48, dtype=np.uint8)
    shift = (-base.ctypes.data) % 16 + offset   # d_bed's alignment is `offset`, whatever the allocator gave
    base[shift:shift + len(bed)] = np.frombuffer(bed, dtype=np.uint8)
    out = _alloc(alloc_tables, prefill)
    n = n_rows if n_override is None else n_override
    wsb = lib().emu_kin_workspace_size(n_rows, S if 0 < S < 1 << 30 else 1) - ws_short
    ws = np.full(wsb + 64, 0xCD, dtype=np.uint8)
    err = np.full(1, 0x1111, dtype=np.uint64)
    st = lib().emu_kin_tables_device(base.ctypes.data + shift, n, row_stride, S, None if null == "tables" else out.ctypes.data,
                                     tables_cap, accumulate, None if null == "ws" else ws.ctypes.data, wsb,
                                     None if null == "err" else err.ctypes.data)
    assert (ws[wsb:] == 0xCD).all(), "written past the workspace"
    return st, int(err[0]), out.tobytes()


def emu_records(body, rec, S, select, tables_cap, alloc_tables, accumulate=0, prefill=None, ws_short=0, null=None,
                n_override=None):
    n = len(rec) - 1
    r = np.array(rec, dtype=np.uint64)
    sel = None if select is None else np.array(select, dtype=np.uint8)
    out = _alloc(alloc_tables, prefill)
    row_of = np.full(n + 2, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    wsb = lib().emu_kin_workspace_size(n, S if 0 < S < 1 << 30 else 1) - ws_short
    ws = np.full(wsb + 64, 0xCD, dtype=np.uint8)
    err = np.full(1, 0x1111, dtype=np.uint64)
    st = lib().emu_kin_records_device(body, r.ctypes.data, None if sel is None else sel.ctypes.data,
                                      n if n_override is None else n_override, S, None if null == "tables" else out.ctypes.data,
                                      tables_cap, accumulate, None if null == "row_of" else row_of.ctypes.data,
                                      None if null == "ws" else ws.ctypes.data, wsb, None if null == "err" else err.ctypes.data)
    assert (ws[wsb:] == 0xCD).all(), "written past the workspace"
    assert row_of[n + 1] == 0xEEEEEEEEEEEEEEEE
    return st, int(err[0]), out.tobytes(), [int(x) for x in row_of[:n + 1]]


# ---- the restatement, before any kernel runs -----------------------------------

def test_known_answer():
    data = KC.kat_file()
    st, idx, sq, bad = KC.kin(data)
    assert (st, idx, bad) == (OK, list(range(6)), KC.NO_RECORD) and sq.shape == (6, 6, 9)
    rows = MC.matrix(data, MC.BED)[2]
    cols = list(zip(*[KC.genotypes(r, KC.KAT_S) for r in rows]))
    assert cols[0] == (0, 1, 2, 1, 0, 1) and cols[2] == (2, 0, 0, 2, 1, None) and cols[5] == (None,) * 6
    for (i, j), t in KC.KAT_TABLES.items():
        assert sq[i, j].tolist() == t == KC.table(cols[i], cols[j]), (i, j)
    for (i, j), x in KC.KAT_STATS.items():
        got = KC.stats(sq[i, j])
        assert got[:7] == x[:7] and (KC.num_text(got[7]), KC.num_text(got[8])) == x[7:], (i, j, got)
    assert KC.stats(sq[0, 1])[7:] == (8.0 / 12.0, 2.0 / 12.0) and KC.stats(sq[0, 2])[7:] == (0.3, -2.25)
    text = KC.tsv(data, sq)
    assert text.startswith(KC.TSV_HEAD) and text.count(b"\n") == 16
    lines = text.split(b"\n")
    for (i, j), line in KC.KAT_LINES.items():
        assert lines[1 + sum(5 - k for k in range(i)) + j - i - 1] + b"\n" == line, (i, j)
    assert KC.tsv(data, sq, 0.0).split(b"\n")[1:-1] == [KC.KAT_LINES[(0, 1)][:-1], KC.KAT_LINES[(2, 3)][:-1]]
    assert KC.genotypes(bytes([0x4B, 0x02]), 5) == [0, 1, 2, None, 1]   # matrix_cases' literal .bed row


def test_restatement_agrees_with_counts_and_itself():
    checked = 0
    files = D.valid_files(1)[:5] + [("kin%d" % S, KC.kin_file(S, 9, 0.1)) for S in (5, 33, 65)]
    for name, data in files:
        st, idx, crow, samples = CC.counts(data)
        vst, vidx, rows, S, bad = MC.matrix(data, MC.BED)
        sq = KC.square(rows, S)
        assert st == OK == vst and sq.shape == (S, S, 9)
        assert np.array_equal(sq, sq.transpose(1, 0, 2)[:, :, [0, 3, 6, 1, 4, 7, 2, 5, 8]])       # t[j][i][3b + a] == t[i][j][3a + b]
        assert not sq[np.arange(S), np.arange(S)][:, [1, 2, 3, 5, 6, 7]].any()                  # the diagonal is diagonal
        assert int(sq.astype(np.int64).sum(axis=2).max()) <= len(rows)
        cols = list(zip(*[KC.genotypes(r, S) for r in rows]))
        for i in range(0, S, max(1, S // 6)):
            for j in range(0, S, max(1, S // 5)):
                assert sq[i, j].tolist() == KC.table(cols[i], cols[j]), (name, i, j)              # the plain count
        for i, s in enumerate(samples):
            if s[4] == 0:   # no c_other: every token of the sample is one of the four phased classes
                assert [int(sq[i, i, 0]), int(sq[i, i, 4]), int(sq[i, i, 8])] == [s[0], s[1] + s[2], s[3]], (name, i)
                checked += 1
    assert checked >= 50, checked


def test_identical_columns():
    sq = KC.kin(KC.twin_file())[2]
    x = KC.stats(sq[2, 7])
    assert x[8] == 0.5 and x[7] == 1.0 and sq[2, 7].tolist() == sq[2, 2].tolist() == sq[7, 7].tolist()
    assert all(KC.stats(sq[i, i])[8] in (0.5, None) for i in range(12)) and KC.stats(sq[9, 9])[8] is None


def test_seeded_coverage():
    """The seeds of the size and row files give what check_sizes and check_rows must see, by the restatement alone."""
    assert KC.seen([KC.kin(d)[2] for n, d in KC.size_files() if n != "S2504"])[2] >= 5
    full, empty, nohet = KC.seen([KC.kin(d, q)[2] for n, d, q in KC.row_files()])
    assert full >= 5 and empty >= 5 and nohet >= 5, (full, empty, nohet)


# ---- the kernels and driver on the emulator --------------------------------------

def test_constants():
    L = lib()
    assert (L.emu_kin_tile_samples(), L.emu_kin_chunk_words(), L.emu_kin_plane_rows()) == \
        (KC.TILE_SAMPLES, KC.CHUNK_WORDS, KC.PLANE_ROWS)


def test_known_answer_on_the_kernels():
    got = emu_run(KC.kat_file(), text="all")
    assert got[0] == OK and got[4] == KC.tsv(KC.kat_file(), KC.kin(KC.kat_file())[2])
    for (i, j), t in KC.KAT_TABLES.items():
        assert got[2][i, j].tolist() == t, (i, j)


def test_sample_counts():
    KC.check_sizes(emu_run)


def test_row_counts():
    KC.check_rows(emu_run)


def test_batches():
    KC.check_batches(emu_run)


def test_tables_device():
    KC.check_tables_device(emu_tables)


def test_tables_device_arguments():
    KC.check_tables_args(emu_tables, lib().emu_kin_workspace_size)


def test_records_device():
    KC.check_records_device(emu_records)


def test_records_device_arguments():
    KC.check_records_args(emu_records, lib().emu_kin_workspace_size)


@pytest.mark.parametrize("seed", [1])
def test_query_files(seed):
    KC.check_queries(emu_run, seed)


def test_region_tables():
    KC.check_regions(emu_run)


@pytest.mark.parametrize("seed", [3])
def test_mutated_files(seed):
    KC.check_mutated(emu_run, seed)


def test_irregular_records():
    KC.check_irregular(emu_run)


def test_bad_headers():
    data = D.valid_files(1)[2][1]
    got = emu_run(data[1:], text="all")
    assert (got[0], got[1], got[3], got[4]) == (E_FORMAT, [], KC.NO_RECORD, b"") and KC.kin(data[1:])[0] == E_FORMAT
    s0 = next(d for n, d in D.mutated_files(3) if n == "S0_row")
    assert emu_run(s0)[0] == E_ARG == KC.kin(s0)[0]


def test_text_file():
    KC.check_tsv(emu_run)
