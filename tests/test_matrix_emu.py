"""genotype-matrix on the CPU: the Python restatement
(matrix_cases.py) pinned to a literal token table, to the oracle -- the
per-token rule over the reference's own decode --, to genotype-counts and to
a hand-written .bed file, then the product kernels (csrc/vcfc_matrix.hip) and
host driver (csrc/vcfc_matrix_driver.h) compiled against the fiber SIMT
emulator, held to the restatement: status, failing record, indices, rows and
the three export-bed files, all exact, and every byte of the output
allocation outside the rows.  test_gpu_matrix.py repeats it on the GPU."""
import ctypes

import numpy as np
import pytest

import counts_cases as CC
import decode_cases as D
import emu_io as E
import golden_io as G
import matrix_cases as MC
import reader_edge_cases as RE
import subset_cases as SC

OK, E_ARG, E_FORMAT = MC.OK, MC.E_ARG, MC.E_FORMAT
_lib = None


def lib():
    """The emulator build of the matrix kernels and driver (flags as tests/simt_emu/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    L = E.build_emu_lib("matrix", ("vcfc_matrix.hip", "vcfc_regions.hip", "vcfc_decode.hip", "vcfc_encode.hip"),
                        "emu_matrix_api.cpp")
    vp, u64, cp, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int
    pu64 = ctypes.POINTER(u64)
    L.emu_matrix_row_bytes.restype = L.emu_matrix_lds_samples.restype = L.emu_matrix_workspace_size.restype = u64
    L.emu_matrix_row_bytes.argtypes = [ci, u64]
    L.emu_matrix_lds_samples.argtypes = [ci]
    L.emu_matrix_workspace_size.argtypes = [u64, u64, ci]
    L.emu_matrix_file.argtypes = [cp, u64, ci, ci, cp, u64, ci, u64, u64, cp, u64, u64, vp, vp, u64, pu64, pu64, pu64,
                                  vp, pu64, vp, pu64, vp, pu64, u64]
    L.emu_matrix_device.argtypes = [cp, vp, vp, u64, u64, ci, vp, u64, u64, vp, vp, u64, vp]
    _lib = L
    return L


def lds_samples(layout):
    return lib().emu_matrix_lds_samples(layout)


def emu_run(data, layout, query=None, regions=None, rec_batch=0):
    """emu_matrix_file: (status, indices, rows, S or None, failing record);
    for .bed the three file renderings are held to the restatement's on the way."""
    h = SC.parse_header(data)
    S = h[1] if h else 1
    cap = len(SC.hop(data[h[0]:])[0]) if h else 1
    rb = MC.row_bytes(layout, S) if 0 < S < 1 << 30 and layout in MC.LAYOUTS else 1
    idx = np.zeros(cap + 1, dtype=np.uint64)
    rows = np.zeros((cap + 1) * rb, dtype=np.uint8)
    tcap = (cap + 1) * rb + len(data) + 64 * max(S, 1) + 256
    bed, bim, fam = (np.zeros(tcap, dtype=np.uint8) for _ in range(3))
    n, ns, bad, bl, ml, fl = (ctypes.c_uint64(0) for _ in range(6))
    q = query or (b"", False, 0, 0)
    mode = 2 if regions is not None else 1 if query is not None else 0
    st = lib().emu_matrix_file(data, len(data), layout, mode, q[0], len(q[0]), int(q[1]), q[2], q[3], regions or b"",
                               len(regions or b""), rec_batch, idx.ctypes.data, rows.ctypes.data, cap + 1, ctypes.byref(n),
                               ctypes.byref(ns), ctypes.byref(bad), bed.ctypes.data, ctypes.byref(bl), bim.ctypes.data,
                               ctypes.byref(ml), fam.ctypes.data, ctypes.byref(fl), tcap)
    buf = rows.tobytes()
    got = (st, [int(x) for x in idx[:n.value]], [buf[k * rb:(k + 1) * rb] for k in range(n.value)],
           ns.value if st in (OK, E_FORMAT) and h else None, bad.value)
    if layout == MC.BED and st in (OK, E_FORMAT) and h and 0 < S < 1 << 30:
        assert bed[:bl.value].tobytes() == MC.bed_file(got[2])
        assert bim[:ml.value].tobytes() == MC.bim_file(data, got[1])
        assert fam[:fl.value].tobytes() == (MC.fam_file(data) if st == OK else b"")
    return got


def emu_device(body, rec, S, layout, select, row_stride, out_cap, alloc, ws_short=0, offset=0, null=None, n_override=None):
    n = len(rec) - 1
    r = np.array(rec, dtype=np.uint64)
    sel = None if select is None else np.array(select, dtype=np.uint8)
    base = np.full(offset + alloc + MC.CANARY + 16, MC.FILL, dtype=np.uint8)
    shift = (-base.ctypes.data) % 16   # d_out's alignment is `offset`, whatever the allocator gave
    out = base[shift + offset:]
    row_of = np.full(n + 2, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    wsb = lib().emu_matrix_workspace_size(n, S, layout) - ws_short
    ws = np.full(wsb + 64, 0xCD, dtype=np.uint8)
    err = np.zeros(1, dtype=np.uint64)
    st = lib().emu_matrix_device(body, r.ctypes.data, None if sel is None else sel.ctypes.data,
                                 n if n_override is None else n_override, S, layout,
                                 None if null == "out" else out.ctypes.data, out_cap, row_stride,
                                 None if null == "row_of" else row_of.ctypes.data, ws.ctypes.data, wsb, err.ctypes.data)
    assert (base[:shift + offset] == MC.FILL).all() and (ws[wsb:] == 0xCD).all(), "written before d_out / past the workspace"
    assert row_of[n + 1] == 0xEEEEEEEEEEEEEEEE
    return st, int(err[0]), out[:alloc + MC.CANARY].tobytes(), [int(x) for x in row_of[:n + 1]]


# ---- the restatement against what it restates (no kernel) ----------------------

def test_token_rule_is_the_literal_table():
    assert len(MC.CODE_TABLE) == 33 and [t for t, _ in MC.CODE_TABLE[:25]] == [t for t, _ in CC.GT_TABLE]
    for tok, want in MC.CODE_TABLE:
        assert MC.token_codes(tok) == want, tok
    for tok, d in MC.EXAMPLES.items():
        assert MC.token_codes(tok)[0] == d, tok
    for tok, hp in MC.HAP_EXAMPLES.items():
        assert MC.token_codes(tok)[1:3] == hp, tok
    for tok, k in CC.CLASS.items():   # the four run classes are constants
        assert MC.token_codes(tok) == [(0, 0, 0, 3), (1, 0, 1, 2), (1, 1, 0, 2), (2, 1, 1, 0)][k]
    assert MC.row(MC.HAP, [b"0|1", b"."]) == bytes([0, 1, 0xFF, 0xFF]) and MC.row(MC.DOSAGE, [b"1|1", b"./."]) == b"\x02\xff"


def test_bed_known_answer():
    data = MC.kat_file()
    st, idx, rows, S, bad = MC.matrix(data, MC.BED)
    assert (st, idx, S) == (OK, [0, 1, 2], 5)
    assert MC.bed_file(rows) == MC.BED_KAT and len(MC.BED_KAT) == 9
    assert all(r[-1] & MC.BED_KAT_PAD_MASK == 0 for r in rows)
    assert MC.bim_file(data, idx) == b"1\trs0\t0\t100\tG\tA\n1\trs1\t0\t101\tG\tA\n1\trs2\t0\t102\tG\tA\n"
    assert MC.fam_file(data) == b"".join(b"S%d\tS%d\t0\t0\t0\t-9\n" % (j, j) for j in range(5))
    assert emu_run(data, MC.BED)[2] == rows


@pytest.mark.parametrize("seed", [1])
def test_restatement_is_the_token_rule_over_the_oracle_decode(seed):
    for name, data in D.valid_files(seed):
        st, text = G.oracle_decompress(data, cap=len(data) * 40 + 4096)
        assert st == 0
        for layout in MC.LAYOUTS:
            got = MC.matrix(data, layout)
            assert got[0] == OK and got[1] == list(range(len(got[2]))), name
            assert got[2] == MC.matrix_of_vcf(text, layout), (name, layout)


@pytest.mark.parametrize("seed", [1])
def test_restatement_agrees_with_counts(seed):
    checked_ac1 = checked_sum = 0
    files = D.valid_files(seed) + [(n, d) for n, d in CC.hand_built() if n == "gt_tokens"]
    for name, data in files:
        body, rec, S = MC.records_of(data)
        st, idx, crow, samples = CC.counts(data)
        hap, dos = MC.matrix(data, MC.HAP)[2], MC.matrix(data, MC.DOSAGE)[2]
        assert st == OK and len(hap) == len(crow)
        for i, c in enumerate(crow):
            toks = SC.regular(body, rec[i], rec[i + 1], S)[1]
            pieces = [t.split(b":", 1)[0].replace(b"/", b"|").split(b"|") for t in toks]
            if all(len(p) <= 2 for p in pieces):
                assert hap[i].count(1) == c[6], (name, i)   # #(h == 1) == AC1
                checked_ac1 += 1
            if all(MC.token_codes(t)[0] >= 0 for t in toks):
                assert sum(dos[i]) == c[6] + c[7], (name, i)   # sum of dosage == AC1 + AC_other
                checked_sum += 1
    assert checked_ac1 >= 100 and checked_sum >= 100


# ---- the kernels and driver on the emulator -------------------------------------

def test_sizes():
    L = lib()
    assert [L.emu_matrix_row_bytes(k, 5) for k in (0, 1, 2, 3)] == [5, 10, 2, 0]
    assert [L.emu_matrix_row_bytes(2, S) for S in (1, 4, 5, 8)] == [1, 1, 2, 2]
    assert [lds_samples(k) for k in (0, 1, 2, 3)] == [5120, 2560, 4096, 0]


@pytest.mark.parametrize("seed", [1])
def test_valid_files(seed):
    MC.check_files(emu_run, D.valid_files(seed))


def test_small_sample_counts():
    MC.check_files(emu_run, MC.small_files())


def test_batch_sizes():
    MC.check_files(emu_run, SC.batch_files(), batches=(0, 1, 7))


def test_hand_built_records():
    MC.check_hand_built(emu_run)


def test_irregular_records():
    MC.check_irregular(emu_run)


@pytest.mark.parametrize("seed", [3, 4, 6])
def test_mutated_files(seed):
    MC.check_mutated(emu_run, seed)


@pytest.mark.parametrize("seed", [1])
def test_query_files(seed):
    MC.check_queries(emu_run, seed)


def test_region_tables():
    MC.check_regions(emu_run)


def test_around_the_tile_limit():
    MC.check_tile_limit(emu_run, lds_samples)
    MC.check_device_tile_limit(emu_device, lds_samples)


def test_bad_headers():
    data = D.valid_files(1)[2][1]
    for layout in MC.LAYOUTS:
        assert emu_run(data[1:], layout) == (E_FORMAT, [], [], None, MC.NO_RECORD) == MC.matrix(data[1:], layout)
    s0 = next(d for n, d in D.mutated_files(3) if n == "S0_row")
    assert emu_run(s0, MC.BED)[0] == E_ARG == MC.matrix(s0, MC.BED)[0]
    assert emu_run(data, 3)[0] == E_ARG


def test_device_entry():
    MC.check_device(emu_device)


def test_device_entry_arguments():
    MC.check_device_args(emu_device, lib().emu_matrix_workspace_size)


# ---- the grid's later trips and the stager's edges (reader_edge_cases.py) ----------

def trip_records(layout):
    L = lib()
    L.emu_matrix_trip_records.restype = ctypes.c_uint64
    L.emu_matrix_trip_records.argtypes = [ctypes.c_int]
    return L.emu_matrix_trip_records(layout)


def test_trip_records():
    """The emulator reports 4 CUs: five blocks a CU, four waves a block, 16
    records a wave; 0 for a layout there is none of."""
    assert [trip_records(k) for k in (0, 1, 2, 3)] == [1280, 1280, 1280, 0]


@pytest.mark.parametrize("layout", MC.LAYOUTS)
def test_second_trip(layout):
    assert RE.check_matrix_trip(emu_device, trip_records, layout) == 1280 + 53


def test_second_trip_irregular_records():
    RE.check_matrix_trip_irregular(emu_device, trip_records)


@pytest.mark.parametrize("fam", RE.FAMILIES)
def test_stager_edges(fam):
    RE.check_edges_matrix(emu_run, fam)
