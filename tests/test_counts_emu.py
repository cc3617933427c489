"""genotype-counts on the CPU: the Python restatement
(counts_cases.py) pinned to a literal GT table and to the oracle -- a plain
tally over the reference's own decode / query --, then the product kernels
(csrc/vcfc_counts.hip) and host driver (csrc/vcfc_counts_driver.h) compiled
against the fiber SIMT emulator, held to the restatement: status, failing
record, indices, rows, the sample table and both renderings, all exact.
test_gpu_counts.py repeats it on the GPU."""
import ctypes

import numpy as np
import pytest

import counts_cases as CC
import decode_cases as D
import emu_io as E
import golden_io as G
import reader_edge_cases as RE
import subset_cases as SC

OK, E_ARG, E_FORMAT = CC.OK, CC.E_ARG, CC.E_FORMAT
NO_ERROR = (1 << 64) - 1
_lib = None


def lib():
    """The emulator build of the counts kernels and driver (flags as tests/simt_emu/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    L = E.build_emu_lib("counts", ("vcfc_counts.hip", "vcfc_decode.hip", "vcfc_encode.hip"), "emu_counts_api.cpp")
    vp, u64, cp, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int
    pu64 = ctypes.POINTER(u64)
    L.emu_counts_lds_samples.restype = u64
    L.emu_counts_workspace_size.restype = u64
    L.emu_counts_workspace_size.argtypes = [u64, u64]
    L.emu_counts_file.argtypes = [cp, u64, ci, cp, u64, ci, u64, u64, u64, vp, vp, u64, pu64, vp, pu64, pu64, vp, pu64,
                                  vp, pu64, u64]
    L.emu_counts_device.argtypes = [cp, vp, vp, u64, u64, vp, vp, vp, u64, vp]
    _lib = L
    return L


def emu_run(data, query, rec_batch=1 << 22, texts=True):
    """emu_counts_file: (status, indices, rows, samples or None, failing
    record); the two renderings are held to the restatement's on the way."""
    h = SC.parse_header(data)
    S = h[1] if h else 1
    cap = len(SC.hop(data[h[0]:])[0]) if h else 1
    idx = np.zeros(cap + 1, dtype=np.uint64)
    rows = np.zeros((cap + 1, 8), dtype=np.uint32)
    samples = np.zeros((max(S, 1), 5), dtype=np.uint64)
    tcap = 64 * (cap + 1) + 48 * max(S, 1) + len(data) + 256
    vt, stx = np.zeros(tcap, dtype=np.uint8), np.zeros(tcap, dtype=np.uint8)
    n, ns, bad, vl, sl = (ctypes.c_uint64(0) for _ in range(5))
    q = query or (b"", False, 0, 0)
    st = lib().emu_counts_file(data, len(data), int(query is not None), q[0], len(q[0]), int(q[1]), q[2], q[3], rec_batch,
                               idx.ctypes.data, rows.ctypes.data, cap + 1, ctypes.byref(n), samples.ctypes.data,
                               ctypes.byref(ns), ctypes.byref(bad), vt.ctypes.data, ctypes.byref(vl), stx.ctypes.data,
                               ctypes.byref(sl), tcap)
    got = (st, [int(x) for x in idx[:n.value]], rows[:n.value].tolist(),
           samples.tolist() if st == OK else None, bad.value)
    if texts and st in (OK, E_FORMAT) and h and 0 < S < 1 << 30:
        assert vt[:vl.value].tobytes() == CC.variants_tsv(data, got[1], got[2])
        assert stx[:sl.value].tobytes() == (CC.samples_tsv(data, got[3]) if st == OK else b"")
    return got


def records_of(data):
    h, S = SC.parse_header(data)
    body = data[h:]
    rec, end = SC.hop(body)
    return body, rec + [end], S


def emu_device(data, select=None, variant=True, sample=True, S=None, ws_short=0, sample_init=None, calls=1):
    """emu_counts_device on the records of a well-formed file: (status, err
    word, rows or None, sample table or None)."""
    body, rec, S0 = records_of(data)
    S = S0 if S is None else S
    n = len(rec) - 1
    r = np.array(rec, dtype=np.uint64)
    sel = None if select is None else np.array(select, dtype=np.uint8)
    rows = np.full((n + 1, 8), 0xEEEEEEEE, dtype=np.uint32)
    Sa = min(S, 1 << 12) if S else 1
    tab = np.zeros((Sa + 1, 5), dtype=np.uint64) if sample_init is None else np.array(sample_init + [[0] * 5], dtype=np.uint64)
    tab[Sa] = 0xEE
    wsb = lib().emu_counts_workspace_size(n, Sa) - ws_short
    ws = np.full(wsb + 64, 0xCD, dtype=np.uint8)
    err = np.zeros(1, dtype=np.uint64)
    for _ in range(calls):
        st = lib().emu_counts_device(body, r.ctypes.data, None if sel is None else sel.ctypes.data, n, S,
                                     rows.ctypes.data if variant else None, tab.ctypes.data if sample else None,
                                     ws.ctypes.data, wsb, err.ctypes.data)
    assert (rows[n] == 0xEEEEEEEE).all() and (tab[Sa] == 0xEE).all() and (ws[wsb:] == 0xCD).all(), "written past an end"
    return st, int(err[0]), rows[:n].tolist() if variant else None, tab[:Sa].tolist() if sample else None


# ---- the restatement against what it restates (no kernel) ----------------------

def test_gt_rule_is_the_literal_table():
    assert len(CC.GT_TABLE) == 25 and len({t for t, _ in CC.GT_TABLE}) == 25
    for tok, want in CC.GT_TABLE:
        assert CC.gt(tok) == want, tok
    assert [CC.CLASS.get(t, 4) for t, _ in CC.GT_TABLE[:6]] == [0, 1, 2, 3, 4, 4]
    assert CC.row([b"0|0", b"1|1", b"2|1", b"./.", b"0|1:7"]) == [1, 0, 0, 1, 3, 8, 4, 1]


def oracle_tally(data, query=None):
    if query is None:
        st, text = G.oracle_decompress(data, cap=len(data) * 40 + 4096)
    else:
        st, text = G.oracle_query(data, SC.query_string(query))
    assert st == 0
    return CC.tally_vcf(text)


@pytest.mark.parametrize("seed", [1])
def test_restatement_is_a_tally_of_the_oracle_decode(seed):
    for name, data in D.valid_files(seed):
        st, idx, rows, samples = CC.counts(data)
        want_rows, want_samples = oracle_tally(data)
        assert st == OK and idx == list(range(len(rows))), name
        assert [r[:5] for r in rows] == want_rows and samples == want_samples, name


@pytest.mark.parametrize("name", ["random_100x10000", "fuzz_decode"])
def test_restatement_on_golden_files(name):
    data = G.gz(name + ".vcfc.gz")
    st, idx, rows, samples = CC.counts(data)
    want_rows, want_samples = oracle_tally(data)
    assert st == OK and [r[:5] for r in rows] == want_rows and samples == want_samples
    assert (want_rows, want_samples) == CC.tally_vcf(G.gz(name + ".vcf.gz"))


def parse_query(qs):
    ref, _, rng = qs.partition(b":")
    return (ref, True, *(int(x) for x in rng.split(b"-"))) if rng else (ref, False, 0, 0)


@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_query_is_a_tally_of_the_oracle_query(seed):
    """decode_cases.query_files: POS fields with blanks, signs and leading
    zeros.  The valid file under every query; the mutated ones wherever both
    sides run through (elsewhere the reference's walk leaves the LEN hops,
    where this definition stops)."""
    hits = both = 0
    for name, data, queries in D.query_files(seed):
        for qs in queries:
            q = parse_query(qs)
            got = CC.counts(data, q)
            st, text = G.oracle_query(data, qs)
            assert name != "mixed" or (got[0] == OK and st == 0), qs
            if got[0] == OK and st == 0:
                want_rows, want_samples = CC.tally_vcf(text)
                assert [r[:5] for r in got[2]] == want_rows, (name, qs)
                assert got[3] == (want_samples or [[0] * 5 for _ in range(len(got[3]))]), (name, qs)
                both += 1
                hits += len(want_rows) > 0
    assert both >= 7 and hits >= 5, (both, hits)   # the valid file's seven queries at the least
    name, data = SC.query_files(seed)[0]   # on plain decimal POS fields the two match rules are one
    body, rec, S = records_of(data)
    for q in SC.QUERIES:
        assert all(CC.match(body, rec[i], rec[i + 1], *q) == SC.match(body, rec[i], rec[i + 1], *q)
                   for i in range(len(rec) - 1))


# ---- the kernels and driver on the emulator -------------------------------------

def test_lds_limit_is_what_the_header_says():
    assert lib().emu_counts_lds_samples() == 2560


@pytest.mark.parametrize("seed", [1])
def test_valid_files(seed):
    CC.check_files(emu_run, D.valid_files(seed))


def test_batch_sizes():
    CC.check_files(emu_run, SC.batch_files())
    for name, data in SC.batch_files():   # the driver's record batches: one record each, seven, all
        for rb in (1, 7):
            CC.same(emu_run(data, None, rec_batch=rb), CC.counts_full(data), (name, rb))


def test_hand_built_records():
    CC.check_hand_built(emu_run)


@pytest.mark.parametrize("seed", [3, 4, 6])
def test_mutated_files(seed):
    CC.check_mutated(emu_run, seed)


@pytest.mark.parametrize("seed", [1])
def test_query_files(seed):
    CC.check_queries(emu_run, seed)


def test_around_the_lds_limit():
    L = lib().emu_counts_lds_samples()
    files = CC.lds_limit_files(L)
    assert [SC.parse_header(d)[1] for _, d in files] == [L - 1, L, L + 1]
    for name, data in files:
        want = CC.counts_full(data)
        assert want[0] == OK and len(want[1]) == 6
        S = L - 1 + files.index((name, data))
        assert want[3][S - 1] == [1, 5, 0, 0, 0] and [r[4] for r in want[3][S - 32:S - 27]] == [1] * 5, name   # the last column; the escapes
        CC.same(emu_run(data, None), want, name)


def test_wide_records():
    files = CC.wide_files()
    assert [SC.parse_header(d)[1] for _, d in files] == [32767, 32768]
    assert CC.counts(files[1][1])[2][1] == [60, 8, 32698, 0, 2, 2 * 32768 - 4 + 2, 32698 + 8 + 0, 2]
    CC.check_files(emu_run, files)


def test_lost_updates():
    CC.check_lost_updates(emu_run)


def test_bad_headers():
    data = D.valid_files(1)[2][1]
    assert emu_run(data[1:], None) == (E_FORMAT, [], [], None, NO_ERROR)
    assert emu_run(D.header(3), None) == (E_FORMAT, [], [], None, NO_ERROR)   # no data line at all: parse_header's rule
    s0 = next(d for n, d in D.mutated_files(3) if n == "S0_row")
    assert emu_run(s0, None) == (E_ARG, [], [], None, NO_ERROR) == CC.counts_full(s0)


def select_cases(n):
    return [None, [1] * n, [int(i % 8 == 0) for i in range(n)], [0] * n]


def test_device_entry():
    name, data = SC.batch_files()[4]   # 41 records, S = 70
    st, idx, rows, samples = CC.counts(data)
    n = len(rows)
    zero = [0] * 8
    for sel in select_cases(n):
        on = [sel is None or sel[i] for i in range(n)]
        want_rows = [r if on[i] else zero for i, r in enumerate(rows)]
        body, rec, S = records_of(data)
        want_tab = [[0] * 5 for _ in range(S)]
        for i in range(n):
            if on[i]:
                for j, t in enumerate(SC.regular(body, rec[i], rec[i + 1], S)[1]):
                    want_tab[j][CC.CLASS.get(t, 4)] += 1
        assert emu_device(data, sel) == (OK, NO_ERROR, want_rows, want_tab), sel
        assert emu_device(data, sel, sample=False) == (OK, NO_ERROR, want_rows, None), sel
        assert emu_device(data, sel, variant=False) == (OK, NO_ERROR, None, want_tab), sel
        assert emu_device(data, sel, variant=False, sample=False)[0] == E_ARG
        # d_sample is added to: twice without zeroing doubles the table, the rows stay
        twice = emu_device(data, sel, calls=2)
        assert twice == (OK, NO_ERROR, want_rows, [[2 * x for x in r] for r in want_tab]), sel
        seeded = emu_device(data, sel, sample_init=[[7, 1, 2, 3, 4]] * S)
        assert seeded[3] == [[a + b for a, b in zip(r, [7, 1, 2, 3, 4])] for r in want_tab], sel
    assert emu_device(data, ws_short=1)[0] == E_ARG
    assert emu_device(data, S=0)[0] == E_ARG and emu_device(data, S=1 << 30)[0] == E_ARG


def test_device_entry_irregular_record_only_where_selected():
    name, data = next(x for x in SC.query_files(1) if x[0] == "no_lf17")
    st, idx, rows, samples, bad = CC.counts_full(data)
    assert (st, bad, len(rows)) == (E_FORMAT, 17, 17)
    st, err, got, tab = emu_device(data)
    assert (st, err) == (OK, (17 << 8) | 3) and got[:17] == rows
    n = len(records_of(data)[1]) - 1
    st, err, got, tab = emu_device(data, [int(i != 17) for i in range(n)])
    assert (st, err) == (OK, NO_ERROR) and got[:17] == rows and got[17] == [0] * 8
    assert [sum(r) for r in tab] == [n - 1] * 40


# ---- the grid's later trips and the stager's edges (reader_edge_cases.py) ----------

def emu_device_records(body, rec, S, select, variant, sample, calls):
    """emu_counts_device on the records body[rec[i], rec[i + 1]) (rec: an
    array of n + 1 offsets): (status, err word, rows or None, sample table or
    None), as arrays."""
    n = len(rec) - 1
    r = np.ascontiguousarray(rec, dtype=np.uint64)
    rows = np.full((n + 1, 8), 0xEEEEEEEE, dtype=np.uint32)
    tab = np.zeros((S + 1, 5), dtype=np.uint64)
    tab[S] = 0xEE
    wsb = lib().emu_counts_workspace_size(n, S)
    ws = np.full(wsb + 64, 0xCD, dtype=np.uint8)
    err = np.zeros(1, dtype=np.uint64)
    for _ in range(calls):
        st = lib().emu_counts_device(body, r.ctypes.data, None if select is None else select.ctypes.data, n, S,
                                     rows.ctypes.data if variant else None, tab.ctypes.data if sample else None,
                                     ws.ctypes.data, wsb, err.ctypes.data)
    assert (rows[n] == 0xEEEEEEEE).all() and (tab[S] == 0xEE).all() and (ws[wsb:] == 0xCD).all(), "written past an end"
    return st, int(err[0]), rows[:n] if variant else None, tab[:S] if sample else None


def trip_records(S, with_sample_table):
    L = lib()
    L.emu_counts_trip_records.restype = ctypes.c_uint64
    L.emu_counts_trip_records.argtypes = [ctypes.c_uint64, ctypes.c_int]
    return L.emu_counts_trip_records(S, int(with_sample_table))


def test_trip_records():
    """The emulator reports 4 CUs: two blocks a CU with the LDS tile, four
    without, eight waves a block, 16 records a wave."""
    L = lib().emu_counts_lds_samples()
    assert [trip_records(5, True), trip_records(L, True), trip_records(L + 1, True), trip_records(5, False)] == \
        [1024, 1024, 2048, 2048]


def test_second_trip_lds():
    assert RE.check_counts_trip(emu_device_records, trip_records, 5, True, True) == 1024 + 53


def test_second_trip_no_table():
    assert RE.check_counts_trip(emu_device_records, trip_records, 5, True, False) == 2048 + 53


def test_second_trip_global():
    L = lib().emu_counts_lds_samples()
    RE.check_counts_trip(emu_device_records, trip_records, L + 1, False, True, L=L)


def test_second_trip_irregular_records():
    RE.check_counts_trip_irregular(emu_device_records, trip_records)


@pytest.mark.parametrize("fam", RE.FAMILIES)
def test_stager_edges(fam):
    RE.check_edges_counts(lambda data, q: emu_run(data, q, texts=False), fam)
