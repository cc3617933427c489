"""Sample-subset decode (decompress-samples, query-samples) on
the CPU: the Python restatement (subset_cases.py) pinned to the oracle -- with
all columns it is the reference's own decode / query --, then the product
kernels (csrc/vcfc_subset.hip) and host driver (csrc/vcfc_subset_driver.h)
compiled against the fiber SIMT emulator, held to the restatement: whole
bytes and status.  test_gpu_subset.py repeats it on the GPU."""
import ctypes

import numpy as np
import pytest

import decode_cases as D
import emu_io as E
import golden_io as G
import reader_edge_cases as RE
import subset_cases as SC

OK, E_ARG, E_FORMAT = SC.OK, SC.E_ARG, SC.E_FORMAT
NO_ERROR = (1 << 64) - 1
_lib = None


def lib():
    """The emulator build of the subset kernels and driver (flags as tests/simt_emu/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    L = E.build_emu_lib("subset", ("vcfc_subset.hip", "vcfc_decode.hip", "vcfc_encode.hip"), "emu_subset_api.cpp")
    vp, u64, cp = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p
    pu64 = ctypes.POINTER(u64)
    L.emu_subset_decompress.argtypes = [cp, u64, vp, u64, vp, u64, pu64, u64]
    L.emu_subset_query.argtypes = [cp, u64, cp, u64, ctypes.c_int, u64, u64, vp, u64, vp, u64, pu64, u64]
    L.emu_subset_device.argtypes = [cp, vp, vp, u64, u64, vp, u64, vp, u64, vp, vp]
    L.emu_sample_columns.argtypes = [cp, u64, cp, u64, vp, u64, pu64, pu64]
    _lib = L
    return L


def emu_dec(data, cols, out_batch=1 << 14, cap=None):
    c = np.array(cols, dtype=np.uint32)
    cap = len(data) * 8 + 4096 if cap is None else cap
    out = np.zeros(cap, dtype=np.uint8)
    n = ctypes.c_uint64(0)
    st = lib().emu_subset_decompress(data, len(data), c.ctypes.data, len(cols), out.ctypes.data, cap, ctypes.byref(n),
                                     out_batch)
    return st, out[:n.value].tobytes()


def emu_qry(data, q, cols, out_batch=1 << 12):
    c = np.array(cols, dtype=np.uint32)
    cap = len(data) * 8 + 4096
    out = np.zeros(cap, dtype=np.uint8)
    n = ctypes.c_uint64(0)
    st = lib().emu_subset_query(data, len(data), q[0], len(q[0]), int(q[1]), q[2], q[3], c.ctypes.data, len(cols),
                                out.ctypes.data, cap, ctypes.byref(n), out_batch)
    return st, out[:n.value].tobytes()


def emu_device(data, cols, select=None, cap=None):
    """The device entry's kernels on the records of a well-formed file:
    (status, err word, line offsets, out bytes, bytes past out_cap untouched)."""
    h, S = SC.parse_header(data)
    body = data[h:]
    rec, end = SC.hop(body)
    n = len(rec)
    r = np.array(rec + [end], dtype=np.uint64)
    c = np.array(cols, dtype=np.uint32)
    sel = None if select is None else np.array(select, dtype=np.uint8)
    total = len(body) * 8 + 64 if cap is None else cap
    out = np.full(total + 64, 0xEE, dtype=np.uint8)
    loff = np.zeros(n + 1, dtype=np.uint64)
    err = np.zeros(1, dtype=np.uint64)
    st = lib().emu_subset_device(body, r.ctypes.data, None if sel is None else sel.ctypes.data, n, S, c.ctypes.data,
                                 len(cols), out.ctypes.data, total, loff.ctypes.data, err.ctypes.data)
    assert (out[total:] == 0xEE).all(), "bytes written past out_cap"
    return st, int(err[0]), [int(x) for x in loff], out[:total].tobytes()


# ---- the restatement against the oracle (no kernel) --------------------------

@pytest.mark.parametrize("seed", [1, 2, 5])
def test_restatement_all_columns_is_the_oracle_decode(seed):
    for name, data in D.valid_files(seed):
        S = SC.parse_header(data)[1]
        st, want = G.oracle_decompress(data, cap=len(data) * 40 + 4096)
        assert st == 0
        assert SC.subset(data, list(range(S))) == (OK, want), name


@pytest.mark.parametrize("name", ["random_100x10000", "fuzz_decode"])
def test_restatement_reproduces_golden_files(name):
    data = G.gz(name + ".vcfc.gz")
    S = SC.parse_header(data)[1]
    assert SC.subset(data, list(range(S))) == (OK, G.gz(name + ".vcf.gz"))
    cols = [S - 1, 0, S // 2]
    assert SC.subset(data, cols) == (OK, SC.cut_vcf(G.gz(name + ".vcf.gz"), cols))


@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_query_all_columns_is_the_oracle_query(seed):
    name, data = SC.query_files(seed)[0]
    assert name == "valid"
    for q in SC.QUERIES:
        st, want = G.oracle_query(data, SC.query_string(q))
        assert st == 0
        assert SC.subset_query(data, q, list(range(40))) == (OK, want), q
    assert sum(len(SC.subset_query(data, q, [0])[1]) > 0 for q in SC.QUERIES) >= 5


@pytest.mark.parametrize("seed,counts", [(3, (9, 20, 9)), (4, (11, 18, 9)), (6, (12, 17, 9))])
def test_restatement_outcomes_on_mutated_files(seed, counts):
    """OK / stop after at least one line / stop before any line (S0_row
    declares no sample: there is no column to ask for)."""
    ok = part = none = 0
    for name, data in D.mutated_files(seed):
        h = SC.parse_header(data)
        if h is not None and h[1] == 0:
            assert name == "S0_row" and SC.subset(data, [0]) == (E_ARG, b"")
            continue
        st, out = SC.subset(data, [0])
        if st == OK:
            ok += 1
        elif h is not None and st == E_FORMAT and out.count(b"\n") > data[:h[0]].count(b"\n"):
            part += 1
        else:
            none += 1
    assert (ok, part, none) == counts


# ---- the kernels and driver on the emulator -------------------------------------

@pytest.mark.parametrize("seed", [1])
def test_valid_files(seed):
    SC.check_files(emu_dec, D.valid_files(seed), seed)


@pytest.mark.parametrize("seed", [3, 4, 6])
def test_mutated_files(seed):
    SC.check_mutated(emu_dec, seed)


def test_hand_built_records():
    SC.check_hand_built(emu_dec)


def test_batch_sizes():
    SC.check_files(emu_dec, SC.batch_files())
    for name, data in SC.batch_files():   # one output batch per line, and one for all
        for ob in (1, 1 << 30):
            assert emu_dec(data, [69, 0, 33], out_batch=ob) == SC.subset(data, [69, 0, 33]), (name, ob)


def test_batch_boundary():
    """A batch takes lines while their total is at most out_batch (the output's
    bytes do not show it, the pieces sunk do): two lines, out_batch their
    total, are one piece behind the header; one byte less, two."""
    data = D.valid_files(1)[2][1]   # S = 64
    h = SC.parse_header(data)[0]
    two = data[:h + SC.hop(data[h:])[0][2]]
    st, want = SC.subset(two, [5, 2])
    lines = want[want.index(b"\n#CHROM"):].split(b"\n", 2)[2]
    assert st == OK and lines.count(b"\n") == 2
    for ob, pieces in ((len(lines), 2), (len(lines) - 1, 3)):
        assert emu_dec(two, [5, 2], out_batch=ob) == (st, want)
        assert lib().emu_subset_sink_calls() == pieces, ob


@pytest.mark.parametrize("seed", [1])
def test_query_files(seed):
    SC.check_queries(emu_qry, seed)


def test_bad_arguments():
    data = D.valid_files(1)[2][1]   # S = 64
    for cols in ([], [64], [0, 64], [3, 3], [5, 1, 5]):
        assert emu_dec(data, cols) == (E_ARG, b"") and emu_qry(data, SC.QUERIES[0], cols) == (E_ARG, b""), cols
    assert emu_dec(data[1:], [0]) == (E_FORMAT, b"")   # a header the decoder refuses
    assert emu_dec(D.header(3), [0]) == (E_FORMAT, b"")   # no data line at all: parse_header's rule


def select_cases(n):
    return [[0] * n, [1] * n, [int(i % 8 == 0) for i in range(n)], [int(i % 8 == 3 or i == n - 1) for i in range(n)]]


def test_device_entry():
    name, data = SC.batch_files()[4]   # 41 records, S = 70
    h, S = SC.parse_header(data)
    body = data[h:]
    rec, end = SC.hop(body)
    n = len(rec)
    for cols in ([0], [69, 0, 33], list(range(70))):
        lines = [SC.line(*SC.regular(body, rec[i], (rec + [end])[i + 1], S), cols) for i in range(n)]
        for sel in [None] + select_cases(n):
            want = [l if sel is None or sel[i] else b"" for i, l in enumerate(lines)]
            off = [0]
            for l in want:
                off.append(off[-1] + len(l))
            st, err, loff, out = emu_device(data, cols, sel)
            assert (st, err) == (OK, NO_ERROR) and loff == off and out[:off[-1]] == b"".join(want), (cols[:4], sel)
            if off[-1]:   # one byte short: the first line that does not fit
                st, err, loff, out = emu_device(data, cols, sel, cap=off[-1] - 1)
                first = next(i for i in range(n) if off[i + 1] > off[-1] - 1)
                assert (st, err) == (OK, (first << 8) | 0xFF) and loff == off, (cols[:4], sel, hex(err))
    for cols in ([], [70], [1, 1]):
        assert emu_device(data, cols)[0] == E_ARG


def test_device_entry_irregular_record_only_where_selected():
    name, data = next(x for x in SC.query_files(1) if x[0] == "no_lf17")
    n = len(SC.hop(data[SC.parse_header(data)[0]:])[0])
    st, err, loff, out = emu_device(data, [0, 5])
    assert (st, err) == (OK, (17 << 8) | 3)
    sel = [int(i != 17) for i in range(n)]
    st, err, loff, out = emu_device(data, [0, 5], sel)
    assert (st, err) == (OK, NO_ERROR) and loff[17] == loff[18]


def test_sample_columns():
    data = D.valid_files(1)[2][1]   # samples S0 .. S63

    def resolve(names, cap=64):
        cols = np.zeros(max(cap, 1), dtype=np.uint32)
        n, bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
        st = lib().emu_sample_columns(data, len(data), names, len(names), cols.ctypes.data, cap, ctypes.byref(n),
                                      ctypes.byref(bad))
        return st, [int(x) for x in cols[:min(n.value, cap)]], n.value, bad.value
    assert resolve(b"S5,S0,S63")[:2] == (OK, [5, 0, 63])
    assert resolve(b"S5,S64,S1") == (E_ARG, [], 0, 3)
    assert resolve(b"S5,S1,S5") == (E_ARG, [], 0, 6)
    assert resolve(b"") == (E_ARG, [], 0, 0) and resolve(b"S1,") == (E_ARG, [], 0, 3)
    assert resolve(b"S1,S2,S3", cap=2)[0] == 4 and resolve(b"S1,S2,S3", cap=2)[2] == 3
    rep = data.replace(b"\tS7\t", b"\tS6\t", 1)   # the header repeats S6: the first one wins
    cols = np.zeros(4, dtype=np.uint32)
    n, bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib().emu_sample_columns(rep, len(rep), b"S6", 2, cols.ctypes.data, 4, ctypes.byref(n), ctypes.byref(bad)) == OK
    assert int(cols[0]) == 6


# ---- the writer's later passes and the stager's edges (reader_edge_cases.py) --------

def workspace_size(n, K):
    L = lib()
    L.emu_subset_workspace_size.restype = ctypes.c_uint64
    L.emu_subset_workspace_size.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    return L.emu_subset_workspace_size(n, K)


@pytest.mark.parametrize("cols", RE.QUEUE_COLS[1:3])
def test_queue_pass(cols):
    """Output batches of 700 bytes (a handful of lines each, so a lane's
    second record falls in another batch than its first) and one batch."""
    assert RE.check_queue_is_longer_than_the_lanes(workspace_size, 1) == 1024
    decs = [lambda data, cols, ob=ob: emu_dec(data, cols, out_batch=ob) for ob in (700, 1 << 30)]
    RE.check_queue_subset(decs, emu_device, [cols])


@pytest.mark.parametrize("fam", RE.FAMILIES)
def test_stager_edges(fam):
    RE.check_edges_subset(lambda data, cols: emu_dec(data, cols, cap=D.edge_cap(data)), fam)
