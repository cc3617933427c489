"""extract (extract-samples, extract-regions) on the CPU: the
Python restatement (extract_cases.py) pinned to the oracle -- its output is the
oracle's compress of the cut of the oracle's decode, and with all columns the
input itself -- and to digests of the reference CLI's own output, then the
product kernels (csrc/vcfc_extract.hip) and host driver
(csrc/vcfc_extract_driver.h) compiled against the fiber SIMT emulator, held to
the restatement: whole bytes, status, error word and offsets.
test_gpu_extract.py repeats it on the GPU."""
import ctypes

import numpy as np
import pytest

import decode_cases as D
import emu_io as E
import extract_cases as EC
import golden_io as G
import reader_edge_cases as RE
import subset_cases as SC

OK, E_NOSPACE, E_ARG, E_FORMAT = EC.OK, EC.E_NOSPACE, EC.E_ARG, EC.E_FORMAT
_lib = None


def lib():
    """The emulator build of the extract kernels and driver (flags as tests/simt_emu/Makefile)."""
    global _lib
    if _lib is not None:
        return _lib
    L = E.build_emu_lib("extract", ("vcfc_extract.hip", "vcfc_regions.hip", "vcfc_decode.hip", "vcfc_encode.hip"),
                        "emu_extract_api.cpp")
    vp, u64, cp, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int
    pu64 = ctypes.POINTER(u64)
    L.emu_extract_bound.restype = u64
    L.emu_extract_bound.argtypes = [u64, u64, u64]
    L.emu_extract_tile.restype = u64
    L.emu_regions_build.argtypes = [cp, u64, vp, u64, pu64, pu64, pu64]
    L.emu_extract.argtypes = [cp, u64, vp, u64, ci, cp, u64, ci, u64, u64, cp, u64, vp, u64, pu64, u64]
    L.emu_extract_device.argtypes = [cp, vp, vp, u64, u64, vp, u64, vp, u64, vp, vp]
    _lib = L
    return L


def table_of(text):
    nb, nr, bad = (ctypes.c_uint64(0) for _ in range(3))
    st = lib().emu_regions_build(text, len(text), None, 0, ctypes.byref(nb), ctypes.byref(nr), ctypes.byref(bad))
    assert st == E_NOSPACE, st
    out = np.zeros(nb.value, dtype=np.uint8)
    st = lib().emu_regions_build(text, len(text), out.ctypes.data, nb.value, ctypes.byref(nb), ctypes.byref(nr),
                                 ctypes.byref(bad))
    assert st == OK
    return out.tobytes()


def emu_ext(data, cols=None, query=None, regions=None, out_batch=1 << 16):
    c = None if cols is None else np.array(cols, dtype=np.uint32)
    if c is not None and len(c) == 0:
        c = np.zeros(1, dtype=np.uint32)   # a list with no column: a pointer, and K = 0
    h = SC.parse_header(data)
    nrec = len(SC.hop(data[h[0]:])[0]) if h else 0
    cap = lib().emu_extract_bound(len(data), nrec, h[1] if h else 0) + 64
    out = np.zeros(cap, dtype=np.uint8)
    n = ctypes.c_uint64(0)
    q = query or (b"", False, 0, 0)
    table = table_of(regions) if regions is not None else b""
    st = lib().emu_extract(data, len(data), None if c is None else c.ctypes.data, 0 if cols is None else len(cols),
                           1 if query is not None else 2 if regions is not None else 0, q[0], len(q[0]), int(q[1]), q[2],
                           q[3], table, len(table), out.ctypes.data, cap, ctypes.byref(n), out_batch)
    return st, out[:n.value].tobytes()


def emu_device(data, cols, select, cap, base):
    """(status, err word, record offsets, out bytes); bytes before the output
    base and past out_cap keep their fill."""
    h, S = SC.parse_header(data)
    body = data[h:]
    rec, end = SC.hop(body)
    n = len(rec)
    r = np.array(rec + [end], dtype=np.uint64)
    c = None if cols is None else np.array(cols if cols else [0], dtype=np.uint32)
    sel = None if select is None else np.array(select, dtype=np.uint8)
    total = lib().emu_extract_bound(len(body), n, S if cols is None else len(cols)) if cap is None else cap
    buf = np.full(16 + total + 64, 0xEE, dtype=np.uint8)
    out = buf[base:]
    roff = np.zeros(n + 1, dtype=np.uint64)
    err = np.zeros(1, dtype=np.uint64)
    st = lib().emu_extract_device(body, r.ctypes.data, None if sel is None else sel.ctypes.data, n, S,
                                  None if c is None else c.ctypes.data, 0 if cols is None else len(cols),
                                  out.ctypes.data, total, roff.ctypes.data, err.ctypes.data)
    assert (buf[:base] == 0xEE).all() and (out[total:] == 0xEE).all(), "bytes written outside [out, out + out_cap)"
    if st == OK:
        used = int(max(x for x in roff if x <= total)) if cap is not None else int(roff[-1])
        assert (out[used:total] == 0xEE).all(), "bytes written past the last record that fits"
    return st, int(err[0]), [int(x) for x in roff], out[:total].tobytes()


# ---- the restatement against the oracle (no kernel) --------------------------

@pytest.mark.parametrize("seed", [0, 1])
def test_restatement_is_the_oracle_compress_of_the_cut(seed):
    for name, data in D.valid_files(seed):
        S = SC.parse_header(data)[1]
        st, vcf = G.oracle_decompress(data, cap=len(data) * 40 + 4096)
        assert st == 0
        for cols in SC.column_sets(S, seed):
            if not SC.check_cols(cols, S):   # (S = 1: [S - 1, 0] names column 0 twice)
                assert EC.extract(data, cols) == (E_ARG, b"")
                continue
            st, want, _ = G.oracle_compress(SC.cut_vcf(vcf, cols))
            assert st == 0
            assert EC.extract(data, cols) == (OK, want), (name, cols[:8])
        assert EC.extract(data) == (OK, data), name


def test_restatement_all_columns_returns_the_golden_file():
    data = G.gz("random_100x10000.vcfc.gz")
    assert EC.extract(data) == (OK, data)
    assert EC.extract(data, list(range(100))) == (OK, data)


def test_restatement_on_hand_built_lines_is_the_oracle_encoder():
    """Every accepted hand-built record, line by line, against vcfo_encode_line."""
    n = 0
    for name, data, sets, code in EC.hand_built():
        h, S = SC.parse_header(data)
        b = data[h:]
        rec, end = SC.hop(b)
        for cols in sets:
            for i, rs in enumerate(rec):
                c, got = EC.record(b, rs, (rec + [end])[i + 1], S, cols)
                if c == 0:
                    R, toks = SC.regular(b, rs, (rec + [end])[i + 1], S)
                    st, want = G.oracle_encode_line(SC.line(R, toks, cols)[:-1])
                    assert st == 0 and got == want, (name, cols[:8], i)
                    n += 1
    assert n > 300


def test_restatement_reproduces_the_reference_digests():
    EC.check_golden(lambda data, cols: EC.extract(data, cols))


def test_restatement_outcomes():
    hb = {name: (data, sets, code) for name, data, sets, code in EC.hand_built()}
    assert all(code == 5 for name, (_, _, code) in hb.items() if name.startswith(("req_", "empty_chosen", "empty_last")))
    for name, (data, sets, code) in hb.items():
        err, off, recs = EC.device(data, sets[0])
        assert (err == EC.NO_ERROR) == (code == 0) and (code == 0 or err == (1 << 8) | code), name


# ---- the kernels and driver on the emulator -------------------------------------

def test_valid_files():
    EC.check_files(emu_ext, D.valid_files(1), 1)


@pytest.mark.parametrize("seed", [3, 4, 6])
def test_mutated_files(seed):
    EC.check_files(emu_ext, D.mutated_files(seed), seed, short=seed != 3)


def test_hand_built_records():
    EC.check_hand_built(emu_ext)
    assert lib().emu_extract_tile() == EC.TILE


def test_batch_sizes():
    EC.check_files(emu_ext, SC.batch_files())
    for name, data in SC.batch_files():   # one output batch per record, and one for all
        for ob in (1, 1 << 30):
            assert emu_ext(data, [69, 0, 33], out_batch=ob) == EC.extract(data, [69, 0, 33]), (name, ob)


def test_batch_boundary():
    """A batch takes records while their total is at most out_batch (the
    output's bytes do not show it, the pieces sunk do): two records, out_batch
    their total, are one piece behind the header; one byte less, two."""
    data = D.valid_files(1)[2][1]   # S = 64
    h = SC.parse_header(data)[0]
    two = data[:h + SC.hop(data[h:])[0][2]]
    st, want = EC.extract(two, [5, 2])
    body = len(want) - SC.parse_header(want)[0]
    assert st == OK and len(SC.hop(want[len(want) - body:])[0]) == 2
    for ob, pieces in ((body, 2), (body - 1, 3)):
        assert emu_ext(two, [5, 2], out_batch=ob) == (st, want)
        assert lib().emu_extract_sink_calls() == pieces, ob


def test_query_files_and_region_tables():
    EC.check_queries(emu_ext, 1)


def test_golden_file_head():
    """The first 150 records of the golden file (the digests of the whole file: the restatement above, and the GPU)."""
    data = G.gz("random_100x10000.vcfc.gz")
    h = SC.parse_header(data)[0]
    head = data[:h + SC.hop(data[h:])[0][150]]
    for cols in (None, list(range(99, -1, -1)), EC.golden_columns({"sample": [2, 64]}, 100)):
        assert emu_ext(head, cols) == EC.extract(head, cols)
    assert emu_ext(head) == (OK, head)


def test_bad_arguments():
    data = D.valid_files(1)[2][1]   # S = 64
    for cols in ([], [64], [0, 64], [3, 3], [5, 1, 5]):
        assert emu_ext(data, cols) == (E_ARG, b"") and emu_ext(data, cols, query=SC.QUERIES[0]) == (E_ARG, b""), cols
    assert emu_ext(data[1:], [0]) == (E_FORMAT, b"") and emu_ext(data[1:]) == (E_FORMAT, b"")
    assert emu_ext(D.header(3), [0]) == (E_FORMAT, b"")   # no data line at all: parse_header's rule


def test_device_entry():
    EC.check_device(emu_device)


def test_bound():
    EC.check_bound(lambda a, b, c: lib().emu_extract_bound(a, b, c))


# ---- the byte-serial lanes' later passes and the stager's edges (reader_edge_cases.py) ----

def workspace_size(n, K):
    L = lib()
    L.emu_extract_workspace_size.restype = ctypes.c_uint64
    L.emu_extract_workspace_size.argtypes = [ctypes.c_uint64, ctypes.c_uint64]
    return L.emu_extract_workspace_size(n, K)


@pytest.mark.parametrize("cols", RE.QUEUE_COLS[1:3])
def test_queue_pass(cols):
    """Output batches of 700 bytes and one batch."""
    assert RE.check_queue_is_longer_than_the_lanes(workspace_size, 2) == 1024
    exts = [lambda data, cols, ob=ob: emu_ext(data, cols, out_batch=ob) for ob in (700, 1 << 30)]
    RE.check_queue_extract(exts, emu_device, [cols])


@pytest.mark.parametrize("fam", RE.FAMILIES)
def test_stager_edges(fam):
    RE.check_edges_extract(emu_ext, fam)
