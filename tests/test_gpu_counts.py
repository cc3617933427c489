"""GPU parity for genotype-counts: status, failing record,
indices, rows and the sample table against the Python restatement
(counts_cases.py, pinned to the oracle by test_counts_emu.py) through the C
ABI (libvcfc.so), the device entry on torch tensors and the file call; both
TSV files of the CLI (build/main) byte for byte; and a 2504-sample file
against a Python count of its source VCF text."""
import io
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import counts_cases as CC
import decode_cases as D
import golden_io as G
import reader_edge_cases as RE
import subset_cases as SC

pytestmark = pytest.mark.gpu
REPO = G.REPO
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
MAIN = os.path.join(REPO, "build", "main")
OK, E_ARG, E_FORMAT = CC.OK, CC.E_ARG, CC.E_FORMAT


@pytest.fixture(scope="module")
def ctx():
    import torch   # before libvcfc: one HIP runtime in the process
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import vcfc
    c = vcfc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def run(ctx):
    import vcfc

    def f(data, query):
        st, idx, rows, tab = ctx.genotype_counts_buffer(data, None if query is None else vcfc.VcfCoordinateQuery(*query))
        return st, [int(x) for x in idx], rows.tolist(), None if tab is None else tab.tolist(), ctx.last_counts_record
    return f


def test_valid_files(run):
    CC.check_files(run, D.valid_files(1))


def test_batch_sizes(run):
    CC.check_files(run, SC.batch_files())


def test_hand_built_records(run):
    CC.check_hand_built(run)


@pytest.mark.parametrize("seed", [3, 4, 6])
def test_mutated_files(run, seed):
    CC.check_mutated(run, seed)


@pytest.mark.parametrize("seed", [1])
def test_query_files(run, seed):
    CC.check_queries(run, seed)


def test_around_the_lds_limit(run):
    import vcfc
    L = vcfc.counts_lds_samples()
    assert L == 2560
    CC.check_files(run, CC.lds_limit_files(L))


def test_wide_records(run):
    CC.check_files(run, CC.wide_files())


def test_lost_updates(run):
    CC.check_lost_updates(run)


def test_bad_headers(run):
    data = D.valid_files(1)[2][1]
    assert run(data[1:], None) == (E_FORMAT, [], [], None, CC.NO_RECORD)
    s0 = next(d for n, d in D.mutated_files(3) if n == "S0_row")
    assert run(s0, None) == (E_ARG, [], [], None, CC.NO_RECORD)


def records_of(data):
    h, S = SC.parse_header(data)
    body = data[h:]
    rec, end = SC.hop(body)
    return body, rec + [end], S


def device_run(data, select=None, variant=True, sample=True, S=None, ws_short=0, sample_init=None, calls=1):
    """vcfc_genotype_counts_device on the records of a well-formed file:
    (status, err word, rows or None, sample table or None)."""
    import torch
    import vcfc
    body, rec, S0 = records_of(data)
    S = S0 if S is None else S
    n = len(rec) - 1
    dev = "cuda:0"
    d_in = torch.from_numpy(np.frombuffer(body + bytes(64), dtype=np.uint8).copy()).to(dev)
    d_rec = torch.from_numpy(np.array(rec, dtype=np.int64)).to(dev)
    d_sel = None if select is None else torch.from_numpy(np.array(select, dtype=np.uint8)).to(dev)
    d_rows = torch.full((n + 1, 8), -0x11111112, dtype=torch.int32, device=dev)
    Sa = min(S, 1 << 12) if S else 1
    init = np.zeros((Sa + 1, 5), dtype=np.int64) if sample_init is None else np.array(sample_init + [[0] * 5], dtype=np.int64)
    init[Sa] = 0xEE
    d_tab = torch.from_numpy(init).to(dev)
    wsb = vcfc.counts_workspace_size(n, Sa) - ws_short
    d_ws = torch.full((wsb + 64,), 0xCD, dtype=torch.uint8, device=dev)
    d_err = torch.zeros(1, dtype=torch.int64, device=dev)
    for _ in range(calls):
        st = vcfc.genotype_counts_device(d_in.data_ptr(), len(body), d_rec.data_ptr(), None if d_sel is None else d_sel.data_ptr(),
                                         n, S, d_rows.data_ptr() if variant else None, d_tab.data_ptr() if sample else None,
                                         d_ws.data_ptr(), wsb, d_err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rows = d_rows.cpu().numpy().view(np.uint32)
    tab = d_tab.cpu().numpy()
    assert (rows[n] == 0xEEEEEEEE).all() and (tab[Sa] == 0xEE).all() and (d_ws[wsb:].cpu().numpy() == 0xCD).all(), \
        "written past an end"
    return st, int(d_err.cpu().numpy().view(np.uint64)[0]), rows[:n].tolist() if variant else None, \
        tab[:Sa].tolist() if sample else None


def test_device_entry():
    import vcfc
    name, data = SC.batch_files()[4]   # 41 records, S = 70
    st, idx, rows, samples = CC.counts(data)
    n = len(rows)
    body, rec, S = records_of(data)
    toks = [SC.regular(body, rec[i], rec[i + 1], S)[1] for i in range(n)]
    for sel in (None, [1] * n, [int(i % 8 == 0) for i in range(n)], [0] * n):
        on = [sel is None or sel[i] for i in range(n)]
        want_rows = [r if on[i] else [0] * 8 for i, r in enumerate(rows)]
        want_tab = [[0] * 5 for _ in range(S)]
        for i in range(n):
            if on[i]:
                for j, t in enumerate(toks[i]):
                    want_tab[j][CC.CLASS.get(t, 4)] += 1
        assert device_run(data, sel) == (OK, vcfc.NO_ERROR, want_rows, want_tab), sel
        assert device_run(data, sel, sample=False) == (OK, vcfc.NO_ERROR, want_rows, None), sel
        assert device_run(data, sel, variant=False) == (OK, vcfc.NO_ERROR, None, want_tab), sel
        assert device_run(data, sel, variant=False, sample=False)[0] == E_ARG
        # d_sample is added to: twice without zeroing doubles the table, the rows stay
        assert device_run(data, sel, calls=2) == (OK, vcfc.NO_ERROR, want_rows, [[2 * x for x in r] for r in want_tab]), sel
    assert device_run(data, ws_short=1)[0] == E_ARG
    assert device_run(data, S=0)[0] == E_ARG and device_run(data, S=1 << 30)[0] == E_ARG


def test_device_entry_irregular_record_only_where_selected():
    import vcfc
    name, data = next(x for x in SC.query_files(1) if x[0] == "no_lf17")
    st, idx, rows, samples, bad = CC.counts_full(data)
    assert (st, bad, len(rows)) == (E_FORMAT, 17, 17)
    st, err, got, tab = device_run(data)
    assert (st, err) == (OK, (17 << 8) | 3) and got[:17] == rows
    n = len(records_of(data)[1]) - 1
    st, err, got, tab = device_run(data, [int(i != 17) for i in range(n)])
    assert (st, err) == (OK, vcfc.NO_ERROR) and got[:17] == rows and got[17] == [0] * 8
    assert [sum(r) for r in tab] == [n - 1] * 40


def test_device_entry_above_the_lds_limit():
    """The general path (global atomics) through the device entry, rows off."""
    import vcfc
    name, data = CC.lds_limit_files(vcfc.counts_lds_samples())[2]
    st, idx, rows, samples = CC.counts(data)
    assert device_run(data, variant=False) == (OK, vcfc.NO_ERROR, None, samples)


def cli(argv):
    return subprocess.run([MAIN] + argv, capture_output=True, timeout=300)


def test_file_call_and_cli(ctx):
    import vcfc
    enc = G.gz("random_100x10000.vcfc.gz")
    with tempfile.TemporaryDirectory() as d:
        src, vt, stx = (os.path.join(d, x) for x in ("t.vcfc", "v.tsv", "s.tsv"))
        with open(src, "wb") as f:
            f.write(enc)
        for region in (None, "1:10100-10300", "2"):
            q = None if region is None else tuple(vcfc.parse_coordinate_string(region))
            st, idx, rows, samples = CC.counts(enc, q)
            assert st == OK and (region == "2" or len(idx) > 0)
            want_v, want_s = CC.variants_tsv(enc, idx, rows), CC.samples_tsv(enc, samples)
            r = cli(["genotype-counts", src, vt, stx] + ([] if region is None else [region]))
            assert r.returncode == 0 and r.stdout == b"", r.stderr
            assert open(vt, "rb").read() == want_v and open(stx, "rb").read() == want_s, region
            os.remove(vt)
            ctx.genotype_counts_file(src, vt, stx, region)
            assert open(vt, "rb").read() == want_v and open(stx, "rb").read() == want_s, region
        r = cli(["genotype-counts", src, vt, stx, "1:5"])
        assert r.returncode == 1 and r.stdout == (b"Query must contain a dash character: <ref>:<start>-<end>\n"
                                                  b"Failed to parse query string: 1:5\n")
        for argv in (["genotype-counts", src, vt], []):
            r = cli(argv)
            assert r.returncode == 1
            assert b"./main genotype-counts <input_file> <variants.tsv> <samples.tsv> [<ref>[:<start>-<end>]]\n" in r.stderr
            assert b"./main gap-analysis <compressed-filename>\n" in r.stderr
        # a file that stops mid-way: exit 134, the lines before the stop, an empty samples file
        name, bad = next(x for x in SC.query_files(1) if x[0] == "no_lf17")
        with open(src, "wb") as f:
            f.write(bad)
        st, idx, rows, samples, at = CC.counts_full(bad)
        assert (st, at, len(idx)) == (E_FORMAT, 17, 17)
        r = cli(["genotype-counts", src, vt, stx])
        assert r.returncode == 134 and b"VcfValidationError" in r.stderr and vcfc.strerror(E_FORMAT).encode() in r.stderr
        assert open(vt, "rb").read() == CC.variants_tsv(bad, idx, rows) and open(stx, "rb").read() == b""
        with pytest.raises(RuntimeError, match=vcfc.strerror(E_FORMAT)):
            ctx.genotype_counts_file(src, vt, stx)
        # a header the decoder refuses: both files created, both empty
        with open(src, "wb") as f:
            f.write(enc[1:])
        r = cli(["genotype-counts", src, vt, stx])
        assert r.returncode == 134 and open(vt, "rb").read() == b"" and open(stx, "rb").read() == b""


def test_file_2504_samples(ctx):
    import random_vcf
    buf = io.BytesIO()
    random_vcf.generate(2504, 300, buf)
    vcf = buf.getvalue()
    enc = ctx.compress_buffer(vcf)
    want_rows, want_samples = CC.tally_vcf(vcf)
    st, idx, rows, tab = ctx.genotype_counts_buffer(enc)
    assert st == OK and idx.tolist() == list(range(300))
    assert rows[:, :5].tolist() == want_rows and tab.tolist() == want_samples
    lines = [l.split(b"\t")[9:] for l in vcf.split(b"\n")[:-1] if not l.startswith(b"#")]
    assert rows[:, 5:].tolist() == [CC.row(t)[5:] for t in lines]
    st, idx, rows, tab = ctx.genotype_counts_buffer(enc, "1:%d-%d" % (10000 + 2 * 17, 10000 + 2 * 217))   # POS = 10000 + 2 i
    assert st == OK and idx.tolist() == list(range(17, 218)) and rows[:, :5].tolist() == want_rows[17:218]


# ---- the grid's later trips and the stager's edges (reader_edge_cases.py) ----------

def device_records(body, rec, S, select, variant, sample, calls):
    """vcfc_genotype_counts_device on the records body[rec[i], rec[i + 1])
    (rec: an array of n + 1 offsets): (status, err word, rows or None, sample
    table or None), as arrays."""
    import torch
    import vcfc
    n = len(rec) - 1
    dev = "cuda:0"
    d_in = torch.from_numpy(np.frombuffer(body + bytes(64), dtype=np.uint8).copy()).to(dev)
    d_rec = torch.from_numpy(np.ascontiguousarray(rec, dtype=np.uint64).view(np.int64)).to(dev)
    d_sel = None if select is None else torch.from_numpy(select).to(dev)
    d_rows = torch.full((n + 1, 8), -0x11111112, dtype=torch.int32, device=dev)
    init = np.zeros((S + 1, 5), dtype=np.int64)
    init[S] = 0xEE
    d_tab = torch.from_numpy(init).to(dev)
    wsb = vcfc.counts_workspace_size(n, S)
    d_ws = torch.full((wsb + 64,), 0xCD, dtype=torch.uint8, device=dev)
    d_err = torch.zeros(1, dtype=torch.int64, device=dev)
    for _ in range(calls):
        st = vcfc.genotype_counts_device(d_in.data_ptr(), len(body), d_rec.data_ptr(), None if d_sel is None else d_sel.data_ptr(),
                                         n, S, d_rows.data_ptr() if variant else None, d_tab.data_ptr() if sample else None,
                                         d_ws.data_ptr(), wsb, d_err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rows = d_rows.cpu().numpy().view(np.uint32)
    tab = d_tab.cpu().numpy().view(np.uint64)
    assert (rows[n] == 0xEEEEEEEE).all() and (tab[S] == 0xEE).all() and (d_ws[wsb:].cpu().numpy() == 0xCD).all(), \
        "written past an end"
    return st, int(d_err.cpu().numpy().view(np.uint64)[0]), rows[:n] if variant else None, tab[:S] if sample else None


def trip_records(S, with_sample_table):
    import vcfc
    return vcfc.counts_trip_records(S, with_sample_table)


def test_trip_records():
    """Whole chunks of 16 records on every CU; the LDS tile's grid up to the
    limit, the same grid above it as without a sample table (the emulator suite
    pins the figures)."""
    import torch
    import vcfc
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = vcfc.counts_lds_samples()
    lds, glob, none = trip_records(5, True), trip_records(L + 1, True), trip_records(5, False)
    assert lds > 0 and lds % (16 * cus) == 0 and trip_records(L, True) == lds
    assert glob == none >= lds and none % (16 * cus) == 0


def test_second_trip_lds():
    n = RE.check_counts_trip(device_records, trip_records, 5, True, True)
    assert n > trip_records(5, True) > 10000   # (10 000: the largest file of the other tests)


def test_second_trip_no_table():
    assert RE.check_counts_trip(device_records, trip_records, 5, True, False) > trip_records(5, False)


def test_second_trip_global():
    import vcfc
    L = vcfc.counts_lds_samples()
    assert RE.check_counts_trip(device_records, trip_records, L + 1, False, True, L=L) > trip_records(L + 1, True)


def test_second_trip_irregular_records():
    RE.check_counts_trip_irregular(device_records, trip_records)


def test_second_trip_of_the_serial_kernel():
    """k_cnt_seq strides over a fixed number of lanes: more queued records than that."""
    RE.check_counts_serial_trip(device_records)


@pytest.mark.parametrize("fam", RE.FAMILIES)
def test_stager_edges(run, fam):
    RE.check_edges_counts(run, fam)
