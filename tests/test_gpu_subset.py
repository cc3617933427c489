"""GPU parity for the sample-subset decode (decompress-samples, query-samples;
DESIGN.md §4i): whole bytes and status against the Python restatement
(subset_cases.py, pinned to the oracle by test_subset_emu.py) through the C
ABI (libvcfc.so), the device entry and the CLI (build/main), and against a
Python cut of the source VCF on the golden file and a 2504-sample file."""
import io
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import decode_cases as D
import golden_io as G
import reader_edge_cases as RE
import subset_cases as SC

pytestmark = pytest.mark.gpu
REPO = G.REPO
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
MAIN = os.path.join(REPO, "build", "main")
OK, E_ARG, E_FORMAT = SC.OK, SC.E_ARG, SC.E_FORMAT


@pytest.fixture(scope="module")
def ctx():
    import torch   # before libvcfc: one HIP runtime in the process
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import vcfc
    c = vcfc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dec(ctx):
    return lambda data, cols: ctx.decompress_samples_buffer(data, cols)


@pytest.fixture(scope="module")
def qry(ctx):
    import vcfc
    return lambda data, q, cols: ctx.query_samples_buffer(data, vcfc.VcfCoordinateQuery(*q), cols)


def test_valid_files(dec):
    SC.check_files(dec, D.valid_files(1), 1)


@pytest.mark.parametrize("seed", [3, 4, 6])
def test_mutated_files(dec, seed):
    SC.check_mutated(dec, seed)


def test_hand_built_records(dec):
    SC.check_hand_built(dec)


def test_batch_sizes(dec):
    SC.check_files(dec, SC.batch_files())


@pytest.mark.parametrize("seed", [1, 2])
def test_query_files(qry, seed):
    SC.check_queries(qry, seed)


def test_bad_arguments_and_short_buffer(ctx, dec, qry):
    data = D.valid_files(1)[2][1]   # S = 64
    for cols in ([], [64], [0, 64], [3, 3], [5, 1, 5]):
        assert dec(data, cols) == (E_ARG, b"") and qry(data, SC.QUERIES[0], cols) == (E_ARG, b""), cols
    assert dec(data[1:], [0]) == (E_FORMAT, b"")
    # a short buffer: VCFC_E_NOSPACE and the size needed (the wrapper then retries with it)
    want = SC.subset(data, [63, 0])
    assert ctx.decompress_samples_buffer(data, [63, 0], cap=len(want[1]) - 1) == want
    assert ctx.decompress_samples_buffer(data, [63, 0], cap=0) == want
    wq = SC.subset_query(data, (b"22", False, 0, 0), [63, 0])
    assert len(wq[1]) > 0 and ctx.query_samples_buffer(data, "22", [63, 0], cap=5) == wq


def test_sample_columns():
    import vcfc
    data = D.valid_files(1)[2][1]   # samples S0 .. S63
    assert vcfc.sample_columns(data, "S5,S0,S63") == [5, 0, 63]
    assert vcfc.sample_columns(data[:SC.parse_header(data)[0] + 1], [b"S1", "S2"]) == [1, 2]
    with pytest.raises(ValueError, match="Unknown sample name: S64"):
        vcfc.sample_columns(data, "S5,S64,S1")
    with pytest.raises(ValueError, match="Duplicate sample name: S5"):
        vcfc.sample_columns(data, "S5,S1,S5")


def device_run(data, cols, select=None, cap=None):
    """vcfc_decode_samples_device on the records of a well-formed file:
    (status, err word, line offsets, out bytes)."""
    import torch
    import vcfc
    h, S = SC.parse_header(data)
    body = data[h:]
    rec, end = SC.hop(body)
    n = len(rec)
    dev = "cuda:0"
    d_in = torch.from_numpy(np.frombuffer(body + bytes(64), dtype=np.uint8).copy()).to(dev)
    d_rec = torch.from_numpy(np.array(rec + [end], dtype=np.int64)).to(dev)
    d_sel = None if select is None else torch.from_numpy(np.array(select, dtype=np.uint8)).to(dev)
    total = len(body) * 8 + 64 if cap is None else cap
    d_out = torch.full((total + 64,), 0xEE, dtype=torch.uint8, device=dev)
    d_loff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_err = torch.zeros(1, dtype=torch.int64, device=dev)
    wsb = vcfc.subset_workspace_size(n, max(len(cols), 1))
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = vcfc.decode_samples_device(d_in.data_ptr(), len(body), d_rec.data_ptr(), None if d_sel is None else d_sel.data_ptr(),
                                    n, S, cols, d_out.data_ptr(), total, d_loff.data_ptr(), d_ws.data_ptr(), wsb,
                                    d_err.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[total:] == 0xEE).all(), "bytes written past out_cap"
    return st, int(d_err.cpu().numpy().view(np.uint64)[0]), [int(x) for x in d_loff.cpu().tolist()], out[:total].tobytes()


def test_device_entry():
    import vcfc
    name, data = SC.batch_files()[4]   # 41 records, S = 70
    h, S = SC.parse_header(data)
    body = data[h:]
    rec, end = SC.hop(body)
    n = len(rec)
    selects = [None, [0] * n, [1] * n, [int(i % 8 == 0) for i in range(n)], [int(i % 8 == 3 or i == n - 1) for i in range(n)]]
    for cols in ([0], [69, 0, 33], list(range(70))):
        lines = [SC.line(*SC.regular(body, rec[i], (rec + [end])[i + 1], S), cols) for i in range(n)]
        for sel in selects:
            want = [l if sel is None or sel[i] else b"" for i, l in enumerate(lines)]
            off = [0]
            for l in want:
                off.append(off[-1] + len(l))
            st, err, loff, out = device_run(data, cols, sel)
            assert (st, err) == (OK, vcfc.NO_ERROR) and loff == off and out[:off[-1]] == b"".join(want), (cols[:4], sel)
            if off[-1]:   # one byte short: the first line that does not fit
                st, err, loff, out = device_run(data, cols, sel, cap=off[-1] - 1)
                first = next(i for i in range(n) if off[i + 1] > off[-1] - 1)
                assert (st, err) == (OK, (first << 8) | 0xFF) and loff == off, (cols[:4], sel, hex(err))
    for cols in ([], [70], [1, 1]):
        assert device_run(data, cols)[0] == E_ARG


def test_device_entry_irregular_record_only_where_selected():
    import vcfc
    name, data = next(x for x in SC.query_files(1) if x[0] == "no_lf17")
    n = len(SC.hop(data[SC.parse_header(data)[0]:])[0])
    st, err, loff, out = device_run(data, [0, 5])
    assert (st, err) == (OK, (17 << 8) | 3)
    st, err, loff, out = device_run(data, [0, 5], [int(i != 17) for i in range(n)])
    assert (st, err) == (OK, vcfc.NO_ERROR) and loff[17] == loff[18]


def test_cli():
    import vcfc
    vcf = G.gz("random_100x10000.vcf.gz")
    enc = G.gz("random_100x10000.vcfc.gz")
    names = vcf[vcf.index(b"#CHROM"):].split(b"\n", 1)[0].split(b"\t")[9:]
    cols = [77, 3, 50]
    pick = b",".join(names[c] for c in cols).decode()
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "t.vcfc"), os.path.join(d, "t.vcf")
        with open(src, "wb") as f:
            f.write(enc)
        r = subprocess.run([MAIN, "decompress-samples", src, dst, pick], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert open(dst, "rb").read() == SC.cut_vcf(vcf, cols)
        r = subprocess.run([MAIN, "query-samples", src, "1:10100-10300", pick], capture_output=True, timeout=300)
        st, want = G.oracle_query(enc, b"1:10100-10300")
        assert r.returncode == 0 and len(want) > 0 and r.stdout == SC.cut_vcf(want, cols), r.stderr
        # names the header lacks, names listed twice: a message, exit 1, nothing written
        os.remove(dst)
        for action, arg in (("decompress-samples", dst), ("query-samples", "1")):
            r = subprocess.run([MAIN, action, src, arg, pick + ",nobody"], capture_output=True, timeout=300)
            assert (r.returncode, r.stdout) == (1, b"Unknown sample name: nobody\n")
            r = subprocess.run([MAIN, action, src, arg, pick + "," + names[3].decode()], capture_output=True, timeout=300)
            assert (r.returncode, r.stdout) == (1, b"Duplicate sample name: " + names[3] + b"\n")
        assert not os.path.exists(dst)
        r = subprocess.run([MAIN, "query-samples", src, "1:5", pick], capture_output=True, timeout=300)
        assert r.returncode == 1 and r.stdout == (b"Query must contain a dash character: <ref>:<start>-<end>\n"
                                                  b"Failed to parse query string: 1:5\n")
        # too few arguments: the usage text, which still holds the earlier actions' lines
        for argv in (["decompress-samples", src, dst], ["query-samples", src, "1"], []):
            r = subprocess.run([MAIN] + argv, capture_output=True, timeout=300)
            assert r.returncode == 1
            for l in (b"./main [compress|decompress|sparsify] <input_file> <output_file>\n",
                      b"./main [query|sparse-query] <input_file> <ref>[:<start>-<end>]\n",
                      b"./main gap-analysis <compressed-filename>\n",
                      b"./main decompress-samples <input_file> <output_file> <name>[,<name>...]\n",
                      b"./main query-samples <input_file> <ref>[:<start>-<end>] <name>[,<name>...]\n"):
                assert l in r.stderr
        r = subprocess.run([MAIN, "frobnicate"], capture_output=True, timeout=300)
        assert (r.returncode, r.stdout) == (0, b"Unknown action name: frobnicate\n")
        # a file that stops mid-way: exit 134 with the lines before the stop written
        name, bad = next(x for x in SC.query_files(1) if x[0] == "no_lf17")
        with open(src, "wb") as f:
            f.write(bad)
        r = subprocess.run([MAIN, "decompress-samples", src, dst, "S39,S0"], capture_output=True, timeout=300)
        want = SC.subset(bad, [39, 0])
        assert want[0] == E_FORMAT and want[1].count(b"\n") == 2 + 17
        assert r.returncode == 134 and b"VcfValidationError" in r.stderr and open(dst, "rb").read() == want[1]
        r = subprocess.run([MAIN, "query-samples", src, "", "S39,S0"], capture_output=True, timeout=300)
        assert r.returncode == 134 and r.stdout == SC.subset_query(bad, (b"", False, 0, 0), [39, 0])[1]
    assert vcfc.strerror(E_FORMAT).encode() in r.stderr


def test_files_2504_samples(ctx):
    import random_vcf
    buf = io.BytesIO()
    random_vcf.generate(2504, 600, buf)
    vcf = buf.getvalue()
    enc = ctx.compress_buffer(vcf)
    cols = [2503, 0, 1234]
    assert ctx.decompress_samples_buffer(enc, cols) == (OK, SC.cut_vcf(vcf, cols))
    lines = SC.cut_vcf(vcf, cols, header_too=False).split(b"\n")[:-1]   # POS = 10000 + 2 i
    st, got = ctx.query_samples_buffer(enc, "1:%d-%d" % (10000 + 2 * 17, 10000 + 2 * 417), cols)
    assert st == OK and got == b"".join(l + b"\n" for l in lines[17:418])
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "t.vcfc"), os.path.join(d, "t.vcf")
        with open(src, "wb") as f:
            f.write(enc)
        ctx.decompress_samples_file(src, dst, cols)
        assert open(dst, "rb").read() == SC.cut_vcf(vcf, cols)
        with open(dst, "wb") as f:
            ctx.query_samples_file(src, "1:10000-10010", cols, out_fd=f.fileno())
        assert open(dst, "rb").read() == b"".join(l + b"\n" for l in lines[0:6])


# ---- the writer's later passes and the stager's edges (reader_edge_cases.py) --------

def test_queue_pass(dec):
    import vcfc
    RE.check_queue_is_longer_than_the_lanes(vcfc.subset_workspace_size, 1)
    RE.check_queue_subset([dec], device_run)


@pytest.mark.parametrize("fam", RE.FAMILIES)
def test_stager_edges(dec, fam):
    RE.check_edges_subset(dec, fam)
