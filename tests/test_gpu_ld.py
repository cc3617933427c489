"""GPU parity for ld-window: status, failing record, indices
and every table of the band against the Python restatement (ld_cases.py,
pinned by test_ld_emu.py) through the C ABI (libvcfc.so) and the Python
binding; the two device entries on torch tensors, every byte of the band's
allocation outside the slots that are due included; the text of the file
call and of the CLI (build/main) byte for byte; the composed call captured in
a graph and replayed on changed input; a 2504-sample file against a numpy
contingency count over a Python parse of its source VCF text.  Every
comparison is exact."""
import io
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import decode_cases as D
import golden_io as G
import ld_cases as LC
import matrix_cases as MC
import subset_cases as SC

pytestmark = pytest.mark.gpu
REPO = G.REPO
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
MAIN = os.path.join(REPO, "build", "main")
OK, E_ARG, E_FORMAT = LC.OK, LC.E_ARG, LC.E_FORMAT


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

    def f(data, W, query=None, regions=None, band_bound=0, min_r2=None):
        q = None if query is None else vcfc.VcfCoordinateQuery(*query)
        st, idx, t = ctx.ld_window_buffer(data, W, q, regions)
        text = None
        if min_r2 is not None and st in (OK, E_FORMAT):   # the file entry on the same bytes
            with tempfile.TemporaryDirectory() as d:
                src, out = os.path.join(d, "t.vcfc"), os.path.join(d, "t.tsv")
                with open(src, "wb") as fh:
                    fh.write(data)
                try:
                    ctx.ld_window_file(src, out, W, min_r2, q, regions)
                    assert st == OK
                except RuntimeError as e:
                    assert st == E_FORMAT and vcfc.strerror(E_FORMAT) in str(e)
                text = open(out, "rb").read()
        return st, [int(x) for x in idx], t.reshape(t.shape[0], t.shape[1], 9), ctx.last_ld_record, text
    return f


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def gpu_tables(bed, n_rows, row_stride, S, W, pairs_cap, alloc_slots, offset=0, ws_short=0, null=None, n_override=None):
    """vcfc_ld_tables_device on torch tensors, as ld_cases' tab."""
    import torch
    import vcfc
    dev = "cuda:0"
    host = np.zeros(offset + len(bed) + 16, dtype=np.uint8)
    host[offset:offset + len(bed)] = np.frombuffer(bed, dtype=np.uint8)
    d_bed = torch.from_numpy(host).to(dev)   # (256-byte aligned: d_bed's alignment is `offset`)
    d_out = torch.full((36 * alloc_slots + LC.CANARY,), LC.FILL, dtype=torch.uint8, device=dev)
    wsb = vcfc.ld_workspace_size(n_rows, S if 0 < S < 1 << 30 else 1, W) - ws_short
    d_ws = torch.full((wsb + 64,), 0xCD, dtype=torch.uint8, device=dev)
    d_err = torch.full((1,), 0x1111, dtype=torch.int64, device=dev)
    st = vcfc.ld_tables_device(d_bed.data_ptr() + offset, n_rows if n_override is None else n_override, row_stride, S, W,
                               None if null == "tables" else d_out.data_ptr(), pairs_cap,
                               None if null == "ws" else d_ws.data_ptr(), wsb, None if null == "err" else d_err.data_ptr(),
                               _stream())
    torch.cuda.synchronize()
    assert (d_ws[wsb:].cpu().numpy() == 0xCD).all(), "written past the workspace"
    return st, int(d_err.cpu().numpy().view(np.uint64)[0]), d_out.cpu().numpy().tobytes()


def gpu_window(body, rec, S, W, select, pairs_cap, alloc_slots, ws_short=0, null=None, n_override=None):
    """vcfc_ld_window_device on torch tensors, as ld_cases' win."""
    import torch
    import vcfc
    n = len(rec) - 1
    dev = "cuda:0"
    d_in = torch.from_numpy(np.frombuffer(body + bytes(64), dtype=np.uint8).copy()).to(dev)
    d_rec = torch.from_numpy(np.array(rec, dtype=np.int64)).to(dev)
    d_sel = None if select is None else torch.from_numpy(np.array(select, dtype=np.uint8)).to(dev)
    d_out = torch.full((36 * alloc_slots + LC.CANARY,), LC.FILL, dtype=torch.uint8, device=dev)
    d_row_of = torch.full((n + 2,), -0x1111111111111112, dtype=torch.int64, device=dev)
    wsb = vcfc.ld_workspace_size(n, S if 0 < S < 1 << 30 else 1, W) - ws_short
    d_ws = torch.full((wsb + 64,), 0xCD, dtype=torch.uint8, device=dev)
    d_err = torch.full((1,), 0x1111, dtype=torch.int64, device=dev)
    st = vcfc.ld_window_device(d_in.data_ptr(), len(body), d_rec.data_ptr(), None if d_sel is None else d_sel.data_ptr(),
                               n if n_override is None else n_override, S, W, None if null == "tables" else d_out.data_ptr(),
                               pairs_cap, None if null == "row_of" else d_row_of.data_ptr(),
                               None if null == "ws" else d_ws.data_ptr(), wsb, None if null == "err" else d_err.data_ptr(),
                               _stream())
    torch.cuda.synchronize()
    row_of = d_row_of.cpu().numpy()
    assert (d_ws[wsb:].cpu().numpy() == 0xCD).all(), "written past the workspace"
    assert row_of[n + 1] == -0x1111111111111112
    return st, int(d_err.cpu().numpy().view(np.uint64)[0]), d_out.cpu().numpy().tobytes(), [int(x) for x in row_of[:n + 1]]


def test_known_answer(run, ctx):
    import vcfc
    got = run(LC.kat_file(), LC.KAT_W, min_r2=0.0)
    assert got[0] == OK and got[2].tolist() == LC.KAT_BAND and got[4] == LC.KAT_TSV
    st, idx, t = ctx.ld_window_buffer(LC.kat_file(), LC.KAT_W)
    assert t.shape == (3, 2, 3, 3) and t.dtype == np.uint32 and t[0, 0, 1, 0] == 2 and t[0, 0, 0, 2] == 1
    r = vcfc.ld_r2(t)
    assert r.dtype == np.float64 and r.shape == (3, 2)
    assert [[LC.r2_text(None if np.isnan(x) else float(x)) for x in row] for row in r] == LC.KAT_R2
    assert r[0, 0] == 16.0 / 88.0 and r[0, 1] == 0.5 and r[1, 0] == 100.0 / 280.0


def test_sample_counts(run):
    import vcfc
    LC.check_sizes(run, vcfc.matrix_lds_samples(MC.BED))


def test_rows_and_windows(run):
    LC.check_shapes(run)


def test_query_files(run):
    LC.check_queries(run, 1)
    LC.check_batches(run)   # (the C ABI has no band bound: the same files through the default one)


def test_region_tables(run):
    LC.check_regions(run)


def test_mutated_files(run):
    LC.check_mutated(run, 3)


def test_irregular_records(run):
    LC.check_irregular(run)


def test_bad_headers_and_windows(run):
    data = D.valid_files(1)[2][1]
    for W in (0, 1 << 16):
        assert run(data, W)[0] == E_ARG
    got = run(data[1:], 2, min_r2=0.0)
    assert (got[0], got[1], got[3], got[4]) == (E_FORMAT, [], LC.NO_RECORD, b"")
    s0 = next(d for n, d in D.mutated_files(3) if n == "S0_row")
    assert run(s0, 2)[0] == E_ARG


def test_ld_r2_is_the_restatement(run):
    import vcfc
    bands = [LC.ld(LC.ld_file(S, 7, 0.25 if S < 8 else 0.1), 3)[2] for S in (3, 33, 600)] + [LC.ld(LC.two_chrom_file(), 4)[2]]
    nan = defined = 0
    for b in bands:
        r = vcfc.ld_r2(b)
        assert r.shape == b.shape[:2]
        for i in range(b.shape[0]):
            for k in range(b.shape[1]):
                want = LC.r2(b[i, k])[1]
                assert (np.isnan(r[i, k]) if want is None else r[i, k] == want), (i, k)
                nan += want is None
                defined += want is not None
    assert nan >= 10 and defined >= 10
    big = np.zeros((3, 3), dtype=np.uint32)   # S just below 2^30: the integers pass 2^53, still exact in int64
    big[0, 0], big[1, 1], big[2, 2], big[0, 1] = (1 << 28) - 1, 1 << 28, (1 << 28) + 3, 1 << 27
    assert vcfc.ld_r2(big) == LC.r2(big.reshape(9))[1]


def test_tables_device():
    LC.check_tables_device(gpu_tables)


def test_tables_device_arguments():
    import vcfc
    LC.check_tables_args(gpu_tables, vcfc.ld_workspace_size)


def test_window_device():
    LC.check_window_device(gpu_window)


def test_window_device_arguments():
    import vcfc
    LC.check_window_args(gpu_window, vcfc.ld_workspace_size)


def test_window_device_captured_in_a_graph():
    """Captured once, replayed twice: the second replay on another file's records in the same tensors."""
    import torch
    import vcfc
    files = [LC.ld_file(65, 18, 0.15, seed=s) for s in (0, 3)]
    recs = [MC.records_of(d) for d in files]
    n, S, W = 18, 65, 3
    assert all(len(r[1]) - 1 == n and r[2] == S for r in recs) and recs[0][0] != recs[1][0]
    sel = [int(i % 3 != 1) for i in range(n)]
    rows = sum(sel)
    cap_bytes = max(len(r[0]) for r in recs) + 64
    dev = "cuda:0"
    d_in = torch.zeros(cap_bytes, dtype=torch.uint8, device=dev)
    d_rec = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_sel = torch.from_numpy(np.array(sel, dtype=np.uint8)).to(dev)
    d_out = torch.full((36 * rows * W + LC.CANARY,), LC.FILL, dtype=torch.uint8, device=dev)
    d_row_of = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    wsb = vcfc.ld_workspace_size(n, S, W)
    d_ws = torch.full((wsb,), 0xCD, dtype=torch.uint8, device=dev)
    d_err = torch.zeros(1, dtype=torch.int64, device=dev)

    def load(k):
        body, rec, _ = recs[k]
        host = np.zeros(cap_bytes, dtype=np.uint8)
        host[:len(body)] = np.frombuffer(body, dtype=np.uint8)
        d_in.copy_(torch.from_numpy(host))
        d_rec.copy_(torch.from_numpy(np.array(rec, dtype=np.int64)))
    load(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = vcfc.ld_window_device(d_in.data_ptr(), cap_bytes - 64, d_rec.data_ptr(), d_sel.data_ptr(), n, S, W, d_out.data_ptr(),
                                   rows * W, d_row_of.data_ptr(), d_ws.data_ptr(), wsb, d_err.data_ptr(), _stream())
    assert st == OK
    for k in (0, 1):
        load(k)
        d_out.fill_(LC.FILL)
        d_err.zero_()
        d_row_of.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        body, rec, _ = recs[k]
        err, buf, mask, row_of = LC.expect_window(body, rec, S, W, sel, rows * W, rows * W)
        assert err == LC.NO_ERROR and int(d_err.cpu().numpy().view(np.uint64)[0]) == err, k
        assert d_row_of.cpu().numpy().tolist() == row_of and d_out.cpu().numpy().tobytes() == buf, k


def cli(argv):
    return subprocess.run([MAIN] + argv, capture_output=True, timeout=300)


def test_file_call_and_cli(run, ctx):
    import vcfc
    LC.check_tsv(run)   # the file entry, through the binding
    data, W = LC.two_chrom_file(), 4
    st, idx, bnd, bad = LC.ld(data, W)
    pick = sorted(x for x in (LC.r2(t)[1] for row in bnd for t in row) if x is not None and x < 1)[-1]
    with tempfile.TemporaryDirectory() as d:
        src, out, reg = os.path.join(d, "t.vcfc"), os.path.join(d, "out.tsv"), os.path.join(d, "targets.bed")
        with open(src, "wb") as f:
            f.write(data)
        for m in ("0", "-1", repr(pick), "1", "1e0"):
            r = cli(["ld-window", src, out, "4", m])
            assert r.returncode == 0 and r.stdout == b"", r.stderr
            assert open(out, "rb").read() == LC.tsv(data, idx, bnd, W, float(m)), m
        qd = LC.ld(data, 2, (b"2", False, 0, 0))
        assert qd[0] == OK and len(qd[1]) == 6
        r = cli(["ld-window", src, out, "2", "0", "2"])
        assert r.returncode == 0 and open(out, "rb").read() == LC.tsv(data, qd[1], qd[2], 2, 0.0)
        text = b"1\t100\t110\n2:121-140\n"
        with open(reg, "wb") as f:
            f.write(text)
        import regions_cases as RC
        rd = LC.ld(data, 3, table=RC.parse_text(text))
        assert rd[0] == OK and len(rd[1]) >= 6
        r = cli(["ld-window-regions", src, out, "3", "0", reg])
        assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == LC.tsv(data, rd[1], rd[2], 3, 0.0), r.stderr
        ctx.ld_window_file(src, out + "2", 3, regions=text)
        assert open(out + "2", "rb").read() == LC.tsv(data, rd[1], rd[2], 3, 0.0)
        r = cli(["ld-window", src, out, "2", "0", "1:5"])
        assert r.returncode == 1 and r.stdout == (b"Query must contain a dash character: <ref>:<start>-<end>\n"
                                                  b"Failed to parse query string: 1:5\n")
        for argv in (["ld-window", src, out, "2"], ["ld-window-regions", src, out, "2", "0"], ["ld-window", src, out, "0", "0"],
                     ["ld-window", src, out, "65536", "0"], ["ld-window", src, out, "2x", "0"], ["ld-window", src, out, "2", "x"],
                     []):
            r = cli(argv)
            assert r.returncode == 1, argv
            assert b"./main ld-window <input_file> <out.tsv> <window> <min-r2> [<ref>[:<start>-<end>]]\n" in r.stderr
            assert b"./main ld-window-regions <input_file> <out.tsv> <window> <min-r2> <regions-file>\n" in r.stderr
            assert b"./main export-bed <input_file> <output_prefix> [<ref>[:<start>-<end>]]\n" in r.stderr
        r = cli(["ld-window", src, src, "2", "0"])
        assert r.returncode == 134 and open(src, "rb").read() == data
        # a file that stops mid-way: exit 134, the pairs among the rows before the stop
        name, bad_file = next(x for x in SC.query_files(1) if x[0] == "no_lf17")
        with open(src, "wb") as f:
            f.write(bad_file)
        bd = LC.ld(bad_file, 3)
        assert (bd[0], bd[3], len(bd[1])) == (E_FORMAT, 17, 17)
        r = cli(["ld-window", src, out, "3", "0"])
        assert r.returncode == 134 and b"VcfValidationError" in r.stderr and vcfc.strerror(E_FORMAT).encode() in r.stderr
        assert open(out, "rb").read() == LC.tsv(bad_file, bd[1], bd[2], 3, 0.0)
        # a header the decoder refuses: the file created, empty
        with open(src, "wb") as f:
            f.write(data[1:])
        r = cli(["ld-window", src, out, "3", "0"])
        assert r.returncode == 134 and open(out, "rb").read() == b""


def test_file_2504_samples(ctx):
    """200 rows of 2504 samples, W = 7: every table against a numpy count over a Python parse of the VCF text."""
    import random_vcf
    import vcfc
    buf = io.BytesIO()
    random_vcf.generate(2504, 200, buf)
    vcf = buf.getvalue()
    enc = ctx.compress_buffer(vcf)
    g = np.array([[{3: 0, 2: 1, 0: 2, 1: -1}[MC.token_codes(t)[3]] for t in l.split(b"\t")[9:]]
                  for l in vcf.split(b"\n")[:-1] if not l.startswith(b"#")], dtype=np.int8)
    assert g.shape == (200, 2504) and (g == -1).any() and (g == 2).any()
    W = 7
    want = np.zeros((200, W, 3, 3), dtype=np.uint32)
    for i in range(200):
        for k in range(1, min(W, 199 - i) + 1):
            for a in range(3):
                for b in range(3):
                    want[i, k - 1, a, b] = np.count_nonzero((g[i] == a) & (g[i + k] == b))
    st, idx, t = ctx.ld_window_buffer(enc, W)
    assert st == OK and idx.tolist() == list(range(200))
    assert t.shape == want.shape and np.array_equal(t, want)
    st, idx, t = ctx.ld_window_buffer(enc, 3, "1:%d-%d" % (10000 + 2 * 17, 10000 + 2 * 97))   # POS = 10000 + 2 i
    assert st == OK and idx.tolist() == list(range(17, 98))
    assert np.array_equal(t[:78], want[17:95, :3]) and np.array_equal(t[78, :2], want[95, :2]) and not t[78, 2].any()
    r = vcfc.ld_r2(want[3, 0])
    assert r == LC.r2(want[3, 0].reshape(9))[1]
