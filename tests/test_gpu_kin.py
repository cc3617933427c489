"""GPU parity for kinship: status, failing record, indices and
every table of the square against the Python restatement (kin_cases.py,
pinned by test_kin_emu.py) through the C ABI (libvcfc.so) and the Python
binding; the two device entries on torch tensors, every byte of the square's
allocation outside it included; the text of the file call and of the CLI
(build/main) byte for byte; the composed call captured in a graph and replayed
on changed input; a 2504-sample file against a numpy contingency count over a
Python parse of its source VCF text; one square whose cell indices pass 2^32.
Every comparison is exact."""
import io
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import decode_cases as D
import golden_io as G
import kin_cases as KC
import matrix_cases as MC
import subset_cases as SC

pytestmark = pytest.mark.gpu
REPO = G.REPO
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
MAIN = os.path.join(REPO, "build", "main")
OK, E_ARG, E_FORMAT = KC.OK, KC.E_ARG, KC.E_FORMAT
USAGE = (b"./main kinship <input_file> <out.tsv> <min-kinship|all> [<ref>[:<start>-<end>]]\n",
         b"./main kinship-regions <input_file> <out.tsv> <min-kinship|all> <regions-file>\n")


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

    def f(data, query=None, regions=None, batch=0, text=None):   # (the C ABI has no batch bound: its default)
        q = None if query is None else vcfc.VcfCoordinateQuery(*query)
        st, idx, t = ctx.kinship_buffer(data, q, regions)
        out = None
        if text is not None:   # the file entry on the same bytes
            with tempfile.TemporaryDirectory() as d:
                src, dst = os.path.join(d, "t.vcfc"), os.path.join(d, "t.tsv")
                with open(src, "wb") as fh:
                    fh.write(data)
                try:
                    ctx.kinship_file(src, dst, None if text == "all" else text, q, regions)
                    assert st == OK
                except RuntimeError as e:
                    assert st != OK and vcfc.strerror(st) in str(e)
                out = open(dst, "rb").read()
        return st, [int(x) for x in idx], t.reshape(t.shape[0], t.shape[1], 9), ctx.last_kinship_record, out
    return f


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _alloc(alloc_tables, prefill):
    import torch
    host = np.full(36 * alloc_tables + KC.CANARY, KC.FILL, dtype=np.uint8)
    if prefill is not None:
        host[:len(prefill)] = np.frombuffer(prefill, dtype=np.uint8)
    return torch.from_numpy(host).to("cuda:0")


def gpu_tables(bed, n_rows, row_stride, S, tables_cap, alloc_tables, accumulate=0, prefill=None, offset=0, ws_short=0, null=None,
               n_override=None):
    """vcfc_kin_tables_device on torch tensors, as kin_cases' tab."""
    import torch
    import vcfc
    dev = "cuda:0"
    host = np.zeros(offset + len(bed) + 16, dtype=np.uint8)
    host[offset:offset + len(bed)] = np.frombuffer(bed, dtype=np.uint8)
    d_bed = torch.from_numpy(host).to(dev)   # (256-byte aligned: d_bed's alignment is `offset`)
    d_out = _alloc(alloc_tables, prefill)
    wsb = vcfc.kin_workspace_size(n_rows, S if 0 < S < 1 << 30 else 1) - ws_short
    d_ws = torch.full((wsb + 64,), 0xCD, dtype=torch.uint8, device=dev)
    d_err = torch.full((1,), 0x1111, dtype=torch.int64, device=dev)
    st = vcfc.kin_tables_device(d_bed.data_ptr() + offset, n_rows if n_override is None else n_override, row_stride, S,
                                None if null == "tables" else d_out.data_ptr(), tables_cap, accumulate,
                                None if null == "ws" else d_ws.data_ptr(), wsb, None if null == "err" else d_err.data_ptr(),
                                _stream())
    torch.cuda.synchronize()
    assert (d_ws[wsb:].cpu().numpy() == 0xCD).all(), "written past the workspace"
    return st, int(d_err.cpu().numpy().view(np.uint64)[0]), d_out.cpu().numpy().tobytes()


def gpu_records(body, rec, S, select, tables_cap, alloc_tables, accumulate=0, prefill=None, ws_short=0, null=None,
                n_override=None):
    """vcfc_kin_records_device on torch tensors, as kin_cases' rec."""
    import torch
    import vcfc
    n = len(rec) - 1
    dev = "cuda:0"
    d_in = torch.from_numpy(np.frombuffer(body + bytes(64), dtype=np.uint8).copy()).to(dev)
    d_rec = torch.from_numpy(np.array(rec, dtype=np.int64)).to(dev)
    d_sel = None if select is None else torch.from_numpy(np.array(select, dtype=np.uint8)).to(dev)
    d_out = _alloc(alloc_tables, prefill)
    d_row_of = torch.full((n + 2,), -0x1111111111111112, dtype=torch.int64, device=dev)
    wsb = vcfc.kin_workspace_size(n, S if 0 < S < 1 << 30 else 1) - ws_short
    d_ws = torch.full((wsb + 64,), 0xCD, dtype=torch.uint8, device=dev)
    d_err = torch.full((1,), 0x1111, dtype=torch.int64, device=dev)
    st = vcfc.kin_records_device(d_in.data_ptr(), len(body), d_rec.data_ptr(), None if d_sel is None else d_sel.data_ptr(),
                                 n if n_override is None else n_override, S, None if null == "tables" else d_out.data_ptr(),
                                 tables_cap, accumulate, None if null == "row_of" else d_row_of.data_ptr(),
                                 None if null == "ws" else d_ws.data_ptr(), wsb, None if null == "err" else d_err.data_ptr(),
                                 _stream())
    torch.cuda.synchronize()
    row_of = d_row_of.cpu().numpy()
    assert (d_ws[wsb:].cpu().numpy() == 0xCD).all(), "written past the workspace"
    assert row_of[n + 1] == -0x1111111111111112
    return st, int(d_err.cpu().numpy().view(np.uint64)[0]), d_out.cpu().numpy().tobytes(), [int(x) for x in row_of[:n + 1]]


def test_known_answer(run, ctx):
    import vcfc
    data = KC.kat_file()
    got = run(data, text="all")
    assert got[0] == OK and got[1] == list(range(6)) and got[4] == KC.tsv(data, KC.kin(data)[2])
    for (i, j), t in KC.KAT_TABLES.items():
        assert got[2][i, j].tolist() == t, (i, j)
    for (i, j), line in KC.KAT_LINES.items():
        assert line in got[4]
    st, idx, t = ctx.kinship_buffer(data)
    assert t.shape == (6, 6, 3, 3) and t.dtype == np.uint32 and t[0, 2, 0, 2] == 1 and t[2, 0, 2, 0] == 1
    N, ibs0, ibs1, ibs2, dst, kin = vcfc.kinship_stats(t)
    assert all(x.dtype == np.int64 and x.shape == (6, 6) for x in (N, ibs0, ibs1, ibs2)) and dst.dtype == kin.dtype == np.float64
    for (i, j), x in KC.KAT_STATS.items():
        assert (N[i, j], ibs0[i, j], ibs1[i, j], ibs2[i, j]) == x[:4], (i, j)
        assert (KC.num_text(None if np.isnan(dst[i, j]) else float(dst[i, j])),
                KC.num_text(None if np.isnan(kin[i, j]) else float(kin[i, j]))) == x[7:], (i, j)
    assert kin[0, 1] == 2.0 / 12.0 and dst[0, 1] == 8.0 / 12.0 and kin[0, 0] == 0.5


def test_kinship_stats_is_the_restatement():
    import vcfc
    squares = [KC.kin(KC.kin_file(S, n, 0.25))[2] for S, n in ((5, 2), (33, 7), (12, 40))] + [KC.kin(KC.twin_file())[2]]
    nan = defined = 0
    for sq in squares:
        got = vcfc.kinship_stats(sq)
        again = vcfc.kinship_stats(sq.reshape(sq.shape[:2] + (3, 3)))
        for i in range(sq.shape[0]):
            for j in range(sq.shape[1]):
                x = KC.stats(sq[i, j])
                assert tuple(int(g[i, j]) for g in got[:4]) == x[:4]
                for g, a, want in ((got[4], again[4], x[7]), (got[5], again[5], x[8])):
                    assert (np.isnan(g[i, j]) and np.isnan(a[i, j])) if want is None else g[i, j] == want == a[i, j], (i, j)
                nan += x[8] is None
                defined += x[8] is not None
    assert nan >= 10 and defined >= 10
    big = np.zeros(9, dtype=np.uint32)   # counts near 2^32: the integers pass 2^32, still exact in int64
    big[:] = [(1 << 32) - 1, 1 << 31, 7, 1 << 30, (1 << 32) - 5, 3, 9, 1 << 29, 1 << 31]
    got = vcfc.kinship_stats(big)
    x = KC.stats(big)
    assert tuple(int(g) for g in got[:4]) == x[:4] and got[4] == x[7] and got[5] == x[8]


def test_sample_counts(run):
    KC.check_sizes(run)


def test_row_counts(run):
    KC.check_rows(run)


def test_query_files(run):
    KC.check_queries(run, 1)


def test_region_tables(run):
    KC.check_regions(run)


def test_mutated_files(run):
    KC.check_mutated(run, 3)


def test_irregular_records(run):
    KC.check_irregular(run)


def test_bad_headers(run):
    data = D.valid_files(1)[2][1]
    got = run(data[1:], text="all")
    assert (got[0], got[1], got[3], got[4]) == (E_FORMAT, [], KC.NO_RECORD, b"") and got[2].shape == (0, 0, 9)
    s0 = next(d for n, d in D.mutated_files(3) if n == "S0_row")
    assert run(s0)[0] == E_ARG


def test_tables_device():
    KC.check_tables_device(gpu_tables)


def test_tables_device_arguments():
    import vcfc
    KC.check_tables_args(gpu_tables, vcfc.kin_workspace_size)


def test_records_device():
    KC.check_records_device(gpu_records)


def test_records_device_arguments():
    import vcfc
    KC.check_records_args(gpu_records, vcfc.kin_workspace_size)


def test_records_device_captured_in_a_graph():
    """Captured once on a side stream, replayed twice: the second replay on another file's records in the same tensors."""
    import torch
    import vcfc
    files = [KC.kin_file(65, 18, 0.15, seed=s) for s in (0, 3)]
    recs = [MC.records_of(d) for d in files]
    n, S = 18, 65
    assert all(len(r[1]) - 1 == n and r[2] == S for r in recs) and recs[0][0] != recs[1][0]
    sel = [int(i % 3 != 1) for i in range(n)]
    cap_bytes = max(len(r[0]) for r in recs) + 64
    dev = "cuda:0"
    d_in = torch.zeros(cap_bytes, dtype=torch.uint8, device=dev)
    d_rec = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_sel = torch.from_numpy(np.array(sel, dtype=np.uint8)).to(dev)
    d_out = torch.full((36 * S * S + KC.CANARY,), KC.FILL, dtype=torch.uint8, device=dev)
    d_row_of = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    wsb = vcfc.kin_workspace_size(n, S)
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
    with torch.cuda.graph(g):   # (one stream: the capture's)
        st = vcfc.kin_records_device(d_in.data_ptr(), cap_bytes - 64, d_rec.data_ptr(), d_sel.data_ptr(), n, S, d_out.data_ptr(),
                                     S * S, 0, d_row_of.data_ptr(), d_ws.data_ptr(), wsb, d_err.data_ptr(), _stream())
    assert st == OK
    for k in (0, 1):
        load(k)
        d_out.fill_(KC.FILL)
        d_err.zero_()
        d_row_of.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        body, rec, _ = recs[k]
        err, sq, row_of = KC.expect_records(body, rec, S, sel)
        assert err == KC.NO_ERROR and int(d_err.cpu().numpy().view(np.uint64)[0]) == err, k
        assert d_row_of.cpu().numpy().tolist() == row_of and d_out.cpu().numpy().tobytes() == KC.expect_bytes(sq, S * S), k


def cli(argv):
    return subprocess.run([MAIN] + argv, capture_output=True, timeout=300)


def test_file_call_and_cli(run, ctx):
    import regions_cases as RC
    import vcfc
    KC.check_tsv(run)   # the file entry, through the binding
    data = KC.twin_file()
    sq = KC.kin(data)[2]
    pick = sorted(v for v in (KC.stats(sq[i, j])[8] for i in range(12) for j in range(i + 1, 12)) if v is not None)[30]
    with tempfile.TemporaryDirectory() as d:
        src, out, reg = os.path.join(d, "t.vcfc"), os.path.join(d, "out.tsv"), os.path.join(d, "targets.bed")
        with open(src, "wb") as f:
            f.write(data)
        for m in ("all", repr(pick), "5e-1"):
            r = cli(["kinship", src, out, m])
            assert r.returncode == 0 and r.stdout == b"", r.stderr
            assert open(out, "rb").read() == KC.tsv(data, sq, None if m == "all" else float(m)), m
        qd = KC.kin(data, (b"22", True, 100, 130))   # POS = 100 + 3 i: rows 0..10
        assert qd[0] == OK and len(qd[1]) == 11
        r = cli(["kinship", src, out, "all", "22:100-130"])
        assert r.returncode == 0 and open(out, "rb").read() == KC.tsv(data, qd[2])
        text = b"22\t99\t112\n22:160-175\n"
        with open(reg, "wb") as f:
            f.write(text)
        rd = KC.kin(data, table=RC.parse_text(text))
        assert rd[0] == OK and len(rd[1]) >= 8
        r = cli(["kinship-regions", src, out, "all", reg])
        assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == KC.tsv(data, rd[2]), r.stderr
        ctx.kinship_file(src, out + "2", 0.0, regions=text)
        assert open(out + "2", "rb").read() == KC.tsv(data, rd[2], 0.0)
        r = cli(["kinship", src, out, "all", "1:5"])
        assert r.returncode == 1 and r.stdout == (b"Query must contain a dash character: <ref>:<start>-<end>\n"
                                                  b"Failed to parse query string: 1:5\n")
        for argv in (["kinship", src, out], ["kinship-regions", src, out, "all"], ["kinship", src, out, "x"],
                     ["kinship", src, out, "0.1x"], ["kinship", src, out, ""], ["kinship", src, out, "nan"], []):
            r = cli(argv)
            assert r.returncode == 1, argv
            assert USAGE[0] in r.stderr and USAGE[1] in r.stderr
            assert r.stderr.index(b"./main ld-window-regions ") < r.stderr.index(USAGE[0]) < r.stderr.index(USAGE[1])
        r = cli(["kinship", src, src, "all"])
        assert r.returncode == 134 and open(src, "rb").read() == data
        # a file that stops mid-way: exit 134, the pairs over the rows before the stop
        name, bad_file = next(x for x in SC.query_files(1) if x[0] == "no_lf17")
        with open(src, "wb") as f:
            f.write(bad_file)
        bd = KC.kin(bad_file)
        assert (bd[0], bd[3], len(bd[1])) == (E_FORMAT, 17, 17)
        r = cli(["kinship", src, out, "all"])
        assert r.returncode == 134 and b"VcfValidationError" in r.stderr and vcfc.strerror(E_FORMAT).encode() in r.stderr
        assert open(out, "rb").read() == KC.tsv(bad_file, bd[2])
        # a header the decoder refuses: the file created, empty
        with open(src, "wb") as f:
            f.write(data[1:])
        r = cli(["kinship", src, out, "all"])
        assert r.returncode == 134 and open(out, "rb").read() == b""


def test_file_2504_samples(ctx):
    """200 rows of 2504 samples: every table against a numpy count over a Python parse of the VCF text."""
    import random_vcf
    buf = io.BytesIO()
    random_vcf.generate(2504, 200, buf)
    vcf = buf.getvalue()
    enc = ctx.compress_buffer(vcf)
    g = np.array([[{3: 0, 2: 1, 0: 2, 1: -1}[MC.token_codes(t)[3]] for t in l.split(b"\t")[9:]]
                  for l in vcf.split(b"\n")[:-1] if not l.startswith(b"#")], dtype=np.int8)
    assert g.shape == (200, 2504) and (g == -1).any() and (g == 2).any()

    def count(rows):
        ind = [(rows == a).astype(np.float64) for a in range(3)]   # (exact: counts <= 200)
        want = np.zeros((2504, 2504, 3, 3), dtype=np.uint32)
        for a in range(3):
            for b in range(3):
                want[:, :, a, b] = ind[a].T @ ind[b]
        return want
    st, idx, t = ctx.kinship_buffer(enc)
    assert st == OK and idx.tolist() == list(range(200))
    assert t.shape == (2504, 2504, 3, 3) and np.array_equal(t, count(g))
    st, idx, t = ctx.kinship_buffer(enc, "1:%d-%d" % (10000 + 2 * 17, 10000 + 2 * 97))   # POS = 10000 + 2 i
    assert st == OK and idx.tolist() == list(range(17, 98)) and np.array_equal(t, count(g[17:98]))


def test_cell_indices_past_2_32():
    """S = 21 849, 3 rows: the square is 17 GB and S * S * 9 passes 2^32; in 512-sample slabs against a count made with
    torch from the unpacked genotype codes."""
    import torch
    import vcfc
    S, n = 21849, 3
    assert S * S * 9 > 1 << 32
    free = torch.cuda.mem_get_info(0)[0]
    if free < 48 << 30:
        pytest.skip("the device has %.1f GB free: the 17 GB square and its slabs need 48 GB" % (free / 2 ** 30))
    dev = "cuda:0"
    rb = (S + 3) // 4
    rnd = np.random.RandomState(11)
    bed = rnd.randint(0, 256, size=(n, rb)).astype(np.uint8)
    bed[:, -1] &= 0x03   # S mod 4 == 1: the pad bits are 00, as a 1|1 would be
    d_bed = torch.from_numpy(bed).to(dev)
    d_tables = torch.empty(S * S * 9, dtype=torch.int32, device=dev)
    wsb = vcfc.kin_workspace_size(n, S)
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    d_err = torch.zeros(1, dtype=torch.int64, device=dev)
    st = vcfc.kin_tables_device(d_bed.data_ptr(), n, rb, S, d_tables.data_ptr(), S * S, 0, d_ws.data_ptr(), wsb, d_err.data_ptr(),
                                _stream())
    torch.cuda.synchronize()
    assert st == OK and int(d_err.item()) == -1
    codes = torch.stack([(d_bed >> (2 * k)) & 3 for k in range(4)], dim=2).reshape(n, 4 * rb)[:, :S]
    g = torch.tensor([2, -1, 1, 0], device=dev)[codes.long()]                              # .bed code -> genotype
    onehot = torch.stack([(g == a) for a in range(3)], dim=2).float()                      # [n, S, 3]
    right = onehot.reshape(n, S * 3)
    t = d_tables.view(S, S, 3, 3)
    for i0 in range(0, S, 512):
        i1 = min(S, i0 + 512)
        left = onehot[:, i0:i1].permute(1, 2, 0).reshape((i1 - i0) * 3, n)
        want = (left @ right).view(i1 - i0, 3, S, 3).permute(0, 2, 1, 3).to(torch.int32)   # (exact: counts <= 3)
        assert torch.equal(t[i0:i1], want), i0
    assert int(t[S - 1, S - 1].sum().item()) == int((g[:, S - 1] >= 0).sum().item())
