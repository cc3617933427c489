"""GPU parity for the binned external index (reference create_binned_index4,
src/main.cpp:1284-1637, and query_binned_index_binarysearch, :2974-3349):
byte-exact against the reference CLI's recorded index files, stdout and exit
codes (tests/golden/binned_index_cases.json) through the C ABI (libvcfc.so)
and the CLI (build/main), the device entry points on freshly encoded batches
against the restatement (index_cases.py), the indexed query against the
full-scan query at 2504 samples, and the hand-built edge families of
index_edge_cases.py -- records compress would not write, both error codes,
the error word's order, a short entries_cap, ends at and above 2^32 -- with
the odd-field and mutated-file cases, uploaded as they stand: the same checks
test_index_emu.py runs on the emulator."""
import io
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import golden_io as G
import index_cases as X
import index_edge_cases as EC

pytestmark = pytest.mark.gpu
REPO = G.REPO
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
MAIN = os.path.join(REPO, "build", "main")
OK, E_ARG, E_FORMAT = 0, 5, 8
NO_ERROR = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    import torch   # before libvcfc: one HIP runtime in the process
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import vcfc
    c = vcfc.Context(0)
    yield c
    c.close()


_INDEX = {}


def golden_or_built_index(ctx, name, b):
    """The index of a golden file at bin b: the reference's bytes where they
    are stored, else this build's (checked against the reference's hash)."""
    if (name, b) not in _INDEX:
        c = X.index_case(name, b)
        idx = X.golden_index(c)
        if idx is None:
            st, idx, _ = ctx.create_binned_index_status(X.file_bytes(name), b)
            assert st == OK and X.sha(idx) == c["index_sha256"]
        _INDEX[(name, b)] = idx
    return _INDEX[(name, b)]


def test_golden_index_cases(ctx):
    for c in X.cases()["index_cases"]:
        st, idx, bad = ctx.create_binned_index_status(X.file_bytes(c["file"]), c["bin"])
        if c["rc"] == 0:
            assert st == OK and len(idx) == c["index_len"] and X.sha(idx) == c["index_sha256"], (c["file"], c["bin"])
        else:   # the reference throws on record 10
            assert st == E_FORMAT and idx == b"" and bad == 10, (c["file"], c["bin"], st, bad)
    assert ctx.create_binned_index_status(X.file_bytes("index_edge"), 0)[0] == E_ARG
    with pytest.raises(RuntimeError):
        ctx.create_binned_index(X.file_bytes("throw_end"), 2)


def test_golden_query_cases(ctx):
    for c in X.cases()["query_cases"]:
        idx = golden_or_built_index(ctx, c["index_file"], c["bin"])
        st, out = ctx.query_binned_index_status(X.file_bytes(c["file"]), idx, c["region"], cap=64)
        assert X.check_query_case(c, st, out), (c, st, len(out))
        if c["rc"] != 0:   # every line before the throw
            assert (st, out) == X.query(X.file_bytes(c["file"]), idx, c["region"])
    v = X.file_bytes("index_edge")
    idx = golden_or_built_index(ctx, "index_edge", 1)
    assert ctx.query_binned_index_status(v, idx[:-1], "1:100-200")[0] == E_FORMAT   # not a multiple of 13
    assert ctx.query_binned_index_status(v, b"", "1:100-200") == (OK, b"")
    assert ctx.query_binned_index_status(v, idx[:13], "1:100-200") == X.query(v, idx[:13], "1:100-200")
    assert ctx.query_binned_index(v, idx, "1:100-200") == X.query(v, idx, "1:100-200")[1]


def test_cli_messages():
    d = X.cases()
    with tempfile.TemporaryDirectory() as wd:
        f, n = os.path.join(wd, "f.vcfc"), os.path.join(wd, "noidx.vcfc")
        for p in (f, n):
            with open(p, "wb") as fh:
                fh.write(X.file_bytes("index_edge"))
        with open(f + ".vcfci", "wb") as fh:
            fh.write(X.golden_index(X.index_case("index_edge", 2)))
        sub = {"{f}": f, "{m}": os.path.join(wd, "missing.vcfc"), "{n}": n}
        for c in d["cli_cases"]:
            r = subprocess.run([MAIN] + [sub.get(a, a) for a in c["argv"]], capture_output=True, timeout=300)
            out = r.stdout.decode()
            for k, v in sub.items():
                out = out.replace(v, k)
            assert (r.returncode, out) == (c["rc"], c["stdout"]), (c, r.stderr)
        r = subprocess.run([MAIN, "create-binned-index", "0", f], capture_output=True, timeout=300)
        assert (r.returncode, r.stdout) == (1, b"bin size must be a positive integer\n")
        r = subprocess.run([MAIN, "frobnicate"], capture_output=True, timeout=300)
        assert r.stdout == b"Unknown action name: frobnicate\n"


FILES = sorted({c["file"] for c in X.cases()["index_cases"]})


@pytest.mark.parametrize("name", FILES)
def test_cli_create_matches_reference_files(name):
    with tempfile.TemporaryDirectory() as wd:
        path = os.path.join(wd, "f.vcfc")
        with open(path, "wb") as f:
            f.write(X.file_bytes(name))
        for c in X.cases()["index_cases"]:
            if c["file"] != name:
                continue
            if os.path.exists(path + ".vcfci"):
                os.unlink(path + ".vcfci")
            r = subprocess.run([MAIN, "create-binned-index", str(c["bin"]), path], capture_output=True, timeout=300)
            idx = open(path + ".vcfci", "rb").read()
            assert r.stdout == b""
            assert len(idx) == c["index_len"] and X.sha(idx) == c["index_sha256"], (name, c["bin"])
            assert r.returncode == (0 if c["rc"] == 0 else 134), (name, c["bin"], r.returncode, r.stderr)


GROUPS = sorted({(c["file"], c["index_file"], c["bin"]) for c in X.cases()["query_cases"]})


@pytest.mark.parametrize("name,index_file,b", GROUPS)
def test_cli_query_matches_reference_stdout(ctx, name, index_file, b):
    with tempfile.TemporaryDirectory() as wd:
        path = os.path.join(wd, "f.vcfc")
        with open(path, "wb") as f:
            f.write(X.file_bytes(name))
        idx = golden_or_built_index(ctx, index_file, b)
        with open(path + ".vcfci", "wb") as f:
            f.write(idx)
        for c in X.cases()["query_cases"]:
            if (c["file"], c["index_file"], c["bin"]) != (name, index_file, b):
                continue
            r = subprocess.run([MAIN, "query-binned-index", path, c["region"]], capture_output=True, timeout=300)
            if c["rc"] == 0:
                assert r.returncode == 0 and len(r.stdout) == c["stdout_len"], (c, r.stderr)
                assert X.sha(r.stdout) == c["stdout_sha256"], c
            else:   # reference: SIGABRT after a partial flush; here exit 134 after every line before the throw
                assert r.returncode == 134, (c, r.stderr)
                assert r.stdout == X.query(X.file_bytes(name), idx, c["region"])[1]
                assert X.sha(r.stdout[:c["stdout_len"]]) == c["stdout_sha256"], c


def test_cli_done_when_lines():
    """create-binned-index 100 then query-binned-index 1:10100-10104 on
    random_100x10000: the three lines the reference prints."""
    vcf = G.gz("random_100x10000.vcf.gz")
    want = [l + b"\n" for l in vcf.split(b"\n") if l[:2] == b"1\t" and 10100 <= int(l.split(b"\t", 2)[1]) <= 10104]
    with tempfile.TemporaryDirectory() as wd:
        path = os.path.join(wd, "f.vcfc")
        with open(path, "wb") as f:
            f.write(G.gz("random_100x10000.vcfc.gz"))
        assert subprocess.run([MAIN, "create-binned-index", "100", path], timeout=300).returncode == 0
        r = subprocess.run([MAIN, "query-binned-index", path, "1:10100-10104"], capture_output=True, timeout=300)
        assert r.returncode == 0 and len(want) == 3 and r.stdout == b"".join(want)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4095, 4096, 4097, 70001])
def test_device_entry_points(n):
    """Encode S = 2 rows on the GPU, then index the encoder's d_out /
    d_rec_off in place: entries, count and the per-record spans against the
    restatement."""
    import torch
    import vcfc
    dev = "cuda:0"
    lines = X.gen_lines(n, 1000 + n, samples=2)
    ll = np.array([len(x) for x in lines], dtype=np.uint32)
    lo = np.zeros(n, dtype=np.uint64)
    lo[1:] = np.cumsum(ll[:-1].astype(np.uint64) + 1)
    buf = np.frombuffer(b"\n".join(lines) + b"\n", dtype=np.uint8)
    total = int(ll.sum(dtype=np.uint64))
    t_buf = torch.from_numpy(buf.copy()).to(dev)
    t_lo = torch.from_numpy(lo.view(np.int64)).to(dev)
    t_ll = torch.from_numpy(ll.view(np.int32)).to(dev)
    cap = vcfc.encode_bound(n, total)
    wsb = vcfc.workspace_size(n, total)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    rec = torch.empty(n + 1, dtype=torch.int64, device=dev)
    err = torch.empty(1, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    vcfc.encode_rows_device(t_buf.data_ptr(), t_lo.data_ptr(), t_ll.data_ptr(), n, total, out.data_ptr(), cap,
                            rec.data_ptr(), ws.data_ptr(), wsb, err.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(err.item()) == -1
    r = rec.cpu().numpy()
    hdr = X.header(2)
    v = hdr + out[:int(r[n])].cpu().numpy().tobytes()
    sp, bad = X.spans_of(v)
    assert bad is None and len(sp) == n and [s_[0] - len(hdr) for s_ in sp] == r[:n].tolist()
    # spans, element-wise
    ref = torch.empty(n, dtype=torch.uint8, device=dev)
    pos = torch.empty(n, dtype=torch.int64, device=dev)
    end = torch.empty(n, dtype=torch.int64, device=dev)
    vcfc.record_span_device(out.data_ptr(), rec.data_ptr(), n, ref.data_ptr(), pos.data_ptr(), end.data_ptr(),
                            err.data_ptr(), s)
    torch.cuda.synchronize()
    assert int(err.item()) == -1
    assert ref.cpu().tolist() == [x[1] for x in sp]
    assert pos.cpu().numpy().view(np.uint64).tolist() == [x[2] for x in sp]
    assert end.cpu().numpy().view(np.uint64).tolist() == [x[3] for x in sp]
    # entries
    iws_b = vcfc.index_workspace_size(n)
    iws = torch.empty(iws_b, dtype=torch.uint8, device=dev)
    ent = torch.empty(13 * n + 16, dtype=torch.uint8, device=dev)
    words = torch.empty(2, dtype=torch.int64, device=dev)   # count, largest end
    for E in (1, 7, 4096):
        ent.fill_(0xEE)
        vcfc.binned_index_device(out.data_ptr(), rec.data_ptr(), n, len(hdr), E, ent.data_ptr(), n,
                                 words.data_ptr(), words.data_ptr() + 8, iws.data_ptr(), iws_b, err.data_ptr(), s)
        torch.cuda.synchronize()
        want = X.pack(X.sequential_entries(sp, E))
        assert int(err.item()) == -1
        w = words.cpu().numpy().view(np.uint64)
        assert int(w[0]) == len(want) // 13 and int(w[1]) == max(x[3] for x in sp), (n, E)
        got = ent.cpu().numpy()
        assert got[:len(want)].tobytes() == want, (n, E)
        assert (got[len(want):] == 0xEE).all()


def test_index_2504x4000(ctx):
    """On sorted single-chromosome SNV data the indexed query and the
    full-scan query agree; both equal the VCF's own lines."""
    import random_vcf
    buf = io.BytesIO()
    random_vcf.generate(2504, 4000, buf)
    vcf = buf.getvalue()
    enc = ctx.compress_buffer(vcf)
    idx = ctx.create_binned_index(enc, 64)
    assert idx == X.build_index(enc, 64)[1] and len(idx) == 13 * 63
    lines = vcf[vcf.index(b"\n1\t") + 1:].split(b"\n")[:-1]
    # POS = 10000 + 2 i: a range picks lines i in [a, b]
    for a, b in ((0, 0), (17, 1017), (3990, 3999), (1234, 1233), (2047, 2049)):
        q = "1:%d-%d" % (10000 + 2 * a, 10000 + 2 * b)
        st, got = ctx.query_binned_index_status(enc, idx, q)
        st_f, full = ctx.query_buffer(enc, q)
        assert st == OK and st_f == OK and got == full == b"".join(l + b"\n" for l in lines[a:b + 1]), (a, b)


# ---- the hand-built edge families (index_edge_cases.py) on the GPU -------------------

def u64(t):
    return t.cpu().numpy().view(np.uint64).tolist()


@pytest.fixture(scope="module")
def gpu(ctx):
    """The callables index_edge_cases.py checks: the device entry points on
    the uploaded records, create and query through the C ABI."""
    import torch
    import vcfc
    dev = "cuda:0"

    def span(v):
        d, rec, n, h, _ = EC.upload(v)
        ref = torch.empty(n, dtype=torch.uint8, device=dev)
        pos = torch.empty(n, dtype=torch.int64, device=dev)
        end = torch.empty(n, dtype=torch.int64, device=dev)
        err = torch.empty(1, dtype=torch.int64, device=dev)
        vcfc.record_span_device(d.data_ptr(), rec.data_ptr(), n, ref.data_ptr(), pos.data_ptr(), end.data_ptr(),
                                err.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return u64(err)[0], ref.cpu().tolist(), u64(pos), u64(end)

    def device(v, E, cap):
        d, rec, n, h, _ = EC.upload(v)
        cap = n if cap is None else cap
        ent = torch.full((13 * cap + 16,), 0xEE, dtype=torch.uint8, device=dev)
        words = torch.empty(2, dtype=torch.int64, device=dev)   # count, largest end
        err = torch.empty(1, dtype=torch.int64, device=dev)
        wsb = vcfc.index_workspace_size(n)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        vcfc.binned_index_device(d.data_ptr(), rec.data_ptr(), n, h, E, ent.data_ptr(), cap, words.data_ptr(),
                                 words.data_ptr() + 8, ws.data_ptr(), wsb, err.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        w, got = u64(words), ent.cpu().numpy()
        used = min(w[0], cap)
        if u64(err)[0] == NO_ERROR or u64(err)[0] & 0xFF == 0xFF:
            assert (got[13 * used:] == 0xEE).all(), "entries written past the count or entries_cap"
        assert (got[13 * cap:] == 0xEE).all(), "entries written past entries_cap"
        return [u64(err)[0], w[0], w[1]], got[:13 * used].tobytes()

    class B:
        pass
    B.span, B.device = staticmethod(span), staticmethod(device)
    B.create = staticmethod(lambda v, E: ctx.create_binned_index_status(v, E))
    B.query = staticmethod(lambda v, idx, q, **kw: ctx.query_binned_index_status(v, idx, q))
    return B


@pytest.mark.parametrize("family", sorted(EC.BINNED))
def test_edge_family(gpu, family):
    EC.BINNED[family](gpu)


@pytest.mark.parametrize("n", EC.NS)
def test_edge_prefix_max(gpu, n):
    EC.binned_prefix_max(gpu, n)


def test_edge_prefix_max_second_trip(gpu):
    """65 836 records: 258 block maxima, so k_idx_partials takes its second trip."""
    EC.binned_prefix_max_second_trip(gpu)


def test_odd_fields(gpu):
    EC.check_odd_fields(gpu)


@pytest.mark.parametrize("seed", EC.MUTATE_SEEDS)
def test_mutated_files(gpu, seed):
    EC.check_mutated_binned(gpu, seed)
