"""GPU parity for extract (extract-samples, extract-regions):
whole bytes, status, error word and offsets against the Python restatement
(extract_cases.py, pinned to the oracle and to the reference CLI's digests by
test_extract_emu.py) through the C ABI (libvcfc.so), the device entry on torch
tensors, the file calls and the CLI (build/main); the reference digests; and
the two laws that tie it to the product's own decoder:
decompress(extract(v, cols)) == decompress-samples(v, cols), and
extract(extract(v, A), B) == extract(v, [A[b] for b in B])."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import decode_cases as D
import extract_cases as EC
import golden_io as G
import reader_edge_cases as RE
import regions_cases as RC
import subset_cases as SC

pytestmark = pytest.mark.gpu
REPO = G.REPO
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))
MAIN = os.path.join(REPO, "build", "main")
OK, E_ARG, E_FORMAT = EC.OK, EC.E_ARG, EC.E_FORMAT


@pytest.fixture(scope="module")
def ctx():
    import torch   # before libvcfc: one HIP runtime in the process
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import vcfc
    c = vcfc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ext(ctx):
    import vcfc

    def run(data, cols=None, query=None, regions=None):
        q = None if query is None else vcfc.VcfCoordinateQuery(*query)
        return ctx.extract_buffer(data, cols, query=q, regions=regions)
    return run


def test_valid_files(ext):
    EC.check_files(ext, D.valid_files(1), 1)


@pytest.mark.parametrize("seed", [3, 4, 6])
def test_mutated_files(ext, seed):
    EC.check_files(ext, D.mutated_files(seed), seed)


def test_hand_built_records(ext):
    import vcfc
    EC.check_hand_built(ext)
    assert vcfc.extract_workspace_size(1, EC.TILE + 1) > vcfc.extract_workspace_size(1, EC.TILE)


def test_batch_sizes(ext):
    EC.check_files(ext, SC.batch_files())


def test_query_files_and_region_tables(ext):
    EC.check_queries(ext, 1)


def test_golden_digests(ext):
    EC.check_golden(ext)
    data = G.gz("random_100x10000.vcfc.gz")
    assert ext(data) == (OK, data)


def test_decompress_of_extract_is_decompress_samples(ctx, ext):
    files = D.valid_files(1) + [(n, d) for n, d, _, code in EC.hand_built() if code == 0]
    checked = 0
    for name, data in files:
        S = SC.parse_header(data)[1]
        for cols in SC.column_sets(S, 1)[2:6]:
            st, cut = ext(data, cols)
            assert st == EC.extract(data, cols)[0], name
            if st == OK:   # (empty_escape: refused where an empty token is chosen)
                assert ctx.decompress_buffer(cut) == ctx.decompress_samples_buffer(data, cols), (name, cols[:8])
                checked += 1
    assert checked >= 3 * len(files)


def test_extract_of_extract(ext):
    import random
    rnd = random.Random(5)
    files = D.valid_files(1)[2:] + [(n, d) for n, d, _, code in EC.hand_built() if code == 0]
    for name, data in files:
        S = SC.parse_header(data)[1]
        A = rnd.sample(range(S), max(1, S * 2 // 3))
        if name == "empty_escape":
            A = [c for c in A if c not in (10, S - 1)]   # (its empty tokens: refused where chosen)
        for B in (list(range(len(A))), list(range(len(A) - 1, -1, -1)), rnd.sample(range(len(A)), max(1, len(A) // 2))):
            st, first = ext(data, A)
            assert st == OK
            assert ext(first, B) == ext(data, [A[b] for b in B]), (name, len(A), len(B))


def test_bad_arguments_and_short_buffer(ctx, ext):
    data = D.valid_files(1)[2][1]   # S = 64
    for cols in ([], [64], [0, 64], [3, 3], [5, 1, 5]):
        assert ext(data, cols) == (E_ARG, b"") and ext(data, cols, query=SC.QUERIES[0]) == (E_ARG, b""), cols
        assert ext(data, cols, regions=RC.SETS["A"]) == (E_ARG, b""), cols
    assert ext(data[1:], [0]) == (E_FORMAT, b"") and ext(data[1:]) == (E_FORMAT, b"")
    # a short buffer: VCFC_E_NOSPACE and the size needed (the wrapper then retries with it)
    want = EC.extract(data, [63, 0])
    assert ctx.extract_buffer(data, [63, 0], cap=len(want[1]) - 1) == want
    assert ctx.extract_buffer(data, [63, 0], cap=0) == want
    wq = EC.extract(data, [63, 0], query=(b"22", False, 0, 0))
    assert len(wq[1]) > len(want[1]) // 2 and ctx.extract_buffer(data, [63, 0], query="22", cap=5) == wq


def device_run(data, cols, select, cap, base):
    """vcfc_extract_samples_device on the records of a well-formed file:
    (status, err word, record offsets, out bytes); 64 canary bytes past
    out_cap, the bytes before the output base and the fill past the last
    record that fits are checked on every call."""
    import torch
    import vcfc
    h, S = SC.parse_header(data)
    body = data[h:]
    rec, end = SC.hop(body)
    n = len(rec)
    dev = "cuda:0"
    K = S if cols is None else len(cols)
    d_in = torch.from_numpy(np.frombuffer(body + bytes(64), dtype=np.uint8).copy()).to(dev)
    d_rec = torch.from_numpy(np.array(rec + [end], dtype=np.int64)).to(dev)
    d_sel = None if select is None else torch.from_numpy(np.array(select, dtype=np.uint8)).to(dev)
    total = vcfc.extract_bound(len(body), n, K) if cap is None else cap
    d_buf = torch.full((16 + total + 64,), 0xEE, dtype=torch.uint8, device=dev)
    d_roff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_err = torch.zeros(1, dtype=torch.int64, device=dev)
    wsb = vcfc.extract_workspace_size(n, max(K, 1))
    d_ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    st = vcfc.extract_samples_device(d_in.data_ptr(), len(body), d_rec.data_ptr(),
                                     None if d_sel is None else d_sel.data_ptr(), n, S, cols, d_buf.data_ptr() + base, total,
                                     d_roff.data_ptr(), d_ws.data_ptr(), wsb, d_err.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    buf = d_buf.cpu().numpy()
    out = buf[base:]
    roff = [int(x) for x in d_roff.cpu().tolist()]
    assert (buf[:base] == 0xEE).all() and (out[total:] == 0xEE).all(), "bytes written outside [out, out + out_cap)"
    if st == OK:
        used = max(x for x in roff if x <= total) if cap is not None else roff[-1]
        assert (out[used:total] == 0xEE).all(), "bytes written past the last record that fits"
    return st, int(d_err.cpu().numpy().view(np.uint64)[0]), roff, out[:total].tobytes()


def test_device_entry():
    EC.check_device(device_run)


def test_bound():
    import vcfc
    EC.check_bound(vcfc.extract_bound)


def test_files_and_cli(ctx):
    vcf = G.gz("random_100x10000.vcf.gz")
    enc = G.gz("random_100x10000.vcfc.gz")
    names = vcf[vcf.index(b"#CHROM"):].split(b"\n", 1)[0].split(b"\t")[9:]
    cols = [77, 3, 50]
    pick = b",".join(names[c] for c in cols).decode()
    q = (b"1", True, 10100, 10300)
    regions = b"1:10100-10300\n1:20000-20100\n"
    with tempfile.TemporaryDirectory() as d:
        src, dst, reg = os.path.join(d, "t.vcfc"), os.path.join(d, "o.vcfc"), os.path.join(d, "r.txt")
        with open(src, "wb") as f:
            f.write(enc)
        with open(reg, "wb") as f:
            f.write(regions)
        # the file calls
        for kw in ({}, {"query": "1:10100-10300"}, {"regions": regions}):
            for cc in (cols, None):
                ctx.extract_file(src, dst, cc, **kw)
                want = EC.extract(enc, cc, query=q if "query" in kw else None, regions=kw.get("regions"))
                hdr = EC.header(enc, SC.parse_header(enc)[0], cc)
                assert want[0] == OK and len(want[1]) > len(hdr) + 100 and open(dst, "rb").read() == want[1], (kw, cc)
        # the CLI
        r = subprocess.run([MAIN, "extract-samples", src, dst, pick], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert open(dst, "rb").read() == EC.extract(enc, cols)[1]
        r = subprocess.run([MAIN, "extract-samples", src, dst, pick, "1:10100-10300"], capture_output=True, timeout=300)
        assert r.returncode == 0 and open(dst, "rb").read() == EC.extract(enc, cols, query=q)[1], r.stderr
        r = subprocess.run([MAIN, "extract-regions", src, dst, reg], capture_output=True, timeout=300)
        assert r.returncode == 0 and open(dst, "rb").read() == EC.extract(enc, None, regions=regions)[1], r.stderr
        r = subprocess.run([MAIN, "extract-regions", src, dst, reg, pick], capture_output=True, timeout=300)
        assert r.returncode == 0 and open(dst, "rb").read() == EC.extract(enc, cols, regions=regions)[1], r.stderr
        # names the header lacks: a message, exit 1, nothing written
        os.remove(dst)
        r = subprocess.run([MAIN, "extract-samples", src, dst, pick + ",nobody"], capture_output=True, timeout=300)
        assert (r.returncode, r.stdout) == (1, b"Unknown sample name: nobody\n") and not os.path.exists(dst)
        r = subprocess.run([MAIN, "extract-samples", src, src, pick], capture_output=True, timeout=300)
        assert r.returncode == 134
        # too few arguments: the usage text, which still holds the earlier actions' lines
        for argv in (["extract-samples", src, dst], ["extract-regions", src, dst]):
            r = subprocess.run([MAIN] + argv, capture_output=True, timeout=300)
            assert r.returncode == 1
            for l in (b"./main [compress|decompress|sparsify] <input_file> <output_file>\n",
                      b"./main export-bed-regions <input_file> <output_prefix> <regions-file>\n",
                      b"./main extract-samples <input_file> <output_file> <name>[,<name>...] [<ref>[:<start>-<end>]]\n",
                      b"./main extract-regions <input_file> <output_file> <regions-file> [<name>[,<name>...]]\n"):
                assert l in r.stderr
        # a file that stops mid-way: exit 134 with the header and the records before the stop written
        name, bad = next(x for x in SC.query_files(1) if x[0] == "no_lf17")
        with open(src, "wb") as f:
            f.write(bad)
        r = subprocess.run([MAIN, "extract-samples", src, dst, "S0,S5"], capture_output=True, timeout=300)
        want = EC.extract(bad, [0, 5])
        assert r.returncode == 134 and want[0] == E_FORMAT and open(dst, "rb").read() == want[1]


# ---- the byte-serial lanes' later passes and the stager's edges (reader_edge_cases.py) ----

def test_queue_pass(ext):
    import vcfc
    RE.check_queue_is_longer_than_the_lanes(vcfc.extract_workspace_size, 2)
    RE.check_queue_extract([ext], device_run)


@pytest.mark.parametrize("fam", RE.FAMILIES)
def test_stager_edges(ext, fam):
    RE.check_edges_extract(ext, fam)
