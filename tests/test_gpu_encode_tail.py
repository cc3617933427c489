"""The tail of k_encode_fast's genotype stream on the GPU: the rows of
encode_tail_cases.py (1 to 8 genotype chunks: the prologue alone, the
load-free epilogue with 1, 2 and 3 chunks, one and two rounds of the refill
loop) through vcfc.encode_rows_device at line alignments 0, 1, 15 and 16 --
every record byte for byte the oracle's, every offset the sum of its sizes,
the error word clear.  The emulator test (test_encode_tail_emu.py) shows
which path each row takes; here the lanes run at once, the buffer loads clamp
to the row's range and the counted vmcnt waits are the hardware's.  Needs a
gfx950 GPU (-m gpu)."""
import os
import sys

import numpy as np
import pytest

import encode_tail_cases as TC
import golden_io as G

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(G.REPO, "vcf-compression_amd"))


@pytest.fixture(scope="module")
def torch():
    import torch as T   # import before libvcfc: one HIP runtime in the process
    assert T.cuda.is_available(), "GPU tests need a GPU"
    return T


@pytest.fixture(scope="module")
def vcfc(torch):
    import vcfc as V
    return V


def _encode(torch, vcfc, lines, lead):
    """b"#" * lead, then the lines, each followed by LF, through
    vcfc.encode_rows_device (deferred records on, the default): (out, rec_off,
    error word)."""
    buf = bytearray(b"#" * lead)
    offs, lens = [], []
    for ln in lines:
        offs.append(len(buf))
        lens.append(len(ln))
        buf += ln + b"\n"
    dev = torch.device("cuda:0")
    d_buf = torch.from_numpy(np.frombuffer(bytes(buf) + b"\0" * 64, dtype=np.uint8).copy()).to(dev)
    d_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    d_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    n, total = len(lines), sum(lens)
    ws_bytes = vcfc.workspace_size(n, total)
    cap = vcfc.encode_bound(n, total)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.full((cap,), 0xEE, dtype=torch.uint8, device=dev)
    rec = torch.empty(n + 1, dtype=torch.int64, device=dev)
    err = torch.empty(1, dtype=torch.int64, device=dev)
    vcfc.encode_rows_device(d_buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, total, out.data_ptr(), cap,
                            rec.data_ptr(), ws.data_ptr(), ws_bytes, err.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out, rec.cpu().numpy().astype(np.uint64), int(err.cpu().numpy().view(np.uint64)[0])


def _check(vcfc, got, tags, want, lead):
    out, rec, err = got
    assert err == vcfc.NO_ERROR, (tags[0][0], lead, hex(err))
    assert np.array_equal(rec, np.cumsum([0] + [len(w) for w in want]).astype(np.uint64)), (tags[0][0], lead)
    host = out[:int(rec[-1])].cpu().numpy().tobytes()
    if host != b"".join(want):
        o = 0
        for t, w in zip(tags, want):
            assert host[o:o + len(w)] == w, (t, lead)
            o += len(w)


@pytest.mark.parametrize("name", TC.FAMILIES)
def test_tail_family_vs_oracle(torch, vcfc, name):
    tags, lines = TC.family(name)
    want = TC.expected(name)
    for lead in TC.LEADS:
        _check(vcfc, _encode(torch, vcfc, lines, lead), tags, want, lead)


def test_tail_mixed_batch(torch, vcfc):
    """Every row of every family in one batch (218 rows), neighbours of
    different chunk counts: the four waves of a k_encode_fast block leave
    the stream at different points -- after the prologue, in the loop, in the
    epilogue, by a refusal or the hand-on."""
    tags, lines, want = TC.mixed_batch()
    assert len({TC.nchunks(t[1]) for t in tags[:8]}) > 2
    for lead in TC.LEADS:
        _check(vcfc, _encode(torch, vcfc, lines, lead), tags, want, lead)
