"""The tail of k_encode_fast's genotype stream on the emulator: rows of 1 to
8 genotype chunks (encode_tail_cases.py) -- the prologue alone, the load-free
epilogue with 1, 2 and 3 chunks, one and two rounds of the refill loop --
with runs across every chunk boundary, escapes in the first and last chunk, a
chunk the fast steps refuse at every chunk position and the hand-on of an
all-escape chunk 0, at line alignments 0, 1, 15 and 16: every record byte
for byte the oracle's, every offset its sizes' sum, the error word clear.

The emulator also tells what the GPU test cannot: no row of the zero,
boundary and escape families reaches the general path or is deferred, and
the hand-on rows of more than one chunk are exactly the deferred ones."""
import numpy as np
import pytest

import emu_io as E
import encode_tail_cases as TC


def run(lines, lead):
    """b"#" * lead, then the lines, each followed by LF (test_kernel_emu.run)."""
    buf = bytearray(b"#" * lead)
    offs, lens = [], []
    for ln in lines:
        offs.append(len(buf))
        lens.append(len(ln))
        buf += ln + b"\n"
    return E.emu_encode(bytes(buf), np.array(offs, np.uint64), np.array(lens, np.uint32))


def _check(name, lead, lines, want):
    st, out, ro, err = run(lines, lead)
    assert err == TC.NO_ERROR, (name, lead, hex(err))
    assert np.array_equal(ro, np.cumsum([0] + [len(w) for w in want]).astype(np.uint64)), (name, lead)
    tags = TC.family(name)[0] if name in TC.FAMILIES else TC.mixed_batch()[0]
    for i, w in enumerate(want):
        assert out[int(ro[i]):int(ro[i + 1])] == w, (tags[i], lead)


@pytest.mark.parametrize("lead", TC.LEADS)
@pytest.mark.parametrize("name", TC.FAMILIES)
def test_tail_family_vs_oracle(name, lead, monkeypatch):
    monkeypatch.delenv("EMU_DEFER", raising=False)   # (deferred records on: the default)
    tags, lines = TC.family(name)
    _check(name, lead, lines, TC.expected(name))
    if name in ("zero", "boundary", "escape"):
        assert E.LAST_RETRIES[0] == 0 and E.last_deferred() == 0
    elif name == "handon":
        assert E.last_deferred() == sum(TC.nchunks(T) > 1 for _, T, _ in tags)


def test_tail_handon_without_deferred_records(monkeypatch):
    """Deferred records off: the all-escape chunk 0 stays on the fast kernel
    (esc8), whatever the row's chunk count."""
    monkeypatch.setenv("EMU_DEFER", "0")
    _check("handon", 1, TC.family("handon")[1], TC.expected("handon"))
    assert E.LAST_RETRIES[0] == 0 and E.last_deferred() == 0


def test_tail_mixed_batch(monkeypatch):
    """Every row of every family in one batch, neighbours of different chunk
    counts (the GPU test's batch)."""
    monkeypatch.delenv("EMU_DEFER", raising=False)
    tags, lines, want = TC.mixed_batch()
    _check("mixed", 15, lines, want)
