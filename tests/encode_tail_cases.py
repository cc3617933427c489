"""Rows aimed at the tail of k_encode_fast's genotype stream, shared by the
emulator test (test_encode_tail_emu.py) and the GPU test
(test_gpu_encode_tail.py).

encode_fast (csrc/vcfc_encode.hip) streams a row's genotype region in 2 KiB
chunks of 512 token slots, three chunks in flight: a prologue loads chunks
0 .. 2, a refill loop runs while chunk C + 3 exists (three steps and three
refills a round), and a load-free epilogue takes the row's last one to three
chunks.  The sample counts below give ncG = ceil(T / 512) = 1 .. 8 chunks:
the prologue alone (T <= 1536: an epilogue of 1, 2 and 3 chunks), one round
of the loop with an epilogue of 1, 2 and 3 chunks (T = 1537 .. 3072) and two
rounds (T = 3073, 3585), with the row's last chunk holding one slot, all but
one, and all of its 512.

Every family is built by hand from (T, chunk index); nothing is drawn at
random.  expected() is the oracle's record of every row, computed once."""
import functools

import golden_io as G

SLOTS = 512   # token slots of a 2 KiB genotype chunk (SLOTS8)
SAMPLES = (1, 2, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 2504, 2560, 2561, 3072, 3073,
           3585)
LEADS = (0, 1, 15, 16)   # bytes before the first line: its alignment mod 16, and one whole 16 further
FAMILIES = ("zero", "boundary", "escape", "length", "refused", "handon")
NO_ERROR = (1 << 64) - 1


def nchunks(T):
    return (T + SLOTS - 1) // SLOTS


def _row(T, toks, tag):
    """A data line of the fast shape's prefix and these tokens; the prefix
    length varies with the row so that token 0 starts on every byte phase."""
    pfx = b"22\t%d\trs%d\tA\tG\t100\tPASS\t%s\tGT\t" % (16050075 + T, tag, b"P" * (1 + (T + tag) % 7))
    return pfx + b"\t".join(toks)


def zero(T):
    """All 0|0: the whole-chunk skip in every chunk, the 127-token run bytes
    counted across the chunk ends."""
    return [_row(T, [b"0|0"] * T, 0)]


def boundary(T):
    """A non-reference token in the last slot of every chunk (the row's last
    token included) and in the first slot of the next chunk: a run crosses
    every chunk boundary."""
    toks = [b"0|0"] * T
    for k in range(1, nchunks(T)):
        toks[k * SLOTS - 1] = toks[k * SLOTS] = (b"0|1", b"1|1", b"1|0")[k % 3]
    toks[T - 1] = b"1|1"
    return [_row(T, toks, 1)]


def escape(T):
    """A 0|2 escape in chunk 0 and one in the last chunk."""
    toks = [b"0|0" if (j // 40) % 3 else b"0|1" for j in range(T)]
    toks[min(3, T - 1)] = b"0|2"
    toks[max((nchunks(T) - 1) * SLOTS, T - 4)] = b"0|2"
    return [_row(T, toks, 2)]


def length(T):
    """For every chunk g whose slots can hold it, one row with a 7-byte token
    (two slots with its TAB, so the region stays a whole number of slots and
    the row reaches the genotype stream) in chunk g: gt_step8 refuses the
    chunk there, the general step takes it and refuses the row, which the
    variable-token kernel encodes.  The token sits in the chunk's second
    half where the chunk has one (the general step then encodes the first
    half before it refuses).  T counts slots: the row has T - 1 tokens."""
    rows = []
    for g in range(nchunks(T)):
        s = min(g * SLOTS + 300, T - 2)   # the token takes slots s and s + 1
        if s < g * SLOTS:
            continue   # (a last chunk of one slot: refused() covers it)
        toks = [b"0|0" if (j // 50) % 2 else b"1|0" for j in range(T)]
        toks[s:s + 2] = [b"0|1:3:9"]
        rows.append(_row(T, toks, 3 + g))
    return rows


def refused(T):
    """For every chunk g, one row whose chunk g holds a 3-byte token that
    neither gt_step8 nor the general step takes (a vertical tab, 0x0B, as
    its second allele): the stream is left at every chunk position, the
    row's last chunk included, whatever that chunk's size."""
    rows = []
    for g in range(nchunks(T)):
        s = min(g * SLOTS + 200, T - 1)
        toks = [b"0|0" if (j // 60) % 2 else b"1|1" for j in range(T)]
        toks[s] = b"0|\x0b"
        rows.append(_row(T, toks, 20 + g))
    return rows


def handon(T):
    """Chunk 0 all escapes (unphased tokens), plain tokens after it: with
    deferred records on, a row of more than one chunk is handed on to the
    variable-token kernel at chunk 0 (f.hand == 2) -- from the epilogue for
    two and three chunks, from the refill loop (its remaining loads
    redirected to an empty range) for more."""
    toks = [(b"0/1", b"./.", b"1/1")[j % 3] if j < SLOTS else (b"0|0" if (j // 30) % 2 else b"0|1") for j in range(T)]
    return [_row(T, toks, 40)]


_BUILD = {"zero": zero, "boundary": boundary, "escape": escape, "length": length, "refused": refused,
          "handon": handon}


@functools.lru_cache(maxsize=None)
def family(name):
    """(tags, lines) of a family over SAMPLES: tags[i] = (name, T, index
    among T's rows) of lines[i]."""
    tags, lines = [], []
    for T in SAMPLES:
        for k, ln in enumerate(_BUILD[name](T)):
            tags.append((name, T, k))
            lines.append(ln)
    return tuple(tags), tuple(lines)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's records of family(name), computed once; every row encodes."""
    recs = []
    for ln in family(name)[1]:
        st, rec = G.oracle_encode_line(ln)
        assert st == 0, name
        recs.append(rec)
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """(tags, lines, records): every row of every family in one batch, the
    families interleaved sample count by sample count, so that the four rows
    of a k_encode_fast block have different chunk counts and leave the
    stream at different points."""
    rows = []
    for name in FAMILIES:
        tags, lines = family(name)
        rows += list(zip(tags, lines, expected(name)))
    rows.sort(key=lambda r: (r[0][2], FAMILIES.index(r[0][0]), r[0][1]))
    out = []   # stride through the sorted rows: neighbours differ in T by several chunks
    stride = 7
    for s in range(stride):
        out += rows[s::stride]
    assert len(out) == len(rows) >= 200
    return tuple(r[0] for r in out), tuple(r[1] for r in out), tuple(r[2] for r in out)
