"""The encoder's rows, shared by the emulator tests (test_kernel_emu.py) and
the GPU tests (test_gpu_encode.py): every family is a function that returns
VCF data lines (bytes, without the LF), and both suites check the records
the kernels make of them against the oracle (golden_io.oracle_encode_line).

Seeded families (moved here from the emulator tests' bodies; the seeds and
the order of the draws are theirs, so the rows are byte for byte the same):
caps, ring_wrap, esc3, esc_chunk_end, sparse_ranges, wide_multi_chunk,
chr22_like, var_rows / gdg (with PFX_V).

Hand-built families (edge_rows(); nothing about the edge is drawn at random):
prefix_edge_{fast,esc,var,general}, size_edge, run_edge, esc_dense; cap_values() gives
the out_cap values around every record boundary of a batch, error_batch()
the batches with failing rows.

The kernel constants they are aimed at (csrc/vcfc_encode.hip): a wave's LDS
ring RING = 4096 bytes, flushed in bursts of BURST = 1024; prefix chunks of
1 KiB (16 bytes a lane), genotype chunks of 2 KiB (32 bytes, 8 token slots a
lane; 512 tokens a chunk); run caps 127 (0|0) and 31; per-row primary staging
of prim_bytes = 1024 or 2048 bytes; compaction tiles of CT = 4096 output
bytes in 16-byte blocks; scan tiles of 4096 rows."""
import functools
import random

import golden_io as G

CLASSES = [b"0|0", b"0|1", b"1|0", b"1|1"]
NO_ERROR = (1 << 64) - 1
E_NOSPACE = 4


# ---- seeded families --------------------------------------------------------

def wide_multi_chunk(seed):
    """Rows spanning many 1 KiB chunks: clean, with an empty field, and with
    long runs."""
    rnd = random.Random(seed)
    pfx = b"22\t16050075\trs1\tA\tG\t100\tPASS\t" + b"AF=0.1;" * rnd.randint(1, 300) + b"\tGT\t"
    toks = []
    for _ in range(rnd.randint(2000, 5000)):
        r = rnd.random()
        toks.append(b"0|0" if r < 0.85 else b"0|1" if r < 0.9 else b"1|1" if r < 0.95 else b"1|0" if r < 0.99 else b"2|1")
    clean = pfx + b"\t".join(toks)
    dirty = pfx + b"\t".join(toks[:100]) + b"\t\t" + b"\t".join(toks[100:])
    runs = pfx + b"\t".join([b"0|0"] * 4000 + [b"1|1"] * 100)
    return [clean, dirty, runs]


def chr22_like(seed, n=40, samples=2504):
    """Long 0|0 runs: the whole-chunk skip, 127-token run boundaries that
    straddle chunks, run transitions at chunk starts."""
    rnd = random.Random(seed)
    rows = []
    for i in range(n):
        af = rnd.choice([0.0, 0.0005, 0.002, 0.01, 0.05, 0.3, 0.9])
        multi = rnd.random() < 0.1
        toks = []
        for _ in range(samples):
            a = [1 if rnd.random() < af else 0 for _ in range(2)]
            if multi and rnd.random() < 0.01:
                a[rnd.randint(0, 1)] = 2
            toks.append(b"%d|%d" % (a[0], a[1]))
        pfx = b"22\t%d\trs%d\tA\tG\t100\tPASS\tAC=1;AF=%.4f;NS=2504\tGT\t" % (16050075 + 32 * i, i, af)
        rows.append(pfx + b"\t".join(toks))
    return rows


def caps(seed):
    """Rows whose first and last genotype chunk coincide (< 256 samples), and
    runs whose lengths sit on and around the caps (31, 127) and the 256-slot
    chunk, at every class."""
    rnd = random.Random(seed)
    lens = [1, 2, 3, 4, 5, 29, 30, 31, 32, 33, 61, 62, 63, 125, 126, 127, 128, 129, 253, 254, 255, 256, 257]
    lines = []
    for i in range(48):
        toks = []
        target = rnd.choice([1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 700, 1500])
        while len(toks) < target:
            c = rnd.choice(CLASSES)
            toks += [c] * rnd.choice(lens)
        toks = toks[:target]
        pfx = b"22\t%d\trs%d\tA\tG\t100\tPASS\t%s\tGT\t" % (100 + i, i, b"X" * rnd.randint(1, 40))
        lines.append(pfx + b"\t".join(toks))
    return lines


def ring_wrap(seed):
    """Rows whose records are many times the 4 KiB LDS ring (a run start at
    most tokens): run groups straddling the ring end, bursts every chunk."""
    rnd = random.Random(seed)
    lines = []
    for i in range(6):
        n = rnd.choice([9000, 17000, 24001])
        p = rnd.choice([0.5, 0.9, 1.0])
        toks, c = [], 0
        for _ in range(n):
            if rnd.random() < p:
                c = rnd.randrange(4)
            toks.append(CLASSES[c])
        pfx = b"22\t%d\trs%d\tA\tG\t100\tPASS\tAF=0.5\tGT\t" % (100 + i, i)
        lines.append(pfx + b"\t".join(toks))
    return lines


def esc3(seed):
    """3-byte escape tokens (multi-allelic, missing, unphased, raw high bytes)
    at every density, at token 0, at chunk edges (512-token chunks), at the
    row end, in runs of escapes, and right after runs that end on the caps."""
    rnd = random.Random(seed)
    escs = [b"0|2", b"2|0", b"./.", b".|.", b"0/1", b"1/1", b"2|2", b"\xff|\x80", b"0|\r", b"3|1"]
    lens = [1, 2, 30, 31, 32, 126, 127, 128, 511, 512, 513]
    lines = []
    for i in range(24):
        target = rnd.choice([1, 2, 511, 512, 513, 1024, 1025, 2504, 5000])
        dens = rnd.choice([0.0005, 0.01, 0.04, 0.3, 1.0])
        toks = []
        while len(toks) < target:
            if rnd.random() < dens:
                toks += [rnd.choice(escs)] * rnd.choice([1, 1, 1, 2, 5])
            else:
                toks += [rnd.choice(CLASSES)] * rnd.choice(lens)
        toks = toks[:target]
        for p in rnd.sample([0, 510, 511, 512, 1023, 1024, target - 1], 3):
            if 0 <= p < target:
                toks[p] = rnd.choice(escs)
        pfx = b"22\t%d\trs%d\tA\tG,T\t100\tPASS\t%s\tGT\t" % (100 + i, i, b"Y" * rnd.randint(1, 60))
        lines.append(pfx + b"\t".join(toks))
    return lines


PFX_V = b"X\t100\trs1\tA\tG\t50\tPASS\tAC=1\tGT\t"


def var_rows(rnd, n, kinds):
    """Rows of odd-length tokens (the variable-token kernel's shape)."""
    rows = []
    for i in range(n):
        kind = kinds[i % len(kinds)]
        S = rnd.choice([1, 2, 3, 17, 63, 64, 65, 200, 511, 512, 513, 1023, 1024, 1025, 1500, 2600])
        toks = []
        p00 = rnd.choice([0.0, 0.5, 0.9, 0.99, 1.0])
        for j in range(S):
            if kind == "hap":       # haploid beside diploid
                toks.append(rnd.choice([b"0", b"1"]) if (j * 7 + i) % 3 == 0 else
                            (b"0|0" if rnd.random() < p00 else rnd.choice([b"0|1", b"1|0", b"1|1", b"0|0"])))
            elif kind == "dot":     # "." for missing
                toks.append(b"." if rnd.random() < 0.2 else (b"0|0" if rnd.random() < p00 else
                                                                  rnd.choice([b"0|1", b"1|1", b"2|1"])))
            elif kind == "long":    # GT:DP:GQ and other odd lengths
                toks.append(rnd.choice([b"0|0:35:99", b"0|1:17:12", b"1|1:123:9", b"0|0", b"1", b"./.",
                                        b"0|0:1", b"0" * 41]))
            elif kind == "gdg":     # escapes of 1, 5, 9 and 41 bytes only (the escape-chunk step)
                toks.append(rnd.choice([b"0|0:35:99", b"0|1:17:12", b"1|1:123:9", b"0|0:1", b"1", b"0" * 41]))
            elif kind == "ones":    # every token one byte
                toks.append(rnd.choice([b"0", b"1", b"."]))
            else:                   # plain runs with long 1-byte stretches
                toks.append(b"0|0" if (j // 200) % 2 == 0 else b"1")
        rows.append(PFX_V + b"\t".join(toks))
    return rows


VAR_KINDS = ["hap", "dot", "long", "ones", "runs", "gdg"]


def var(seed):
    """72 rows of var_rows, every kind."""
    return var_rows(random.Random(seed), 72, VAR_KINDS)


def gdg(rnd, S):
    """One GT:DP:GQ row of S samples."""
    return PFX_V + b"\t".join(b"%d|%d:%d:%d" % (rnd.randint(0, 1), rnd.randint(0, 1), rnd.randint(10, 99),
                                             rnd.randint(10, 99)) for _ in range(S))


def gdg_batch(seed, n=12, S=700):
    """GT:DP:GQ rows of one sample count (deferred, their sizes predicted)
    with a staged 3-byte-token row after every third of them."""
    rnd = random.Random(seed)
    lines = []
    for i in range(n):
        lines.append(gdg(rnd, S))
        if i % 3 == 2:
            lines.append(PFX_V + b"\t".join(CLASSES[(i + j) % 4] for j in range(1 + 13 * i)))
    return lines


def esc_chunk_end(seed):
    """Rows whose genotype region is a whole number of 2 KiB chunks (1024 /
    2048 one-byte tokens, 1024 GT:DP:GQ tokens) beside rows one half-slot
    shorter and longer."""
    rnd = random.Random(seed)
    lines = []
    for S in (1023, 1024, 1025, 2047, 2048, 2049):
        lines.append(PFX_V + b"\t".join(rnd.choice([b"0", b"1", b"."]) for _ in range(S)))
    for S in (1023, 1024, 1025):
        lines.append(PFX_V + b"\t".join(b"%d|%d:%d:%d" % (rnd.randint(0, 1), rnd.randint(0, 1), rnd.randint(10, 99),
                                                         rnd.randint(10, 99)) for _ in range(S)))
    return lines


def sparse_ranges(seed):
    """512-token chunks holding 0, 1, a few, 62, 63, 64 or 65 non-0|0 tokens,
    runs of one class crossing chunk ends, 0|0 gaps spanning whole chunks and
    127-multiples, ranges cut by dense, escape and last chunks, and an event
    at token 0."""
    rnd = random.Random(seed)
    classes = [b"0|1", b"1|0", b"1|1"]
    lines = []
    for i in range(16):
        nch = rnd.choice([3, 5, 6, 9, 13])
        toks = []
        for c in range(nch):
            kind = rnd.choice(["zero", "few", "edge", "edge", "dense", "esc", "run"])
            chunk = [b"0|0"] * 512
            if kind == "few":
                for p in rnd.sample(range(512), rnd.choice([1, 2, 5, 20])):
                    chunk[p] = rnd.choice(classes)
            elif kind == "edge":
                for p in rnd.sample(range(512), rnd.choice([61, 62, 63, 64, 65])):
                    chunk[p] = rnd.choice(classes)
            elif kind == "dense":
                chunk = [rnd.choice(classes + [b"0|0"]) for _ in range(512)]
            elif kind == "esc":
                chunk[rnd.randrange(512)] = b"0|2"
            elif kind == "run":   # one class from near the chunk end into the next chunk
                cl = rnd.choice(classes)
                for p in range(512 - rnd.randint(1, 40), 512):
                    chunk[p] = cl
                toks += chunk
                chunk = [cl] * rnd.randint(1, 40) + [b"0|0"] * 600
                chunk = chunk[:512]
            toks += chunk
        if rnd.random() < 0.5:
            toks[0] = rnd.choice(classes)
        toks = toks[:len(toks) - rnd.randrange(300)]
        pfx = b"22\t%d\trs%d\tA\tG\t100\tPASS\t%s\tGT\t" % (100 + i, i, b"Z" * rnd.randint(1, 50))
        lines.append(pfx + b"\t".join(toks))
    return lines


# (function, the seeds the emulator tests run it with)
SEEDED = {
    "caps": (caps, (21, 22, 23)),
    "ring_wrap": (ring_wrap, (31, 32)),
    "esc3": (esc3, (41, 42, 43)),
    "esc_chunk_end": (esc_chunk_end, (2024,)),
    "sparse_ranges": (sparse_ranges, (51, 52, 53, 54)),
    "wide_multi_chunk": (wide_multi_chunk, (1, 2, 3)),
    "chr22_like": (chr22_like, (11, 12)),
    "var": (var, (51, 52, 53)),
    "gdg_batch": (gdg_batch, (5,)),
}


# SHA-256 (first 16 hex digits) of b"\\n".join(lines) of the seeded families,
# taken from the emulator tests' bodies before the rows moved here: the rows
# the suites have always run stay the rows they run
SEEDED_SHA256 = {
    ("caps", 21): "c33d537151f5c046",
    ("caps", 22): "f5fd491df4163c08",
    ("caps", 23): "50746a55b08a76d6",
    ("chr22_like", 11): "b3882161942d7cdd",
    ("chr22_like", 12): "1e6d0fdee8f4c273",
    ("esc3", 41): "4278f007f9d3ccfb",
    ("esc3", 42): "a62a20341e2ca784",
    ("esc3", 43): "87b985ab01ca72aa",
    ("esc_chunk_end", 2024): "ea8fa789c1faf38d",
    ("ring_wrap", 31): "b491b26024b7c8c8",
    ("ring_wrap", 32): "2d7a8607354267af",
    ("sparse_ranges", 51): "1a09532e14cf35e5",
    ("sparse_ranges", 52): "f9c52eeb30f9ce8a",
    ("sparse_ranges", 53): "78458ee9f7614c2e",
    ("sparse_ranges", 54): "82aef0478a8eadf7",
    ("var", 51): "fcf249017e552c63",
    ("var", 52): "1d50f5b8bf26ded2",
    ("var", 53): "146fa82ba9cb37fa",
    ("wide_multi_chunk", 1): "b5504a5da9d7b579",
    ("wide_multi_chunk", 2): "9e6e48ab17bf7125",
    ("wide_multi_chunk", 3): "67b56d0d21607faa",
}


# ---- hand-built families ----------------------------------------------------

# prefix lengths (through the TAB after FORMAT): around one and two prefix
# chunks, around the ring (4096 less the 8 header bytes, and the ring itself),
# around two rings, and far past them (real INFO columns are longer than the
# ring); then every residue mod 32 near 100 bytes, so the first sample starts
# on every byte of a lane's 32
PREFIX_LENS = [1000, 1015, 1016, 1017, 2040, 2048, 4080, 4088, 4089, 4090, 4096, 4100, 5000, 8184, 8192, 9000,
               20000, 70000] + list(range(100, 132))
PREFIX_SAMPLES = (1, 3, 300, 2504)
PREFIX_SHAPES = ("fast", "esc", "var", "general")


def prefix_of(n):
    """Nine columns and their TABs in exactly n bytes: one long INFO field."""
    head, tail = b"22\t16050075\trs1\tA\tG\t100\tPASS\t", b"\tGT\t"
    assert n > len(head) + len(tail)
    p = head + b"I" * (n - len(head) - len(tail)) + tail
    assert len(p) == n and p.count(b"\t") == 9
    return p


def _plain(j):
    """Token j of the fast shape: runs of 1 .. 5 tokens over the four classes."""
    return CLASSES[(j // (1 + j % 5)) % 4]


def shape_tokens(shape, S):
    """S sample tokens joined by TABs: fast (a|b only), esc (0|2 and ./. among
    them, 0|2 first), var (0, 1 and 0|1:33:99: odd lengths only) or general
    (an even-length token and, from three tokens on, an empty field)."""
    if shape == "fast":
        return b"\t".join(_plain(j) for j in range(S))
    if shape == "esc":
        return b"\t".join(b"0|2" if j % 7 == 0 else b"./." if j % 11 == 5 else _plain(j) for j in range(S))
    if shape == "var":
        return b"\t".join((b"0", b"1", b"0|1:33:99")[(j + j // 5) % 3] for j in range(S))
    assert shape == "general"
    toks = [b"10" if j == S // 2 else _plain(j) for j in range(S)]
    if S < 3:
        return b"\t".join(toks)
    return b"\t".join(toks[:S // 3]) + b"\t\t" + b"\t".join(toks[S // 3:])


def prefix_edge(shape):
    return [prefix_of(n) + shape_tokens(shape, S) for n in PREFIX_LENS for S in PREFIX_SAMPLES]


PFX_S = b"22\t1\trs\tA\tG\t1\tPASS\t.\tGT\t"
SIZE_BASES = (1024, 2048, 3072, 4096, 8192, 12288)
TINY = PFX_S + b"0|1"


def size_row(target):
    """A row whose record is exactly `target` bytes: the 8 header bytes, the
    prefix, one byte per token (0|1 and 1|0 in turn: runs of one) and the LF."""
    T = target - 9 - len(PFX_S)
    assert T >= 1
    return PFX_S + b"\t".join((b"0|1", b"1|0")[j & 1] for j in range(T))


def size_edge(base):
    """Records of base + d bytes, d = -3 .. 3, each followed by a one-token
    row and two more copies: record ends and starts on both sides of a
    compaction block (16 B), a tile (4 KiB), a burst and the primary staging's
    end, at every d."""
    lines = []
    for d in range(-3, 4):
        r = size_row(base + d)
        assert len(G.oracle_encode_line(r)[1]) == base + d
        lines += [r, TINY, r, r]
    return lines


def prim_bytes(n, total):
    """vcfc_prim_bytes (csrc/vcfc_device.h)."""
    return 2048 if n and total // n >= 4096 else 1024


def size_edge_batch(base, pb):
    """(lines, total_line_bytes or None): the size_edge(base) batch with
    primary staging size pb (vcfc_prim_bytes) -- its own, or the other one,
    reached by a larger total_line_bytes (1024 -> 2048; the ABI takes any
    bound of the sum) or by short rows behind the batch (2048 -> 1024)."""
    lines = size_edge(base)
    n, total = len(lines), sum(len(x) for x in lines)
    if prim_bytes(n, total) == pb:
        return lines, None
    if pb == 2048:
        return lines, 4096 * n
    pad = total // 4096 + 2 - n
    lines = lines + [TINY] * pad
    assert prim_bytes(len(lines), total + pad * len(TINY)) == 1024
    return lines, None


SIZE_BATCHES = [(base, pb) for base in SIZE_BASES for pb in (1024, 2048)]


RUN_ENDS = (255, 256, 257, 511, 512, 513, 1023, 1024)


def run_edge():
    """For each class, runs of cap * m + d tokens (cap 127 for 0|0, else 31;
    m = 1, 2, 4; d = -1, 0, 1) that end at token 255 .. 257, 511 .. 513, 1023,
    1024 (the token after the run has that index) and at the row's last
    token, followed by another class, by the same class after a one-token
    break, and by an escape.  The tokens before the run alternate between
    two other classes."""
    lines = []

    def row(toks):
        i = len(lines)
        pfx = b"22\t%d\trs%d\tA\tG\t100\tPASS\t%s\tGT\t" % (100 + i, i, b"X" * (1 + i % 16))
        lines.append(pfx + b"\t".join(toks))

    for c in range(4):
        cap = 127 if c == 0 else 31
        a, b, o = CLASSES[(c + 1) % 4], CLASSES[(c + 2) % 4], CLASSES[(c + 3) % 4]
        tail = [b, a] * 3
        for m in (1, 2, 4):
            for d in (-1, 0, 1):
                L = cap * m + d
                run = [CLASSES[c]] * L
                for end in RUN_ENDS:
                    if L > end:
                        continue
                    pre = [(a, b)[j & 1] for j in range(end - L)]
                    row(pre + run + [o] * 3 + tail)
                    row(pre + run + [a] + [CLASSES[c]] * 5 + tail)
                    row(pre + run + [b"0|2"] + [CLASSES[c]] * 2 + tail)
                row([(a, b)[j & 1] for j in range(40)] + run)
    return lines


def esc_dense():
    """Chunks of 512 three-byte escapes on the fast kernel: 5 record bytes a
    token, 2 560 a chunk, the most a chunk can add to the ring -- with 512
    bytes or more pending before it, a flush has three bursts to send, and
    consecutive such chunks alternate between two and three.  Token 0 is
    plain (a first chunk of escapes only is handed to k_encode_var when
    records may be deferred) or an escape too; prefixes put every quarter of
    a burst pending before the first genotype chunk; the row ends one token
    into a chunk, on its last token, and in its middle."""
    lines = []
    for first in (b"0|1", b"0|2"):
        for S in (513, 1024, 1537, 2600):
            for P in (100, 356, 612, 868):
                toks = [first] + [(b"0|2", b"./.", b"2|1")[j % 3] for j in range(1, S)]
                lines.append(prefix_of(P) + b"\t".join(toks))
    return lines


EDGE_FAMILIES = tuple("prefix_edge_" + s for s in PREFIX_SHAPES) + tuple("size_edge_%d" % b for b in SIZE_BASES) + \
    ("run_edge", "esc_dense")


@functools.lru_cache(maxsize=None)
def edge_rows():
    """{family: lines} of the hand-built families EDGE_FAMILIES (size_edge:
    the six batches at their own primary staging size; size_edge_batch() has
    both)."""
    fam = {"prefix_edge_" + s: prefix_edge(s) for s in PREFIX_SHAPES}
    for base in SIZE_BASES:
        fam["size_edge_%d" % base] = size_edge(base)
    fam["run_edge"] = run_edge()
    fam["esc_dense"] = esc_dense()
    assert tuple(fam) == EDGE_FAMILIES
    return fam


# families whose rows all have the fast kernel's shape (3-byte tokens, a
# clean prefix): none of them may reach the general path
FAST_SHAPED = ("prefix_edge_fast", "prefix_edge_esc", "run_edge", "esc_dense") + tuple("size_edge_%d" % b for b in SIZE_BASES)
# families with rows for the variable-token kernel (esc_dense: the rows it is handed
# when records may be deferred): run with and without deferred records
VAR_SHAPED = ("prefix_edge_var", "esc_dense")


@functools.lru_cache(maxsize=None)
def family(name, seed=None):
    """Lines of a seeded or hand-built family (made once)."""
    return tuple(SEEDED[name][0](seed)) if name in SEEDED else tuple(edge_rows()[name])


@functools.lru_cache(maxsize=None)
def expected(name, seed=None):
    """The oracle's records of family(name, seed), computed once; every line
    of a family encodes."""
    recs = []
    for ln in family(name, seed):
        st, rec = G.oracle_encode_line(ln)
        assert st == 0, name
        recs.append(rec)
    return tuple(recs)


def all_families():
    """(name, seed) of every family."""
    return [(n, s) for n, (_, seeds) in SEEDED.items() for s in seeds] + [(n, None) for n in EDGE_FAMILIES]


def cap_values(sizes):
    """out_cap values for records of these sizes: 0, 1, 7, 8, every record
    boundary - 1 / 0 / + 1, the total - 1 and the total (ascending, once each)."""
    bounds, o = [], 0
    for s in sizes:
        o += s
        bounds.append(o)
    total = o
    vals = {0, 1, 7, 8, total - 1, total}
    for b in bounds:
        vals.update((b - 1, b, b + 1))
    return sorted(v for v in vals if 0 <= v <= total)


def cap_expected(sizes, cap):
    """(error word, first row whose record ends past cap) for out_cap = cap;
    (NO_ERROR, len(sizes)) when every record fits."""
    o = 0
    for i, s in enumerate(sizes):
        o += s
        if o > cap:
            return (i << 8) | E_NOSPACE, i
    return NO_ERROR, len(sizes)


ERROR_BATCHES = ("eight_then_seven", "seven_then_eight", "three_tiles")


def error_batch(name):
    """(lines, error word, first failing row): the golden seven_cols (error
    1) and eight_cols (error 2) lines among good rows -- two short batches,
    and 9 000 rows with failing rows in three scan tiles (and so three blocks
    of every kernel), the first of them reported."""
    ec = {c["name"]: c for c in G.edge_cases()["cases"]}
    ok = bytes.fromhex(ec["run300_00"]["line"])
    eight = bytes.fromhex(ec["eight_cols"]["line"])
    seven = bytes.fromhex(ec["seven_cols"]["line"])
    if name == "eight_then_seven":
        return [ok, ok, eight, ok, seven], (2 << 8) | 2, 2
    if name == "seven_then_eight":
        return [ok, seven, eight], (1 << 8) | 1, 1
    assert name == "three_tiles"
    big = [PFX_S + b"\t".join(CLASSES[(i + j) & 3] for j in range(1 + i % 23)) for i in range(9000)]
    big[8000], big[4097], big[37] = seven, eight, eight
    return big, (37 << 8) | 2, 37
