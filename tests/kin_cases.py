"""kinship restated in Python, and its test inputs.

The feature has no reference action: its oracle is this restatement over the
.bed rows of matrix_cases.py -- the genotype of a 2-bit code, the 3 x 3 table
of two samples, the square of all pairs, the statistics of a table in integer
and float arithmetic, and the text file.  test_kin_emu.py pins it to a
hand-written known answer, to genotype-counts and to its own symmetries, then
holds the kernels and driver to it on the CPU emulator; test_gpu_kin.py does
the same on the GPU.  Every comparison is exact."""
import numpy as np

import decode_cases as D
import ld_cases as LC
import matrix_cases as MC
import regions_cases as RC
import subset_cases as SC

OK, E_NOSPACE, E_ARG, E_FORMAT = MC.OK, MC.E_NOSPACE, MC.E_ARG, MC.E_FORMAT
NO_RECORD, NO_ERROR = MC.NO_RECORD, MC.NO_ERROR
FILL, CANARY = MC.FILL, MC.CANARY
TILE_SAMPLES = 32    # samples a side of a block of k_kin_pairs   (the emulator suite holds these three
CHUNK_WORDS = 16     # variant words of a staged sample in LDS      to csrc/vcfc_device.h)
PLANE_ROWS = 256     # variant rows of a block of k_kin_planes
TSV_HEAD = b"#ID_A\tID_B\tN\tIBS0\tIBS1\tIBS2\tHETHET\tHET_A\tHET_B\tDST\tKINSHIP\n"
G_OF_CODE = {3: 0, 2: 1, 0: 2, 1: None}   # VCFC_GM_BED code -> genotype


def genotypes(bed_row, S):
    """The S genotypes of a .bed row (None: missing); the pad bits are never looked at."""
    return [G_OF_CODE[(bed_row[s >> 2] >> (2 * (s & 3))) & 3] for s in range(S)]


def table(gi, gj):
    """The table of two samples: gi, gj = their genotypes, row by row."""
    t = [0] * 9
    for a, b in zip(gi, gj):
        if a is not None and b is not None:
            t[3 * a + b] += 1
    return t


def square(bed_rows, S):
    """uint32[S, S, 9]: the table of every pair of samples (indicator products; test_kin_emu holds it to `table`)."""
    g = np.array([[-1 if x is None else x for x in genotypes(r, S)] for r in bed_rows], dtype=np.int64).reshape(len(bed_rows), S)
    ind = [(g == a).astype(np.int64) for a in range(3)]
    out = np.zeros((S, S, 9), dtype=np.uint32)
    for a in range(3):
        for b in range(3):
            out[:, :, 3 * a + b] = ind[a].T @ ind[b]
    return out


def stats(t):
    """(N, IBS0, IBS1, IBS2, HH, HET_A, HET_B, DST or None, KINSHIP or None): Python integers, then one conversion
    per operand and one division."""
    t = [int(x) for x in t]
    N = sum(t)
    ibs0, ibs2, hh = t[2] + t[6], t[0] + t[4] + t[8], t[4]
    het_a, het_b = t[3] + t[4] + t[5], t[1] + t[4] + t[7]
    m = min(het_a, het_b)
    dst = float(2 * ibs2 + (N - ibs0 - ibs2)) / float(2 * N) if N else None
    kin = float(2 * hh - 4 * ibs0 + 2 * m - het_a - het_b) / float(4 * m) if m else None
    return N, ibs0, N - ibs0 - ibs2, ibs2, hh, het_a, het_b, dst, kin


def num_text(x):
    return b"nan" if x is None else b"%.6g" % x


def kin(v, query=None, table=None):
    """(status, indices, square uint32[S, S, 9], failing record): the rows are genotype-matrix's."""
    st, idx, rows, S, bad = MC.matrix(v, MC.BED, query, table)
    return st, idx, square(rows, S) if S else np.zeros((0, 0, 9), dtype=np.uint32), bad


def tsv(v, sq, min_kinship=None):
    """The text of the file entry for a square; min_kinship None: every pair."""
    data_off, S = SC.parse_header(v)
    names = v[v.rfind(b"\n", 0, data_off - 1) + 1:data_off - 1].split(b"\t")[9:]
    out = [TSV_HEAD]
    for i in range(S):
        for j in range(i + 1, S):
            x = stats(sq[i, j])
            if min_kinship is not None and not (x[8] is not None and x[8] >= min_kinship):
                continue
            out.append(b"\t".join([names[i], names[j]] + [b"%d" % k for k in x[:7]] + [num_text(x[7]), num_text(x[8])]) + b"\n")
    return b"".join(out)


# ---- inputs ---------------------------------------------------------------

# the known answer, counted by hand: 6 rows x 6 samples.  Samples 0..3:
#   r0: 0|0 0|1 1|1 0|1      r3: 0|1 0|0 1|1 1|1
#   r1: 0|1 0|1 0|0 ./.      r4: 0|0 0|0 0|1 1|0
#   r2: 1|1 1|0 0|0 0|1      r5: 1|0 1|1 ./. 0|0
# so g0 = 0 1 2 1 0 1, g1 = 1 1 1 0 0 2, g2 = 2 0 0 2 1 ., g3 = 1 . 1 2 1 0.
# (0, 1): (0,1) (1,1) (2,1) (1,0) (0,0) (1,2) -> cells 1 4 7 3 0 5: 1 1 0 1 1 1 0 1 0; N 6, IBS0 = t2 + t6 = 0, IBS2 = t0 +
#         t4 + t8 = 2, IBS1 4, HH 1, HET_A = t3 + t4 + t5 = 3, HET_B = t1 + t4 + t7 = 3: DST = (4 + 4) / 12, KINSHIP = (2 - 0 +
#         6 - 3 - 3) / 12 = 2 / 12
# (0, 2): rows 0..4: (0,2) (1,0) (2,0) (1,2) (0,1) -> cells 2 3 6 5 1: 0 1 1 1 0 1 1 0 0; N 5, IBS0 2, IBS2 0, IBS1 3, HH 0,
#         HET_A 2, HET_B 1, m 1: DST = 3 / 10, KINSHIP = (0 - 8 + 2 - 2 - 1) / 4 = -9 / 4
# (2, 3): rows 0 2 3 4: (2,1) (0,1) (2,2) (1,1) -> cells 7 1 8 4: 0 1 0 0 1 0 0 1 1; N 4, IBS0 0, IBS2 2, IBS1 2, HH 1, HET_A 1,
#         HET_B 3, m 1: DST = 6 / 8, KINSHIP = (2 - 0 + 2 - 1 - 3) / 4 = 0
# Sample 4 is 0|0 in every row (no heterozygote: m == 0 against everyone, N > 0) and sample 5 ./. in every row (N == 0):
# (i, 4) = the counts of g_i in cells 0 3 6; (0, 4) = 2 0 0 3 0 0 1 0 0: N 6, IBS0 = t6 = 1, IBS2 = t0 = 2, IBS1 3, HET_A 3,
#         HET_B 0: DST = (4 + 3) / 12, KINSHIP undefined;  (2, 4) = 2 0 0 1 0 0 2 0 0: N 5, IBS0 2, IBS2 2, IBS1 1: DST = 5 / 10
KAT_TOKENS = [[b"0|0", b"0|1", b"1|1", b"0|1"], [b"0|1", b"0|1", b"0|0", b"./."], [b"1|1", b"1|0", b"0|0", b"0|1"],
              [b"0|1", b"0|0", b"1|1", b"1|1"], [b"0|0", b"0|0", b"0|1", b"1|0"], [b"1|0", b"1|1", b"./.", b"0|0"]]
KAT_S = 6
KAT_TABLES = {(0, 0): [2, 0, 0, 0, 3, 0, 0, 0, 1], (0, 1): [1, 1, 0, 1, 1, 1, 0, 1, 0], (0, 2): [0, 1, 1, 1, 0, 1, 1, 0, 0],
              (0, 3): [0, 2, 0, 1, 0, 1, 0, 1, 0], (1, 2): [0, 1, 1, 2, 0, 1, 0, 0, 0], (1, 3): [0, 1, 1, 0, 2, 0, 1, 0, 0],
              (2, 3): [0, 1, 0, 0, 1, 0, 0, 1, 1], (2, 2): [2, 0, 0, 0, 1, 0, 0, 0, 2], (3, 3): [1, 0, 0, 0, 3, 0, 0, 0, 1],
              (1, 1): [2, 0, 0, 0, 3, 0, 0, 0, 1], (4, 4): [6, 0, 0, 0, 0, 0, 0, 0, 0], (5, 5): [0] * 9,
              (0, 4): [2, 0, 0, 3, 0, 0, 1, 0, 0], (1, 4): [2, 0, 0, 3, 0, 0, 1, 0, 0], (2, 4): [2, 0, 0, 1, 0, 0, 2, 0, 0],
              (3, 4): [1, 0, 0, 3, 0, 0, 1, 0, 0], (0, 5): [0] * 9, (1, 5): [0] * 9, (2, 5): [0] * 9, (3, 5): [0] * 9,
              (4, 5): [0] * 9}
# pair -> N IBS0 IBS1 IBS2 HH HET_A HET_B and the two strings
KAT_STATS = {(0, 0): (6, 0, 0, 6, 3, 3, 3, b"1", b"0.5"), (0, 1): (6, 0, 4, 2, 1, 3, 3, b"0.666667", b"0.166667"),
             (0, 2): (5, 2, 3, 0, 0, 2, 1, b"0.3", b"-2.25"), (0, 3): (5, 0, 5, 0, 0, 2, 3, b"0.5", b"-0.125"),
             (1, 2): (5, 1, 4, 0, 0, 3, 1, b"0.4", b"-1.5"), (1, 3): (5, 2, 1, 2, 2, 2, 3, b"0.5", b"-0.625"),
             (2, 3): (4, 0, 2, 2, 1, 1, 3, b"0.75", b"0"), (0, 4): (6, 1, 3, 2, 0, 3, 0, b"0.583333", b"nan"),
             (1, 4): (6, 1, 3, 2, 0, 3, 0, b"0.583333", b"nan"), (2, 4): (5, 2, 1, 2, 0, 1, 0, b"0.5", b"nan"),
             (3, 4): (5, 1, 3, 1, 0, 3, 0, b"0.5", b"nan"), (0, 5): (0, 0, 0, 0, 0, 0, 0, b"nan", b"nan"),
             (4, 5): (0, 0, 0, 0, 0, 0, 0, b"nan", b"nan")}
KAT_LINES = {(0, 1): b"S0\tS1\t6\t0\t4\t2\t1\t3\t3\t0.666667\t0.166667\n", (0, 2): b"S0\tS2\t5\t2\t3\t0\t0\t2\t1\t0.3\t-2.25\n",
             (2, 3): b"S2\tS3\t4\t0\t2\t2\t1\t1\t3\t0.75\t0\n", (2, 4): b"S2\tS4\t5\t2\t1\t2\t0\t1\t0\t0.5\tnan\n",
             (4, 5): b"S4\tS5\t0\t0\t0\t0\t0\t0\t0\tnan\tnan\n"}


def kat_file():
    lines = [b"1\t%d\trs%d\tA\tG\t1\tPASS\t.\tGT\t" % (100 + i, i) + b"\t".join(t + [b"0|0", b"./."]) for i, t in enumerate(KAT_TOKENS)]
    return D.encode_file(KAT_S, lines)


kin_file = LC.ld_file   # (S, n, miss, seed, last): the seeded files of ld_cases, shared and cached

SIZES = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 95, 96, 97)
ROWS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129)


def size_files():
    """(name, bytes): the sample counts around a tile of 32, a plane word, two tiles and a third; for S mod 4 != 0 files
    whose last real sample is 1|1 in every row (code 00, as the pad bits); 2504 samples with a handful of rows."""
    out = [("S%d" % S, kin_file(S, 7, 0.25 if S < 8 else 0.1)) for S in SIZES]
    out += [("S%d_last11" % S, kin_file(S, 6, 0.1, last=b"1|1")) for S in SIZES if S % 4]
    out.append(("S2504", kin_file(2504, 5, 0.1)))
    return out


def row_files():
    """(name, bytes, query): no row at all (a query that matches none of five records), the row counts around a plane
    word and a wave's 64 rows, and both sides of k_kin_planes' block and of the LDS chunk of variant words."""
    out = [("rows0", kin_file(33, 5, 0.15), (b"21", False, 0, 0))]
    out += [("rows%d" % n, kin_file(33, n, 0.15), None) for n in ROWS]
    edges = sorted({PLANE_ROWS - 1, PLANE_ROWS, PLANE_ROWS + 1, 32 * CHUNK_WORDS - 1, 32 * CHUNK_WORDS, 32 * CHUNK_WORDS + 1})
    out += [("rows%d" % n, kin_file(6, n, 0.3), None) for n in edges]
    return out


REGION_TEXTS = MC.REGION_TEXTS
QUERIES = MC.QUERIES


# ---- checks shared by the emulator and the GPU suites ----------------------
# run(data, query=None, regions=None, batch=0, text=None) ->
#     (status, indices, square uint32[S, S, 9], failing record, text of the file entry or None);
#     batch: records a batch of the driver (0: its default; a runner without the knob ignores it);
#     text: None: not asked for, "all", or the least kinship

def same(got, want, what):
    assert got[0] == want[0], (what, "status", got[0], want[0])
    assert got[3] == want[3], (what, "failing record", got[3], want[3])
    assert list(got[1]) == list(want[1]), (what, "indices")
    if want[0] not in (OK, E_FORMAT):
        return
    assert got[2].shape == want[2].shape, (what, "square", got[2].shape, want[2].shape)
    if not np.array_equal(got[2], want[2]):
        bad = np.argwhere(got[2] != want[2])
        raise AssertionError((what, "first differing cell (i, j, cell)", bad[0].tolist(), len(bad)))


def check_file(run, name, data, query=None, regions=None, batch=0, text=None):
    want = kin(data, query, RC.parse_text(regions) if regions is not None else None)
    got = run(data, query, regions, batch, text)
    same(got, want, (name, query, batch))
    if text is not None and got[4] is not None:
        past_header = want[0] in (OK, E_FORMAT) and SC.parse_header(data) and want[2].size
        assert got[4] == (tsv(data, want[2], None if text == "all" else text) if past_header else b""), (name, text)
    return want


def seen(squares):
    """What the seeded tables must cover, over the squares of a test: tables with every cell non-zero, pairs
    i < j with N == 0, pairs with N > 0 and m == 0."""
    full = empty = nohet = 0
    for sq in squares:
        t = sq.astype(np.int64)
        upper = np.triu(np.ones(t.shape[:2], dtype=bool), 1)
        N = t.sum(axis=2)
        m = np.minimum(t[:, :, 3:6].sum(axis=2), t[:, :, 1] + t[:, :, 4] + t[:, :, 7])
        full += int(((t != 0).all(axis=2) & upper).sum())
        empty += int(((N == 0) & upper).sum())
        nohet += int(((N > 0) & (m == 0) & upper).sum())
    return full, empty, nohet


def check_sizes(run):
    squares = []
    for name, data in size_files():
        want = check_file(run, name, data)
        assert want[0] == OK and len(want[1]) >= 5, name
        squares.append(want[2])
    assert seen(squares)[2] >= 5   # (pairs without a heterozygote; check_rows holds all three kinds)


def check_rows(run):
    squares = []
    for name, data, q in row_files():
        want = check_file(run, name, data, q)
        assert want[0] == OK and len(want[1]) == int(name[4:]), name
        assert int(want[2].sum(axis=2).max(initial=0)) <= len(want[1])
        squares.append(want[2])
    assert not squares[0].any()
    full, empty, nohet = seen(squares)
    assert full >= 5 and empty >= 5 and nohet >= 5, (full, empty, nohet)


def check_batches(run):
    """Batches of 1, 2, 31, 32, 33, 64 and 65 records over one file: the sum over batches is the one-batch answer; a
    query's flags and the stop rules with the failing record first and last in a batch."""
    data = kin_file(17, 130, 0.2)
    for b in (1, 2, 31, 32, 33, 64, 65):
        check_file(run, "batch%d" % b, data, batch=b)
    name, data = SC.query_files(1)[0]
    for b in (1, 7):
        for q in QUERIES[:3]:
            check_file(run, name, data, q, batch=b)
    for name, data, at in MC.irregular_files():
        for b in {max(at, 1), at + 1}:   # the failing record first in its batch, and last
            want = check_file(run, name, data, batch=b)
            assert (want[0], want[3], len(want[1])) == (E_FORMAT, at, at), name


def check_queries(run, seed=1):
    stopped = unstopped = 0
    for name, data in SC.query_files(seed):
        for q in (QUERIES if name == "valid" else QUERIES[:3] + QUERIES[5:6]):
            want = check_file(run, name, data, q)
            check_file(run, name, data, q, batch=17)   # records 17, 33 (34 = 2 x 17: last, first) and 59 fail in these files
            if q is not None and name.startswith(("no_lf", "nul_req")):
                stopped += want[0] == E_FORMAT
                unstopped += want[0] == OK
    assert stopped >= 5 and unstopped >= 5, (stopped, unstopped)


def check_regions(run, seed=1):
    hits = 0
    for text in REGION_TEXTS:
        for name, data in SC.query_files(seed)[:6]:
            want = check_file(run, name, data, regions=text)
            for b in (17, 18):   # records 17 and 33 fail in these files: first and last (17), last (18) in a batch
                check_file(run, name, data, regions=text, batch=b)
            hits += len(want[1]) > 0
    assert hits >= 6


def check_mutated(run, seed):
    """The stop rules: every mutated file, also in batches that put the failing record first and last."""
    ok = partial = 0
    for name, data in D.mutated_files(seed):
        want = check_file(run, name, data)
        if want[0] == E_FORMAT and want[3] != NO_RECORD:
            for b in {max(want[3], 1), want[3] + 1}:
                check_file(run, name, data, batch=b)
        ok += want[0] == OK
        partial += want[0] == E_FORMAT and len(want[1]) > 0
    assert ok >= 5 and partial >= 5, (ok, partial)


def check_irregular(run):
    for name, data, at in MC.irregular_files():
        want = check_file(run, name, data, text="all")
        assert (want[0], want[3], len(want[1])) == (E_FORMAT, at, at), name


def twin_file():
    """25 rows of 12 samples; sample 7 repeats sample 2 (a duplicate: KINSHIP 0.5, DST 1) and sample 9 is 1|1 or missing
    in every row (no heterozygote: KINSHIP undefined)."""
    if "kin_twin" not in LC._files:
        import random
        lines = LC.lines_of(random.Random(5 * 7919), 25, 12, 0.1)
        out = []
        for l in lines:
            f = l.split(b"\t")
            f[9 + 7] = f[9 + 2]
            f[9 + 9] = b"1|1" if f[9 + 9] not in LC.MISSING else f[9 + 9]
            out.append(b"\t".join(f))
        LC._files["kin_twin"] = D.encode_file(12, out)
    return LC._files["kin_twin"]


def check_tsv(run):
    """Every pair; a threshold equal to one pair's kinship (kept); 0.5 with a duplicated column present; undefined
    pairs; a file that stops at record 17."""
    data = twin_file()
    st, idx, sq, bad = kin(data)
    assert st == OK and len(idx) == 25
    x = stats(sq[2, 7])
    assert (x[7], x[8]) == (1.0, 0.5) and x[0] > 0
    vals = [stats(sq[i, j])[8] for i in range(12) for j in range(i + 1, 12)]
    defined = sorted(v for v in vals if v is not None)
    assert len(defined) >= 20 and vals.count(None) >= 5, "the file holds defined and undefined pairs"
    pick = defined[len(defined) // 2]
    assert pick < 0.5
    lines = {}
    for m in ("all", pick, 0.5, -100.0):
        check_file(run, "twin", data, text=m)
        lines[m] = tsv(data, sq, None if m == "all" else m).split(b"\n")[1:-1]
    assert len(lines["all"]) == 66 and sum(1 for l in lines["all"] if l.endswith(b"\tnan")) == vals.count(None)
    assert len(lines[-100.0]) == len(defined) and not any(l.endswith(b"nan") for l in lines[-100.0])
    assert len(lines[pick]) == sum(1 for v in defined if v >= pick)
    assert sum(1 for l in lines[pick] if l.endswith(b"\t" + num_text(pick))) >= 1, "the pair at the threshold is kept"
    assert any(l.startswith(b"S2\tS7\t") and l.endswith(b"\t1\t0.5") for l in lines[0.5])
    assert len(lines[0.5]) == sum(1 for v in defined if v >= 0.5) >= 1
    check_file(run, "kat", kat_file(), text="all")
    name, data = next(x for x in SC.query_files(1) if x[0] == "no_lf17")   # stops at record 17: the pairs over 17 rows
    want = check_file(run, name, data, text="all")
    assert (want[0], want[3], len(want[1])) == (E_FORMAT, 17, 17)


# ---- the two device entries ---------------------------------------------------
# tab(bed bytes, n_rows, row_stride, S, tables_cap, alloc_tables, accumulate=0, prefill=None, offset=0, ws_short=0,
#     null=None, n_override=None) -> (status, err word, the 36 * alloc_tables + CANARY bytes of the square's allocation);
#     the allocation held FILL, or `prefill` in its first bytes; byte `offset` (0..15) of an allocation is d_bed
# rec(body, rec, S, select, tables_cap, alloc_tables, accumulate=0, prefill=None, ws_short=0, null=None, n_override=None)
#     -> (status, err word, the allocation's bytes, row_of as a list of n + 1)

def expect_bytes(sq, alloc_tables):
    buf = bytearray([FILL]) * (36 * alloc_tables + CANARY)
    buf[:sq.size * 4] = sq.tobytes()
    return bytes(buf)


def bed_bytes(rows_bytes, S, stride):
    rb = MC.row_bytes(MC.BED, S)
    bed = bytearray([0x5A]) * (len(rows_bytes) * stride + 1)   # (0x5A: codes 10 10 01 01 between and behind the rows)
    for r, row in enumerate(rows_bytes):
        bed[r * stride:r * stride + rb] = row
    return bytes(bed)


def check_tables_call(tab, rows_bytes, S, stride_of=lambda rb: rb, offset=0, extra=0):
    stride = stride_of(MC.row_bytes(MC.BED, S))
    want = expect_bytes(square(rows_bytes, S), S * S + extra)
    st, err, got = tab(bed_bytes(rows_bytes, S, stride), len(rows_bytes), stride, S, S * S + extra, S * S + extra, offset=offset)
    what = (S, len(rows_bytes), stride, offset)
    assert st == OK and err == NO_ERROR, (what, st, err)
    assert got == want, (what, "first differing byte", LC.first_diff(got, want))


def check_tables_device(tab):
    for S, n in ((65, 18), (5, 9), (33, 70), (97, 6)):
        rows = MC.matrix(kin_file(S, n, 0.15, last=b"1|1"), MC.BED)[2]
        assert len(rows) == n
        for stride_of in (lambda rb: rb, lambda rb: (rb + 15) & ~15, lambda rb: rb + 1):
            check_tables_call(tab, rows, S, stride_of)
        for offset in range(16):
            check_tables_call(tab, rows, S, lambda rb: rb + 1, offset=offset)
        check_tables_call(tab, rows, S, extra=3)   # a roomier allocation: nothing past the square
        # accumulate: two calls on halves of the rows are one call on all of them; on a zeroed square it is a store
        rb = MC.row_bytes(MC.BED, S)
        whole = expect_bytes(square(rows, S), S * S)
        h = n // 2
        st, err, first = tab(bed_bytes(rows[:h], S, rb), h, rb, S, S * S, S * S)
        assert st == OK and first == expect_bytes(square(rows[:h], S), S * S)
        st, err, both = tab(bed_bytes(rows[h:], S, rb), n - h, rb, S, S * S, S * S, accumulate=1, prefill=first[:36 * S * S])
        assert st == OK and err == NO_ERROR and both == whole, (S, "first differing byte", LC.first_diff(both, whole))
        st, err, zeroed = tab(bed_bytes(rows, S, rb), n, rb, S, S * S, S * S, accumulate=1, prefill=bytes(36 * S * S))
        assert st == OK and zeroed == whole
        st, err, none = tab(b"", 0, rb, S, S * S, S * S, accumulate=1, prefill=whole[:36 * S * S])   # no rows: nothing added
        assert st == OK and none == whole
    check_tables_call(tab, [], 7)   # no rows, stored: zeros


def check_tables_args(tab, workspace_size):
    S, n = 33, 6
    rows = MC.matrix(kin_file(S, n, 0.15), MC.BED)[2]
    rb = MC.row_bytes(MC.BED, S)
    ok = dict(bed=b"".join(rows), n_rows=n, row_stride=rb, S=S, tables_cap=S * S, alloc_tables=S * S)
    assert tab(**ok)[0] == OK
    for bad in (dict(S=0), dict(S=1 << 30), dict(n_override=1 << 32), dict(row_stride=rb - 1), dict(tables_cap=S * S - 1),
                dict(tables_cap=0), dict(ws_short=1), dict(null="tables"), dict(null="ws"), dict(null="err")):
        st, err, buf = tab(**dict(ok, **bad))
        assert st == E_ARG and buf == bytes([FILL]) * len(buf) and err == 0x1111, bad
    assert workspace_size(n + 1000, S) > workspace_size(n, S) > 0


def expect_records(body, rec, S, select):
    """(err word, the square of the rows before the first selected record that is not regular, row_of)."""
    n = len(rec) - 1
    rows, row_of, err, count = [], [], NO_ERROR, 0
    for i in range(n):
        row_of.append(count)
        if select is not None and not select[i]:
            continue
        reg = SC.regular(body, rec[i], rec[i + 1], S)
        if reg is None:
            err = min(err, (i << 8) | 3)
        elif err == NO_ERROR:
            rows.append(MC.row(MC.BED, reg[1]))
        count += 1
    row_of.append(count)
    return err, square(rows, S), row_of


def check_records_call(rec, data, select=None, accumulate=0, prefill=None):
    body, r, S = MC.records_of(data)
    err, sq, row_of = expect_records(body, r, S, select)
    if accumulate:
        sq = sq + np.frombuffer(prefill, dtype=np.uint32).reshape(S, S, 9)
    st, gerr, gbuf, grow_of = rec(body, r, S, select, S * S, S * S, accumulate=accumulate, prefill=prefill)
    what = (S, len(r) - 1, None if select is None else sum(select), accumulate)
    assert st == OK and gerr == err, (what, st, gerr, err)
    assert grow_of == row_of, what
    want = expect_bytes(sq, S * S)
    assert gbuf == want, (what, "first differing byte", LC.first_diff(gbuf, want))
    return err


def check_records_device(rec):
    data, n = kin_file(65, 18, 0.15), 18
    for sel in (None, [1] * n, [int(i % 8 == 0) for i in range(n)], [0] * n):
        assert check_records_call(rec, data, sel) == NO_ERROR
    held = square(MC.matrix(kin_file(65, 9, 0.2), MC.BED)[2], 65).tobytes()
    assert check_records_call(rec, data, [int(i % 3 != 1) for i in range(n)], accumulate=1, prefill=held) == NO_ERROR
    # an irregular record selected: the error word and row_of pinned, the tables those of the rows before it;
    # unselected: not looked at
    for name, data, at in MC.irregular_files():
        n = len(MC.records_of(data)[1]) - 1
        assert check_records_call(rec, data) == (at << 8) | 3, name
        assert check_records_call(rec, data, [int(i != at) for i in range(n)]) == NO_ERROR, name


def check_records_args(rec, workspace_size):
    data = kin_file(33, 6, 0.15)
    body, r, S = MC.records_of(data)
    ok = dict(body=body, rec=r, S=S, select=None, tables_cap=S * S, alloc_tables=S * S)
    assert rec(**ok)[0] == OK
    for bad in (dict(S=0), dict(S=1 << 30), dict(n_override=1 << 32), dict(tables_cap=S * S - 1), dict(ws_short=1),
                dict(null="tables"), dict(null="row_of"), dict(null="ws"), dict(null="err")):
        st, err, buf, row_of = rec(**dict(ok, **bad))
        assert st == E_ARG and buf == bytes([FILL]) * len(buf) and err == 0x1111, bad
