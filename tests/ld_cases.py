"""ld-window restated in Python, and its test inputs.

The feature has no reference action: its oracle is this restatement over the
.bed rows of matrix_cases.py -- the genotype of a 2-bit code, the 3 x 3 table
of a pair of rows, the band of slots in row space, r2 of a table in integer
and float arithmetic, and the text file.  test_ld_emu.py pins it to a
hand-written known answer, to genotype-counts and to its own symmetries,
then holds the kernels and driver to it on the CPU emulator; test_gpu_ld.py
does the same on the GPU.  Every comparison is exact."""
import random

import numpy as np

import decode_cases as D
import matrix_cases as MC
import regions_cases as RC
import subset_cases as SC

OK, E_NOSPACE, E_ARG, E_FORMAT = MC.OK, MC.E_NOSPACE, MC.E_ARG, MC.E_FORMAT
NO_RECORD, NO_ERROR = MC.NO_RECORD, MC.NO_ERROR
FILL, CANARY = MC.FILL, MC.CANARY
TILE_ROWS = 16        # rows i of a block of k_ld_pairs      (the emulator suite holds these three
TILE_PARTNERS = 64    # partners k of a block                  to csrc/vcfc_device.h)
CHUNK_SAMPLES = 512   # samples of a staged row in LDS at a time
TSV_HEAD = b"#CHROM_A\tPOS_A\tID_A\tCHROM_B\tPOS_B\tID_B\tN\tR2\n"
G_OF_CODE = {3: 0, 2: 1, 0: 2, 1: None}   # VCFC_GM_BED code -> genotype


def genotypes(bed_row, S):
    """The S genotypes of a .bed row (None: missing); the pad bits are never looked at."""
    return [G_OF_CODE[(bed_row[s >> 2] >> (2 * (s & 3))) & 3] for s in range(S)]


def table(gi, gj):
    t = [0] * 9
    for a, b in zip(gi, gj):
        if a is not None and b is not None:
            t[3 * a + b] += 1
    return t


def band(bed_rows, S, W):
    """uint32[rows, W, 9]: slot (i, k - 1) = the table of rows (i, i + k), zeros where row i + k does not exist."""
    g = [genotypes(r, S) for r in bed_rows]
    out = np.zeros((len(g), W, 9), dtype=np.uint32)
    for i in range(len(g)):
        for k in range(1, min(W, len(g) - 1 - i) + 1):
            out[i, k - 1] = table(g[i], g[i + k])
    return out


def r2(t):
    """(N, r2 or None where it is undefined): Python integers, then three conversions, two products, one division."""
    t = [int(x) for x in t]
    N = sum(t)
    sx = sum(a * t[3 * a + b] for a in range(3) for b in range(3))
    sy = sum(b * t[3 * a + b] for a in range(3) for b in range(3))
    sxx = sum(a * a * t[3 * a + b] for a in range(3) for b in range(3))
    syy = sum(b * b * t[3 * a + b] for a in range(3) for b in range(3))
    sxy = sum(a * b * t[3 * a + b] for a in range(3) for b in range(3))
    cov, vx, vy = N * sxy - sx * sy, N * sxx - sx * sx, N * syy - sy * sy
    if vx == 0 or vy == 0:
        return N, None
    return N, (float(cov) * float(cov)) / (float(vx) * float(vy))


def r2_text(x):
    return b"nan" if x is None else b"%.6g" % x


def window_ok(W):
    return 0 < W < 1 << 16


def ld(v, W, query=None, table=None):
    """(status, indices, band uint32[rows, W, 9], failing record): the rows are genotype-matrix's."""
    if not window_ok(W):
        return E_ARG, [], np.zeros((0, 0, 9), dtype=np.uint32), NO_RECORD
    st, idx, rows, S, bad = MC.matrix(v, MC.BED, query, table)
    return st, idx, band(rows, S or 1, W), bad


def tsv(v, idx, bnd, W, min_r2):
    """The text of the file entry for rows idx and their band."""
    data_off, S = SC.parse_header(v)
    b = v[data_off:]
    rec, end = SC.hop(b)
    f = [b[rec[i] + 8:].split(b"\t", 3)[:3] for i in idx]
    out = [TSV_HEAD]
    for i in range(len(idx)):
        for k in range(1, W + 1):
            if i + k >= len(idx) or f[i][0] != f[i + k][0]:
                continue
            N, x = r2(bnd[i, k - 1])
            if min_r2 > 0 and not (x is not None and x >= min_r2):
                continue
            out.append(b"\t".join(f[i] + f[i + k] + [b"%d" % N, r2_text(x)]) + b"\n")
    return b"".join(out)


# ---- inputs ---------------------------------------------------------------

# the known answer, written out by hand: 3 rows x 5 samples, sample 3 missing in row 0, W = 2
#   row 0: 0|0 0|1 1|1 ./. 1|0 -> g = 0 1 2 . 1
#   row 1: 1|1 0|0 0|1 1|1 0|0 -> g = 2 0 1 2 0
#   row 2: 0|1 1|0 0|0 1|1 0|0 -> g = 1 1 0 2 0
# (0, 1): samples 0 1 2 4 -> (0,2) (1,0) (2,1) (1,0);  N = 4: Sx 4 Sy 3 Sxx 6 Syy 5 Sxy 2
#         cov = 8 - 12 = -4, vx = 24 - 16 = 8, vy = 20 - 9 = 11: r2 = 16 / 88
# (0, 2): (0,1) (1,1) (2,0) (1,0); N = 4: Sx 4 Sy 2 Sxx 6 Syy 2 Sxy 1
#         cov = 4 - 8 = -4, vx = 8, vy = 8 - 4 = 4: r2 = 16 / 32
# (1, 2): all five -> (2,1) (0,1) (1,0) (2,2) (0,0); N = 5: Sx 5 Sy 4 Sxx 9 Syy 6 Sxy 6
#         cov = 30 - 20 = 10, vx = 45 - 25 = 20, vy = 30 - 16 = 14: r2 = 100 / 280
KAT_TOKENS = [[b"0|0", b"0|1", b"1|1", b"./.", b"1|0"], [b"1|1", b"0|0", b"0|1", b"1|1", b"0|0"],
              [b"0|1", b"1|0", b"0|0", b"1|1", b"0|0"]]
KAT_W = 2
KAT_BAND = [[[0, 0, 1, 2, 0, 0, 0, 1, 0], [0, 1, 0, 1, 1, 0, 1, 0, 0]],
            [[1, 1, 0, 1, 0, 0, 0, 1, 1], [0] * 9],
            [[0] * 9, [0] * 9]]
KAT_N = [[4, 4], [5, 0], [0, 0]]
KAT_R2 = [[b"0.181818", b"0.5"], [b"0.357143", b"nan"], [b"nan", b"nan"]]
KAT_TSV = (TSV_HEAD + b"1\t100\trs0\t1\t101\trs1\t4\t0.181818\n" + b"1\t100\trs0\t1\t102\trs2\t4\t0.5\n" +
           b"1\t101\trs1\t1\t102\trs2\t5\t0.357143\n")


def kat_file():
    lines = [b"1\t%d\trs%d\tA\tG\t1\tPASS\t.\tGT\t" % (100 + i, i) + b"\t".join(t) for i, t in enumerate(KAT_TOKENS)]
    return D.encode_file(5, lines)


MISSING = [b"./.", b"./.", b".|.", b"2|0", b"1", b"0|2"]   # all missing in .bed: no call, multi-allelic, haploid


def lines_of(rnd, n, S, miss, chrom=lambda i: b"22", last=None):
    """n data lines of S tokens: a row's alternate-allele frequency is drawn from a few values (0 and 1 give rows
    without variance), a token is missing at rate `miss` (every 5th row: 4 x miss, every 7th: none); `last`: the
    last sample's token in every row."""
    out = []
    for i in range(n):
        p = rnd.choice([0.0, 0.05, 0.3, 0.5, 0.5, 0.8, 1.0])
        m = 0.0 if i % 7 == 6 else min(0.95, 4 * miss) if i % 5 == 4 else miss
        toks = []
        for s in range(S):
            if rnd.random() < m:
                toks.append(rnd.choice(MISSING))
            else:
                a, b = rnd.random() < p, rnd.random() < p
                toks.append((b"%d/%d" if rnd.random() < 0.05 else b"%d|%d") % (a, b))
        if last is not None:
            toks[-1] = last
        out.append(chrom(i) + b"\t%d\trs%d\tA\tG\t50\tPASS\t.\tGT\t" % (100 + 3 * i, i) + b"\t".join(toks))
    return out


_files = {}


def ld_file(S, n, miss=0.2, seed=0, last=None, chroms=None):
    """A seeded file of n rows (cached: the tests share them)."""
    key = (S, n, miss, seed, last, chroms)
    if key not in _files:
        rnd = random.Random(7919 * seed + 31 * S + n)
        chrom = (lambda i: chroms[i * len(chroms) // max(n, 1)]) if chroms else (lambda i: b"22")
        _files[key] = D.encode_file(S, lines_of(rnd, n, S, miss, chrom, last))
    return _files[key]


SIZES = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 600, 2504)


def size_files(lds_bed):
    """(name, bytes, W): the sample counts around a byte, a plane word, a
    16-byte plane stride and the staged chunk, one above the matrix kernel's LDS
    tile (a handful of rows), and for S mod 4 != 0 files whose last real sample
    is 1|1 in every row (code 00, as the pad bits)."""
    out = [("S%d" % S, ld_file(S, 7 if S < 600 else 5, 0.25 if S < 8 else 0.1), 3) for S in SIZES]
    out += [("S%d" % S, ld_file(S, 5, 0.1), 2) for S in (CHUNK_SAMPLES - 1, CHUNK_SAMPLES, CHUNK_SAMPLES + 1)]
    out.append(("S%d" % (lds_bed + 1), ld_file(lds_bed + 1, 4, 0.05), 2))
    out += [("S%d_last11" % S, ld_file(S, 6, 0.1, last=b"1|1"), 3) for S in (1, 3, 5, 17, 30, 63, 65, 130, 513)]
    return out


def shape_cases():
    """(rows, W): rows 0, 1, 2, W - 1, W, W + 1 and both sides of the row tile; W 1, 2, 63, 64, 65, rows - 1, rows,
    rows + 5."""
    T = TILE_ROWS
    out = set()
    for rows in (0, 1, 2, T - 1, T, T + 1, 2 * T + 1):
        for W in (1, 2, rows - 1, rows, rows + 5):
            if W >= 1:
                out.add((rows, W))
    for W in (TILE_PARTNERS - 1, TILE_PARTNERS, TILE_PARTNERS + 1):
        for rows in (W - 1, W, W + 1):
            out.add((rows, W))
    out |= {(2 * TILE_PARTNERS + 9, TILE_PARTNERS + 1), (5, 2 * TILE_PARTNERS + 3)}
    return sorted(out)


REGION_TEXTS = MC.REGION_TEXTS
QUERIES = MC.QUERIES


# ---- checks shared by the emulator and the GPU suites ----------------------
# run(data, W, query=None, regions=None, band_bound=0, min_r2=None) ->
#     (status, indices, band uint32[rows, W, 9], failing record, text of the file entry or None);
#     min_r2 None: the text is not asked for (a runner may still give it, for min_r2 = 0)

def same(got, want, what):
    assert got[0] == want[0], (what, "status", got[0], want[0])
    assert got[3] == want[3], (what, "failing record", got[3], want[3])
    assert list(got[1]) == list(want[1]), (what, "indices")
    if want[0] not in (OK, E_FORMAT):
        return
    assert got[2].shape == want[2].shape, (what, "band", got[2].shape, want[2].shape)
    bad = np.argwhere(got[2] != want[2])
    assert len(bad) == 0, (what, "first differing cell (row, k - 1, cell)", bad[0].tolist(), len(bad))


def check_file(run, name, data, W, query=None, regions=None, band_bound=0, min_r2=None):
    want = ld(data, W, query, RC.parse_text(regions) if regions is not None else None)
    got = run(data, W, query, regions, band_bound, min_r2)
    same(got, want, (name, W, query, band_bound))
    if want[0] in (OK, E_FORMAT) and SC.parse_header(data) and got[4] is not None:
        assert got[4] == tsv(data, want[1], want[2], W, min_r2 or 0.0), (name, W, min_r2)
    return want


def seen(bands):
    """What the seeded tables must cover, over all the bands of a test: a table with every cell non-zero, one
    with N == 0 between two rows that exist, one with vx == 0 and N > 0."""
    full = empty = flat = 0
    for b, rows in bands:
        for i in range(rows):
            for k in range(1, min(b.shape[1], rows - 1 - i) + 1):
                t = b[i, k - 1]
                N = int(t.sum())
                full += bool(t.all())
                empty += N == 0
                flat += N > 0 and N * int(t[3:6].sum() + 4 * t[6:9].sum()) == int(t[3:6].sum() + 2 * t[6:9].sum()) ** 2
    return full, empty, flat


def check_sizes(run, lds_bed):
    bands = []
    for name, data, W in size_files(lds_bed):
        want = check_file(run, name, data, W)
        assert want[0] == OK and len(want[1]) >= 4, name
        bands.append((want[2], len(want[1])))
    full, empty, flat = seen(bands)
    assert full >= 5 and empty >= 5 and flat >= 5, (full, empty, flat)


def check_shapes(run):
    for rows, W in shape_cases():
        if rows == 0:   # (a .vcfc without records is no .vcfc: a query that matches none of five)
            want = check_file(run, "rows0", ld_file(33, 5, 0.15), W, (b"21", False, 0, 0))
        else:
            want = check_file(run, "rows%d" % rows, ld_file(33, rows, 0.15), W)
        assert want[0] == OK and want[2].shape == (rows, W, 9)


def check_batches(run):
    """Band bounds that give 1, 2, W - 1, W and W + 1 owned rows a batch: the halo of W rows carries the pairs
    across every batch end."""
    W, data = 5, ld_file(17, 23, 0.2)
    for own in (1, 2, W - 1, W, W + 1):
        check_file(run, "own%d" % own, data, W, band_bound=36 * W * own)
    name, data = SC.query_files(1)[0]
    for own in (1, 3):
        for q in QUERIES[:3]:
            check_file(run, name, data, 4, q, band_bound=36 * 4 * own)


def check_queries(run, seed=1):
    stopped = unstopped = 0
    for name, data in SC.query_files(seed):
        for q in (QUERIES if name == "valid" else QUERIES[:3] + QUERIES[5:6]):
            want = check_file(run, name, data, 3, q)
            if q is not None and name.startswith(("no_lf", "nul_req")):
                stopped += want[0] == E_FORMAT
                unstopped += want[0] == OK
    assert stopped >= 5 and unstopped >= 5, (stopped, unstopped)


def check_regions(run, seed=1):
    hits = 0
    for text in REGION_TEXTS:
        for name, data in SC.query_files(seed)[:6]:
            want = check_file(run, name, data, 3, regions=text)
            hits += len(want[1]) > 0
    assert hits >= 6


def check_mutated(run, seed):
    """The stop rules: every mutated file, also in batches that put the failing record into a halo."""
    ok = partial = 0
    for name, data in D.mutated_files(seed):
        want = check_file(run, name, data, 3)
        check_file(run, name, data, 2, band_bound=36 * 2 * 2)
        ok += want[0] == OK
        partial += want[0] == E_FORMAT and len(want[1]) > 0
    assert ok >= 5 and partial >= 5, (ok, partial)


def check_irregular(run):
    for name, data, at in MC.irregular_files():
        for bound in (0, 36 * 2, 36 * 2 * 2):
            want = check_file(run, name, data, 2, band_bound=bound)
            assert (want[0], want[3], len(want[1])) == (E_FORMAT, at, at), name


def two_chrom_file():
    """12 rows of 40 samples, CHROM 1 then 2; the first row of CHROM 1 with two called genotypes is repeated in the
    row behind it (r2 == 1)."""
    if "two_chroms" not in _files:
        lines = lines_of(random.Random(2 * 7919), 12, 40, 0.1, lambda i: b"1" if i < 6 else b"2")
        toks = [l.split(b"\t", 9)[9] for l in lines]
        i = next(i for i in range(5) if len({MC.token_codes(t)[3] for t in toks[i].split(b"\t")} - {1}) >= 2)
        lines[i + 1] = b"\t".join(lines[i + 1].split(b"\t", 9)[:9] + [toks[i]])
        _files["two_chroms"] = D.encode_file(40, lines)
    return _files["two_chroms"]


def check_tsv(run):
    """Two CHROMs in one file (pairs across the boundary are dropped); min_r2 0, equal to a pair's r2 (kept) and 1;
    undefined pairs."""
    data, W = two_chrom_file(), 4
    st, idx, bnd, bad = ld(data, W)
    assert st == OK and len(idx) == 12
    vals = [r2(bnd[i, k - 1])[1] for i in range(12) for k in range(1, W + 1) if i + k < 12 and (i < 6) == (i + k < 6)]
    defined = sorted(x for x in vals if x is not None)
    assert len(defined) >= 8 and None in vals, "the file holds defined and undefined pairs"
    pick = defined[len(defined) // 2]
    assert 0 < pick < 1
    lines = {}
    for m in (0.0, -1.0, pick, 1.0):
        check_file(run, "two_chroms", data, W, min_r2=m)
        lines[m] = tsv(data, idx, bnd, W, m).split(b"\n")[1:-1]
    assert len(lines[0.0]) == len(vals) < sum(1 for i in range(12) for k in range(1, W + 1) if i + k < 12)
    assert lines[-1.0] == lines[0.0] and any(l.endswith(b"\tnan") for l in lines[0.0])
    assert sum(1 for l in lines[pick] if l.endswith(b"\t" + r2_text(pick))) >= 1, "the pair at the threshold is kept"
    assert len(lines[pick]) == sum(1 for x in defined if x >= pick) and not any(l.endswith(b"nan") for l in lines[pick])
    assert len(lines[1.0]) == sum(1 for x in defined if x >= 1.0) >= 1
    check_file(run, "kat", kat_file(), KAT_W, min_r2=0.0)
    name, data = next(x for x in SC.query_files(1) if x[0] == "no_lf17")   # stops at record 17: the pairs among 17 rows
    want = check_file(run, name, data, 3, min_r2=0.0)
    assert (want[0], want[3], len(want[1])) == (E_FORMAT, 17, 17)


# ---- the two device entries ---------------------------------------------------
# tab(bed bytes, n_rows, row_stride, S, W, pairs_cap, alloc_slots, offset=0, ws_short=0, null=None, n_override=None)
#     -> (status, err word, the 36 * alloc_slots + CANARY bytes of the band's allocation, which held FILL);
#     byte `offset` (0..15) of an allocation is d_bed
# win(body, rec, S, W, select, pairs_cap, alloc_slots, ws_short=0, null=None, n_override=None)
#     -> (status, err word, the allocation's bytes, row_of as a list of n + 1)

def expect_band_bytes(bnd, rows, W, pairs_cap, alloc_slots):
    """The allocation after a call: the rows whose W slots all fit pairs_cap, FILL elsewhere."""
    buf = bytearray([FILL]) * (36 * alloc_slots + CANARY)
    fit = min(rows, pairs_cap // W)
    buf[:36 * W * fit] = bnd[:fit].tobytes()
    return bytes(buf), fit


def first_diff(a, b, mask=None):
    return next((k for k in range(len(b)) if (mask is None or mask[k]) and a[k] != b[k]), None)


def check_tables_call(tab, rows_bytes, S, W, stride_of=lambda rb: rb, offset=0, cut=None):
    rb = MC.row_bytes(MC.BED, S)
    n, stride = len(rows_bytes), stride_of(rb)
    bed = bytearray([0x5A]) * (n * stride + 1)   # (0x5A: codes 10 10 01 01 between and behind the rows)
    for r, row in enumerate(rows_bytes):
        bed[r * stride:r * stride + rb] = row
    slots = n * W
    cap = slots if cut is None else max(0, slots - cut) if cut >= 0 else 0
    want, fit = expect_band_bytes(band(rows_bytes, S, W), n, W, cap, max(slots, 1))
    st, err, got = tab(bytes(bed), n, stride, S, W, cap, max(slots, 1), offset=offset)
    what = (S, n, W, stride, offset, cap)
    assert st == OK and err == (NO_ERROR if fit == n else (fit << 8) | 0xFF), (what, st, err)
    assert len(got) == len(want) and got == want, (what, "first differing byte", first_diff(got, want), "canary from", 36 * cap)


def check_tables_device(tab):
    for S, n, W in ((65, 18, 3), (5, 9, 2), (33, 17, 20), (130, 6, 1)):
        rows = MC.matrix(ld_file(S, n, 0.15, last=b"1|1"), MC.BED)[2]
        assert len(rows) == n
        for stride_of in (lambda rb: rb, lambda rb: (rb + 15) & ~15, lambda rb: rb + 1):
            check_tables_call(tab, rows, S, W, stride_of)
        for offset in range(16):
            check_tables_call(tab, rows, S, W, lambda rb: rb + 1, offset=offset)
        check_tables_call(tab, rows, S, W, cut=1)      # pairs_cap one short: the last row's slots stay unwritten
        check_tables_call(tab, rows, S, W, cut=-1)     # pairs_cap 0
    check_tables_call(tab, [], 7, 3)


def check_tables_args(tab, workspace_size):
    S, n, W = 33, 6, 2
    rows = MC.matrix(ld_file(S, n, 0.15), MC.BED)[2]
    rb = MC.row_bytes(MC.BED, S)
    ok = dict(bed=b"".join(rows), n_rows=n, row_stride=rb, S=S, W=W, pairs_cap=n * W, alloc_slots=n * W)
    assert tab(**ok)[0] == OK
    for bad in (dict(W=0), dict(W=1 << 16), dict(S=0), dict(S=1 << 30), dict(n_override=1 << 32), dict(row_stride=rb - 1),
                dict(ws_short=1), dict(null="tables"), dict(null="ws"), dict(null="err")):
        st, err, buf = tab(**dict(ok, **bad))
        assert st == E_ARG and buf == bytes([FILL]) * len(buf), bad
    assert workspace_size(n, S, W) > 0


def expect_window(body, rec, S, W, select, pairs_cap, alloc_slots):
    """(err word, expected bytes, mask of the bytes that are compared, row_of)."""
    n = len(rec) - 1
    rows, row_of, err, bad_row = [], [], NO_ERROR, None
    for i in range(n):
        row_of.append(len(rows))
        if select is not None and not select[i]:
            continue
        reg = SC.regular(body, rec[i], rec[i + 1], S)
        if reg is None:
            err = min(err, (i << 8) | 3)
            bad_row = len(rows) if bad_row is None else bad_row
        rows.append(MC.row(MC.BED, reg[1]) if reg is not None else bytes(MC.row_bytes(MC.BED, S)))
        if len(rows) * W > pairs_cap:
            err = min(err, (i << 8) | 0xFF)
    row_of.append(len(rows))
    bnd = band(rows, S, W)
    buf, fit = expect_band_bytes(bnd, len(rows), W, pairs_cap, alloc_slots)
    mask = bytearray([1]) * len(buf)
    if bad_row is not None:   # tables that touch rows >= bad_row are not meaningful
        for i in range(fit):
            for k in range(1, W + 1):
                if i + k < len(rows) and i + k >= bad_row:
                    p = 36 * (i * W + k - 1)
                    mask[p:p + 36] = bytes(36)
    return err, buf, bytes(mask), row_of


def check_window_call(win, data, W, select=None, cut=None):
    body, rec, S = MC.records_of(data)
    n = len(rec) - 1
    rows = n if select is None else sum(1 for x in select if x)
    slots = rows * W
    cap = slots if cut is None else max(0, slots - cut) if cut >= 0 else 0
    err, buf, mask, row_of = expect_window(body, rec, S, W, select, cap, max(slots, 1))
    st, gerr, gbuf, grow_of = win(body, rec, S, W, select, cap, max(slots, 1))
    what = (S, n, W, cap, None if select is None else sum(select))
    assert st == OK and gerr == err, (what, st, gerr, err)
    assert grow_of == row_of, what
    assert len(gbuf) == len(buf) and first_diff(gbuf, buf, mask) is None, (what, "first differing byte", first_diff(gbuf, buf, mask))
    return err


def check_window_device(win):
    data = ld_file(65, 18, 0.15)
    n = 18
    for W in (1, 3, 20):
        for sel in (None, [1] * n, [int(i % 8 == 0) for i in range(n)]):
            assert check_window_call(win, data, W, sel) == NO_ERROR
        assert check_window_call(win, data, W, cut=1) == ((n - 1) << 8) | 0xFF
        assert check_window_call(win, data, W, cut=-1) == 0xFF
    sel = [int(i % 3 != 1) for i in range(n)]
    assert check_window_call(win, data, 2, sel, cut=3) == (15 << 8) | 0xFF   # 12 rows, 21 slots: row 10 (record 15) is the first that does not fit
    # an irregular record selected: the error word, the tables of the rows before it exact; unselected: not looked at
    for name, data, at in MC.irregular_files():
        n = len(MC.records_of(data)[1]) - 1
        assert check_window_call(win, data, 2) == (at << 8) | 3, name
        assert check_window_call(win, data, 2, [int(i != at) for i in range(n)]) == NO_ERROR, name


def check_window_args(win, workspace_size):
    data = ld_file(33, 6, 0.15)
    body, rec, S = MC.records_of(data)
    n = len(rec) - 1
    ok = dict(body=body, rec=rec, S=S, W=2, select=None, pairs_cap=2 * n, alloc_slots=2 * n)
    assert win(**ok)[0] == OK
    for bad in (dict(W=0), dict(W=1 << 16), dict(S=0), dict(S=1 << 30), dict(n_override=1 << 32), dict(ws_short=1),
                dict(null="tables"), dict(null="row_of"), dict(null="ws"), dict(null="err")):
        st, err, buf, row_of = win(**dict(ok, **bad))
        assert st == E_ARG and buf == bytes([FILL]) * len(buf), bad
    assert workspace_size(n, S, 2) >= workspace_size(n, S, 1) > 0
