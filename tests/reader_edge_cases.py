"""The four compressed-domain readers -- the sample subset,
genotype-counts (§4j), genotype-matrix (§4l) and extract (§4m) -- at the edges
of their grids and of the stager they share, against the restatements
(subset_cases, counts_cases, matrix_cases, extract_cases).  Inputs and check_*
functions that take a runner; test_{subset,counts,matrix,extract}_emu.py call
them on the CPU emulator, test_gpu_{subset,counts,matrix,extract}.py on the
GPU.  Every comparison is exact.  Three families:

second_trip   k_cnt_scan and k_gm_scan launch only as many blocks as stay
              resident, and every wave loops over chunks of 16 records with
              the grid's stride.  The inputs here are longer than one trip of
              that loop (the trip comes from the library:
              vcfc_counts_trip_records / vcfc_matrix_trip_records), by three
              chunks and a partial one, so the stride step, the partial last
              chunk of a later trip, `counted` and the LDS histogram carried
              over trips and the zero rows of unselected records in a later
              trip are all run.  The same for the byte-serial kernels'
              fixed lanes (GPU only: 262 144 of them).
queue_pass    k_sub_wseq, k_ex_seq and k_ex_wseq run a fixed number of lanes
              over the queue of byte-serial records; each lane owns one slice
              of the scratch array and uses it again for its next record.
              A file whose queue is longer than the lanes.
stager_edges  decode_cases.edge_files() -- REQ lengths around a copy step and a
              staged piece at every record alignment, NULs and a tenth TAB
              behind the first step, escape flag bytes last in a window and in
              a staged piece, S = 40 000, late records that are not simple --
              through all four readers.

What no test here can tell: the readers ask the stager for each window with
need(cur, 256 + 8), the 8 for an escape's payload past the window.
Staged::load stages 8 bytes of look-ahead behind every piece whatever was
asked for, and a window accepted as resident ends at or before the piece's
end, so need(cur, 256) reads the same bytes: the + 8 only moves a reload one
window earlier."""
import functools
import random

import numpy as np

import counts_cases as CC
import decode_cases as D
import extract_cases as EC
import matrix_cases as MC
import subset_cases as SC

OK, E_FORMAT = 0, 8
NO_ERROR = (1 << 64) - 1
rec, req_of, fill = D.rec, D.req_of, D.fill

# ---- second_trip ------------------------------------------------------------

PERIOD = 61            # records of the tiled period: prime, so every record meets every chunk position and lane
TAIL = 3 * 16 + 5      # records past one trip: three whole chunks and a partial one
MAX_INPUT = 64 << 20   # a device with many more CUs fails loudly here
SERIAL_LANES = 1024 * 256   # lanes k_cnt_seq and k_gm_seq stride over (vcfc_counts.hip, vcfc_matrix.hip)
KINDS = 11
SERIAL_KINDS = (8, 9, 10)


def spots(S, L=None):
    """The columns the differing item of a period's records stands at; with
    the LDS limit L given, columns on both sides of it."""
    if S <= 8:
        return list(range(S))
    out = [0, 1, 255, 256, S - 3, S - 2, S - 1]
    return out if L is None else out + [L - 2, L - 1, L]


def items(kind, c, S):
    """The sample section of one record: kind 0..10, its differing item at column c."""
    rest = S - 1 - c
    esc = lambda t: b"\xe1" + t + (b"\t" if rest else b"")
    if kind == 0:    # one 0|1 among 0|0 runs
        return fill(c) + b"\xa1" + fill(rest)
    if kind == 1:    # one 1|0 among 1|1 runs
        return fill(c, 0x80) + b"\xc1" + fill(rest, 0x80)
    if kind == 2:    # one 1|1 among 0|1 runs
        return fill(c, 0xA0) + b"\x81" + fill(rest, 0xA0)
    if kind == 3:    # one 0|0 among 1|0 runs
        return fill(c, 0xC0) + b"\x01" + fill(rest, 0xC0)
    if kind == 4:    # a one-token escape that spells a class
        return fill(c) + esc(b"0|1") + fill(rest, 0x80)
    if kind == 5:    # ... of another token
        return fill(c, 0xC0) + esc(b"2|1") + fill(rest)
    if kind == 6:
        return fill(c) + esc(b"./.") + fill(rest, 0xA0)
    if kind == 7:    # a run that ends at S
        return fill(c) + fill(S - c, 0xA0)
    # the byte-serial path's records
    if kind == 8:    # a two-token escape
        c = min(c, S - 2)
        return fill(c) + b"\xe22|1\t0|2" + (b"\t" if S - 2 - c else b"") + fill(S - 2 - c, 0xC0)
    if kind == 9:    # a long last token, ended by the LF
        return fill(c) + fill(rest, 0xA0) + b"\xe10|1:35:99"
    return fill(c) + b"\x00" + fill(S - c, 0x80)   # a zero-count item


def period(S, L=None, kinds=tuple(range(KINDS))):
    """The 61 records of the period and their tokens."""
    sp = spots(S, L)
    recs = [rec(req_of(k), items(kinds[k % len(kinds)], sp[k % len(sp)], S)) for k in range(PERIOD)]
    toks = [SC.regular(r, 0, len(r), S) for r in recs]
    assert all(t is not None for t in toks) and len(set(recs)) == PERIOD
    assert sum(kinds[k % len(kinds)] in SERIAL_KINDS for k in range(PERIOD)) >= 4
    return recs, [t[1] for t in toks]


class Tiled:
    """n records: the period repeated.  body, rec (n + 1 offsets, uint64),
    and per period record its counts row, its class per sample and its tokens."""

    def __init__(self, S, n, L=None, kinds=tuple(range(KINDS))):
        recs, toks = period(S, L, kinds)
        reps, rem = divmod(n, PERIOD)
        self.S, self.n, self.toks = S, n, toks
        self.body = bytearray(b"".join(recs) * reps + b"".join(recs[:rem]))
        lens = np.tile(np.array([len(r) for r in recs], dtype=np.uint64), reps + 1)[:n]
        self.rec = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(lens, dtype=np.uint64)])
        assert int(self.rec[n]) == len(self.body) < MAX_INPUT, len(self.body)
        self.rows = np.array([CC.row(t) for t in toks], dtype=np.uint32)
        self.cls = np.array([[CC.CLASS.get(x, 4) for x in t] for t in toks], dtype=np.int64)   # [61][S]

    def want_rows(self, on):
        out = self.rows[np.arange(self.n) % PERIOD]
        out[~on] = 0
        return out

    def want_table(self, on, calls=1):
        """The per-period table times the records of each residue that are on."""
        per = np.bincount(np.arange(self.n)[on] % PERIOD, minlength=PERIOD)
        tab = np.zeros((self.S, 5), dtype=np.uint64)
        for k in range(5):
            tab[:, k] = (per[:, None] * (self.cls == k)).sum(axis=0)
        assert int(tab.sum()) == int(on.sum()) * self.S
        return tab * np.uint64(calls)

    def break_lf(self, i):
        self.body[int(self.rec[i + 1]) - 1] = ord("x")


def trip_n(trip):
    n = trip + TAIL
    assert trip > 0 and trip % 16 == 0 and n > trip and (n - trip) % 16 != 0, trip
    return n


def select_of(n):
    return np.array([int(i % 3 == 0) for i in range(n)], dtype=np.uint8)


def on_of(n, select):
    return np.ones(n, dtype=bool) if select is None else select.astype(bool)


# counts.  dev(body, rec, S, select, variant, sample, calls) -> (status, err word, rows array or None, table array
# or None); body bytes, rec an array of n + 1 offsets, select an array or None; it checks its canaries itself.

def check_counts_trip(dev, trip_records, S, variant, sample, L=None, kinds=tuple(range(KINDS)), n=None):
    """Rows and / or table of a call longer than one trip: every record, every
    third record, and twice (the table doubles, the rows stay)."""
    n = trip_n(trip_records(S, sample)) if n is None else n
    T = Tiled(S, n, L, kinds)
    body = bytes(T.body)
    for select, calls in ((None, 1), (select_of(n), 1)) + (((None, 2),) if sample else ()):
        on = on_of(n, select)
        st, err, rows, tab = dev(body, T.rec, S, select, variant, sample, calls)
        what = (S, n, select is not None, calls)
        assert (st, err) == (OK, NO_ERROR), (what, st, hex(err))
        if variant:
            want = T.want_rows(on)
            bad = np.flatnonzero((rows != want).any(axis=1))
            assert bad.size == 0, (what, "rows", bad[:8].tolist(), rows[bad[0]].tolist(), want[bad[0]].tolist())
        if sample:
            want = T.want_table(on, calls)
            bad = np.flatnonzero((tab != want).any(axis=1))
            assert bad.size == 0, (what, "sample table", bad[:8].tolist(), tab[bad[0]].tolist(), want[bad[0]].tolist())
    return n


def check_counts_trip_irregular(dev, trip_records, S=5):
    """A record that is not regular in each trip: the err word is the smaller
    index, every other row exact; both unselected, nothing is reported."""
    trip = trip_records(S, True)
    n = trip_n(trip)
    T = Tiled(S, n)
    first, second = 21, trip + 7
    T.break_lf(first)
    T.break_lf(second)
    body = bytes(T.body)
    assert SC.regular(body, int(T.rec[second]), int(T.rec[second + 1]), S) is None
    keep = np.ones(n, dtype=bool)
    keep[[first, second]] = False
    st, err, rows, tab = dev(body, T.rec, S, None, True, True, 1)
    assert (st, err) == (OK, (first << 8) | 3), (st, hex(err))
    assert (rows[keep] == T.want_rows(keep)[keep]).all()
    select = keep.astype(np.uint8)
    st, err, rows, tab = dev(body, T.rec, S, select, True, True, 1)
    assert (st, err) == (OK, NO_ERROR), (st, hex(err))
    assert (rows == T.want_rows(keep)).all() and (tab == T.want_table(keep)).all()
    select[second] = 1   # only the later trip's: its index, and the first trip's an unselected record's zero row
    st, err, rows, tab = dev(body, T.rec, S, select, True, False, 1)
    assert (st, err) == (OK, (second << 8) | 3), (st, hex(err))
    keep[first] = True
    assert (rows[keep] == T.want_rows(select.astype(bool))[keep]).all() and not rows[first].any()


# the matrix.  dev: matrix_cases' device runner (body, rec list, S, layout, select, row_stride, out_cap, alloc) ->
# (status, err word, the alloc + CANARY bytes of the allocation, row_of)

def matrix_want(T, layout, on, stride, skip=()):
    """(expected allocation, mask of the bytes compared, row_of)."""
    rb = MC.row_bytes(layout, T.S)
    rows61 = np.array([np.frombuffer(MC.row(layout, t), dtype=np.uint8) for t in T.toks])
    idx = np.flatnonzero(on)
    m = len(idx)
    buf = np.full((m, stride), MC.FILL, dtype=np.uint8)
    buf[:, :rb] = rows61[idx % PERIOD]
    mask = np.ones((m, stride), dtype=bool)
    for i in skip:   # a record that is not regular: its own row is not compared
        mask[np.searchsorted(idx, i), :rb] = False
    alloc = (m - 1) * stride + rb
    tail = np.full(MC.CANARY, MC.FILL, dtype=np.uint8)
    row_of = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(on, dtype=np.int64)])
    return (np.concatenate([buf.reshape(-1)[:alloc], tail]),
            np.concatenate([mask.reshape(-1)[:alloc], np.ones(MC.CANARY, dtype=bool)]), row_of.tolist(), alloc)


def matrix_call(dev, T, layout, select, extra, want_err=NO_ERROR, skip=()):
    rb = MC.row_bytes(layout, T.S)
    on = on_of(T.n, select)
    want, mask, row_of, alloc = matrix_want(T, layout, on, rb + extra, skip)
    st, err, got, grow_of = dev(bytes(T.body), T.rec.tolist(), T.S, layout, None if select is None else select.tolist(),
                                rb + extra, alloc, alloc)
    what = (layout, T.S, T.n, select is not None, extra)
    assert (st, err) == (OK, want_err), (what, st, hex(err))
    assert grow_of == row_of, (what, "row_of")   # the exclusive scan of the flags
    g = np.frombuffer(got, dtype=np.uint8)
    bad = np.flatnonzero((g != want) & mask)
    assert g.size == want.size and bad.size == 0, (what, "first differing byte", bad[:1].tolist(), "row",
                                                   int(bad[0]) // (rb + extra), "canary from", alloc)


def check_matrix_trip(dev, trip_records, layout, S=5):
    """S = 5: .bed pad bits and an odd row length, so with row_stride =
    row_bytes the rows land on every 16-byte phase; unselected rows' bytes
    keep their fill; once with row_stride = row_bytes + 3."""
    n = trip_n(trip_records(layout))
    T = Tiled(S, n)
    matrix_call(dev, T, layout, None, 0)
    matrix_call(dev, T, layout, select_of(n), 0)
    matrix_call(dev, T, layout, None, 3)
    return n


def check_matrix_trip_irregular(dev, trip_records, layout=MC.DOSAGE, S=5):
    trip = trip_records(layout)
    n = trip_n(trip)
    T = Tiled(S, n)
    first, second = 21, trip + 7
    T.break_lf(first)
    T.break_lf(second)
    matrix_call(dev, T, layout, None, 0, (first << 8) | 3, skip=(first, second))
    select = np.ones(n, dtype=np.uint8)
    select[[first, second]] = 0
    matrix_call(dev, T, layout, select, 1)
    select[first] = 1
    matrix_call(dev, T, layout, select, 0, (first << 8) | 3, skip=(first,))
    select[[first, second]] = 0, 1
    matrix_call(dev, T, layout, select, 0, (second << 8) | 3, skip=(second,))


def serial_tiled(S=4):
    """More records than the byte-serial kernels have lanes, every one of
    them byte-serial."""
    n = SERIAL_LANES + 100
    return Tiled(S, n, kinds=SERIAL_KINDS)


def check_counts_serial_trip(dev):
    T = serial_tiled()
    on = on_of(T.n, None)
    st, err, rows, tab = dev(bytes(T.body), T.rec, T.S, None, True, True, 1)
    assert (st, err) == (OK, NO_ERROR), (st, hex(err))
    assert (rows == T.want_rows(on)).all() and (tab == T.want_table(on)).all()


def check_matrix_serial_trip(dev):
    matrix_call(dev, serial_tiled(), MC.DOSAGE, None, 0)


# ---- queue_pass -------------------------------------------------------------

QUEUE_S, QUEUE_N = 6, 2100
QUEUE_COLS = [[0], [5, 0, 2], list(range(QUEUE_S)), [1, 0]]
QUEUE_KINDS = [fill(2) + b"\xa1" + fill(3, 0x80),                      # simple
               fill(1) + b"\xe12|1\t" + fill(4, 0xC0),                 # simple, an other-token escape
               fill(2) + b"\xe22|1\t0|2\t" + fill(2, 0x80),            # a two-token escape
               b"\x01\xe31\t0\t.\t" + fill(2, 0xA0),                   # a three-token escape, one-byte tokens
               fill(5, 0xC0) + b"\xe10|1:35:99",                       # a long last token, ended by the LF
               fill(3) + b"\xe10|1:5\t" + fill(2, 0x80),               # a 5-byte token in mid-record
               b"\x00" + fill(6, 0xA0)]                                # a leading zero-count byte
QUEUE_SERIAL = 5   # of the seven


@functools.lru_cache(maxsize=None)
def queue_file():
    return D.header(QUEUE_S) + b"".join(rec(req_of(i), QUEUE_KINDS[i % 7]) for i in range(QUEUE_N))


def seq_lanes(workspace_size, words):
    """Lanes of the byte-serial writer, from the scratch array's share of the
    workspace: `words` 32-bit words a chosen column and lane (the two column
    arrays grow by 256 bytes each from K = 64 to 128)."""
    grow = workspace_size(1, 128) - workspace_size(1, 64) - 2 * 256
    assert grow > 0 and grow % (4 * words * 64) == 0, grow
    return grow // (4 * words * 64)


def queue_select():
    return [int(i % 3 != 1) for i in range(QUEUE_N)]


def check_queue_is_longer_than_the_lanes(workspace_size, words):
    lanes = seq_lanes(workspace_size, words)
    assert lanes >= 64 and QUEUE_N // 7 * QUEUE_SERIAL > lanes, lanes   # every lane takes a second record
    return lanes


def check_queue_subset(decs, dev, col_sets=QUEUE_COLS):
    """decs: buffer runners (data, cols) -> (status, bytes), one per output
    batch size; dev(data, cols, select) -> (status, err word, offsets, out
    bytes whose unwritten bytes hold 0xEE)."""
    data = queue_file()
    h, S = SC.parse_header(data)
    body = data[h:]
    starts, end = SC.hop(body)
    assert len(starts) == QUEUE_N
    for cols in col_sets:
        want = SC.subset(data, cols)
        assert want[0] == OK
        for dec in decs:
            got = dec(data, cols)
            assert got[0] == OK and got[1] == want[1], (cols, got[0], len(got[1]), len(want[1]))
        lines = [SC.line(*SC.regular(body, starts[i], (starts + [end])[i + 1], S), cols) for i in range(QUEUE_N)]
        for sel in (None, queue_select()):
            kept = [l if sel is None or sel[i] else b"" for i, l in enumerate(lines)]
            off = np.concatenate([[0], np.cumsum([len(l) for l in kept])]).tolist()
            st, err, loff, out = dev(data, cols, sel)
            assert (st, err) == (OK, NO_ERROR), (cols, sel is not None, st, hex(err))
            assert loff == off, (cols, sel is not None, "offsets")
            assert out[:off[-1]] == b"".join(kept), (cols, sel is not None, "bytes")
            assert out[off[-1]:].count(0xEE) == len(out) - off[-1], (cols, sel is not None, "fill")


def check_queue_extract(exts, dev, col_sets=QUEUE_COLS):
    """exts: buffer runners (data, cols) -> (status, bytes); dev:
    extract_cases' device runner (data, cols, select, cap, base)."""
    data = queue_file()
    for cols in col_sets:
        want = EC.extract(data, cols)
        assert want[0] == OK
        for ext in exts:
            got = ext(data, cols)
            assert got[0] == OK and got[1] == want[1], (cols, got[0], len(got[1]), len(want[1]))
        for sel in (None, queue_select()):
            err, off, recs = EC.device(data, cols, sel)
            st, gerr, goff, out = dev(data, cols, sel, None, 0)   # (it checks the fill behind the last record)
            assert (st, gerr) == (OK, NO_ERROR) == (OK, err), (cols, sel is not None, st, hex(gerr))
            assert goff == off and out[:off[-1]] == b"".join(recs), (cols, sel is not None)


# ---- stager_edges -----------------------------------------------------------

FAMILIES = ["req_len", "req_nul", "req_tabs", "tile_edge", "esc_edge", "dense", "wide", "late_bad"]


def family(name):
    return [(n, d) for n, d, _ in D.edge_files() if n.startswith(name)]


def stops_at(name):
    """The record the readers stop at, None where the file ends OK.  A NUL
    in REQ and a token count past S are irregular for the readers even where
    decompress accepts them."""
    if name.startswith("req_nul_"):
        return 1
    if name.startswith("req_tabs_"):
        return 2
    return 9 if name in ("late_bad_short", "late_bad_overshoot") else None


def edge_column_sets(S):
    sets = [[0], [S - 1], [S - 1, 0], list(range(0, S, 7))]
    if S >= 270:
        sets.append(list(range(240, 270)))           # the first window's edge
    if S >= 2060:
        sets.append(list(reversed(range(2025, 2060))))   # the staged piece's edge in esc_edge
    sets.append(list(range(S)) if S <= 3000 else random.Random(S).sample(range(S), 600))
    seen, out = set(), []
    for c in sets:
        if SC.check_cols(c, S) and tuple(c) not in seen:
            seen.add(tuple(c))
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def want_subset(name, cols):
    return SC.subset(dict(family(name))[name], list(cols))


@functools.lru_cache(maxsize=None)
def want_extract(name, cols):
    return EC.extract(dict(family(name))[name], None if cols is None else list(cols))


@functools.lru_cache(maxsize=None)
def want_counts(name):
    return CC.counts_full(dict(family(name))[name])


@functools.lru_cache(maxsize=None)
def want_matrix(name, layout):
    return MC.matrix(dict(family(name))[name], layout)


def check_edges_subset(dec, fam):
    """dec(data, cols) -> (status, bytes), its output cap at least
    decode_cases.edge_cap(data)."""
    files = family(fam)
    assert files
    for name, data in files:
        S = SC.parse_header(data)[1]
        head = data[:SC.parse_header(data)[0]].count(b"\n")
        for cols in edge_column_sets(S):
            want = want_subset(name, tuple(cols))
            at = stops_at(name)
            assert want[0] == (OK if at is None else E_FORMAT), (name, want[0])
            assert want[1].count(b"\n") - head == (D.records_in(data) if at is None else at) > 0, name
            got = dec(data, cols)
            assert got[0] == want[0], (name, cols[:8], len(cols), got[0], want[0])
            assert got[1] == want[1], (name, cols[:8], len(cols), len(got[1]), len(want[1]))


def check_edges_extract(ext, fam):
    """S = 40 000 with all 600 sampled columns stays on the wave path; all
    columns (cols None) is above extract's tile: every record byte-serial."""
    files = family(fam)
    assert files
    for name, data in files:
        h, S = SC.parse_header(data)
        for cols in [None] + edge_column_sets(S):
            want = want_extract(name, None if cols is None else tuple(cols))
            at = stops_at(name)
            assert want[0] == (OK if at is None else E_FORMAT), (name, want[0])
            kept = len(SC.hop(want[1][len(EC.header(data, h, cols)):])[0])
            assert kept == (D.records_in(data) if at is None else at) > 0, (name, kept)
            got = ext(data, cols)
            assert got[0] == want[0], (name, cols and cols[:8], got[0], want[0])
            assert got[1] == want[1], (name, cols and cols[:8], len(got[1]), len(want[1]))


def check_edges_counts(run, fam):
    """run: counts_cases' runner.  S = 40 000 is above the LDS limit: the
    histogram takes global atomics (H_GLOBAL)."""
    files = family(fam)
    assert files
    for name, data in files:
        want = want_counts(name)
        at = stops_at(name)
        assert (want[0], want[4]) == ((OK, CC.NO_RECORD) if at is None else (E_FORMAT, at)), (name, want[0], want[4])
        assert len(want[2]) == (D.records_in(data) if at is None else at) > 0, name
        CC.same(run(data, None), want, name)


def check_edges_matrix(run, fam):
    """run: matrix_cases' runner.  S = 40 000 is above every layout's tile:
    the byte-serial kernel writes every row (k_gm_seq<.., true>)."""
    files = family(fam)
    assert files
    for name, data in files:
        for layout in MC.LAYOUTS:
            want = want_matrix(name, layout)
            at = stops_at(name)
            assert (want[0], want[4]) == ((OK, MC.NO_RECORD) if at is None else (E_FORMAT, at)), (name, want[0], want[4])
            assert len(want[2]) == (D.records_in(data) if at is None else at) > 0, name
            MC.same(run(data, layout), want, (name, layout))
