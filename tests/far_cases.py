"""Where in memory the records lie ("far placements"): the
device entries on a few kilobytes of records placed so that byte offsets 2^31
and 2^32 fall before, inside and behind them.  A data section larger than
4 GiB hands every kernel absolute record starts of that size; the kernels
carry them as 64-bit words and work record-relative in 32 bits, and nothing
but these cases holds them to it.

Arena      one allocation of FAR + SLACK bytes, made once per process: the
           input of every call starts at its base.  host_arena() is a lazy
           anonymous mapping (only the pages written are touched); the GPU
           suite brings its own (an uninitialised tensor).
Placement  a shift sh: the body's bytes at arena[sh, sh + len(body)), the call
           gets the arena's base, rec + sh and in_bytes = sh + len(body).
Decoy      for a placement with bytes at or above FAR, at the address a
           zero-extended 32-bit copy of each such record's offset reaches
           lies a well-formed record of the same length and sample count
           whose CHROM, POS and genotypes differ: a truncated offset gives a
           plausible wrong answer, not a read of unwritten memory.

The expected values are the suites' restatements on (body, rec); every
placement must also give the control placement's result (sh = 0) word for
word.  Entries that report input byte offsets are given rec + sh.  Every
comparison is exact.  The check_* functions take callables, as the other
*_cases.py modules; test_far_emu.py runs them on the CPU emulator,
test_gpu_far.py on the GPU."""
import collections
import functools
import mmap

import numpy as np

import counts_cases as CC
import decode_cases as D
import encode_cases as C
import extract_cases as XC
import index_cases as X
import index_edge_cases as IE
import ld_cases as LC
import matrix_cases as MC
import reader_edge_cases as RE
import regions_cases as RC
import sparse_cases as SP
import sparse_index_cases as SX
import subset_cases as SC

FAR = 1 << 32
SLACK = 8 << 20
BOUNDARIES = (1 << 31, 1 << 32)
OK = 0
NO_ERROR = (1 << 64) - 1
SB = 2048   # bytes of a staged piece (vcfc_decode_dev.h)
BASES = (FAR - 1, FAR, (1 << 40) + 7)   # base_offset / data_start of the entries that add one to an offset


class HostArena:
    """FAR + SLACK bytes of zero pages nobody has touched yet."""

    def __init__(self):
        try:
            self.map = mmap.mmap(-1, FAR + SLACK, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | 0x4000)   # MAP_NORESERVE
        except (OSError, ValueError, OverflowError) as e:
            raise AssertionError("the far arena (%d bytes of address space) could not be mapped: %s" % (FAR + SLACK, e))
        self.a = np.frombuffer(self.map, dtype=np.uint8)
        self.ptr = self.a.ctypes.data

    def write(self, off, data):
        self.a[off:off + len(data)] = np.frombuffer(data, dtype=np.uint8)

    def read(self, off, n):
        return self.a[off:off + n].tobytes()


@functools.lru_cache(maxsize=None)
def host_arena():
    return HostArena()


# ---- files and placements ---------------------------------------------------------

File = collections.namedtuple("File", "name data body rec S k bad")       # rec: n + 1 offsets; k: the chosen record
Placed = collections.namedtuple("Placed", "ptr in_bytes rec n S sh f")    # rec: n + 1 absolute offsets


def _file(name, data, k, bad=None):
    h, S = SC.parse_header(data)
    body = data[h:]
    rec, end = SC.hop(body)
    assert end == len(body) and 0 < k < len(rec) - 1, name
    return File(name, data, body, rec + [end], S, k, bad)


@functools.lru_cache(maxsize=None)
def files():
    """regular: 41 simple records; serial: records of the byte-serial kernels
    (k_cnt_seq, k_gm_seq, k_sub_wseq, k_ex_seq, k_dec_seq) among simple ones,
    the chosen one a long last token; pieces: a record of more than two staged
    pieces among short ones; irregular: an item that passes S, record 2."""
    out = [_file("regular", SC.batch_files()[4][1], 20)]
    recs, _ = RE.period(300)
    assert RE.KINDS == 11   # records 8, 9, 10 of the period: a two-token escape, a long last token, a zero-count item
    out.append(_file("serial", D.header(300) + b"".join(recs[:24]), 9))
    data = next(d for n, d, _ in D.edge_files() if n == "req_len_S257")
    h, S = SC.parse_header(data)
    rec, end = SC.hop(data[h:])
    cut = [data[h + a:h + b] for a, b in zip(rec, rec[1:] + [end])]
    out.append(_file("pieces", data[:h] + b"".join(cut[-6:] + cut[:3]), 5))   # REQ of 5000 bytes, behind 2055 .. 2059
    assert len(cut[-1]) > 2 * SB + 16 and SB + 16 <= len(cut[-1]) // 2 < 2 * SB
    name, data, at = MC.irregular_files()[0]
    out.append(_file("irregular", data, at, at))
    assert SC.regular(out[3].body, out[3].rec[at], out[3].rec[at + 1], out[3].S) is None
    return out


@functools.lru_cache(maxsize=None)
def match_file():
    """60 records of three CHROMs whose POS fields take every spelling strtoul reads (blanks, a sign, leading zeros)."""
    name, data, _ = D.query_files(1)[0]
    f = _file("mixed_pos", data, 30)
    spell = [RC.fields(f.body, f.rec[i], f.rec[i + 1])[1] for i in range(len(f.rec) - 1)]
    assert any(s[:1] == b" " for s in spell) and any(s[:1] == b"+" for s in spell) and any(s.isdigit() for s in spell)
    return f


def req_of(f, i):
    p = f.rec[i]
    return ((f.body[p + 4] & 0x3F) << 24) | (f.body[p + 5] << 16) | (f.body[p + 6] << 8) | f.body[p + 7]


def placements(f):
    """[(label, sh)]: the control, then per boundary the six shifts that put it
    at the chosen record's first byte, in its header, in REQ, in its sample
    items (the second staged piece of `pieces`), on its LF and at its end, and
    one with everything above the boundary at an odd address."""
    rk, L = f.rec[f.k], f.rec[f.k + 1] - f.rec[f.k]
    req = req_of(f, f.k)
    mid = L // 2 if L > 2 * SB else 8 + req + (L - 9 - req) // 2
    out = [("control", 0)]
    for B in BOUNDARIES:
        for d in (0, 3, 8 + req // 2, mid, L - 1, L):
            out.append(("2^%d-%d" % (B.bit_length() - 1, d), B - rk - d))
        out.append(("2^%d+5" % (B.bit_length() - 1), B + 5))
    return out


def check_builder(fs=None):
    """What the placements promise, on the CPU."""
    for f in (files() + [match_file()]) if fs is None else fs:
        n = len(f.rec) - 1
        pl = placements(f)
        assert len(pl) == 15 and pl[0] == ("control", 0)
        for B in BOUNDARIES:
            mine = [sh for label, sh in pl if label.startswith("2^%d-" % (B.bit_length() - 1))]
            assert len(mine) == 6 and len(set(mine)) == 6
            straddle = starts = 0
            for sh in mine:
                assert 0 <= sh and sh + len(f.body) + 64 <= FAR + SLACK
                assert sh + f.rec[1] <= B, (f.name, "a record wholly below")
                assert sh + f.rec[n - 1] >= B, (f.name, "a record wholly above")
                straddle += any(sh + f.rec[i] < B < sh + f.rec[i + 1] for i in range(n))
                starts += any(sh + f.rec[i] == B for i in range(n))
            assert straddle >= 4 and starts == 2, (f.name, B, straddle, starts)
            if f.bad is not None:
                assert any(sh + f.rec[f.bad] >= B for sh in mine), f.name
        assert any(sh + len(f.body) > FAR for _, sh in pl)
    assert [f.name for f in files()] == ["regular", "serial", "pieces", "irregular"]


def decoy_record(length, i, S):
    """A simple record of `length` bytes and S samples, 1|1 then 0|0 runs, on CHROM 9."""
    fld = [b"9", b"%d" % (7 + i), b"x", b"C", b"T", b"1", b"P", b".", b"GT"]
    items = b"\x81" + D.fill(S - 1)
    pad = length - (8 + len(b"\t".join(fld)) + 1 + len(items) + 1)
    assert pad >= 0, (length, S)
    fld[7] += b"x" * pad
    r = D.rec(b"\t".join(fld) + b"\t", items)
    assert len(r) == length and SC.regular(r, 0, length, S) is not None
    return r


def place(arena, f, sh):
    n = len(f.rec) - 1
    assert 0 <= sh and sh + len(f.body) + 64 <= FAR + SLACK
    for i in range(n):
        if sh + f.rec[i] >= FAR:
            at = (sh + f.rec[i]) % FAR
            assert at + (f.rec[i + 1] - f.rec[i]) <= sh, "the decoy would lie in the records"
            arena.write(at, decoy_record(f.rec[i + 1] - f.rec[i], i, f.S))
    arena.write(sh, f.body)
    return Placed(arena.ptr, sh + len(f.body), [r + sh for r in f.rec], n, f.S, sh, f)


def selects(f):
    n = len(f.rec) - 1
    return [None, [int(i % 3 != 1 or i == f.k) for i in range(n)]]


def first_diff(a, b):
    if type(a) is not type(b) and not (isinstance(a, (list, tuple)) and isinstance(b, (list, tuple))):
        return "types %s / %s" % (type(a).__name__, type(b).__name__)
    if isinstance(a, (list, tuple, bytes)):
        if len(a) != len(b):
            return "lengths %d / %d" % (len(a), len(b))
        for k in range(len(a)):
            if a[k] != b[k]:
                d = first_diff(a[k], b[k]) if isinstance(a[k], (list, tuple, bytes)) else "%r / %r" % (a[k], b[k])
                return "[%d] %s" % (k, d)
        return None
    return None if a == b else "%r / %r" % (a, b)


_WANT = {}


def memo(tag, fn):
    """A restatement's value for (entry, file, variant): computed once, shared by every placement and both suites."""
    key = (tag[0], tag[1], tag[3])
    if key not in _WANT:
        _WANT[key] = fn()
    return _WANT[key]


def sweep(arena, what, fs, variants, call, verify, moves=False):
    """Every placement of every file: call(P, v) for each variant v of
    variants(f), verify(f, v, got, sh, tag) against the restatement, and --
    unless the result moves with the input's offsets -- the control's result
    again: all of it, or what verify returns where the entry leaves a part of
    its output undefined behind an error word."""
    for f in fs:
        base = {}
        for label, sh in placements(f):
            P = place(arena, f, sh)
            for vi, v in enumerate(variants(f)):
                got = call(P, v)
                tag = (what, f.name, label, vi)
                kept = verify(f, v, got, sh, tag)
                got = got if kept is None else kept
                if sh == 0:
                    base[vi] = got
                elif not moves:
                    assert got == base[vi], tag + ("differs from the control placement at", first_diff(got, base[vi]))


# ---- matching -------------------------------------------------------------------------
# match(P, q) -> (status, err word, flags);  q = (ref, has_range, start, end)
# regions(P, region text) -> (status, err word, flags)

def _pos(f):
    """POS of the chosen record (plain decimal in every file but mixed_pos)."""
    return int(RC.fields(f.body, f.rec[f.k], f.rec[f.k + 1])[1])


def _queries(f):
    if f.name == "mixed_pos":
        return [(b"1", False, 0, 0), (b"2", True, 100, 400), (b"", True, 150, 500), (b"chrX", True, 0, (1 << 64) - 1)]
    p = _pos(f)
    return [(b"22", False, 0, 0), (b"22", True, p - 1, p), (b"", True, 0, p), (b"", False, 0, 0), (b"21", True, p, p)]


def want_flags(f, decide):
    flags, err = [], NO_ERROR
    for i in range(len(f.rec) - 1):
        m = decide(f.body, f.rec[i], f.rec[i + 1])
        if m is None:
            err = min(err, (i << 8) | (3 if RC.fields(f.body, f.rec[i], f.rec[i + 1]) is None else 2))
        flags.append(1 if m else 0)
    return err, flags


def check_match(arena, match):
    hits = []

    def verify(f, q, got, sh, tag):
        err, flags = memo(tag, lambda: want_flags(f, lambda b, rs, re: CC.match(b, rs, re, *q)))
        assert got == (OK, err, flags), tag + (first_diff(got, (OK, err, flags)),)
        hits.append(sum(flags))
    sweep(arena, "query_match", files() + [match_file()], _queries, match, verify)
    assert any(0 < h < 10 for h in hits) and any(h >= 20 for h in hits)


REGION_TEXT = {"mixed_pos": b"1:100-300\n2\t90\t400\nchrX:0-18446744073709551615\n:480-520\n"}


def _region_texts(f):
    p = 0 if f.name in REGION_TEXT else _pos(f)
    return [REGION_TEXT.get(f.name, b"22:%d-%d\n22\t%d\t%d\n21:0-1000\n:%d-%d\n" % (p - 1, p, p + 4, p + 7, 100, 101))]


def check_regions(arena, regions):
    def verify(f, text, got, sh, tag):
        flags, err = memo(tag, lambda: RC.expected(f.body, f.rec, RC.parse_text(text)))
        assert 0 < sum(flags) < len(flags)
        assert got == (OK, err, flags), tag + (first_diff(got, (OK, err, flags)),)
    sweep(arena, "regions_match", files() + [match_file()], _region_texts, regions, verify)


# ---- decode ---------------------------------------------------------------------------
# sizes(P) -> (status, err word, line_off, pos_off, pos_len, ccount)
# decode(P, select or None, exact) -> (status, err word, line_off, out bytes up to line_off[n])

_LINES = {}


def _lines(f):
    if f.name not in _LINES:
        h = SC.parse_header(f.data)[0]
        _LINES[f.name] = [RC.full_line(f.data, h, f.body, f.rec[i], f.rec[i + 1], f.S) for i in range(len(f.rec) - 1)]
    return _LINES[f.name]


def check_sizes(arena, sizes):
    def verify(f, v, got, sh, tag):
        rows, bad, code = memo(tag, lambda: IE.gap_rows(f.data))
        st, err, lo, po, pl, cc = got
        assert st == OK and lo[0] == 0, tag
        if bad < 0:
            assert err == NO_ERROR and len(rows) == len(f.rec) - 1, tag + (hex(err),)
        else:
            assert err >> 8 == bad and err & 0xFF in ((code,) if code else (2, 3)), tag + (hex(err),)
        for i, (t, off, n, c) in enumerate(rows):
            assert (po[i], pl[i], lo[i + 1] - lo[i], cc[i]) == (off + sh, len(t), n, c), tag + (i,)
    sweep(arena, "decode_sizes", files(), lambda f: [None], lambda P, v: sizes(P), verify, moves=True)


def check_decode(arena, decode):
    def verify(f, v, got, sh, tag):
        sel, exact = v
        lines = [l if sel is None or sel[i] else b"" for i, l in enumerate(_lines(f))]
        st, err, lo, out = got
        bad = next((i for i, l in enumerate(lines) if l is None), None)
        if bad is not None:   # (lines behind an error word are not meaningful)
            assert st == OK and err >> 8 == bad and err & 0xFF in (2, 3, 4), tag + (hex(err),)
            return st, err
        off = [0]
        for l in lines:
            off.append(off[-1] + len(l))
        if err == NO_ERROR or exact:   # (a light plan may ask for the exact one: code 4)
            assert (st, err, lo) == (OK, NO_ERROR, off) and out == b"".join(lines), tag + (hex(err), first_diff(lo, off))
        else:
            assert st == OK and err & 0xFF == 4, tag + (hex(err),)
            return st, err
    sweep(arena, "decode_records", files(), lambda f: [(s, e) for s in selects(f) for e in (False, True)],
          lambda P, v: decode(P, v[0], v[1]), verify)


# ---- the readers ------------------------------------------------------------------------
# subset(P, cols, select) -> (status, err word, line_off, out bytes up to line_off[n])
# counts(P, select) -> (status, err word, rows as lists, sample table as lists)
# matrix(P, layout, select, row_stride, out_cap, alloc) -> (status, err word, the alloc + MC.CANARY bytes, row_of)
# extract(P, cols or None, select) -> (status, err word, rec_off, out bytes up to rec_off[n])
# ldwin(P, W, select, pairs_cap, alloc_slots) -> (status, err word, the 36 * alloc_slots + LC.CANARY bytes, row_of)

def _regular(f, i):
    return SC.regular(f.body, f.rec[i], f.rec[i + 1], f.S)


def _on(f, sel):
    return [i for i in range(len(f.rec) - 1) if sel is None or sel[i]]


def _bad_word(f, sel):
    bad = [i for i in _on(f, sel) if _regular(f, i) is None]
    return (bad[0] << 8) | 3 if bad else NO_ERROR


def _columns(f):
    return [[f.S - 1, 0, f.S // 2], list(range(f.S))]


def check_subset(arena, subset):
    def verify(f, v, got, sh, tag):
        cols, sel = v
        err = _bad_word(f, sel)
        st, gerr, lo, out = got
        assert (st, gerr) == (OK, err), tag + (hex(gerr), hex(err))
        if err == NO_ERROR:
            def want():
                lines = [SC.line(*_regular(f, i), cols) if sel is None or sel[i] else b"" for i in range(len(f.rec) - 1)]
                off = [0]
                for l in lines:
                    off.append(off[-1] + len(l))
                return off, b"".join(lines)
            off, text = memo(tag, want)
            assert lo == off and out == text, tag + (first_diff(lo, off),)
            return None
        return st, gerr
    sweep(arena, "decode_samples", files(), lambda f: [(c, s) for c in _columns(f) for s in selects(f)],
          lambda P, v: subset(P, v[0], v[1]), verify)


def check_counts(arena, counts):
    def verify(f, sel, got, sh, tag):
        err = _bad_word(f, sel)
        st, gerr, rows, tab = got
        assert (st, gerr) == (OK, err), tag + (hex(gerr), hex(err))
        stop = len(f.rec) - 1 if err == NO_ERROR else err >> 8
        def table():
            wt = [[0] * 5 for _ in range(f.S)]
            for i in _on(f, sel):
                for j, t in enumerate(_regular(f, i)[1]):
                    wt[j][CC.CLASS.get(t, 4)] += 1
            return wt
        want, wt = memo(tag, lambda: ([CC.row(_regular(f, i)[1]) if sel is None or sel[i] else [0] * 8 for i in range(stop)],
                                      table() if err == NO_ERROR else None))
        assert rows[:stop] == want, tag + (first_diff(rows[:stop], want),)
        if err == NO_ERROR:
            assert tab == wt, tag + (first_diff(tab, wt),)
            return None
        return st, gerr, rows[:stop]
    sweep(arena, "genotype_counts", files(), selects, counts, verify)


def check_matrix(arena, matrix):
    def variants(f):
        return [(layout, sel) for layout in MC.LAYOUTS for sel in selects(f)]

    def shape(f, v):
        rb = MC.row_bytes(v[0], f.S)
        return rb + 1, len(_on(f, v[1])) * (rb + 1)

    def verify(f, v, got, sh, tag):
        stride, cap = shape(f, v)
        err, buf, mask, row_of = memo(tag, lambda: MC.expect_device(f.body, f.rec, f.S, v[0], v[1], stride, cap, cap))
        st, gerr, gbuf, grow_of = got
        assert (st, gerr, grow_of) == (OK, err, row_of), tag + (hex(gerr), hex(err))
        assert len(gbuf) == len(buf) and LC.first_diff(gbuf, buf, mask) is None, tag + (LC.first_diff(gbuf, buf, mask),)
        return st, gerr, grow_of, bytes(g if m else 0 for g, m in zip(gbuf, mask))
    sweep(arena, "genotype_matrix", files(), variants, lambda P, v: matrix(P, v[0], v[1], *shape(P.f, v), shape(P.f, v)[1]), verify)


def check_extract(arena, extract):
    def verify(f, v, got, sh, tag):
        cols, sel = v
        err, off, recs = memo(tag, lambda: XC.device(f.data, cols, sel))
        st, gerr, goff, out = got
        assert err == _bad_word(f, sel)
        assert (st, gerr, goff) == (OK, err, off) and out == b"".join(recs), tag + (hex(gerr), hex(err), first_diff(goff, off))
    sweep(arena, "extract_samples", files(), lambda f: [(c, s) for c in [None] + _columns(f)[:1] for s in selects(f)],
          lambda P, v: extract(P, v[0], v[1]), verify)


LD_W = 3


def check_ld_window(arena, ldwin):
    def verify(f, sel, got, sh, tag):
        slots = len(_on(f, sel)) * LD_W
        err, buf, mask, row_of = memo(tag, lambda: LC.expect_window(f.body, f.rec, f.S, LD_W, sel, slots, slots))
        st, gerr, gbuf, grow_of = got
        assert (st, gerr, grow_of) == (OK, err, row_of), tag + (hex(gerr), hex(err))
        assert len(gbuf) == len(buf) and LC.first_diff(gbuf, buf, mask) is None, tag + (LC.first_diff(gbuf, buf, mask),)
        return st, gerr, grow_of, bytes(g if m else 0 for g, m in zip(gbuf, mask))
    sweep(arena, "ld_window", files(), selects, lambda P, sel: ldwin(P, LD_W, sel, len(_on(P.f, sel)) * LD_W,
                                                                      len(_on(P.f, sel)) * LD_W), verify)


# ---- the indexes ----------------------------------------------------------------------------
# binned(P, base_offset, E) -> ([err word, count, largest end], the entries' bytes)
# span(P) -> (err word, ref_idx, pos, end) as lists
# spx(P, base_offset) -> ([err word, count, status 0, 1, 2], the kept entries' bytes, their file offsets)
# splan(P, data_start) -> (file_off, the 16 n prefix bytes, the two status words)

def _records(f):
    return [f.body[a:b] for a, b in zip(f.rec, f.rec[1:])]


def _base_sweep(arena, what, call, verify):
    """The placements with base 7, then the control placement with the far bases."""
    sweep(arena, what, files(), lambda f: [7], call, verify, moves=True)
    for f in files():
        P = place(arena, f, 0)
        for base in BASES:
            verify(f, base, call(P, base), 0, (what, f.name, "base", base))


def check_binned(arena, binned):
    def verify(f, v, got, sh, tag):
        base, E = v
        spans = memo(tag[:3] + (0,), lambda: [X.span(r) for r in _records(f)])
        sp = [(base + f.rec[i] + sh,) + s for i, s in enumerate(spans)]
        exp = X.parallel_entries(sp, E)
        assert max(s[3] for s in sp) < 1 << 32
        assert got == ([NO_ERROR, len(exp), max(s[3] for s in sp)], X.pack(exp)), tag + (got[0], len(exp))
    sweep(arena, "binned_index", files(), lambda f: [(7, 1), (7, 4)], lambda P, v: binned(P, *v), verify, moves=True)
    for f in files():
        P = place(arena, f, 0)
        for base in BASES:
            verify(f, (base, 4), binned(P, base, 4), 0, ("binned_index", f.name, "base", base))


def check_span(arena, span):
    def verify(f, v, got, sh, tag):
        sp = memo(tag, lambda: [X.span(r) for r in _records(f)])
        assert got == (NO_ERROR, [s[0] for s in sp], [s[1] for s in sp], [s[2] for s in sp]), tag
    sweep(arena, "record_span", files(), lambda f: [None], lambda P, v: span(P), verify)


def check_sparse_index(arena, spx):
    def verify(f, base, got, sh, tag):
        fields = memo(tag[:3] + (0,), lambda: [SX.create_fields(r) for r in _records(f)])
        offs = [SX.slot_offset(p) for _, p in fields]
        ent, off = [], []
        for i, (ref, pos) in enumerate(fields):
            if i + 1 == len(fields) or offs[i + 1] != offs[i]:
                ent.append(SX.entry(ref, pos, base + f.rec[i] + sh))
                off.append(offs[i])
        down = int(any(b < a for a, b in zip(offs, offs[1:])))
        want = ([NO_ERROR, len(off), 0, down, NO_ERROR], b"".join(ent), off)
        assert got == want, tag + (first_diff(got, want),)
    _base_sweep(arena, "sparse_index", spx, verify)


def check_sparse_plan(arena, splan):
    def verify(f, data_start, got, sh, tag):
        recs = _records(f)
        off, prefix, bad, anomaly = memo(tag, lambda: SP.plan(recs, data_start))
        fo, pf, st = got
        assert bad is None and int(st[0]) == SP.NONE and (int(st[1]) != 0) == anomaly, tag + (st,)
        assert list(fo) == off, tag + (first_diff(list(fo), off),)
        assert pf == b"".join(a + b for a, b in prefix), tag
    sweep(arena, "sparse_plan", files(), lambda f: list(BASES), splan, verify)


# ---- the digest -----------------------------------------------------------------------------
# rhash(P) -> the n digests

def check_record_hash(arena, rhash, py_hash64):
    def verify(f, v, got, sh, tag):
        want = memo(tag, lambda: [py_hash64(r) for r in _records(f)])
        assert list(got) == want, tag + (first_diff(list(got), want),)
    sweep(arena, "record_hash", files(), lambda f: [None], lambda P, v: rhash(P), verify)


# ---- the encoder's input ---------------------------------------------------------------------
# encode(arena ptr, line_off, line_len) -> (error word, rec_off as a list, the records' bytes)

def encode_batches():
    """(name, lines, the oracle's records): the hand-built families, and GT:DP:GQ rows (deferred records are on)."""
    out = [(name, C.family(name), C.expected(name)) for name in C.EDGE_FAMILIES]
    seed = C.SEEDED["gdg_batch"][1][0]
    return out + [("gdg_batch", C.family("gdg_batch", seed), C.expected("gdg_batch", seed))]


def line_shifts(offs, lens):
    """The shifts of placements() for a batch of lines, the chosen line the middle one."""
    k = len(offs) // 2
    out = [0]
    for B in BOUNDARIES:
        out += [B - offs[k] - d for d in (0, 3, lens[k] // 2, lens[k], lens[k] + 1)] + [B + 5]
    return out


def check_encode(arena, encode, names=None):
    for name, lines, want in encode_batches():
        if names is not None and name not in names:
            continue
        offs, lens, buf = [], [], bytearray()
        for ln in lines:
            offs.append(len(buf))
            lens.append(len(ln))
            buf += ln + b"\n"
        rec = [0]
        for w in want:
            rec.append(rec[-1] + len(w))
        for sh in line_shifts(offs, lens):
            assert 0 <= sh and sh + len(buf) + 64 <= FAR + SLACK
            if sh + len(buf) > FAR:   # the decoy: the same lines, every genotype's first allele another digit
                lo = max(0, FAR - sh)
                arena.write((sh + lo) % FAR, bytes(buf[lo:]).replace(b"\t0", b"\t1"))
            arena.write(sh, bytes(buf))
            err, grec, out = encode(arena.ptr, [o + sh for o in offs], lens)
            assert err == NO_ERROR and grec == rec, (name, sh, hex(err), first_diff(grec, rec))
            assert out == b"".join(want), (name, sh, first_diff(out, b"".join(want)))


# ---- strides -----------------------------------------------------------------------------------
# matrix_rows(P, layout, row_stride, out_cap) -> (status, err word, row_of): the rows into the suite's one
#     uninitialised output of STRIDE_ROWS * MATRIX_STRIDE bytes; peek(off, n) / poke(off, bytes) read and write it
# tables(arena ptr + off, n_rows, row_stride, S, W, pairs_cap) -> (status, err word, the band uint32[n_rows, W, 9])

STRIDE_ROWS = 5
MATRIX_STRIDE = (1 << 30) + 16
BED_STRIDE = (1 << 30) + 1
CANARY = 256


def check_matrix_stride(arena, matrix_rows, peek, poke):
    f = files()[0]
    n = STRIDE_ROWS
    g = File(f.name, f.data, f.body[:f.rec[n]], f.rec[:n + 1], f.S, 2, None)
    P = place(arena, g, 0)
    for layout in MC.LAYOUTS:
        rb = MC.row_bytes(layout, f.S)
        can = bytes((37 * j + layout) & 0xFF for j in range(CANARY))
        for r in range(n):
            if r:
                poke(r * MATRIX_STRIDE - CANARY, can)
            poke(r * MATRIX_STRIDE + rb, can)
        cap = n * MATRIX_STRIDE
        st, err, row_of = matrix_rows(P, layout, MATRIX_STRIDE, cap)
        assert (st, err, row_of) == (OK, NO_ERROR, list(range(n + 1))), (layout, st, hex(err))
        for r in range(n):
            want = MC.row(layout, _regular(g, r)[1])
            assert peek(r * MATRIX_STRIDE, rb) == want, (layout, r)
            if r:
                assert peek(r * MATRIX_STRIDE - CANARY, CANARY) == can, (layout, r, "before")
            assert peek(r * MATRIX_STRIDE + rb, CANARY) == can, (layout, r, "behind")


def check_bed_stride(arena, tables):
    """Five .bed rows at offsets r * BED_STRIDE of the arena (from byte 0 and
    from byte 5): rows 0 and 1 below 2^31, rows 2 and 3 above it, row 4 above
    2^32, where a 32-bit product lands in row 0's bytes."""
    S, n, W = 65, STRIDE_ROWS, 3
    rows = MC.matrix(LC.ld_file(S, n, 0.15, last=b"1|1"), MC.BED)[2]
    rb = MC.row_bytes(MC.BED, S)
    assert len(rows) == n and len(set(rows)) == n
    assert [r * BED_STRIDE >> 31 for r in range(n)] == [0, 0, 1, 1, 2]
    for start in (0, 5):
        assert start + (n - 1) * BED_STRIDE + rb + 64 <= FAR + SLACK
        for r, row in enumerate(rows):
            arena.write(start + r * BED_STRIDE, row)
        st, err, band = tables(arena.ptr + start, n, BED_STRIDE, S, W, n * W)
        assert (st, err) == (OK, NO_ERROR), (start, st, hex(err))
        assert np.array_equal(band, LC.band(rows, S, W)), start
