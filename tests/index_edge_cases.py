"""TEST INFRASTRUCTURE ONLY: hand-built records aimed at the constants of the
two external indexes and of gap-analysis (csrc/vcfc_index.hip,
csrc/vcfc_sparse_index.hip, csrc/vcfc_index_dev.h), and the checks that hold
an implementation to the restatements (index_cases.py, sparse_index_cases.py)
on them.  Each check takes callables, so test_index_emu.py /
test_sparse_index_emu.py run the families on the fiber emulator and
test_gpu_index.py / test_gpu_sparse_index.py on the GPU.

Records come from decode_cases.rec (S = 2, sample bytes 02 unless a family
says otherwise) and are used as they stand: none passes through an encoder,
so they include records compress would not write.  Every family asserts, on
the records' own geometry (TAB offsets from the CHROM start, record sizes,
start phases) and on the restatement, that it means what its name says.

Families: win_tabs, rec_len, more_tabs, sv_info, pos_spellings, err_order,
big_end, prefix_max (prefix_max_second_trip: GPU only), slot_runs,
gap_fields, queries; and the cases that moved here from the emulator files:
odd_fields, short_structural, unsorted, mutated.

Callables (a namespace with these attributes; `v` is a whole .vcfc):
  binned: span(v) -> (err word, ref[], pos[], end[])
          device(v, E, cap or None) -> ([err, count, largest end], entry bytes
                  below min(count, cap)); it checks that nothing lies past cap
          create(v, E) -> (status, index bytes, failing record or -1)
          query(v, index, region) -> (status, stdout)
  sparse: device(v) -> ([err, count, status0, status1, status2], entry bytes,
                  file offsets)
          create(v) -> (status, {offset: entry}, failing record, seek_failed,
                  apparent size)
          query(v, slots, region) -> (status, stdout)
          span(v, walk) -> (err word, ref[], pos[])       (emulator only)
          gap(v) -> (status, text, failing record)
          sizes(v, S) -> (err word, line offsets, pos offsets, pos lengths,
                  compressed counts)                      (GPU only)"""
import functools
import random
import struct

import decode_cases as D
import golden_io as G
import index_cases as X
import sparse_index_cases as SX

OK, E_FORMAT = 0, 8
NO_ERROR = (1 << 64) - 1
M64 = (1 << 64) - 1
WIN = 48            # IS_WIN, SPX_WIN: bytes from the CHROM start
GATE = 8 + WIN      # the smallest record the fast path takes
HDR = X.header(2)
S2 = b"\x02"        # two 0|0 tokens as one run byte

CHROM, POS, ID, REF, ALT, QUAL, FILTER, INFO = range(8)
_PAD = {CHROM: b"c", POS: b"0", ID: b"i", REF: b"A", ALT: b"C", QUAL: b"1", FILTER: b"P", INFO: b";"}


def F(chrom=b"1", pos=b"7", rid=b".", ref=b"A", alt=b"C", qual=b"1", filt=b"P", info=b"."):
    return [chrom, pos, rid, ref, alt, qual, filt, info]


def R(f, fmt=b"GT\t", samples=S2, lf=b"\n", last_tab=True):
    """A record of the eight fields f; fmt = b"": the eighth TAB is the last
    REQ byte; last_tab = False: seven TABs in REQ."""
    return D.rec(b"\t".join(f) + (b"\t" if last_tab else b"") + fmt, samples, lf)


def tabs(rec):
    """Offsets of the record's TABs from its CHROM start (sample bytes included)."""
    return [i - 8 for i in range(8, len(rec)) if rec[i] == 9]


def padded(f, k, n):
    """f with field k made n bytes longer (POS: leading zeros, else trailing filler)."""
    g = list(f)
    g[k] = _PAD[k] * n + g[k] if k == POS else g[k] + _PAD[k] * n
    return g


def place(f, k, w):
    """f with the field in front of TAB k (1-based) padded so that TAB k stands at window byte w."""
    t = tabs(R(f))[k - 1]
    assert t <= w, (f, k, w)
    g = padded(f, k - 1, w - t)
    assert tabs(R(g))[k - 1] == w
    return g


def vfile(recs, samples=2):
    return X.header(samples) + b"".join(recs)


def records(v):
    """[(offset, bytes)] of the records of a well-framed file."""
    p, out = X.header_end(v), []
    while p < len(v):
        k = X.record_at(v, p)
        assert k is not None
        out.append((p, v[p:p + k]))
        p += k
    return out


def fast_binned(rec):
    """The binned span takes its window path to the end: the gate, five TABs inside, no '<' in ALT."""
    t = tabs(rec)
    return len(rec) >= GATE and len(t) >= 5 and t[4] < WIN and b"<" not in rec[8 + t[3]:8 + t[4]]


def inside(rec):
    """How many of TABs 6 .. 8 lie inside the window."""
    return sum(1 for x in tabs(rec)[5:8] if x < WIN)


# ---- expected values ----------------------------------------------------------

def binned_spans(v):
    """Per record (ref, pos, end) or the code it is refused with."""
    out = []
    for _, r in records(v):
        try:
            out.append(X.span(r))
        except X.Throw as e:
            out.append(e.code)
    return out


def sparse_fields(v, walk=False):
    out = []
    for _, r in records(v):
        try:
            out.append((SX.walk_fields if walk else SX.create_fields)(r))
        except X.Throw as e:
            out.append(e.code)
    return out


def err_word(per_record):
    """The error word: the lowest refused record with its own code."""
    for i, s in enumerate(per_record):
        if isinstance(s, int):
            return (i << 8) | s
    return NO_ERROR


def check_binned_span(B, v):
    want = binned_spans(v)
    err, ref, pos, end = B.span(v)
    assert err == err_word(want), (hex(err), hex(err_word(want)))
    stop = len(want) if err == NO_ERROR else err >> 8
    for i in range(stop):
        assert (ref[i], pos[i], end[i]) == want[i], (i, ref[i], pos[i], end[i], want[i])
    return want


def check_binned_device(B, v, Es, caps=False):
    """The device entry: error word, count, largest end and the entries of the
    parallel form; caps: entries_cap = count - 1 and 0 as well."""
    want = binned_spans(v)
    ew = err_word(want)
    recs = records(v)
    for E in Es:
        words, ent = B.device(v, E, None)
        assert words[0] == ew, (E, hex(words[0]), hex(ew))
        if ew != NO_ERROR:
            continue
        sp = [(p,) + s for (p, _), s in zip(recs, want)]
        exp = X.parallel_entries(sp, E)
        assert words[1] == len(exp) and words[2] == max(s[3] for s in sp), (E, words, len(exp))
        assert ent == X.pack(exp), E
        if max(s[3] for s in sp) < 1 << 32:
            assert X.pack(X.sequential_entries(sp, E)) == ent
        if caps:
            openers = [i for i, s in enumerate(sp) if i == 0 or (i % E == 0 and s[3] > max(x[3] for x in sp[:i]))]
            assert len(openers) == len(exp)
            for cap in sorted({len(exp) - 1, 0}):
                words, ent = B.device(v, E, cap)
                assert words[0] == (openers[cap] << 8 | 0xFF), (E, cap, hex(words[0]), openers[cap])
                assert words[1] == len(exp) and ent == X.pack(exp)[:13 * cap], (E, cap, words)


def check_binned_create(B, v, Es):
    for E in Es:
        want = X.build_index(v, E)
        assert B.create(v, E) == want, (E, want[0], want[2])


def kept(v, fields):
    """The entries and offsets vcfc_sparse_index_device keeps: the last record of each run of equal adjacent offsets."""
    recs = records(v)
    ent, off = [], []
    for i, (ref, pos) in enumerate(fields):
        o = SX.slot_offset(pos)
        if i + 1 == len(fields) or SX.slot_offset(fields[i + 1][1]) != o:
            ent.append(SX.entry(ref, pos, recs[i][0]))
            off.append(o)
    return b"".join(ent), off


def check_sparse_device(B, v):
    want = sparse_fields(v)
    ew = err_word(want)
    words, ent, off = B.device(v)
    assert words[0] == ew, (hex(words[0]), hex(ew))
    if ew != NO_ERROR:
        return
    offs = [SX.slot_offset(p) for _, p in want]
    down = int(any(b < a for a, b in zip(offs, offs[1:])))
    neg = [i for i, o in enumerate(offs) if o >> 63]
    e_ent, e_off = kept(v, want)
    assert words[1:] == [len(e_off), 0, down, neg[0] if neg else NO_ERROR], words
    assert (ent, off) == (e_ent, e_off)


def check_sparse_span(B, v):
    for walk in (0, 1):
        want = sparse_fields(v, bool(walk))
        err, ref, pos = B.span(v, walk)
        assert err == err_word(want), (walk, hex(err), hex(err_word(want)))
        stop = len(want) if err == NO_ERROR else err >> 8
        assert list(zip(ref, pos))[:stop] == want[:stop], walk


def check_sparse_create(B, v):
    want = SX.create(v)
    got = B.create(v)
    assert got[:4] == want, (got[0], got[2], got[3], want[0], want[2], want[3], len(got[1]), len(want[1]))
    assert got[4] == SX.apparent_size(want[1])
    return want


def gap_rows(v):
    """Per record (POS text, its offset from the first record, decoded line
    bytes, compressed count) by the restatement, the failing record or -1,
    and its code (None: whichever the decoder refuses it with).
    A record whose second non-empty field does not lie wholly in its required
    columns -- fewer than two such fields there, or the second ended by the
    columns' end with sample tokens after it -- is refused: the reference
    prints the field as it runs on into the sample tokens (or, without
    samples, reads past its list of fields); k_gap_fields gives code 3, the
    one documented place where it and the decode plan differ."""
    h = X.header_end(v)
    S = len(v[:h].rstrip(b"\n").split(b"\n")[-1].split(b"\t")) - 9
    rows = []
    for i, (p, r) in enumerate(records(v)):
        line = X._line(v, h, p, len(r))
        if line is None:
            return rows, i, None
        terms = [t for t in line[:-1].split(b"\t") if t]
        req = ((r[4] & 0x3F) << 24) | (r[5] << 16) | (r[6] << 8) | r[7]
        inreq = [t for t in r[8:8 + req].split(b"\t") if t]
        if len(inreq) < 2 or (len(inreq) == 2 and S > 0 and r[8 + req - 1] != 9):
            return rows, i, 3
        # where the second non-empty field of the required columns starts
        q, seen, off = 8, 0, None
        for piece in r[8:8 + req].split(b"\t"):
            if piece:
                seen += 1
                if seen == 2:
                    off = q
                    assert piece == terms[1], (i, piece, terms[1])
                    break
            q += len(piece) + 1
        assert off is not None, i
        rows.append((terms[1], p - h + off, len(line), SX.compressed_count(r, max(S, 0))))
    return rows, -1, None


def check_gap(B, v, S):
    rows, bad, code = gap_rows(v)
    text = b"".join(b"%s %d %d\n" % (t, n, c) for t, _, n, c in rows)
    if hasattr(B, "gap"):
        st, txt, er = B.gap(v)   # (er is None where the entry does not report the record)
        assert st == (OK if bad < 0 else E_FORMAT) and er in (None, bad), (st, er, bad)
        assert txt.split(b"\n") == text.split(b"\n")
    if hasattr(B, "sizes"):
        err, lo, po, pl, cc = B.sizes(v, S)
        if bad < 0:
            assert err == NO_ERROR, hex(err)
        else:
            assert err >> 8 == bad and err & 0xFF in ((code,) if code else (2, 3)), (hex(err), bad, code)
        assert lo[0] == 0
        for i, (t, off, n, c) in enumerate(rows):
            assert (po[i], pl[i], lo[i + 1] - lo[i], cc[i]) == (off, len(t), n, c), i


def check_binned_queries(B, v, Es, regions):
    for E in Es:
        st, idx, _ = X.build_index(v, E)
        assert st == OK
        for q in regions:
            assert B.query(v, idx, q) == X.query(v, idx, q), (E, q)


def check_sparse_queries(B, v, regions):
    st, slots, _, _ = SX.create(v)
    assert st == OK and slots
    for q in regions:
        assert B.query(v, slots, q) == SX.query(v, slots, q), q


# ---- families: files ------------------------------------------------------------

def _numbered(recs_fields, **kw):
    return [R(f, **kw) for f in recs_fields]


@functools.lru_cache(maxsize=None)
def win_tabs():
    """{name: file}.  `create`: TAB k = 1 .. 5 at window bytes 46 .. 49 (47 the
    last inside); `tail`: TABs 6 .. 8 with 3, 2, 1, 0 of them inside, with and
    without FORMAT after the eighth; `walk`: TAB 2 at 46 .. 49."""
    create, seen = [], set()
    for k in range(1, 6):
        for w in (46, 47, 48, 49):
            f = place(F(pos=b"%d" % (100 + 10 * k + w)), k, w)
            r = R(f)
            assert tabs(r)[k - 1] == w and fast_binned(r) == (tabs(r)[4] < WIN)
            seen.add((k, w, fast_binned(r)))
            create.append(r)
    assert {(k, w) for k, w, _ in seen} == {(k, w) for k in range(1, 6) for w in (46, 47, 48, 49)}
    assert (5, 47, True) in seen and (5, 48, False) in seen and (4, 47, False) in seen
    tail, haves = [], []
    for fmt in (b"GT\t", b""):
        for t5 in (40, 42, 44, 46):
            r = R(place(F(pos=b"%d" % (500 + t5)), 5, t5), fmt=fmt)
            assert fast_binned(r) and tabs(r)[5:8] == [t5 + 2, t5 + 4, t5 + 6]
            haves.append((inside(r), len(tabs(r)) - 5 - inside(r)))
            tail.append(r)
    # (inside, TABs past the window): 3 - have of them are needed, fewer than 3 are there
    assert [h for h, _ in haves] == [3, 2, 1, 0] * 2 and (2, 1) in haves and (1, 2) in haves
    walk = []
    for w in (46, 47, 48, 49):
        r = R(place(F(pos=b"%d" % (900 + w)), 2, w))
        assert tabs(r)[1] == w and tabs(r)[0] == 1
        walk.append(r)
    return {"create": vfile(create), "tail": vfile(tail), "walk": vfile(walk), "all": vfile(create + tail + walk)}


@functools.lru_cache(maxsize=None)
def rec_len():
    """Record sizes 40 .. 72 (INFO padded: the five TABs stay in front), in an
    order that starts a window-path record at every rs mod 16; `last_55`,
    `last_56`: files that end with a record under and on the gate."""
    base = len(R(F()))
    assert base <= 40
    recs, phases, sizes = [], set(), set()
    at, pos = 0, 100
    for rep in range(4):
        order = list(range(40, 73))
        random.Random(rep).shuffle(order)
        for size in order + [41 + 2 * rep]:
            pos += 3
            r = R(padded(F(pos=b"%d" % pos, info=b"I"), INFO, size - base - len(b"%d" % pos) + 1))
            assert len(r) == size and tabs(r)[4] < WIN
            assert fast_binned(r) == (size >= GATE)
            if fast_binned(r):
                phases.add(at % 16)
            sizes.add(size)
            recs.append(r)
            at += size
    assert sizes == set(range(40, 73)) and phases == set(range(16))
    assert {55, 56, 57} <= sizes
    # the gate guards the window's loads: a last record one byte under it, whose window would end past the
    # data, and one on it, whose window ends with the data (the emulator keeps a guard page there)
    out = {"sizes": vfile(recs)}
    for size in (55, 56):
        r = R(padded(F(pos=b"9", info=b"I"), INFO, size - base))
        assert len(r) == size and (size - 8 >= WIN) == fast_binned(r)
        out["last_%d" % size] = vfile(recs[:5] + [r])
    return out


@functools.lru_cache(maxsize=None)
def more_tabs():
    """`ok`: the eighth TAB 0, 1, 15, 16, 17, 31, 32, 33 bytes past the window,
    with seven (one needed) and with five (three needed) TABs inside, the
    eighth followed by FORMAT or as the last REQ byte (the byte tail); the
    eighth TAB inside an escaped sample token.  `seven_*`: a record with only
    seven TABs, alone behind good records (code 3)."""
    ok = []
    for d in (0, 1, 15, 16, 17, 31, 32, 33):
        for fmt in (b"GT\t", b""):
            f = place(F(pos=b"%d" % (1000 + d)), 7, 46)     # TABs 1 .. 7 inside
            r = R(place(f, 8, WIN + d), fmt=fmt)
            assert fast_binned(r) and inside(r) == 2 and tabs(r)[7] == WIN + d
            assert (fmt == b"") == (len(r) == 8 + WIN + d + 3)
            ok.append(r)
            f = place(F(pos=b"%d" % (2000 + d)), 5, 44)     # TABs 1 .. 5 inside, 6 .. 8 past the window
            r = R(place(place(f, 6, WIN + d), 8, WIN + d + 4), fmt=fmt)
            assert fast_binned(r) and inside(r) == 0 and tabs(r)[5] == WIN + d
            ok.append(r)
    # the eighth TAB is the one that ends the first token of a two-token escape
    esc = R(place(F(pos=b"3000"), 7, 46), fmt=b"", samples=b"\xE20/1\t1/1", lf=b"\n", last_tab=False)
    assert len(tabs(esc)) == 8 and tabs(esc)[7] > WIN and esc[8 + tabs(esc)[7] + 1:] == b"1/1\n"
    esc_sv = R(F(pos=b"3001", alt=b"<X>", info=b"END=3100;X"), fmt=b"", samples=b"\xE20/1\t1/1", last_tab=False)
    assert len(tabs(esc_sv)) == 8 and X.span(esc_sv)[2] == 3100   # (INFO runs on to that TAB: END=3100;X<E2>0/1)
    ok += [esc, esc_sv]
    out = {"ok": vfile(ok)}
    assert err_word(binned_spans(out["ok"])) == NO_ERROR == err_word(sparse_fields(out["ok"]))
    good = [R(F(pos=b"%d" % (10 + i))) for i in range(3)]
    for name, f in (("seven_short", F(pos=b"50")), ("seven_window", place(F(pos=b"51"), 5, 40)),
                    ("seven_past", place(place(F(pos=b"52"), 5, 44), 7, 70))):
        r = R(f, fmt=b"", last_tab=False)
        assert len(tabs(r)) == 7
        out[name] = vfile(good + [r] + good)
        assert err_word(binned_spans(out[name])) == (3 << 8 | 3)
        assert err_word(sparse_fields(out[name])) == NO_ERROR      # create reads five TABs of a plain ALT
    assert fast_binned(R(place(F(pos=b"51"), 5, 40), fmt=b"", last_tab=False))
    return out


SV_INFO = [b"END=-5, 70,+60", b"END=", b"END", b"=END=9;END=8", b"SVLEN=-9223372036854775808,4",
           b"SVLEN=18446744073709551615", b"X=1", b".", b"END=;SVLEN=5", b"END=7;END=900", b"SVLEN=3;SVLEN=-80",
           b"SVLEN=-9223372036854775808", b"DB;;SVLEN=-40,30;X==", b"END=4294967296"]
SV_THROWS = [b"END=1;=", b"A=B=C", b"END=1x", b"SVLEN=3,x"]


@functools.lru_cache(maxsize=None)
def sv_info():
    """`ok`: structural ALTs ('<' first, last, the only byte; an ALT across
    window byte 48) and the INFO forms, each with its five TABs inside and
    outside the window; `throw_*`: the four throwing forms, inside and outside."""
    ok, pos = [], 100
    alts = [b"<X>", b"<", b"C<", b"<C", b"A,<DEL>,G"]
    for alt in alts:
        for far in (0, 50):
            pos += 1
            r = R(padded(F(pos=b"%d" % pos, alt=alt, info=b"END=%d" % (pos + 30)), ID, far))
            assert (tabs(r)[4] < WIN) == (far == 0)
            ok.append(r)
    cross = R(place(F(pos=b"150", alt=b"CCC<CCCC", info=b"SVLEN=12"), 4, 44))
    assert tabs(cross)[3] < WIN < tabs(cross)[4] and cross[8 + WIN] == 0x3C
    plain_cross = R(place(F(pos=b"151", alt=b"CCCC,CCCCCC"), 4, 44))
    assert tabs(plain_cross)[3] < WIN < tabs(plain_cross)[4]
    ok += [cross, plain_cross]
    for info in SV_INFO:
        for far in (0, 50):
            pos += 2
            r = R(padded(F(pos=b"%d" % pos, alt=b"<X>", info=info), ID, far))
            assert (tabs(r)[4] < WIN) == (far == 0)
            ok.append(r)
    out = {"ok": vfile(ok)}
    assert err_word(binned_spans(out["ok"])) == NO_ERROR
    ends = {s[2] for s in binned_spans(out["ok"])}
    assert 0 in ends and 900 in ends and (1 << 32) in ends and any(e == p - 1 for _, p, e in binned_spans(out["ok"]))
    good = [R(F(pos=b"%d" % (10 + i))) for i in range(2)]
    for j, info in enumerate(SV_THROWS):
        for far in (0, 50):
            v = vfile(good + [R(padded(F(pos=b"60", alt=b"<X>", info=info), ID, far))] + good)
            assert err_word(binned_spans(v)) == (2 << 8 | 2) == err_word(sparse_fields(v))
            assert err_word(sparse_fields(v, True)) == NO_ERROR    # the walk reads CHROM and POS only
            out["throw_%d_%s" % (j, "far" if far else "near")] = v
    return out


POS_GOOD = [b"", b"0", b"+5", b"-1", b"007", b"18446744073709551616", b"18446744073709551615", b"1", b" 0", b"-0",
            b"18446744073709551614", b"99999999999999999999", b"\v\f\r 9", b"-18446744073709551615"]
POS_BAD = [b" ", b"+", b"-", b"1x", b"5 ", b"+-1", b"0x10", b"1.5", b"\x00"]


@functools.lru_cache(maxsize=None)
def pos_spellings():
    """`ok`: every spelling strtoul takes whole (POS read in the window and,
    with a long CHROM, byte by byte); `bad_*`: one that it does not (code 2 in
    both indexes); `bad_short_*`: the same with seven TABs (code 3 in the
    binned index, whose TAB search comes first, code 2 in the sparse create)."""
    ok = []
    for p in POS_GOOD:
        ok.append(R(F(pos=p)))
        ok.append(R(padded(F(pos=p, chrom=b"chr1"), CHROM, 50)))
        ok.append(R(padded(F(pos=p), INFO, 30)))
    out = {"ok": vfile(ok)}
    assert err_word(binned_spans(out["ok"])) == NO_ERROR == err_word(sparse_fields(out["ok"]))
    assert {s[1] for s in binned_spans(out["ok"])} >= {0, 5, 7, 9, M64, M64 - 1, 1}
    good = [R(F(pos=b"%d" % (10 + i))) for i in range(2)]
    for j, p in enumerate(POS_BAD):
        assert X.strtoul_whole(p) is None
        for far, name in ((0, "near"), (30, "far")):
            v = vfile(good + [R(padded(F(pos=p), INFO, far))] + good)
            assert err_word(binned_spans(v)) == (2 << 8 | 2) == err_word(sparse_fields(v)) == err_word(sparse_fields(v, True))
            out["bad_%d_%s" % (j, name)] = v
            v = vfile(good + [R(padded(F(pos=p), QUAL, far), fmt=b"", last_tab=False)] + good)
            assert err_word(binned_spans(v)) == (2 << 8 | 3) and err_word(sparse_fields(v)) == (2 << 8 | 2)
            out["bad_short_%d_%s" % (j, name)] = v
    return out


ERR_AT = (0, 63, 64, 255, 256, 300)


@functools.lru_cache(maxsize=None)
def err_order():
    """301 records; the records ERR_AT[j:] fail, with codes 2 and 3 in turn
    (and 3 and 2): the lowest names the error word with its own code."""
    out = {}
    for j in range(len(ERR_AT)):
        for first in (2, 3):
            recs = []
            for i in range(301):
                if i in ERR_AT[j:]:
                    code = first if ERR_AT.index(i) % 2 == 0 else 5 - first
                    # code 2: a POS that does not parse; code 3: two TABs only (the sparse walk's second is missing)
                    recs.append(R(F(pos=b"1x")) if code == 2 else D.rec(b"1\t%d" % (100 + i), S2))
                else:
                    recs.append(R(padded(F(pos=b"%d" % (100 + i)), INFO, i % 40)))
            v = vfile(recs)
            want = ERR_AT[j] << 8 | (first if j % 2 == 0 else 5 - first)
            assert err_word(binned_spans(v)) == want == err_word(sparse_fields(v)) == err_word(sparse_fields(v, True))
            out["from_%d_code_%d" % (ERR_AT[j], want & 0xFF)] = v
    return out


BIG = [(1 << 32), (1 << 32) + 5, 0xFFFFFFF0 + (1 << 33), (1 << 40) + 1, M64, (1 << 63) + 2]


def _end_rec(i, end):
    """Record i (POS 1000 + i) whose end position is `end`."""
    if end == M64:
        return R(F(pos=b"0", ref=b"", alt=b""))
    if end >> 63:   # (an END list is compared as signed: a plain record at that POS)
        return R(F(pos=b"%d" % end))
    return R(F(pos=b"%d" % (1000 + i), alt=b"<X>", info=b"END=%d" % end))


@functools.lru_cache(maxsize=None)
def big_end():
    """600 records (three blocks).  `at_<p>`: one end at or above 2^32 at
    record p (lanes 0, 31, 32, 63; records 64, 255, 256; the last block);
    `halves`: several, whose low words are ordered against the full values."""
    out = {}
    n = 600
    for j, p in enumerate((0, 31, 32, 63, 64, 255, 256, 599)):
        recs = [_end_rec(i, BIG[j % len(BIG)]) if i == p else R(F(pos=b"%d" % (1000 + i))) for i in range(n)]
        out["at_%d" % p] = vfile(recs)
        sp = binned_spans(out["at_%d" % p])
        assert sp[p][2] == BIG[j % len(BIG)] and max(s[2] for s in sp) == sp[p][2]
    # full values rise while the low words fall, then the reverse: a scan on one half fails either way
    seq = {10: (1 << 32) + 9, 31: (2 << 32) + 7, 32: (3 << 32) + 5, 63: (3 << 32) + 4, 64: (4 << 32) + 1,
           100: 0xFFFFFFF0, 255: (4 << 32) + 0xFFFFFFF0, 256: (5 << 32), 257: (4 << 32) + 0xFFFFFFFF,
           300: (1 << 63) + 2, 511: M64, 512: (1 << 63) + 9, 599: M64}
    recs = [_end_rec(i, seq[i]) if i in seq else R(F(pos=b"%d" % (1000 + i))) for i in range(n)]
    out["halves"] = vfile(recs)
    sp = binned_spans(out["halves"])
    assert all(sp[i][2] == e for i, e in seq.items())
    lows = [(seq[a] & 0xFFFFFFFF) < (seq[b] & 0xFFFFFFFF) for a, b in ((31, 10), (32, 31), (64, 63), (256, 255))]
    fulls = [seq[a] > seq[b] for a, b in ((31, 10), (32, 31), (64, 63), (256, 255))]
    assert all(lows) and all(fulls)
    assert seq[257] < seq[256] and (seq[257] & 0xFFFFFFFF) > (seq[256] & 0xFFFFFFFF)
    for v in out.values():   # the host replay differs from the parallel form somewhere
        assert err_word(binned_spans(v)) == NO_ERROR
    return out


NS = (1, 2, 63, 64, 65, 255, 256, 257)


def bins_for(n):
    return sorted({1, 2, 63, 64, 65, 255, 256, 257, max(n - 1, 1), n, n + 1})


def _pos_file(ends):
    """Plain SNVs whose end positions (= POS) are `ends`."""
    return vfile([R(F(pos=b"%d" % e)) for e in ends])


@functools.lru_cache(maxsize=None)
def prefix_max(n):
    """{name: (file, bins)} for n records: ends decreasing, all equal, one huge
    early end, and per bin size E a staircase that rises once at i % E == 0
    and once at i % E == E - 1."""
    out = {"decreasing": (_pos_file([5000 - i for i in range(n)]), bins_for(n)),
           "equal": (_pos_file([777] * n), bins_for(n)),
           "huge_early": (_pos_file([100 + i if i != min(1, n - 1) else 4000000000 for i in range(n)]), bins_for(n))}
    for E in bins_for(n):
        a, b = E, 2 * E - 1 if E > 1 else 2
        if b >= n:
            continue
        ends = [100 + (i >= a) + (i >= b) for i in range(n)]
        assert a % E == 0 and b % E == E - 1 and ends[a] > ends[a - 1] and ends[b] > ends[b - 1]
        out["stairs_%d" % E] = (_pos_file(ends), [E])
    return out


def prefix_max_second_trip():
    """65 536 + 300 short records: the block maxima fill k_idx_partials' first
    256-wide trip and reach into its second.  `early`: the largest end is in
    block 0, so every later block's prefix comes through the carry; `late`:
    ends rise by one per record, so each trip's own scan decides."""
    n = 65536 + 300
    early = _pos_file([4000000000 if i == 3 else 1000 + i for i in range(n)])
    late = _pos_file([1000 + i for i in range(n)])
    assert (n + 255) // 256 > 256
    return {"early": early, "late": late}


@functools.lru_cache(maxsize=None)
def slot_runs():
    """Sparse index.  `runs`: runs of equal offsets of length 2 and 3 across
    lane 63 | 64 and record 255 | 256, a pair POS, POS + 2^56 (one offset after
    the wrap, two entries) and a pair POS, POS + 2^24 (offsets equal in their
    low 32 bits only); `run_300`: one run of 300 across both; `down`: a single
    decrease at 255 -> 256; `neg_*`: offsets negative as off_t."""
    n = 600

    def build(pos_of, chrom_of=lambda i: b"1"):
        return vfile([R(F(chrom=chrom_of(i), pos=b"%d" % pos_of(i))) for i in range(n)])
    ps = [100 + 2 * i for i in range(n)]
    ps[64] = ps[63]
    ps[255] = ps[256] = ps[254]
    ps[401] = ps[400] + (1 << 56)
    for i in range(500, n):
        ps[i] += 1 << 24
    ps[499] = ps[500] - (1 << 24)
    runs = build(lambda i: ps[i], lambda i: b"2" if i == 401 else b"1")
    so = [SX.slot_offset(p) for p in ps]
    assert so[63] == so[64] and so[254] == so[255] == so[256] and so[400] == so[401]
    assert so[500] - so[499] == 1 << 32 and all(b >= a for a, b in zip(so, so[1:]))
    run300 = build(lambda i: 100 + 2 * i if i < 100 else 300 if i < 400 else 100 + 2 * i)
    down = build(lambda i: 100 + 2 * i if i < 256 else 2 * i - 500)
    d = [SX.slot_offset(p) for _, p in sparse_fields(down)]
    assert [i for i in range(n - 1) if d[i + 1] < d[i]] == [255]
    big = 1 << 55
    neg_tail = build(lambda i: 100 + 2 * i if i < 200 else big + i)
    neg_mixed = build(lambda i: big + i if i in (70, 256, 300) else 100 + 2 * i)
    assert SX.slot_offset(big) >> 63
    return {"runs": runs, "run_300": run300, "down": down, "neg_tail": neg_tail, "neg_mixed": neg_mixed}


@functools.lru_cache(maxsize=None)
def gap_fields():
    """{name: (file, S)}: `fields`: empty leading fields and doubled TABs (POS
    is the second non-empty field), escapes ended by LF and by TAB, a
    two-token escape; `pos_last`: S = 0 records whose POS is the last REQ
    field, ended by the REQ end itself; `one_field`, `one_field_s0`: a record
    with fewer than two non-empty REQ fields behind good ones; `pos_runs_on`:
    the same POS-ends-REQ record with samples after it (refused)."""
    tail = b".\tA\tC\t1\tP\t.\tGT\t"
    recs = [D.rec(b"1\t77\t" + tail, S2), D.rec(b"\t\t1\t\t78\t.\tA\tC\tGT\t", S2),
            D.rec(b"\t1\t\t\t79\t\t\tA\t\t", S2),
            D.rec(b"1\t80\t" + tail, b"\x01\xE10/1"),                  # an escape ended by the LF
            D.rec(b"1\t81\t" + tail, b"\xE10/1\t\x01"),                # an escape ended by a TAB
            D.rec(b"1\t82\t" + tail, b"\xE20/1\t1/1"),                 # a two-token escape
            D.rec(b"1\t83\t" + tail, b"\xE1./.\t\xE11|2"),
            D.rec(b"X\t 84\t" + tail, b"\xA1\xC1")]
    assert all(r[8:].count(b"\t", 0, len(r) - 8) >= 9 for r in recs)
    out = {"fields": (vfile(recs), 2)}
    rows, bad, _ = gap_rows(out["fields"][0])
    assert bad == -1 and [r[0] for r in rows] == [b"77", b"78", b"79", b"80", b"81", b"82", b"83", b" 84"]
    assert [r[1] - sum(len(x) for x in recs[:i]) for i, r in enumerate(rows)][:3] == [10, 13, 13]
    # S = 0: eight TABs in REQ; POS ends with REQ itself, and with REQ's last TAB
    last = [D.rec(b"\t\t\t\t\t\t\t1\t91", b""), D.rec(b"1\t\t\t\t\t\t\t\t92", b""), D.rec(b"\t\t\t\t\t\t1\t93\t", b"")]
    out["pos_last"] = (vfile(last, 0), 0)
    rows, bad, _ = gap_rows(out["pos_last"][0])
    assert bad == -1 and [r[0] for r in rows] == [b"91", b"92", b"93"], (rows, bad)
    one = [D.rec(b"1\t94\t" + tail, S2), D.rec(b"\t\t95\t\t\t\t\t\t\t", S2), D.rec(b"1\t96\t" + tail, S2)]
    out["one_field"] = (vfile(one), 2)
    st, dec = G.oracle_decompress(out["one_field"][0])
    assert st == 0 and dec.count(b"\n") == 5      # the decoder takes the record; gap-analysis has no POS to print
    assert gap_rows(out["one_field"][0])[1:] == (1, 3)
    # POS ended by REQ's end with samples after it: the line's field is 990|0, which REQ does not hold
    on = [D.rec(b"1\t94\t" + tail, S2), D.rec(b"1\t\t\t\t\t\t\t\t\t99", S2), D.rec(b"1\t96\t" + tail, S2)]
    out["pos_runs_on"] = (vfile(on), 2)
    assert SX.gap_analysis(out["pos_runs_on"][0])[1].split(b"\n")[1] == b"990|0 20 21"
    assert gap_rows(out["pos_runs_on"][0])[1:] == (1, 3)
    one0 = [D.rec(b"\t\t\t\t\t\t\t1\t97", b""), D.rec(b"98\t\t\t\t\t\t\t\t", b"")]
    out["one_field_s0"] = (vfile(one0, 0), 0)
    assert G.oracle_decompress(out["one_field_s0"][0])[0] == 0 and gap_rows(out["one_field_s0"][0])[1:] == (1, 3)
    return out


QUERY_AFTER = (63, 64, 255, 256)


@functools.lru_cache(maxsize=None)
def queries():
    """300 sorted records of CHROM 1 (POS 100 + 10 i, every seventh a deletion
    of 25 bases, sizes on both sides of the gate) and the regions whose first
    record after the query is record 63, 64, 255, 256."""
    recs = []
    for i in range(300):
        f = F(pos=b"%d" % (100 + 10 * i), ref=b"A" * 25 if i % 7 == 0 else b"A")
        recs.append(R(padded(f, INFO, i % 30)))
    regions = ["1:%d-%d" % (100 + 10 * (r - 5), 100 + 10 * (r - 1)) for r in QUERY_AFTER]
    regions += ["1:%d-%d" % (100 + 10 * (r - 1) + 1, 100 + 10 * r - 1) for r in QUERY_AFTER]   # between two records
    regions += ["1:100-%d" % (100 + 10 * 255), "1:3000-4000", "2:1-9", "1"]
    return vfile(recs), regions


# ---- the cases that moved here from the emulator files ---------------------------

ODD_ROWS = [b"1\t 7\t.\tACG\tA\t1\tPASS\t.", b"1\t-3\t.\tA\tC\t1\tPASS\t.", b"1\t99999999999999999999\t.\tA\tC\t1\tPASS\t.",
            b"1\t50\t.\tA\t<X>\t1\tPASS\tEND=-5, 70,+60", b"1\t50\t.\tA\t<X>\t1\tPASS\tEND=",
            b"1\t50\t.\tA\t<X>\t1\tPASS\tEND", b"1\t50\t.\tA\t<X>\t1\tPASS\t=END=9;END=8",
            b"1\t50\t.\tA\t<X>\t1\tPASS\tSVLEN=-9223372036854775808,4",
            b"1\t50\t.\tA\tC<\t1\tPASS\tSVLEN=18446744073709551615",
            b"22\t0\t.\tA\t,\t1\tPASS\t.", b"M\t5\t" + b"i" * 70 + b"\tA\tCC\t1\tPASS\t.", b"23\t5\t.\tA\tC\t1\tPASS\t."]


def _compress(vcf):
    st, v, _ = G.oracle_compress(vcf)
    assert st == 0
    return v


def check_odd_fields(B):
    """Fields the generator does not draw: negative and overflowing POS,
    END lists with signs and blanks, '=' runs, duplicate keys, an ALT of commas only."""
    vcf = X.header(1) + b"".join(r + b"\tGT\t0|1\n" for r in ODD_ROWS)
    v = _compress(vcf)
    sp, bad = X.spans_of(v)
    assert bad is None
    err, ref, pos, end = B.span(v)
    assert err == NO_ERROR
    assert (ref, pos, end) == ([s[1] for s in sp], [s[2] for s in sp], [s[3] for s in sp])
    for E in (1, 2):
        assert B.create(v, E) == X.build_index(v, E)
    for bad_info in SV_THROWS:
        w = _compress(vcf + b"1\t60\t.\tA\t<X>\t1\tPASS\t" + bad_info + b"\tGT\t0|1\n")
        assert B.create(w, 1) == (E_FORMAT, b"", len(ODD_ROWS)) == X.build_index(w, 1), bad_info


SHORT_ROWS = [b"1\t7\t.\tA\tC\t1\tPASS\t.", b"1\t 9\t.\tACG\tA\t1\tPASS\t.", b"1\t12\t.\tA\t<X>\t1\tPASS\tEND=-5, 70,+60",
              b"1\t15\t.\tA\t<X>\t1\tPASS\tEND", b"1\t20\t.\tA\tC<\t1\tPASS\tSVLEN=18446744073709551615",
              b"22\t30\t.\tA\t,\t1\tPASS\t.", b"M\t35\t" + b"i" * 70 + b"\tA\tCC\t1\tPASS\t.",
              b"23\t40\t.\tA\t" + b"C" * 50 + b"<\t1\tPASS\tX=1", b"X\t36028797018963968\t.\tA\tC\t1\tPASS\t."]


def check_short_and_structural(B):
    """A record shorter than the 56-byte fast-path window (S = 1, short
    fields), structural ALTs (eight TABs and the INFO walk), fields the
    generator does not draw, and where the two passes differ: a bad INFO stops
    create and not the walk."""
    rows = SHORT_ROWS
    v = _compress(X.header(1) + b"".join(r + b"\tGT\t0|1\n" for r in rows))
    assert min(len(r) for _, r in records(v)) < GATE
    if hasattr(B, "span"):
        check_sparse_span(B, v)
    check_sparse_device(B, v)
    want = SX.create(v)
    assert want[0] == OK and want[3] == 1 and len(want[1]) == len(rows) - 1   # POS 2^55: the offset is negative as off_t
    assert B.create(v)[:4] == want
    for bad_info in SV_THROWS:
        w = _compress(X.header(1) + b"".join(r + b"\tGT\t0|1\n" for r in rows[:8]) +
                      b"M\t60\t.\tA\t<X>\t1\tPASS\t" + bad_info + b"\tGT\t0|1\n" + b"M\t61\t.\tA\tC\t1\tPASS\t.\tGT\t0|1\n")
        got = B.create(w)
        assert got[:4] == SX.create(w) and got[0] == E_FORMAT and got[2] == 8 and len(got[1]) == 8, bad_info
        assert B.device(w)[0][0] == (8 << 8 | 2)
        if hasattr(B, "span"):
            assert B.span(w, 0)[0] == (8 << 8 | 2) and B.span(w, 1)[0] == NO_ERROR
        slots = got[1]
        st, out = B.query(w, slots, "M:1-100")
        assert (st, out) == SX.query(w, slots, "M:1-100") and st == OK and out.count(b"\n") == 3   # M 35, the bad M 60, M 61


def check_unsorted(B):
    """Offsets that decrease: status[1], and the entries the reference's record-order writes leave."""
    v = SX.gen_vcfc(300, 17, pairs=(63, 255), unsorted=True)
    words, _, _ = B.device(v)
    assert words[0] == NO_ERROR and words[3] == 1 and words[4] == NO_ERROR
    got = B.create(v)
    assert got[:4] == SX.create(v)
    u = SX.file_bytes("unsorted")   # a slot written twice out of order: the later record stays
    st, slots = B.create(u)[:2]
    assert st == OK and struct.unpack("<BIQ", slots[SX.slot_offset(100)])[2] == \
        sorted(struct.unpack("<BIQ", e)[2] for e in slots.values())[-2]
    return got


# 1 .. 4: the seeds the emulator files drew; 18, 48, 69: chosen, by the restatement alone, for their
# code 3 refusals (two each) -- see mutated_floor
MUTATE_SEEDS = (1, 2, 3, 4, 18, 48, 69)


def mutate(v, rnd, patches):
    """Random byte patches in record headers (LEN, REQ) and prefixes (CHROM .. INFO)."""
    b = bytearray(v)
    recs = records(v)
    for _ in range(patches):
        p = recs[rnd.randrange(len(recs))][0] + rnd.choice([rnd.randrange(0, 8), rnd.randrange(8, 60)])
        if p < len(b):
            b[p] = rnd.choice([rnd.randrange(256), 9, 0x3C, 0x3D, 0x3B, 0x2C, 0x30])
    return bytes(b)


@functools.lru_cache(maxsize=None)
def mutated(seed, sparse):
    """[(file, base file)]: twelve mutations of the golden index_edge file and of a generated one."""
    rnd = random.Random(seed)
    base = [SX.file_bytes("index_edge"), SX.gen_vcfc(150, 77, pairs=(63,))] if sparse else \
        [X.file_bytes("index_edge"), X.gen_vcfc(150, 77)]
    return [(mutate(base[k % 2], rnd, rnd.randrange(1, 4)), base[k % 2]) for k in range(12)]


def refusal(v, sparse):
    """0 where create takes the whole file, else the code (2, 3) it refuses a
    record's fields with; 1: a record header it cannot read."""
    p = X.header_end(v)
    if p is None:
        return 1
    while p < len(v):
        k = X.record_at(v, p)
        if k is None:
            return 1
        try:
            (SX.create_fields if sparse else X.span)(v[p:p + k])
        except X.Throw as e:
            return e.code
        p += k
    return 0


def mutated_floor(sparse):
    """Over the seeds: how many files end OK, under code 2 and under code 3."""
    codes = [refusal(v, sparse) for seed in MUTATE_SEEDS for v, _ in mutated(seed, sparse)]
    return codes.count(0), codes.count(2), codes.count(3)


BINNED_MUT_Q = ("1:100-400", "2:100-2000", "X:1-100000", "foo:1-100000")
SPARSE_MUT_Q = BINNED_MUT_Q + ("1:60-90",)


def check_mutated_binned(B, seed, **kw):
    for k, (v, v0) in enumerate(mutated(seed, False)):
        idx0 = X.build_index(v0, 2)[1]
        want = X.build_index(v, 2)
        got = B.create(v, 2)
        assert got == want, (seed, k, got[0], got[2], want[0], want[2])
        for q in BINNED_MUT_Q:
            st_w, out_w = X.query(v, idx0, q)
            st, out = B.query(v, idx0, q, **kw)
            if st == OK:
                assert (st_w, out_w) == (OK, out), (seed, k, q)
            else:   # refused: nothing but lines the restatement also writes
                assert st == E_FORMAT and out_w.startswith(out), (seed, k, q, st)


def check_mutated_sparse(B, seed, **kw):
    for k, (v, v0) in enumerate(mutated(seed, True)):
        slots0 = SX.create(v0)[1]
        want = SX.create(v)
        got = B.create(v)
        assert got[:4] == want, (seed, k, got[0], got[2], want[0], want[2])
        for q in SPARSE_MUT_Q:
            st_w, out_w = SX.query(v, slots0, q)
            st, out = B.query(v, slots0, q, **kw)
            if st == OK:
                assert (st_w, out_w) == (OK, out), (seed, k, q)
            else:   # refused at a malformed record: the same lines up to it (its own line may or may not decode)
                assert st == E_FORMAT and (out_w.startswith(out) or (st_w == E_FORMAT and out.startswith(out_w))), \
                    (seed, k, q, st)


# ---- families: checks -----------------------------------------------------------

def _binned_all(B, v, Es=(1, 2, 64), caps=False):
    check_binned_span(B, v)
    check_binned_device(B, v, Es, caps)
    check_binned_create(B, v, Es)


def binned_win_tabs(B):
    for v in win_tabs().values():
        _binned_all(B, v)


def binned_rec_len(B):
    for v in rec_len().values():
        _binned_all(B, v, (1, 3, 64))


def binned_more_tabs(B):
    for v in more_tabs().values():
        _binned_all(B, v, (1, 2))


def binned_sv_info(B):
    for v in sv_info().values():
        _binned_all(B, v, (1, 2))


def binned_pos_spellings(B):
    for name, v in pos_spellings().items():
        want = check_binned_span(B, v)
        if name.startswith("bad_short"):
            assert want[2] == 3
        elif name.startswith("bad"):
            assert want[2] == 2
        check_binned_device(B, v, (1,))
        check_binned_create(B, v, (1, 2))


def binned_err_order(B):
    for v in err_order().values():
        _binned_all(B, v, (1,))


def binned_big_end(B):
    differ = False
    for v in big_end().values():
        _binned_all(B, v, (1, 2, 64))
        sp, _ = X.spans_of(v)
        differ = differ or any(X.pack(X.parallel_entries(sp, E)) != X.build_index(v, E)[1] for E in (1, 2, 64))
    assert differ   # somewhere the host replay is not the parallel form


def binned_prefix_max(B, n):
    for name, (v, Es) in prefix_max(n).items():
        check_binned_device(B, v, Es, caps=True)
        check_binned_create(B, v, sorted({Es[0], Es[-1], Es[len(Es) // 2]}))


def binned_prefix_max_second_trip(B):
    n = 65536 + 300
    for name, v in prefix_max_second_trip().items():
        check_binned_device(B, v, (1, 256))
        # what the carry between the two trips decides: after record 3 of `early` nothing opens, in `late` all do
        assert B.device(v, 1, None)[0][1] == (4 if name == "early" else n)
        assert B.device(v, 256, None)[0][1] == (1 if name == "early" else (n + 255) // 256)
        assert B.create(v, 256) == X.build_index(v, 256)


def binned_queries(B):
    v, regions = queries()
    sp, _ = X.spans_of(v)
    for r, q in zip(QUERY_AFTER, regions):   # the first record after the query
        a, b = G.oracle_parse_query(q.encode())[2:]
        assert min(i for i, s in enumerate(sp) if s[2] > b) == r
    check_binned_queries(B, v, (1, 7, 64), regions)
    check_binned_queries(B, win_tabs()["all"], (1, 3), ["1:100-200", "1:500-600", "1:900-950", "1", "c:1-999"])
    check_binned_queries(B, rec_len()["sizes"], (1, 5), ["1:100-130", "1:300-420", "1:480-2000"])
    check_binned_queries(B, sv_info()["ok"], (1, 4), ["1:100-120", "1:125-170", "1:1-1"])


def sparse_family(B, files):
    for v in files:
        if hasattr(B, "span"):
            check_sparse_span(B, v)
        check_sparse_device(B, v)
        check_sparse_create(B, v)


def sparse_win_tabs(B):
    sparse_family(B, win_tabs().values())


def sparse_rec_len(B):
    sparse_family(B, rec_len().values())


def sparse_more_tabs(B):
    sparse_family(B, more_tabs().values())


def sparse_sv_info(B):
    sparse_family(B, sv_info().values())


def sparse_pos_spellings(B):
    f = pos_spellings()
    # (the spellings at or above 2^55 give offsets no file system takes: create stops there, as the restatement)
    sparse_family(B, f.values())
    for name, v in f.items():
        if name.startswith("bad"):
            assert err_word(sparse_fields(v)) & 0xFF == 2


def sparse_err_order(B):
    sparse_family(B, err_order().values())


def sparse_slot_runs(B):
    f = slot_runs()
    sparse_family(B, f.values())
    assert B.device(f["down"])[0][3] == 1 and B.device(f["runs"])[0][3] == 0
    assert B.device(f["neg_tail"])[0][3:] == [0, 200] and B.device(f["neg_mixed"])[0][3:] == [1, 70]
    assert B.device(f["runs"])[0][1] == 600 - 4 and B.device(f["run_300"])[0][1] == 301
    assert B.create(f["neg_tail"])[3] == 1 and B.create(f["down"])[3] == 0


def sparse_gap_fields(B):
    for name, (v, S) in gap_fields().items():
        check_gap(B, v, S)
    for v in (win_tabs()["all"], rec_len()["sizes"], more_tabs()["ok"]):
        check_gap(B, v, 2)


def sparse_queries(B):
    v, regions = queries()
    fl = sparse_fields(v, True)
    for r, q in zip(QUERY_AFTER, regions):
        b = G.oracle_parse_query(q.encode())[3]
        assert min(i for i, s in enumerate(fl) if s[1] > b) == r
    check_sparse_queries(B, v, regions)
    check_sparse_queries(B, win_tabs()["walk"], ["1:946-949", "1:900-1000", "1:947-947", "1:1-2000"])
    check_sparse_queries(B, win_tabs()["all"], ["1:100-200", "1:540-546", "1:900-950", "1"])
    check_sparse_queries(B, rec_len()["sizes"], ["1:100-130", "1:300-420", "1:480-2000"])
    check_sparse_queries(B, slot_runs()["runs"], ["1:226-228", "1:608-612", "1:900-902", "1:100-1400"])


BINNED = {"win_tabs": binned_win_tabs, "rec_len": binned_rec_len, "more_tabs": binned_more_tabs,
          "sv_info": binned_sv_info, "pos_spellings": binned_pos_spellings, "err_order": binned_err_order,
          "big_end": binned_big_end, "queries": binned_queries}
SPARSE = {"win_tabs": sparse_win_tabs, "rec_len": sparse_rec_len, "more_tabs": sparse_more_tabs,
          "sv_info": sparse_sv_info, "pos_spellings": sparse_pos_spellings, "err_order": sparse_err_order,
          "slot_runs": sparse_slot_runs, "gap_fields": sparse_gap_fields, "queries": sparse_queries}


# ---- uploading a hand-built file ---------------------------------------------------

@functools.lru_cache(maxsize=4)
def upload(v, dev="cuda:0"):
    """(records on the GPU, their n + 1 offsets on the GPU, n, header bytes, data bytes) of a well-framed file."""
    import numpy as np
    import torch
    recs = records(v)
    h = X.header_end(v)
    ro = np.array([p - h for p, _ in recs] + [len(v) - h], dtype=np.int64)
    d = torch.from_numpy(np.frombuffer(v[h:] + b"\0", dtype=np.uint8).copy()).to(dev)   # (never empty)
    return d, torch.from_numpy(ro).to(dev), len(recs), h, len(v) - h


# ---- the files pinned to the reference CLI (tests/golden/index_edge_cases.json) -----

def holds_tabs(v):
    """Every record holds the TABs both creates read: none is refused with code 3."""
    return 3 not in binned_spans(v) and 3 not in sparse_fields(v)


def pinned_files():
    """{name: file}: the edge files whose records all hold their TABs.  Where
    they do not, the reference reads on into the next record -- the documented
    deviation -- and the restatement stays the authority."""
    out = {}
    for fam, files in (("win_tabs", win_tabs()), ("rec_len", rec_len()), ("more_tabs", more_tabs()),
                       ("sv_info", sv_info()), ("big_end", big_end()), ("slot_runs", slot_runs()),
                       ("pos_spellings", {k: v for k, v in pos_spellings().items() if not k.endswith("_far")}),
                       ("prefix_max_257", {k: v for k, (v, _) in prefix_max(257).items()
                                           if k in ("decreasing", "equal", "huge_early", "stairs_64")}),
                       ("gap_fields", {k: v for k, (v, _) in gap_fields().items()}),
                       ("queries", {"sorted": queries()[0]})):
        for k, v in files.items():
            if holds_tabs(v):
                out["%s/%s" % (fam, k)] = v
    return out


# gap-analysis is left out where the reference's own decoder reads on or has no second field to print
PINNED_NO_GAP = ("gap_fields/one_field", "gap_fields/one_field_s0", "gap_fields/pos_runs_on")
PINNED_BINNED_QUERIES = {"queries/sorted": (2, queries()[1]), "win_tabs/create": (1, ["1:100-200", "1", "c:1-999"]),
                         "rec_len/sizes": (2, ["1:100-130", "1:300-420", "1:480-2000"]),
                         "sv_info/ok": (2, ["1:100-120", "1:125-170", "1:1-1"])}
PINNED_SPARSE_QUERIES = {"queries/sorted": queries()[1], "win_tabs/walk": ["1:946-949", "1:900-1000", "1:947-947"],
                         "rec_len/sizes": ["1:100-130", "1:300-420", "1:480-2000"],
                         "slot_runs/runs": ["1:226-228", "1:608-612", "1:900-902", "1:100-1400"]}
PINNED_JSON = G.GOLDEN + "/index_edge_cases.json"


@functools.lru_cache(maxsize=None)
def pinned():
    """The recorded results, after checking that the generator still writes the files they were recorded over."""
    import json
    with open(PINNED_JSON) as f:
        d = json.load(f)
    files = pinned_files()
    assert sorted(files) == sorted(d["files"])
    for name, v in files.items():
        assert (len(v), X.sha(v)) == (d["files"][name]["len"], d["files"][name]["sha256"]), name
    return d


def check_pinned_binned():
    """index_cases.build_index / query against the reference CLI's recorded results."""
    d, files = pinned(), pinned_files()
    assert len(d["index_cases"]) == 3 * len(files)
    thrown = 0
    for c in d["index_cases"]:
        st, idx, _ = X.build_index(files[c["file"]], c["bin"])
        assert (st == OK) == (c["rc"] == 0), c
        assert (len(idx), X.sha(idx)) == (c["index_len"], c["index_sha256"]), c
        thrown += c["rc"] != 0
    assert thrown >= 3 * 17   # the nine bad POS spellings and the eight throwing INFO files
    assert len(d["binned_query_cases"]) >= 20
    for c in d["binned_query_cases"]:
        v = files[c["file"]]
        st, out = X.query(v, X.build_index(v, c["bin"])[1], c["region"])
        assert X.check_query_case(c, st, out), (c, st, len(out))


def check_pinned_sparse():
    """sparse_index_cases.create / query / gap_analysis against the reference CLI's recorded results."""
    d, files = pinned(), pinned_files()
    assert len(d["create_cases"]) == len(files) and len(d["gap_cases"]) == len(files) - len(PINNED_NO_GAP)
    for c in d["create_cases"]:
        st, slots, _, sf = SX.create(files[c["file"]])
        assert (st == OK) == (c["rc"] == 0) and sf == c["seek_failed"], c
        assert (SX.apparent_size(slots), len(slots), SX.slots_digest(slots)) == (c["size"], c["n_slots"], c["slots_sha256"]), c
    assert sum(c["seek_failed"] for c in d["create_cases"]) >= 2 and sum(c["rc"] != 0 for c in d["create_cases"]) >= 17
    assert len(d["sparse_query_cases"]) >= 20
    for c in d["sparse_query_cases"]:
        v = files[c["file"]]
        st, out = SX.query(v, SX.create(v)[1], c["region"])
        assert X.check_query_case(c, st, out), (c, st, len(out))
    for c in d["gap_cases"]:
        st, txt, _ = SX.gap_analysis(files[c["file"]])
        if c["rc"] == 0:
            assert st == OK and (len(txt), X.sha(txt)) == (c["txt_len"], c["txt_sha256"]), c
        else:   # the reference aborts: its text is the part written out before, a prefix of the lines before the record
            assert st == E_FORMAT and X.sha(txt[:c["txt_len"]]) == c["txt_sha256"], c
    assert sum(c["rc"] == 0 and c["txt_len"] > 0 for c in d["gap_cases"]) >= 30
