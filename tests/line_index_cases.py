"""The line index (csrc/vcfc_ingest.hip) against a plain line split: the plain
statement, the hop walk's universal property, the host's hints restated, and
families of hand-built inputs aimed at the index's constants -- SEG 16384,
WIN 1024, NL_SLOT 128, GW 256, LINE's window of 1 / 2 / 4 rows, the 124-byte
TAB check, GUESS_MIN 512, GUESS_LEAD 160, jf >= 64, HOP_K 3, HOP_TRUST 8 and
S_hint >= 32.  Shared by the emulator tests (test_line_index_emu.py) and the
GPU tests (test_gpu_line_index.py), as decode_cases.py and encode_cases.py.

A case is (name, buf, S, expectation).  The expectation is a dict:
  missing   f(cfg) -> the true line ends the hop index does not record under
            that configuration (the `traps` family only; absent: none, the
            tables equal plain_index exactly)
  cfg       the configuration the step counts below are stated for
  steps     {step name: exact count} of the walkers' steps (the emulator's
            VCFC_DIAG_HOP_STEP counters) under `cfg`
  at_least  {step name: lower bound} likewise
A configuration is a dict: S_hint, hop_walkers, learn, len_hint, cands."""
import random

from hop_cases import hop_trap_file, law2_like

SEG, WIN, NL_SLOT, GW = 16384, 1024, 128, 256
GUESS_MIN, GUESS_LEAD, HOP_K, HOP_TRUST = 512, 160, 3, 8
TABLES = ("line_off", "line_len", "line_no", "pass_off", "pass_len", "pass_no", "pass_before")
STEPS = ("LINE_FIRST", "LINE_CHECK", "VERIFY_HIT", "VERIFY_MISS", "FIND", "TRY_HIT", "TRY_MISS", "LEARN",
         "GUESS_TAKEN", "GUESS_FAIL", "TRUST_ZERO")


# ---------------------------------------------------------------------------
# the plain statement

def true_ends(buf):
    """Offsets of every '\\n' of buf."""
    out, p = [], buf.find(b"\n")
    while p >= 0:
        out.append(p)
        p = buf.find(b"\n", p + 1)
    return out


def index_of_ends(buf, ends):
    """counts and the seven tables of VcfcLineIndex for the lines that end at
    `ends` (increasing, the last one len(buf) - 1): a data line's first byte is
    not '#' and it is not empty, a pass line's first byte is '#', an empty
    line is counted in the line numbers and sits in no table; pass_before is
    the number of data lines before the pass line."""
    t = {k: [] for k in TABLES}
    s = 0
    for no, e in enumerate(ends):
        if e > s and buf[s] != 0x23:
            t["line_off"].append(s); t["line_len"].append(e - s); t["line_no"].append(no)
        elif e > s:
            t["pass_off"].append(s); t["pass_len"].append(e - s); t["pass_no"].append(no)
            t["pass_before"].append(len(t["line_off"]))
        s = e + 1
    t["counts"] = [len(ends), len(t["line_off"]), len(t["pass_off"]), 0]
    t["ends"] = list(ends)
    return t


def plain_index(buf):
    """The index of buf (its last byte '\\n') by a split on b"\\n"."""
    assert buf.endswith(b"\n")
    ends, p = [], -1
    for ln in buf[:-1].split(b"\n"):
        p += len(ln) + 1
        ends.append(p)
    assert ends[-1] == len(buf) - 1
    return index_of_ends(buf, ends)


def tiles(buf, ends):
    """What holds of the ends the hop walk records on any input under any
    configuration: strictly increasing, each a real '\\n', the last n - 1."""
    assert len(ends) > 0 and ends[-1] == len(buf) - 1, (len(ends), ends[-1:], len(buf))
    prev = -1
    for e in ends:
        assert e > prev and e < len(buf) and buf[e] == 0x0A, (prev, e)
        prev = e


# ---------------------------------------------------------------------------
# the host's hints (vcfc_ingest_driver.h), restated: compress_device computes
# them over the file's first 64 KiB

def _data_lines_after_chrom(p):
    """(start, end) of the complete non-empty, non-'#' lines after the first
    line that begins "#CHROM\\t"."""
    q, in_data = 0, False
    while q < len(p):
        end = p.find(b"\n", q)
        if end < 0:
            return
        if not in_data:
            in_data = p[q:q + 7] == b"#CHROM\t"
        elif end > q and p[q] != 0x23:
            yield q, end
        q = end + 1


def _ninth_tab(p, q, end):
    """(the byte after the 9th TAB of p[q, end) or where the scan stopped, TABs seen)"""
    t, tabs = q, 0
    while t < end and tabs < 9:
        tabs += p[t] == 0x09
        t += 1
    return t, tabs


def first_data_line_len(p):
    for q, end in _data_lines_after_chrom(p):
        return end + 1 - q if end + 1 - q < (1 << 30) else 0
    return 0


def data_lines_irregular(p, S):
    for q, end in _data_lines_after_chrom(p):
        k, _ = _ninth_tab(p, q, end)
        if end - k != 4 * S - 1:
            return True
    return False


def learn_candidates(p, S):
    """(g[3], sig[3][16]): up to three distinct region lengths G != 4 S - 1,
    G >= 255, each with the 16 16-bit TAB masks of the 256 bytes ending at
    that line's '\\n'."""
    g, sig = [0, 0, 0], [[0] * 16 for _ in range(3)]
    k = 0
    for q, end in _data_lines_after_chrom(p):
        if k == 3:
            break
        t, tabs = _ninth_tab(p, q, end)
        G = end - t
        if tabs == 9 and G != 4 * S - 1 and 255 <= G < (1 << 31) and G != g[0] and G != g[1]:
            g0 = end + 1 - 256
            for wl in range(16):
                sig[k][wl] = sum((p[g0 + 16 * wl + j] == 0x09) << j for j in range(16))
            g[k] = G
            k += 1
    return g, sig


def configs(buf, S, walkers=(0, 1, 4)):
    """The configurations of a hop family's case: the scan (S_hint 0), and
    with S_hint = S the GUESS walkers (learn False) over hop_walkers x
    len_hint in {0, the first data line's}, the TRY / LEARN walkers (learn
    True) over hop_walkers x cands in {none, the restated learn_candidates}.
    (The kernel launch hands the learning walkers no len_hint, so len_hint is
    not crossed with learn True: it could not change anything.)"""
    head = buf[:65536]
    fl, cands = first_data_line_len(head), learn_candidates(head, S)
    out = [dict(S_hint=0, hop_walkers=0, learn=True, len_hint=0, cands=None)]
    for w in walkers:
        for lh in (0, fl):
            out.append(dict(S_hint=S, hop_walkers=w, learn=False, len_hint=lh, cands=None))
        for c in (None, cands):
            out.append(dict(S_hint=S, hop_walkers=w, learn=True, len_hint=0, cands=c))
    return out


def cfg_id(c):
    return "S%d-w%d-%s-lh%d-%s" % (c["S_hint"], c["hop_walkers"], "learn" if c["learn"] else "guess", c["len_hint"],
                                  "cands" if c["cands"] else "nocands")


# ---------------------------------------------------------------------------
# rows

T3 = [b"0|0", b"0|1", b"1|0", b"1|1", b"0|2"]
MIN_PL = 19   # b"1\t7\tr\tA\tC\t5\tP\t.\tGT\t"


def prefix(pl, pos=7, fmt=b"GT"):
    """Nine fields and their TABs in exactly pl bytes: the 9th TAB is byte
    pl - 1 of the line."""
    base = b"\t".join([b"1", b"%d" % pos, b"r", b"A", b"C", b"5", b"P", b".", fmt]) + b"\t"
    assert pl >= len(base), (pl, len(base))
    out = base.replace(b"\tr\t", b"\tr" + b"s" * (pl - len(base)) + b"\t", 1)
    assert len(out) == pl and out.count(b"\t") == 9 and out[pl - 1] == 0x09
    return out


def row3(rnd, pl, S, pos=7):
    """A row of S 3-byte tokens behind a prefix of pl bytes (no '\\n')."""
    r = prefix(pl, pos) + b"\t".join(rnd.choice(T3) for _ in range(S))
    assert len(r) == pl + 4 * S - 1
    return r


def row_len(rnd, length, S, pos=7):
    """The same, `length` bytes with its '\\n'."""
    return row3(rnd, length - 4 * S, S, pos)


def region(rnd, S, G, front=True):
    """S tokens, none of 3 bytes' width only: G bytes with their TABs, made of
    3-, 4-, 5- and 6-byte tokens ("a|b", "a|b:d" ...); front: the wide tokens
    first, else last (another TAB mask for the same G)."""
    extra = G - (4 * S - 1)
    assert extra >= 0 and extra <= 3 * S, (S, G)
    w = [3] * S
    i = 0
    while extra > 0:
        d = min(3, extra)
        w[i if front else S - 1 - i] += d
        extra -= d
        i += 1
    toks = [(b"%d|%d" % (rnd.randrange(2), rnd.randrange(2)) + b":12"[:k - 3]) for k in w]
    out = b"\t".join(toks)
    assert len(out) == G
    return out


def rowG(rnd, pl, S, G, front=True, pos=7):
    return prefix(pl, pos, b"GT:DP") + region(rnd, S, G, front)


def rows_to(rnd, lines, n, target, S):
    """Rows of about 1000 bytes appended to `lines` (n bytes so far) until
    they hold exactly `target` bytes; returns target."""
    assert target - n >= 4 * S + MIN_PL
    while target - n > 2100:
        ln = 4 * S + GR_PL + rnd.randrange(-20, 21)
        lines.append(row_len(rnd, ln, S, pos=len(lines)))
        n += ln
    r = target - n
    for ln in ([r // 2, r - r // 2] if r >= 2 * (4 * S + MIN_PL) else [r]):
        lines.append(row_len(rnd, ln, S, pos=len(lines)))
    return target


def header(S):
    cols = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + b"".join(b"\tS%d" % i for i in range(S))
    return [b"##fileformat=VCFv4.2", cols]


def join(lines):
    return b"\n".join(lines) + b"\n"


# ---------------------------------------------------------------------------
# LINE, modelled: which step finds each line of a file walked by one walker
# without learned candidates, every data row standing alone (a '#' or empty
# line before it, so that no GUESS round takes it).  The state is the kernel's:
# pl (the last prefix length seen) and rows (256-byte rows of the next first
# window: 1 when pl + 96 <= 256, 2 when <= 512, else 4).

def line_model(buf, S):
    n = len(buf)
    c = dict.fromkeys(STEPS, 0)
    pl, rows, p = 0, 4, 0
    for e in true_ends(buf):
        ln = e + 1 - p
        while True:
            mw = 256 * rows
            if ln <= mw:
                c["LINE_FIRST"] += 1
                break
            if buf[p] == 0x23:
                c["FIND"] += 1
                break
            t, tabs = _ninth_tab(buf, p, min(e, p + mw))
            if tabs < 9:
                if rows < 4:
                    rows = 4
                    continue
                c["FIND"] += 1
                break
            x = p + pl + 4 * S - 1
            g0 = max(x - 190, 0)
            pl = t - p
            rows = 1 if pl + 96 <= 256 else 2 if pl + 96 <= 512 else 4
            pe = t + 4 * S - 1               # the predicted end
            ok = pe == e and all(buf[pe - 4 * i] == 0x09 for i in range(1, 32))
            if pe >= n:
                c["FIND"] += 1
            elif g0 + 256 <= n and g0 + 124 <= pe < g0 + 256:
                c["LINE_CHECK" if ok else "FIND"] += 1
            elif ok:
                c["VERIFY_HIT"] += 1
            else:
                c["VERIFY_MISS"] += 1
                c["FIND"] += 1
            assert pe == e or pe >= n or buf[pe] != 0x0A, "a trap: the model is for exact files"
            break
        p = e + 1
    return {k: v for k, v in c.items() if k in ("LINE_FIRST", "LINE_CHECK", "VERIFY_HIT", "VERIFY_MISS", "FIND")}


ONE = dict(hop_walkers=1, learn=True, len_hint=0, cands=None)   # one walker, LINE / VERIFY / FIND only


def line_expect(buf, S, also_learn=True):
    """The expectation of a file of rows standing alone: line_model's counts,
    for one GUESS walker (the separators keep GUESS out) and, where every row
    searched for is too short to be learned from, one learning walker."""
    also = [dict(ONE, S_hint=S)] if also_learn else []
    return dict(cfg=dict(ONE, S_hint=S, learn=False), steps=line_model(buf, S), also=also)


# ---------------------------------------------------------------------------
# scan path (S_hint = 0)

SWAR_SET = bytes([0x0A, 0x8A, 0x0B, 0x09, 0x89, 0x00, 0xFF, 0x7F, 0x80, 0x1A])
SWAR_N = (1, 15, 16, 17, 1023, 1024, 1025, 16383, 16384, 16385, 32768, 40000)


def swar_bytes(n):
    """n bytes drawn from the values next to '\\n' in every bit a SWAR byte
    test can get wrong (bit 7 set, one bit off, the borrow and carry
    neighbours); the last one '\\n'."""
    rnd = random.Random(n)
    buf = bytes(rnd.choice(SWAR_SET) for _ in range(n - 1)) + b"\n"
    assert len(buf) == n and (n < 64 or all(bytes([v]) in buf for v in SWAR_SET))
    return "swar_bytes-%d" % n, buf, 0, {}


def _segment(rnd, k, size=SEG, tail=0, kinds=(0, 1, 2)):
    """`size` bytes holding exactly k '\\n': data, '#' and empty lines in turn,
    then `tail` bytes of a line that goes on in the next segment."""
    lines = []
    for i in range(k):
        kind = kinds[i % len(kinds)]
        lines.append(b"" if kind == 2 else (b"#p%d" if kind == 1 else b"d%d") % i)
    used = sum(len(x) + 1 for x in lines) + tail
    assert used <= size, (k, used, size)
    j = next((i for i in range(k // 2, k) if lines[i][:1] == b"d"), None)
    if j is None:
        j = next(i for i in range(k) if lines[i][:1] == b"d")
    lines[j] += b"." * (size - used)
    out = b"".join(x + b"\n" for x in lines) + b"t" * tail
    assert len(out) == size and out.count(b"\n") == k
    return out


SLOT_VARIANTS = ("first", "middle", "bare", "partial_last", "two_in_wave_and_across_waves")


def slot_edge(variant):
    """Segments with 127, 128, 129 and 130 line ends around k_nl_place's
    `c <= NL_SLOT`, and one of 16384 bare '\\n'; data, '#' and empty lines
    mixed, lines running across the segment ends."""
    rnd = random.Random(variant)
    if variant == "first":
        segs = [(130, 7), (5, 0), (127, 3), (128, 0), (129, 9), (128, 1)]
    elif variant == "middle":
        segs = [(3, 5), (128, 2), (129, 0), (127, 1), (130, 4), (2, 0)]
    elif variant == "bare":
        segs = [(5, 3), (SEG, 0), (128, 5), (SEG, 0), (4, 0)]
    elif variant == "partial_last":
        segs = [(5, 2), (127, 0), (128, 6)]
    else:
        segs = [(2, 1)] * 66
        segs[3], segs[40], segs[63], segs[64] = (129, 4), (300, 0), (130, 2), (129, 3)
    parts = [b"\n" * SEG if k == SEG else _segment(rnd, k, SEG, tail) for k, tail in segs]
    if variant == "partial_last":
        parts.append(_segment(rnd, 200, 8000))
    elif variant != "bare":
        parts.append(_segment(rnd, 3, 777))
    buf = b"".join(parts)
    if not buf.endswith(b"\n"):
        buf += b"\n"
    for i, (k, _) in enumerate(segs):
        assert buf[i * SEG:(i + 1) * SEG].count(b"\n") == k
    return "slot_edge-" + variant, buf, 0, {}


KIND_VARIANTS = ("starts_empty", "starts_pass", "starts_data", "segment_first_byte", "empty_run", "pass_places")


def kind_edge(variant):
    """The kind of a line is its first byte: files beginning with each kind,
    a line whose first byte is a segment's first, empty lines across a segment
    end, '#' lines before, between and after the data lines (pass_before and
    the counts the last lane writes)."""
    if variant == "starts_empty":
        buf = b"\n\n#a\nd1\n\nd2\n"
    elif variant == "starts_pass":
        buf = b"#a\n#b\nd1\n"
    elif variant == "starts_data":
        buf = b"d0\n#a\n\n"
    elif variant == "segment_first_byte":
        # a line end at SEG - 1; the next segment's first byte a data, '#' and '\n' byte in turn
        parts = []
        for first in (b"dx\n", b"#x\n", b"\n", b"dx\n"):
            parts.append(first + b"##k\n" + b"y" * (SEG - len(first) - 5) + b"\n")
        buf = b"".join(parts) + b"#z\n"
        for i in range(1, 5):
            assert buf[i * SEG - 1] == 0x0A and len(parts[i - 1]) == SEG, (i, len(parts[i - 1]))
        assert buf[SEG:SEG + 1] == b"#" and buf[2 * SEG:2 * SEG + 1] == b"\n" and buf[3 * SEG:3 * SEG + 1] == b"d"
    elif variant == "empty_run":
        buf = b"d" * (SEG - 7) + b"\n" * 13 + b"#q\n" + b"e" * 50 + b"\n"
        assert buf[SEG - 7:SEG + 6] == b"\n" * 13
    else:
        buf = b"##a\n#b\n" + b"d1\nd2\n#mid1\n\n#mid2\nd3\n" * 3 + b"d4\n#tail1\n\n#tail2\n"
    return "kind_edge-" + variant, buf, 0, {}


# ---------------------------------------------------------------------------
# hop path

def alone(rows):
    """Each row behind a '#' or an empty line in turn: GUESS takes none of them."""
    out = []
    for i, r in enumerate(rows):
        out += [b"#s%d" % i if i % 2 == 0 else b"", r]
    return out


def s_gate(S):
    """The sample counts around `S_hint >= 32`.  Rows with the shortest legal
    prefix (19 bytes) end inside LINE's first window.  A row is predicted only
    when it is longer than the window, and the window shrinks only after a
    predicted row, so at S = 32 (rows of pl + 128 bytes) the predicted rows
    have prefixes of 897 .. 1024 bytes behind a 1 KiB window; there the 31-TAB
    check reaches back to byte gt0 + 3, the TAB after the first token.  No
    header: the first line is a data line at byte 0, where x = pl + 4 S - 1
    < 190 and g0 clamps to 0."""
    rnd = random.Random(S)
    pls = (900, 950, 1015, 897, 1024, 940)
    rows = [row3(rnd, MIN_PL, S), row3(rnd, MIN_PL, S)] + alone([row3(rnd, pl, S) for pl in pls])
    buf = join(rows)
    assert buf[0:1] == b"1" and MIN_PL + 4 * S - 1 < 190
    if S == 32:
        r = rows[-1]
        gt, e = 940, 940 + 127
        assert len(r) == e and e - 124 == gt + 3 and r[gt + 3] == 0x09 and r[gt + 2] != 0x09
    exp = line_expect(buf, S) if S >= 32 else {}
    if S >= 32:
        # from pl 0: VERIFY; +50, +65: in the round; -118, +127, -84: VERIFY
        assert exp["steps"]["LINE_CHECK"] == 2 and exp["steps"]["VERIFY_HIT"] == 4 and exp["steps"]["FIND"] == 0, exp
    return "s_gate-%d" % S, buf, S, exp


def s_gate_tiny(S=32):
    """One row shorter than the guess window: n < GW, no window is valid."""
    rnd = random.Random(5)
    buf = join([row3(rnd, MIN_PL, S)])
    assert len(buf) < GW
    return "s_gate-tiny", buf, S, line_expect(buf, S)


LW_S = 300


def line_window(variant):
    """LINE's first window of 1, 2 or 4 256-byte rows (the last prefix length
    + 96, rounded up): the 9th TAB at line byte 254 .. 257 behind a 1-row
    window, 510 .. 513 behind 2 rows, 1022 .. 1024 behind 4 (1024: none in
    1 KiB, FIND); pl + 96 on both sides of 256 and 512, told apart by a next
    row that ends inside the larger window only; every row alone."""
    rnd = random.Random(variant)
    if variant == "tab9":
        S, pls = LW_S, []
        for prev, t9s in ((100, (254, 255, 256, 257)), (300, (510, 511, 512, 513)), (600, (1022, 1023, 1024))):
            for t9 in t9s:
                pls += [prev, t9 + 1]
        rows = [row3(rnd, pl, S) for pl in pls]
        for r, pl in zip(rows, pls):
            assert r[pl - 1] == 0x09 and r[:pl - 1].count(b"\t") == 8   # the 9th TAB is byte pl - 1 of its line
        lines = header(S) + alone(rows)
    elif variant == "rows_choice":
        # After pl = 160 (pl + 96 = 256: 1 row) a row of 400 bytes (64 samples:
        # its predicted end is wrong) is not seen to end in the window and is
        # searched for; after pl = 161 (2 rows) it ends in the first window.
        # Likewise 416 / 417 and a row of 700 bytes.
        S = LW_S
        short = lambda ln, pl: row3(rnd, pl, (ln - pl) // 4)
        rows = [row3(rnd, 100, S), row3(rnd, 160, S), short(400, 144), row3(rnd, 161, S), short(400, 144),
                row3(rnd, 300, S), row3(rnd, 416, S), short(700, 444), row3(rnd, 417, S), short(700, 444),
                row3(rnd, 100, S)]
        assert [len(rows[i]) + 1 for i in (2, 4, 7, 9)] == [400, 400, 700, 700]
        lines = header(S) + alone(rows)
    else:
        # a long-prefix row straight after a short-prefix row (1 row, no 9th
        # TAB, the line again with 1 KiB); a prefix over 1 KiB (FIND)
        S = LW_S
        pls = [30, 900, 30, 1500, 40, 700, 1025, 2000, 19]
        lines = header(S) + alone([row3(rnd, pl, S) for pl in pls])
    buf = join(lines)
    exp = line_expect(buf, S, also_learn=variant != "rows_choice")
    if variant == "tab9":
        assert exp["steps"]["FIND"] == 2      # the "#CHROM" line and the row whose 9th TAB is byte 1024
    if variant == "rows_choice":
        # found in the first window: "##fileformat", the 11 lines between the rows, the two short
        # rows behind the larger windows; searched for: "#CHROM", the two behind the smaller ones
        assert exp["steps"]["LINE_FIRST"] == 1 + 11 + 2 and exp["steps"]["FIND"] == 1 + 2, exp
    if variant == "long_prefix":
        assert exp["steps"]["FIND"] == 1 + 3
    return "line_window-" + variant, buf, S, exp


GWE_DELTAS = (-67, -66, -65, 64, 65, 66)


def guess_window_edge(delta, last):
    """LINE's 256-byte guess window starts at g0 = x - 190, x the end if the
    prefix were as long as the last one: a prefix `delta` bytes longer puts
    the real end at window byte 190 + delta -- 123 (before the 124 bytes the
    check needs: VERIFY), 124, 125, 254, 255 (checked in the round), 256 (past
    the window: VERIFY).  last: "" the row inside the file; "row" it is the
    file's last line (g0 + GW > n unless the end is window byte 255); "short"
    the last line has fewer samples, so its predicted end is past n."""
    S, base = LW_S, 120
    rnd = random.Random(delta)
    rows = [row3(rnd, base, S), row3(rnd, base, S), row3(rnd, base + delta, S)]
    if last == "":
        rows += [row3(rnd, base, S)]
    elif last == "short":
        rows += [row3(rnd, base + delta, S), row3(rnd, base, S - 10)]
    tail = [b"#" + b"t" * 300] if last == "" else []          # (so that the last row's window lies inside the file)
    buf = join(header(S) + alone(rows) + tail)
    exp = line_expect(buf, S, also_learn=last != "short")
    # the row `delta` after a row of `base`: in the round or by VERIFY, as the window's edges say
    inround = 124 <= 190 + delta < 256
    if last == "":
        # rows: VERIFY (pl 0 -> 120), check (0), `delta`, and back (-delta)
        back = 124 <= 190 - delta < 256
        assert exp["steps"]["LINE_CHECK"] == 1 + inround + back and exp["steps"]["VERIFY_HIT"] == 1 + (not inround) + (not back), exp
    elif last == "row":
        fits = 190 + delta == 255     # g0 + GW <= n only then
        assert exp["steps"]["LINE_CHECK"] == 1 + fits and exp["steps"]["VERIFY_HIT"] == 1 + (not fits), exp
    else:
        # checks: the second row, `delta`, and the row of the same prefix after it
        assert exp["steps"]["LINE_CHECK"] == 2 + inround and exp["steps"]["FIND"] == 2, exp
    return "guess_window_edge%+d-%s" % (delta, last or "inside"), buf, S, exp


GR_S, GR_PL = 200, 200
GR_L = GR_PL + 4 * GR_S         # 1000 bytes a row with its '\n'
GR_D = (-97, -96, -95, 94, 95, 96)
GUESS1 = dict(S_hint=GR_S, hop_walkers=1, learn=False, len_hint=0, cands=None)


def guess_rounds(variant):
    """GUESS: after a row of L bytes found by LINE, one 256-byte window from
    160 bytes before each guessed end.  A next row d bytes longer than L ends
    at window byte jf = 160 + d: 63 (refused), 64, 65, 254, 255 (taken), 256
    (not in the window).  Groups of: a '#' line, row A (L bytes, by LINE), row
    B (L + d), then N -- a '#' line, an empty line, or a data row made to end
    at byte 160 of its own window.  B's '\\n' at window byte 254 / 255 puts N's
    first byte at 255 (seen) / 256 (not seen: the next round's head byte)."""
    rnd = random.Random(variant)
    if variant == "edges":
        lines, taken, fail = header(GR_S), 0, 0
        for d in GR_D:
            for kind in ("pass", "empty", "data"):
                jf = 160 + d
                b_ok = 64 <= jf <= 255
                if kind == "empty" and jf != 255:
                    b_ok = False                     # "\n\n" inside the window: two '\n', refused
                lines += [b"#g%d%s" % (d, kind.encode()) + b"." * 300, row_len(rnd, GR_L, GR_S), row_len(rnd, GR_L + d, GR_S)]
                taken += b_ok
                fail += not b_ok
                if kind == "data":
                    # N at byte 160 of its window: B taken and N seen (the same round, the window
                    # at 2 L): L - d; B taken, N not seen (the next round, L the mean of A and B,
                    # L + 48 for d = 95); B by LINE (the next streak's L is B's length)
                    ln = GR_L - d if b_ok and jf < 255 else GR_L + 48 if b_ok else GR_L + d
                    lines.append(row_len(rnd, ln, GR_S))
                    taken += 1
                else:
                    lines.append(b"#n" + b"." * 300 if kind == "pass" else b"")   # ('#' lines end past the window)
        lines += [b"#end" + b"." * 300]
        buf = join(lines)
        exp = dict(cfg=GUESS1, steps=dict(GUESS_TAKEN=taken, GUESS_FAIL=fail))
    elif variant == "streak":
        # rows of 1000 +- 30 bytes and no other lines: streaks across every walker's span end; a
        # row's '\n' at byte 32767 (hi - 1 of the first 2-segment span: the next start is hi) and
        # one at 65535 + 700 (a guessed end past hi)
        lines = header(GR_S)
        n = len(join(lines))
        for target in (2 * SEG, 4 * SEG + 700, 150_000):
            n = rows_to(rnd, lines, n, target, GR_S)
        buf = join(lines)
        assert buf[2 * SEG - 1] == 0x0A and buf[4 * SEG + 699] == 0x0A
        exp = dict(cfg=GUESS1, at_least=dict(GUESS_TAKEN=120))
    elif variant == "shrink_grow":
        # rows shrinking by 60 bytes from 1400 to the shortest the prefix allows, then growing by 60
        lens = list(range(1400, GR_S * 4 + MIN_PL, -60)) + list(range(GR_S * 4 + MIN_PL + 5, 1500, 60))
        buf = join(header(GR_S) + [row_len(rnd, ln, GR_S) for ln in lens])
        exp = dict(cfg=GUESS1, at_least=dict(GUESS_TAKEN=8, GUESS_FAIL=8))
    else:
        # short rows (S = 100: 419 + pl bytes) on both sides of GUESS_MIN
        S = 100
        lens = [511, 511, 512, 512, 513, 513, 511, 600, 600, 600, 600, 600, 600]
        buf = join(header(S) + [row_len(rnd, ln, S) for ln in lens])
        # every row ends in LINE's first window (1 KiB).  The two rows of 511 bytes start no GUESS,
        # the first of 512 does: the next four are taken (the ends 0, 1, 2, 1 bytes past the
        # guesses), L stays 512; the first 600 is taken (window byte 248), the second is not in
        # its window and goes to LINE, the last four are taken from L = 600
        exp = dict(cfg=dict(GUESS1, S_hint=S), steps=dict(LINE_FIRST=2 + 4, GUESS_TAKEN=4 + 1 + 4, GUESS_FAIL=1))
        return "guess_rounds-" + variant, buf, S, exp
    return "guess_rounds-" + variant, buf, GR_S, exp


GR_VARIANTS = ("edges", "streak", "shrink_grow", "guess_min")
GR_LEN_HINTS = (GR_L, 700, 511, 512, (1 << 30) - 1)   # the streak file's first guess: right, wrong, around GUESS_MIN, the largest

SPAN_VARIANTS = ("end-1", "end+0", "end+1", "pass", "empties", "row", "long_row", "long_row_at_hi", "multiple")
SPAN_WALKERS = (0, 1, 2, 3)
SPAN_EDGES = (2 * SEG, 3 * SEG, 4 * SEG, 6 * SEG)   # the span ends of 7 segments under 4, 2 and 3 walkers


def span_edge(variant):
    """About 112 KiB (7 segments) under hop_walkers 0 (4 spans of 2 segments),
    1, 2 (4 + 3 segments) and 3 (3 + 3 + 1): at each span end hi a line end at
    hi - 1, hi and hi + 1, a '#' line, a run of empty lines and a data row
    across it; a row longer than a span (36 KB: one walker without a start,
    segments without ends); a file that is a whole number of spans."""
    rnd = random.Random(variant)
    S = 200
    if variant == "long_row":
        S = 9000
        lines = [b"##long"] + [row3(rnd, 40 + i, S, pos=i) for i in range(3)] + [b"#t"]
        buf = join(lines)
        assert 108_000 < len(buf) < 7 * SEG and len(lines[1]) > 2 * SEG
        return "span_edge-long_row", buf, S, dict(cfg=dict(ONE, S_hint=S), at_least=dict(VERIFY_HIT=1))
    if variant == "long_row_at_hi":
        # a row over a whole span whose '\n' is the span end's own byte hi (64 KiB under 4 walkers
        # a wave of 2 segments each): k_nl_hop_start finds no end before hi for that walker
        S = 16370
        lines = [b"##long", row3(rnd, 50, S), row3(rnd, 60, S, pos=8), b"#t"]
        buf = join(lines)
        assert buf[4 * SEG] == 0x0A and buf.find(b"\n", 7) == 4 * SEG and len(buf) <= 9 * SEG
        return "span_edge-long_row_at_hi", buf, S, dict(cfg=dict(ONE, S_hint=S), at_least=dict(VERIFY_HIT=1))
    size = 6 * SEG if variant == "multiple" else 7 * SEG - 500
    lines = header(S)
    n = len(join(lines))
    for edge in [x for x in SPAN_EDGES if x < size]:
        if variant.startswith("end"):
            n = rows_to(rnd, lines, n, edge + int(variant[3:]) + 1, S)   # a row's '\n' at edge + k
        elif variant in ("pass", "empties"):
            n = rows_to(rnd, lines, n, edge - 2, S)                      # a row's '\n' 3 bytes before the edge ...
            mid = b"#straddle" if variant == "pass" else b"\n\n\n\n"
            lines.append(mid)                                            # ... and this line (these 5) across it
            n += len(mid) + 1
        else:
            n = rows_to(rnd, lines, n, edge - 500, S)
            n = rows_to(rnd, lines, n, edge + 500, S)                    # a row across the edge
    n = rows_to(rnd, lines, n, size, S)
    buf = join(lines)
    assert len(buf) == size
    if variant.startswith("end"):
        for x in SPAN_EDGES:
            assert buf[x + int(variant[3:])] == 0x0A
    if variant == "row":
        for x in SPAN_EDGES:
            assert b"\n" not in buf[x - 400:x + 400]
    if variant == "pass":
        for x in SPAN_EDGES:
            assert buf[x - 3:x + 1] == b"\n#st"
    if variant == "empties":
        for x in SPAN_EDGES:
            assert buf[x - 3:x + 2] == b"\n" * 5
    if variant == "multiple":
        assert len(buf) % (2 * SEG) == 0 and len(buf) % (3 * SEG) == 0
    return "span_edge-" + variant, buf, S, dict(cfg=GUESS1, at_least=dict(GUESS_TAKEN=50))


TL_S = 60    # 4 S - 1 = 239; a region of 3- to 6-byte tokens: up to 419
TL_PL = 800
TRY1 = dict(S_hint=TL_S, hop_walkers=1, learn=True, len_hint=0, cands=None)
TL_VARIANTS = ("G254", "G255", "G256", "kinds3", "kinds4", "kinds5", "kinds_in_turn", "same_G", "trust", "end_past_n", "law2")


def try_learn(variant):
    """TRY / LEARN: rows whose genotype region is G != 4 S - 1 bytes.  A region
    is learned from the 256 bytes ending at its '\\n' (G >= 255: G = 254 is
    never learned, every such row goes to FIND), HOP_K = 3 candidates are kept
    round robin, and a walker stops trying after HOP_TRUST misses more than
    hits.  Prefixes of 800 bytes: a row must be longer than LINE's 1 KiB first
    window to be predicted at all."""
    rnd = random.Random(variant)
    S = TL_S
    exp = dict(cfg=TRY1)
    if variant in ("G254", "G255", "G256"):
        G = int(variant[1:])
        rows = [rowG(rnd, TL_PL + i, S, G, pos=i) for i in range(10)]
        lines = header(S) + rows
        if G == 254:
            exp["steps"] = dict(FIND=10, LEARN=0, TRY_HIT=0, TRY_MISS=0)     # every row
        else:
            exp["steps"] = dict(FIND=1, LEARN=1, TRY_HIT=9, TRY_MISS=0)      # the first row
        # with the host's candidates no row is searched for
        exp["seeded"] = dict(FIND=10, LEARN=0, TRY_HIT=0) if G == 254 else dict(FIND=0, LEARN=0, TRY_HIT=10)
    elif variant in ("kinds3", "kinds4", "kinds5"):
        # k kinds in blocks of three rows, twice round.  The first row of a block is searched for
        # and learned (round robin over HOP_K = 3 places: with 4 or 5 kinds the kind that comes
        # again was replaced), the other two hit; a miss for every first row but the file's first.
        k = int(variant[5:])
        Gs = [260 + 30 * j for j in range(k)]
        lines = header(S) + [rowG(rnd, TL_PL + (i % 7), S, Gs[(i // 3) % k], pos=i) for i in range(6 * k)]
        if k == 3:
            exp["steps"] = dict(LEARN=3, FIND=3, TRY_MISS=2, TRY_HIT=15, TRUST_ZERO=0)
        else:
            exp["steps"] = dict(LEARN=2 * k, FIND=2 * k, TRY_MISS=2 * k - 1, TRY_HIT=4 * k, TRUST_ZERO=0)
    elif variant == "kinds_in_turn":
        # 4 kinds one row each in turn: none is held when it comes again, the walker's credit
        # (HOP_TRUST = 8) runs out at the 9th row and it neither tries nor learns after that
        Gs = [260 + 30 * j for j in range(4)]
        lines = header(S) + [rowG(rnd, TL_PL + (i % 7), S, Gs[i % 4], pos=i) for i in range(24)]
        exp["steps"] = dict(LEARN=8, FIND=24, TRY_MISS=8, TRY_HIT=0, TRUST_ZERO=1)
    elif variant == "same_G":
        # two kinds of one region length, the wide tokens first / last: a TAB mask each; the second
        # is not learned (the length is held), so its rows miss and are searched for
        lines = header(S) + [rowG(rnd, TL_PL, S, 330, front=i % 2 == 0, pos=i) for i in range(12)]
        exp["steps"] = dict(LEARN=1, TRY_HIT=5, TRY_MISS=6, FIND=1 + 6)
    elif variant == "trust":
        # two kinds learned and hit, then 12 rows of lengths never seen twice (the walker's credit
        # runs out after 8), then the two kinds again: no longer tried
        kinds = [rowG(rnd, TL_PL, S, 300 + 40 * (i % 2), pos=i) for i in range(8)]
        odd = [rowG(rnd, TL_PL, S, 350 + 3 * i, pos=i) for i in range(12)]
        again = [rowG(rnd, TL_PL, S, 300 + 40 * (i % 2), pos=i) for i in range(6)]
        lines = header(S) + kinds + odd + again
        # (the second kind's first row misses too; the first 7 odd rows are still learned)
        exp["steps"] = dict(TRUST_ZERO=1, TRY_HIT=6, TRY_MISS=1 + 8, LEARN=2 + 7, FIND=2 + 12 + 6)
    elif variant == "end_past_n":
        # the last rows are shorter than every learned region: a candidate's end gt + G >= n
        lines = header(S) + [rowG(rnd, TL_PL, S, 410, pos=i) for i in range(5)] + [rowG(rnd, TL_PL, S, 250), rowG(rnd, TL_PL, S, 260)]
        exp["at_least"] = dict(TRY_HIT=4, TRY_MISS=1)
    else:
        buf = law2_like(rnd, 60, 300)
        return "try_learn-law2", buf, 300, dict(cfg=dict(TRY1, S_hint=300), at_least=dict(TRY_HIT=10, LEARN=2))
    return "try_learn-" + variant, join(lines), S, exp


# ---------------------------------------------------------------------------
# traps: the only inputs on which the hop index may differ from plain_index

TRAP_VARIANTS = ("tab", "escape", "var", "lines", "guess", "try")


def guess_trap_file(rnd, lead_rows=70):
    """Rows of 1000 bytes; then a short data row B1 and a row B2 that ends
    exactly where a row of 1000 bytes would, its '\\n' and the 15 TABs before it
    in place, B1's '\\n' before the guess window: GUESS takes B1 + B2 as one
    line.  lead_rows rows come first (over 64 KiB: compress_device's look at
    the first data lines finds them regular and chooses GUESS)."""
    S = GR_S
    b1 = row3(rnd, 30, 100)                    # 429 bytes + '\n'
    b2 = row3(rnd, 50, 130)                    # 569 bytes + '\n'
    assert len(b1) + 1 + len(b2) + 1 == GR_L and len(b2) + 1 > GUESS_LEAD + 1
    lines = header(S) + [row_len(rnd, GR_L, S, pos=i) for i in range(lead_rows)] + [b1, b2] + \
        [row_len(rnd, GR_L, S, pos=900 + i) for i in range(4)]
    buf = join(lines)
    at = len(join(lines[:2 + lead_rows])) + len(b1)
    assert buf[at] == 0x0A and buf[at + len(b2) + 1] == 0x0A
    return buf, S, at


def try_trap_file(rnd):
    """Rows of 300 6-byte tokens (G = 2099, learned); then a row T1 of 170
    such tokens (longer than LINE's first window, which would find its end)
    and a row T2 of 100 that ends where T1 would with 300, the last 256 bytes
    before its '\n' the learned TAB mask: T1's '\n' lies 910 bytes before that
    end, outside the window TRY reads, and T1 + T2 are one line."""
    S = 300
    wide = lambda k: b"\t".join(b"%d|%d:%d" % (rnd.randrange(2), rnd.randrange(2), rnd.randrange(10, 100)) for _ in range(k))
    row = lambda pl, k, pos: prefix(pl, pos, b"GT:DP") + wide(k)
    t1, t2 = row(40, 170, 500), row(210, 100, 501)
    G = 7 * S - 1
    assert len(t1) > WIN and len(t1) - 40 + 1 + len(t2) == G and G - (len(t1) - 40) > GW
    lines = header(S) + [row(40, S, i) for i in range(6)] + [t1, t2] + [row(40, S, 600 + i) for i in range(3)]
    buf = join(lines)
    at = len(join(lines[:8])) + len(t1)
    assert buf[at] == 0x0A and buf[at + len(t2) + 1] == 0x0A and buf[at + len(t2) + 1 - G - 1] == 0x09
    return buf, S, at


def traps(variant):
    """The files on which a guessed end is a real '\\n' with everything the
    walker checks in place, but lines end before it that it did not see.  The
    expectation names those ends per configuration; the hop result is the true
    ends minus exactly those (and tiles() holds)."""
    rnd = random.Random(variant)
    if variant == "guess":
        buf, S, at = guess_trap_file(rnd)
        return "traps-guess", buf, S, dict(missing=lambda c: [at] if c["S_hint"] and not c["learn"] else [])
    if variant == "try":
        buf, S, at = try_trap_file(rnd)
        return "traps-try", buf, S, dict(missing=lambda c: [at] if c["S_hint"] and c["learn"] else [])
    buf = hop_trap_file(variant, rnd)
    S = buf.split(b"\n")[1].count(b"\t") - 8
    ends = true_ends(buf)
    # lines: 2 header lines, 3 rows, A (line 5), [the lines between], B
    a = ends[5]
    gone = ends[5:8] if variant == "lines" else [a]
    assert buf[ends[4] + 1:ends[4] + 3] == b"1\t" and (variant != "lines" or buf[a + 1:a + 10] == b"##between")
    return "traps-" + variant, buf, S, dict(missing=lambda c: gone if c["S_hint"] else [])


# ---------------------------------------------------------------------------
# the registry: (family, name, builder[, hop_walkers]); a case is built when
# its test runs

def scan_registry():
    out = [("swar_bytes", "swar_bytes-%d" % n, lambda n=n: swar_bytes(n)) for n in SWAR_N]
    out += [("slot_edge", "slot_edge-" + v, lambda v=v: slot_edge(v)) for v in SLOT_VARIANTS]
    out += [("kind_edge", "kind_edge-" + v, lambda v=v: kind_edge(v)) for v in KIND_VARIANTS]
    return out


def hop_registry():
    """Every hop family but the traps."""
    W = (0, 1, 4)
    out = [("s_gate", "s_gate-%d" % S, lambda S=S: s_gate(S), W) for S in (31, 32, 33)]
    out.append(("s_gate", "s_gate-tiny", s_gate_tiny, W))
    out += [("line_window", "line_window-" + v, lambda v=v: line_window(v), W) for v in ("tab9", "rows_choice", "long_prefix")]
    out += [("guess_window_edge", "guess_window_edge%+d-%s" % (d, last or "inside"),
             lambda d=d, last=last: guess_window_edge(d, last), W) for d in GWE_DELTAS for last in ("", "row", "short")]
    out += [("guess_rounds", "guess_rounds-" + v, lambda v=v: guess_rounds(v), W) for v in GR_VARIANTS]
    out += [("span_edge", "span_edge-" + v, lambda v=v: span_edge(v), SPAN_WALKERS) for v in SPAN_VARIANTS]
    out += [("try_learn", "try_learn-" + v, lambda v=v: try_learn(v), W) for v in TL_VARIANTS]
    return out


def trap_registry():
    return [("traps", "traps-" + v, lambda v=v: traps(v), (0, 1, 4)) for v in TRAP_VARIANTS]


# the steps a family is named for: each must occur in at least one of its
# cases under the case's stated configuration
FAMILY_STEPS = {
    "s_gate": ("LINE_FIRST", "LINE_CHECK", "VERIFY_HIT"),
    "line_window": ("LINE_FIRST", "LINE_CHECK", "VERIFY_HIT", "FIND"),
    "guess_window_edge": ("LINE_CHECK", "VERIFY_HIT", "FIND"),
    "guess_rounds": ("GUESS_TAKEN", "GUESS_FAIL"),
    "span_edge": ("GUESS_TAKEN", "VERIFY_HIT"),
    "try_learn": ("TRY_HIT", "TRY_MISS", "LEARN", "FIND", "TRUST_ZERO"),
}


def expected(buf, exp, cfg):
    """The index a case must give under cfg."""
    gone = set(exp["missing"](cfg)) if "missing" in exp else set()
    if not gone:
        return plain_index(buf)
    ends = true_ends(buf)
    assert gone <= set(ends)
    return index_of_ends(buf, [e for e in ends if e not in gone])
