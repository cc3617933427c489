"""Region-list queries (query-regions, query-samples-regions,
genotype-counts-regions) restated in Python, and their test
inputs.

The feature has no reference counterpart: a record matches a region set iff
it matches one of its regions as the range query decides.  `match_or` says
exactly that, as the OR of subset_cases.match (counts_cases.match where a POS
has one of strtoul's other spellings) over the regions; `Table` / `match_table`
say it a second way, by bisection over merged intervals, the way the kernel's
table works.  The two are held equal on every case, and the kernel to them:
test_regions_emu.py on the CPU emulator, test_gpu_regions.py on the GPU."""
import bisect
import hashlib
import json
import os
import random

import counts_cases as CC
import decode_cases as D
import golden_io as G
import subset_cases as SC

OK, E_NOSPACE, E_ARG, E_FORMAT = 0, 4, 5, 8
U64 = (1 << 64) - 1
NO_ERROR = U64


# ---- region text ------------------------------------------------------------

class RegionError(ValueError):
    def __init__(self, line):
        ValueError.__init__(self, "line %d" % line)
        self.line = line


def _strtoul(s):
    """str_to_uint64: the whole string by strtoul; b"" is 0; None: no parse."""
    return CC.pos_parse(s)


def parse_query(q):
    """vcfc_parse_query: (ref, has_range, start, end), or None."""
    c = q.find(b":")
    if c < 0:
        return q, False, 0, 0
    d = q.find(b"-", c + 1)
    if d < 0:
        return None
    a, b = _strtoul(q[c + 1:d]), _strtoul(q[d + 1:])
    if a is None or b is None:
        return None
    return q[:c], True, a, b


def _bed_number(s):
    if not 1 <= len(s) <= 20 or not all(0x30 <= c <= 0x39 for c in s):
        return None
    v = int(s)
    return v if v <= U64 else None


def parse_text(text):
    """The regions of region text, (name, start, end) inclusive, an empty one
    as start > end; RegionError(line) for the first line that does not parse."""
    out = []
    parts = text.split(b"\n")
    if parts[-1] == b"":
        parts.pop()          # the text ends with its LF
        last_has_lf = True
    else:
        last_has_lf = False
    for no, l in enumerate(parts, 1):
        if (no < len(parts) or last_has_lf) and l.endswith(b"\r"):
            l = l[:-1]
        if l == b"" or l.startswith((b"#", b"track", b"browser")):
            continue
        if b"\t" in l:
            f = l.split(b"\t")
            if len(f) < 3:
                raise RegionError(no)
            a, b = _bed_number(f[1]), _bed_number(f[2])
            if a is None or b is None:
                raise RegionError(no)
            out.append((f[0], a + 1, b) if b > a else (f[0], 1, 0))
        else:
            q = parse_query(l)
            if q is None:
                raise RegionError(no)
            out.append((q[0], q[2], q[3]) if q[1] else (q[0], 0, U64))
    return out


def text_of(regions):
    """Coordinate-string text of (name, start, end) regions."""
    return b"".join(b"%s:%d-%d\n" % r for r in regions)


# ---- the set match, two ways ------------------------------------------------

def match_or(b, rs, re, regions, match=SC.match):
    """The OR of the one-region match over the regions; None, a match error,
    wins (it does not depend on the region)."""
    m = match(b, rs, re, b"", False, 0, 0)
    if m is None:
        return None
    return any(match(b, rs, re, name, True, start, end) for name, start, end in regions)


class Table:
    """Per name the sorted, disjoint intervals, overlapping and adjacent ones
    merged: what vcfc_regions_build keeps."""

    def __init__(self, regions):
        by = {}
        for name, a, b in regions:
            if a <= b:
                by.setdefault(name, []).append((a, b))
        self.starts, self.ends = {}, {}
        for name, iv in by.items():
            iv.sort()
            st, en = [], []
            for a, b in iv:
                if st and a <= min(en[-1], U64 - 1) + 1:
                    en[-1] = max(en[-1], b)
                else:
                    st.append(a)
                    en.append(b)
            self.starts[name], self.ends[name] = st, en

    def hit(self, name, pos):
        st = self.starts.get(name)
        if st is None:
            return False
        k = bisect.bisect_right(st, pos)
        return k > 0 and pos <= self.ends[name][k - 1]

    def intervals(self):
        return sum(len(v) for v in self.starts.values())


def fields(b, rs, re):
    """(CHROM, POS text) of record b[rs:re], or None where a TAB is missing."""
    t1 = b.find(b"\t", rs + 8, re)
    t2 = b.find(b"\t", t1 + 1, re) if t1 >= 0 else -1
    if t1 < 0 or t2 < 0:
        return None
    return b[rs + 8:t1], b[t1 + 1:t2]


def match_table(b, rs, re, table):
    f = fields(b, rs, re)
    pos = None if f is None else CC.pos_parse(f[1])
    if pos is None:
        return None
    return table.hit(f[0], pos) or table.hit(b"", pos)


def plain(b, rec):
    """Every POS is plain decimal below 2^64: subset_cases.match reads it right."""
    for i in range(len(rec) - 1):
        f = fields(b, rec[i], rec[i + 1])
        if f is not None and f[1].isdigit() and int(f[1]) > U64:
            return False
        if f is not None and f[1] and not f[1].isdigit() and CC.pos_parse(f[1]) is not None:
            return False
    return True


def expected(b, rec, regions):
    """(flags, error word) of records b[rec[i]:rec[i + 1]] against the set:
    the bisect restatement, held equal to the OR restatement on the way."""
    table = Table(regions)
    flags, err = [], NO_ERROR
    is_plain = plain(b, rec)
    for i in range(len(rec) - 1):
        m = match_table(b, rec[i], rec[i + 1], table)
        assert m == match_or(b, rec[i], rec[i + 1], regions, CC.match), (i, regions[:4])
        if is_plain:
            assert m == match_or(b, rec[i], rec[i + 1], regions), (i, regions[:4])
        if m is None:
            code = 3 if fields(b, rec[i], rec[i + 1]) is None else 2
            err = min(err, (i << 8) | code)
        flags.append(1 if m else 0)
    return flags, err


def records_of(data):
    """(data section, record offsets with the hop end, S) of a .vcfc."""
    h, S = SC.parse_header(data)
    body = data[h:]
    rec, end = SC.hop(body)
    return body, rec + [end], S


# ---- the three actions --------------------------------------------------------

def full_line(v, data_off, b, rs, re, S):
    """The line the decoder writes for record b[rs:re], or None where it
    reports the record in its error word.  A regular record: its fields as
    they stand.  Any other: the oracle's decode of the record alone has to
    end cleanly with exactly one line."""
    r = SC.regular(b, rs, re, S)
    if r is not None:
        return SC.line(r[0], r[1], range(S))
    st, out = G.oracle_decompress(v[:data_off] + b[rs:re], cap=(re - rs) * 8 + 4 * S + 4096)
    lines = out[len(v[:data_off]):] if out.startswith(v[:data_off]) else out
    if st != 0 or lines.count(b"\n") != 1 or not lines.endswith(b"\n"):
        return None
    return lines


def walk(v, regions, emit):
    """The stop rule the three actions share: emit(i, b, rs, re, S) gives a
    matching record's output, None where the record cannot be taken.  Returns
    (status, outputs, failing record)."""
    h = SC.parse_header(v)
    data_off, S = h
    b = v[data_off:]
    rec, end = SC.hop(b)
    out = []
    for i, rs in enumerate(rec):
        re = rec[i + 1] if i + 1 < len(rec) else end
        m = match_or(b, rs, re, regions, CC.match)
        if m is None:
            return E_FORMAT, out, i
        if m:
            r = emit(i, b, rs, re, S)
            if r is None:
                return E_FORMAT, out, i
            out.append(r)
    return (E_FORMAT, out, len(rec)) if len(b) - end >= 8 else (OK, out, CC.NO_RECORD)


def query_regions(v, regions):
    """query-regions: (status, bytes)."""
    h = SC.parse_header(v)
    if h is None:
        return E_FORMAT, b""
    st, out, _ = walk(v, regions, lambda i, b, rs, re, S: full_line(v, h[0], b, rs, re, S))
    return st, b"".join(out)


def query_samples_regions(v, regions, cols):
    """query-samples-regions: (status, bytes)."""
    h = SC.parse_header(v)
    if h is None:
        return E_FORMAT, b""
    if not SC.check_cols(cols, h[1]):
        return E_ARG, b""

    def emit(i, b, rs, re, S):
        r = SC.regular(b, rs, re, S)
        return None if r is None else SC.line(r[0], r[1], cols)
    st, out, _ = walk(v, regions, emit)
    return st, b"".join(out)


def counts_regions(v, regions):
    """genotype-counts-regions: (status, indices, rows, samples or None,
    failing record), as counts_cases.counts_full."""
    h = SC.parse_header(v)
    if h is None:
        return E_FORMAT, [], [], None, CC.NO_RECORD
    if h[1] == 0 or h[1] >= 1 << 30:
        return E_ARG, [], [], None, CC.NO_RECORD
    samples = [[0] * 5 for _ in range(h[1])]

    def emit(i, b, rs, re, S):
        r = SC.regular(b, rs, re, S)
        if r is None:
            return None
        for j, t in enumerate(r[1]):
            samples[j][CC.CLASS.get(t, 4)] += 1
        return i, CC.row(r[1])
    st, out, bad = walk(v, regions, emit)
    return st, [x[0] for x in out], [x[1] for x in out], samples if st == OK else None, bad


# ---- inputs -------------------------------------------------------------------

SETS = {
    "A": b"1:100-250\n2:300-400\nchrX\n1:240-300\n3:1-1000\n1:500-400\n",
    "B": b":150-200\n2\n",
    "C": b"".join(b"1:%d-%d\n" % (100 + 20 * k, 109 + 20 * k) for k in range(30)),
    "D": b"11\nchr\n:1000-2000\n",
    "E": b"1:100-100\n1:690-690\n2:0-99\nchrX:691-18446744073709551615\n",
}
SET_MATCHES = {"A": 33, "B": 21, "C": 13, "D": 0, "E": 1}   # of query_files(1)'s 60 records

TEXT_ERRORS = [   # (text, the line that does not parse)
    (b"1:100-200\n1:5\n", 2),                        # no dash after the colon
    (b"1:x-5\n", 1),                                 # start
    (b"#c\n\n1:5-y\n", 3),                           # end (skipped lines count)
    (b"1\t5\n", 1),                                  # BED with two fields
    (b"1\t5\t\n", 1),                                # an empty BED number
    (b"1\t-5\t9\n", 1),                              # BED takes digits only
    (b"1\t5\t+9\n", 1),
    (b"1\t5\t9x\tname\n", 1),
    (b"1\t5\t18446744073709551616\n", 1),            # past 2^64 - 1
    (b"1\t5\t000000000000000000009\n", 1),           # 21 digits
    (b"2\n1\t1\t2\n3:1-2\r\nbad:1\r\n", 4),
    (b"1:1-2\nbad:", 2),                             # the last line without its LF
]

TEXT_SAME = [   # texts that give one table
    (b"1\t99\t250\n", b"1:100-250\n"),
    (b"1\t99\t250\tgene\t0\t+\n", b"1:100-250\n"),
    (b"1:100-250\r\n2\r\n", b"1:100-250\n2\n"),
    (b"1:100-250\n2", b"1:100-250\n2\n"),
    (b"# comment\ntrack name=x\nbrowser position 1\n\n1:100-250\n", b"1:100-250\n"),
    (b"1\t0\t18446744073709551615\n", b"1:1-18446744073709551615\n"),
    (b"1\t5\t5\n1\t9\t3\n2:7-7\n", b"2:7-7\n"),      # end <= start: empty regions
    (b"1:10-19\n1:20-29\n", b"1:10-29\n"),            # adjacent
    (b"1:5-50\n1:10-20\n1:5-50\n1:40-60\n", b"1:5-60\n"),   # nested, duplicate, overlapping
    (b"1:0-18446744073709551615\n1:7-9\n1:18446744073709551615-18446744073709551615\n", b"1\n"),
    (b":5-9\nchr1\n", b"chr1:0-18446744073709551615\n:5-9\n"),
]


def make_file(fields_list, S=3):
    """A .vcfc of regular records with the given (CHROM, POS text) fields."""
    return D.header(S) + b"".join(SC.rec(c + b"\t" + p + b"\trs\tA\tG\t1\tPASS\t.\tGT\t", SC.fill(S)) for c, p in fields_list)


def _edge_positions(rnd, intervals, n):
    """n POS values on and beside the edges of some of the intervals."""
    picks = [intervals[0], intervals[-1]] + [rnd.choice(intervals) for _ in range(n)]
    out = []
    for a, b in picks:
        out += [a - 1, a, b, b + 1]
    return [p for p in out if 0 <= p <= U64][:n]


def shape_cases():
    """(name, regions, file bytes): the table shapes, each with a 300-record
    file whose POS lie on the interval edges."""
    rnd = random.Random(11)
    out = []
    for n_iv in (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 5000):
        iv = [(1000 + 100 * k, 1000 + 100 * k + 9 + k % 7) for k in range(n_iv)]
        regions = [(b"7", a, b) for a, b in iv]
        rnd.shuffle(regions)
        pos = _edge_positions(rnd, iv, 300)
        pos += [rnd.randrange(900, 1000 + 100 * n_iv + 200) for _ in range(300 - len(pos))]
        chroms = [b"7"] * 280 + [b"8"] * 20
        out.append(("intervals%d" % n_iv, regions, make_file([(c, b"%d" % p) for c, p in zip(chroms, pos)])))
    for n_names in (1, 2, 33, 300):
        names = [b"n%d" % (k * k) for k in range(n_names)]
        regions = [(nm, 100 + k, 200 + k) for k, nm in enumerate(names)]
        rnd.shuffle(regions)
        f = []
        for j in range(300):
            k = j % n_names
            nm = names[k] if j % 5 else names[k] + b"x"      # one in five: a name the table lacks
            f.append((nm, b"%d" % rnd.choice([99 + k, 100 + k, 200 + k, 201 + k, 150])))
        out.append(("names%d" % n_names, regions, make_file(f)))
    pre = [b"1", b"11", b"chr1", b"chr11", b"chr"]
    regions = [(nm, 10 * k, 10 * k + 5) for k, nm in enumerate(pre)]
    f = [(nm, b"%d" % p) for nm in pre + [b"c", b"chr111", b"", b"ch"] for p in range(0, 50, 5)]
    out.append(("prefix_names", regions, make_file(f)))
    long_name = b"chrUn_" + b"K" * 34           # 40 bytes: CHROM alone leaves the 32-byte window
    regions = [(long_name, 5, 9), (b"1", 5, 9), (long_name[:-1] + b"L", 0, U64)]
    f = [(long_name, b"7"), (long_name, b"10"), (long_name[:-1], b"7"), (long_name[:-1] + b"L", b"7"),
         (b"1", b"0000000000000000000000007"), (b"1", b"0000000000000000000000010"), (b"2", b"0000000000000000000000007"),
         (long_name, b"0000000000000000000000005")]
    out.append(("past_window", regions, make_file(f * 3)))
    regions = [(b"", 150, 200), (b"1", 100, 120), (b"2", 0, U64), (b"", 400, 400)]
    f = [(c, b"%d" % p) for c in (b"1", b"2", b"3", b"") for p in (99, 100, 120, 121, 149, 150, 200, 201, 399, 400, 401)]
    out.append(("wildcard", regions, make_file(f)))
    regions = [(b"1", 10, 19), (b"1", 20, 29), (b"1", 10, 19), (b"1", 12, 14), (b"1", 40, 50), (b"1", 45, 47), (b"1", 50, 60)]
    out.append(("merge", regions, make_file([(b"1", b"%d" % p) for p in range(5, 65)])))
    regions = [(b"1", 0, 0), (b"1", U64, U64)]
    spell = [b"", b"0", b"+5", b"-1", b"007", b"18446744073709551616", b"18446744073709551615", b"1", b" 0", b"-0",
             b"18446744073709551614"]
    out.append(("pos_spellings", regions, make_file([(b"1", p) for p in spell] + [(b"2", p) for p in spell])))
    out.append(("pos_spellings_wild", [(b"", 0, 0), (b"", U64, U64)], make_file([(b"1", p) for p in spell])))
    return out


def count_cases():
    """(n, regions, file bytes): record counts on the block edges."""
    regions = [(b"1", 100, 130), (b"1", 2000, 2300), (b"2", 0, U64)]
    return [(n, regions, make_file([(b"1" if i % 3 else b"2", b"%d" % (100 + 9 * i)) for i in range(n)]))
            for n in (0, 1, 255, 256, 257)]


# ---- checks shared by the emulator and the GPU suites ---------------------------
# build(text) -> table bytes (raises RegionError(line))
# flags(body, rec, table) -> (flag list, error word)
# single(body, rec, q) -> (flag list, error word) of the one-region match

def check_text(build):
    for a, b in TEXT_SAME:
        assert build(a) == build(b), (a, b)
        assert Table(parse_text(a)).starts == Table(parse_text(b)).starts and \
            Table(parse_text(a)).ends == Table(parse_text(b)).ends, (a, b)
    for text, line in TEXT_ERRORS:
        try:
            parse_text(text)
            raise AssertionError("the restatement takes %r" % text)
        except RegionError as e:
            assert e.line == line, (text, e.line)
        try:
            build(text)
            raise AssertionError("the build takes %r" % text)
        except RegionError as e:
            assert e.line == line, (text, e.line)
    assert build(b"") == build(b"# nothing\n\n1:5-4\n")   # an empty set is a table too


def check_sets(flags, build, seed=1):
    """Sets A..E on the valid file and its mutations; the outcome counts the
    sets were chosen for."""
    files = SC.query_files(seed)
    for key, text in SETS.items():
        regions = parse_text(text)
        table = build(text)
        for name, data in files:
            body, rec, S = records_of(data)
            want = expected(body, rec, regions)
            assert flags(body, rec, table) == want, (key, name)
            if name == "valid" and seed == 1:
                assert sum(want[0]) == SET_MATCHES[key] and len(want[0]) == 60, (key, sum(want[0]))


def check_invariant(flags, single, build, seed=1):
    """Set flags == OR of the one-region flags, equal error words."""
    for key, text in SETS.items():
        regions = parse_text(text)
        table = build(text)
        for name, data in SC.query_files(seed):
            body, rec, S = records_of(data)
            got = flags(body, rec, table)
            acc, errs = [0] * (len(rec) - 1), set()
            for nm, a, b in regions:
                f, e = single(body, rec, (nm, True, a, b))
                acc = [x | y for x, y in zip(acc, f)]
                errs.add(e)
            assert len(errs) == 1 and got == (acc, errs.pop()), (key, name)


def check_shapes(flags, build):
    for name, regions, data in shape_cases():
        body, rec, S = records_of(data)
        table = build(text_of(regions))
        want = expected(body, rec, regions)
        assert want[1] == NO_ERROR or name.startswith("pos_spellings"), name
        assert flags(body, rec, table) == want, name
        if name not in ("names1", "names2"):
            assert 0 < sum(want[0]) < len(want[0]), (name, sum(want[0]))
    for n, regions, data in count_cases():
        body, rec, S = records_of(data) if n else (b"", [0], 3)   # (a header without records is no .vcfc)
        assert len(rec) - 1 == n
        assert flags(body, rec, build(text_of(regions))) == expected(body, rec, regions), n


def check_drivers(qry, qsam, cnt, seed=1):
    """The three actions on query_files(seed) x A..E; over the no_lf / nul_req
    mutations and sets A..C, how many (file, set) pairs stop and run through
    (sample subset: only matching records must be regular)."""
    stopped = through = 0
    for name, data in SC.query_files(seed):
        for key, text in SETS.items():
            regions = parse_text(text)
            assert qry(data, text) == query_regions(data, regions), (name, key)
            for cols in ([0], [39, 0, 17]):
                want = query_samples_regions(data, regions, cols)
                assert qsam(data, text, cols) == want, (name, key, cols)
            assert cnt(data, text) == counts_regions(data, regions), (name, key)
            if name.startswith(("no_lf", "nul_req")) and key in "ABC":
                stopped += want[0] == E_FORMAT
                through += want[0] == OK
    assert stopped >= 6 and through >= 12, (stopped, through)
    return stopped, through


# ---- the golden pin to the reference's own CLI -----------------------------------

def golden():
    with open(os.path.join(G.GOLDEN, "regions_cases.json")) as f:
        return json.load(f)


def check_golden(qry):
    """qry(data, text) -> (status, bytes) against tests/golden/regions_cases.json
    (make_regions_golden.py: the reference's `main query` once per region)."""
    g = golden()
    data = G.gz(g["file"])
    text = g["regions"].encode()
    st, out = qry(data, text)
    assert st == OK
    assert out.count(b"\n") == g["union_lines"] and hashlib.sha256(out).hexdigest() == g["union_sha256"]
    for region, n in zip(text.split(b"\n"), g["region_lines"]):
        st, one = qry(data, region + b"\n")
        assert st == OK and one.count(b"\n") == n, region
