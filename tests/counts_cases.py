"""genotype-counts restated in Python, and its test inputs.

The feature has no reference action: its oracle is a tally over the
reference's own decode.  `counts` below restates the definition (header, LEN
hops, the regular-record rule of subset_cases, the query match, the GT rule,
the stop rule); test_counts_emu.py pins it to the oracle and to a literal GT
table, then holds the kernels and driver to it on the CPU emulator, exact
integers and bytes; test_gpu_counts.py does the same on the GPU."""
import decode_cases as D
import subset_cases as SC

OK, E_ARG, E_FORMAT = SC.OK, SC.E_ARG, SC.E_FORMAT
NO_RECORD = (1 << 64) - 1
CLASS = {b"0|0": 0, b"0|1": 1, b"1|0": 2, b"1|1": 3}   # every other token: 4


def gt(tok):
    """(AN, AC1, AC_other) of a token."""
    g = tok.split(b":", 1)[0]
    an = ac1 = aco = 0
    for piece in g.replace(b"/", b"|").split(b"|"):
        if piece and all(0x30 <= d <= 0x39 for d in piece):
            v = 0
            for d in piece:
                v = min(2, 10 * v + d - 0x30)
            an += 1
            ac1 += v == 1
            aco += v == 2
    return an, ac1, aco


def row(toks):
    """n00 n01 n10 n11 n_other AN AC1 AC_other of a record's tokens."""
    r = [0] * 8
    for t in toks:
        r[CLASS.get(t, 4)] += 1
        a = gt(t)
        r[5] += a[0]
        r[6] += a[1]
        r[7] += a[2]
    return r


def pos_parse(s):
    """k_query_match's POS: strtoul(s, &end, 10) with the whole field used;
    an empty field is 0; None where it does not parse."""
    if not s:
        return 0
    i, n = 0, len(s)
    while i < n and s[i] in b" \t\n\v\f\r":
        i += 1
    neg = i < n and s[i] == 0x2D
    if i < n and s[i] in b"+-":
        i += 1
    if i >= n or not s[i:].isdigit():
        return None
    v = min(int(s[i:]), (1 << 64) - 1)
    return (-v) % (1 << 64) if neg and v < (1 << 64) - 1 else v


def match(b, rs, re, ref, has_range, start, end):
    """subset_cases.match with the POS forms strtoul takes (blanks, a sign):
    True / False, or None for a match error."""
    t1 = b.find(b"\t", rs + 8, re)
    t2 = b.find(b"\t", t1 + 1, re) if t1 >= 0 else -1
    if t1 < 0 or t2 < 0:
        return None
    pos = pos_parse(b[t1 + 1:t2])
    if pos is None:
        return None
    if ref and b[rs + 8:t1] != ref:
        return False
    return not has_range or start <= pos <= end


def counts_full(v, query=None):
    """(status, indices, rows, samples or None, failing record): query = None,
    or (ref, has_range, start, end)."""
    h = SC.parse_header(v)
    if h is None:
        return E_FORMAT, [], [], None, NO_RECORD
    data_off, S = h
    if S == 0 or S >= 1 << 30:
        return E_ARG, [], [], None, NO_RECORD
    b = v[data_off:]
    rec, end = SC.hop(b)
    idx, rows = [], []
    samples = [[0] * 5 for _ in range(S)]
    for i, rs in enumerate(rec):
        re = rec[i + 1] if i + 1 < len(rec) else end
        if query is not None:
            m = match(b, rs, re, *query)
            if m is None:
                return E_FORMAT, idx, rows, None, i
            if not m:
                continue
        r = SC.regular(b, rs, re, S)
        if r is None:
            return E_FORMAT, idx, rows, None, i
        idx.append(i)
        rows.append(row(r[1]))
        for j, t in enumerate(r[1]):
            samples[j][CLASS.get(t, 4)] += 1
    if len(b) - end >= 8:
        return E_FORMAT, idx, rows, None, len(rec)
    return OK, idx, rows, samples, NO_RECORD


def counts(v, query=None):
    return counts_full(v, query)[:4]


def variants_tsv(v, idx, rows):
    """The variants file of the counted records idx (their rows)."""
    data_off, S = SC.parse_header(v)
    b = v[data_off:]
    rec, end = SC.hop(b)
    out = [b"#CHROM\tPOS\tN_00\tN_01\tN_10\tN_11\tN_OTHER\tAN\tAC1\tAC_OTHER\n"]
    for i, r in zip(idx, rows):
        f = b[rec[i] + 8:].split(b"\t", 2)
        out.append(f[0] + b"\t" + f[1] + b"".join(b"\t%d" % x for x in r) + b"\n")
    return b"".join(out)


def samples_tsv(v, samples):
    data_off, S = SC.parse_header(v)
    ls = v.rfind(b"\n", 0, data_off - 1) + 1
    names = v[ls:data_off - 1].split(b"\t")[9:]
    return b"#SAMPLE\tN_00\tN_01\tN_10\tN_11\tN_OTHER\n" + \
        b"".join(n + b"".join(b"\t%d" % x for x in s) + b"\n" for n, s in zip(names, samples))


def tally_vcf(vcf):
    """(rows' class counters, sample table) of VCF text, by a plain count of
    its tokens (the oracle side: no .vcfc is read)."""
    from collections import Counter
    rows, samples = [], None
    for l in vcf.split(b"\n")[:-1]:
        if l.startswith(b"#"):
            continue
        toks = l.split(b"\t")[9:]
        c = Counter(CLASS.get(t, 4) for t in toks)
        rows.append([c[k] for k in range(5)])
        if samples is None:
            samples = [[0] * 5 for _ in toks]
        for j, t in enumerate(toks):
            samples[j][CLASS.get(t, 4)] += 1
    return rows, samples


# ---- inputs ---------------------------------------------------------------

# the GT rule's literal table: token -> (AN, AC1, AC_other), written out
GT_TABLE = [
    (b"0|0", (2, 0, 0)), (b"0|1", (2, 1, 0)), (b"1|0", (2, 1, 0)), (b"1|1", (2, 2, 0)), (b"2|0", (2, 0, 1)),
    (b"0|2", (2, 0, 1)), (b"1|2", (2, 1, 1)), (b".|.", (0, 0, 0)), (b"0/1", (2, 1, 0)), (b"0", (1, 0, 0)),
    (b"1", (1, 1, 0)), (b".", (0, 0, 0)), (b"./.:0", (0, 0, 0)), (b"1|0:35", (2, 1, 0)), (b"10|2", (2, 0, 2)),
    (b"01|1", (2, 2, 0)), (b"00", (1, 0, 0)), (b"010", (1, 0, 1)), (b"1/", (1, 1, 0)), (b"|", (0, 0, 0)),
    (b"0|1|1", (3, 2, 0)), (b"a|1", (1, 1, 0)), (b"1|a:1|1", (1, 1, 0)), (b":1|1", (0, 0, 0)), (b"", (0, 0, 0)),
]

HS = SC.HS   # samples of the hand-built records (600)


def hand_built():
    """(name, file bytes): S = 600 records aimed at the histogram's column
    ranges and at the classification of escaped tokens."""
    hd = D.header(HS)
    rec, req_of, fill = SC.rec, SC.req_of, SC.fill
    out = []
    # a 0|1 x 31 run byte whose columns start at 225 .. 256 (around the first window's tokens) and at S - 31
    starts = list(range(225, 257)) + [HS - 31]
    out.append(("run31_at", hd + b"".join(rec(req_of(i), fill(a) + b"\xbf" + fill(HS - a - 31)) for i, a in enumerate(starts))))
    out.append(("all_11x31", hd + rec(req_of(0), fill(HS, 0x80)) + rec(req_of(1), fill(HS, 0x80))))
    out.append(("escaped_01", hd + rec(req_of(0), fill(10) + b"\xe10|1\t" + fill(HS - 11)) +
                rec(req_of(1), fill(HS - 1, 0xC0) + b"\xe10|1") + rec(req_of(2), b"\xe21|1\t0|0\t" + fill(HS - 2, 0xA0))))
    body = []
    for t, _ in GT_TABLE:
        for c in (0, 255, 256, HS - 1):   # (the last token once ended by the LF, once by a TAB)
            body.append(rec(req_of(len(body)), fill(c) + b"\xe1" + t + (b"" if c == HS - 1 and len(body) % 8 < 4 else b"\t") +
                            fill(HS - c - 1, 0x80)))
    out.append(("gt_tokens", hd + b"".join(body)))
    # class runs filling the first 256-byte window, then an item only the byte-serial path takes: what the
    # wave-parallel scan had added to the histogram by then must not stay
    out.append(("not_simple_late", hd + rec(req_of(0), b"\xa1\xc1" * 140 + b"\xe15|12345\t" + fill(HS - 281, 0x80)) +
                rec(req_of(1), b"\x81" * 300 + b"\xe0" + fill(HS - 301, 0xA0) + b"\xe1.")))
    return out


def lds_limit_files(L):
    """(name, bytes): S = L - 1, L, L + 1 (L = the LDS tile's samples), six
    records each: non-reference runs and one escape in the last 40 columns,
    so some lie across columns L - 1 | L and one run ends at S."""
    rec, req_of, fill = SC.rec, SC.req_of, SC.fill
    out = []
    for S in (L - 1, L, L + 1):
        body = []
        for i in range(5):
            tail = bytes([0xA0 | (5 + i), 0xC0 | 3]) + b"\xe12|1\t" + bytes([0x80 | 20]) + fill(11 - 2 * i) + \
                (bytes([0xA0 | i]) if i else b"")
            body.append(rec(req_of(i), fill(S - 40) + tail))
        body.append(rec(req_of(5), fill(S - 32) + b"\x9f" + b"\xe10|1"))
        out.append(("S%d" % S, D.header(S) + b"".join(body)))
    return out


def wide_files():
    """(name, bytes): S = 2^15 - 1 and 2^15, where a record's counters stop
    fitting 16 bits each (the kernel sums them two to a register below that),
    three records each: long class runs, escapes of every kind, a last run
    that ends at S."""
    rec, req_of, fill = SC.rec, SC.req_of, SC.fill
    out = []
    for S in ((1 << 15) - 1, 1 << 15):
        body = [rec(req_of(0), fill(S - 9000) + fill(4000, 0xA0) + b"\xe12|1\t" + fill(4999, 0x80)),
                rec(req_of(1), fill(S - 70, 0xC0) + b"\xe1.|.\t" + fill(60) + b"\xe10|1\t\xe12|2\t" + fill(7, 0xA0)),
                rec(req_of(2), fill(S))]
        out.append(("S%d" % S, D.header(S) + b"".join(body)))
    return out


def lost_update_files():
    """(name, bytes, expected sample table): many records over few columns."""
    rec, req_of, fill = SC.rec, SC.req_of, SC.fill
    n = 3000
    a = D.header(8) + b"".join(rec(req_of(i), fill(8, 0x80)) for i in range(n))
    m = 700
    b = D.header(70) + b"".join(rec(req_of(i), fill(i % 70) + b"\xa1" + fill(69 - i % 70)) for i in range(m))
    return [("all_11", a, [[0, 0, 0, n, 0] for _ in range(8)]),
            ("diagonal_01", b, [[m - m // 70, m // 70, 0, 0, 0] for _ in range(70)])]


QUERIES = [None] + SC.QUERIES


# ---- checks shared by the emulator and the GPU suites ----------------------
# run(data, query) -> (status, indices, rows, samples or None, failing record)

def same(got, want, what):
    assert got[0] == want[0], (what, "status", got[0], want[0])
    assert got[4] == want[4], (what, "failing record", got[4], want[4])
    assert list(got[1]) == want[1], (what, "indices")
    assert [list(r) for r in got[2]] == want[2], (what, "rows")
    if want[3] is None:
        assert got[3] is None, (what, "a sample table where none is due")
    else:
        assert got[3] is not None and [list(r) for r in got[3]] == want[3], (what, "sample table")


def check_files(run, files, queries=(None,)):
    for name, data in files:
        for q in queries:
            same(run(data, q), counts_full(data, q), (name, q))


def check_hand_built(run):
    for name, data, _ in SC.hand_built():
        same(run(data, None), counts_full(data, None), name)
    hb = {name: data for name, data in hand_built()}
    for name, data in hb.items():
        want = counts_full(data, None)
        assert want[0] == OK, name
        same(run(data, None), want, name)
    # the cases mean what their names say
    st, idx, rows, samples = counts(hb["run31_at"])
    assert all(r == [HS - 31, 31, 0, 0, 0, 2 * HS, 31, 0] for r in rows)
    assert [s[1] for s in samples[224:227]] == [0, 1, 2] and samples[286][1] == 1 and samples[287][1] == 0
    assert samples[HS - 1][1] == 1 and samples[HS - 32][1] == 0
    assert counts(hb["all_11x31"])[2] == [[0, 0, 0, HS, 0, 2 * HS, 2 * HS, 0]] * 2
    st, idx, rows, samples = counts(hb["escaped_01"])
    assert rows[0][:5] == [HS - 1, 1, 0, 0, 0] and samples[10] == [0, 2, 1, 0, 0] and samples[HS - 1][1] == 2
    assert rows[2][:5] == [1, HS - 2, 0, 1, 0] and samples[1][0] == 2
    st, idx, rows, samples = counts(hb["not_simple_late"])
    assert samples[0] == [0, 1, 0, 1, 0] and samples[1] == [0, 0, 1, 1, 0] and rows[0][4] == 1
    st, idx, rows, samples = counts(hb["gt_tokens"])
    for k, (t, g) in enumerate(GT_TABLE):
        for r, c in zip(rows[4 * k:4 * k + 4], (0, 255, 256, HS - 1)):
            assert r[5:] == [g[0] + 2 * (HS - 1), g[1] + 2 * (HS - c - 1), g[2]], t


def check_mutated(run, seed):
    """Every mutated file; at least 5 end OK and at least 5 stop after at
    least one row."""
    ok = partial = 0
    for name, data in D.mutated_files(seed):
        want = counts_full(data, None)
        same(run(data, None), want, name)
        ok += want[0] == OK
        partial += want[0] == E_FORMAT and len(want[1]) > 0
    assert ok >= 5 and partial >= 5, (ok, partial)


def check_queries(run, seed):
    stopped = unstopped = 0
    for name, data in SC.query_files(seed):
        for q in (QUERIES if name == "valid" else QUERIES[:3] + QUERIES[5:6]):
            want = counts_full(data, q)
            same(run(data, q), want, (name, q))
            if q is not None and name.startswith(("no_lf", "nul_req")):
                stopped += want[0] == E_FORMAT
                unstopped += want[0] == OK   # the irregular record does not match: the query runs through
    assert stopped >= 5 and unstopped >= 5, (stopped, unstopped)


def check_lost_updates(run):
    for name, data, table in lost_update_files():
        st, idx, rows, samples, bad = run(data, None)
        assert st == OK and [list(r) for r in samples] == table, name
        assert counts(data)[3] == table, name
