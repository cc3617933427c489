"""The sample-subset decode (decompress-samples, query-samples)
restated in Python, and its test inputs.

The feature has no reference counterpart: its oracle is a cut of the
reference's own decode.  `subset` / `subset_query` below restate the
definition (header rewrite, LEN hops, the regular-record walk, the stop
rule); test_subset_emu.py pins them to the oracle (all columns == the
oracle's decode / query) and then holds the kernels to them, whole bytes and
status, on the CPU emulator; test_gpu_subset.py does the same on the GPU."""
import random

import decode_cases as D

OK, E_ARG, E_FORMAT = 0, 5, 8


def parse_header(v):
    """vcfc_dec::parse_header: (data_off, S), or None where it fails."""
    got_meta = got_header = False
    ip = samples = 0
    n = len(v)
    while True:
        if ip >= n:
            return None
        if v[ip] != 0x23:
            if not got_meta or not got_header:
                return None
            break
        if got_header or ip + 1 >= n:
            return None
        if v[ip + 1] == 0x23:
            got_meta = True
        else:
            if not got_meta:
                return None
            got_header = True
        q = v.find(b"\n", ip + 2)
        if q < 0:
            return None
        if got_header:
            samples = max(0, v.count(b"\t", ip + 2, q) - 8)
        ip = q + 1
    return ip, samples


def hop(b):
    """vcfc_dec::hop: (record starts, where hopping stopped)."""
    rec, p, n = [], 0, len(b)
    while n - p >= 8:
        if (b[p] >> 6) != 3 or (b[p + 4] >> 6) != 3:
            break
        L = ((b[p] & 0x3F) << 24) | (b[p + 1] << 16) | (b[p + 2] << 8) | b[p + 3]
        if L < 4 or L + 4 > n - p:
            break
        rec.append(p)
        p += 4 + L
    return rec, p


RUN = {0x80: b"1|1", 0xA0: b"0|1", 0xC0: b"1|0"}


def regular(b, rs, re, S):
    """(REQ, the S tokens) of the regular record b[rs:re], else None."""
    if re - rs < 8 or (b[rs] >> 6) != 3 or (b[rs + 4] >> 6) != 3:
        return None
    req = ((b[rs + 4] & 0x3F) << 24) | (b[rs + 5] << 16) | (b[rs + 6] << 8) | b[rs + 7]
    ip = rs + 8 + req
    if req == 0 or ip > re:
        return None
    R = b[rs + 8:ip]
    if R.count(b"\t") != 9 or b"\x00" in R:
        return None
    toks = []
    while len(toks) < S:
        if ip >= re:
            return None
        x = b[ip]
        ip += 1
        if x < 0x80:
            toks += [b"0|0"] * x
        elif x < 0xE0:
            toks += [RUN[x & 0xE0]] * (x & 0x1F)
        else:
            for u in range(x & 0x1F):
                t0 = ip
                while ip < re and b[ip] not in (9, 10):
                    ip += 1
                if ip >= re:
                    return None
                toks.append(b[t0:ip])
                if b[ip] == 9:
                    ip += 1
                elif not (u + 1 == (x & 0x1F) and len(toks) == S):   # only the very last token may end at the LF
                    return None
        if len(toks) > S:   # an item overshoots S
            return None
    if ip != re - 1 or b[ip] != 10:
        return None
    return R, toks


def check_cols(cols, S):
    return len(cols) > 0 and all(0 <= c < S for c in cols) and len(set(cols)) == len(cols)


def line(R, toks, cols):
    return R + b"\t".join(toks[c] for c in cols) + b"\n"


def header(v, data_off, cols):
    ls = v.rfind(b"\n", 0, data_off - 1) + 1
    f = v[ls:data_off - 1].split(b"\t")
    return v[:ls] + b"\t".join(f[:9] + [f[9 + c] for c in cols]) + b"\n"


def subset(v, cols):
    """decompress-samples: (status, bytes)."""
    h = parse_header(v)
    if h is None:
        return E_FORMAT, b""
    data_off, S = h
    if not check_cols(cols, S):
        return E_ARG, b""
    out = [header(v, data_off, cols)]
    b = v[data_off:]
    rec, end = hop(b)
    for i, rs in enumerate(rec):
        r = regular(b, rs, rec[i + 1] if i + 1 < len(rec) else end, S)
        if r is None:
            return E_FORMAT, b"".join(out)
        out.append(line(r[0], r[1], cols))
    return (E_FORMAT if len(b) - end >= 8 else OK), b"".join(out)


def match(b, rs, re, ref, has_range, start, end):
    """vcfc_query_match_device on plain decimal POS fields: True / False, or
    None for a match error (POS does not parse, CHROM or POS past the record)."""
    t1 = b.find(b"\t", rs + 8, re)
    t2 = b.find(b"\t", t1 + 1, re) if t1 >= 0 else -1
    if t1 < 0 or t2 < 0:
        return None
    pos = b[t1 + 1:t2]
    if pos and not pos.isdigit():
        return None
    if ref and b[rs + 8:t1] != ref:
        return False
    return not has_range or start <= int(pos or b"0") <= end


def subset_query(v, q, cols):
    """query-samples: (status, bytes); q = (ref, has_range, start, end)."""
    h = parse_header(v)
    if h is None:
        return E_FORMAT, b""
    data_off, S = h
    if not check_cols(cols, S):
        return E_ARG, b""
    out = []
    b = v[data_off:]
    rec, end = hop(b)
    for i, rs in enumerate(rec):
        re = rec[i + 1] if i + 1 < len(rec) else end
        m = match(b, rs, re, *q)
        if m is None:
            return E_FORMAT, b"".join(out)
        if m:
            r = regular(b, rs, re, S)
            if r is None:
                return E_FORMAT, b"".join(out)
            out.append(line(r[0], r[1], cols))
    return (E_FORMAT if len(b) - end >= 8 else OK), b"".join(out)


def cut_vcf(vcf, cols, header_too=True):
    """The chosen sample columns of VCF text ('##' lines verbatim)."""
    out = []
    for l in vcf.split(b"\n")[:-1]:
        if l.startswith(b"##"):
            if header_too:
                out.append(l)
            continue
        if l.startswith(b"#") and not header_too:
            continue
        f = l.split(b"\t")
        out.append(b"\t".join(f[:9] + [f[9 + c] for c in cols]))
    return b"".join(x + b"\n" for x in out)


# ---- inputs ---------------------------------------------------------------

def column_sets(S, seed=0):
    """The column sets every file is cut by (the ones S allows)."""
    rnd = random.Random(1000 * seed + S)
    sets = [[0], [S - 1], [S - 1, 0], list(range(S)), list(range(S - 1, -1, -1)), list(range(0, S, 7))]
    for k in (63, 64, 65):
        if S >= k:
            sets.append(rnd.sample(range(S), k))
    if S > 256:
        sets.append(rnd.sample(range(S), min(S, 300)))
    if S > 512:   # the kernel's LDS line tile holds 512 words: at it, and past it
        sets.append(rnd.sample(range(S), 512))
    if S > 1100:
        sets.append(rnd.sample(range(S), 1100))
    seen, out = set(), []
    for c in sets:
        if tuple(c) not in seen:
            seen.add(tuple(c))
            out.append(c)
    return out


rec, req_of, fill = D.rec, D.req_of, D.fill   # (the record builders: decode_cases.py)


HS = 600   # samples of the hand-built records


def hand_built():
    """(name, file bytes, column sets): S = 600 records aimed at the kernel's
    window edges and at the byte-serial path."""
    hd = D.header(HS)
    out = []
    # one 0|0 run chain of 1-token bytes crossing the first 256-byte window edge (and a 1|0 run behind it)
    chain = b"\x01" * 299 + fill(200) + fill(101, 0xC0)
    out.append(("run_chain", hd + rec(req_of(0), chain),
                [[0, 5, 250, 255, 256, 257, 298, 299, 400, 498, 499, 599], [257, 255, 256], [599], list(range(HS))]))
    out.append(("one_run_byte", hd + rec(req_of(0), fill(HS)), [list(range(130, 141)), [253, 127, 200], [126, 127, 254]]))
    # an escape lead at sample-section offsets 244..263: whatever the record's
    # alignment, one of them is the last byte of a window (a record per offset)
    body = b"".join(rec(req_of(i), b"\x01" * off + b"\xe12|1\t" + fill(HS - 1 - off, 0xA0)) for i, off in enumerate(range(244, 264)))
    out.append(("escape_at_edge", hd + body, [list(range(240, 270)), [263, 0, 244, 599], list(range(HS - 1, -1, -1))]))
    out.append(("last_token_lf", hd + rec(req_of(0), fill(HS - 1, 0x80) + b"\xe12|2") + rec(req_of(1), fill(HS - 1) + b"\xe13|12345"),
                [[HS - 1], [HS - 1, 0], [0, HS - 1, 7]]))
    out.append(("empty_escape", hd + rec(req_of(0), fill(10) + b"\xe1\t" + fill(HS - 11, 0xC0)) + rec(req_of(1), fill(HS - 1) + b"\xe1"),
                [[10], [9, 10, 11], [HS - 1, 10, 0], list(range(HS))]))
    out.append(("two_token_escape", hd + rec(req_of(0), fill(300) + b"\xe22|1\t0|2:77\t" + fill(HS - 302, 0x80)),
                [[300], [301], [301, 300, 299, 302], list(range(0, HS, 7))]))
    out.append(("zero_counts", hd + rec(req_of(0), b"\x00\xa0" + fill(HS, 0xA0) + b"") + rec(req_of(1), fill(5) + b"\xe0\x80" + fill(HS - 5)),
                [[0], [4, 5, 6], [HS - 1, 0]]))
    # NUL in REQ: irregular even where decompress accepts it (the second record: one line comes first)
    r = req_of(1)
    out.append(("nul_in_req", hd + rec(req_of(0), fill(HS)) + rec(r[:5] + b"\x00" + r[6:], fill(HS)) + rec(req_of(2), fill(HS)),
                [[0], [HS - 1, 3]]))
    out.append(("overshoot", hd + rec(req_of(0), fill(HS)) + rec(req_of(1), fill(HS - 3) + b"\x04"), [[0], [HS - 1]]))
    out.append(("bytes_after_items", hd + rec(req_of(0), fill(HS) + b"\x00"), [[0]]))
    return out + frame_edges()


def frame_edges():
    """(name, file bytes, column sets): the checks of a record's frame, one
    edge record each between two valid records (a wrong classification also
    shifts a neighbour).  Every edge record but the last is irregular."""
    hd = D.header(HS)
    items = fill(299) + b"\xe12|1\t" + fill(200, 0xA0) + fill(100, 0x80)
    r = req_of(1)
    f = r.split(b"\t")
    long_req = b"\t".join(f[:7] + [b"X" * 2500] + f[8:])   # the sample section starts in a later staged piece
    edges = [("req_zero", rec(r, items, reqlen=0)),
             ("no_samples", rec(r, b"")),                        # 9 + req == len: the last byte is the LF
             ("len_flags_10", rec(r, items, flags=(0x80, 0xC0))),
             ("req_flags_10", rec(r, items, flags=(0xC0, 0x80))),
             ("tabs8", rec(b"\t".join(f[:2] + f[3:]), items)),
             ("tabs10", rec(b"\t".join(f[:3] + f[2:]), items)),
             ("no_lf", rec(r, items, lf=b"\t")),
             ("bytes9", rec(b"", b"", reqlen=1)),
             ("bytes10", rec(b"A", b"")),
             ("long_req", rec(long_req, items))]
    sets = [[0], [HS - 1, 0, 299, 300], list(range(0, HS, 7))]
    return [("frame_" + name, hd + rec(req_of(0), items) + e + rec(req_of(2), items), sets) for name, e in edges]


def batch_files():
    """(name, bytes): 1, 3, 4, 5 and 41 records (four records per block)."""
    rnd = random.Random(77)
    return [("batch%d" % n, D.encode_file(70, D.rows(rnd, n, 70, escapes=0.03, odd=0.01))) for n in (1, 3, 4, 5, 41)]


QUERIES = [(b"1", False, 0, 0), (b"2", True, 100, 400), (b"chrX", False, 0, 0), (b"1", True, 0, (1 << 64) - 1),
           (b"", True, 150, 500), (b"", False, 0, 0), (b"3", False, 0, 0), (b"1", True, 300, 200)]


def query_string(q):
    return q[0] + (b":%d-%d" % (q[2], q[3]) if q[1] else b"")


def query_files(seed):
    """(name, bytes): 60 records, S = 40, CHROMs 1 / 2 / chrX, plain decimal
    POS; the valid file first, then mutations of single records: made
    irregular (stops a query only where the record matches), POS that does
    not parse, CHROM / POS running past the record (stop every query that
    reaches them)."""
    rnd = random.Random(seed)
    S = 40
    lines = []
    for i in range(60):
        chrom = rnd.choice([b"1", b"1", b"2", b"chrX"])
        toks = [D.CLASSES[rnd.randrange(4) if rnd.random() < 0.3 else 0] for _ in range(S)]
        if rnd.random() < 0.2:
            toks[rnd.randrange(S)] = rnd.choice([b"2|0", b"./.", b"0|1:35", b"7"])
        lines.append(chrom + b"\t%d\trs\tA\tG\t1\tPASS\t.\tGT\t" % (100 + 10 * i) + b"\t".join(toks))
    enc = D.encode_file(S, lines)
    h = len(D.header(S))
    out = [("valid", enc)]
    recs, end = hop(enc[h:])
    recs = [h + r for r in recs] + [h + end]

    def mut(name, k, f):
        b = bytearray(enc)
        f(b, recs[k], recs[k + 1])
        out.append(("%s%d" % (name, k), bytes(b)))

    def retab(b, r, e, keep):
        seen = 0
        for j in range(r + 8, e):
            if b[j] == 9:
                seen += 1
                if seen > keep:
                    b[j] = ord("z")
    for k in (0, 17, 33, 59):
        mut("no_lf", k, lambda b, r, e: b.__setitem__(e - 1, ord("x")))        # irregular: the last byte is no LF
        mut("nul_req", k, lambda b, r, e: b.__setitem__(b.index(b"rs", r) + 1, 0))   # irregular: NUL in REQ
        mut("pos_bad", k, lambda b, r, e: b.__setitem__(b.index(b"\t", r + 8) + 1, ord("q")))
    for k in (17, 59):
        mut("chrom_past", k, lambda b, r, e: retab(b, r, e, 0))
        mut("pos_past", k, lambda b, r, e: retab(b, r, e, 1))
    out.append(("truncate9", enc[:-9]))
    out.append(("tail8", enc + b"\xc0\x00\x00\x10\xc0\x00\x00\x01"))
    return out


# ---- checks shared by the emulator and the GPU suites ----------------------
# dec(data, cols) -> (status, bytes); qry(data, q, cols) -> (status, bytes)

def check_files(dec, files, seed=0):
    for name, data in files:
        h = parse_header(data)
        S = h[1] if h else 4
        for cols in column_sets(max(S, 1), seed):
            want = subset(data, cols)
            got = dec(data, cols)
            assert got[0] == want[0], (name, cols[:8], len(cols), got[0], want[0])
            assert got[1] == want[1], (name, cols[:8], len(cols), len(got[1]), len(want[1]))


def check_mutated(dec, seed):
    """Every column set on every mutated file, and the three outcomes: at
    least 5 files end OK and at least 5 stop with at least one line written."""
    files = D.mutated_files(seed)
    check_files(dec, files, seed)
    ok = partial = 0
    for name, data in files:
        h = parse_header(data)
        if h is None or h[1] == 0:
            continue
        st, out = dec(data, [0])
        assert (st, out) == subset(data, [0]), name
        ok += st == OK
        partial += st == E_FORMAT and out.count(b"\n") > data[:h[0]].count(b"\n")
    assert ok >= 5 and partial >= 5, (ok, partial)


def check_hand_built(dec):
    for name, data, sets in hand_built():
        for cols in sets:
            want = subset(data, cols)
            got = dec(data, cols)
            assert got == want, (name, cols[:8], got[0], want[0], len(got[1]), len(want[1]))
    # the cases mean what their names say
    hb = {name: (data, sets) for name, data, sets in hand_built()}
    assert subset(hb["nul_in_req"][0], [0])[0] == E_FORMAT and subset(hb["nul_in_req"][0], [0])[1].count(b"\n") == 3
    assert subset(hb["overshoot"][0], [0])[0] == E_FORMAT and subset(hb["bytes_after_items"][0], [0])[0] == E_FORMAT
    for k in ("run_chain", "one_run_byte", "escape_at_edge", "last_token_lf", "empty_escape", "two_token_escape",
              "zero_counts"):
        assert subset(hb[k][0], [0])[0] == OK, k
    lines = D.header(HS).count(b"\n")
    for name, data, _ in frame_edges():   # the first record's line, then the stop; all three of long_req
        st, out = subset(data, [299])
        assert (st, out.count(b"\n") - lines) == ((OK, 3) if name == "frame_long_req" else (E_FORMAT, 1)), name
        assert out.endswith(b"\t2|1\n"), name
    assert subset(hb["empty_escape"][0], [9, 10, 11])[1].endswith(b"\t0|0\t\t1|0\n" + req_of(1) + b"0|0\t0|0\t0|0\n")
    assert subset(hb["last_token_lf"][0], [HS - 1, 0])[1].endswith(b"\t2|2\t1|1\n" + req_of(1) + b"3|12345\t0|0\n")


def check_queries(qry, seed):
    stopped = unstopped = 0
    for name, data in query_files(seed):
        for q in QUERIES:
            for cols in ([0], [39, 0, 17], list(range(40)), list(range(0, 40, 7))):
                want = subset_query(data, q, cols)
                got = qry(data, q, cols)
                assert got == want, (name, q, cols[:8], got[0], want[0], len(got[1]), len(want[1]))
            if name.startswith(("no_lf", "nul_req")):
                stopped += want[0] == E_FORMAT
                unstopped += want[0] == OK   # the irregular record does not match: the query runs through
    assert stopped >= 5 and unstopped >= 5, (stopped, unstopped)
