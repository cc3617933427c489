"""genotype-matrix restated in Python, and its test inputs.

The feature has no reference action: its oracle is a per-token rule applied
to the reference's own decode.  `matrix` below restates the definition
(header, LEN hops, the regular-record rule of subset_cases, the query or
region-table match, the per-token rule, the row layouts, the stop rule);
test_matrix_emu.py pins it to a literal table, to the oracle's decode, to
genotype-counts and to a hand-written .bed file, then holds the kernels and
driver to it on the CPU emulator, exact bytes; test_gpu_matrix.py does the
same on the GPU."""
import random

import counts_cases as CC
import decode_cases as D
import regions_cases as RC
import subset_cases as SC

OK, E_NOSPACE, E_ARG, E_FORMAT = 0, 4, SC.E_ARG, SC.E_FORMAT
NO_RECORD = (1 << 64) - 1
NO_ERROR = (1 << 64) - 1
DOSAGE, HAP, BED = 0, 1, 2
LAYOUTS = (DOSAGE, HAP, BED)
FILL = 0xEE        # what every output buffer holds before a device call
CANARY = 64        # bytes past out_cap inside the same allocation


def token_codes(tok):
    """(dosage, h0, h1, bed) of a decoded token."""
    gt = tok.split(b":", 1)[0]
    cls = []   # per piece: its class, None where the piece is missing
    for piece in gt.replace(b"/", b"|").split(b"|"):
        if piece and all(0x30 <= d <= 0x39 for d in piece):
            v = 0
            for d in piece:
                v = min(2, 10 * v + d - 0x30)
            cls.append(v)
        else:
            cls.append(None)
    dosage = -1 if None in cls else min(127, sum(1 for c in cls if c != 0))
    h0, h1 = (cls[k] if k < len(cls) and cls[k] is not None else -1 for k in (0, 1))
    bed = 1
    if len(cls) == 2 and None not in cls and max(cls) <= 1:
        bed = {0: 3, 1: 2, 2: 0}[cls[0] + cls[1]]
    return dosage, h0, h1, bed


def row_bytes(layout, S):
    return {DOSAGE: S, HAP: 2 * S, BED: (S + 3) // 4}[layout]


def row(layout, toks):
    """A record's row, as bytes."""
    codes = [token_codes(t) for t in toks]
    if layout == DOSAGE:
        return bytes(c[0] & 0xFF for c in codes)
    if layout == HAP:
        return bytes(x & 0xFF for c in codes for x in c[1:3])
    out = bytearray((len(codes) + 3) // 4)
    for j, c in enumerate(codes):
        out[j // 4] |= c[3] << (2 * (j % 4))
    return bytes(out)


def matrix(v, layout, query=None, table=None):
    """(status, indices, rows, S or None, failing record): query = (ref,
    has_range, start, end), or table = the (name, start, end) regions of a
    region table, or neither."""
    h = SC.parse_header(v)
    if h is None:
        return E_FORMAT, [], [], None, NO_RECORD
    data_off, S = h
    if S == 0 or S >= 1 << 30:
        return E_ARG, [], [], None, NO_RECORD
    b = v[data_off:]
    rec, end = SC.hop(b)
    idx, rows = [], []
    for i, rs in enumerate(rec):
        re = rec[i + 1] if i + 1 < len(rec) else end
        if query is not None or table is not None:
            m = CC.match(b, rs, re, *query) if query is not None else RC.match_or(b, rs, re, table, CC.match)
            if m is None:
                return E_FORMAT, idx, rows, S, i
            if not m:
                continue
        r = SC.regular(b, rs, re, S)
        if r is None:
            return E_FORMAT, idx, rows, S, i
        idx.append(i)
        rows.append(row(layout, r[1]))
    if len(b) - end >= 8:
        return E_FORMAT, idx, rows, S, len(rec)
    return OK, idx, rows, S, NO_RECORD


def bed_file(rows):
    return b"\x6c\x1b\x01" + b"".join(rows)


def bim_file(v, idx):
    data_off, S = SC.parse_header(v)
    b = v[data_off:]
    rec, end = SC.hop(b)
    out = []
    for i in idx:
        f = b[rec[i] + 8:].split(b"\t", 5)
        out.append(b"\t".join([f[0], f[2], b"0", f[1], f[4], f[3]]) + b"\n")
    return b"".join(out)


def fam_file(v):
    data_off, S = SC.parse_header(v)
    ls = v.rfind(b"\n", 0, data_off - 1) + 1
    names = v[ls:data_off - 1].split(b"\t")[9:]
    return b"".join(n + b"\t" + n + b"\t0\t0\t0\t-9\n" for n in names)


def matrix_of_vcf(vcf, layout):
    """The rows of VCF text, by the per-token rule alone (the oracle side: no
    .vcfc is read)."""
    return [row(layout, l.split(b"\t")[9:]) for l in vcf.split(b"\n")[:-1] if not l.startswith(b"#")]


# ---- inputs ---------------------------------------------------------------

# the per-token rule's literal table: token -> (dosage, h0, h1, bed), written
# out by hand: the 25 tokens of counts_cases.GT_TABLE, then eight more
CODE_TABLE = [
    (b"0|0", (0, 0, 0, 3)), (b"0|1", (1, 0, 1, 2)), (b"1|0", (1, 1, 0, 2)), (b"1|1", (2, 1, 1, 0)),
    (b"2|0", (1, 2, 0, 1)), (b"0|2", (1, 0, 2, 1)), (b"1|2", (2, 1, 2, 1)), (b".|.", (-1, -1, -1, 1)),
    (b"0/1", (1, 0, 1, 2)), (b"0", (0, 0, -1, 1)), (b"1", (1, 1, -1, 1)), (b".", (-1, -1, -1, 1)),
    (b"./.:0", (-1, -1, -1, 1)), (b"1|0:35", (1, 1, 0, 2)), (b"10|2", (2, 2, 2, 1)), (b"01|1", (2, 1, 1, 0)),
    (b"00", (0, 0, -1, 1)), (b"010", (1, 2, -1, 1)), (b"1/", (-1, 1, -1, 1)), (b"|", (-1, -1, -1, 1)),
    (b"0|1|1", (2, 0, 1, 1)), (b"a|1", (-1, -1, 1, 1)), (b"1|a:1|1", (-1, 1, -1, 1)), (b":1|1", (-1, -1, -1, 1)),
    (b"", (-1, -1, -1, 1)),
    (b"1", (1, 1, -1, 1)), (b"0|0|1", (1, 0, 0, 1)), (b".|1", (-1, -1, 1, 1)), (b"2/0", (1, 2, 0, 1)),
    (b"0|2", (1, 0, 2, 1)), (b"10|1", (2, 2, 1, 1)), (b"", (-1, -1, -1, 1)), (b":5", (-1, -1, -1, 1)),
]

# the issue's worked examples, as written there
EXAMPLES = {b"0|0": 0, b"0|1": 1, b"1|0": 1, b"1|1": 2, b"1": 1, b"0|2": 1, b"./.": -1, b"0|.": -1, b"0/1:12:40": 1}
HAP_EXAMPLES = {b"0|1": (0, 1), b"1": (1, -1), b"2/0": (2, 0), b".|1": (-1, 1)}

# a literal .bed file: S = 5, nine bytes written out by hand: the three magic
# bytes and three rows of ceil(5 / 4) = 2 bytes.
#   record 0: 0|0 0|1 1|1 ./. 1|0 -> codes 11 10 00 01 10 -> byte 0 = 01 00 10 11 = 0x4B, byte 1 = 0x02
#   record 1: 1|1 0|0 0|0 2|0 0|0 -> codes 00 11 11 01 11 -> byte 0 = 01 11 11 00 = 0x7C, byte 1 = 0x03
#   record 2: 0/1 1|0 0|0 1|1 0|0 -> codes 10 10 11 00 11 -> byte 0 = 00 11 10 10 = 0x3A, byte 1 = 0x03
BED_KAT_TOKENS = [[b"0|0", b"0|1", b"1|1", b"./.", b"1|0"], [b"1|1", b"0|0", b"0|0", b"2|0", b"0|0"],
                  [b"0/1", b"1|0", b"0|0", b"1|1", b"0|0"]]
BED_KAT = bytes([0x6C, 0x1B, 0x01, 0x4B, 0x02, 0x7C, 0x03, 0x3A, 0x03])
BED_KAT_PAD_MASK = 0xFC   # bits of a row's last byte that must be 0 for S = 5

HS = SC.HS


def kat_file():
    lines = [b"1\t%d\trs%d\tA\tG\t1\tPASS\t.\tGT\t" % (100 + i, i) + b"\t".join(t) for i, t in enumerate(BED_KAT_TOKENS)]
    return D.encode_file(5, lines)


def small_files():
    """(name, bytes): the small sample counts (the .bed pad bits, odd row
    sizes, around a wave and a 256-byte window), 18 records each."""
    rnd = random.Random(4242)
    return [("S%d" % S, D.encode_file(S, D.rows(rnd, 18, S, escapes=0.06, odd=0.04)))
            for S in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)]


def table_tokens():
    """(name, bytes): S = 600, every CODE_TABLE token as an escape at columns
    0, 255, 256 and S - 1."""
    rec, req_of, fill = SC.rec, SC.req_of, SC.fill
    body = []
    for t, _ in CODE_TABLE:
        for c in (0, 255, 256, HS - 1):   # (the last token once ended by the LF, once by a TAB)
            body.append(rec(req_of(len(body)), fill(c) + b"\xe1" + t + (b"" if c == HS - 1 and len(body) % 8 < 4 else b"\t") +
                            fill(HS - c - 1, 0xA0)))
    return [("code_tokens", D.header(HS) + b"".join(body))]


def irregular_files():
    """(name, bytes, failing record): an item that passes S, each kind in a
    different position among regular records."""
    rec, req_of, fill = SC.rec, SC.req_of, SC.fill
    hd = D.header(HS)
    good = [rec(req_of(i), fill(100 + i, 0xC0) + b"\xe12|1\t" + fill(HS - 101 - i)) for i in range(4)]
    by1 = rec(req_of(9), fill(HS - 30) + b"\xbf")                      # the last run passes S by 1
    by30 = rec(req_of(9), fill(HS - 1, 0x80) + b"\x9f")                # the last run passes S by 30
    esc = rec(req_of(9), fill(HS, 0xA0) + b"\xe12|1\t")                # an escape passes S
    esc2 = rec(req_of(9), fill(HS - 1) + b"\xe22|1\t0|2\t")            # a two-token escape passes S
    return [("run_over_1", hd + good[0] + good[1] + by1 + good[2], 2),
            ("run_over_30", hd + good[0] + by30 + good[1] + good[2], 1),
            ("escape_over", hd + esc + good[0] + good[1], 0),
            ("escape2_over", hd + good[0] + good[1] + good[2] + esc2, 3)]


def tile_limit_files(L):
    """(name, bytes): S = L - 1, L, L + 1 (L = the LDS tile's samples), three
    records each, mostly 0|0: one of a single class, one with a 0|1 x 31 run
    ending at column S - 1, one with escapes and runs in the last columns."""
    rec, req_of, fill = SC.rec, SC.req_of, SC.fill
    out = []
    for S in (L - 1, L, L + 1):
        body = [rec(req_of(0), fill(S)), rec(req_of(1), fill(S - 31) + b"\xbf"),
                rec(req_of(2), fill(7, 0x80) + fill(S - 20) + b"\xe12|1\t\xc3\xe1./.\t" + fill(5) + b"\x83")]
        out.append(("S%d" % S, D.header(S) + b"".join(body)))
    return out


REGION_TEXTS = [RC.SETS["C"], RC.SETS["B"]]   # many intervals; the wildcard name
QUERIES = [None] + SC.QUERIES


# ---- checks shared by the emulator and the GPU suites ----------------------
# run(data, layout, query=None, regions=None, rec_batch=0) ->
#     (status, indices, rows as a list of bytes, S or None, failing record)

def same(got, want, what):
    assert got[0] == want[0], (what, "status", got[0], want[0])
    assert got[4] == want[4], (what, "failing record", got[4], want[4])
    assert list(got[1]) == want[1], (what, "indices")
    assert len(got[2]) == len(want[2]), (what, "rows", len(got[2]), len(want[2]))
    for k, (a, b) in enumerate(zip(got[2], want[2])):
        assert a == b, (what, "row", k, next(j for j in range(len(b)) if a[j:j + 1] != b[j:j + 1]))


def check_files(run, files, queries=(None,), batches=(0,)):
    for name, data in files:
        for layout in LAYOUTS:
            for q in queries:
                want = matrix(data, layout, q)
                for rb in batches:
                    same(run(data, layout, q, None, rb), want, (name, layout, q, rb))


def check_hand_built(run):
    files = [(n, d) for n, d, _ in SC.hand_built()] + CC.hand_built() + table_tokens()
    check_files(run, files)
    hb = dict(files)
    # the cases mean what their names say
    st, idx, rows, S, bad = matrix(hb["run31_at"], DOSAGE)
    assert st == OK and rows[0] == bytes(225) + b"\x01" * 31 + bytes(HS - 256) and rows[32][HS - 32:] == b"\x00" + b"\x01" * 31
    assert matrix(hb["all_11x31"], BED)[2] == [bytes(HS // 4)] * 2 and matrix(hb["all_11x31"], HAP)[2] == [b"\x01" * 2 * HS] * 2
    assert matrix(hb["escaped_01"], HAP)[2][0][18:24] == bytes([0, 0, 0, 1, 0, 0])
    st, idx, rows, S, bad = matrix(hb["code_tokens"], DOSAGE)
    assert st == OK and len(rows) == 4 * len(CODE_TABLE)
    for k, (t, c) in enumerate(CODE_TABLE):
        for r, col in zip(rows[4 * k:4 * k + 4], (0, 255, 256, HS - 1)):
            assert r[col] == c[0] & 0xFF and r.count(1) >= HS - col - 1, t
    assert matrix(hb["overshoot"], DOSAGE)[0] == E_FORMAT and matrix(hb["not_simple_late"], BED)[0] == OK


def check_irregular(run):
    for name, data, at in irregular_files():
        for layout in LAYOUTS:
            want = matrix(data, layout)
            assert (want[0], want[4], len(want[1])) == (E_FORMAT, at, at), name
            same(run(data, layout), want, (name, layout))


def check_mutated(run, seed):
    """Every mutated file; at least 5 end OK and at least 5 stop after at
    least one row."""
    ok = partial = 0
    for name, data in D.mutated_files(seed):
        for layout in LAYOUTS:
            want = matrix(data, layout)
            same(run(data, layout), want, (name, layout))
        ok += want[0] == OK
        partial += want[0] == E_FORMAT and len(want[1]) > 0
    assert ok >= 5 and partial >= 5, (ok, partial)


def check_queries(run, seed):
    stopped = unstopped = 0
    for name, data in SC.query_files(seed):
        for q in (QUERIES if name == "valid" else QUERIES[:3] + QUERIES[5:6]):
            for layout in (LAYOUTS if name == "valid" or q is None else (BED,)):
                want = matrix(data, layout, q)
                same(run(data, layout, q), want, (name, q, layout))
            if q is not None and name.startswith(("no_lf", "nul_req")):
                stopped += want[0] == E_FORMAT
                unstopped += want[0] == OK   # the irregular record does not match: the query runs through
    assert stopped >= 5 and unstopped >= 5, (stopped, unstopped)


def check_regions(run, seed=1):
    hits = 0
    for text in REGION_TEXTS:
        regions = RC.parse_text(text)
        for name, data in SC.query_files(seed)[:6]:
            for layout in LAYOUTS:
                want = matrix(data, layout, table=regions)
                same(run(data, layout, None, text), want, (name, layout))
                hits += len(want[1]) > 0
    assert hits >= 6


def check_tile_limit(run, lds_samples):
    for layout in LAYOUTS:
        L = lds_samples(layout)
        files = tile_limit_files(L)
        assert [SC.parse_header(d)[1] for _, d in files] == [L - 1, L, L + 1]
        for name, data in files:
            want = matrix(data, layout)
            assert want[0] == OK and len(want[1]) == 3
            S = SC.parse_header(data)[1]
            assert matrix(data, DOSAGE)[2][1][S - 32:] == b"\x00" + b"\x01" * 31
            same(run(data, layout), want, (name, layout))


# ---- the device entry ---------------------------------------------------------
# dev(body, rec, S, layout, select, row_stride, out_cap, alloc, ws_short=0, offset=0) -> (status, err word, the alloc +
# CANARY bytes of the output allocation, which held FILL before the call and whose byte `offset` is d_out, row_of
# as a list of n + 1); the rows lie at d_out + r * row_stride, out_cap counts from d_out

def records_of(data):
    h, S = SC.parse_header(data)
    body = data[h:]
    rec, end = SC.hop(body)
    return body, rec + [end], S


def expect_device(body, rec, S, layout, select, stride, out_cap, alloc):
    """(err word, expected buffer, mask of the bytes that are compared, row_of)."""
    n = len(rec) - 1
    rb = row_bytes(layout, S)
    buf = bytearray([FILL]) * (alloc + CANARY)
    mask = bytearray([1]) * (alloc + CANARY)
    row_of, err, r = [], NO_ERROR, 0
    for i in range(n):
        row_of.append(r)
        if select is not None and not select[i]:
            continue
        if r * stride + rb > out_cap:
            err = min(err, (i << 8) | 0xFF)
        else:
            reg = SC.regular(body, rec[i], rec[i + 1], S)
            if reg is None:
                err = min(err, (i << 8) | 3)
            if reg is None or (i << 8) > err:   # not meaningful: its own bytes are not compared
                mask[r * stride:r * stride + rb] = bytes(rb)
            else:
                buf[r * stride:r * stride + rb] = row(layout, reg[1])
        r += 1
    row_of.append(r)
    return err, bytes(buf), bytes(mask), row_of


def check_device_call(dev, data, layout, select=None, stride_of=lambda rb: rb, cut=None, offset=0, S=None):
    body, rec, S0 = records_of(data)
    S = S0 if S is None else S
    n = len(rec) - 1
    rb = row_bytes(layout, S)
    stride = stride_of(rb)
    rows = n if select is None else sum(1 for x in select if x)
    full = (rows - 1) * stride + rb if rows else 0
    out_cap = full if cut is None else max(0, full - cut) if cut >= 0 else 0
    alloc = max(full, 1)
    err, buf, mask, row_of = expect_device(body, rec, S, layout, select, stride, out_cap, alloc)
    st, gerr, gbuf, grow_of = dev(body, rec, S, layout, select, stride, out_cap, alloc, offset=offset)
    what = (layout, S, stride, out_cap, offset, None if select is None else sum(select))
    assert st == OK and gerr == err, (what, st, gerr, err)
    assert grow_of == row_of, what
    assert len(gbuf) == len(buf)
    bad = [k for k in range(len(buf)) if mask[k] and gbuf[k] != buf[k]]
    assert not bad, (what, "first differing byte", bad[0], "of", len(buf), "canary from", out_cap)
    return err


def check_device(dev):
    name, data = small_files()[6]   # S = 65, 18 records: odd rows, every alignment 0..15 with stride = row_bytes
    assert SC.parse_header(data)[1] == 65
    n = len(records_of(data)[1]) - 1
    selects = [None, [1] * n, [int(i % 8 == 0) for i in range(n)]]
    for layout in LAYOUTS:
        for sel in selects:
            for stride_of in (lambda rb: rb, lambda rb: (rb + 15) & ~15, lambda rb: rb + 1):
                assert check_device_call(dev, data, layout, sel, stride_of) == NO_ERROR
        for offset in (0, 1, 7, 15):
            check_device_call(dev, data, layout, None, lambda rb: rb + 1, offset=offset)
        # out_cap one byte short of the last row, and 0
        assert check_device_call(dev, data, layout, cut=1) == ((n - 1) << 8) | 0xFF
        assert check_device_call(dev, data, layout, cut=-1) == 0xFF
    # a wide record through both strides (16-byte stores in the body, byte heads and tails)
    name, data = SC.batch_files()[3]
    for layout in LAYOUTS:
        check_device_call(dev, data, layout, None, lambda rb: rb + 3)
    for name, data, _ in SC.hand_built()[:3]:
        for layout in LAYOUTS:
            check_device_call(dev, data, layout, None, lambda rb: rb + 5, offset=3)
    # irregular records: the error word, the rows before exact, every byte outside the rows kept
    for name, data, at in irregular_files():
        n = len(records_of(data)[1]) - 1
        for layout in LAYOUTS:
            for stride_of in (lambda rb: rb, lambda rb: rb + 1):
                assert check_device_call(dev, data, layout, None, stride_of) == (at << 8) | 3, name
            # ... and unselected, it is not looked at
            assert check_device_call(dev, data, layout, [int(i != at) for i in range(n)]) == NO_ERROR, name


def check_device_tile_limit(dev, lds_samples):
    for layout in LAYOUTS:
        for name, data in tile_limit_files(lds_samples(layout)):
            assert check_device_call(dev, data, layout, None, lambda rb: rb + 1, offset=5) == NO_ERROR
            assert check_device_call(dev, data, layout, [1, 0, 1]) == NO_ERROR


def check_device_args(dev, workspace_size):
    name, data = SC.batch_files()[2]
    body, rec, S = records_of(data)
    n = len(rec) - 1
    for layout in LAYOUTS:
        rb = row_bytes(layout, S)
        ok = dict(body=body, rec=rec, S=S, layout=layout, select=None, row_stride=rb, out_cap=n * rb, alloc=n * rb)
        assert dev(**ok)[0] == OK
        assert dev(**dict(ok, ws_short=1))[0] == E_ARG
        assert dev(**dict(ok, S=0))[0] == E_ARG and dev(**dict(ok, S=1 << 30))[0] == E_ARG
        assert dev(**dict(ok, row_stride=rb - 1))[0] == E_ARG
        assert dev(**dict(ok, null="out"))[0] == E_ARG and dev(**dict(ok, null="row_of"))[0] == E_ARG
    assert dev(**dict(ok, layout=3))[0] == E_ARG and dev(**dict(ok, layout=-1))[0] == E_ARG
    assert dev(**dict(ok, n_override=1 << 32))[0] == E_ARG
    assert workspace_size(n, S, BED) > 0
