"""Decoder inputs for the parity tests (CPU emulator and GPU): valid .vcfc
files from the oracle encoder, and mutations that drive every branch of the
reference's byte-serial decoder (decompress2_data_line, reference
src/compress.cpp:741-986): records whose token count differs from the header,
multi-token and long escapes, NULs in the required columns, zero-count run
bytes, truncation, bad header bits, trailing bytes.  Expected outputs come
from the oracle (pinned to the reference on tests/golden/*decode*).

edge_files(): records built by hand (rec / fill / req_of, shared with
subset_cases.py) at the writer's own edges -- k_dec_write's REQ copy in
256-byte steps, its 256-token LDS tiles and their carry, the 256-byte item
windows, the 2048-byte staged pieces, the light plan's check-while-writing
and the exact re-plan.  Families: req_len, req_nul, req_tabs, tile_edge,
esc_edge, dense, wide, late_bad."""
import functools
import random

import golden_io as G

CLASSES = [b"0|0", b"0|1", b"1|0", b"1|1"]


def header(samples):
    cols = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    if samples:
        cols += b"\tFORMAT" + b"".join(b"\tS%d" % i for i in range(samples))
    return b"##fileformat=VCFv4.2\n" + cols + b"\n"


def rows(rnd, n, samples, escapes=0.0, odd=0.0):
    out = []
    for i in range(n):
        p = rnd.choice([0.0, 0.01, 0.2, 0.9])
        toks = []
        for _ in range(samples):
            r = rnd.random()
            if r < escapes:
                toks.append(rnd.choice([b"2|0", b"0|2", b"1|2", b".|.", b"0/1"]))
            elif r < escapes + odd:
                toks.append(rnd.choice([b"0", b"1|0:35", b"./.:0", b"10|2"]))
            else:
                toks.append(CLASSES[(1 + rnd.randrange(3)) if rnd.random() < p else 0])
        out.append(b"22\t%d\trs%d\tA\tG\t50\tPASS\tAC=%d\tGT\t" % (100 + i, i, i) + b"\t".join(toks))
    return out


def encode_file(samples, lines):
    vcf = header(samples) + b"".join(l + b"\n" for l in lines)
    st, enc, _ = G.oracle_compress(vcf)
    assert st == 0, st
    return enc


def rec(req, samples_bytes, lf=b"\n", reqlen=None, flags=(0xC0, 0xC0)):
    """A record; reqlen / flags: a REQ length field other than len(req), the
    two header bytes' top bits other than 11 (LEN stays right either way)."""
    body = req + samples_bytes + lf
    L = len(body) + 4
    n = len(req) if reqlen is None else reqlen
    return bytes([flags[0] | (L >> 24) & 0x3F, (L >> 16) & 0xFF, (L >> 8) & 0xFF, L & 0xFF, flags[1] | (n >> 24) & 0x3F,
                  (n >> 16) & 0xFF, (n >> 8) & 0xFF, n & 0xFF]) + body


def req_of(i):
    return b"22\t%d\trs%d\tA\tG\t50\tPASS\tAC=%d\tGT\t" % (100 + i, i, i)


def fill(n, code=0x00):
    """n tokens of one class as run bytes (0|0: up to 127 a byte, else 31)."""
    m = 127 if code == 0 else 31
    out = b""
    while n:
        k = min(n, m)
        out += bytes([code | k])
        n -= k
    return out


def valid_files(seed):
    rnd = random.Random(seed)
    files = []
    for S in (1, 3, 64, 256, 300, 513, 2504):   # (tile edges: 256 tokens per decoder tile)
        n = 40 if S < 2504 else 12
        files.append(("S%d" % S, encode_file(S, rows(rnd, n, S))))
    files.append(("escapes", encode_file(200, rows(rnd, 30, 200, escapes=0.05))))
    files.append(("odd_tokens", encode_file(150, rows(rnd, 30, 150, escapes=0.02, odd=0.03))))
    return files


def mutated_files(seed):
    """(name, bytes) pairs: each a valid file with one reference-visible defect."""
    rnd = random.Random(seed)
    S = 120
    base_lines = rows(rnd, 30, S, escapes=0.02)
    out = []
    # header declares more / fewer samples than the rows carry
    for dS in (-7, -1, 1, 5, 200):
        enc = encode_file(S, base_lines)
        body = enc[len(header(S)):]
        out.append(("hdr_samples%+d" % dS, header(S + dS) + body))
    # one row with fewer / more tokens than the header
    for k, extra in ((3, -2), (10, 3), (29, -1)):
        ls = list(base_lines)
        toks = ls[k].split(b"\t")
        toks = toks[:len(toks) + extra] if extra < 0 else toks + [b"0|0"] * extra
        ls[k] = b"\t".join(toks)
        out.append(("row%d_tokens%+d" % (k, extra), encode_file(S, ls)))
    enc = encode_file(S, base_lines)
    h = len(header(S))
    # truncations, trailing bytes
    for cut in (1, 5, 8, 9, 40):
        out.append(("truncate%d" % cut, enc[:-cut]))
    for tail in (b"\x00", b"abc", b"\xc0\x00\x00\x10\xc0\x00\x00"):
        out.append(("tail_%s" % tail.hex(), enc + tail))
    # byte-level corruption inside records (after the headers)
    for j in range(12):
        b = bytearray(enc)
        pos = rnd.randrange(h, len(b))
        b[pos] = rnd.choice([0x00, 0x09, 0x0A, 0x3F, 0x80, 0xA0, 0xC5, 0xE0, 0xE1, 0xE3, 0xFF])
        out.append(("corrupt%d" % j, bytes(b)))
    # hand-built records: NUL in REQ, zero-count runs, 2-token escape, long escape
    req = b"22\t1\trs1\tA\tG\t50\tPASS\tAC=1\tGT\t"
    S2 = 4
    hd = header(S2)
    out.append(("nul_in_req", hd + rec(req[:5] + b"\x00" + req[6:], b"\x04")))
    out.append(("zero_run", hd + rec(req, b"\x00\x04")))
    out.append(("zero_run_1x", hd + rec(req, b"\xa0\x04")))
    out.append(("two_token_escape", hd + rec(req, b"\xe2" + b"2|1\t0|2\t" + b"\x02")))
    out.append(("long_escape", hd + rec(req, b"\xe1" + b"0|1:35:99\t" + b"\x03")))
    out.append(("escape_lf_end", hd + rec(req, b"\x03\xe1" + b"2|2")))
    out.append(("escape_0_tokens", hd + rec(req, b"\xe0\x04")))
    out.append(("overshoot_00", hd + rec(req, b"\x02\x07")))
    out.append(("overshoot_1x", hd + rec(req, b"\x02\x8a")))
    out.append(("req_9tabs_missing", hd + rec(req[:-1], b"\x04")))
    out.append(("S0_row", header(0) + rec(req[:-1].rsplit(b"\t", 1)[0], b"")))
    return out


def query_files(seed):
    """(name, bytes, queries) for the range query (query_compressed_file,
    reference src/main.cpp:3777-3929): valid files with several CHROMs and
    odd POS fields, and mutations that make the reference's walk leave the
    LEN hops (CHROM or POS running past its record, a matched record whose
    parse ends off its hop) or throw (POS that does not parse)."""
    rnd = random.Random(seed)
    S = 40
    lines = []
    for i in range(60):
        chrom = rnd.choice([b"1", b"1", b"2", b"chrX"])   # (the encoder drops empty fields)
        pos = rnd.choice([b"%d" % (100 + 10 * i), b" %d" % (100 + 10 * i), b"+%d" % i, b"0%d" % i])
        toks = [CLASSES[rnd.randrange(4) if rnd.random() < 0.3 else 0] for _ in range(S)]
        lines.append(chrom + b"\t" + pos + b"\trs\tA\tG\t1\tPASS\t.\tGT\t" + b"\t".join(toks))
    enc = encode_file(S, lines)
    h = len(header(S))
    queries = [b"1", b"2:100-400", b"1:0-18446744073709551615", b":150-500", b"chrX:0-0", b"", b"1:300-200"]
    out = [("mixed", enc, queries)]
    # locate the records (LEN hops) to aim the mutations
    recs, p = [], h
    while p + 8 <= len(enc):
        L = ((enc[p] & 0x3F) << 24) | (enc[p + 1] << 16) | (enc[p + 2] << 8) | enc[p + 3]
        recs.append(p)
        p += 4 + L
    def mut(name, k, f):
        b = bytearray(enc)
        f(b, recs[k])
        out.append((name, bytes(b), queries[:4]))
    def retab(b, r, keep):   # TABs of record r past the first `keep` become 'z'
        end = recs[recs.index(r) + 1] if r != recs[-1] else len(b)
        seen = 0
        for j in range(r + 8, end):
            if b[j] == 9:
                seen += 1
                if seen > keep:
                    b[j] = ord("z")
    for k in (0, 17, 59):
        mut("chrom_past%d" % k, k, lambda b, r: retab(b, r, 0))   # CHROM runs into the next record / EOF
        mut("pos_past%d" % k, k, lambda b, r: retab(b, r, 1))     # POS does
        mut("pos_bad%d" % k, k, lambda b, r: b.__setitem__(b.index(b"\t", r + 8) + 1, ord("q")))
    # token counts off the header: matched records whose parse ends off
    # their hop or throws
    for k, extra in ((12, -1), (12, 1), (30, -3)):
        ls = list(lines)
        ls[k] = b"1" + ls[k][ls[k].index(b"\t"):] + (b"\t0|0" * extra if extra > 0 else b"")
        if extra < 0:
            ls[k] = ls[k][:ls[k].rindex(b"\t")] if extra == -1 else b"\t".join(ls[k].split(b"\t")[:extra])
        out.append(("row%d_tokens%+d" % (k, extra), encode_file(S, ls), queries[:4]))
    body = enc[h:]
    for dS in (-1, 2):
        out.append(("hdr_samples%+d" % dS, header(S + dS) + body, queries[:3]))
    for cut in (1, 9, 30):
        out.append(("truncate%d" % cut, enc[:-cut], queries[:3]))
    return out


# ---- hand-built files at the writer's edges ---------------------------------
# The kernel constants they are aimed at (vcfc_decode.hip, vcfc_decode_dev.h):
# token tile TB = 256 tokens; item window 256 bytes from s0 & ~3; staged piece
# SB = 2048 bytes (+ 8 of look-ahead) from rs & ~15; REQ copy 256 bytes a
# step, 4 bytes a lane; DEC_WAVES = 4 records a block; SEL_R = 8 records a
# wave in the selected kernels.

OK, E_FORMAT = 0, 8
EDGE_QUERIES = [b"22", b"22:103-110", b":0-101", b"22:109-109", b"21"]
CODE = {b"0|0": 0x00, b"0|1": 0xA0, b"1|0": 0xC0, b"1|1": 0x80}


def req_len(i, n, rid=None):
    """req_of(i) (its ID `rid` if given) with INFO padded so that REQ is
    exactly n bytes."""
    f = req_of(i).split(b"\t")
    f[2] = f[2] if rid is None else rid
    base = b"\t".join(f)
    assert n >= len(base), (i, n)
    f[7] += b";" + b"x" * (n - len(base) - 1) if n > len(base) else b""
    r = b"\t".join(f)
    assert len(r) == n and r.count(b"\t") == 9
    return r


def items_of(tokens):
    """The sample section of 3-byte tokens: runs of the four classes as run
    bytes, any other token as a one-token escape (the last one ends at the LF)."""
    out, k, n = b"", 0, len(tokens)
    while k < n:
        t = tokens[k]
        if t in CODE:
            m = k
            while m < n and tokens[m] == t:
                m += 1
            out += fill(m - k, CODE[t])
            k = m
        else:
            out += b"\xe1" + t + (b"\t" if k + 1 < n else b"")
            k += 1
    return out


def _mixed(S):
    """S tokens: a 0|0 run, one escape, a 1|0 run (S = 1: the escape alone,
    ending at the LF)."""
    if S == 1:
        return b"\xe12|1"
    return fill(S // 3) + b"\xe12|1\t" + fill(S - S // 3 - 1, 0xC0)


@functools.lru_cache(maxsize=None)
def edge_files():
    """(name, bytes, expected status) -- status 0 for every file but
    late_bad_short, where the reference throws at record 9 and keeps the nine
    lines before it, and req_tabs_*, where it throws at record 2 and keeps two."""
    out = []
    # req_len: REQ lengths around one copy step (256), around one staged piece
    # (2048 less the header and the alignment slack) and well past it; one
    # record each, so consecutive records also sweep the 16 record alignments
    # and the 0..3-byte tail of the copy
    lens = list(range(250, 263)) + list(range(2036, 2060)) + [5000]
    for S in (1, 255, 256, 257, 600):
        body = b"".join(rec(req_len(i, n), _mixed(S)) for i, n in enumerate(lens))
        out.append(("req_len_S%d" % S, header(S) + body, OK))
    # req_nul: REQ' is REQ cut at its first NUL; a light plan took REQ' = REQ
    # and has to be planned again
    S = 300
    its = _mixed(S)
    for nul in ((0,), (3,), (255,), (256,), (257,), (300,), (511,), (512,), (10, 300)):
        r = bytearray(req_len(1, 640, b"rs00000001"))   # (byte 10 lies in the ID: no TAB is lost)
        for k in nul:
            assert r[k] != 9
            r[k] = 0
        out.append(("req_nul_" + "_".join("%d" % k for k in nul),
                    header(S) + rec(req_of(0), its) + rec(bytes(r), its) + rec(req_of(2), its), OK))
    # req_tabs: ten TABs in REQ, nine of them in the copy's first step and the
    # tenth behind it: the reference throws at the record, so a light plan
    # must not stand
    for k in (256, 300, 512):
        r = bytearray(req_len(2, 640).replace(b"\tGT\t", b"xGTx"))
        r[40], r[41], r[k] = 9, 9, 9
        assert bytes(r[:256]).count(b"\t") == 9 and bytes(r).count(b"\t") == 10
        out.append(("req_tabs_%d" % k, header(S) + rec(req_of(0), its) + rec(req_of(1), its) + rec(bytes(r), its) +
                    rec(req_of(3), its), E_FORMAT))
    # tile_edge: a class change at token j, and a 127-token 0|0 run from j - 1
    for S in (257, 512, 513, 769):
        body, i = b"", 0
        for j in (127, 129, 255, 256, 257, 511, 512):
            if j >= S:
                continue
            body += rec(req_of(i), fill(j) + fill(S - j, 0xA0))
            run = min(127, S - (j - 1))
            body += rec(req_of(i + 1), fill(j - 1, 0x80) + fill(run) + fill(S - (j - 1) - run, 0xC0))
            i += 2
        out.append(("tile_edge_S%d" % S, header(S) + body, OK))
    # esc_edge: the escape's flag byte at sample-section offsets around a
    # window's end and a staged piece's end, a record per offset: whatever the
    # record's alignment, one has it last in a window and one last in a piece
    S = 3000
    offs = list(range(244, 268)) + list(range(2030, 2054))
    body = b"".join(rec(req_of(i), b"\x01" * off + b"\xe12|1\t" + fill(S - 1 - off, 0xA0)) for i, off in enumerate(offs))
    out.append(("esc_edge", header(S) + body, OK))
    # dense: half the tokens escapes
    rnd = random.Random(20240611)
    for S in (257, 1025):
        body = b""
        for i in range(20):
            toks = [rnd.choice([b"2|0", b"0|2", b".|.", b"0/1", b"7|7"]) if rnd.random() < 0.5 else CLASSES[rnd.randrange(4)]
                    for _ in range(S)]
            body += rec(req_len(i, len(req_of(i)) + i % 17), items_of(toks))
        out.append(("dense_S%d" % S, header(S) + body, OK))
    # wide: more than 100 tiles out of one 256-byte window
    S = 40000
    for name, its in (("zeros", fill(S)), ("zeros_esc_lf", fill(S - 1) + b"\xe12|2"),
                      ("halves", fill(S // 2) + fill(S // 2, 0xC0))):
        out.append(("wide_" + name, header(S) + b"".join(rec(req_of(i), its) for i in range(3)), OK))
    # late_bad: record 9 of 12 is not simple; at a small output batch the
    # light plan is found wrong with lines already written
    S = 600
    good = fill(299) + b"\xe12|1\t" + fill(200, 0xA0) + fill(100, 0x80)
    for name, its, st in (("short", fill(S - 1, 0x80), E_FORMAT),            # S - 1 tokens
                          ("overshoot", fill(S - 3) + b"\x04", OK),           # S + 1 tokens
                          ("two_token_escape", fill(300) + b"\xe22|1\t0|2\t" + fill(S - 302, 0x80), OK),
                          ("zero_count", fill(254) + b"\x00" + fill(S - 254, 0xA0), OK),
                          ("long_last_escape", fill(S - 1, 0xC0) + b"\xe10|1:35:99", OK)):
        body = b"".join(rec(req_of(i), its if i == 9 else good) for i in range(12))
        out.append(("late_bad_" + name, header(S) + body, st))
    return out


def records_in(data):
    """Records of a .vcfc built by rec() (LEN hops from the end of the header)."""
    p = data.index(b"\n", data.index(b"\n#CHROM") + 1) + 1
    n = 0
    while p + 8 <= len(data):
        p += 4 + (((data[p] & 0x3F) << 24) | (data[p + 1] << 16) | (data[p + 2] << 8) | data[p + 3])
        n += 1
    assert p == len(data)
    return n


def edge_cap(data):
    """An output size no decode or query of an edge file exceeds: per record
    its own bytes, four a token, and a run byte's overshoot."""
    S = data[data.index(b"\n#CHROM") + 1:].split(b"\n", 1)[0].count(b"\t") - 8
    return len(data) + records_in(data) * (4 * S + 1024) + 4096


@functools.lru_cache(maxsize=None)
def edge_expected():
    """{name: (oracle status, decompressed bytes, {query: (oracle status,
    lines)})} of edge_files(), computed once; and what keeps a test from
    passing emptily: the status is the expected one, there is a line per
    record (late_bad_short, req_tabs_*: those before the throw), and a query of every
    file returns a non-empty proper subset of its lines."""
    exp = {}
    for name, data, status in edge_files():
        cap = edge_cap(data)
        st, want = G.oracle_decompress(data, cap=cap)
        assert (st == 0) == (status == OK), (name, st)
        lines = want.count(b"\n") - 2
        kept = 9 if name == "late_bad_short" else 2 if name.startswith("req_tabs") else records_in(data)
        assert lines == kept, (name, lines)
        qs = {q: G.oracle_query(data, q, cap=cap) for q in EDGE_QUERIES}
        assert any(0 < r[1].count(b"\n") < lines for r in qs.values()), name
        exp[name] = (st, want, qs)
    return exp
