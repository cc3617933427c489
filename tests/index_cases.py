"""TEST INFRASTRUCTURE ONLY: a plain-Python restatement of the binned external
index (reference create_binned_index4, src/main.cpp:1284-1637;
compute_end_position, :763-852; query_binned_index_binarysearch, :2974-3349;
compare_to_range, :110-137), the loaders of tests/golden/binned_index_cases.json
and generated inputs.  test_index_emu.py checks the restatement against every
golden case (recorded from the reference CLI); it then serves as the expected
value for generated inputs."""
import hashlib
import json
import os
import random
import struct

import golden_io as G

OK, E_ARG, E_FORMAT = 0, 5, 8
M64 = (1 << 64) - 1
ENTRY = 13
CASES_JSON = os.path.join(G.GOLDEN, "binned_index_cases.json")
NAMES = [str(i) for i in range(1, 23)] + ["X", "Y", "M"]


class Throw(Exception):
    """The reference throws here (code 2), or the record is refused (code 3)."""

    def __init__(self, code):
        Exception.__init__(self, "code %d" % code)
        self.code = code


def s64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


def strtoul_whole(b):
    """strtoul(s, &end, 10) with end == s + len required; b"" is 0; None: no parse."""
    if not b:
        return 0
    i, n = 0, len(b)
    while i < n and b[i] in b" \t\n\v\f\r":
        i += 1
    neg = False
    if i < n and b[i] in b"+-":
        neg = b[i] == 0x2D
        i += 1
    j = i
    while j < n and 0x30 <= b[j] <= 0x39:
        j += 1
    if j == i or j != n:
        return None
    v = int(b[i:j])
    if v > M64:
        return M64
    return (-v) & M64 if neg else v


def ref_idx(name):
    """reference_name_map (src/utils.hpp:97-100)."""
    try:
        return NAMES.index(name.decode("latin-1")) + 1
    except ValueError:
        return 0


def split_drop(b, sep):
    """split_string (src/utils.cpp:82-116): empty pieces are dropped."""
    return [x for x in b.split(sep) if x]


def end_position(pos, ref, alt, info):
    """compute_end_position in 64-bit wrap-around arithmetic (unsigned result)."""
    if b"<" not in alt:
        longest = max([len(x) for x in split_drop(alt, b",")] or [0])
        return (pos + max(len(ref), longest) - 1) & M64
    kv = {}
    for pair in split_drop(info, b";"):
        parts = split_drop(pair, b"=")
        if len(parts) == 2:
            kv[parts[0]] = parts[1]
        elif len(parts) == 1:
            kv[parts[0]] = b""
        else:
            raise Throw(2)
    if b"END" in kv:
        best = 0
        for piece in split_drop(kv[b"END"], b","):
            v = strtoul_whole(piece)
            if v is None:
                raise Throw(2)
            best = max(best, s64(v))
        return best & M64
    if b"SVLEN" in kv:
        best = 0
        for piece in split_drop(kv[b"SVLEN"], b","):
            v = strtoul_whole(piece)
            if v is None:
                raise Throw(2)
            a = s64(v)
            a = s64(-a) if a < 0 else a   # std::abs (LONG_MIN stays)
            best = max(best, a)
        return (pos + best - 1) & M64
    return pos


def span(rec):
    """(ref_idx, pos, end) of one record (its bytes from the LEN header on)."""
    tabs, k = [], 8
    while len(tabs) < 8:
        k = rec.find(b"\t", k)
        if k < 0:
            raise Throw(3)
        tabs.append(k)
        k += 1
    f = [rec[8:tabs[0]]] + [rec[tabs[i] + 1:tabs[i + 1]] for i in range(7)]
    pos = strtoul_whole(f[1])
    if pos is None:
        raise Throw(2)
    return ref_idx(f[0]), pos, end_position(pos, f[3], f[4], f[7])


def header_end(v):
    """Offset of the first data byte ('##' lines then one '#' line), or None."""
    p, meta, head = 0, False, False
    while True:
        if p >= len(v):
            return None
        if v[p] != 0x23:
            return p if meta and head else None
        if head or p + 1 >= len(v):
            return None
        if v[p + 1] == 0x23:
            meta = True
        elif not meta:
            return None
        else:
            head = True
        e = v.find(b"\n", p + 2)
        if e < 0:
            return None
        p = e + 1


def record_at(v, p):
    """Length of the well-formed record starting at absolute offset p, or None."""
    if len(v) - p < 8 or (v[p] >> 6) != 3 or (v[p + 4] >> 6) != 3:
        return None
    L = ((v[p] & 0x3F) << 24) | (v[p + 1] << 16) | (v[p + 2] << 8) | v[p + 3]
    if L < 4 or p + 4 + L > len(v):
        return None
    return 4 + L


def pack(entries):
    return b"".join(struct.pack("<BIQ", r, p & 0xFFFFFFFF, o) for r, p, o in entries)


def unpack(index):
    return [struct.unpack_from("<BIQ", index, ENTRY * j) for j in range(len(index) // ENTRY)]


def spans_of(v):
    """[(offset, ref_idx, pos, end)] of every record, or (list so far, failing record)."""
    p = header_end(v)
    if p is None:
        return [], 0
    out = []
    while p < len(v):
        k = record_at(v, p)
        if k is None:
            return out, len(out)
        try:
            out.append((p,) + span(v[p:p + k]))
        except Throw:
            return out, len(out)
        p += k
    return out, None


def sequential_entries(sp, E):
    """The reference's rule (:1430-1482) over [(offset, ref_idx, pos, end)]."""
    ent = []
    for i, (o, r, _, e) in enumerate(sp):
        if not ent:
            ent.append([r, e & 0xFFFFFFFF, o])
        elif i % E == 0:
            if e > ent[-1][1]:
                ent.append([r, e & 0xFFFFFFFF, o])
        elif e > ent[-1][1]:
            ent[-1][1] = e & 0xFFFFFFFF
    return ent


def parallel_entries(sp, E):
    """The parallel form (valid while every end < 2^32): prefix maximum M,
    record i opens iff i == 0 or (i % E == 0 and end_i > M_{i-1})."""
    ent, m = [], 0
    for i, (o, r, _, e) in enumerate(sp):
        if i == 0 or (i % E == 0 and e > m):
            ent.append([r, 0, o])
        m = max(m, e)
        ent[-1][1] = m & 0xFFFFFFFF
    return ent


def build_index(v, E):
    """(status, index bytes, failing record or -1)."""
    if E == 0:
        return E_ARG, b"", -1
    if header_end(v) is None:
        return E_FORMAT, b"", -1
    sp, bad = spans_of(v)
    if bad is not None:
        return E_FORMAT, b"", bad
    return OK, pack(sequential_entries(sp, E)), -1


def search(index, qidx, qstart):
    """The binary search of :3047-3167: (entry or None, stepped back?)."""
    ent = unpack(index)
    if not ent:
        return None, False

    def after(e):
        return e[0] > qidx or (e[0] == qidx and e[1] > qstart)
    lo, hi = 0, len(ent) - 1
    mid = (lo + hi) // 2
    e = ent[0]   # (single-entry index: defined as entry 0)
    while lo < hi:
        mid = (lo + hi) // 2
        e = ent[mid]
        if e[0] == qidx and e[1] == qstart:
            break
        if after(e):
            if mid == 0:
                break
            hi = mid - 1
        else:
            lo = mid + 1
    if mid > 0 and after(e):
        return ent[mid - 1], True
    return e, False


_LINES = {}


def _line(v, h, p, k):
    """The decoded line of the record v[p, p + k) (None: the decode throws)."""
    key = (id(v), len(v))
    if key not in _LINES:
        st, out = G.oracle_decompress(v)
        lines = out[h:].split(b"\n")[:-1] if st == 0 else None
        starts = []
        q = h
        while lines is not None and q < len(v):
            r = record_at(v, q)
            if r is None:
                lines = None
                break
            starts.append(q)
            q += r
        if lines is not None and len(lines) != len(starts):
            lines = None
        _LINES.clear()
        _LINES[key] = dict(zip(starts, lines)) if lines is not None else None
    table = _LINES[key]
    if table is not None and p in table:
        return table[p] + b"\n"
    # this record and up to two more, so a parse that runs on finds the bytes the reference reads
    q = p + k
    for _ in range(2):
        r = record_at(v, q) if q < len(v) else None
        if r is None:
            break
        q += r
    st, out = G.oracle_decompress(v[:h] + v[p:q])
    body = out[h:]
    e = body.find(b"\n")
    return body[:e + 1] if e >= 0 else None


def query(v, index, q):
    """(status, stdout) of the indexed query; q = (ref, has_range, start, end)
    or a coordinate string."""
    if isinstance(q, (bytes, str)):
        q = G.oracle_parse_query(q.encode() if isinstance(q, str) else q)
    name, has_range, start, end = q
    if not has_range:
        start = end = 0
    h = header_end(v)
    if h is None or len(index) % ENTRY:
        return E_FORMAT, b""
    qidx = ref_idx(name)
    e, _ = search(index, qidx, start)
    if e is None:
        return OK, b""
    p = e[2]
    if p >= len(v):
        return OK, b""
    if p < h:
        return E_FORMAT, b""
    out = []
    while p < len(v):
        k = record_at(v, p)
        if k is None:
            return E_FORMAT, b"".join(out)
        try:
            idx, pos, rend = span(v[p:p + k])
        except Throw:
            return E_FORMAT, b"".join(out)
        before = idx < qidx or (idx == qidx and rend < start)
        if not before:
            if idx > qidx or (idx == qidx and pos > end):
                break
            line = _line(v, h, p, k)
            if line is None:
                return E_FORMAT, b"".join(out)
            out.append(line)
        p += k
    return OK, b"".join(out)


# ---- golden cases -----------------------------------------------------------

_cases = None


def cases():
    global _cases
    if _cases is None:
        with open(CASES_JSON) as f:
            _cases = json.load(f)
    return _cases


_files = {}


def file_bytes(name):
    if name not in _files:
        inline = cases()["inline_files"]
        _files[name] = bytes.fromhex(inline[name]) if name in inline else G.gz(name)
    return _files[name]


def golden_index(c):
    """The reference's index bytes of an index case (None where only the hash is stored)."""
    return bytes.fromhex(c["index_hex"]) if "index_hex" in c else None


def index_case(name, bin_size):
    for c in cases()["index_cases"]:
        if c["file"] == name and c["bin"] == bin_size:
            return c
    raise KeyError((name, bin_size))


def sha(b):
    return hashlib.sha256(b).hexdigest()


def check_query_case(c, st, out):
    """A result against a golden query case: exact stdout when the reference
    exits 0; where it aborts (uncaught throw), its stdout is the flushed prefix
    of the lines before the throw."""
    if c["rc"] == 0:
        return st == OK and len(out) == c["stdout_len"] and sha(out) == c["stdout_sha256"]
    return st == E_FORMAT and len(out) >= c["stdout_len"] and sha(out[:c["stdout_len"]]) == c["stdout_sha256"]


# ---- generated inputs ---------------------------------------------------------

HEADER = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"


def header(samples):
    return HEADER + b"".join(b"\tS%d" % i for i in range(samples)) + b"\n"


def gen_lines(n, seed, samples=2, big_end=False):
    """n sorted data lines over CHROM 1, 2, chrZ, X with SNVs, indels, long
    deletions, multi-ALT and structural records (END, SVLEN, neither).
    big_end: one record whose END passes 2^32 (the host replay)."""
    rnd = random.Random(seed)
    chroms = [b"1", b"2", b"chrZ", b"X"]
    out = []
    per = max(1, (n + 3) // 4)
    for i in range(n):
        c = chroms[min(i // per, 3)]
        if i % per == 0:
            pos = 100
        pos += rnd.choice([0, 1, 1, 2, 7, 40])
        r = rnd.random()
        info = b"AC=%d;AF=0.%03d" % (rnd.randrange(1, 9), rnd.randrange(1000))
        ref, alt = rnd.choice(b"ACGT"), rnd.choice(b"ACGT")
        ref, alt = bytes([ref]), bytes([alt])
        if r < 0.05:
            ref = ref + b"ACGT" * rnd.randrange(1, 30)
        elif r < 0.10:
            alt = b",".join(bytes([rnd.choice(b"ACGT")]) * rnd.randrange(1, 9) for _ in range(rnd.randrange(2, 4)))
        elif r < 0.13:
            alt, info = b"<DEL>", b"SVTYPE=DEL;END=%d" % (pos + rnd.randrange(1, 3000))
        elif r < 0.16:
            alt, info = b"<CN0>,<CN2>", b"DB;;SVLEN=-%d,%d;X==" % (rnd.randrange(1, 900), rnd.randrange(1, 900))
        elif r < 0.18:
            alt, info = b"<INS:ME:ALU>", b"SVTYPE=ALU;TSD=null"
        elif r < 0.19:
            ref = ref * 60   # the five TABs leave the fast window
        if big_end and i == n // 2:
            alt, info = b"<DEL>", b"END=%d" % ((1 << 32) + 5 + i)
        gts = b"\t".join(rnd.choice([b"0|0", b"0|1", b"1|0", b"1|1"]) for _ in range(samples))
        out.append(b"%s\t%d\trs%d\t%s\t%s\t%d\tPASS\t%s\tGT\t%s" % (c, pos, i, ref, alt, rnd.randrange(100), info, gts))
    return out


def gen_vcfc(n, seed, samples=2, big_end=False):
    """A .vcfc of gen_lines (the oracle's compress); n == 0 is not a valid file."""
    st, v, _ = G.oracle_compress(header(samples) + b"".join(x + b"\n" for x in gen_lines(n, seed, samples, big_end)))
    assert st == 0
    return v
