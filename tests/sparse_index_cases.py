"""TEST INFRASTRUCTURE ONLY: a plain-Python restatement of the sparse external
index (reference create_sparse_external_index, src/main.cpp:854-999;
query_sparse_external_index, :1002-1281; compute_sparse_offset,
src/sparse.cpp:18-51; compare_to, src/main.cpp:88-108) and of gap-analysis
(:3931-3980), the loaders of tests/golden/sparse_index_cases.json and
generated inputs.  test_sparse_index_emu.py checks the restatement against
every golden case (recorded from the reference CLI); it then serves as the
expected value for generated inputs.

An index is held as {file offset: 13 entry bytes} over its non-zero slots,
with its apparent size."""
import hashlib
import json
import os
import random
import struct

import golden_io as G
import index_cases as X

OK, E_FORMAT = 0, 8
M64 = (1 << 64) - 1
SLOT = 256
MAX_POSITION = 300000000
CASES_JSON = os.path.join(G.GOLDEN, "sparse_index_cases.json")


def slot_offset(pos):
    """compute_sparse_offset with multiplication_factor 1 and block_size 256:
    CHROM is not part of it (VCFC_SPARSE_MULTIPLE_REF_PER_FILE is false)."""
    return ((MAX_POSITION + pos) * SLOT) & M64


def _tabs(rec, k, count):
    out = []
    while len(out) < count:
        k = rec.find(b"\t", k)
        if k < 0:
            raise X.Throw(3)
        out.append(k)
        k += 1
    return out


def create_fields(rec):
    """(ref_idx, pos) of one record under create's rules: five TABs, POS
    parsed after the second, eight TABs and compute_end_position's throws
    only when ALT holds '<'."""
    t = _tabs(rec, 8, 2)
    pos = X.strtoul_whole(rec[t[0] + 1:t[1]])
    if pos is None:
        raise X.Throw(2)
    t += _tabs(rec, t[1] + 1, 3)
    alt = rec[t[3] + 1:t[4]]
    if b"<" in alt:
        t += _tabs(rec, t[4] + 1, 3)
        X.end_position(pos, rec[t[2] + 1:t[3]], alt, rec[t[6] + 1:t[7]])   # for its throws only
    return X.ref_idx(rec[8:t[0]]), pos


def walk_fields(rec):
    """(ref_idx, pos) under the query walk's rules: CHROM and POS only."""
    t = _tabs(rec, 8, 2)
    pos = X.strtoul_whole(rec[t[0] + 1:t[1]])
    if pos is None:
        raise X.Throw(2)
    return X.ref_idx(rec[8:t[0]]), pos


def entry(ref, pos, off):
    return struct.pack("<BIQ", ref, pos & 0xFFFFFFFF, off)


def create(v, limit=1 << 63):
    """(status, {offset: entry}, failing record or -1, seek_failed): entries
    are written one record at a time, so those of the records before the
    first stopping record stay.  limit: the first offset lseek refuses."""
    p = X.header_end(v)
    if p is None:
        return E_FORMAT, {}, -1, 0
    slots, i = {}, 0
    while p < len(v):
        k = X.record_at(v, p)
        if k is None:
            return E_FORMAT, slots, i, 0
        try:
            ref, pos = create_fields(v[p:p + k])
        except X.Throw:
            return E_FORMAT, slots, i, 0
        off = slot_offset(pos)
        if off >= limit:
            return OK, slots, -1, 1
        slots[off] = entry(ref, pos, p)
        p += k
        i += 1
    return OK, slots, -1, 0


def apparent_size(slots):
    return max(slots) + 13 if slots else 0


def lookup(slots, start, end):
    """The entry bytes the lookup of :1069-1174 ends on, or None."""
    size = apparent_size(slots)
    off = slot_offset(start)
    if off >= 1 << 63 or off + 13 > size:
        return None
    if off in slots:
        return slots[off]
    if start == end:
        return None
    later = [o for o in slots if o > off]
    return slots[min(later)] if later else None


def query(v, slots, q):
    """(status, stdout) of query-sparse-index."""
    if isinstance(q, (bytes, str)):
        q = G.oracle_parse_query(q.encode() if isinstance(q, str) else q)
    name, has_range, start, end = q
    if not has_range:
        start = end = 0
    if not slots:   # the SEEK_DATA probe at 10 000 000 fails before the header is read
        return OK, b""
    h = X.header_end(v)
    if h is None:
        return E_FORMAT, b""
    qidx = X.ref_idx(name)
    e = lookup(slots, start, end)
    if e is None:
        return OK, b""
    p = struct.unpack("<BIQ", e)[2]
    if p >= len(v):
        return OK, b""
    if p < h:
        return E_FORMAT, b""
    out = []
    while p < len(v):
        k = X.record_at(v, p)
        if k is None:
            return E_FORMAT, b"".join(out)
        try:
            idx, pos = walk_fields(v[p:p + k])
        except X.Throw:
            return E_FORMAT, b"".join(out)
        before = idx < qidx or (idx == qidx and pos < start)
        if not before:
            if idx > qidx or (idx == qidx and pos > end):
                break
            line = X._line(v, h, p, k)
            if line is None:
                return E_FORMAT, b"".join(out)
            out.append(line)
        p += k
    return OK, b"".join(out)


def compressed_count(rec, S):
    """line_byte_count of decompress2_data_line (src/compress.cpp:764-968) for
    one well-formed record: the 8 header bytes, the required columns and every
    sample-section byte read; the closing LF counts only where it ends an
    uncompressed column (:880-891), the one read at :958 does not."""
    req = ((rec[4] & 0x3F) << 24) | (rec[5] << 16) | (rec[6] << 8) | rec[7]
    cnt, ip, got = 8 + req, 8 + req, 0
    while got < S:
        b = rec[ip]
        ip += 1
        cnt += 1
        if b < 0x80:
            got += b
        elif b & 0xE0 == 0xE0:
            u = 0
            while u < (b & 0x1F):
                x = rec[ip]
                ip += 1
                cnt += 1
                if x == 0x0A:
                    u += 1
                    got += 1
                    ip -= 1
                elif x == 0x09:
                    u += 1
                    got += 1
        else:
            got += b & 0x1F
    return cnt


def gap_analysis(v):
    """(status, text of start-positions.txt, failing record or -1): per record
    "<POS> <decoded line bytes> <compressed count>\n", POS being the second
    non-empty TAB field of the decoded line, verbatim."""
    h = X.header_end(v)
    if h is None:
        return E_FORMAT, b"", -1
    S = len(v[:h].rstrip(b"\n").split(b"\n")[-1].split(b"\t")) - 9
    out, p, i = [], h, 0
    while p < len(v):
        k = X.record_at(v, p)
        line = X._line(v, h, p, k) if k is not None else None
        if line is None:
            return E_FORMAT, b"".join(out), i
        terms = [t for t in line.split(b"\t") if t]
        out.append(b"%s %d %d\n" % (terms[1], len(line), compressed_count(v[p:p + k], max(S, 0))))
        p += k
        i += 1
    return OK, b"".join(out), -1


def slots_digest(slots):
    """sha256 over the ascending (offset, entry) list, offsets as 8 LE bytes."""
    d = hashlib.sha256()
    for o in sorted(slots):
        d.update(struct.pack("<Q", o) + slots[o])
    return d.hexdigest()


def read_sparse_file(path):
    """({offset: entry} over the non-zero 256-byte slots, apparent size) of an
    index file, its holes skipped with SEEK_DATA / SEEK_HOLE."""
    slots = {}
    fd = os.open(path, os.O_RDONLY)
    try:
        size = os.fstat(fd).st_size
        p = 0
        while p < size:
            try:
                a = os.lseek(fd, p, os.SEEK_DATA)
            except OSError:
                break
            b = os.lseek(fd, a, os.SEEK_HOLE)
            a -= a % SLOT
            data = os.pread(fd, b - a, a)
            for o in range(0, len(data), SLOT):
                e = data[o:o + 13]
                if e.strip(b"\0"):
                    slots[a + o] = e + b"\0" * (13 - len(e))
                assert not data[o + 13:o + SLOT].strip(b"\0"), "bytes outside an entry"
            p = b
        return slots, size
    finally:
        os.close(fd)


def write_sparse_file(path, slots, size=None):
    """An index file holding `slots` (a sparse file; size: its apparent size)."""
    fd = os.open(path, os.O_CREAT | os.O_TRUNC | os.O_WRONLY, 0o600)
    try:
        for o in sorted(slots):
            os.pwrite(fd, slots[o], o)
        if size is not None and size != apparent_size(slots):
            os.ftruncate(fd, size)
    finally:
        os.close(fd)


# ---- golden cases -----------------------------------------------------------

_cases = None
_files = {}


def cases():
    global _cases
    if _cases is None:
        with open(CASES_JSON) as f:
            _cases = json.load(f)
    return _cases


def file_bytes(name):
    if name not in _files:
        inline = cases()["inline_files"]
        _files[name] = bytes.fromhex(inline[name]) if name in inline else G.gz(name)
    return _files[name]


def case_slots(c):
    """The reference's slots of a create case (None where only the digest is stored)."""
    if "slots" not in c:
        return None
    return {int(o): bytes.fromhex(e) for o, e in c["slots"]}


def create_case(name):
    for c in cases()["create_cases"]:
        if c["file"] == name:
            return c
    raise KeyError(name)


def check_create_case(c, slots, size):
    """Slots and apparent size against a golden create case."""
    if size != c["size"] or len(slots) != c["n_slots"] or slots_digest(slots) != c["slots_sha256"]:
        return False
    want = case_slots(c)
    return want is None or want == slots


# ---- generated inputs ---------------------------------------------------------

def gen_vcfc(n, seed, pairs=(), samples=2, unsorted=False):
    """A .vcfc of X.gen_lines with POS made strictly increasing across the
    whole file (so no two records share a slot) except that record i + 1
    takes the POS of record i for every i in `pairs`; unsorted: two records
    swap their POS."""
    lines = X.gen_lines(n, seed, samples)
    rnd = random.Random(seed)
    pos, out = 50, []
    ps = []
    for i, l in enumerate(lines):
        if not (i and (i - 1) in pairs):
            pos += rnd.choice([1, 1, 2, 7, 40])
        ps.append(pos)
    if unsorted and n >= 3:
        ps[0], ps[n // 2] = ps[n // 2], ps[0]
    for l, p in zip(lines, ps):
        f = l.split(b"\t")
        f[1] = b"%d" % p
        out.append(b"\t".join(f))
    st, v, _ = G.oracle_compress(X.header(samples) + b"".join(x + b"\n" for x in out))
    assert st == 0
    return v
