"""Sparse-layout inputs for the parity tests (CPU emulator and GPU): a plain
statement of sparsify_file (reference src/sparse.cpp:290-580) and hand-built
.vcfc files at the edges of k_sparse_plan (csrc/vcfc_sparse.hip) and of the
host code that writes its plan (sparse_plan_range, sparse_write_range,
vcfc_sparsify_file, vcfc_sparsify_shard in csrc/vcfc_api.cpp).

The statement is pure Python over unbounded ints, reduced mod 2^64 where the
format is (offsets and distances are uint64); it never calls the code under
test.  pos_of / plan / slice_plan say what the plan kernel owes, image() the
writes the reference's loop leaves in the file.

Families, each a list of (name, .vcfc bytes): pos_forms (every form of the
POS text and of a body with too few TABs), adjacent (a record ending one byte
short of, at, and one byte into the next record's slot; duplicate and
decreasing POS; a record over two slots), block_edge (record counts and
defects around the kernel's 256-thread blocks), err_order (several
unparsable records: the lowest is reported), tail_bad (bytes after the last
whole record).  A case is disk-bound when every POS in it is below 10^6, so
its file stays near 4.9 TB as the committed fixtures do; the others (POS -1,
2^64 - 1, an offset that wraps below data_start) go to the plan entry only."""
import functools
import hashlib
import json
import os
import random
import tempfile

import decode_cases as D
import sparse_digest

M64 = (1 << 64) - 1
SPARSE_L, STRIDE = 300000000, 4 * 4096
OK, E_FORMAT = 0, 8
NONE = M64
DISK_POS_LIMIT = 10 ** 6
SPACE = b" \t\n\v\f\r"


# ---- the plain statement ----------------------------------------------------

def header_end(v):
    p = 0
    while v[p:p + 1] == b"#":
        p = v.index(b"\n", p) + 1
    return p


def split(v):
    """(header bytes, [whole records], tail_ok) as the reference's read loop
    takes them: 8 header bytes (none left: the end; fewer than 8, or top bits
    other than 11: a throw), then LEN - 4 bytes (EOF before that: a throw)."""
    h = header_end(v)
    recs, p = [], h
    while True:
        if p == len(v):
            return v[:h], recs, True
        hd = v[p:p + 8]
        if len(hd) < 8 or hd[0] >> 6 != 3 or hd[4] >> 6 != 3:
            return v[:h], recs, False
        L = ((hd[0] & 0x3F) << 24) | (hd[1] << 16) | (hd[2] << 8) | hd[3]
        if L < 4 or p + 8 + L - 4 > len(v):
            return v[:h], recs, False
        recs.append(v[p:p + 8 + L - 4])
        p += 8 + L - 4


def strtoul_whole(s):
    """strtoul(s, &end, 10) with end required at the end of s; None = not so."""
    i = 0
    while i < len(s) and s[i] in SPACE:
        i += 1
    neg = s[i:i + 1] == b"-"
    if s[i:i + 1] in (b"+", b"-"):
        i += 1
    digits = s[i:]
    if not digits or not all(0x30 <= c <= 0x39 for c in digits):
        return None
    val = int(digits)
    if val > M64:
        return M64                      # overflow saturates, whatever the sign
    return (-val) & M64 if neg else val


def pos_of(body):
    """POS of a record body (the bytes behind its 8 header bytes), None where
    the reference throws: an empty CHROM or POS before its TAB throws, a CHROM
    or POS that is never TAB-terminated leaves POS 0, the whole POS field has
    to be taken by strtoul."""
    t1 = body.find(b"\t")
    if t1 < 0:
        return 0
    if t1 == 0:
        return None
    t2 = body.find(b"\t", t1 + 1)
    if t2 < 0:
        return 0
    if t2 == t1 + 1:
        return None
    return strtoul_whole(body[t1 + 1:t2])


def offset_of(pos, data_start):
    return (data_start + (SPARSE_L + pos) * STRIDE) & M64


def be64(x):
    return (x & M64).to_bytes(8, "big")


def plan(records, data_start):
    """(file_off[], prefix16[], first_bad or None, anomaly) of a record list.
    With k = first_bad (n where none): file_off and prefix16 have k entries;
    prefix16[i] = (dist_to_prev, dist_to_next), dist_to_prev measured from
    data_start for record 0, dist_to_next 0 for the last record and None for
    record k - 1 < n - 1 (its neighbour has no offset; the file keeps 0 there).
    anomaly: an offset below data_start, or an adjacent pair that is not
    strictly increasing or overlaps (off_i + 16 + len_i > off_{i+1}), or a
    record followed by an unparsable one -- the one-write-per-record plan is
    then not what the reference's write sequence leaves."""
    n = len(records)
    off = []
    for r in records:
        p = pos_of(r[8:])
        off.append(None if p is None else offset_of(p, data_start))
    first_bad = next((i for i in range(n) if off[i] is None), None)
    k = n if first_bad is None else first_bad
    prefix = []
    for i in range(k):
        prev = data_start if i == 0 else off[i - 1]
        nxt = be64(0) if i + 1 == n else None if i + 1 == k else be64(off[i + 1] - off[i])
        prefix.append((be64(off[i] - prev), nxt))
    anomaly = False
    for i in range(n):
        if off[i] is None:
            continue
        anomaly |= off[i] < data_start
        if i + 1 < n:
            anomaly |= off[i + 1] is None or off[i + 1] <= off[i] or off[i] + 16 + len(records[i]) > off[i + 1]
    return off[:k], prefix, first_bad, anomaly


def slice_plan(records, data_start, a, b):
    """plan() over records [a, b) only, as a shard sees them (first_bad is
    local to a)."""
    return plan(records[a:b], data_start)


def shard_info(records, rank, world, data_start):
    """[lo, hi, first_err (global) or None, anomaly] that vcfc_sparsify_shard
    owes for a file whose bytes all belong to whole records: the slice plan
    over the rank's records and one halo record each side."""
    n = len(records)
    lo, hi = n * rank // world, n * (rank + 1) // world
    if hi == lo:
        return [lo, hi, None, 0]
    a, b = max(lo - 1, 0), min(hi + 1, n)
    _, _, bad, anomaly = slice_plan(records, data_start, a, b)
    return [lo, hi, None if bad is None else a + bad, int(anomaly)]


def image(v):
    """(status, writes): the reference's write sequence over .vcfc bytes v as
    an ordered list of (offset, bytes) -- later writes win where they overlap,
    so the order is part of the statement.  The header lines and the zeroed
    8-byte slot; per record the first-offset slot (record 0, little endian) or
    the patch of the previous record's bytes 8..15, then the record behind its
    prefix with dist_to_next = 0.  It stops at the first throw.  A file that
    ends behind its header lines is a throw of the header reader, which runs
    before anything is written: the output is created and left empty."""
    hdr, records, tail_ok = split(v)
    if len(v) == len(hdr):
        return E_FORMAT, []
    data_start = len(hdr) + 8
    writes = [(0, hdr + b"\0" * 8)]
    prev = data_start
    for i, r in enumerate(records):
        p = pos_of(r[8:])
        if p is None:
            return E_FORMAT, writes
        off = offset_of(p, data_start)
        if i == 0:
            writes.append((data_start - 8, ((off - data_start) & M64).to_bytes(8, "little")))
        else:
            writes.append((prev + 8, be64(off - prev)))
        writes.append((off, be64(off - prev) + be64(0) + r))
        prev = off
    return (OK if tail_ok else E_FORMAT), writes


def write_image(writes, path):
    fd = os.open(path, os.O_CREAT | os.O_TRUNC | os.O_RDWR, 0o600)
    try:
        for off, b in writes:
            assert os.pwrite(fd, b, off) == len(b)
    finally:
        os.close(fd)


@functools.lru_cache(maxsize=None)
def image_digest(v):
    """(status, hole-aware digest) of image(v), through a sparse temp file."""
    st, writes = image(v)
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        p = os.path.join(d, "image.sparse")
        write_image(writes, p)
        return st, sparse_digest.digest(p)


def same_as_image(v, status, path):
    """Whether (status, the file at path) is what image(v) says."""
    st, dg = image_digest(v)
    return status == st and sparse_digest.digest(path) == dg


def check_plan(name, v, fo, pf, st):
    """The plan contract, for the emulator and the GPU alike (fo: n offsets,
    pf: 16 n prefix bytes, st: the two status words, all as the kernel left
    them).  With k = first_bad (n where nothing fails): status[0] is exact;
    file_off[i] and prefix bytes 0..7 are exact for i < k, bytes 8..15 for
    i + 1 < k and for the last record of the file.

    For i = k - 1 < n - 1 the planned dist_to_next is NOT compared: the kernel
    has no offset for the failing neighbour.  status[1] != 0 is required
    instead.  sparse_write_range rests on exactly this: the flag sends it down
    the replay branch, which writes every dist_to_next as 0 and patches it from
    the next record's step, so the last record written keeps 0 as it does in
    the reference, which throws before patching."""
    _, records, _ = split(v)
    n = len(records)
    off, prefix, bad, anomaly = plan(records, data_start_of(v))
    k = n if bad is None else bad
    assert int(st[0]) == (NONE if bad is None else (bad << 8) | E_FORMAT), (name, hex(int(st[0])), bad)
    for i in range(k):
        assert int(fo[i]) == off[i], (name, i, int(fo[i]), off[i])
        assert bytes(pf[16 * i:16 * i + 8]) == prefix[i][0], (name, i, "dist_to_prev")
        if prefix[i][1] is not None:
            assert bytes(pf[16 * i + 8:16 * i + 16]) == prefix[i][1], (name, i, "dist_to_next")
    if bad is None:
        assert (int(st[1]) != 0) == anomaly, (name, int(st[1]), anomaly)
    elif 1 <= k:
        assert int(st[1]) != 0, (name, "record %d is written last: the writer needs the replay branch" % (k - 1))


def data_start_of(v):
    return header_end(v) + 8


def rec_offsets(records):
    ro = [0]
    for r in records:
        ro.append(ro[-1] + len(r))
    return ro


def is_disk(v):
    _, records, _ = split(v)
    return all((pos_of(r[8:]) or 0) < DISK_POS_LIMIT for r in records)


# ---- the families -----------------------------------------------------------

S = 2
HDR = D.header(S)
ITS = D.fill(S)


def prec(pos_text, i=0, chrom=b"22"):
    """A short record whose second column is pos_text."""
    return D.rec(chrom + b"\t" + pos_text + b"\trs%d\tA\tG\t50\tPASS\tAC=%d\tGT\t" % (i, i), ITS)


VALID_DISK = [b"0", b"7", b"0012", b"+7", b" 9", b"\v\f\r9", b"-0"]
VALID_PLAN_ONLY = [b"-1", b"18446744073709551615", b"18446744073709551616", b"1234567890123456789012345",
                   b"-1234567890123456789012345"]
FAILING = [b"", b"+", b"-", b" ", b"1 ", b"12a", b"0x10", b"1.5"]
WRAP_POS = (1 << 50) - 1 - SPARSE_L      # (L + POS) * 16384 = 2^64 - 16384
BIG_HDR = b"##fileformat=VCFv4.2\n##pad=" + b"x" * 20000 + b"\n" + HDR.split(b"\n", 1)[1]


def _tag(t):
    return t.hex() or "empty"


@functools.lru_cache(maxsize=None)
def pos_forms():
    out = []
    for t in VALID_DISK:                  # one POS text ahead of a plain record
        out.append(("ok_" + _tag(t), HDR + prec(t, 0) + prec(b"20", 1)))
    out.append(("ok_all", HDR + b"".join(prec(t, i) for i, t in enumerate(VALID_DISK))))
    for t in VALID_PLAN_ONLY:
        out.append(("huge_" + t.decode().replace("-", "neg"), HDR + prec(b"5", 0) + prec(t, 1) + prec(b"20", 2)))
    # an offset below data_start: the header is longer than one slot
    out.append(("wrap_alone", BIG_HDR + prec(b"%d" % WRAP_POS, 0)))
    out.append(("wrap_first", BIG_HDR + prec(b"%d" % WRAP_POS, 0) + prec(b"%d" % (WRAP_POS + 2), 1)))
    # the last slot of the 2^64 offset space under a record longer than a slot:
    # off + 16 + len passes 2^64, so in uint64 arithmetic the overlap with the
    # next record does not show and only "not increasing" flags the pair
    long_req = b"22\t%d\trs0\tA\tG\t50\tPASS\tAC=0;" % WRAP_POS + b"x" * 20000 + b"\tGT\t"
    out.append(("wrap_long", HDR + D.rec(long_req, ITS) + prec(b"20", 1)))
    for t in FAILING:                     # each failing text in the middle of three
        out.append(("bad_" + _tag(t), HDR + prec(b"5", 0) + prec(t, 1) + prec(b"20", 2)))
    out.append(("bad_chrom", HDR + prec(b"5", 0) + prec(b"7", 1, chrom=b"") + prec(b"20", 2)))
    out.append(("bad_first", HDR + prec(b"12a", 0) + prec(b"20", 1)))
    out.append(("bad_last", HDR + prec(b"5", 0) + prec(b"12a", 1)))
    out.append(("bad_only", HDR + prec(b"", 0)))
    # too few TABs: POS stays 0 and nothing throws
    notab = D.rec(b"22 7 rs1 A G 50 PASS AC=1 GT ", ITS)
    onetab = D.rec(b"22\t7 rs1 A G 50 PASS AC=1 GT ", ITS)
    for name, r in (("notab", notab), ("onetab", onetab)):
        assert pos_of(r[8:]) == 0
        out.append((name + "_first", HDR + r + prec(b"20", 1)))
        out.append((name + "_middle", HDR + prec(b"5", 0) + r + prec(b"20", 2)))
    return out


@functools.lru_cache(maxsize=None)
def adjacent():
    out = []
    for d in (1, 2):
        for e, tag in ((-1, "m1"), (0, "eq"), (1, "p1")):
            # 16 prefix bytes + 8 header bytes + REQ + the run byte + LF = d * 16384 + e
            first = D.rec(D.req_len(0, d * STRIDE + e - 16 - 8 - len(ITS) - 1), ITS)
            assert 16 + len(first) == d * STRIDE + e
            v = HDR + first + D.rec(D.req_of(d), ITS) + D.rec(D.req_of(d + 5), ITS)
            _, _, bad, anomaly = plan(split(v)[1], data_start_of(v))
            # the required edge: touching is not overlapping
            assert bad is None and anomaly == (e > 0), (d, e, anomaly)
            out.append(("d%d_%s" % (d, tag), v))
    out.append(("duplicate", HDR + D.rec(D.req_of(0), ITS) + D.rec(D.req_len(0, 60, b"rsdup"), ITS) +
                D.rec(D.req_of(2), ITS)))
    out.append(("decreasing", HDR + D.rec(D.req_of(5), ITS) + D.rec(D.req_of(3), ITS) + D.rec(D.req_of(10), ITS)))
    out.append(("swallow2", HDR + D.rec(D.req_len(0, 2 * STRIDE + 100), ITS) + D.rec(D.req_of(1), ITS) +
                D.rec(D.req_of(2), ITS) + D.rec(D.req_of(10), ITS)))
    return out


BLOCK_N = (1, 2, 3, 255, 256, 257, 512, 513)
DEFECTS = ("dec", "dup", "bad")


def block_file(n, defect=None, at=()):
    """n short records at POS 1000 + 2 i; `defect` at each index of `at`: POS
    one below the record before (dec), equal to it (dup), or unparsable (bad)."""
    recs = []
    for i in range(n):
        t = b"%d" % (1000 + 2 * i)
        if i in at:
            t = {"dec": b"%d" % (1000 + 2 * (i - 1) - 1), "dup": b"%d" % (1000 + 2 * (i - 1)), "bad": b"12a"}[defect]
        recs.append(prec(t, i))
    return HDR + b"".join(recs)


@functools.lru_cache(maxsize=None)
def block_edge():
    out = [("n0", HDR)]
    for n in BLOCK_N:
        out.append(("n%d" % n, block_file(n)))
    for n in BLOCK_N:
        if n < 257:
            continue
        for at in (254, 255, 256, 257):
            if at < n:
                for k in DEFECTS:
                    out.append(("n%d_%s%d" % (n, k, at), block_file(n, k, (at,))))
    return out


@functools.lru_cache(maxsize=None)
def err_order():
    """(name, bytes); the failing records are in different blocks and the
    lowest is neither the first nor the last of them."""
    out = []
    for n, at in ((513, (300, 40, 511)), (513, (300, 40)), (513, (0, 300)), (513, (512,)), (513, (40, 512)),
                  (513, (0,)), (257, (256, 255)), (1, (0,))):
        out.append(("n%d_" % n + "_".join("%d" % k for k in at), block_file(n, "bad", at)))
    return out


@functools.lru_cache(maxsize=None)
def tail_bad():
    good = block_file(5)
    r = prec(b"2000", 9)
    out = [("partial1", good + r[:1]), ("partial7", good + r[:7]),
           ("flags_len", good + D.rec(b"22\t2000\trs9\tA\tG\t50\tPASS\tAC=9\tGT\t", ITS, flags=(0x80, 0xC0))),
           ("flags_req", good + D.rec(b"22\t2000\trs9\tA\tG\t50\tPASS\tAC=9\tGT\t", ITS, flags=(0xC0, 0x40)) +
            prec(b"2002", 10)),
           ("len_past_eof", good + r[:-1]), ("header_only_rec", good + r[:8]),
           ("empty_partial", HDR + r[:3]),
           # the defect in the first record: no record is whole
           ("first_flags", HDR + D.rec(b"22\t2000\trs9\tA\tG\t50\tPASS\tAC=9\tGT\t", ITS, flags=(0x40, 0xC0))),
           ("first_len_past_eof", HDR + r[:-1])]
    return out


FAMILIES = {"pos_forms": pos_forms, "adjacent": adjacent, "block_edge": block_edge, "err_order": err_order,
            "tail_bad": tail_bad}


@functools.lru_cache(maxsize=None)
def all_cases():
    """[(family/name, bytes, disk_bound)] of every family, with what keeps a
    test from passing emptily asserted once: each family has an expected-clean
    and an expected-anomaly case (err_order and tail_bad apart: theirs is the
    status), err_order and pos_forms each have first_bad at 0, in the interior
    and last, plan-only cases exist, and no disk-bound offset reaches 2^43."""
    out = []
    for fam, f in FAMILIES.items():
        clean = anom = 0
        where = set()
        for name, v in f():
            _, records, tail_ok = split(v)
            off, _, bad, anomaly = plan(records, data_start_of(v))
            disk = is_disk(v)
            if disk:
                assert all(o < 1 << 43 for o in off), (fam, name)
            if bad is None:
                clean += not anomaly
                anom += anomaly
            else:
                where.add("first" if bad == 0 else "last" if bad == len(records) - 1 else "interior")
            if fam == "tail_bad":
                assert not tail_ok and bad is None and image(v)[0] == E_FORMAT, name
            out.append((fam + "/" + name, v, disk))
        if fam in ("pos_forms", "adjacent", "block_edge"):
            assert clean and anom, (fam, clean, anom)
        if fam in ("pos_forms", "err_order"):
            assert where == {"first", "interior", "last"}, (fam, where)
    assert len(set(c[0] for c in out)) == len(out)
    assert sum(not c[2] for c in out) >= 3
    return out


def disk_cases():
    return [(name, v) for name, v, disk in all_cases() if disk]


def golden_cases():
    """The disk-bound cases the reference's own `main sparsify` is recorded on
    (tests/golden/sparse_edge_cases.json): pos_forms, adjacent, err_order,
    tail_bad, block_edge at n = 257 with each defect, and the header-only file."""
    return [(name, v) for name, v in disk_cases()
            if not name.startswith("block_edge/") or name.startswith("block_edge/n257_") or name == "block_edge/n0"]


def sha(v):
    return hashlib.sha256(v).hexdigest()


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/sparse_edge_cases.json: {case: {input_sha256, rc, digest}}
    of the reference's own `main sparsify`; every golden case is recorded."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_edge_cases.json")) as f:
        g = json.load(f)["cases"]
    assert sorted(g) == sorted(name for name, _ in golden_cases())
    return g


def ref_exit_code(name):
    """The recorded exit code of the reference as a shell reports it (an
    uncaught throw is SIGABRT: -6 to a Python parent, 134 to a shell)."""
    rc = golden()[name]["rc"]
    return 134 if rc == -6 else rc


def check_golden(name, v, status, digest):
    """(status, digest) of a sparsify of v against the reference's record."""
    c = golden()[name]
    assert c["input_sha256"] == sha(v), (name, "the case drifted from the recorded input")
    assert ref_exit_code(name) in (0, 134) and (status == OK) == (c["rc"] == 0), (name, status, c["rc"])
    assert status in (OK, E_FORMAT), (name, status)
    if c["digest"] is not None:
        assert digest == c["digest"], (name, digest, c["digest"])


# ---- the mutated sparse file of the query tests -------------------------------

MUTATED_QUERIES = [b"1:10000-10200", b"1:10010-10050", b"1:10040-10040", b"1:10001-10090", b"1:10100-10100"]


def mutate_random_sparse(path, seed):
    """Six random byte patches in the distance prefixes, record headers and
    bodies of the sparse file of random_100x10000 at `path` (walk errors,
    off-hop parses, bad POS fields); the same bytes for a seed everywhere."""
    import golden_io as G
    rnd = random.Random(seed)
    ds = data_start_of(G.gz("random_100x10000.vcfc.gz"))
    with open(path, "r+b") as f:
        for _ in range(6):
            k = rnd.randrange(0, 60)
            slot = ds + (SPARSE_L + 10000 + 2 * k) * STRIDE
            off = slot + rnd.choice([rnd.randrange(0, 16), rnd.randrange(16, 24), rnd.randrange(24, 400)])
            f.seek(off)
            f.write(bytes([rnd.randrange(256)]))


def span_queries(v):
    """Sparse-file queries over a disk-bound case: each record's own POS and
    the whole span of the file."""
    _, records, _ = split(v)
    pos = [pos_of(r[8:]) for r in records]
    qs = [b"22:%d-%d" % (p, p) for p in dict.fromkeys(pos)]
    return qs + [b"22:%d-%d" % (min(pos), max(pos)), b"22:0-%d" % (max(pos) + 5)]


# ---- shard files: a defect on and next to every shard bound -------------------

SHARD_WORLDS = (2, 3, 5)
SHARD_N = (257, 513)


@functools.lru_cache(maxsize=None)
def shard_files():
    """(name, bytes): block_edge files of 257 and 513 records, clean and with
    one defect at each index from two below to one above every shard bound
    n * r // world -- the bound itself is the lower rank's halo record `hi`,
    the index below it the upper rank's halo record `lo - 1`, and the two
    outer indexes lie one record outside a halo."""
    out = []
    for n in SHARD_N:
        out.append(("n%d" % n, block_file(n)))
        idx = sorted({n * r // w + dlt for w in SHARD_WORLDS for r in range(1, w) for dlt in (-2, -1, 0, 1)})
        for at in idx:
            for k in DEFECTS if n == 257 else ("dec", "bad"):
                out.append(("n%d_%s%d" % (n, k, at), block_file(n, k, (at,))))
    return out
