"""The wave primitives of vcfc_wave.h stated plainly, and the inputs they are
tried on.

The CPU suite runs the product kernels against tests/simt_emu/vcfc_wave.h, a
twin of vcf-compression_amd/csrc/vcfc_wave.h; its results mean what they
claim only where the twin does what the real header does (hand-written DPP
assembly with hand-counted wait states, raw-buffer loads whose out-of-range
dwords read 0, v_perm, alignbyte, udot4).  tests/wave_probe/wave_probe.hip
calls every primitive from tiny kernels and compiles against either header;
`check(probe)` below holds a build of it to the statements in this file, which
are taken from neither header: integer arithmetic on Python ints, lane by lane.
test_wave_twin.py does that for the twin (g++, the emulator),
test_gpu_wave.py for the real header (gfx950).  All comparisons are exact.

A probe is an object with lanes(a, b), scans(a, b, c), bits(a, b, c, sel),
lds(a, b, c, v), glob(src) and buffer(src, nbytes, off): uint32 arrays of
256 in (thread t = 64 w + l reads [t]), a uint32 array (results, 256) out;
glob gives (results, dst, dst_nt), the two byte arrays preset to 0xEE."""
import random

import numpy as np

NT, M32 = 256, 0xFFFFFFFF
EDGE_LANES = (0, 15, 16, 31, 32, 47, 48, 63)


def vectors():
    """(name, 256 values): all zeros, all ones (1 and every bit), the lane
    index, 0xFFFFFFFF in one lane only of every wave, three seeded random
    vectors and a sparse one (three lanes in four zero)."""
    out = [("zeros", [0] * NT), ("ones", [1] * NT), ("all_bits", [M32] * NT), ("lane", [t & 63 for t in range(NT)])]
    for e in EDGE_LANES:
        out.append(("only%d" % e, [M32 if (t & 63) == e else 0 for t in range(NT)]))
    for seed in (11, 12, 13):
        rnd = random.Random(seed)
        out.append(("random%d" % seed, [rnd.getrandbits(32) for _ in range(NT)]))
    rnd = random.Random(14)
    out.append(("sparse", [rnd.getrandbits(32) if rnd.random() < 0.25 else 0 for _ in range(NT)]))
    return out


def triples():
    """(name, a, b, c): every vector as a, with two others beside it."""
    v = vectors()
    n = len(v)
    out = [(v[i][0], v[i][1], v[(i + 3) % n][1], v[(i + 7) % n][1]) for i in range(n)]
    # a * b + c == a: the scans on each vector itself
    out += [(name + "_self", a, [1] * NT, [0] * NT) for name, a in v]
    return out


def sext24(x):
    x &= 0xFFFFFF
    return x - (1 << 24) if x & 0x800000 else x


def waves(x):
    return [list(x[64 * w:64 * w + 64]) for w in range(4)]


# ---- the statements ---------------------------------------------------------

def want_lanes(a, b):
    rows = [[] for _ in range(20)]
    for x, y in zip(waves(a), waves(b)):
        bal = sum(1 << l for l in range(64) if x[l] & 1)
        for l in range(64):
            lt = (1 << l) - 1
            r = [l, bal & M32, bal >> 32, lt & M32, lt >> 32, x[0]] + [x[e] for e in EDGE_LANES] + [x[y[0] & 63]]
            r.append(x[l - 1] if l else y[0])                    # shr1: lane 0 keeps its own fill
            r.append(x[l - 1] if l else 0)                       # shr1z
            r.append(x[l + 1] if l < 63 else y[63])              # shl1: lane 63 keeps its own fill
            r.append(x[l + 1] if l % 16 != 15 else 0)            # row_shl1: rows of 16 lanes
            r.append(x[y[l] & 63])                               # shfl
            for k, val in enumerate(r):
                rows[k].append(val)
    return rows


def scan(v, f):
    out, acc = [], None
    for x in v:
        acc = x if acc is None else f(acc, x)
        out.append(acc)
    return out


def want_scans(a, b, c):
    rows = [[] for _ in range(11)]
    add = lambda p, q: (p + q) & M32
    last = lambda p, q: q if q else p
    for x, y, z in zip(waves(a), waves(b), waves(c)):
        v = [(p * q + r) & M32 for p, q, r in zip(x, y, z)]
        s1 = scan(v, add)
        s2 = scan(s1, add)
        s3 = scan([p ^ q for p, q in zip(s2, x)], add)
        n1 = scan(v, last)
        n2 = scan(n1, last)
        n3 = scan([p ^ q for p, q in zip(n1, v)], last)
        m1 = scan(v, max)
        m2 = scan(m1, max)
        m3 = scan([(p - q) & M32 for p, q in zip(m1, v)], max)
        w = [(p + q) & M32 for p, q in zip(x, y)]
        d1 = [0] + scan(w, last)[:63]            # shr1z of the scan
        d2 = [z[0]] + scan(w, add)[:63]          # shr1 of the scan, lane 0 keeping its fill
        for k, r in enumerate((s1, s2, s3, n1, n2, n3, m1, m2, m3, d1, d2)):
            rows[k] += r
    return rows


def selectors(seed):
    """Selector words for perm: bytes 0..7 (byte k of s0:s1) and 0x0C (zero),
    the only ones the kernels use."""
    rnd = random.Random(seed)
    pick = list(range(8)) + [0x0C]
    return [sum(rnd.choice(pick) << (8 * i) for i in range(4)) for _ in range(NT)]


def want_bits(a, b, c, sel):
    rows = [[] for _ in range(15)]
    for x, y, z, s in zip(a, b, c, sel):
        xy = (x << 32) | y
        perm = 0
        for i in range(4):
            k = (s >> (8 * i)) & 0xFF
            perm |= (0 if k == 0x0C else (xy >> (8 * k)) & 0xFF) << (8 * i)
        r = [perm,
             (xy >> (z & 31)) & M32,                                  # alignbit
             (xy >> (8 * (z & 3))) & M32,                             # alignbyte
             (z + sext24(x) * sext24(y)) & M32,                       # mad24
             ((x & 0xFFFFFF) * (y & 0xFFFFFF)) & M32,                 # umul24
             (sext24(x) * sext24(y)) & M32,                           # mulsel
             (z + sum(((x >> (8 * i)) & 0xFF) * ((y >> (8 * i)) & 0xFF) for i in range(4))) & M32,   # dot4u
             (x & z) | (y & ~z & M32),                                # bfi
             M32 if (x >> (z & 31)) & 1 else 0,                       # sbit
             (x * y) >> 32,                                           # mulhi
             (x & -x).bit_length() - 1 if x else 0xFF,                # ffbl
             bin(xy).count("1"),                                      # popc64
             xy.bit_length() - 1 if xy else 0xFF,                     # hibit64
             max(x, y),                                               # umax
             (((y << 32) | x) >> (8 * ((z >> 8) % 3 + 1))) & M32]     # alignbyte, shifts 1..3
        for k, val in enumerate(r):
            rows[k].append(val)
    return rows


def want_lds(a, b, c, v):
    rows = [[] for _ in range(8)]
    for x, y, z, val in zip(a, b, c, v):
        m = bytearray([0xEE] * 32)
        o = (x & 1) * (y % 5) + z % 3
        m[1 + o], m[2 + o] = val & 0xFF, (val >> 16) & 0xFF
        m[9 + o], m[10 + o] = (val >> 16) & 0xFF, val & 0xFF
        m[17 + o:21 + o] = val.to_bytes(4, "little")
        for q in range(8):
            rows[q].append(int.from_bytes(m[4 * q:4 * q + 4], "little"))
    return rows


def want_glob(src):
    rows = [[] for _ in range(4)]
    dst, dst_nt = bytearray([0xEE] * (32 * NT)), bytearray([0xEE] * (32 * NT))
    for t in range(NT):
        off = 32 * t + t % 16
        for k in range(4):
            rows[k].append(int.from_bytes(src[off + 4 * k:off + 4 * k + 4], "little"))
        dst[off:off + 16] = src[off:off + 16]
        dst_nt[off:off + 16] = bytes(x ^ 0xFF for x in src[off:off + 16])
    return rows, bytes(dst), bytes(dst_nt)


def want_buffer(src, nbytes, off):
    """A dword at offset o of the range [0, nbytes) reads memory where it lies
    wholly inside the range, else 0; the four dwords of a 16-byte load each
    on their own."""
    dw = lambda o: int.from_bytes(src[o:o + 4], "little") if o + 4 <= nbytes else 0
    rows = [[] for _ in range(10)]
    for o in off:
        r = [dw(o), dw(o + 4), dw(o + 8), dw(o + 12), dw(o)]
        for k, val in enumerate(r + r):
            rows[k].append(val)
    return rows


BUFFER_RANGES = list(range(0, 50)) + list(range(1008, 1042))   # ending at every byte count mod 16, small and past 1 KiB


def buffer_offsets(nbytes):
    """Dword offsets from 64 bytes before the range's end to 92 past it:
    loads inside, straddling the end and past it."""
    base = max(0, (nbytes & ~3) - 64)
    return [base + 4 * (t % 40) for t in range(NT)]


# ---- the check --------------------------------------------------------------

def same(got, want, what):
    got = np.asarray(got, dtype=np.uint32).reshape(len(want), NT)
    want = np.array(want, dtype=np.uint64).astype(np.uint32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "result %d thread %d: got %#x want %#x (%d differ)" % (
        bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])], len(bad)))


def u32(x):
    return np.array(x, dtype=np.uint64).astype(np.uint32)


def check(probe):
    for name, a, b, c in triples():
        same(probe.lanes(u32(a), u32(b)), want_lanes(a, b), "lanes " + name)
        same(probe.scans(u32(a), u32(b), u32(c)), want_scans(a, b, c), "scans " + name)
        sel = selectors(len(name))
        same(probe.bits(u32(a), u32(b), u32(c), u32(sel)), want_bits(a, b, c, sel), "bits " + name)
        v = a[::-1]
        same(probe.lds(u32(a), u32(b), u32(c), u32(v)), want_lds(a, b, c, v), "lds " + name)
    rnd = random.Random(21)
    src = bytes(rnd.randrange(1, 256) for _ in range(32 * NT))
    got, dst, dst_nt = probe.glob(np.frombuffer(src, dtype=np.uint8))
    rows, wdst, wdst_nt = want_glob(src)
    same(got, rows, "global loads")
    assert bytes(dst) == wdst and bytes(dst_nt) == wdst_nt, "global stores"
    src = bytes(rnd.randrange(1, 256) for _ in range(2048))   # no zero byte: a load that ignores the range shows
    for nbytes in BUFFER_RANGES:
        off = buffer_offsets(nbytes)
        same(probe.buffer(np.frombuffer(src, dtype=np.uint8), nbytes, u32(off)), want_buffer(src, nbytes, off),
             "buffer loads, range %d" % nbytes)
