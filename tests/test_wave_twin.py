"""The emulated twin of the wave header (tests/simt_emu/vcfc_wave.h) against
the plain statement of every primitive (wave_cases.py): the probe kernels
(tests/wave_probe/wave_probe.hip) built with g++ against the fiber SIMT
emulator.  test_gpu_wave.py holds the real header (csrc/vcfc_wave.h, gfx950)
to the same statements; together they say that what the CPU suite computes
with the twin is what the GPU computes."""
import ctypes
import fcntl
import os
import subprocess

import numpy as np

import wave_cases as WC

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wave_probe")
SO = os.path.join(HERE, "_build", "libwave_probe_emu.so")


class Probe:
    """The probe's launchers over numpy arrays."""

    def __init__(self, lib):
        self.lib = lib
        for name, n in (("lanes", 3), ("scans", 4), ("bits", 5), ("lds", 5), ("global", 4)):
            getattr(lib, "wave_probe_" + name).argtypes = [ctypes.c_void_p] * (n + 1)
        lib.wave_probe_buffer.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def run(self, name, rows, *arrays):
        arrays = [np.ascontiguousarray(x) for x in arrays]
        out = np.zeros((rows, WC.NT), dtype=np.uint32)
        assert getattr(self.lib, "wave_probe_" + name)(*[x.ctypes.data for x in arrays], out.ctypes.data, None) == 0
        return out

    def lanes(self, a, b):
        return self.run("lanes", 20, a, b)

    def scans(self, a, b, c):
        return self.run("scans", 11, a, b, c)

    def bits(self, a, b, c, sel):
        return self.run("bits", 15, a, b, c, sel)

    def lds(self, a, b, c, v):
        return self.run("lds", 8, a, b, c, v)

    def glob(self, src):
        dst = np.full(32 * WC.NT, 0xEE, dtype=np.uint8)
        dst_nt = np.full(32 * WC.NT, 0xEE, dtype=np.uint8)
        out = self.run("global", 4, src, dst, dst_nt)   # (run keeps contiguous arrays as they are: written in place)
        return out, dst.tobytes(), dst_nt.tobytes()

    def buffer(self, src, nbytes, off):
        src, off = np.ascontiguousarray(src), np.ascontiguousarray(off)
        out = np.zeros((10, WC.NT), dtype=np.uint32)
        assert self.lib.wave_probe_buffer(src.ctypes.data, nbytes, off.ctypes.data, out.ctypes.data, None) == 0
        return out


def lib():
    os.makedirs(os.path.dirname(SO), exist_ok=True)
    with open(SO + ".lock", "w") as lk:   # one build at a time (pytest -n workers)
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.run(["make", "-s", "-C", HERE], check=True)
    return ctypes.CDLL(SO)


def test_twin_matches_the_plain_statements():
    WC.check(Probe(lib()))


def test_statements_are_not_vacuous():
    """The inputs reach the cases the statements distinguish: a scan whose
    back-to-back result differs from its first, a last-non-zero scan with
    zeros to fill, buffer dwords on both sides of a range's end."""
    name, a, b, c = next(t for t in WC.triples() if t[0] == "sparse_self")
    s = WC.want_scans(a, b, c)
    assert s[0] != s[1] and s[3] != [x for x in a] and 0 in a and any(s[3])
    r = WC.want_buffer(bytes(range(1, 201)), 37, WC.buffer_offsets(37))
    assert 0 in r[0] and any(r[0]) and any(x and not y for x, y in zip(r[0], r[1]))   # a 16-byte load straddling the end
    assert sorted(set(n % 16 for n in WC.BUFFER_RANGES)) == list(range(16))
