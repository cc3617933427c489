"""The wave header the kernels are built with (csrc/vcfc_wave.h, gfx950)
against the plain statement of every primitive (wave_cases.py): the probe
kernels (tests/wave_probe/wave_probe.hip) as build/libvcfc_waveprobe.so, made
by the product Makefile beside libvcfc.so with the same flags.
test_wave_twin.py holds the emulated twin to the same statements."""
import ctypes
import os

import numpy as np
import pytest

import golden_io as G
import wave_cases as WC

pytestmark = pytest.mark.gpu
SO = os.path.join(G.REPO, "build", "libvcfc_waveprobe.so")
DEV = "cuda:0"


class Probe:
    """The probe's launchers over torch tensors on the current stream."""

    def __init__(self, torch, lib):
        self.torch, self.lib = torch, lib
        for name, n in (("lanes", 3), ("scans", 4), ("bits", 5), ("lds", 5), ("global", 4)):
            getattr(lib, "wave_probe_" + name).argtypes = [ctypes.c_void_p] * (n + 1)
        lib.wave_probe_buffer.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def dev(self, x):
        x = np.ascontiguousarray(x)
        return self.torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x.copy()).to(DEV)

    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def run(self, name, rows, *arrays):
        d = [self.dev(x) for x in arrays]
        out = self.torch.zeros((rows, WC.NT), dtype=self.torch.int32, device=DEV)
        assert getattr(self.lib, "wave_probe_" + name)(*[x.data_ptr() for x in d], out.data_ptr(), self.stream()) == 0
        return out.cpu().numpy().view(np.uint32), d

    def lanes(self, a, b):
        return self.run("lanes", 20, a, b)[0]

    def scans(self, a, b, c):
        return self.run("scans", 11, a, b, c)[0]

    def bits(self, a, b, c, sel):
        return self.run("bits", 15, a, b, c, sel)[0]

    def lds(self, a, b, c, v):
        return self.run("lds", 8, a, b, c, v)[0]

    def glob(self, src):
        dst = np.full(32 * WC.NT, 0xEE, dtype=np.uint8)
        out, d = self.run("global", 4, src, dst, dst)
        return out, d[1].cpu().numpy().tobytes(), d[2].cpu().numpy().tobytes()

    def buffer(self, src, nbytes, off):
        d_src, d_off = self.dev(src), self.dev(off)
        out = self.torch.zeros((10, WC.NT), dtype=self.torch.int32, device=DEV)
        assert self.lib.wave_probe_buffer(d_src.data_ptr(), nbytes, d_off.data_ptr(), out.data_ptr(), self.stream()) == 0
        return out.cpu().numpy().view(np.uint32)


def test_header_matches_the_plain_statements():
    import torch   # before the probe: one HIP runtime in the process
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert os.path.exists(SO), "libvcfc_waveprobe.so not built: run `make -C vcf-compression_amd`"
    WC.check(Probe(torch, ctypes.CDLL(SO)))
