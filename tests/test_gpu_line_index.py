"""The line index kernels (csrc/vcfc_ingest.hip) on the GPU against a plain
line split (line_index_cases.plain_index), mode by mode: counts, all seven
tables and the recorded line ends of every family of line_index_cases.py
under every configuration, through the probe (tests/line_probe, built as
build/libvcfc_lineprobe.so beside libvcfc.so and linked against it, so the
kernels are the product's own code objects).

Each buffer starts 0, 1 and 15 bytes past a 16-byte boundary (compress_device
hands the kernels d_in + pos at any alignment) inside an allocation with 4 KiB
of slack on both sides, filled once with '\\n' bytes and once with "\\t0|0"
repeated: the tables may not depend on bytes outside [0, n).  The workspaces
are poisoned before every run.  test_line_index_emu.py runs the same cases on
the emulator and also counts the walkers' steps."""
import ctypes
import os

import numpy as np
import pytest

import golden_io as G
import line_index_cases as C

pytestmark = pytest.mark.gpu
SO = os.path.join(G.REPO, "build", "libvcfc_lineprobe.so")
DEV = "cuda:0"
SLACK = 4096
STARTS = (0, 1, 15)
FILLS = (b"\n", b"\t0|0")
SCAN = dict(S_hint=0, hop_walkers=0, learn=True, len_hint=0, cands=None)
U64 = ("line_off", "pass_off", "pass_before")
ORDER = ("line_off", "line_len", "line_no", "pass_off", "pass_len", "pass_no", "pass_before")


class HopCands(ctypes.Structure):   # VcfcHopCands
    _fields_ = [("g", ctypes.c_uint32 * 3), ("sig", (ctypes.c_uint16 * 16) * 3)]


class Probe:
    def __init__(self, torch, lib):
        self.T, self.lib = torch, lib
        u64, vp = ctypes.c_uint64, ctypes.c_void_p
        lib.line_probe_layout.argtypes = [u64, u64, ctypes.POINTER(u64)]
        lib.line_probe_layout.restype = None
        lib.line_probe_index.argtypes = [vp, u64, ctypes.c_uint32, u64, ctypes.c_int, ctypes.c_uint32, vp, vp, vp, u64,
                                         vp, u64, u64, ctypes.POINTER(vp), vp, ctypes.POINTER(u64)]

    def layout(self, n, n_lines):
        out = (ctypes.c_uint64 * 3)()
        self.lib.line_probe_layout(n, n_lines, out)
        return int(out[0]), int(out[1]), int(out[2])

    def place(self, buf, start, fill):
        """buf in device memory at `start` bytes past a 16-byte boundary, SLACK
        bytes of `fill` repeated on both sides: (the allocation, buf's offset)."""
        T = self.T
        off = SLACK + start
        total = off + len(buf) + SLACK
        host = np.frombuffer((fill * (total // len(fill) + 1))[:total], dtype=np.uint8).copy()
        host[off:off + len(buf)] = np.frombuffer(buf, dtype=np.uint8)
        d = T.from_numpy(host).to(DEV)
        assert d.data_ptr() % 16 == 0
        return d, off

    def arrays(self, n, cap):
        """Workspaces and output arrays for buffers of n bytes and up to cap lines."""
        T = self.T
        t1, t2, _ = self.layout(n, cap)
        a = dict(ws1=T.empty(t1 + 256, dtype=T.uint8, device=DEV), ws2=T.empty(t2 + 256, dtype=T.uint8, device=DEV),
                 counts=T.empty(4, dtype=T.int64, device=DEV))
        for k in ORDER:
            a[k] = T.empty(cap + 1, dtype=T.int64 if k in U64 else T.int32, device=DEV)
        return a

    def index(self, d, off, n, cap, a, cfg):
        """The index of d[off, off + n) under cfg: counts, the tables and the ends as lists."""
        T = self.T
        for t in a.values():   # poison: nothing may be read before it is written
            t.view(T.uint8).fill_(0xCD)
        hc = None
        if cfg["cands"] is not None:
            hc = HopCands()
            for k in range(3):
                hc.g[k] = cfg["cands"][0][k]
                for j in range(16):
                    hc.sig[k][j] = cfg["cands"][1][k][j]
        tab = (ctypes.c_void_p * 7)(*[a[k].data_ptr() for k in ORDER])
        lines = ctypes.c_uint64(0)
        st = self.lib.line_probe_index(d.data_ptr() + off, n, cfg["S_hint"], cfg["hop_walkers"], int(cfg["learn"]),
                                       cfg["len_hint"], ctypes.byref(hc) if hc is not None else None,
                                       T.cuda.current_stream().cuda_stream, a["ws1"].data_ptr(), a["ws1"].numel(),
                                       a["ws2"].data_ptr(), a["ws2"].numel(), cap, tab, a["counts"].data_ptr(),
                                       ctypes.byref(lines))
        assert st == 0, (st, lines.value, cap)
        counts = [int(x) for x in a["counts"].cpu().numpy().view(np.uint64)]
        assert counts[0] == lines.value and counts[1] <= counts[0] and counts[2] <= counts[0], counts
        nl_off = self.layout(n, counts[0])[2]
        ends = a["ws2"][nl_off:nl_off + 8 * counts[0]].cpu().numpy().view(np.uint64)
        got = {"counts": counts, "ends": ends}
        for k in ORDER:
            m = counts[1] if k.startswith("line") else counts[2]
            got[k] = a[k][:m].cpu().numpy().view(np.uint64 if k in U64 else np.uint32)
        return got


@pytest.fixture(scope="module")
def torch():
    import torch as T   # before the probe: one HIP runtime in the process
    assert T.cuda.is_available(), "GPU tests need a GPU"
    return T


@pytest.fixture(scope="module")
def probe(torch):
    assert os.path.exists(SO), "libvcfc_lineprobe.so not built: run `make -C vcf-compression_amd`"
    return Probe(torch, ctypes.CDLL(SO))


def check_case(probe, name, buf, exp, cfgs):
    """Every configuration at every start and slack fill: the index the case
    expects, the recorded ends tiling the file, nothing depending on the
    bytes around the buffer."""
    n = len(buf)
    cap = buf.count(b"\n")
    arrays = probe.arrays(n, cap)
    want = {}
    for i, cfg in enumerate(cfgs):   # (one plain index per distinct set of missing ends)
        key = tuple(exp["missing"](cfg)) if "missing" in exp else ()
        if key not in want:
            w = C.expected(buf, exp, cfg)
            want[key] = {k: np.asarray(v, dtype=np.uint64) for k, v in w.items()}
    for start in STARTS:
        for fill in FILLS:
            d, off = probe.place(buf, start, fill)
            for cfg in cfgs:
                where = (name, C.cfg_id(cfg), start, fill)
                got = probe.index(d, off, n, cap, arrays, cfg)
                w = want[tuple(exp["missing"](cfg)) if "missing" in exp else ()]
                assert got["counts"] == [int(x) for x in w["counts"]], (where, got["counts"])
                C.tiles(buf, got["ends"].tolist())
                for k in ("ends",) + ORDER:
                    assert np.array_equal(got[k].astype(np.uint64), w[k]), (where, k)


SCAN_CASES = C.scan_registry()
HOP_CASES = C.hop_registry() + C.trap_registry()


@pytest.mark.parametrize("build", [c[2] for c in SCAN_CASES], ids=[c[1] for c in SCAN_CASES])
def test_scan_index_equals_plain_split_on_gpu(probe, build):
    name, buf, S, exp = build()
    check_case(probe, name, buf, exp, [SCAN])


@pytest.mark.parametrize("build,walkers", [(c[2], c[3]) for c in HOP_CASES], ids=[c[1] for c in HOP_CASES])
def test_hop_index_equals_plain_split_on_gpu(probe, build, walkers):
    name, buf, S, exp = build()
    check_case(probe, name, buf, exp, C.configs(buf, S, walkers))


def test_guess_first_length_hints_on_gpu(probe):
    """The GUESS walkers' first guess: right, wrong, around GUESS_MIN, the largest."""
    name, buf, S, exp = C.guess_rounds("streak")
    cfgs = [dict(S_hint=S, hop_walkers=w, learn=False, len_hint=lh, cands=None) for w in (0, 1, 4) for lh in C.GR_LEN_HINTS]
    check_case(probe, name, buf, exp, cfgs)


@pytest.fixture(scope="module")
def ctx(torch):
    import sys
    sys.path.insert(0, os.path.join(G.REPO, "vcf-compression_amd"))
    import vcfc as V
    c = V.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("variant", ["guess", "try"])
def test_new_traps_through_every_ingest_path_on_gpu(ctx, variant):
    """The GUESS and TRY traps through compress_buffer, compress_file and
    compress_device (test_gpu_ingest.both_paths): the oracle's output."""
    from test_gpu_ingest import both_paths
    name, buf, S, exp = C.traps(variant)
    st_o, want, _ = G.oracle_compress(buf)
    assert st_o == 0
    assert both_paths(ctx, buf, 1 << 20) == (0, want, -1)
