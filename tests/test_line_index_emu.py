"""The line index (csrc/vcfc_ingest.hip: k_nl_scan, k_nl_hop_start, k_nl_hop,
k_nl_place, k_line_place) on the CPU emulator against a plain line split
(line_index_cases.plain_index): counts, all seven tables and the recorded
line ends, for every family of line_index_cases.py under every configuration
(hop_walkers, learn, len_hint, cands, and the scan).  The traps give the true
index minus exactly the ends their expectation names.  Each case also states
the walkers' steps (VCFC_DIAG_HOP_STEP) it was built to cause, and they are
counted: a case cannot pass without taking the path it is named for."""
import pytest

import emu_io as E
import golden_io as G
import line_index_cases as C

SCAN = dict(S_hint=0, hop_walkers=0, learn=True, len_hint=0, cands=None)
KEYS = ("counts", "ends") + C.TABLES


def index_and_steps(buf, cfg):
    E.emu_hop_steps()
    got = E.emu_line_index_full(buf, **cfg)
    return got, E.emu_hop_steps()


def check_index(name, buf, exp, cfg, got):
    want = C.expected(buf, exp, cfg)
    C.tiles(buf, got["ends"])
    for k in KEYS:
        assert got[k] == want[k], (name, C.cfg_id(cfg), k)


def check_steps(name, exp, cfg, steps):
    """The case's stated steps, under the configurations they are stated for."""
    stated = [exp.get("cfg")] + exp.get("also", [])
    if cfg in stated:
        for k, v in exp.get("steps", {}).items():
            assert steps[k] == v, (name, C.cfg_id(cfg), k, steps)
        for k, v in exp.get("at_least", {}).items():
            assert steps[k] >= v, (name, C.cfg_id(cfg), k, steps)
    if "seeded" in exp and cfg == dict(exp["cfg"], cands=cfg["cands"]) and cfg["cands"] is not None:
        for k, v in exp["seeded"].items():
            assert steps[k] == v, (name, "seeded", k, steps)
    # one walker without learning: every line end is recorded by exactly one step
    if cfg["S_hint"] >= 32 and cfg["hop_walkers"] == 1 and not cfg["learn"] and "missing" not in exp:
        by = sum(steps[k] for k in ("LINE_FIRST", "LINE_CHECK", "VERIFY_HIT", "FIND", "GUESS_TAKEN"))
        assert by == steps["ends"], (name, C.cfg_id(cfg), steps)


@pytest.mark.parametrize("build", [c[2] for c in C.scan_registry()], ids=[c[1] for c in C.scan_registry()])
def test_scan_index_equals_plain_split(build):
    name, buf, S, exp = build()
    got, _ = index_and_steps(buf, SCAN)
    check_index(name, buf, exp, SCAN, got)


HOP = C.hop_registry() + C.trap_registry()


@pytest.mark.parametrize("build,walkers", [(c[2], c[3]) for c in HOP], ids=[c[1] for c in HOP])
def test_hop_index_equals_plain_split(build, walkers):
    """Every configuration of the case: the tables are the plain split's (a
    trap's: less its named ends), the recorded ends tile the file, and the
    walkers took the steps the case states."""
    name, buf, S, exp = build()
    for cfg in C.configs(buf, S, walkers):
        got, steps = index_and_steps(buf, cfg)
        check_index(name, buf, exp, cfg, got)
        steps["ends"] = got["counts"][0]
        check_steps(name, exp, cfg, steps)


@pytest.mark.parametrize("family", sorted(C.FAMILY_STEPS))
def test_family_takes_the_steps_it_is_named_for(family):
    total = dict.fromkeys(C.STEPS, 0)
    for fam, name, build, _ in C.hop_registry():
        if fam != family:
            continue
        _, buf, S, exp = build()
        if S < 32:
            continue
        _, steps = index_and_steps(buf, exp["cfg"])
        for k in C.STEPS:
            total[k] += steps[k]
    for k in C.FAMILY_STEPS[family]:
        assert total[k] > 0, (family, k, total)


@pytest.mark.parametrize("walkers", [0, 1, 4])
def test_guess_first_length_hints(walkers):
    """The GUESS walkers' first guess (len_hint): the right length, a wrong
    one, 511 and 512 around GUESS_MIN and the largest the host hands over --
    the index is exact whatever the hint."""
    name, buf, S, exp = C.guess_rounds("streak")
    for lh in C.GR_LEN_HINTS:
        cfg = dict(S_hint=S, hop_walkers=walkers, learn=False, len_hint=lh, cands=None)
        got, _ = index_and_steps(buf, cfg)
        check_index(name, buf, exp, cfg, got)


def test_hints_restated_as_the_driver_computes_them():
    """line_index_cases' restatements of the host's hints against the product
    functions (vcfc_ingest_driver.h data_lines_irregular, first_data_line_len,
    learn_candidates) over the first 64 KiB, as compress_device calls them."""
    import ctypes
    lib = E.lib()
    lib.emu_data_lines_irregular.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32]
    lib.emu_first_data_line_len.argtypes = [ctypes.c_char_p, ctypes.c_uint64]
    lib.emu_first_data_line_len.restype = ctypes.c_uint32
    lib.emu_learn_candidates.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
    seen = 0
    for build in (lambda: C.try_learn("G254"), lambda: C.try_learn("G255"), lambda: C.try_learn("kinds5"),
                  lambda: C.try_learn("same_G"), lambda: C.try_learn("law2"), lambda: C.guess_rounds("streak"),
                  lambda: C.traps("guess"), lambda: C.traps("try"), lambda: C.line_window("rows_choice"),
                  lambda: C.s_gate(32), lambda: C.span_edge("long_row")):
        _, buf, S, _ = build()
        head = buf[:65536]
        assert bool(lib.emu_data_lines_irregular(head, len(head), S)) == C.data_lines_irregular(head, S)
        assert lib.emu_first_data_line_len(head, len(head)) == C.first_data_line_len(head)
        hc = E._HopCands()
        lib.emu_learn_candidates(head, len(head), S, ctypes.byref(hc))
        g, sig = C.learn_candidates(head, S)
        assert list(hc.g) == g and [list(r) for r in hc.sig] == sig
        seen += sum(x != 0 for x in g)
    assert seen >= 8   # (candidates were compared, not only their absence)


@pytest.mark.parametrize("variant", ["guess", "try"])
def test_new_traps_are_caught_by_compress_device(variant):
    """The GUESS and TRY traps through compress_device (its own choice of
    walkers and hints): the encoder sees the '\\n' inside the merged row, the
    chunk is indexed again once, and the output is the oracle's."""
    name, buf, S, exp = C.traps(variant)
    st_o, want, _ = G.oracle_compress(buf)
    assert st_o == 0
    redo = []
    st, got, _ = E.emu_compress_device(buf, chunk=1 << 20, redo=redo)
    assert st == 0 and got == want
    assert redo == [1]
