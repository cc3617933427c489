"""extract (extract-samples, extract-regions) restated in
Python, and its test inputs.

The rule: the output record is what the reference's `compress` writes for the
line "REQ, chosen tokens joined by TAB, LF".  `extract` below restates it
(header rule, LEN hops, the regular-record walk of subset_cases.py, the
re-encodable check, the greedy re-code, the stop rule);
test_extract_emu.py pins it to the oracle (oracle_compress of the cut of
oracle_decompress, whole files) and to digests of the reference CLI's own
output (tests/golden/extract_cases.json), then holds the kernels to it, whole
bytes, status, error word and offsets, on the CPU emulator;
test_gpu_extract.py does the same on the GPU."""
import hashlib
import json
import os
import random

import decode_cases as D
import golden_io as G
import regions_cases as RC
import subset_cases as SC

OK, E_NOSPACE, E_ARG, E_FORMAT = 0, 4, 5, 8
NO_ERROR = (1 << 64) - 1
CODE = D.CODE
CAP = {b"0|0": 127, b"0|1": 31, b"1|0": 31, b"1|1": 31}


def encodable_req(R):
    return R[0] not in (9, 0x23) and R[-1] == 9 and b"\t\t" not in R


def encode_tokens(toks):
    """The sample section of the chosen tokens, greedily in output order."""
    out = bytearray()
    cur, cnt = None, 0
    for k, t in enumerate(toks):
        if t in CODE:
            if t != cur and cnt:
                out.append(CODE[cur] | cnt)
                cnt = 0
            cur = t
            cnt += 1
            if cnt == CAP[t]:
                out.append(CODE[cur] | cnt)
                cnt = 0
        else:
            if cnt:
                out.append(CODE[cur] | cnt)
                cnt = 0
            cur = None
            out += b"\xe1" + t + (b"\t" if k + 1 < len(toks) else b"")
    if cnt:
        out.append(CODE[cur] | cnt)
    return bytes(out)


def record(b, rs, re, S, cols):
    """(error code, output record) of record b[rs:re]: code 0, 3 (not regular)
    or 5 (regular, not re-encodable)."""
    r = SC.regular(b, rs, re, S)
    if r is None:
        return 3, b""
    R, toks = r
    chosen = [toks[c] for c in cols]
    if not encodable_req(R) or b"" in chosen:
        return 5, b""
    return 0, D.rec(R, encode_tokens(chosen))


def header(v, data_off, cols):
    return v[:data_off] if cols is None else SC.header(v, data_off, cols)


def extract(v, cols=None, query=None, regions=None):
    """extract: (status, bytes).  cols None: all columns; query (ref,
    has_range, start, end) or regions (region text), at most one of them."""
    h = SC.parse_header(v)
    if h is None:
        return E_FORMAT, b""
    data_off, S = h
    if cols is None:
        if S == 0:
            return E_ARG, b""
    elif not SC.check_cols(cols, S):
        return E_ARG, b""
    cc = list(range(S)) if cols is None else cols
    out = [header(v, data_off, cols)]
    b = v[data_off:]
    rec, end = SC.hop(b)
    reg = RC.parse_text(regions) if regions is not None else None
    for i, rs in enumerate(rec):
        re = rec[i + 1] if i + 1 < len(rec) else end
        if query is not None or reg is not None:
            m = SC.match(b, rs, re, *query) if query is not None else RC.match_or(b, rs, re, reg, RC.CC.match)
            if m is None:
                return E_FORMAT, b"".join(out)
            if not m:
                continue
        code, r = record(b, rs, re, S, cc)
        if code:
            return E_FORMAT, b"".join(out)
        out.append(r)
    return (E_FORMAT if len(b) - end >= 8 else OK), b"".join(out)


def device(data, cols=None, select=None, cap=None):
    """The device entry on the records of a well-formed file: (error word,
    record offsets, output bytes up to the last record that fits)."""
    h, S = SC.parse_header(data)
    b = data[h:]
    rec, end = SC.hop(b)
    cc = list(range(S)) if cols is None else cols
    err, off, out = NO_ERROR, [0], []
    for i, rs in enumerate(rec):
        r = b""
        if select is None or select[i]:
            code, r = record(b, rs, (rec + [end])[i + 1], S, cc)
            if code:
                err = min(err, (i << 8) | code)
        off.append(off[-1] + len(r))
        out.append(r)
    if cap is not None:
        for i in range(len(rec)):
            if off[i + 1] > cap:
                err = min(err, (i << 8) | 0xFF)
                break
    return err, off, out


# ---- inputs ---------------------------------------------------------------

HS = SC.HS
TILE = 4096   # VCFC_EXTRACT_TILE: chosen columns of the wave path's LDS tile
OTHERS = 248  # EX_OTH (vcfc_extract.hip): chosen other tokens of a record on the wave path
rec, req_of, fill = D.rec, D.req_of, D.fill


def _file(S, *items):
    return D.header(S) + b"".join(rec(req_of(i), it) for i, it in enumerate(items))


def hand_built():
    """(name, file bytes, column sets, error code of the first refused record
    or 0 -- per column set): S = 600 records at the re-code's edges."""
    out = []
    ALL = list(range(HS))
    # cap edges: a chosen run of n tokens of each class, in the middle and ending exactly at K
    for code, ns in ((0x00, (126, 127, 128, 254, 255)), (0xA0, (30, 31, 32, 62, 63)), (0xC0, (30, 31, 32, 62, 63)),
                     (0x80, (30, 31, 32, 62, 63))):
        other = 0x80 if code != 0x80 else 0x00
        items = [fill(100, other) + fill(n, code) + fill(HS - 100 - n, other) for n in ns]
        sets = [ALL, list(range(90, 100 + max(ns) + 10)), list(range(100 + max(ns), 95, -1))]
        sets += [list(range(50, 100 + n)) for n in ns]   # the run ends exactly at K
        out.append(("cap_%02x" % code, _file(HS, *items), sets, 0))
    # merges: two runs adjacent after the cut; across a source window, a 64-slot batch
    out.append(("merge_skip", _file(HS, fill(200) + fill(1, 0xA0) + fill(399), fill(30, 0xC0) + b"\xe12|2\t" + fill(569, 0xC0),
                                    b"\x01" * 300 + fill(1, 0x80) + b"\x01" * 299),
                [[c for c in ALL if c != 200], [c for c in ALL if c not in (30, 200, 300)],
                 list(range(190, 200)) + list(range(201, 260)), list(range(140, 200)) + list(range(201, 210)),
                 list(range(137, 200)) + list(range(201, 203))], 0))
    # merges through an escape that spells the class, also as the source's last token
    out.append(("merge_escape", _file(HS, fill(100) + b"\xe10|0\t" + fill(499), fill(599, 0x80) + b"\xe11|1",
                                      fill(100, 0xA0) + b"\xe10|1\t\xe10|1\t" + b"\xe11|0\t" + fill(497, 0xC0),
                                      fill(598) + b"\xe20|0\t0|0"),
                [ALL, list(range(90, 110)), [599, 598, 100, 101, 102, 0], list(range(599, 560, -1)), [100], [599]], 0))
    # 127 + 127 + 46 cut to every 2nd column (150: 127 + 23)
    out.append(("merge_300", _file(HS, fill(300) + fill(300, 0x80), fill(150, 0xC0) + fill(300) + fill(150, 0xA0)),
                [list(range(0, HS, 2)), list(range(1, HS, 2)), list(range(0, 300, 2)), list(range(150, 450, 2))], 0))
    # other tokens: the last chosen one an escape; the LF-ended source token in the middle; one of a
    # 2-token escape; a 300-byte token across a window; zero-count items
    long_tok = b"0|1:" + b"9" * 296
    out.append(("others", _file(HS, fill(HS - 1, 0x80) + b"\xe12|2", fill(HS - 1) + b"\xe13|12345",
                                fill(300) + b"\xe22|1\t0|2:77\t" + fill(HS - 302, 0x80),
                                fill(120) + b"\xe1" + long_tok + b"\t" + fill(HS - 121, 0xA0),
                                b"\x00\xa0" + fill(HS, 0xA0), fill(5) + b"\xe0\x80" + fill(HS - 5),
                                fill(10) + b"\xe12|1\t" + fill(HS - 11, 0xC0)),
                [ALL, [0, HS - 1], [HS - 1, 0], [HS - 1, 0, 7], [300], [301], [301, 300, 299, 302], [5, 120, 4],
                 [3, 10], [10, 3], list(range(0, HS, 7))], 0))
    # 260 other tokens: the wave path names at most OTHERS of a record's chosen ones (above: byte-serial)
    toks = [b"2|1" if c % 2 == 0 and c < 520 else D.CLASSES[(c // 5) % 4] for c in range(HS)]
    out.append(("many_others", _file(HS, D.items_of(toks), D.items_of(toks[::-1])),
                [ALL, list(range(2 * OTHERS)), list(range(2 * OTHERS + 1)), list(range(2 * OTHERS + 1, -1, -1)),
                 list(range(HS - 1, HS - 2 * OTHERS - 1, -1)), list(range(HS - 1, HS - 2 * OTHERS - 3, -1))], 0))
    # refusals
    out.append(("empty_escape", _file(HS, fill(HS), fill(10) + b"\xe1\t" + fill(HS - 11, 0xC0), fill(HS - 1) + b"\xe1"),
                [[9, 11], [0, HS - 2]], 0))
    out.append(("empty_chosen", _file(HS, fill(HS), fill(10) + b"\xe1\t" + fill(HS - 11, 0xC0), fill(HS)),
                [[10], [9, 10, 11], ALL], 5))
    out.append(("empty_last_chosen", _file(HS, fill(HS), fill(HS - 1) + b"\xe1"), [[HS - 1], [3, HS - 1, 0]], 5))
    r = req_of(1)
    for name, bad in (("req_hash", b"#" + r[1:]), ("req_tab_first", b"\t" + r.replace(b"\tA\t", b"\tA", 1)),
                      ("req_tabs_doubled", r.replace(b"\tA\tG", b"\t\tAG", 1)), ("req_no_last_tab", r[:-1].replace(b"AC=", b"AC\t=", 1) + b"x")):
        assert bad.count(b"\t") == 9
        simple = D.header(HS) + rec(req_of(0), fill(HS)) + rec(bad, fill(300) + b"\xe12|1\t" + fill(299)) + rec(req_of(2), fill(HS))
        serial = D.header(HS) + rec(req_of(0), fill(HS)) + rec(bad, fill(298) + b"\xe22|1\t3|4\t" + fill(300)) + rec(req_of(2), fill(HS))
        out.append((name, simple, [[0], ALL], 5))
        out.append((name + "_serial", serial, [[0], ALL], 5))
    return out


def tile_cases():
    """(name, file, column sets): S past the tile limit -- K at the limit
    (wave path) and above it (byte-serial), a run merging across slot TILE."""
    S = TILE + 200
    items = [fill(2000) + fill(1, 0xA0) + fill(2200) + fill(S - 4201, 0x80), fill(S - 1, 0xC0) + b"\xe12|1"]
    keep = [c for c in range(S) if c != 2000]
    return [("tile", _file(S, *items), [keep[:TILE], keep[:TILE + 1], keep[:TILE - 1] + [S - 1], list(range(S)),
                                        list(range(S - 1, -1, -1))[:TILE]])]


def check_hand_built(ext):
    """ext(data, cols) -> (status, bytes)."""
    for name, data, sets, code in hand_built() + [(n, d, s, 0) for n, d, s in tile_cases()]:
        for cols in sets:
            want = extract(data, cols)
            assert want[0] == (E_FORMAT if code else OK), (name, cols[:8])
            got = ext(data, cols)
            assert got == want, (name, cols[:8], len(cols), got[0], want[0], len(got[1]), len(want[1]))
    for name, data, sets in SC.hand_built():   # §4i's records: window edges, the serial path, every frame edge
        for cols in sets:
            want = extract(data, cols)
            got = ext(data, cols)
            assert got == want, (name, cols[:8], len(cols), got[0], want[0], len(got[1]), len(want[1]))
    # the cases mean what their names say
    hb = {name: data for name, data, _, _ in hand_built()}
    assert extract(hb["cap_00"], list(range(HS)))[1].count(b"\x7f") >= 6   # full 0|0 bytes

    def records(name, cols):
        st, out = extract(hb[name], cols)
        return out[len(header(hb[name], len(D.header(HS)), cols)):]
    assert records("merge_skip", [c for c in range(HS) if c != 200]).startswith(rec(req_of(0), fill(599)))
    assert records("merge_escape", None).startswith(rec(req_of(0), fill(HS)) + rec(req_of(1), fill(HS, 0x80)))
    assert records("others", [HS - 1, 0, 7]).startswith(rec(req_of(0), b"\xe12|2\t\x82") + rec(req_of(1), b"\xe13|12345\t\x02"))
    for name, data, _ in SC.frame_edges():   # the first record, then the stop; all three of long_req
        st, out = extract(data, [299])
        n = len(SC.hop(out[len(header(data, len(D.header(HS)), [299])):])[0])
        assert (st, n) == ((OK, 3) if name == "frame_long_req" else (E_FORMAT, 1)), name


def check_files(ext, files, seed=0, short=False):
    """short: all columns, one column, reversed and a random 65 only (the
    emulator's further seeds; the GPU takes every set)."""
    for name, data in files:
        h = SC.parse_header(data)
        S = h[1] if h else 4
        sets = SC.column_sets(max(S, 1), seed)
        for cols in [None] + ([c for c in sets if len(c) == 1 or len(c) == 65 or c[:2] == [S - 1, S - 2]] if short else sets):
            want = extract(data, cols)
            got = ext(data, cols)
            assert got[0] == want[0], (name, cols and cols[:8], got[0], want[0])
            assert got[1] == want[1], (name, cols and cols[:8], len(got[1]), len(want[1]))


def check_queries(ext, seed):
    """ext(data, cols, query=..., regions=...) -> (status, bytes)."""
    stopped = unstopped = 0
    for name, data in SC.query_files(seed):
        for q in SC.QUERIES:
            for cols in (None, [39, 0, 17], list(range(0, 40, 7))):
                want = extract(data, cols, query=q)
                got = ext(data, cols, query=q)
                assert got == want, (name, q, cols and cols[:8], got[0], want[0], len(got[1]), len(want[1]))
            if name.startswith(("no_lf", "nul_req")):
                stopped += want[0] == E_FORMAT
                unstopped += want[0] == OK
        for key in ("A", "C"):   # two region tables
            for cols in (None, [39, 0, 17]):
                want = extract(data, cols, regions=RC.SETS[key])
                got = ext(data, cols, regions=RC.SETS[key])
                assert got == want, (name, key, cols and cols[:8], got[0], want[0], len(got[1]), len(want[1]))
    assert stopped >= 5 and unstopped >= 5, (stopped, unstopped)


def select_cases(n):
    return [[0] * n, [1] * n, [int(i % 8 == 0) for i in range(n)], [int(i % 8 == 3 or i == n - 1) for i in range(n)]]


def check_device(dev):
    """dev(data, cols, select, cap, base) -> (status, err word, offsets, out
    bytes); it checks the canary and fill bytes itself."""
    name, data = SC.batch_files()[4]   # 41 records, S = 70
    n = 41
    for cols in (None, [0], [69, 0, 33], list(range(69, -1, -1))):
        for sel in [None] + select_cases(n):
            err, off, recs = device(data, cols, sel)
            st, gerr, goff, out = dev(data, cols, sel, None, 0)
            assert (st, gerr) == (OK, NO_ERROR) == (OK, err) and goff == off and out[:off[-1]] == b"".join(recs), (cols, sel)
            if off[-1]:   # one byte short: the first record that does not fit; and no room at all
                for cap in (off[-1] - 1, 0):
                    err, _, _ = device(data, cols, sel, cap)
                    st, gerr, goff, out = dev(data, cols, sel, cap, 0)
                    assert (st, gerr) == (OK, err) and goff == off, (cols, sel, cap, hex(gerr))
                    k = max(i for i in range(n + 1) if off[i] <= cap)
                    assert out[:off[k]] == b"".join(recs[:k])
    for base in range(16):   # every alignment of the output
        err, off, recs = device(data, [69, 0, 33])
        st, gerr, goff, out = dev(data, [69, 0, 33], None, None, base)
        assert (st, gerr, goff) == (OK, NO_ERROR, off) and out[:off[-1]] == b"".join(recs), base
    for cols in ([], [70], [1, 1], [0, 70]):
        assert dev(data, cols, None, None, 0)[0] == E_ARG
    # an irregular record counts only where it is selected
    name, data = next(x for x in SC.query_files(1) if x[0] == "no_lf17")
    st, gerr, goff, out = dev(data, [0, 5], None, None, 0)
    assert (st, gerr) == (OK, (17 << 8) | 3)
    sel = [int(i != 17) for i in range(60)]
    st, gerr, goff, out = dev(data, [0, 5], sel, None, 0)
    assert (st, gerr) == (OK, NO_ERROR) and goff[17] == goff[18] and goff == device(data, [0, 5], sel)[1]
    # refusals by code, hand-built
    for name, data, sets, code in hand_built():
        for cols in sets[:2]:
            err, off, recs = device(data, cols)
            st, gerr, goff, out = dev(data, cols, None, None, 0)
            assert (st, gerr, goff) == (OK, err, off) and out[:off[-1]] == b"".join(recs), (name, cols[:8], hex(gerr))
            assert (err & 0xFF) == (code if code else 0xFF), name


def check_bound(bound):
    """bound(in_bytes, n_records, K) holds for every case here."""
    for name, data, sets, _ in hand_built():
        n = len(SC.hop(data[SC.parse_header(data)[0]:])[0])
        for cols in sets:
            st, out = extract(data, cols)
            assert len(out) <= bound(len(data), n, len(cols)), name


# ---- golden digests of the reference CLI's output ----------------------------

def golden():
    with open(os.path.join(G.GOLDEN, "extract_cases.json")) as f:
        return json.load(f)


def golden_columns(spec, S):
    """The column set a golden case names: {"range": [a, b, step]}, or
    {"sample": [seed, k]}."""
    if "range" in spec:
        return list(range(*spec["range"]))
    return random.Random(spec["sample"][0]).sample(range(S), spec["sample"][1])


def check_golden(ext):
    d = golden()
    data = G.gz(d["file"])
    S = SC.parse_header(data)[1]
    assert len(d["cases"]) >= 5
    for c in d["cases"]:
        st, out = ext(data, golden_columns(c["cols"], S))
        assert st == OK and len(out) == c["size"] and hashlib.sha256(out).hexdigest() == c["sha256"], c["cols"]
