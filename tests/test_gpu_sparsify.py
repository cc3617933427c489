"""GPU parity for the sparse layout at its edges (tests/sparse_cases.py):
k_sparse_plan through vcfc_sparse_plan_device under the plan contract,
vcfc_sparsify_file (C ABI and `build/main sparsify`) against the plain
statement's file and the reference's own recorded files
(tests/golden/sparse_edge_cases.json), and vcfc_sparsify_shard rank by rank
in one process against the slice plan, with a defect on and next to every
halo record.  Every comparison is byte-exact."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import golden_io as G
import sparse_cases as C
import sparse_digest

pytestmark = pytest.mark.gpu
REPO = G.REPO
sys.path.insert(0, os.path.join(REPO, "vcf-compression_amd"))


@pytest.fixture(scope="module")
def ctx():
    import torch   # before libvcfc: one HIP runtime in the process
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import vcfc
    c = vcfc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wd():
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        yield d


def put(wd, name, v):
    p = os.path.join(wd, name.replace("/", "-") + ".vcfc")
    if not os.path.exists(p):
        with open(p, "wb") as f:
            f.write(v)
    return p


def gpu_plan(v):
    """vcfc_sparse_plan_device over the records of v; outputs prefilled 0xAB."""
    import torch
    import vcfc
    _, recs, _ = C.split(v)
    n = len(recs)
    dev = "cuda:0"
    body = torch.frombuffer(bytearray(b"".join(recs) + b"\0" * 16), dtype=torch.uint8).to(dev)
    ro = torch.tensor(C.rec_offsets(recs), dtype=torch.int64, device=dev)
    fo = torch.full((8 * max(n, 1),), 0xAB, dtype=torch.uint8, device=dev)
    pf = torch.full((16 * max(n, 1),), 0xAB, dtype=torch.uint8, device=dev)
    st = torch.full((16,), 0xAB, dtype=torch.uint8, device=dev)
    vcfc.sparse_plan_device(body.data_ptr(), ro.data_ptr(), n, C.data_start_of(v), fo.data_ptr(), pf.data_ptr(),
                            st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return fo.cpu().numpy().view(np.uint64), pf.cpu().numpy().tobytes(), st.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("family", sorted(C.FAMILIES))
def test_plan_entry(ctx, family):
    ran = 0
    for name, v, _ in C.all_cases():
        if name.startswith(family + "/"):
            C.check_plan(name, v, *gpu_plan(v))
            ran += 1
    assert ran == len(C.FAMILIES[family]())


@pytest.mark.parametrize("family", sorted(C.FAMILIES))
def test_sparsify_file(ctx, wd, family):
    """ctx.sparsify_status on every disk-bound case: status and file are the
    plain statement's and, where recorded, the reference's own; behind a throw
    the last record written keeps dist_to_next = 0."""
    gold = C.golden()
    dst = os.path.join(wd, "out.sparse")
    ran = zero_next = 0
    for name, v in C.disk_cases():
        if not name.startswith(family + "/"):
            continue
        if os.path.exists(dst):
            os.unlink(dst)
        st = ctx.sparsify_status(put(wd, name, v), dst)
        assert C.same_as_image(v, st, dst), (name, st, C.image_digest(v)[0])
        if name in gold:
            C.check_golden(name, v, st, sparse_digest.digest(dst))
        _, recs, _ = C.split(v)
        off, _, bad, _ = C.plan(recs, C.data_start_of(v))
        if bad:   # records 0 .. bad - 1 are in the file
            with open(dst, "rb") as f:
                f.seek(off[bad - 1])
                pre = f.read(16)
            assert pre[8:16] == b"\0" * 8, (name, pre.hex())
            zero_next += 1
        ran += 1
    assert ran and (zero_next >= 5 or family not in ("err_order", "pos_forms"))


@pytest.mark.parametrize("name", ["adjacent/d1_eq", "adjacent/d1_p1", "pos_forms/bad_313261"])
def test_cli_sparsify(wd, name):
    """`build/main sparsify` on a clean, an anomaly and an error case: the
    reference's recorded exit code and file."""
    v = dict(C.golden_cases())[name]
    _, recs, _ = C.split(v)
    _, _, bad, anomaly = C.plan(recs, C.data_start_of(v))
    assert (bad is not None, anomaly) == {"adjacent/d1_eq": (False, False), "adjacent/d1_p1": (False, True),
                                          "pos_forms/bad_313261": (True, True)}[name]
    dst = os.path.join(wd, "cli.sparse")
    r = subprocess.run([os.path.join(REPO, "build", "main"), "sparsify", put(wd, name, v), dst],
                       capture_output=True, timeout=120)
    assert r.returncode == (134 if bad is not None else 0) == C.ref_exit_code(name), (name, r.returncode, r.stderr)
    dg = sparse_digest.digest(dst)
    C.check_golden(name, v, C.OK if r.returncode == 0 else C.E_FORMAT, dg)
    assert dg == C.image_digest(v)[1]


def sees(n, rank, world, at):
    """Whether record `at` lies in the planned range of a rank, and where:
    "own", "halo_lo" (lo - 1), "halo_hi" (hi), "outside" (one record past a
    halo record) or None."""
    lo, hi = n * rank // world, n * (rank + 1) // world
    if lo <= at < hi:
        return "own"
    if lo and at == lo - 1:
        return "halo_lo"
    if hi < n and at == hi:
        return "halo_hi"
    if at == lo - 2 or at == hi + 1:
        return "outside"
    return None


@pytest.mark.parametrize("n", C.SHARD_N)
def test_shard_info(ctx, wd, n):
    """vcfc_sparsify_shard, plan only, every rank of worlds 2, 3 and 5 in one
    process: [lo, hi, first_err, anomaly] is the slice plan's over the rank's
    records and its halo.  A rank whose halo record carries the defect reports
    it, a rank one record further away reports a clean plan."""
    import vcfc
    seen = {"own": 0, "halo_lo": 0, "halo_hi": 0, "outside": 0}
    for name, v in C.shard_files():
        if not name.startswith("n%d" % n):
            continue
        _, recs, _ = C.split(v)
        assert len(recs) == n
        src = put(wd, "shard-" + name, v)
        bad_at = next((i for i, r in enumerate(recs) if C.pos_of(r[8:]) is None), None)
        for world in C.SHARD_WORLDS:
            for rank in range(world):
                st, info = ctx.sparsify_shard(src, None, rank, world)
                want = C.shard_info(recs, rank, world, C.data_start_of(v))
                assert st == vcfc.OK and info == want, (name, world, rank, info, want)
                if bad_at is not None:
                    where = sees(n, rank, world, bad_at)
                    if where in ("own", "halo_lo", "halo_hi"):
                        assert info[2] == bad_at, (name, world, rank, info)
                    else:
                        assert info[2] is None and info[3] == 0, (name, world, rank, info)
                    if where:
                        seen[where] += 1
    assert all(seen.values()), seen


@pytest.mark.parametrize("n", C.SHARD_N)
def test_shard_write(ctx, wd, n):
    """A clean file: every rank writes its slice, highest rank first, into
    one file, which equals sparsify_file's.  A file with a defect: a rank that
    sees it refuses to write (VCFC_E_ARG) and creates nothing."""
    import vcfc
    files = dict(C.shard_files())
    v = files["n%d" % n]
    src = put(wd, "shard-n%d" % n, v)
    whole = os.path.join(wd, "whole.sparse")
    assert ctx.sparsify_status(src, whole) == vcfc.OK
    want = sparse_digest.digest(whole)
    assert want == C.image_digest(v)[1]
    for world in C.SHARD_WORLDS:
        dst = os.path.join(wd, "shards%d.sparse" % world)
        for rank in reversed(range(world)):
            st, info = ctx.sparsify_shard(src, dst, rank, world)
            assert st == vcfc.OK and info[2] is None and info[3] == 0, (world, rank, st, info)
        assert sparse_digest.digest(dst) == want, world
        os.unlink(dst)
    refused = 0
    for name, v in C.shard_files():
        if not name.startswith("n%d_" % n):
            continue
        _, recs, _ = C.split(v)
        src = put(wd, "shard-" + name, v)
        dst = os.path.join(wd, "refused.sparse")
        world = 3
        for rank in range(world):
            want = C.shard_info(recs, rank, world, C.data_start_of(v))
            if want[2] is not None or want[3]:
                st, info = ctx.sparsify_shard(src, dst, rank, world)
                assert st == vcfc.E_ARG and info == want and not os.path.exists(dst), (name, rank, st, info)
                refused += 1
    assert refused >= 10
