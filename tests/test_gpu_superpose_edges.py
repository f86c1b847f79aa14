"""k_superpose / k_superpose4, k_metrics / k_metrics4 and k_lms_qcp on the hand-made cases of tests/superpose_cases.py — the guard, h == 0, the flush,
rank deficiency, keep-first, the lane layouts, the GDT cutoffs to the ulp, a contracted transform, the partial fit's discrete choices — through
match.kabsch_batch / metrics_batch / lms_qcp_batch only, in both packings (FDGPU_SP_PACK unset and 0), compared with the CPU oracle."""
import collections
import os

import numpy as np
import pytest

from tests import superpose_cases as sc

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.40282347e+38)
EYE = np.eye(3, dtype=np.float32)


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


def _both_packings(call):
    """call() with FDGPU_SP_PACK unset and = 0 (the library reads it per call)"""
    saved = os.environ.pop("FDGPU_SP_PACK", None)
    try:
        packed = call()
        os.environ["FDGPU_SP_PACK"] = "0"
        wave = call()
    finally:
        os.environ.pop("FDGPU_SP_PACK", None)
        if saved is not None:
            os.environ["FDGPU_SP_PACK"] = saved
    return packed, wave


@pytest.fixture(scope="module")
def sp_runs(ctx):
    from folddisco_amd import match
    out = {}
    for name, batch, _ in sc.batches():
        xs, ys, off = sc.pack(batch)
        out[name] = (batch,) + _both_packings(lambda: match.kabsch_batch(ctx, xs, ys, off))
    return out


@pytest.fixture(scope="module")
def metric_runs(ctx):
    from folddisco_amd import match
    out = {}
    for name, batch, _ in sc.metrics_batches():
        refs, movs, off, rot, tran = sc.pack_metrics(batch)
        out[name] = (batch,) + _both_packings(lambda: match.metrics_batch(ctx, refs, movs, off, rot, tran))
    return out


BATCHES = ("all", "small", "mixed", "positions")


@pytest.mark.parametrize("name", BATCHES)
def test_superposition_packings_are_the_same_bits(sp_runs, name):
    _, packed, wave = sp_runs[name]
    for a, b in zip(packed, wave):
        assert a.tobytes() == b.tobytes(), name


def _check_case(c, rmsd, rot, tran, where):
    if c is None:
        assert rmsd == FLT_MAX and np.array_equal(rot, EYE) and not tran.any(), where
        return
    assert abs(float(rmsd) - c.rmsd) <= sc.TOL_RMSD * max(1.0, abs(c.rmsd)), (where, c, rmsd, c.rmsd, c.trace)
    if c.kind == "identity":
        assert np.array_equal(rot, EYE), (where, c, rot)
        if c.trace["spur_pos"]:
            assert not tran.any(), (where, c, tran)                     # the construction gave up: zero translation
        else:
            assert np.array_equal(tran, c.tran), (where, c, tran, c.tran)   # no spread: yc - xc of exact sums, the oracle's bits
    elif c.kind == "pinned":
        assert np.abs(rot - c.rot).max() <= sc.TOL_ROT and np.abs(tran - c.tran).max() <= sc.TOL_TRAN, (where, c, rot, c.rot, tran, c.tran, c.trace)
    else:
        u = rot.astype(np.float64)
        assert np.abs(u.T @ u - np.eye(3)).max() <= 1e-6 and np.linalg.det(u) > 0, (where, c, rot)
        assert abs(sc.rmsd_of(c.x, c.y, rot, tran) - float(rmsd)) <= 1e-4, (where, c, rmsd)
    if c.yardstick:
        assert float(rmsd) <= c.optimum + 1e-4, (where, c, rmsd, c.optimum)


@pytest.mark.parametrize("name", BATCHES)
def test_superposition_equals_the_oracle_on_every_case(sp_runs, name):
    batch, (rmsd, rot, tran), _ = sp_runs[name]
    assert len(rmsd) == len(batch)
    for k, c in enumerate(batch):
        _check_case(c, rmsd[k], rot[k], tran[k], (name, k))


def test_superposition_figures_per_family(sp_runs, capsys):
    """the largest differences from the oracle per family, in f32 ulps (rmsd: of the oracle's rmsd; rotation: of 1.0; translation: of the larger
    of 1.0 and the component) — printed for DESIGN §2 item 8; every one is inside the tolerances by the test above"""
    batch, (rmsd, rot, tran), _ = sp_runs["all"]
    worst = collections.defaultdict(lambda: [0.0, 0.0, 0.0, 0])
    for k, c in enumerate(batch):
        if c is None:
            continue
        w = worst[c.family]
        w[3] += 1
        w[0] = max(w[0], abs(float(rmsd[k]) - c.rmsd) / float(np.spacing(np.float32(max(abs(c.rmsd), 1e-30)))))
        if c.kind != "free":
            w[1] = max(w[1], float(np.abs(rot[k] - c.rot).max()) / float(np.spacing(np.float32(1.0))))
            w[2] = max(w[2], float((np.abs(tran[k] - c.tran) / np.spacing(np.maximum(np.abs(c.tran), np.float32(1.0)))).max()))
    with capsys.disabled():
        print("\nsuperposition, largest difference from the oracle in f32 ulps (rmsd / rotation / translation), cases:")
        for fam in sc.FAMILIES:
            w = worst[fam]
            print(f"  {fam:12s} {w[0]:8.1f} {w[1]:8.1f} {w[2]:8.1f}   {w[3]}")
    assert set(worst) == set(sc.FAMILIES)


@pytest.mark.parametrize("name", ("all", "small"))
def test_metrics_on_the_cutoffs(metric_runs, name):
    """gdt_ts, gdt_ha and hausdorff carry the oracle's bits (counts and an f32 maximum do not depend on the order), tm_score and chamfer are within
    rtol = atol = 1e-6; both packings give the same bytes; empty problems give 0 / 0 / 0 / inf / inf"""
    batch, packed, wave = metric_runs[name]
    assert packed.tobytes() == wave.tobytes()
    fams = collections.Counter()
    for k, c in enumerate(batch):
        got = packed[k]
        if c is None:
            assert not got[:3].any() and np.isinf(got[3]) and np.isinf(got[4]), (name, k, got)
            continue
        assert np.array_equal(got[[1, 2, 4]].view(np.uint32), c.want[[1, 2, 4]].view(np.uint32)), (name, k, c, got, c.want)
        assert np.allclose(got[[0, 3]], c.want[[0, 3]], rtol=1e-6, atol=1e-6), (name, k, c, got, c.want)
        fams[c.family] += 1
    assert fams["threshold"] >= 45                       # (small: every threshold case of 1 and 16 points)
    if name == "all":
        assert fams["contraction"] >= 2 and fams["equidistant"] == 5 and fams["hausdorff_last"] == 5


def test_partial_fit_is_the_oracle_bit_for_bit(ctx):
    from folddisco_amd import match
    lc = sc.lms_cases()
    xs = np.concatenate([c.x for c in lc]); ys = np.concatenate([c.y for c in lc])
    off = np.concatenate([[0], np.cumsum([c.n for c in lc])]).astype(np.uint64)
    rms, rot, tran, cores = match.lms_qcp_batch(ctx, xs, ys, off)
    for k, c in enumerate(lc):
        assert np.array_equal(cores[k].astype(np.uint64), c.core), (c, cores[k], c.core)
        assert np.float32(rms[k]).view(np.uint32) == np.float32(c.rms).view(np.uint32), (c, rms[k], c.rms)
        assert np.array_equal(rot[k].view(np.uint32), c.rot.view(np.uint32)) and np.array_equal(tran[k].view(np.uint32), c.tran.view(np.uint32)), c
