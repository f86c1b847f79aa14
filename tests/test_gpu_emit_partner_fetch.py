"""The drain of the index build's pair kernel (k_hash.hip, drain2) on hand-made structures at the limits of its queue.  A drain holds up to 64
queue entries (lane i, partner j) in runs of one partner.  The frame layout puts what the speculative descriptor reads into the first 64 bytes
(fd_geom.h, fd_frame) and the drain gathers only those for partner j; the exact routine and the other encodings read the whole frame.  Every
case is built with the default build and compared byte for byte with oracle.build_index.

A host restatement of the kernel's queue (fd_filter_block + the drain loop of k_pair_emit2) states the number of runs of every drain, to show
that the cases reach one run of 64 lanes, 64 runs of one lane and both sides of 16 and 32 runs: the sizes at which a fetch of the partner
frames once per run, 16 runs at a time, changes its path.  That fetch was built and measured and is not in the kernel (HISTORY.md, "Index
build: partner frames once per drain"); the cases stay as the drains any next form of it has to get right.

The restatement needs the order in which k_frames_perm leaves the residues of a structure: by residue type (unhashable ones last), and inside
a type in residue order as long as the residues of the type lie in ONE 64-residue span of the structure (one wavefront of that kernel claims
their slots in lane order; types spread over several wavefronts are ordered by a race).  The cases whose drains depend on the order inside a
type keep every type inside one span; the others (all pairs pass, or one lane per partner) give the same drains for any order."""
import faulthandler

import numpy as np
import pytest

import oracle
from tests import quantiser_edges as qe

pytestmark = pytest.mark.gpu

NH = 0x100          # kind of an unhashable partner (FD_NOT_HASHABLE)
D2_MAX = np.float32(400.0)      # largest f32 whose square root is <= 20


# ---- structures ------------------------------------------------------------------------------------------------------------------------------
def _residues(rng, ca):
    """N, CA, CB of residues at the given CA positions, side chains in random directions (the construction of quantiser_edges._draw)"""
    ca = np.asarray(ca, np.float64)
    n = len(ca)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    w = rng.normal(size=(n, 3))
    w -= (w * u).sum(1)[:, None] * u
    w /= np.linalg.norm(w, axis=1)[:, None]
    cb = ca + rng.uniform(qe.BOND_MIN, qe.BOND_MAX, n)[:, None] * u
    nn = ca + 1.46 * (-0.33 * u + 0.94 * w)
    return nn.astype(np.float32), ca.astype(np.float32), cb.astype(np.float32)


def _layout(structs):
    """[(ca positions, aa)] -> the layout dict of quantiser_edges (to_packed / to_oracle_structs)"""
    rng = np.random.Generator(np.random.PCG64(606))
    N, CA, CB, AA, off = [], [], [], [], [0]
    for ca, aa in structs:
        n, c, b = _residues(rng, ca)
        N.append(n); CA.append(c); CB.append(b); AA.append(np.asarray(aa, np.uint8))
        off.append(off[-1] + len(aa))
    return dict(res_off=np.asarray(off, np.uint64), n_xyz=np.concatenate(N), ca_xyz=np.concatenate(CA), cb_xyz=np.concatenate(CB), aa=np.concatenate(AA))


def _blob(rng, n, radius=8.0):
    """n CA positions inside a ball: every pair is closer than 2 * radius < 20 A"""
    p = rng.normal(size=(n, 3))
    p *= (radius * rng.uniform(0.2, 1.0, n) ** (1 / 3) / np.linalg.norm(p, axis=1))[:, None]
    return p


def _lattice(n, step=100.0):
    g = np.arange(4) * step
    return np.array([[x, y, z] for x in g for y in g for z in g], np.float64)[:n]


def _hub_groups(sizes, sats, step=100.0):
    """hubs of residue type 0 in groups (sizes[g] hubs 3 A apart along x, the groups on a lattice of 100 A) and sats[g] satellites of type 1
    within 8 A of every hub of their group; hubs first, then the satellites group by group"""
    cells = _lattice(len(sizes), step)
    hubs, sat = [], []
    for g, (m, k) in enumerate(zip(sizes, sats)):
        hubs += [cells[g] + [3.0 * a, 0.0, 0.0] for a in range(m)]
        sat += [cells[g] + [1.5 * (m - 1), 4.0 + 0.3 * b, 2.0] for b in range(k)]
    return np.array(hubs + sat), [0] * len(hubs) + [1] * len(sat)


def case_one_partner():
    """65 residues, all within the cutoff: partner 64 passes all 64 lanes of tile 0 -> a drain of one run"""
    rng = np.random.Generator(np.random.PCG64(11))
    return [(_blob(rng, 65), rng.integers(0, 20, 65))]


def case_one_lane_per_partner():
    """64 hubs of type 0 (tile 0), 100 A apart; satellites of type 1 and 2 at 6 A to either side of their hub: each passes one lane only"""
    hubs = _lattice(64)
    return [(np.concatenate([hubs, hubs + [6.0, 0, 0], hubs - [6.0, 0, 0]]), [0] * 64 + [1] * 64 + [2] * 64)]


def case_round_boundary():
    """satellites that pass four lanes (16 partners to a drain) behind a group of three hubs with three satellites, which shifts the alignment
    (17); the same with two lanes per satellite (32) behind a single hub with one satellite (33)"""
    return [_hub_groups([4] * 8 + [3, 1] + [4] * 7, [4] * 8 + [3, 0] + [4] * 7), _hub_groups([2] * 8 + [1, 1] + [2] * 23, [2] * 8 + [1, 0] + [2] * 23)]


def case_short_drains():
    """n = 1 (two residues); n < 64 with several runs (ten residues: 45 pairs); a tile whose last lanes are unhashable or past the end"""
    rng = np.random.Generator(np.random.PCG64(13))
    aa = rng.integers(0, 20, 100)
    aa[90:] = 255
    return [(_blob(rng, 2, 3.0), [3, 7]), (_blob(rng, 10), rng.integers(0, 20, 10)), (_blob(rng, 100, 9.0), aa), (_blob(rng, 67), rng.integers(0, 20, 67))]


CASES = {"one partner": case_one_partner, "one lane per partner": case_one_lane_per_partner, "round boundary": case_round_boundary,
         "short drains": case_short_drains}


# ---- the kernel's queue, restated --------------------------------------------------------------------------------------------------------------
def drain_runs(ca, aa):
    """number of runs (stretches of one partner) of every drain the pair kernel makes for one structure, tile by tile, in the kernel's order"""
    aa = np.asarray(aa).astype(np.int64)
    ok = aa < 20
    order = np.argsort(np.where(ok, aa, 20), kind="stable")          # k_frames_perm: by type, unhashable last (see the module docstring)
    ca = np.asarray(ca, np.float32)[order]
    kind = np.where(ok[order], aa[order], NH)
    n = len(aa)
    d = ca[:, None, :] - ca[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]      # f32, fd_dist2's order
    passes = ~(d2 > D2_MAX) & (kind != NH)[:, None] & (kind != NH)[None, :]
    out = []
    for i0 in range(0, n, 64):
        lanes = np.arange(i0, min(i0 + 64, n))
        q = []
        for jb in range(i0, n, 64):
            kb = np.full(64, NH, np.int64)
            kb[: min(64, n - jb)] = kind[jb: jb + 64]
            hashable = np.nonzero(kb != NH)[0]
            nk = int(hashable[-1]) + 1 if len(hashable) else 0
            last_block = jb + 64 >= n
            nkf = 1 if (last_block and nk == 0) else nk
            k = 0
            while k < nkf:
                ke = k + 1
                while ke < 64 and kb[ke] == kb[ke - 1]:
                    ke += 1
                ke = min(ke, nkf)
                run_last = last_block and ke >= nkf
                dead = kb[k] == NH
                if dead and not run_last:
                    k = ke
                    continue
                while True:
                    for kk in (k, k + 1):
                        if kk < ke and not dead:
                            j = jb + kk
                            m = passes[lanes, j] & ((lanes < j) if jb == i0 else True)
                            q += [j] * int(np.count_nonzero(m))
                    k += 2
                    last = run_last and k >= ke
                    while len(q) >= 64 or (last and q):
                        take = q[-64:]
                        del q[-64:]
                        out.append(1 + sum(1 for a, b in zip(take, take[1:]) if a != b))
                    if k >= ke:
                        break
                k = ke
    return out


def rounds_of(runs):
    """(drains of more than 16, 32, 48 runs: 2, 3, 4 rounds of 16) of a list of run counts"""
    r = [(x + 15) // 16 for x in runs]
    return tuple(r.count(k) for k in (2, 3, 4))


def _restate(structs):
    runs = []
    for ca, aa in structs:
        runs += drain_runs(ca, aa)
    return runs


def test_restatement_covers_the_limits():
    """the hand-made cases reach 1, 16, 17, 32, 33 and 64 runs in a drain (no GPU work: the restatement alone)"""
    seen = set()
    for name, make in CASES.items():
        runs = _restate(make())
        print(f"{name}: {len(runs)} drains, runs per drain {sorted(set(runs))}, rounds (2, 3, 4) {rounds_of(runs)}")
        seen |= set(runs)
    assert {1, 16, 17, 32, 33, 64} <= seen, sorted(seen)
    assert 64 in _restate(case_one_lane_per_partner()) and 1 in _restate(case_one_partner())
    assert rounds_of(_restate(case_one_partner())) == (0, 0, 0) and rounds_of(_restate(case_one_lane_per_partner())) == (0, 0, 3)
    assert rounds_of(_restate(case_round_boundary())) == (4, 3, 0)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    faulthandler.dump_traceback_later(600, exit=True)
    c = fd.Context(0)
    yield c
    c.close()
    faulthandler.cancel_dump_traceback_later()


def _default_env(monkeypatch):
    for k in ("FDGPU_DTAB", "FDGPU_EXACT", "FDGPU_MSD"):
        monkeypatch.delenv(k, raising=False)


def _assert_index(got, oix, what):
    v, h, o = got
    assert np.array_equal(h, oix.hashes()), (what, "hashes")
    assert np.array_equal(o, oix.offsets()), (what, "offsets")
    assert np.array_equal(v, oix.values()), (what, "values")


@pytest.mark.parametrize("name", list(CASES))
def test_hand_made_case_equals_oracle(ctx, monkeypatch, name):
    import folddisco_amd as fd
    _default_env(monkeypatch)
    d = _layout(CASES[name]())
    got = fd.FolddiscoIndex.build(ctx, ctx.upload(qe.to_packed(d))).export()
    oix, _, _ = oracle.build_index(qe.to_oracle_structs(d))
    assert oix.H > 0
    _assert_index(got, oix, name)


def test_exact_routine_keeps_its_own_loads(ctx, monkeypatch):
    """pairs of the torsion reversal set (one structure per pair: every drain holds one entry, one run): the disagreeing ones take the exact
    routine, which loads all five words of both frames itself"""
    import folddisco_amd as fd
    from tests import torsion_reversal_cases as trc
    _default_env(monkeypatch)
    rs = trc.reversal_set()
    d = rs.per_pair()
    ctx.spec_fallbacks()
    got = fd.FolddiscoIndex.build(ctx, ctx.upload(qe.to_packed(d))).export()
    n_fb = ctx.spec_fallbacks()
    oix, _, _ = oracle.build_index(qe.to_oracle_structs(d))
    _assert_index(got, oix, "reversal set")
    assert n_fb >= int(rs.disagree.any(1).sum()) > 0


def test_other_encoding_loads_whole_frames(ctx, monkeypatch):
    """PDBMotif goes through fd_pair_both, which reads s2 / nv2 of the reordered frame: the blob and hub structures under hash type 0"""
    import folddisco_amd as fd
    _default_env(monkeypatch)
    d = _layout(case_short_drains() + case_one_lane_per_partner())
    got = fd.FolddiscoIndex.build(ctx, ctx.upload(qe.to_packed(d)), hash_type=0).export()
    with oracle.hash_type(0):
        oix, _, _ = oracle.build_index(qe.to_oracle_structs(d))
    assert oix.H > 0
    _assert_index(got, oix, "pdbmotif")


def test_synthetic_database(ctx, monkeypatch):
    """synth.generate(2048, seed=1): index equal to the oracle's, and the same pairs fall back as before the frame was reordered (6,039 of
    33,431,018: frame bits do not change).  With the fetch of partner frames once per run, 7,733 of its 522,360 or more drains held more than
    16 runs (7,727 of 17 to 32, 6 of 33 to 48, none beyond): 1.5 %."""
    import folddisco_amd as fd
    from folddisco_amd import synth
    from tests.helpers import packed_to_oracle_structs
    _default_env(monkeypatch)
    ps = synth.to_packed(synth.generate(2048, seed=1))
    ctx.spec_fallbacks()
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(ps))
    n_fb = ctx.spec_fallbacks()
    pairs = ix.num_postings // 2
    print(f"pairs {pairs}, fallbacks {n_fb}")
    oix, _, _ = oracle.build_index(packed_to_oracle_structs(ps))
    _assert_index(ix.export(), oix, "synth 2048")
    assert (n_fb, pairs) == (6039, 33431018)
