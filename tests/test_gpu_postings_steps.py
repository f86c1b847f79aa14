"""The step-edge cases of tests/postings_step_cases.py on the device: remove, split, permute (LDS sort, LDS bitmap, global slab) and rebase of a
loaded index whose lists put a wide varint across the 256-byte step of the walks, against the list-level Python model; every result is verified."""
import numpy as np
import pytest

from tests import postings_step_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


def _eq(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


def _load(ctx, first_id, narrow=False):
    import folddisco_amd as fd
    v, h, o = sc.source(first_id, narrow)
    return fd.FolddiscoIndex.load(ctx, h, o, v, sc.n_structures(narrow), first_id=first_id)      # loaded: no per-list last ids


def _check(got, want, first_id, n):
    assert _eq(got.export(), want)
    rep = got.verify()
    assert rep.ok and rep.n_lists == len(want[1]) and rep.n_postings == got.num_postings, str(rep)
    assert got.first_id == first_id and got.n_structures == n


@pytest.mark.parametrize("kind", ["around_wide", "below_heads"])
@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_remove(ctx, first_id, kind):
    ix = _load(ctx, first_id)
    keep = sc.keep_mask(first_id, kind)
    got = ix.remove(keep)
    want = sc.removed(first_id, kind)
    _check(got, want, first_id, int(keep.sum()))
    assert got.num_postings == sum(len(sc.decode(bytes(want[0][int(a):int(b)]))) for a, b in zip(want[2], want[2][1:]))
    assert _eq(ix.export(), sc.source(first_id, False))


@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_split(ctx, first_id):
    ix = _load(ctx, first_id)
    b = sc.bounds(first_id)
    parts = ix.split(b)
    want = sc.split_parts(first_id)
    assert len(parts) == len(want) == 3
    for r, (g, w) in enumerate(zip(parts, want)):
        _check(g, w, int(b[r]), int(b[r + 1] - b[r]))
    assert sum(p.num_postings for p in parts) == ix.num_postings


SETTINGS = {      # name -> (narrow index, environment, the write stages that must have run and the one that must not)
    "sort": (False, {}, {"permute_write_sort"}, {"permute_write_lds", "permute_write_slab"}),
    "wide_bitmap_slab": (False, {"FDGPU_PERM_SORT_BYTES": str(sc.SORT_BYTES_LOW)}, {"permute_write_slab"}, {"permute_write_sort", "permute_write_lds"}),
    "narrow_bitmap_lds": (True, {"FDGPU_PERM_SORT_BYTES": str(sc.SORT_BYTES_LOW)}, {"permute_write_lds"}, {"permute_write_sort", "permute_write_slab"}),
    "narrow_bitmap_slab": (True, {"FDGPU_PERM_SORT_BYTES": str(sc.SORT_BYTES_LOW), "FDGPU_PERM_LDS_BITS": str(sc.LDS_BITS_LOW)}, {"permute_write_slab"},
                           {"permute_write_sort", "permute_write_lds"}),
}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("name", sc.PERMUTATIONS)
@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_permute(ctx, monkeypatch, first_id, name, setting):
    narrow, env, must_run, must_not = SETTINGS[setting]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    ix = _load(ctx, first_id, narrow)
    ctx.enable_timing(True)
    try:
        got = ix.permute(sc.permutation(narrow, name))
        stages = {n for n, _, _ in ctx.last_timings()}
    finally:
        ctx.enable_timing(False)
    assert must_run <= stages and not must_not & stages, stages
    _check(got, sc.permuted(first_id, narrow, name), first_id, sc.n_structures(narrow))
    assert got.num_postings == ix.num_postings


@pytest.mark.parametrize("first_id,new_first_id", sc.REBASES)
def test_rebase(ctx, first_id, new_first_id):
    ix = _load(ctx, first_id)
    got = ix.rebase(new_first_id)
    _check(got, sc.rebased(first_id, new_first_id), new_first_id, sc.N_WIDE)
    assert got.num_postings == ix.num_postings
