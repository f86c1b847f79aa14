"""The merge cases of tests/merge_cases.py on the device: fdgpu_index_merge of LOADED hand-made parts (so k_mg_last_ids runs) against the
list-level Python model, byte for byte and verified; the merge in two rounds (the last ids k_mg_sizes writes); the last ids that remove, split,
rebase, permute, slice and merge leave with their results, shown by merging each result with the part that follows it; the limits of the ABI;
and fdgpu_index_range_bounds / _slice / _save_part on hand-made indices, up to the single-index pipeline with parts in the role of the ranks."""
import ctypes as C

import numpy as np
import pytest

from tests import merge_cases as mc
from tests import postings_step_cases as sc
from tests.test_gpu_postings_steps import SETTINGS

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -4


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


def _eq(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


def _load(ctx, arrays, n, first_id):
    import folddisco_amd as fd
    v, h, o = arrays
    return fd.FolddiscoIndex.load(ctx, h, o, v, n, first_id=first_id)      # loaded: no per-list last ids


def _load_case(ctx, family, name):
    return [_load(ctx, a, n, f) for (f, n, _), a in zip(mc.case(family, name), mc.packed(family, name))]


def _merge(parts):
    import folddisco_amd as fd
    return fd.FolddiscoIndexSet(parts).merge()


def _check(got, want, first_id, n):
    """the resident index equals the model's arrays in everything it reports, and the checker passes it"""
    assert _eq(got.export(), want)
    assert got.num_hashes == len(want[1]) and got.value_len == len(want[0]) and got.num_postings == mc.n_postings(want)
    assert got.first_id == first_id and got.n_structures == n
    rep = got.verify()
    assert rep.ok and rep.n_lists == len(want[1]) and rep.n_postings == mc.n_postings(want), str(rep)


# ---- the merge of every family
@pytest.mark.parametrize("family,name", mc.ALL_CASES)
def test_merge_equals_model(ctx, family, name):
    case, src = mc.case(family, name), mc.packed(family, name)
    parts = _load_case(ctx, family, name)
    ctx.enable_timing(True)
    try:
        got = _merge(parts)
        stages = {s: b for s, _, b in ctx.last_timings()}
    finally:
        ctx.enable_timing(False)
    _check(got, mc.expected(family, name), case[0][0], sum(p[1] for p in case))
    # the bitmap: 2^30 bits up to a largest hash of 2^30 - 1, 2^32 bits from 2^30 on (merge_union reports 4 bytes per hash and 24 per word)
    assert stages["merge_union"] - 4 * sum(len(a[1]) for a in src) == 24 * mc.bitmap_words(case), stages
    for p, a in zip(parts, src):                                           # the sources are as they were
        assert _eq(p.export(), a)
    if len(parts) == 1:
        assert _eq(got.export(), src[0])                                   # one part: a copy


@pytest.mark.parametrize("family,name", [("presence", "subsets3"), ("presence", "parts64"), ("presence", "empties_b"), ("last_step", "steps")])
def test_merge_in_two_rounds(ctx, family, name):
    """(A + B) + C: the continuation in C is re-based against the last ids that the first round wrote (out_last of k_mg_sizes), for a hash
    that B lacks too, and the second round's result carries last ids of hashes that C lacks"""
    case = mc.case(family, name)
    parts = _load_case(ctx, family, name)
    want = mc.expected(family, name)
    first, n = case[0][0], sum(p[1] for p in case)
    ab = _merge(parts[:-1])
    _check(ab, mc.merged(case[:-1]), first, n - case[-1][1])
    abc = _merge([ab, parts[-1]])
    _check(abc, want, first, n)
    _with_probe(ctx, abc, want)


def test_merge_abi_limits(ctx):
    parts = _load_case(ctx, "presence", "parts64")
    extra = _load(ctx, mc.pack_part((640, 10, {11: [645]})), 10, 640)
    L = ctx.L

    def call(ps):
        arr = (C.c_void_p * len(ps))(*[p.h for p in ps])
        h = C.c_void_p(1)                                                  # not null before the call
        rc = L.fdgpu_index_merge(ctx.h, arr, len(ps), C.byref(h))
        assert rc != 0 and h.value is None, (rc, h.value)                  # the out handle stays null
        return rc
    assert call(parts + [extra]) == ERANGE                                 # 65 parts
    assert call([parts[1], parts[0]]) == EINVAL                            # the wrong order
    assert call([parts[0], parts[2]]) == EINVAL                            # a gap in the id ranges
    assert call([parts[0], parts[0]]) == EINVAL                            # the same range twice
    h = C.c_void_p()
    assert L.fdgpu_index_merge(ctx.h, (C.c_void_p * 64)(*[p.h for p in parts]), 64, C.byref(h)) == 0 and h.value      # 64 still pass
    L.fdgpu_index_destroy(h)


# ---- carried last ids: a result merged with the part that follows it (one id per list) shows the last ids it carries
def _with_probe(ctx, got, want):
    first, n = got.first_id, got.n_structures
    probe = mc.probe_part(first, n, want)
    merged = _merge([got, _load(ctx, mc.pack_part(probe), 1, first + n)])
    model = mc.merged((mc.as_part(first, n, want), probe))
    assert len(model[1]) == len(want[1]) and mc.n_postings(model) == mc.n_postings(want) + len(want[1])
    _check(merged, model, first, n + 1)


def _source(ctx, first_id, narrow=False):
    return _load(ctx, sc.source(first_id, narrow), sc.n_structures(narrow), first_id)


@pytest.mark.parametrize("kind", ["around_wide", "below_heads"])
@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_last_ids_of_remove(ctx, first_id, kind):
    got = _source(ctx, first_id).remove(sc.keep_mask(first_id, kind))
    want = sc.removed(first_id, kind)
    assert _eq(got.export(), want)
    _with_probe(ctx, got, want)


@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_last_ids_of_split(ctx, first_id):
    parts = _source(ctx, first_id).split(sc.bounds(first_id))
    for g, w in zip(parts, sc.split_parts(first_id)):
        assert _eq(g.export(), w)
        _with_probe(ctx, g, w)
    _check(_merge(parts), sc.source(first_id, False), first_id, sc.N_WIDE)      # and the parts give the source back


@pytest.mark.parametrize("first_id,new_first_id", sc.REBASES)
def test_last_ids_of_rebase(ctx, first_id, new_first_id):
    want = sc.rebased(first_id, new_first_id)
    src = _source(ctx, first_id)
    got = src.rebase(new_first_id)                                         # of a loaded source: the result carries no last ids either
    assert _eq(got.export(), want)
    _with_probe(ctx, got, want)
    again =_merge([src]).rebase(new_first_id)                             # of a source that carries them
    assert _eq(again.export(), want)
    _with_probe(ctx, again, want)


@pytest.mark.parametrize("setting,first_id,name", [("sort", 0, "shuffle"), ("wide_bitmap_slab", 1 << 28, "reversal"), ("narrow_bitmap_lds", 1 << 28, "shuffle"),
                                                   ("narrow_bitmap_slab", 0, "reversal")])
def test_last_ids_of_permute(ctx, monkeypatch, setting, first_id, name):
    narrow, env, must_run, must_not = SETTINGS[setting]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    src = _source(ctx, first_id, narrow)
    ctx.enable_timing(True)
    try:
        got = src.permute(sc.permutation(narrow, name))
        stages = {n for n, _, _ in ctx.last_timings()}
    finally:
        ctx.enable_timing(False)
    assert must_run <= stages and not must_not & stages, stages
    want = sc.permuted(first_id, narrow, name)
    assert _eq(got.export(), want)
    _with_probe(ctx, got, want)


@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_last_ids_of_slice_and_merge(ctx, first_id):
    src = _source(ctx, first_id)
    want = sc.source(first_id, False)
    h = want[1]
    lo, hi = int(h[2]), int(h[-3]) + 1
    cut = _model_slice(want, lo, hi)
    got = src.slice(lo, hi)                                                # of a loaded index: no last ids to take along
    assert _eq(got.export(), cut)
    _with_probe(ctx, got, cut)
    whole = _merge([src])                                                  # a one-part merge: a copy that carries last ids
    _with_probe(ctx, whole, want)
    got = whole.slice(lo, hi)                                              # ... of which the slice takes its range
    assert _eq(got.export(), cut)
    _with_probe(ctx, got, cut)


# ---- slice and bounds on hand-made indices, the model in numpy
def _model_slice(arrays, lo, hi):
    v, h, o = arrays
    i0, i1 = int(np.searchsorted(h, lo, "left")) if lo <= 0xffffffff else len(h), int(np.searchsorted(h, hi, "left")) if hi <= 0xffffffff else len(h)
    return v[int(o[i0]):int(o[i1])].copy(), h[i0:i1].copy(), (o[i0:i1 + 1] - o[i0]).astype(np.uint64)


def _model_bounds(arrays, n):
    v, h, o = arrays
    H, V = len(h), len(v)
    out = []
    for k in range(1, n):
        i = int(np.searchsorted(o[:H], np.uint64(V * k // n), "left"))      # the first list whose byte offset reaches V k / n
        out.append(int(h[i]) if i < H else 0xffffffff)
    return out


@pytest.fixture(scope="module")
def sliced(ctx):
    """name -> (the model's arrays, first_id, n_structures, the index loaded from them, the index merged from the loaded parts)"""
    out = {}
    for family, name in (("last_step", "steps"), ("hash_space", "wide_top"), ("junction", "a5")):
        case, want = mc.case(family, name), mc.expected(family, name)
        first, n = case[0][0], sum(p[1] for p in case)
        out[name] = (want, first, n, _load(ctx, want, n, first), _merge(_load_case(ctx, family, name)))
    return out


@pytest.mark.parametrize("name", ["steps", "wide_top", "a5"])
def test_range_bounds(sliced, name):
    want, _, _, loaded, merged = sliced[name]
    H = len(want[1])
    for n in (1, 2, 3, 8, H + 5):
        model = _model_bounds(want, n)
        for ix in (loaded, merged):
            got = ix.range_bounds(n)
            assert got.dtype == np.uint32 and got.tolist() == model, n
        assert len(model) == n - 1 and model == sorted(model)
    many = _model_bounds(want, H + 5)
    assert 0xffffffff in many and len(set(many)) < len(many)               # more ranges than lists: equal bounds, and bounds behind the last list

def _ranges(h):
    """(lo, hi) of the slices of an index with the hashes h"""
    H = len(h)
    a, b = int(h[H // 4]), int(h[(3 * H) // 4])
    out = [(a, a), (0, 0), (1 << 32, 1 << 32), (0, 1 << 32), (a, b), (a, b + 1), (int(h[0]), int(h[-1])), (int(h[-1]), 1 << 32)]      # empty, whole, present hashes
    if a + 1 < b and a + 1 not in h:
        out += [(a + 1, b), (a + 1, a + 2), (int(h[-1]) - 1, 1 << 32)]                                                              # bounds between hashes
    return out


@pytest.mark.parametrize("name", ["steps", "wide_top"])
def test_slice_equals_model(ctx, sliced, name):
    want, first, n, loaded, merged = sliced[name]
    ranges = _ranges(want[1])
    if name == "wide_top":
        ranges += [(0xffffffff, 1 << 32), (0xfffffffe, 0xffffffff), (1, 0xffffffff), (1 << 31, (1 << 31) + 1)]      # with and without hash 0xffffffff
        assert any(lo <= 0xffffffff < hi for lo, hi in ranges) and int(want[1][-1]) == 0xffffffff
    seen = set()
    for lo, hi in ranges:
        cut = _model_slice(want, lo, hi)
        assert all(lo <= int(x) < hi for x in cut[1]) and len(cut[1]) == sum(lo <= int(x) < hi for x in want[1])
        seen.add(len(cut[1]))
        for ix in (loaded, merged):                                        # without and with last ids
            got = ix.slice(lo, hi)
            _check(got, cut, first, n)
            if len(cut[1]) and (hi - lo > 1 or lo == 0xffffffff):
                _with_probe(ctx, got, cut)
    assert {0, len(want[1])} <= seen and len(seen) > 3
    assert _eq(loaded.export(), want) and _eq(merged.export(), want)


@pytest.mark.parametrize("family,name,empty", [("junction", "a5", None), ("junction", "a5", 0), ("presence", "subsets3", None), ("presence", "subsets3", 1),
                                               ("hash_space", "wide_top", None)])
def test_single_index_pipeline(ctx, tmp_path, family, name, empty):
    """the parts take the role of the ranks: bounds from part 0, every part sliced at them, the pieces of a range merged, every range written
    into its regions of one PREFIX / PREFIX.offset pair; `empty`: the bounds are set so that this range holds nothing"""
    parts = _load_case(ctx, family, name)
    want = mc.expected(family, name)
    W, H, V = len(parts), len(want[1]), len(want[0])
    assert W in (2, 3)
    b = [int(x) for x in parts[0].range_bounds(W)]
    assert b == _model_bounds(mc.packed(family, name)[0], W)
    if empty is not None:
        b = [0] if W == 2 else [b[0], b[0]]
    edge = [0] + b + [1 << 32]
    ranges = [_merge([p.slice(edge[j], edge[j + 1]) for p in parts]) for j in range(W)]
    for j, r in enumerate(ranges):
        _check(r, _model_slice(want, edge[j], edge[j + 1]), parts[0].first_id, sum(p.n_structures for p in parts))
    assert [r.num_hashes == 0 for r in ranges] == [j == empty for j in range(W)]
    pre = str(tmp_path / "single")
    pos, hb, vb = [], 0, 0
    for r in ranges:
        pos.append((hb, vb))
        hb, vb = hb + r.num_hashes, vb + r.value_len
    assert (hb, vb) == (H, V)
    for j in reversed(range(W)):                                           # the ranks write in any order: the last range first
        ranges[j].save_part(pre, pos[j][0], pos[j][1], H, V, write_header=(j == 0), is_last=(j == W - 1))
    files = mc.file_bytes(*want)
    assert open(pre, "rb").read() == files[0] and open(pre + ".offset", "rb").read() == files[1]
