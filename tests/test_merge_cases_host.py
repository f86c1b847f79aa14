"""The merge cases of tests/merge_cases.py on the host, no GPU: the model checked against itself and the cases against their coverage, then
fdgpu_merge_subindices (indexio.merge_subindices) over every family against the model, its refusal of id ranges that do not ascend, and the
results of fdgpu_split_host, fdgpu_rebase_host and fdgpu_permute_host over the step-edge lists merged with the part that follows them."""
import numpy as np
import pytest

from folddisco_amd import indexio
from tests import merge_cases as mc
from tests import postings_step_cases as sc


def _eq(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


@pytest.fixture
def no_device(monkeypatch):
    import folddisco_amd as fd

    def boom(*a, **k):
        raise AssertionError("a device was touched by a host-side merge")
    monkeypatch.setattr(fd, "Context", boom)


def test_model_on_lists_checked_by_hand():
    """ids 3 5 | 300 of two parts -> 03 02 a7 02 (300 - 5 = 295 = 0x127); a hash of the second part alone keeps its absolute head"""
    parts = ((0, 10, {7: [3, 5], 9: [1]}), (10, 500, {7: [300], 8: [200]}))
    v, h, o = mc.merged(parts)
    assert v.tolist() == [3, 2, 0xa7, 0x02, 0xc8, 0x01, 1] and h.tolist() == [7, 8, 9] and o.tolist() == [0, 4, 6, 7]
    assert mc.pack_part(parts[1])[0].tolist() == [0xac, 0x02, 0xc8, 0x01] and mc.n_postings((v, h, o)) == 5
    val, off = mc.file_bytes(v, h, o)
    assert val == bytes(v) and len(off) == 8 + 4 * 3 + 8 * 4 and off[:8] == (3).to_bytes(8, "little") and off[8:12] == (7).to_bytes(4, "little")
    assert off[-8:] == (7).to_bytes(8, "little")
    assert mc.probe_part(10, 500, mc.pack_part(parts[1])) == (510, 1, {7: [510], 8: [510]})


@pytest.mark.parametrize("family,name", mc.ALL_CASES)
def test_model_self_checks(family, name):
    """every part is well formed, every expected list ascends strictly inside the declared ranges, and the host checker agrees"""
    parts = mc.case(family, name)                # the generators assert their coverage on the way
    mc.check_parts(parts)
    want = mc.expected(family, name)
    first, n = parts[0][0], sum(p[1] for p in parts)
    lists = mc.lists_of(want)
    assert list(lists) == sorted(lists) == sorted(set().union(*[p[2] for p in parts]))
    for ids in lists.values():
        assert first <= ids[0] and ids[-1] < first + n and all(a < b for a, b in zip(ids, ids[1:]))
    assert sum(len(l) for l in lists.values()) == sum(len(l) for p in parts for l in p[2].values())
    assert int(want[2][-1]) == len(want[0]) <= sum(len(a[0]) for a in mc.packed(family, name))      # a re-based head is never longer
    assert len(lists) < 600                                                                        # a few hundred lists at the most
    if lists:
        rep = indexio.verify_host(*want, n_structures=n, first_id=first)
        assert rep.ok and rep.n_lists == len(lists) and rep.n_postings == mc.n_postings(want), str(rep)


def test_coverage_of_the_families():
    pairs, deltas = mc.junction_pairs([mc.case("junction", f"a{a}") for a in range(1, 6)])
    assert len(pairs) == 15 and all({b - 1, b} <= deltas for b in mc.BOUNDARIES)
    assert [len(mc.varint(mc.junction_first_id(a))) for a in range(1, 6)] == [1, 2, 3, 4, 5]
    top = mc.case("junction", "top")
    assert top[1][0] + top[1][1] == mc.ID_TOP and max(l[-1] for l in top[1][2].values()) == mc.ID_TOP - 1
    ls = mc.last_step_lists()
    assert len(ls) == 2 * 4 * 10 + 9 and {len(mc.encode(ids)) for _, ids, _ in ls} >= set(mc.STEP_LENGTHS)
    steps = mc.case("last_step", "steps")
    assert set(steps[1][2]) == set(steps[0][2]) and len(steps) == 3                    # every list of part 0 goes on in part 1
    assert len(mc.case("presence", "parts64")) == mc.MAX_PARTS and len(mc.case("presence", "one_part")) == 1


@pytest.mark.parametrize("family,name", mc.ALL_CASES)
def test_host_merge_equals_model(no_device, family, name):
    src = mc.packed(family, name)
    got = indexio.merge_subindices([tuple(a.copy() for a in p) for p in src])
    assert _eq(got, mc.expected(family, name))


def test_host_merge_at_the_top_of_the_id_space(no_device):
    """the host merge takes arrays alone, so here a list may end at id 2^32 - 1 (a resident index keeps that id free: mc.ID_TOP)"""
    parts = mc.junction_top(1 << 32)
    mc.check_parts(parts)
    want = mc.merged(parts)
    assert max(l[-1] for l in mc.lists_of(want).values()) == (1 << 32) - 1
    assert _eq(indexio.merge_subindices([mc.pack_part(p) for p in parts]), want)


def test_host_merge_in_two_rounds(no_device):
    for family, name in (("presence", "subsets3"), ("last_step", "steps")):
        src = mc.packed(family, name)
        ab = indexio.merge_subindices(list(src[:2]))
        assert _eq(indexio.merge_subindices([ab, src[2]]), mc.expected(family, name))


def test_host_merge_refuses_ranges_that_do_not_ascend(no_device):
    a, b = mc.pack_part((0, 100, {4: [10, 20], 9: [5]})), mc.pack_part((100, 100, {4: [120], 8: [150]}))
    assert _eq(indexio.merge_subindices([a, b]), mc.merged(((0, 100, {4: [10, 20], 9: [5]}), (100, 100, {4: [120], 8: [150]}))))
    with pytest.raises(RuntimeError, match="ascending id ranges"):
        indexio.merge_subindices([b, a])                                               # 10 follows 120
    with pytest.raises(RuntimeError, match="ascending id ranges"):
        indexio.merge_subindices([a, mc.pack_part((20, 100, {4: [20]}))])              # an equal id: the delta would be 0


# ---- carried last ids, host forms: the result of an operation over the step-edge lists, merged with the part that follows it
def _with_probe(got, first_id, n):
    want = mc.merged((mc.as_part(first_id, n, got), mc.probe_part(first_id, n, got)))
    merged = indexio.merge_subindices([got, mc.pack_part(mc.probe_part(first_id, n, got))])
    assert _eq(merged, want) and len(want[1]) == len(got[1]) and mc.n_postings(want) == mc.n_postings(got) + len(got[1])


@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_split_host_then_merge(no_device, first_id):
    b = sc.bounds(first_id)
    parts = indexio.split_host(*sc.source(first_id, False), b, first_id=first_id, threads=2)
    for r, (g, w) in enumerate(zip(parts, sc.split_parts(first_id))):
        assert _eq(g, w)
        _with_probe(g, int(b[r]), int(b[r + 1] - b[r]))
    assert _eq(indexio.merge_subindices(parts), sc.source(first_id, False))            # and the parts give the source back


@pytest.mark.parametrize("first_id,new_first_id", sc.REBASES)
def test_rebase_host_then_merge(no_device, first_id, new_first_id):
    got = indexio.rebase_host(*sc.source(first_id, False), first_id, new_first_id, sc.N_WIDE, threads=2)
    assert _eq(got, sc.rebased(first_id, new_first_id))
    _with_probe(got, new_first_id, sc.N_WIDE)


@pytest.mark.parametrize("name", sc.PERMUTATIONS)
@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_permute_host_then_merge(no_device, first_id, name):
    got = indexio.permute_host(*sc.source(first_id, True), sc.permutation(True, name), first_id=first_id, threads=2)
    assert _eq(got, sc.permuted(first_id, True, name))
    _with_probe(got, first_id, sc.N_NARROW)
