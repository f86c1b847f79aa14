"""The step-edge cases of tests/postings_step_cases.py on the host, no GPU: the shape the cases rely on, and fdgpu_split_host, fdgpu_permute_host
and fdgpu_rebase_host (indexio) against the list-level Python model on the same arrays."""
import numpy as np
import pytest

from folddisco_amd import indexio
from tests import postings_step_cases as sc


def _eq(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3


@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_cases_have_the_edges(first_id):
    ls = sc.lists_of(first_id, False)
    by_name = {name: (ids, wide) for name, ids, wide in ls}
    v, h, o = sc.source(first_id, False)
    lens = dict(zip([name for name, _, _ in ls], np.diff(o.astype(np.int64)).tolist()))
    assert int(o[-1]) == len(v) and len(h) == len(ls) == 15 + 6 + 3
    assert indexio.verify_host(v, h, o, sc.N_WIDE, first_id=first_id).ok
    assert len(sc.varint(first_id + sc.HEAD)) == (5 if first_id else 1)
    for w in sc.WIDTHS:
        assert len(sc.varint(sc.WIDE_DELTA[w])) == w
        for p in sc.STARTS:
            ids, wide = by_name[f"straddle_w{w}_p{p}"]
            (k, start, width), = wide
            assert (start, width) == (p, w) and len(ids) == k + 1 + sc.TAIL and lens[f"straddle_w{w}_p{p}"] == p + w + sc.TAIL
            # the split bounds: one inside the one-byte run, one between the two ids around the wide delta
            assert ids[0] < first_id + sc.RUN_MID <= ids[k - 1] < first_id + sc.RUN_END <= ids[k]
        assert {p for p in sc.STARTS if p < 256 < p + w} == set(range(256 - w + 1, 256))      # every straddle of the step edge
    for n in sc.EXACT_LENGTHS:
        assert lens[f"exact_{n}"] == n
    for w1, w2 in sc.MULTI:
        ids, wide = by_name[f"multi_w{w1}_w{w2}"]
        assert [(s, w) for _, s, w in wide] == [(255, w1), (513 - w2, w2)] and lens[f"multi_w{w1}_w{w2}"] > 512      # three steps, both edges straddled
        assert ids[wide[0][0] - 1] < first_id + sc.RUN_END <= ids[wide[0][0]]
    # remove: "around_wide" drops an id inside every list that has a wide delta (RE-ENCODE), "below_heads" none inside any but some below every head (RE-BASE)
    around, below = sc.keep_mask(first_id, "around_wide"), sc.keep_mask(first_id, "below_heads")
    for name, ids, wide in ls:
        loc = np.array(ids) - first_id
        assert not around[loc].all() and below[loc].all() and not below[:loc[0]].all(), name
        for k, _, _ in wide:
            assert not around[loc[k - 1]] and (k + 1 == len(ids) or not around[loc[k + 1]])
    narrow = sc.lists_of(first_id, True)
    assert [e for e in ls if all(w < 4 for _, _, w in e[2])] == narrow and 0 < len(narrow) < len(ls)
    assert indexio.verify_host(*sc.source(first_id, True), sc.N_NARROW, first_id=first_id).ok
    assert sc.LDS_BITS_LOW < sc.N_NARROW and sc.SORT_BYTES_LOW < min(lens.values())


def test_removed_model_on_a_small_list():
    """the model itself on something checked by hand: ids 3 5 9 of first_id 0, structures 1 and 5 dropped -> 2 7"""
    keep = np.ones(10, np.uint8)
    keep[[1, 5]] = 0
    new = np.concatenate([[0], np.cumsum(keep)])
    assert [int(new[x]) for x in [3, 5, 9] if keep[x]] == [2, 7]
    assert sc.pack([[2, 7], [], [300]], [1, 4, 7])[1].tolist() == [1, 7] and sc.pack([[2, 7], [], [300]], [1, 4, 7])[0].tolist() == [2, 5, 0xac, 2]


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_split_host_equals_model(first_id, threads):
    src = sc.source(first_id, False)
    keep = [x.copy() for x in src]
    got = indexio.split_host(*src, sc.bounds(first_id), first_id=first_id, threads=threads)
    want = sc.split_parts(first_id)
    assert len(got) == len(want) == 3
    b = sc.bounds(first_id)
    for r, (g, w) in enumerate(zip(got, want)):
        assert _eq(g, w), r
        assert len(w[1]) > 0 and indexio.verify_host(*g, n_structures=int(b[r + 1] - b[r]), first_id=int(b[r])).ok
    assert _eq(src, keep)


@pytest.mark.parametrize("name", sc.PERMUTATIONS)
@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_permute_host_equals_model(first_id, narrow, name):
    src = sc.source(first_id, narrow)
    got = indexio.permute_host(*src, sc.permutation(narrow, name), first_id=first_id, threads=2)
    assert _eq(got, sc.permuted(first_id, narrow, name))
    assert indexio.verify_host(*got, n_structures=sc.n_structures(narrow), first_id=first_id).ok
    if name == "identity":
        assert _eq(got, src)


@pytest.mark.parametrize("first_id,new_first_id", sc.REBASES)
def test_rebase_host_equals_model(first_id, new_first_id):
    src = sc.source(first_id, False)
    got = indexio.rebase_host(*src, first_id, new_first_id, sc.N_WIDE, threads=2)
    assert _eq(got, sc.rebased(first_id, new_first_id))
    assert indexio.verify_host(*got, n_structures=sc.N_WIDE, first_id=new_first_id).ok
    assert len(got[0]) != len(src[0])                                      # the head width changed
