"""Which form fdgpu_make_query_map[_batch] takes for "candidates -> hashes", at the switches of its dispatch (csrc/fd_query_map.hip, qm_choose_form),
read back through fdgpu_debug_last_query_map_path after every call.  The expected flags are the dispatch's rule restated here and evaluated on what
the call returned: with the default cutoff a pair of the default encoding is valid exactly when it enters the observed-distance list (CA distance
<= 20 A), so n_valid = n_aad, and per_pair = 1 + 2 (n_dist_fields n_dist + n_angle_fields n_angle) with 2 and 3 fields.  Synthetic structures of
at most 150 residues; every call takes milliseconds."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOST, DEVICE, CHAIN, CHAIN_LEN, SORT = 1, 2, 4, 8, 16


def per_pair(n_dist, n_angle):
    return 1 + 2 * (2 * n_dist + 3 * n_angle)


def expected(n_valid, pp, n_dist, n_angle, mode=None, subs=False, bins=False, lengths=False):
    """the dispatch's rule; n_valid: valid pairs per query; lengths: an index whose length table exists was given"""
    nc = sum(n_valid) * pp
    dev = not subs and not bins and n_dist <= 8 and n_angle <= 8 and mode != "0" and sum(n_valid) > 0 and nc < 2 ** 31
    sort = dev and len(n_valid) == 1 and nc >= (1 if mode == "1" else 32768)
    chain = dev and not sort and max(n_valid) * pp <= 2048 and mode != "2"
    return (DEVICE if dev else HOST) | (CHAIN if chain else 0) | (CHAIN_LEN if chain and lengths else 0) | (SORT if sort else 0)


@pytest.fixture(scope="module")
def env():
    import folddisco_amd as fd
    from tests.helpers import synthetic_packed
    ctx = fd.Context(0)
    ps = synthetic_packed(4, 4242, lengths=np.array([150, 60, 40, 25]))
    sb = ctx.upload(ps)
    ix = fd.FolddiscoIndex.build(ctx, sb)
    h, n = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    ctx.check(ctx.L.fdgpu_posting_lengths(ctx.h, ix.h, h.ctypes.data_as(C.POINTER(C.c_uint32)), 1, n.ctypes.data_as(C.POINTER(C.c_uint64))))          # the index's length table exists from here on
    yield ctx, sb, ix
    ctx.close()


def flags(ctx):
    f = C.c_uint32(0xdead)
    ctx.check(ctx.L.fdgpu_debug_last_query_map_path(ctx.h, C.byref(f)))
    return f.value


def run(ctx, sb, queries, index=None, dthr=(0.5,), athr=(5.0,), **kw):
    """-> (flags, n_aad per query)"""
    from folddisco_amd import query as fq
    maps = fq.make_query_maps(ctx, sb, queries, index, 4.0, dist_thr=dthr, angle_thr=athr, **kw)
    return flags(ctx), [len(m.aad_dist) for m in maps]


def first(m):
    return np.arange(m, dtype=np.uint32)


def test_one_query_on_either_side_of_the_sort_dedupe_switch(env, monkeypatch):
    ctx, sb, ix = env
    monkeypatch.delenv("FDGPU_QM_DEVICE", raising=False)
    sizes = list(range(60, 151, 3))
    n_valid = {m: run(ctx, sb, [(0, first(m))], None, (), ())[1][0] for m in sizes}          # does not depend on the thresholds
    cases = [(n_valid[m] * per_pair(a, b), m, a, b) for m in sizes for a in range(9) for b in range(9)]
    below, above = max(c for c in cases if c[0] < 32768), min(c for c in cases if c[0] >= 32768)          # per_pair is odd: 32,768 itself is mostly out of reach
    assert 32768 - below[0] < 328 and above[0] - 32768 < 328, (below, above)          # the fixture has a case within 1 % on each side
    for nc, m, a, b in (below, above):
        dthr, athr = tuple(0.25 * (k + 1) for k in range(a)), tuple(2.5 * (k + 1) for k in range(b))
        for index in (None, ix):
            got, n_aad = run(ctx, sb, [(0, first(m))], index, dthr, athr)
            assert n_aad == [n_valid[m]]
            want = expected(n_aad, per_pair(a, b), a, b, lengths=index is not None)
            assert got == want and want == (DEVICE | SORT if nc >= 32768 else DEVICE), (nc, m, a, b, got, want)


def test_batch_on_either_side_of_the_chain_switch(env, monkeypatch):
    ctx, sb, ix = env
    monkeypatch.delenv("FDGPU_QM_DEVICE", raising=False)
    pp = per_pair(1, 1)          # 11 candidates per pair: 14 residues give 2,002 insertions, 15 give 2,310 when every pair is valid
    n_valid = {m: run(ctx, sb, [(0, first(m))])[1][0] for m in range(8, 26)}
    fits, beyond = max(m for m in n_valid if n_valid[m] * pp <= 2048), min(m for m in n_valid if n_valid[m] * pp > 2048)
    assert n_valid[fits] * pp > 1500 and n_valid[beyond] * pp < 2600, (n_valid[fits], n_valid[beyond])
    small = [(1, np.array([3, 9, 20, 41], np.uint32)), (2, first(6)), (3, np.array([5, 5, 9], np.uint32)), (1, np.array([1000, 3], np.uint32)), (2, np.zeros(0, np.uint32))]
    for m, chain in ((fits, True), (beyond, False)):
        for index in (None, ix):
            got, n_aad = run(ctx, sb, small + [(0, first(m))] + small[:2], index)
            assert max(n_aad) == n_valid[m] and sum(n_aad) > n_valid[m]
            want = expected(n_aad, pp, 1, 1, lengths=index is not None)
            assert got == want and want == (DEVICE | ((CHAIN | (CHAIN_LEN if index is not None else 0)) if chain else 0)), (m, got, want)


def test_chain_takes_the_lengths_once_the_index_has_its_length_table(env, monkeypatch):
    import folddisco_amd as fd
    ctx, sb, _ = env
    monkeypatch.delenv("FDGPU_QM_DEVICE", raising=False)
    fresh = fd.FolddiscoIndex.build(ctx, sb)
    q = [(1, first(7)), (2, first(5))]
    assert run(ctx, sb, q, fresh)[0] == DEVICE | CHAIN          # the host-side lookup of this call makes the table
    assert run(ctx, sb, q, fresh)[0] == DEVICE | CHAIN | CHAIN_LEN


def test_substitutions_bin_lists_and_long_threshold_lists_take_the_host_form(env, monkeypatch):
    ctx, sb, ix = env
    monkeypatch.delenv("FDGPU_QM_DEVICE", raising=False)
    plain = [(1, first(7)), (2, first(5)), (3, first(4))]
    assert run(ctx, sb, plain, ix)[0] == DEVICE | CHAIN | CHAIN_LEN
    subbed = [plain[0], (2, first(5), [None, None, [3], None, None]), plain[2]]          # one substituted residue in the batch
    got, n_aad = run(ctx, sb, subbed, ix)
    assert got == HOST == expected(n_aad, per_pair(1, 1), 1, 1, subs=True, lengths=True)
    got, n_aad = run(ctx, sb, plain, ix, multiple_bins=[(16, 4), (8, 3)])
    assert got == HOST == expected(n_aad, per_pair(1, 1), 1, 1, bins=True, lengths=True)
    nine = tuple(0.1 * (k + 1) for k in range(9))
    got, n_aad = run(ctx, sb, plain, ix, dthr=nine)
    assert got == HOST == expected(n_aad, per_pair(9, 1), 9, 1, lengths=True)
    got, n_aad = run(ctx, sb, plain[1:], ix, dthr=nine[:8], athr=nine[:8])          # eight of each still go to the device: 81 candidates a pair, 20 pairs at most
    assert got == DEVICE | CHAIN | CHAIN_LEN == expected(n_aad, per_pair(8, 8), 8, 8, lengths=True)
    got, n_aad = run(ctx, sb, [(3, np.array([2, 1000], np.uint32))], ix)          # no valid pair: nothing for the device to expand
    assert n_aad == [0] and got == HOST


@pytest.mark.parametrize("mode,want", (("0", HOST), ("1", DEVICE | SORT), ("2", DEVICE), (None, DEVICE | CHAIN | CHAIN_LEN)))
def test_forced_forms(env, monkeypatch, mode, want):
    """FDGPU_QM_DEVICE: 0 the host form, 1 the sort-based dedupe for one query of any size, 2 device expansion without the chain"""
    ctx, sb, ix = env
    if mode is None:
        monkeypatch.delenv("FDGPU_QM_DEVICE", raising=False)
    else:
        monkeypatch.setenv("FDGPU_QM_DEVICE", mode)
    got, n_aad = run(ctx, sb, [(1, first(9))], ix)
    assert got == want == expected(n_aad, per_pair(1, 1), 1, 1, mode=mode, lengths=True)
    got, n_aad = run(ctx, sb, [(1, first(9)), (2, first(4))], ix)          # two queries: the sort-based dedupe is for one
    assert got == expected(n_aad, per_pair(1, 1), 1, 1, mode=mode, lengths=True) == (DEVICE | CHAIN | CHAIN_LEN if mode == "1" else want)


def test_refusals_come_with_their_messages(env, monkeypatch):
    import folddisco_amd as fd
    ctx, sb, ix = env
    monkeypatch.delenv("FDGPU_QM_DEVICE", raising=False)
    assert run(ctx, sb, [(1, first(7))], ix)[0] == DEVICE | CHAIN | CHAIN_LEN
    with pytest.raises(fd.api.FdgpuError, match=r"libfdgpu error -1: multiple_bins: at most 8 \(dist, angle\) bin pairs, no zero counts"):
        run(ctx, sb, [(1, first(7))], ix, multiple_bins=[(16, 0)])
    with pytest.raises(fd.api.FdgpuError, match=r"libfdgpu error -1: hash_type: only the encodings over the \(d_CA, d_CB, theta, tau1, tau2\) descriptor are built"):
        run(ctx, sb, [(1, first(7))], ix, hash_type=9)
    assert ctx.L.fdgpu_debug_last_query_map_path(ctx.h, None) != 0
