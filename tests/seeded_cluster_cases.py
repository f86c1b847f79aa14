"""Shared cases of the seeded signature clusters tests (host and device): the grid of drops S and seed tables T cut from one hand-made table,
the planted cases in three placements, the tables of the concatenation property, and an independent brute force over the eq / E matrices
of the concatenated table [T; S].  No product code is used here.

Ids of the brute force are the combined ones of the definition while it walks: seed j is j, position p of S is nT + p.  A record that names
a seed carries SEED in its flags and the seed's position in T, any other a position in S."""
import functools

import numpy as np

from tests import cluster_cases as cc
from tests import signature_cases as sc      # noqa: F401  (the tables of cluster_cases come from it)

B = cc.B
NS = (1, 64, 65, 256, 257, 513)
NTS = (0, 1, 64, 65, 257, 700)
THRESHOLDS = cc.THRESHOLDS
ORDERS = cc.ORDERS
SEED_SPLITS = (1, 2, 3, 7, 1000)
WALK_SPLITS = (1, 7)
SPLIT_CELLS = ((257, 700), (513, 257))
CONCAT_CELLS = ((257, 257), (513, 65), (65, 700))
NO_ID = cc.NO_ID
EMPTY = cc.EMPTY
IDENTICAL, SEED = 1, 2
# the layouts of include/fdgpu.h (fd_signature, fd_sig_neighbor), stated here: the brute force of the grid runs when this module is imported
SDT = np.dtype([("n", "<u4"), ("reserved", "<u4"), ("d0", "<u8"), ("d1", "<u8"), ("sk", "<u4", (64,))])
DT = np.dtype([("id", "<u4"), ("match", "u1"), ("filled", "u1"), ("flags", "<u2")])


def tables(n, nT, dtype):
    """-> (S, T): a drop of n and a seed table of nT records, a random cut of one table so that groups reach across the two"""
    X = cc.table(n + nT, dtype)
    perm = np.random.Generator(np.random.PCG64(811 + n + 7 * nT)).permutation(n + nT)
    return X[perm[nT:]].copy(), X[perm[:nT]].copy()


def matrices(S, X):
    """eq, E -> match, filled of every position of S (rows) with every combined id (columns)"""
    eq = (S["sk"][:, None, :] == X["sk"][None, :, :]).sum(-1)
    E = ((S["sk"] == EMPTY)[:, None, :] & (X["sk"] == EMPTY)[None, :, :]).sum(-1)
    return eq - E, 64 - E


def brute_seeded(S, order, thr64, T, dtype, mats=None):
    """the definition, one position after the other: the candidates are the seeds with n > 0 and the representatives chosen so far, the
    nearest is the largest match / filled (a quotient of integers up to 64: equal fractions give equal doubles, different ones differ by more
    than 1 / 4096), then the largest filled, then the smallest combined id"""
    n, nT = len(S), len(T)
    X = np.concatenate([T, S]) if nT else S
    order = np.arange(n) if order is None else np.asarray(order)
    match, filled = matrices(S, X) if mats is None else mats
    out = np.zeros(n, dtype)
    out["id"] = NO_ID
    cand = np.zeros(nT + n, bool)                    # over combined ids
    cand[:nT] = T["n"] > 0
    for p in order.tolist():
        if S["n"][p] == 0:
            continue
        x = nT + p
        m, f = match[p], filled[p]
        ok = cand & (f > 0) & (m * 64 >= thr64 * f)
        c = np.nonzero(ok)[0]
        if not len(c):
            k = int((S["sk"][p] != EMPTY).sum())
            out[p] = (p, k, k, IDENTICAL)
            cand[x] = True
            continue
        ratio = m[c] / f[c]
        c = c[ratio == ratio.max()]
        c = c[f[c] == f[c].max()]
        r = int(c.min())
        for q in c.tolist():                         # the total order, stated with integers
            assert q == r or cc.nearer(m[r], f[r], r, m[q], f[q], q)
        same = int(X["n"][r] == S["n"][p] and X["d0"][r] == S["d0"][p] and X["d1"][r] == S["d1"][p])
        out[p] = (r, m[r], f[r], same | SEED) if r < nT else (r - nT, m[r], f[r], same)
    return out


@functools.lru_cache(maxsize=None)
def grid_tables(n, nT):
    S, T = tables(n, nT, SDT)
    S.setflags(write=False)
    T.setflags(write=False)
    return S, T


@functools.lru_cache(maxsize=2)
def _grid_matrices(n, nT):
    S, T = grid_tables(n, nT)
    return matrices(S, np.concatenate([T, S]))


@functools.lru_cache(maxsize=None)
def want(n, nT, thr, order):
    """the brute force of a grid cell, computed once and left alone"""
    S, T = grid_tables(n, nT)
    w = brute_seeded(S, cc.order_of(S, order), thr, T, DT, _grid_matrices(n, nT))
    w.setflags(write=False)
    return w


def kinds(w):
    """-> (members of seeds, new representatives, members of new representatives) of a result, as boolean arrays"""
    ids = np.arange(len(w))
    of_seed = (w["flags"] & SEED) != 0
    rep = ~of_seed & (w["id"] == ids)
    member = ~rep & (w["id"] != NO_ID)
    return member & of_seed, rep, member & ~of_seed


# drops of 64 and 65 against 700 seeds: 32 to 55 of their positions join seeds and the 9 to 33 new representatives get no member, in every
# walk order and at both thresholds.  Every other cell with n >= 64 and nT >= 64 has all three kinds
NO_NEW_MEMBERS = ((64, 700), (65, 700))


def check_cells():
    """every cell with n >= 64 and nT >= 64 at the thresholds 32 and 48 has members of seeds, new representatives and, but for the two cells
    of NO_NEW_MEMBERS, members of new representatives"""
    for n in NS:
        for nT in NTS:
            if n < 64 or nT < 64:
                continue
            for thr in (32, 48):
                for o in ORDERS:
                    a, b, c = kinds(want(n, nT, thr, o))
                    assert a.any() and b.any() and c.any() == ((n, nT) not in NO_NEW_MEMBERS), (n, nT, thr, o, int(a.sum()), int(b.sum()), int(c.sum()))


check_cells()


# ---- the concatenation property: tables and the expected records from an UNSEEDED result of [A; B]
def concat_expected(joined, nA, dtype):
    """joined: the unseeded records of [A; B] walked as (oA, nA + oB) -> (RA, the records of the seeded call (S = B, T = A[RA], order = oB)):
    a representative RA[j] inside A reads as seed j, a position nA + p as p"""
    ids = np.arange(len(joined))
    RA = ids[:nA][joined["id"][:nA] == ids[:nA]]
    out = np.zeros(len(joined) - nA, dtype)
    for p, rec in enumerate(joined[nA:]):
        r = int(rec["id"])
        if r == NO_ID:
            out[p] = (NO_ID, 0, 0, 0)
        elif r < nA:
            j = int(np.searchsorted(RA, r))
            assert RA[j] == r                         # a member of A never represents
            out[p] = (j, rec["match"], rec["filled"], int(rec["flags"]) | SEED)
        else:
            out[p] = (r - nA, rec["match"], rec["filled"], rec["flags"])
    return RA, out


def concat_orders(A, Bt):
    """the walk orders of the two sides and the joined one"""
    oA, oB = cc.order_of(A, "n_descending"), cc.order_of(Bt, "random")
    return oA, oB, np.concatenate([oA, len(A) + oB]).astype(np.uint32)


# ---- planted cases.  The drop S has 600 random records, the seed table T 700 (no two of them agree in a bucket); the planted records go
# to fixed positions.  `first` (the deciding new representative, or what stands in its place) and `second` (what it decides) are walked
#   far    first in block 0, second in block 1
#   wave   both in block 1, first in its wavefront 0, second in its wavefront 1
#   lane   both in wavefront 0 of block 1, second right behind first
PLACEMENTS = ("far", "wave", "lane")
N_DROP, N_SEEDS = 600, 700


def _walk(first, second, how):
    at = {"far": (5, B + 10), "wave": (B + 4, B + 64 + 5), "lane": (B + 4, B + 4 + len(first))}[how]
    slots = {}
    for base, group in zip(at, (first, second)):
        for k, p in enumerate(group):
            slots[base + k] = p
    fill = iter(p for p in range(N_DROP) if p not in first + second)
    order = [slots[w] if w in slots else next(fill) for w in range(N_DROP)]
    assert sorted(order) == list(range(N_DROP))
    w1, w2 = order.index(first[0]), order.index(second[0])
    assert w1 < w2 and {"far": w1 // B < w2 // B, "wave": w1 // B == w2 // B and w1 // 64 < w2 // 64, "lane": w1 // 64 == w2 // 64}[how]
    return np.array(order, np.uint32)


def _case(dtype, seed, seeds, drop, first, second, how):
    """seeds: {position in T: record}, drop: {position in S: record}"""
    S, T = cc.random_table(N_DROP, 100 + seed, dtype), cc.random_table(N_SEEDS, 200 + seed, dtype)
    for p, r in seeds.items():
        T[p] = r
    for p, r in drop.items():
        S[p] = r
    return S, T, _walk(first, second, how)


def planted(dtype):
    """-> [(name, S, T, order, thr64, {position of S: (id, the record names a seed)})], every case in the three placements"""
    rng = np.random.Generator(np.random.PCG64(6160))
    X = cc._draw(rng, 64)
    k = np.arange(64)
    rec = functools.partial(cc._rec, dtype)
    P = X
    Q = cc._other(P, k[32:])                         # agrees with P in 0..31 only: no pair from 33/64 on
    out = []
    for how in PLACEMENTS:
        case = functools.partial(_case, dtype, how=how)
        # (a) the full tie: E agrees with P in 0..47 and with Q in 0..31, 48..63, 48 of 64 each.  The seed wins, at whatever position
        E = P.copy()
        E[48:] = Q[48:]
        S, T, o = case(1, {650: rec(P, d=1)}, {3: rec(Q, d=2), 299: rec(E, d=3)}, [3], [299])
        out.append((f"tie_seed_wins_{how}", S, T, o, 48, {3: (3, False), 299: (650, True)}))
        # (b) the new representative is nearer: E agrees with P in 52 buckets (0..51), with Q in 44 (0..31, 52..63); at 40 both are candidates
        E = P.copy()
        E[52:] = Q[52:]
        S, T, o = case(2, {650: rec(Q, d=2)}, {3: rec(P, d=1), 299: rec(E, d=3)}, [3], [299])
        out.append((f"new_nearer_{how}", S, T, o, 40, {3: (3, False), 299: (3, False)}))
        # (c) the seed is nearer
        S, T, o = case(3, {650: rec(P, d=1)}, {3: rec(Q, d=2), 299: rec(E, d=3)}, [3], [299])
        out.append((f"seed_nearer_{how}", S, T, o, 40, {3: (3, False), 299: (650, True)}))
        # (d) two seeds that are a reported pair (56 of 64) both stand, in different tiles of T.  M agrees with each in 56: the smaller
        # position.  M2 agrees with V in 62 and with U in 54: it joins V, which it could not if V had been dropped for U
        U = X
        V = cc._other(U, k[56:])
        M = cc._other(U, k[44:48])
        M[60:] = V[60:]
        M2 = cc._other(V, k[:2])
        S, T, o = case(4, {3: rec(U, d=1), 300: rec(V, d=2)}, {7: rec(M2, d=4), 299: rec(M, d=3)}, [7], [299])
        out.append((f"paired_seeds_{how}", S, T, o, 48, {7: (300, True), 299: (3, True)}))
        S, T, o = case(4, {300: rec(U, d=1), 3: rec(V, d=2)}, {7: rec(M2, d=4), 299: rec(M, d=3)}, [7], [299])
        out.append((f"paired_seeds_swapped_{how}", S, T, o, 48, {7: (3, True), 299: (3, True)}))
        # (e) a seed with n = 0 and a full sketch is never joined: its copy in the drop represents itself and a second copy joins that one
        S, T, o = case(5, {650: rec(X, n=0, d=0)}, {3: rec(X, n=7, d=9), 299: rec(X, n=7, d=9)}, [3], [299])
        out.append((f"empty_seed_{how}", S, T, o, 64, {3: (3, False), 299: (3, False)}))
        # (f) a member is never a candidate: Bk joins the seed A (48 of 64); Ck agrees with Bk in 48 and with A in 32 only and represents itself
        Bk = cc._other(X, k[48:])
        Ck = cc._other(Bk, k[:16])
        S, T, o = case(6, {650: rec(X, d=1)}, {3: rec(Bk, d=2), 299: rec(Ck, d=3)}, [3], [299])
        out.append((f"member_no_candidate_{how}", S, T, o, 48, {3: (650, True), 299: (299, False)}))
        # (g) equal ratio, different filled (cluster_cases, case d): Ed with Qd 24 / 32, with Pd 30 / 40, Pd and Qd no pair.  The larger
        # filled wins on whichever side it is
        even = k[::2]
        Ed = X.copy()
        Ed[1::2] = EMPTY
        Qd = cc._other(Ed, even[24:])
        Pd = cc._other(Ed, even[:2])
        Pd[k[1:16:2]] = cc._draw(rng, 8)
        S, T, o = case(7, {650: rec(Pd, d=1)}, {3: rec(Qd, d=2), 299: rec(Ed, d=3)}, [3], [299])
        out.append((f"filled_seed_{how}", S, T, o, 48, {3: (3, False), 299: (650, True)}))
        S, T, o = case(7, {650: rec(Qd, d=2)}, {3: rec(Pd, d=1), 299: rec(Ed, d=3)}, [3], [299])
        out.append((f"filled_new_{how}", S, T, o, 48, {3: (3, False), 299: (3, False)}))
    return out


@functools.lru_cache(maxsize=None)
def planted_want():
    """the planted cases with their brute force, computed once and left alone: [(name, S, T, order, thr64, expectation, records)]"""
    out = []
    for name, S, T, o, thr, expect in planted(SDT):
        w = brute_seeded(S, o, thr, T, DT)
        for x in (S, T, o, w):
            x.setflags(write=False)
        out.append((name, S, T, o, thr, expect, w))
    return out


def named(w, expect):
    """what a result says about the positions of an expectation, in its form"""
    return {p: (int(w["id"][p]), bool(w["flags"][p] & SEED)) for p in expect}
