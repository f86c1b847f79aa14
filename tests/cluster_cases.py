"""Shared cases of the signature clusters tests (host and device): the tables, thresholds and walk orders of the grid, two extreme tables, the
planted cases, and an independent brute force: a Python loop over the eq / E matrices of a whole table, as signature_cases.brute_pairs
computes them.  No product code is used here.

The device walks in blocks of B = 256 positions and stages representatives in tiles of 64: the sizes straddle both edges."""
import numpy as np

from tests import signature_cases as sc

B = 256                                              # the device's block of the walk (SG_BLOCK_B)
SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 700)
HOST_B = 1024                                        # the host form's block of the walk: it scans the representatives of earlier blocks with its threads
HOST_SIZES = (HOST_B - 1, HOST_B, HOST_B + 1, 2 * HOST_B + 1)
HOST_THREAD_WORK = 65536                             # compares a host thread is started for
THRESHOLDS = (1, 32, 48, 64)
SPLITS = (1, 2, 3, 7, 1000)
SPLIT_SIZES = (257, 700)
NO_ID = 0xffffffff
EMPTY = sc.EMPTY
ORDERS = ("identity", "reverse", "n_descending", "random")


def table(n, dtype):
    return sc.pair_table(n, 4100 + n, dtype)


def order_of(S, name):
    n = len(S)
    if name == "identity":
        return np.arange(n, dtype=np.uint32)
    if name == "reverse":
        return np.arange(n, dtype=np.uint32)[::-1].copy()
    if name == "n_descending":                       # ties by ascending position
        return np.lexsort((np.arange(n), -S["n"].astype(np.int64))).astype(np.uint32)
    return np.random.Generator(np.random.PCG64(977 + n)).permutation(n).astype(np.uint32)


def matrices(S):
    """eq, E -> match, filled of every pair of the table"""
    eq = (S["sk"][:, None, :] == S["sk"][None, :, :]).sum(-1)
    E = ((S["sk"] == EMPTY)[:, None, :] & (S["sk"] == EMPTY)[None, :, :]).sum(-1)
    return eq - E, 64 - E


def nearer(mx, fx, ix, my, fy, iy):
    """the total order, with Python integers: the larger match / filled, then the larger filled, then the smaller position"""
    l, r = int(mx) * int(fy), int(my) * int(fx)
    return l > r if l != r else int(fx) > int(fy) if fx != fy else int(ix) < int(iy)


def brute_clusters(S, order, thr64, dtype):
    """the definition, one position after the other"""
    n = len(S)
    order = np.arange(n) if order is None else np.asarray(order)
    match, filled = matrices(S)
    out = np.zeros(n, dtype)
    out["id"] = NO_ID
    reps = []
    for p in order.tolist():
        if S["n"][p] == 0:
            continue
        best = None
        for r in reps:
            m, f = int(match[p, r]), int(filled[p, r])
            if f > 0 and m * 64 >= thr64 * f and (best is None or nearer(m, f, r, *best)):
                best = (m, f, r)
        if best is None:
            k = int((S["sk"][p] != EMPTY).sum())
            out[p] = (p, k, k, 1)
            reps.append(p)
        else:
            m, f, r = best
            out[p] = (r, m, f, int(S["n"][r] == S["n"][p] and S["d0"][r] == S["d0"][p] and S["d1"][r] == S["d1"][p]))
    return out


def _draw(rng, k):
    return rng.integers(0, EMPTY, size=k, dtype=np.uint64).astype(np.uint32)      # never 0xffffffff


def random_table(n, seed, dtype):
    """n records with random sketches: no two agree in a bucket"""
    rng = np.random.Generator(np.random.PCG64(seed))
    t = np.zeros(n, dtype)
    t["n"] = rng.integers(1, 5000, size=n)
    t["d0"] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    t["d1"] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    t["sk"] = _draw(rng, n * 64).reshape(n, 64)
    return t


def all_random(dtype, n=700):
    """700 representatives at every threshold: the table of representatives passes 64 and 256 entries and several splits"""
    return random_table(n, 31337, dtype)


def all_copies(dtype, n=700):
    """700 copies of one record: one cluster"""
    return np.repeat(random_table(1, 4242, dtype), n)


def _other(x, idx):
    """x with the buckets idx set to other values (never 0xffffffff, never x's)"""
    y = x.copy()
    y[idx] = (x[idx] + np.uint32(1)) % np.uint32(EMPTY)
    return y


N_PLANTED = 600


def _place(dtype, seed, records, positions, walk, n_first, far):
    """a table of N_PLANTED random records with `records` at the table positions `positions`, and its walk: the planted records in the order
    `walk` (indices into records).  far: the first n_first of them, then 256 unrelated records, then the others (the deciding representatives
    are in an earlier block than what they decide); else all of them side by side from place 260 on (inside one block)"""
    S = random_table(N_PLANTED, seed, dtype)
    for r, p in zip(records, positions):
        S[p] = r
    fill = [p for p in range(N_PLANTED) if p not in positions]
    planted = [positions[k] for k in walk]
    if far:
        order = planted[:n_first] + fill[:B] + planted[n_first:] + fill[B:]
        assert all(order.index(p) < B for p in planted[:n_first]) and all(order.index(p) >= B for p in planted[n_first:])
    else:
        order = fill[:B + 4] + planted + fill[B + 4:]
        assert len({order.index(p) // B for p in planted}) == 1
    return S, np.array(order, np.uint32)


def _rec(dtype, sk, n=100, d=1):
    r = np.zeros(1, dtype)
    r["n"], r["d0"], r["d1"], r["sk"] = n, d, d, sk
    return r[0]


def planted(dtype):
    """-> [(name, S, order, thr64, {position: representative's position, or NO_ID for unclustered})], every case in both placements"""
    rng = np.random.Generator(np.random.PCG64(5150))
    X = _draw(rng, 64)
    k = np.arange(64)
    out = []
    for far in (True, False):
        tag = "far" if far else "near"
        # (a) the chain at 48: B agrees with A in 0..47, C with B in 16..63 and so with A in 16..47 only
        A = X
        Bk = _other(A, k[48:])
        Ck = _other(Bk, k[:16])
        recs, pos = [_rec(dtype, A, d=1), _rec(dtype, Bk, d=2), _rec(dtype, Ck, d=3)], [400, 17, 300]
        S, o = _place(dtype, 1, recs, pos, [0, 1, 2], 1, far)
        out.append((f"chain_ABC_{tag}", S, o, 48, {400: 400, 17: 400, 300: 300}))
        S, o = _place(dtype, 1, recs, pos, [1, 0, 2], 1, far)
        out.append((f"chain_BAC_{tag}", S, o, 48, {17: 17, 400: 17, 300: 17}))
        # (b) nearest beats first, at 40: Q agrees with P in 0..31 only; E agrees with P in 52 buckets (0..51), with Q in 44 (0..31, 52..63)
        P = X
        Q = _other(P, k[32:])
        E = P.copy()
        E[52:] = Q[52:]
        for pp, pq in ((50, 450), (450, 50)):        # P at the smaller and at the larger position
            for walk in ([0, 1, 2], [1, 0, 2]):      # P walked first, Q walked first
                S, o = _place(dtype, 2, [_rec(dtype, P, d=1), _rec(dtype, Q, d=2), _rec(dtype, E, d=3)], [pp, pq, 299], walk, 2, far)
                out.append((f"nearest_P{pp}_walk{walk[0]}_{tag}", S, o, 40, {pp: pp, pq: pq, 299: pp}))
        # (c) the full tie: E agrees with P in 0..47 and with Q in 0..31, 48..63: 48 of 64 each; the smaller position wins
        E = P.copy()
        E[48:] = Q[48:]
        for pp, pq in ((50, 450), (450, 50)):
            for walk in ([0, 1, 2], [1, 0, 2]):
                S, o = _place(dtype, 3, [_rec(dtype, P, d=1), _rec(dtype, Q, d=2), _rec(dtype, E, d=3)], [pp, pq, 299], walk, 2, far)
                out.append((f"tie_P{pp}_walk{walk[0]}_{tag}", S, o, 48, {pp: pp, pq: pq, 299: min(pp, pq)}))
        # (d) equal ratio, different filled.  E fills the 32 even buckets.  Q fills the same ones and agrees in the first 24 of them: 24 / 32.
        # P fills them and 8 odd ones and agrees in the last 30 of the 32: 30 / 40 (P and Q agree in 22 of 40: no pair).  The larger filled wins.
        even = k[::2]
        Ed = X.copy()
        Ed[1::2] = EMPTY
        Qd = _other(Ed, even[24:])
        Pd = _other(Ed, even[:2])
        Pd[k[1:16:2]] = _draw(rng, 8)
        for pp, pq in ((50, 450), (450, 50)):
            for walk in ([0, 1, 2], [1, 0, 2]):
                S, o = _place(dtype, 4, [_rec(dtype, Pd, d=1), _rec(dtype, Qd, d=2), _rec(dtype, Ed, d=3)], [pp, pq, 299], walk, 2, far)
                out.append((f"filled_P{pp}_walk{walk[0]}_{tag}", S, o, 48, {pp: pp, pq: pq, 299: pp}))
    # (e) empty signatures at the first and the last place of a block; one of them has n = 0 and a full sketch, which a later copy does not join
    full = _rec(dtype, X, n=0, d=0)
    void = _rec(dtype, np.full(64, EMPTY, np.uint32), n=0, d=0)
    twin = _rec(dtype, X, n=7, d=9)
    pos = [5, 100, 200, 333, 444, 555]               # full, void, void, void, twin, twin
    S = random_table(N_PLANTED, 5, dtype)
    for r, p in zip([full, void, void, void, twin, twin], pos):
        S[p] = r
    fill = [p for p in range(N_PLANTED) if p not in pos]
    order = [5] + fill[:B - 2] + [100, 200] + fill[B - 2:2 * B - 4] + [333, 444] + fill[2 * B - 4:] + [555]
    assert [order.index(p) for p in (5, 100, 200, 333)] == [0, B - 1, B, 2 * B - 1] and sorted(order) == list(range(N_PLANTED))
    out.append(("empties", S, np.array(order, np.uint32), 1, {5: NO_ID, 100: NO_ID, 200: NO_ID, 333: NO_ID, 444: 444, 555: 444}))
    return out
