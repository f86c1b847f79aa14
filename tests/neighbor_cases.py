"""What the signature neighbours tests (device and host) share: the sizes, k, thresholds and splits they walk, the hand-made tables of
tests/signature_cases.py, and a numpy brute force over whole tables that states the definition of include/fdgpu.h once more, independent of
any build: d is a candidate of q iff the pair would be reported at thr64 and d is not excluded; candidates are ordered by descending
match / filled, then descending filled, then ascending id."""
import numpy as np

from tests import signature_cases as sc

SIZES = (1, 63, 64, 65, 129, 257, 600)      # the tile edges; one, two and three workgroups of queries with a partial last one
KS = (1, 4, 32)
THRESHOLDS = (1, 32, 64)
SPLITS = (1, 2, 3, 7, 1000)                  # the last one is clamped
NO_ID = 0xffffffff


def table(n: int, dtype):
    return sc.pair_table(n, 100 + n, dtype)


def other(A):
    return sc.other_table(A, 7)


def brute_neighbors(Q, D, k: int, thr64: int, exclude, nb_dtype):
    """the (len(Q), k) records by the definition, over whole tables at once; D = None: inside Q, nobody its own neighbour"""
    self_mode = D is None
    if self_mode:
        D = Q
    eq = (Q["sk"][:, None, :] == D["sk"][None, :, :]).sum(-1)
    E = ((Q["sk"] == sc.EMPTY)[:, None, :] & (D["sk"] == sc.EMPTY)[None, :, :]).sum(-1)
    match, filled = eq - E, 64 - E
    ok = (Q["n"] > 0)[:, None] & (D["n"] > 0)[None, :] & (filled > 0) & (match * 64 >= thr64 * filled)
    if self_mode:
        ok &= np.arange(len(Q))[:, None] != np.arange(len(D))[None, :]
    elif exclude is not None:
        ok &= np.asarray(exclude, np.int64)[:, None] != np.arange(len(D))[None, :]
    key = (match.astype(np.int64) << 20) // np.maximum(filled, 1)      # distinct fractions over <= 64 stay distinct, equal ones equal
    same = (Q["n"][:, None] == D["n"][None, :]) & (Q["d0"][:, None] == D["d0"][None, :]) & (Q["d1"][:, None] == D["d1"][None, :])
    out = np.zeros((len(Q), k), nb_dtype)
    out["id"] = NO_ID
    for q in range(len(Q)):
        c = np.nonzero(ok[q])[0]
        c = c[np.lexsort((c, -filled[q, c], -key[q, c]))][:k]         # last key first: ratio, then filled, then id
        out["id"][q, :len(c)], out["match"][q, :len(c)], out["filled"][q, :len(c)], out["flags"][q, :len(c)] = c, match[q, c], filled[q, c], same[q, c]
    return out


def nearer(x, y) -> bool:
    """the order itself, by cross-multiplication with Python integers: is record x nearer than record y?"""
    mx, fx, ix, my, fy, iy = int(x["match"]), int(x["filled"]), int(x["id"]), int(y["match"]), int(y["filled"]), int(y["id"])
    if mx * fy != my * fx:
        return mx * fy > my * fx
    return fx > fy if fx != fy else ix < iy
