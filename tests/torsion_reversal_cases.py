"""Inputs of the torsion reversal tests (test_torsion_reversal_host.py, test_gpu_torsion_reversal.py): residue pairs on which the reference
evaluates ONE dihedral to two different bins, depending on the direction it is read in.  Only the CPU oracle is used.

For an unordered pair (i, j) the descriptor holds four torsion fields that are two dihedrals read in both directions:
    dihedral 0:  tor1(i,j) = torsion(N_i, CA_i, CB_i, CB_j)   and   tor2(j,i) = torsion(CB_j, CB_i, CA_i, N_i)
    dihedral 1:  tor1(j,i) = torsion(N_j, CA_j, CB_j, CB_i)   and   tor2(i,j) = torsion(CB_i, CB_j, CA_j, N_j)
The atan2f x-operands of the two readings are bit-identical, the y-operands differ by a few eps (fd_geom.h), so next to a bin threshold the two
fields can DISAGREE.  The speculative path of the index build decides each dihedral once and copies the key: it must refuse every such pair.

Construction: a torsion edge of one of the four fields is found like in tests/quantiser_edges.py (one coordinate bisected until two adjacent
floats give different keys of THAT field; the moved coordinate is one the field's dihedral depends on), then the rungs 1, 2, 4 ... 64 ulps
beyond either side are added.  Of these 16 arrangements the ones whose two readings of a dihedral differ under the oracle are kept, plus the
same number of arrangements on which both dihedrals agree: the outermost such rungs of the same ladder (of the next ones where it has too few).  Rounds of 64 edges (one per cell of quantiser_edges.CELLS, so
that the per-pair and the packed layout hold the same coordinates) are added until each dihedral has MIN_DISAGREE disagreeing pairs, at
least MIN_PER_QUADRANT of them in every sign quadrant of the forward reading's atan2f operands.

Deterministic (PCG64, fixed seed), bounded (RuntimeError when the try budget ends first), nothing is written to disk."""
import numpy as np

from tests import quantiser_edges as qe

RUNGS = tuple(1 << k for k in range(7))          # 1 .. 64 ulps
MIN_DISAGREE = 256
MIN_PER_QUADRANT = 16
# (forward field, reversed field) of the two dihedrals as indices into the keys (tor1_ij, tor2_ij, tor1_ji, tor2_ji) = qe.TOR_FIELDS
DIHEDRAL_FIELDS = ((0, 3), (2, 1))
# the coordinates a dihedral depends on, as (residue, atom): dihedral 0 = (N_0, CA_0, CB_0, CB_1), dihedral 1 = (N_1, CA_1, CB_1, CB_0)
_MOVABLE = (((0, 0), (0, 1), (0, 2), (1, 2)), ((1, 0), (1, 1), (1, 2), (0, 2)))


def tor_keys(h):
    """(tor1_ij, tor2_ij, tor1_ji, tor2_ji) keys of the hash list of a two-residue structure, or None when the pair is not hashed"""
    if len(h) != 2:
        return None
    return ((h[0] >> 4) & 15, h[0] & 15, (h[1] >> 4) & 15, h[1] & 15)


def disagreement(h):
    """(dihedral 0 disagrees, dihedral 1 disagrees) under the oracle's hashes (h_ij, h_ji)"""
    k = tor_keys(h)
    return tuple(k[f] != k[r] for f, r in DIHEDRAL_FIELDS)


class ReversalSet:
    """X [n, 2, 3, 3] f32, aa [n, 2], cell [n], H [n, 2] the oracle's (h_ij, h_ji), disagree [n, 2] bool (per dihedral), quadrant [n, 2]: the sign
    quadrant (y < 0) | (x < 0) << 1 of the forward reading of each dihedral, step [n]: the rung (0: a side of the edge; negative: A side)"""

    def __init__(self, X, aa, cell, H, disagree, quadrant, step, tries, edges):
        self.X, self.aa, self.cell, self.H, self.disagree, self.quadrant, self.step = X, aa, cell, H, disagree, quadrant, step
        self.tries, self.edges = tries, edges

    def __len__(self):
        return len(self.X)

    def tobytes(self):
        return b"".join(a.tobytes() for a in (self.X, self.aa, self.cell, self.H, self.disagree, self.quadrant, self.step))

    def counts(self):
        """[dihedral][quadrant] -> disagreeing pairs"""
        return [[int(np.sum(self.disagree[:, d] & (self.quadrant[:, d] == m))) for m in range(4)] for d in range(2)]

    def per_pair(self):
        return qe.layout_per_pair(self.X, self.aa)

    def packed(self):
        return qe.layout_packed(self.X, self.aa, self.cell)


def generate(seed=20250, max_tries=400000, min_disagree=MIN_DISAGREE, min_per_quadrant=MIN_PER_QUADRANT):
    cfg = qe.DEFAULT
    rng = np.random.Generator(np.random.PCG64(seed))
    probe = qe._Probe(2)
    X_out, aa_out, cell_out, H_out, dis_out, step_out = [], [], [], [], [], []
    counts = np.zeros((2, 4), np.int64)
    tries = edges = slot = debt = 0

    def lacking():
        return [(d, m) for d in range(2) for m in range(4) if counts[d, m] < min_per_quadrant] + [(d, None) for d in range(2) if counts[d].sum() < min_disagree]

    while lacking() or debt:
        for _ in range(64):
            cell = slot % 64
            lack = lacking()
            dih = lack[0][0] if lack else slot % 2                    # steer to the dihedral that still lacks pairs; its two fields in turn
            field = DIHEDRAL_FIELDS[dih][(slot // 2) % 2]
            while True:
                if tries >= max_tries:
                    raise RuntimeError(f"torsion_reversal_cases: try budget ended, disagreeing pairs per [dihedral][quadrant] = {counts.tolist()}")
                tries += 1
                d = qe._draw(rng, cfg, cell, "any", float(rng.uniform(2.2, 19.5)))
                if d is None:
                    continue
                X, aa, _, delta = d
                res, atom = _MOVABLE[dih][int(rng.integers(4))]
                idx = (res, atom, int(rng.integers(3)))
                r = qe._find_edge(probe, cfg, X, aa, idx, delta, lambda h: None if tor_keys(h) is None else tor_keys(h)[field])
                if r is None or len(r[2]) != 2 or len(r[3]) != 2:
                    continue
                break
            a, b, _, _ = r
            ia, ib = qe.f2i(a), qe.f2i(b)
            sgn = 1 if ib > ia else -1
            rungs = [(ia, 0, -1), (ib, 0, 1)] + [(ia - sgn * s, s, -1) for s in RUNGS] + [(ib + sgn * s, s, 1) for s in RUNGS]
            ladder = []
            for iv, s, side in rungs:
                probe.poke(idx, qe.i2f(iv))
                h = probe.hashes(cfg)
                if len(h) == 2:
                    ladder.append((iv, h, disagreement(h), s, side))
            bad = [t for t in ladder if t[2][0] or t[2][1]]
            # the outermost agreeing rungs: some of them lie beyond the speculation's margin and are ACCEPTED decisions next to a threshold;
            # a ladder with more disagreeing than agreeing rungs leaves a debt that the next ladders pay
            good = sorted((t for t in ladder if not (t[2][0] or t[2][1])), key=lambda t: (-t[3], t[4]))
            good = good[: len(bad) + debt]
            debt += len(bad) - len(good)
            keep = bad + good
            for iv, h, dis, s, side in keep:
                x = X.copy()
                x[idx] = qe.i2f(iv)
                X_out.append(x); aa_out.append(aa); cell_out.append(cell); H_out.append(h); dis_out.append(dis); step_out.append(side * s)
            if bad:
                q = qe._quadrants(np.asarray([X_out[k] for k in range(len(X_out) - len(keep), len(X_out) - len(keep) + len(bad))], np.float32))
                for k, t in enumerate(bad):
                    for dd in range(2):
                        if t[2][dd]:
                            counts[dd, q[k, DIHEDRAL_FIELDS[dd][0]]] += 1
            edges += 1
            slot += 1
    X = np.asarray(X_out, np.float32).reshape(-1, 2, 3, 3)
    quad = qe._quadrants(X)[:, [DIHEDRAL_FIELDS[0][0], DIHEDRAL_FIELDS[1][0]]]
    return ReversalSet(X, np.asarray(aa_out, np.uint8).reshape(-1, 2), np.asarray(cell_out, np.int64), np.asarray(H_out, np.uint32).reshape(-1, 2),
                       np.asarray(dis_out, bool).reshape(-1, 2), quad, np.asarray(step_out, np.int64), tries, edges)


_SET = None


def reversal_set():
    """the set of the tests, generated once per process"""
    global _SET
    if _SET is None:
        _SET = generate()
    return _SET
