"""Inputs of the quantiser edge tests (test_quantiser_edges_host.py, test_gpu_quantiser_edges.py): residue pairs placed ON the thresholds of
the hash's quantisers.  Only the CPU oracle is used.

An EDGE is a pair of structures that differ in one ulp of one coordinate and that oracle.hash_structure hashes differently: a residue-pair
arrangement (N, CA, CB per residue, hashable residue types) is drawn, one coordinate of its second residue is moved until the hash list
changes, and the two values are bisected over the f32 bit patterns until they are adjacent floats.  A CUTOFF edge is the same with the LENGTH
of the hash list as the criterion (the accept test).  A LADDER adds, for an edge, the structures 1, 2, 4, ..., 2^12 ulps further out on either
side.

Every pair is bisected at its final position: pair k of a packed structure sits in cell k of a fixed lattice (CELLS; cell 0 is the origin, the
others reach +-500 A, the nearest two are 72 A apart = more than twice the largest cutoff plus the extent of a pair), so the per-pair layout
(one structure per pair) and the packed layout (64 pairs = 128 residues per structure) hold the same coordinates bit for bit.

Everything is deterministic (PCG64 with fixed seeds), bounded (a try budget; RuntimeError when it ends before the coverage condition holds) and
nothing is written to disk."""
import ctypes as C
import os
import re
import struct
from collections import Counter
from dataclasses import dataclass

import numpy as np

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_AXIS = (0.0, 72.0, -200.0, 470.0)
CELLS = np.array([[x, y, z] for x in _AXIS for y in _AXIS for z in _AXIS], np.float64)      # cell 0 = the origin
BOND_MIN, BOND_MAX = 1.2, 2.6          # |CB - CA| of a drawn residue: CB distances reach cutoff + 2 * BOND_MAX
MIN_PER_CLASS = 16
CUTOFFS = (6.0, 12.5, 20.0, 25.0)
LADDER_STEPS = tuple(1 << k for k in range(13))


@dataclass(frozen=True)
class Cfg:
    name: str
    hash_type: int = 3
    nd: int = 0
    na: int = 0
    cutoff: float = 20.0
    nres: int = 2                      # 4: the pair sits between two flanking residues (TertiaryInteraction, Hybrid need i-1 / i+1)

    @property
    def pair(self):
        return (0, 1) if self.nres == 2 else (1, 2)


DEFAULT = Cfg("default")
# fields of the other configurations: name -> mask over the hash (geometry/*.rs layouts as oracle/fdo_geometry.c restates them)
_PDBTR_FIELDS = {"ca": 0xf << 16, "cb": 0xf << 12, "theta": 0xf << 8, "tor1": 0xf << 4, "tor2": 0xf}
OTHER = [
    (Cfg("pdbtr_8_4", 3, 8, 4), _PDBTR_FIELDS),
    (Cfg("pdbtr_12_4", 3, 12, 4), _PDBTR_FIELDS),
    (Cfg("pdbmotif", 0), {"ca": 0x1f << 10, "cb": 0x1f << 5, "theta": 0x1f}),
    (Cfg("pdbmotif_sincos", 1), {"ca": 0xf << 12, "cb": 0xf << 8, "sin": 0xf << 4, "cos": 0xf}),
    (Cfg("folddisco_angle", 7), {"ca": 7 << 18, "cb": 7 << 15, "theta": 0x1f << 10, "tor1": 0x1f << 5, "tor2": 0x1f}),
    (Cfg("folddisco_dist", 8), {"ca": 0x1f << 16, "cb": 0x1f << 11, "theta": 7 << 8, "tor1": 0xf << 4, "tor2": 0xf}),
    (Cfg("trrosetta", 2), dict([("cb", 7 << 20)] + [("ang%d" % k, 0xf << (16 - 4 * k)) for k in range(5)])),
    (Cfg("ppf", 4), dict([("dist", 0xf << 18)] + [("ang%d" % k, 0x3f << (12 - 6 * k)) for k in range(3)])),
    (Cfg("tertiary", 5, nres=4), dict([("ca", 0xf << 4)] + [("cos%d" % k, 7 << (26 - 3 * k)) for k in range(7)])),
    (Cfg("hybrid", 6, nres=4), dict([("ca", 0xf << 24), ("cb", 0xf << 20)] + [("ang%d" % k, 0xf << (16 - 4 * k)) for k in range(5)])),
]
# one encoding per branch of fd_accept_other (CB distance; |(cb2 - ca1) - (cb1 - ca1)|; CA distance of interior residues, with and without
# the CB test) next to the default encoding's CA distance
CUTOFF_ENCODINGS = [(3, 2), (2, 2), (4, 2), (5, 4), (6, 4)]       # (hash type, residues per arrangement)


# ---- tables of the device headers (the class list is pinned against them) ----------------------------------------------------------------
def header_tables():
    bt = open(os.path.join(ROOT, "folddisco_amd", "csrc", "fd_bin_tables.h")).read()
    dt = open(os.path.join(ROOT, "folddisco_amd", "csrc", "fd_dist_table.h")).read()

    def nums(txt, name, base):
        body = re.search(name + r"\[[^=]*=\s*\{(.*?)\};", txt, re.S).group(1)
        return [int(x.rstrip("u"), base) for x in re.findall(r"0x[0-9a-fA-F]+u?|\d+", body)]
    tor_thr = np.array(nums(bt, "fd_tor_thr_bits", 16), np.uint32).reshape(4, 5)
    tor_key = np.array(nums(bt, "fd_tor_key", 10), np.uint8).reshape(4, 5)
    return dict(theta_thr=np.array(nums(bt, "fd_theta_thr_bits", 16), np.uint32), theta_key=nums(bt, "fd_theta_key", 10),
                tor_nseg=nums(bt, "fd_tor_nseg", 10), tor_thr=tor_thr, tor_key=tor_key, dist_thr=np.array(nums(dt, "fd_dist_thr_bits", 16), np.uint32))


TOR_FIELDS = ("tor1_ij", "tor2_ij", "tor1_ji", "tor2_ji")


def reachable_classes(cutoff=20.0):
    """the classes of the default encoding that a drawn arrangement can reach, from the tables of fd_bin_tables.h / fd_dist_table.h:
    ("ca", k-1, k) for every distance breakpoint at or below the cutoff, ("cb", k-1, k) up to cutoff + 2 BOND_MAX, ("theta", key, key') for the
    six breakpoints of fd_theta_thr_bits and (field, m, key, key') for every segment boundary of fd_tor_thr_bits of quadrant m.  A torsion edge
    counts for quadrant m's boundary when its two sides hold the boundary's two keys and at least one side lies in quadrant m (the boundaries
    at |y/x| ~ 3e-8 and 2^25 coincide with a sign change of y or x: there the other side lies in the neighbouring quadrant)."""
    t = header_tables()
    d = np.sqrt(t["dist_thr"].view(np.float32).astype(np.float64))
    out = [("ca", k - 1, k) for k in range(1, len(d)) if d[k] <= cutoff]
    out += [("cb", k - 1, k) for k in range(1, len(d)) if d[k] <= cutoff + 2 * BOND_MAX - 0.5]
    out += [("theta", t["theta_key"][k - 1], t["theta_key"][k]) for k in range(1, len(t["theta_key"]))]
    for f in TOR_FIELDS:
        for m in range(4):
            for k in range(1, t["tor_nseg"][m]):
                out.append((f, m, int(t["tor_key"][m][k - 1]), int(t["tor_key"][m][k])))
    return out


# ---- f32 bit patterns in value order -------------------------------------------------------------------------------------------------------
def f2i(v):
    i = struct.unpack("<i", struct.pack("<f", v))[0]
    return i if i >= 0 else -(i & 0x7fffffff)


def i2f(i):
    return struct.unpack("<f", struct.pack("<I", i if i >= 0 else (0x80000000 | -i)))[0]


class _Probe:
    """one oracle structure whose coordinates are rewritten in place (a hash costs one library call)"""

    def __init__(self, nres):
        z = np.zeros((nres, 3), np.float32)
        self.s = oracle.structure_from_packed(z, z, z, np.zeros(nres, np.uint8))
        c = self.s.ptr.contents
        self.v = [np.ctypeslib.as_array(p, shape=(nres * 3,)).reshape(nres, 3) for p in (c.n_xyz, c.ca_xyz, c.cb_xyz)]
        self.aa = np.ctypeslib.as_array(c.aa, shape=(nres,))
        self.L = oracle.lib()
        self.out, self.cnt, self.feat = oracle.u32p(), C.c_uint64(), (C.c_float * 9)()

    def load(self, X, aa):
        for a in range(3):
            self.v[a][:] = X[:, a, :]
        self.aa[:] = aa

    def poke(self, idx, val):
        self.v[idx[1]][idx[0], idx[2]] = val

    def hashes(self, cfg):
        self.L.fdo_hash_structure(self.s.ptr, cfg.nd, cfg.na, cfg.cutoff, C.byref(self.out), C.byref(self.cnt))
        t = tuple(self.out[: self.cnt.value])
        self.L.fdo_free(self.out)
        return t

    def dist_bins(self, cfg):
        i, j = cfg.pair
        if not self.L.fdo_pair_feature(self.s.ptr, i, j, cfg.cutoff, self.feat):
            return (-1, -1)
        return (int(self.L.fdo_discretize(self.feat[2], 2.0, 20.0, 16.0)), int(self.L.fdo_discretize(self.feat[3], 2.0, 20.0, 16.0)))


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _perp(rng, u):
    w = _unit(rng)
    w = w - (w @ u) * u
    return w / np.linalg.norm(w)


def _draw(rng, cfg, cell, kind, target):
    """-> (X[nres, 3 atoms (N, CA, CB), 3] f32, aa[nres], idx = (residue, atom, axis) of the coordinate to move, delta) or None"""
    c = CELLS[cell] + rng.uniform(-2.0, 2.0, 3)
    e = _unit(rng)
    bond = rng.uniform(BOND_MIN, BOND_MAX, 2)
    u = [_unit(rng), _unit(rng)]
    atom, axis = int(rng.integers(3)), int(rng.integers(3))
    delta = float(rng.uniform(0.02, 1.5)) * (1 if rng.integers(2) else -1)
    if kind == "cb":
        if target > cfg.cutoff - 2.0:         # CB distances beyond the CA cutoff: side chains point outwards
            u = [-e + 0.35 * rng.normal(size=3), e + 0.35 * rng.normal(size=3)]
            u = [x / np.linalg.norm(x) for x in u]
            bond = rng.uniform(min(max(BOND_MIN, (target - cfg.cutoff) / 2 + 0.4), BOND_MAX), BOND_MAX, 2)
        cb = [c - e * target / 2, c + e * target / 2]
        ca = [cb[k] - bond[k] * u[k] for k in range(2)]
        if np.linalg.norm(ca[0] - ca[1]) > cfg.cutoff - 0.05:
            return None
        atom, axis = 2, int(np.argmax(np.abs(e)))
    elif kind == "anti":                      # CA->CB vectors exactly antiparallel along an axis: cos(theta) = -1, the first theta breakpoint
        ax = int(rng.integers(3))
        u[0] = np.eye(3)[ax] * (1 if rng.integers(2) else -1)
        u[1] = -u[0]
        ca = [c - e * target / 2, c + e * target / 2]
        ca = [np.float32(x).astype(np.float64) for x in ca]
        cb = [ca[k] + bond[k] * u[k] for k in range(2)]
        atom, axis, delta = 2, (ax + 1 + int(rng.integers(2))) % 3, float(rng.uniform(0.01, 0.2))
    else:
        ca = [c - e * target / 2, c + e * target / 2]
        cb = [ca[k] + bond[k] * u[k] for k in range(2)]
        if kind == "ca":
            atom, axis = 1, int(np.argmax(np.abs(e)))
    n = [ca[k] + 1.46 * (-0.33 * u[k] + 0.94 * _perp(rng, u[k])) for k in range(2)]
    res = [np.stack([n[k], ca[k], cb[k]]) for k in range(2)]
    if cfg.nres == 4:                         # flanking residues one virtual bond away from their neighbours
        fl = []
        for k in range(2):
            fca = ca[k] + 3.8 * _unit(rng)
            fu = _unit(rng)
            fl.append(np.stack([fca + 1.46 * _perp(rng, fu), fca, fca + 1.53 * fu]))
        res = [fl[0], res[0], res[1], fl[1]]
    X = np.stack(res).astype(np.float32)
    aa = rng.integers(0, 20, cfg.nres).astype(np.uint8)
    return X, aa, (cfg.pair[1], atom, axis), delta


def _find_edge(probe, cfg, X, aa, idx, delta, key):
    """-> (value a, value b, hashes at a, hashes at b) with a, b adjacent floats and key(h_a) != key(h_b), or None"""
    probe.load(X, aa)
    a = float(X[idx])
    b = float(np.float32(a + delta))
    ha = probe.hashes(cfg)
    probe.poke(idx, b)
    hb = probe.hashes(cfg)
    if key(ha) == key(hb):
        return None
    ia, ib = f2i(a), f2i(b)
    while abs(ib - ia) > 1:
        im = (ia + ib) // 2
        probe.poke(idx, i2f(im))
        hm = probe.hashes(cfg)
        if key(hm) == key(ha):
            ia, ha = im, hm
        else:
            ib, hb = im, hm
    return i2f(ia), i2f(ib), ha, hb


def far_pairs(n, d_lo, d_hi, seed):
    """n arrangements of the default encoding (no edge search) whose CA distance is drawn from [d_lo, d_hi] A, at cells drawn from the lattice
    -> (X [n, 2, 3, 3], aa [n, 2], d_CA [n] in f64)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    X, aa = [], []
    for _ in range(n):
        x, a, _, _ = _draw(rng, DEFAULT, int(rng.integers(64)), "any", float(rng.uniform(d_lo, d_hi)))
        X.append(x); aa.append(a)
    X = np.asarray(X, np.float32)
    return X, np.asarray(aa, np.uint8), np.linalg.norm(X[:, 0, 1].astype(np.float64) - X[:, 1, 1], axis=1)


class EdgeSet:
    """XA / XB [E, nres, 3, 3] f32: the two sides (they differ in coordinate idx[e] by one ulp); aa [E, nres]; cell [E]; HA / HB: the oracle's
    hash lists of the two sides; classes: per edge the list of classes it counts for"""

    def __init__(self, cfg):
        self.cfg, self.XA, self.XB, self.aa, self.cell, self.idx, self.HA, self.HB, self.classes = cfg, [], [], [], [], [], [], [], []
        self.tries = 0

    def add(self, X, aa, cell, idx, a, b, ha, hb):
        xa, xb = X.copy(), X.copy()
        xa[idx], xb[idx] = a, b
        self.XA.append(xa); self.XB.append(xb); self.aa.append(aa); self.cell.append(cell); self.idx.append(idx); self.HA.append(ha); self.HB.append(hb)

    def freeze(self):
        n = self.cfg.nres
        self.XA = np.asarray(self.XA, np.float32).reshape(-1, n, 3, 3)
        self.XB = np.asarray(self.XB, np.float32).reshape(-1, n, 3, 3)
        self.aa = np.asarray(self.aa, np.uint8).reshape(-1, n)
        self.cell = np.asarray(self.cell, np.int64)
        self.idx = np.asarray(self.idx, np.int64).reshape(-1, 3)
        return self

    def __len__(self):
        return len(self.XA)

    def tobytes(self):
        return self.XA.tobytes() + self.XB.tobytes() + self.aa.tobytes() + self.cell.tobytes() + self.idx.tobytes()

    def class_counts(self):
        return Counter(c for cl in self.classes for c in cl)

    def sides(self):
        """both sides as one array of arrangements [2E, nres, 3, 3] (A sides first), aa [2E, nres], cell [2E]"""
        return np.concatenate([self.XA, self.XB]), np.concatenate([self.aa, self.aa]), np.concatenate([self.cell, self.cell])


# ---- classification of the default encoding's edges ---------------------------------------------------------------------------------------
def _torsion_yx(a, b, c, d):
    """the atan2f operands of calc_torsion_radian (coordinate.rs:204-215) in f32, vectorised: only their SIGNS are used (the quadrant)"""
    def sub(p, q):
        return p - q

    def cross(p, q):
        return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)

    def dot(p, q):
        return p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1] + p[:, 2] * q[:, 2]

    def normalize(p):
        return p / np.sqrt(dot(p, p))[:, None]
    with np.errstate(all="ignore"):
        v1, v2, v3 = sub(b, a), sub(c, b), sub(d, c)
        r, s = normalize(cross(v1, v2)), normalize(cross(v2, v3))
        t = normalize(cross(r, normalize(v2)))
        return dot(s, t), dot(r, s)


def _quadrants(X):
    """[E, 2, 3, 3] -> [E, 4] quadrant m = (y < 0) | (x < 0) << 1 of the four torsion fields (TOR_FIELDS order)"""
    N, CA, CB = X[:, :, 0, :], X[:, :, 1, :], X[:, :, 2, :]
    out = []
    for i, j in ((0, 1), (1, 0)):
        for y, x in (_torsion_yx(N[:, i], CA[:, i], CB[:, i], CB[:, j]), _torsion_yx(CB[:, i], CB[:, j], CA[:, j], N[:, j])):
            out.append(np.signbit(y).astype(np.int64) | (np.signbit(x).astype(np.int64) << 1))
    return np.stack(out, 1)


def _classify_default(es, first, bins, tables):
    """classes of edges first.. of a default-encoding set; bins[e] = ((ca, cb) of side A, (ca, cb) of side B)"""
    XA = np.asarray(es.XA[first:], np.float32).reshape(-1, 2, 3, 3)
    XB = np.asarray(es.XB[first:], np.float32).reshape(-1, 2, 3, 3)
    qa, qb = _quadrants(XA), _quadrants(XB)
    bound = {}
    for m in range(4):
        for k in range(1, tables["tor_nseg"][m]):
            bound.setdefault(frozenset((int(tables["tor_key"][m][k - 1]), int(tables["tor_key"][m][k]))), []).append((m, int(tables["tor_key"][m][k - 1]), int(tables["tor_key"][m][k])))
    th_pairs = {frozenset((tables["theta_key"][k - 1], tables["theta_key"][k])): (tables["theta_key"][k - 1], tables["theta_key"][k]) for k in range(1, 7)}
    for e in range(len(XA)):
        ha, hb = es.HA[first + e], es.HB[first + e]
        cl = []
        (caa, cba), (cab, cbb) = bins[e]
        if caa != cab:
            cl.append(("ca", min(caa, cab), max(caa, cab)))
        if cba != cbb:
            cl.append(("cb", min(cba, cbb), max(cba, cbb)))
        if len(ha) == 2 and len(hb) == 2:
            ta, tb = (ha[0] >> 8) & 15, (hb[0] >> 8) & 15
            if ta != tb:
                cl.append(("theta",) + tuple(th_pairs.get(frozenset((ta, tb)), (min(ta, tb), max(ta, tb)))))
            keys_a = ((ha[0] >> 4) & 15, ha[0] & 15, (ha[1] >> 4) & 15, ha[1] & 15)
            keys_b = ((hb[0] >> 4) & 15, hb[0] & 15, (hb[1] >> 4) & 15, hb[1] & 15)
            for f in range(4):
                if keys_a[f] != keys_b[f]:
                    hit = [b for b in bound.get(frozenset((keys_a[f], keys_b[f])), []) if b[0] in (qa[e, f], qb[e, f])]
                    cl += [(TOR_FIELDS[f],) + b for b in hit] or [(TOR_FIELDS[f], "other", int(keys_a[f]), int(keys_b[f]))]
        es.classes.append(cl)


def default_edges(seed=20240, min_slots=64 * 96, max_tries=400000, cells=None, min_per_class=MIN_PER_CLASS):
    """edges of the default encoding (PDBTrRosetta, 16 / 4 bins, cutoff 20): slot s is filled at cell s % 64 (or cells[s % len(cells)]); whole
    rounds of 64 slots are added until every class of reachable_classes() holds min_per_class edges (0: no coverage condition)."""
    cfg = DEFAULT
    rng = np.random.Generator(np.random.PCG64(seed))
    probe = _Probe(2)
    tables = header_tables()
    want = reachable_classes(cfg.cutoff) if min_per_class else []
    dthr = np.sqrt(tables["dist_thr"].view(np.float32).astype(np.float64))
    cells = list(range(64)) if cells is None else list(cells)
    es = EdgeSet(cfg)
    bins, counts, slot, done = [], Counter(), 0, 0
    while True:
        lack = [c for c in want if counts[c] < min_per_class]
        if slot >= min_slots and not lack:
            break
        lack_d = [c for c in lack if c[0] in ("ca", "cb")]
        lack_anti = any(c[0] == "theta" and c[1:] == (4, 8) for c in lack)
        for _ in range(64):
            cell = cells[slot % len(cells)]
            while True:
                if es.tries >= max_tries:
                    raise RuntimeError(f"quantiser_edges: try budget ended with classes missing: {[(c, counts[c]) for c in lack][:12]}")
                es.tries += 1
                r = rng.random()
                if lack_d and r < 0.5:                                    # steer to a distance breakpoint that still lacks edges
                    c = lack_d[int(rng.integers(len(lack_d)))]
                    kind, target = c[0], dthr[c[2]] + rng.uniform(-0.25, 0.25)
                elif lack_anti and r < 0.7:
                    kind, target = "anti", rng.uniform(3.0, 19.0)
                elif r < 0.2:
                    k = int(rng.integers(1, 16))
                    kind, target = "ca", dthr[k] + rng.uniform(-0.25, 0.25)
                elif r < 0.4:
                    k = int(rng.integers(1, 20))
                    kind, target = "cb", dthr[k] + rng.uniform(-0.25, 0.25)
                else:
                    kind, target = "any", rng.uniform(2.2, 19.9)
                d = _draw(rng, cfg, cell, kind, max(target, 0.5))
                if d is None:
                    continue
                X, aa, idx, delta = d
                if kind in ("ca", "cb"):
                    delta = 0.8 if delta > 0 else -0.8
                r = _find_edge(probe, cfg, X, aa, idx, delta, lambda h: h)
                if r is None:
                    continue
                a, b, ha, hb = r
                probe.poke(idx, a)
                ba = probe.dist_bins(cfg)
                probe.poke(idx, b)
                bins.append((ba, probe.dist_bins(cfg)))
                es.add(X, aa, cell, idx, a, b, ha, hb)
                break
            slot += 1
        _classify_default(es, done, bins[done:], tables)
        for cl in es.classes[done:]:
            counts.update(cl)
        done = len(es.classes)
    return es.freeze()


def config_edges(cfg, fields, seed, min_slots=256, max_tries=200000, min_per_field=MIN_PER_CLASS):
    """edges of another configuration, under oracle.hash_type(cfg.hash_type): rounds of 64 slots until every hash field of `fields` differs
    across at least min_per_field edges"""
    rng = np.random.Generator(np.random.PCG64(seed))
    probe = _Probe(cfg.nres)
    es = EdgeSet(cfg)
    counts, slot = Counter(), 0
    with oracle.hash_type(cfg.hash_type):
        while slot < min_slots or any(counts[f] < min_per_field for f in fields):
            for _ in range(64):
                while True:
                    if es.tries >= max_tries:
                        raise RuntimeError(f"quantiser_edges: try budget ended for {cfg.name}: {dict(counts)}")
                    es.tries += 1
                    kind = ("any", "ca", "cb")[int(rng.integers(3))]
                    d = _draw(rng, cfg, slot % 64, kind, rng.uniform(2.2, cfg.cutoff - 0.1))
                    if d is None:
                        continue
                    X, aa, idx, delta = d
                    r = _find_edge(probe, cfg, X, aa, idx, delta, lambda h: h)
                    if r is None:
                        continue
                    a, b, ha, hb = r
                    es.add(X, aa, slot % 64, idx, a, b, ha, hb)
                    x = 0
                    if len(ha) == len(hb):
                        for p, q in zip(ha, hb):
                            x |= p ^ q
                    cl = [f for f, m in fields.items() if x & m]
                    es.classes.append(cl)
                    counts.update(cl)
                    break
                slot += 1
    return es.freeze()


def cutoff_edges(hash_type, nres, cutoff, seed, n_slots=128, max_tries=100000):
    """edges that straddle the accept test of the encoding at `cutoff`: the hash list changes its LENGTH across the ulp (2 <-> 0; the
    PointPairFeature test depends on the orientation, so 1 occurs there)"""
    cfg = Cfg(f"cut{cutoff}_t{hash_type}", hash_type, 0, 0, float(cutoff), nres)
    rng = np.random.Generator(np.random.PCG64(seed))
    probe = _Probe(nres)
    es = EdgeSet(cfg)
    with oracle.hash_type(hash_type):
        for slot in range(n_slots):
            while True:
                if es.tries >= max_tries:
                    raise RuntimeError(f"quantiser_edges: try budget ended for {cfg.name}")
                es.tries += 1
                kind = "cb" if hash_type in (2, 4) else "ca"          # the distance fd_accept_other cuts on
                big = Cfg(cfg.name, hash_type, 0, 0, cutoff + 10.0, nres)      # _draw's own CA filter must not reject what is drawn above the cutoff
                d = _draw(rng, big, slot % 64, kind, cutoff + rng.uniform(-0.2, 0.2))
                if d is None:
                    continue
                X, aa, idx, delta = d
                r = _find_edge(probe, cfg, X, aa, idx, 0.8 if delta > 0 else -0.8, len)
                if r is None:
                    continue
                a, b, ha, hb = r
                es.add(X, aa, slot % 64, idx, a, b, ha, hb)
                es.classes.append([("cutoff", len(ha), len(hb))])
                break
    return es.freeze()


def ladder(es, every=3, steps=LADDER_STEPS):
    """for every `every`-th edge: the arrangements whose moved coordinate lies s ulps beyond side A (away from B) and s ulps beyond side B
    (away from A), s in steps -> (X [n, nres, 3, 3], aa, cell, step [n] (negative: A side))"""
    X, aa, cell, st = [], [], [], []
    for e in range(0, len(es), every):
        idx = tuple(es.idx[e])
        ia, ib = f2i(float(es.XA[e][idx])), f2i(float(es.XB[e][idx]))
        sgn = 1 if ib > ia else -1
        for s in steps:
            for base, i0, k in ((es.XA[e], ia, -sgn * s), (es.XB[e], ib, sgn * s)):
                x = base.copy()
                x[idx] = i2f(i0 + k)
                X.append(x); aa.append(es.aa[e]); cell.append(es.cell[e]); st.append(-s if base is es.XA[e] else s)
    return np.asarray(X, np.float32), np.asarray(aa, np.uint8), np.asarray(cell, np.int64), np.asarray(st, np.int64)


# ---- layouts -------------------------------------------------------------------------------------------------------------------------------
def layout_per_pair(X, aa):
    """one structure per arrangement -> dict(res_off, n_xyz, ca_xyz, cb_xyz, aa)"""
    E, n = aa.shape
    return dict(res_off=(np.arange(E + 1, dtype=np.uint64) * np.uint64(n)), n_xyz=np.ascontiguousarray(X[:, :, 0, :]).reshape(-1, 3),
                ca_xyz=np.ascontiguousarray(X[:, :, 1, :]).reshape(-1, 3), cb_xyz=np.ascontiguousarray(X[:, :, 2, :]).reshape(-1, 3), aa=aa.reshape(-1).copy())


def layout_packed(X, aa, cell):
    """the same arrangements, 64 to a structure: structure r holds the r-th arrangement of every cell, in cell order; no coordinate moves"""
    rank = np.zeros(len(cell), np.int64)
    seen = Counter()
    for e, c in enumerate(cell.tolist()):
        rank[e] = seen[c]
        seen[c] += 1
    order = np.lexsort((cell, rank))
    per = aa.shape[1]
    sizes = np.bincount(rank, minlength=int(rank.max()) + 1 if len(rank) else 0) * per
    d = layout_per_pair(X[order], aa[order])
    d["res_off"] = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    d["order"] = order
    return d


def to_oracle_structs(d):
    off = d["res_off"].astype(np.int64)
    ok = d.get("cb_ok")
    return [oracle.structure_from_packed(d["n_xyz"][a:b], d["ca_xyz"][a:b], d["cb_xyz"][a:b], d["aa"][a:b], cb_ok=None if ok is None else ok[a:b])
            for a, b in zip(off[:-1], off[1:])]


def to_packed(d):
    from folddisco_amd import PackedStructures
    return PackedStructures(d["res_off"], d["n_xyz"], d["ca_xyz"], d["cb_xyz"], d["aa"], d.get("cb_ok"))


def oracle_lists(d, cfg, multiple_bins=None):
    """the oracle's raw hash lists (CSR) of every structure of a layout under the configuration"""
    structs = to_oracle_structs(d)
    hs, off = [], [0]
    with oracle.hash_type(cfg.hash_type):
        for s in structs:
            if multiple_bins:
                with oracle.multiple_bins(multiple_bins):
                    h = oracle.hash_structure(s, cfg.nd, cfg.na, cfg.cutoff)
            else:
                h = oracle.hash_structure(s, cfg.nd, cfg.na, cfg.cutoff)
            hs.append(h)
            off.append(off[-1] + len(h))
    return (np.concatenate(hs) if hs else np.zeros(0, np.uint32)), np.asarray(off, np.uint64)


_SETS = None


def all_sets():
    """every edge set of the tests, generated once per process: default (mixed scales, class coverage), origin (the default encoding with every
    pair at cell 0: coordinates below 16 A), ladder (of the default set), cutoff[(hash type, cutoff)], config[name] = (set, fields)"""
    global _SETS
    if _SETS is None:
        d = default_edges()
        _SETS = dict(default=d, origin=default_edges(seed=20241, min_slots=1024, cells=[0], min_per_class=0), ladder=ladder(d),
                     cutoff={(t, c): cutoff_edges(t, n, c, seed=7000 + 10 * k + t) for k, c in enumerate(CUTOFFS) for t, n in CUTOFF_ENCODINGS},
                     config={cfg.name: (config_edges(cfg, fields, seed=9000 + k), fields) for k, (cfg, fields) in enumerate(OTHER)})
    return _SETS
