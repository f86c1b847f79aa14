"""CPU-only tests of the quantiser edge sets (tests/quantiser_edges.py): the generator's own conditions, the device geometry headers compiled
for the host against the oracle ON the thresholds, and the squared-distance table's correction logic."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oracle
from tests import quantiser_edges as qe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _all_edge_sets(S):
    return [S["default"], S["origin"]] + list(S["cutoff"].values()) + [v for v, _ in S["config"].values()]


def test_generator_covers_every_reachable_class(capsys):
    """the class list is pinned against fd_bin_tables.h / fd_dist_table.h, and every class holds at least 16 edges (the generator raises
    otherwise); the counts are printed"""
    t = qe.header_tables()
    want = qe.reachable_classes()
    # distance breakpoints of fd_dist_table.h: sqrt(T[k]) = 2 + (k - 0.5) * 1.2 -> CA bins up to the 20 A cutoff, CB bins up to 24.2 A
    d = np.sqrt(t["dist_thr"].view(np.float32).astype(np.float64))
    assert np.allclose(d[1:], 2.0 + (np.arange(1, 33) - 0.5) * 1.2, atol=1e-5)
    assert [c[1:] for c in want if c[0] == "ca"] == [(k - 1, k) for k in range(1, 16)]
    assert [c[1:] for c in want if c[0] == "cb"] == [(k - 1, k) for k in range(1, 20)] and ("cb", 15, 16) in want
    assert [c[1:] for c in want if c[0] == "theta"] == [(4, 8), (8, 12), (12, 13), (13, 14), (14, 15), (15, 11)] and len(t["theta_thr"]) == 7
    assert t["tor_nseg"] == [5, 4, 5, 5]
    for f in qe.TOR_FIELDS:
        assert [c[1:] for c in want if c[0] == f] == [(0, 11, 7), (0, 7, 3), (0, 3, 2), (0, 2, 1), (1, 11, 15), (1, 15, 14), (1, 14, 13),
                                                     (2, 8, 4), (2, 4, 0), (2, 0, 1), (2, 1, 2), (3, 4, 8), (3, 8, 12), (3, 12, 13), (3, 13, 14)]
    assert len(want) == 15 + 19 + 6 + 4 * 15
    S = qe.all_sets()
    cc = S["default"].class_counts()
    with capsys.disabled():
        print(f"\n{len(S['default'])} default edges from {S['default'].tries} tries")
        for c in want:
            print("  ", c, cc[c])
    assert all(cc[c] >= qe.MIN_PER_CLASS for c in want), [(c, cc[c]) for c in want if cc[c] < qe.MIN_PER_CLASS]
    # both coordinate scales: cell 0 is the origin, the others reach PDB-like magnitudes
    X = S["default"].XA
    near = S["default"].cell == 0
    assert near.sum() * 64 == len(X) and np.abs(X[near]).max() < 20.0 and np.abs(X[~near]).max() > 450.0 and np.abs(S["origin"].XA).max() < 20.0
    # the other configurations: at least 16 edges per hash field; the cutoff sets: both directions of the accept test
    for name, (es, fields) in S["config"].items():
        c2 = es.class_counts()
        assert all(c2[f] >= qe.MIN_PER_CLASS for f in fields), (name, dict(c2))
    for (t_, cut), es in S["cutoff"].items():
        assert len(es) == 128 and all(cl[0][1] != cl[0][2] for cl in es.classes), (t_, cut)
        if t_ != 4:
            assert set(es.class_counts()) == {("cutoff", 0, 2), ("cutoff", 2, 0)}


def test_generator_is_deterministic():
    S = qe.all_sets()
    again = qe.default_edges()
    assert again.tobytes() == S["default"].tobytes() and again.HA == S["default"].HA and again.tries == S["default"].tries
    assert qe.cutoff_edges(4, 2, 12.5, seed=7000 + 10 * 1 + 4).tobytes() == S["cutoff"][(4, 12.5)].tobytes()
    cfg, fields = qe.OTHER[8]
    assert cfg.name == "tertiary" and qe.config_edges(cfg, fields, seed=9008).tobytes() == S["config"]["tertiary"][0].tobytes()


def test_every_edge_differs_across_one_ulp_under_the_oracle():
    S = qe.all_sets()
    n = 0
    for es in _all_edge_sets(S):
        diff = es.XA.view(np.uint32) != es.XB.view(np.uint32)
        assert np.all(diff.reshape(len(es), -1).sum(1) == 1)
        ia = np.array([qe.f2i(float(v)) for v in es.XA[diff]])
        ib = np.array([qe.f2i(float(v)) for v in es.XB[diff]])
        assert np.all(np.abs(ia - ib) == 1) and np.all(np.isfinite(es.XA)) and np.all(es.aa < 20)
        cfg = es.cfg
        ha, oa = qe.oracle_lists(qe.layout_per_pair(es.XA, es.aa), cfg)
        hb, ob = qe.oracle_lists(qe.layout_per_pair(es.XB, es.aa), cfg)
        for e in range(len(es)):
            a, b = ha[int(oa[e]):int(oa[e + 1])], hb[int(ob[e]):int(ob[e + 1])]
            assert tuple(a) == es.HA[e] and tuple(b) == es.HB[e] and tuple(a) != tuple(b), (cfg.name, e)
            if cfg.name.startswith("cut"):
                assert len(a) != len(b)
            n += 1
    assert n > 14000
    # the ladder: the step-1 rungs are the next floats beyond the edge, the rungs of one edge differ in the moved coordinate only
    X, aa, cell, st = S["ladder"]
    assert len(X) == 2 * len(qe.LADDER_STEPS) * ((len(S["default"]) + 2) // 3) and set(np.abs(st).tolist()) == set(qe.LADDER_STEPS)


def _write_case(path, d, cfg):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<5I", 0x45514446, len(d["res_off"]) - 1, cfg.hash_type, cfg.nd, cfg.na) + struct.pack("<f", cfg.cutoff) + struct.pack("<2I", len(d["aa"]), 0))
        fh.write(np.ascontiguousarray(d["res_off"], np.uint64).tobytes())
        for k in ("n_xyz", "ca_xyz", "cb_xyz"):
            fh.write(np.ascontiguousarray(d[k], np.float32).tobytes())
        fh.write(np.ascontiguousarray(d["aa"], np.uint8).tobytes())


def test_device_geometry_headers_equal_oracle_on_the_edges(tmp_path):
    """fd_geom.h (generic, shared-subexpression and table forms, both accept tests; the speculative form with and without the squared-distance
    table, its device instructions emulated by tools/host_hip: whatever it accepts) and fd_geom_other.h compiled for the host == oracle on
    the default set (both layouts), the origin set, the ladders, the cutoff edges of every encoding and the other configurations; on the
    ladders the speculation both accepts and refuses"""
    oracle.build()
    exe = str(tmp_path / "check_geom_edges")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-D__HIPCC__", "-Itools/host_hip", "tools/check_geom_edges.cpp", "-Loracle", "-lfdoracle",
                           f"-Wl,-rpath,{ROOT}/oracle", "-o", exe], cwd=ROOT)
    S = qe.all_sets()
    cases = []
    X, aa, cell = S["default"].sides()
    cases += [("default per pair", qe.layout_per_pair(X, aa), qe.DEFAULT), ("default packed", qe.layout_packed(X, aa, cell), qe.DEFAULT)]
    X, aa, cell = S["origin"].sides()
    cases.append(("origin", qe.layout_per_pair(X, aa), qe.DEFAULT))
    X, aa, cell, _ = S["ladder"]
    cases += [("ladder per pair", qe.layout_per_pair(X, aa), qe.DEFAULT), ("ladder packed", qe.layout_packed(X, aa, cell), qe.DEFAULT)]
    for es in list(S["cutoff"].values()) + [v for v, _ in S["config"].values()]:
        X, aa, cell = es.sides()
        cases.append((es.cfg.name, qe.layout_per_pair(X, aa), es.cfg))
        if es.cfg.nres == 2:
            cases.append((es.cfg.name + " packed", qe.layout_packed(X, aa, cell), es.cfg))
    accepted = 0
    spec = {}
    for k, (name, d, cfg) in enumerate(cases):
        path = str(tmp_path / f"case{k}.bin")
        _write_case(path, d, cfg)
        out = subprocess.run([exe, path], capture_output=True, text=True)
        assert out.returncode == 0 and "mismatches: 0" in out.stdout, (name, out.stdout[-500:], out.stderr[-2000:])
        accepted += int(re.search(r"(\d+) accepted", out.stdout).group(1))
        spec[name] = tuple(int(x) for x in re.search(r"speculation (\d+) of (\d+)", out.stdout).groups())
        os.remove(path)
    assert accepted > 300000
    print({k: v for k, v in spec.items() if v[1]})
    for name in ("ladder per pair", "ladder packed", "default per pair"):
        assert 0 < spec[name][0] < spec[name][1], (name, spec[name])
    assert spec["origin"][1] > 0 and spec["pdbtr_8_4"][1] > 0


def test_squared_distance_table_corrects_every_guess_within_one_bin():
    """fd_dist_bin_tab restated for the host with its v_sqrt_f32 guess replaced by EVERY bin within one of the true bin: bin = b + (x >= T[b + 1]) -
    (x < T[b]) equals sqrtf + quantiser at every breakpoint +-2 ulps of the squared distance and on the squared CA / CB distances of the distance
    edges (both sides of each); a guess beyond the table clears ok like the device code (clamp to FD_DIST_NTHR - 2)"""
    T = qe.header_tables()["dist_thr"]
    thr = T.view(np.float32)
    disc = np.float32(1.0) / (np.float32(18.0) / np.float32(15.0))

    def chain(x):
        with np.errstate(invalid="ignore"):
            v = (np.sqrt(x.astype(np.float32)) - np.float32(2.0)) * disc + np.float32(0.5)
        return np.where(v > 0, np.floor(np.maximum(v, np.float32(0))), 0).astype(np.int64)
    S = qe.all_sets()
    es = S["default"]
    pick = np.array([any(c[0] in ("ca", "cb") for c in cl) for cl in es.classes])
    assert pick.sum() > 2000
    xs = [(T[1:, None].astype(np.int64) + np.arange(-2, 3)[None, :]).ravel().astype(np.uint32).view(np.float32)]
    for X in (es.XA[pick], es.XB[pick]):
        for atom in (1, 2):
            dlt = X[:, 0, atom, :] - X[:, 1, atom, :]
            xs.append(dlt[:, 0] * dlt[:, 0] + dlt[:, 1] * dlt[:, 1] + dlt[:, 2] * dlt[:, 2])       # fd_dist2: same order, f32
    x = np.concatenate(xs).astype(np.float32)
    want = chain(x)
    assert want.max() == 32 and len(np.unique(want)) >= 20
    assert np.array_equal(want, np.searchsorted(thr[1:], x, side="right"))
    n_thr = len(T)
    for dg in (-1, 0, 1):
        b0 = np.maximum(want + dg, 0)
        b = np.minimum(b0, n_thr - 2)
        ok = b0 == b                                      # false: the device hands the pair to the exact routine
        got = b + (x >= thr[b + 1]).astype(np.int64) - (x < thr[b]).astype(np.int64)
        assert np.array_equal(got[ok], want[ok]) and np.all(want[~ok] + dg > n_thr - 2) and ok.sum() >= len(x) - 10, dg
    # a one-ulp move of a breakpoint would be seen: the edges' squared distances sit on the breakpoints themselves
    on = np.isin(x.view(np.uint32), T[1:]) | np.isin(x.view(np.uint32) + 1, T[1:])
    assert on.sum() >= 16 * 15
