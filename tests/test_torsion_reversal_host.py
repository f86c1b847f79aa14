"""CPU-only tests of the torsion reversal set (tests/torsion_reversal_cases.py): the generator's own conditions, and the speculative form of
fd_geom.h compiled for the host (tools/check_geom_edges.cpp) on pairs whose two readings of one dihedral land in different bins under the
oracle: it decides each dihedral once for both readings, so it must refuse every such pair, and whatever it accepts must be the oracle's hash."""
import os
import re
import subprocess

import numpy as np

import oracle
from tests import quantiser_edges as qe
from tests import torsion_reversal_cases as trc
from tests.test_quantiser_edges_host import _write_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generator_meets_its_conditions_and_is_deterministic(capsys):
    rs = trc.reversal_set()
    cnt = rs.counts()
    with capsys.disabled():
        print(f"\n{len(rs)} pairs from {rs.edges} torsion edges ({rs.tries} tries); disagreeing pairs per [dihedral][quadrant]: {cnt}")
    for d in range(2):
        assert sum(cnt[d]) >= trc.MIN_DISAGREE and min(cnt[d]) >= trc.MIN_PER_QUADRANT, cnt
    # as many agreeing ladder neighbours as disagreeing pairs, all within 64 ulps of an edge
    bad = rs.disagree.any(1)
    assert bad.sum() * 2 == len(rs) and np.abs(rs.step).max() <= 64 and 2000 > len(rs) >= 4 * trc.MIN_DISAGREE
    # the flags restate the oracle's hashes, and the hashes are the oracle's on both layouts
    for lay in (rs.per_pair(), rs.packed()):
        h, off = qe.oracle_lists(lay, qe.DEFAULT)
        assert len(h) == 2 * len(rs)
    h, off = qe.oracle_lists(rs.per_pair(), qe.DEFAULT)
    assert np.array_equal(h.reshape(-1, 2), rs.H) and np.array_equal(off, np.arange(len(rs) + 1) * 2)
    k = [(rs.H[:, 0] >> 4) & 15, rs.H[:, 0] & 15, (rs.H[:, 1] >> 4) & 15, rs.H[:, 1] & 15]
    for d, (f, r) in enumerate(trc.DIHEDRAL_FIELDS):
        assert np.array_equal(k[f] != k[r], rs.disagree[:, d])
    assert trc.generate().tobytes() == rs.tobytes()


def test_speculation_refuses_every_pair_whose_readings_differ(tmp_path):
    """zero wrong hashes with and without the distance table (the tool runs both forms); none of the disagreeing pairs accepted; some pairs
    accepted, so decisions a few ulps from a threshold are compared too"""
    oracle.build()
    exe = str(tmp_path / "check_geom_edges")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-D__HIPCC__", "-Itools/host_hip", "tools/check_geom_edges.cpp", "-Loracle", "-lfdoracle",
                           f"-Wl,-rpath,{ROOT}/oracle", "-o", exe], cwd=ROOT)
    rs = trc.reversal_set()
    n_bad = int(rs.disagree.any(1).sum())
    for name, lay in (("per pair", rs.per_pair()), ("packed", rs.packed())):
        path = str(tmp_path / "case.bin")
        _write_case(path, lay, qe.DEFAULT)
        out = subprocess.run([exe, path], capture_output=True, text=True)
        print(name, out.stdout.strip())
        assert out.returncode == 0 and "mismatches: 0" in out.stdout, (name, out.stdout[-500:], out.stderr[-2000:])
        taken, tried = (int(x) for x in re.search(r"speculation (\d+) of (\d+)", out.stdout).groups())
        differ, differ_taken = (int(x) for x in re.search(r"reversed readings differ on (\d+), speculation took (\d+) of them", out.stdout).groups())
        # the tool walks ordered pairs: every pair of the set twice
        assert tried == 2 * len(rs) and differ == 2 * n_bad and differ_taken == 0, (name, out.stdout)
        assert 0 < taken <= tried - differ, (name, out.stdout)
        os.remove(path)
