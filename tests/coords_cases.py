"""Cases of the resident-batch tests (tests/test_gpu_coords.py): a hand-made batch whose structure lengths sit on every edge of the select kernel's
64-residue tiles, with bytes a copy must not touch (NaN, -0.0, aa = 255, cb_valid = 0), the id lists, and the expected result by numpy alone."""
import functools

import numpy as np

# 0 (no work item), one residue, the tile edges 63 / 64 / 65, 127 / 128 / 129, 191 / 192 / 193 (the three 64-lane steps of a 192-dword run),
# more than one block of four wavefronts (300), many tiles (1000), a length that is 1 past a multiple of 64 (4097)
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 300, 1000, 4097]
LONG = 65535                                 # the longest structure a batch accepts (copy tests only: 1,024 tiles of one structure)


@functools.lru_cache(maxsize=None)
def arrays(with_long: bool = True):
    """-> dict(res_off, n_xyz, ca_xyz, cb_xyz, aa, cb_valid), computed once per process: callers leave the arrays as they are"""
    lens = LENGTHS + ([LONG] if with_long else [])
    rng = np.random.Generator(np.random.PCG64(20261018))
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    R = int(off[-1])
    xyz = lambda: (rng.standard_normal((R, 3)) * 30.0).astype(np.float32)
    d = dict(res_off=off, n_xyz=xyz(), ca_xyz=xyz(), cb_xyz=xyz(), aa=rng.integers(0, 20, R).astype(np.uint8), cb_valid=np.ones(R, np.uint8))
    d["aa"][rng.integers(0, R, 40)] = 255
    d["aa"][[int(off[3]) + 62, int(off[4]) + 63, int(off[5]) + 64]] = 255      # the last residue of the 63 / 64 / 65 structures
    d["cb_valid"][rng.integers(0, R, 40)] = 0
    d["cb_valid"][[int(off[6]), int(off[8]) + 128]] = 0
    d["ca_xyz"][int(off[5]) + 64, 1] = np.nan                 # the one residue of a structure's second tile
    d["cb_xyz"][int(off[7]) + 127, 2] = np.float32(-0.0)      # the last residue of a full tile
    d["n_xyz"].view(np.uint32)[int(off[9]) + 100, 0] = 0x7fc12345      # a NaN with a payload: compared as bytes
    for a in d.values():
        a.setflags(write=False)
    return d


def packed(with_long: bool = True, with_cbv: bool = True):
    from folddisco_amd import PackedStructures
    d = arrays(with_long)
    return PackedStructures(d["res_off"], d["n_xyz"], d["ca_xyz"], d["cb_xyz"], d["aa"], d["cb_valid"] if with_cbv else None)


def id_lists(n: int):
    """name -> ids over a batch of n structures whose structure 0 is the empty one"""
    rng = np.random.Generator(np.random.PCG64(77))
    return {
        "identity": np.arange(n),
        "reverse": np.arange(n)[::-1].copy(),
        "random": rng.permutation(n),
        "gaps": np.arange(1, n, 3),
        "repeats": np.array([5, 5, 0, n - 1, 5, 3, 0, 3, n - 1, n - 1, 12]),
        "empty": np.zeros(0, np.int64),
        "last": np.array([n - 1]),
        "only_zero_length": np.array([0, 0, 0]),
    }


def gather(ps, ids):
    """the numpy expectation of Batch.select(ids).export() -> dict of arrays"""
    off = ps.res_off.astype(np.int64)
    ids = np.asarray(ids, np.int64)
    lens = off[ids + 1] - off[ids]
    new = np.zeros(len(ids) + 1, np.uint64)
    new[1:] = np.cumsum(lens)
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in ids]) if len(ids) else np.zeros(0, np.int64)
    return dict(res_off=new, n_xyz=ps.n_xyz[idx], ca_xyz=ps.ca_xyz[idx], cb_xyz=ps.cb_xyz[idx], aa=ps.aa[idx],
                cb_valid=None if ps.cb_valid is None else ps.cb_valid[idx])


def same_bytes(got, want) -> bool:
    """exported PackedStructures against gather()'s dict, every array as bytes (NaN payloads and the sign of zero included)"""
    for name in ("res_off", "n_xyz", "ca_xyz", "cb_xyz", "aa", "cb_valid"):
        g, w = getattr(got, name), want[name]
        if (g is None) != (w is None):
            return False
        if g is not None and (g.size != np.asarray(w).size or g.tobytes() != np.ascontiguousarray(w).tobytes()):
            return False
    return True
