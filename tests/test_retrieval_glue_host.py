"""The retrieval's host glue itself (csrc/fd_retrieve_host.cpp, through fdgpu_debug_host_retrieve_slot) on the CPU: every hand-made case of
retrieval_cases.py, every target, fed with the oracle's own found triples and candidate pairs, against the oracle's records — their number and order,
both residue lists, `same`, and the idf bit for bit (every idf of these cases is a multiple of 2^-8: the f32 sum is exact in any order).  Single-scan
and two-scan form, candidate pairs as records and packed.  No GPU: the slot function is host C++."""
import ctypes as C

import numpy as np
import pytest

from folddisco_amd import _lib
from tests import retrieval_cases as rc

HASH_TYPE = 3          # the default encoding (FD_HASH_PDBTR): what oracle.pair_hash computes
_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def _res(m):
    return [-1 if x is None else x[2] for x in m["residues"]]


def _u32(a):
    a = np.ascontiguousarray(a, np.uint32)
    return a, a.ctypes.data_as(_lib.u32p)


def host_slot(c, k, two_pass, packed):
    """-> [(idf bits, same, from_hash, processed)] of target k's slot as the host glue emits them"""
    R = rc.oracle_results(c)[k]
    qm = rc.library_map(c.arrays)
    keep = [_u32(R["found"][:, z]) for z in range(3)] + [_u32(R["cand"][:, z]) for z in range(3)]
    n, idf, same, res = C.c_uint64(0), _lib.f32p(), _lib.u32p(), C.POINTER(C.c_int32)()
    err = _lib.load().fdgpu_debug_host_retrieve_slot(keep[0][1], keep[1][1], keep[2][1], len(R["found"]), keep[3][1], keep[4][1], keep[5][1], len(R["cand"]),
                                                     c.targets[k].n, qm.handle, HASH_TYPE, c.node_count, int(two_pass), int(packed), C.byref(n), C.byref(idf),
                                                     C.byref(same), C.byref(res))
    assert err == 0, (c, k, err)
    nq = len(c.arrays["indices"])
    out = [(int(np.float32(idf[r]).view(np.uint32)), int(same[r]), [res[2 * nq * r + z] for z in range(nq)], [res[2 * nq * r + nq + z] for z in range(nq)])
           for r in range(n.value)]
    for p in (idf, same, res):
        _libc.free(C.cast(p, C.c_void_p))
    return out


@pytest.mark.parametrize("packed", (0, 1))
@pytest.mark.parametrize("two_pass", (0, 1))
@pytest.mark.parametrize("cls", rc.CLASSES)
def test_host_slot_equals_oracle(cls, two_pass, packed):
    for c in rc.cases(cls):
        for k, R in enumerate(rc.oracle_results(c)):
            if packed and c.targets[k].n > 65536:
                continue
            got = host_slot(c, k, two_pass, packed)
            assert len(got) == len(R["from_hash"]), (c, k, len(got))
            for (idf, same, fh, pr), ofh, opr in zip(got, R["from_hash"], R["processed"]):
                assert fh == _res(ofh) and pr == _res(opr), (c, k)
                assert same == int(_res(ofh) == _res(opr)), (c, k)
                assert idf == int(np.float32(ofh["idf"]).view(np.uint32)), (c, k)


def _slot_quantities(c, k):
    R = rc.oracle_results(c)[k]
    nodes = len(set(R["found"][:, 0].tolist()) | set(R["found"][:, 1].tolist()))
    q_size = int(max(c.arrays["qi"].max(initial=0), c.arrays["qj"].max(initial=0), c.arrays["indices"].max(initial=0))) + 1
    return dict(edges=len(R["found"]), hashes=len(np.unique(c.arrays["hash"])), dense_votes=len(R["found"]) > 4096 and q_size * c.targets[k].n <= 1 << 20, nodes=nodes)


def test_cases_sit_on_both_sides_of_the_slot_switches():
    """the switches inside fd_rh_slot: 256 found triples (dense residue -> node table), 4,096 triples with q_size x n_target <= 2^20 (dense vote table),
    4,096 hashes (entry table instead of bisection); the 255 saturation and duplicate `indices` are claims of the votes class (test_retrieval_cases_host.py)"""
    q = [_slot_quantities(c, k) for cls in rc.CLASSES for c in rc.cases(cls) for k in range(len(c.targets))]
    assert any(x["edges"] <= 256 for x in q) and any(x["edges"] > 256 for x in q)
    assert any(x["dense_votes"] for x in q) and any(not x["dense_votes"] for x in q)
    assert any(x["hashes"] <= 4096 for x in q) and any(x["hashes"] > 4096 for x in q)
    names = {c.name: c for c in rc.cases("votes")}
    assert names["saturation"].claims["max_vote"] == 255 and names["dup_first"].claims["quirk"]


def test_rejects_what_no_scan_emits():
    c = rc.cases("comps")[0]
    R = rc.oracle_results(c)[0]
    qm = rc.library_map(c.arrays)
    f = [_u32(R["found"][:, z]) for z in range(3)]
    n, idf, same, res = C.c_uint64(0), _lib.f32p(), _lib.u32p(), C.POINTER(C.c_int32)()
    args = lambda n_target, packed, cq: (f[0][1], f[1][1], f[2][1], len(R["found"]), cq, cq, cq, 1, n_target, qm.handle, HASH_TYPE, 2, 0, packed, C.byref(n), C.byref(idf),
                                         C.byref(same), C.byref(res))
    big = _u32([70000])
    assert _lib.load().fdgpu_debug_host_retrieve_slot(*args(int(R["found"][:, :2].max()), 0, big[1])) == -1          # a found residue beyond the target
    assert _lib.load().fdgpu_debug_host_retrieve_slot(*args(c.targets[0].n, 1, big[1])) == -1          # a packed field beyond 16 bits
