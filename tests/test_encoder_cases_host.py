"""CPU: the streams of tests/encoder_cases.py and the numpy model of the index format they are checked against on the device
(tests/test_gpu_encoder_edges.py).  The model equals the oracle's index wherever the ids are small enough to hand the stream to the oracle as
per-structure hash lists, and every property a case is there for is asserted on the model's output, so a case cannot silently stop covering it."""
import numpy as np
import pytest

import oracle
from tests import encoder_cases as ec

CASES = ec.all_cases()
ORACLE_MAX_STRUCTURES = 1 << 20


def test_every_case_is_sorted_and_shows_what_it_claims():
    assert len(CASES) >= 6 + 36 + 16 + 6
    for name, (h, i, check) in CASES.items():
        assert len(h) <= 4 * ec.TILE + 8, name            # at most four tiles (and a few elements of a fifth)
        m = ec.Model(h, i)                                 # asserts sortedness
        check(m)
        assert len(m.hashes) + 1 == len(m.offsets) == len(m.last_ids) + 1 and int(m.offsets[-1]) == len(m.value), name
        assert np.all(np.diff(m.hashes.astype(np.int64)) > 0), name


def test_model_equals_the_oracle_where_the_ids_are_small():
    compared = 0
    for name, (h, i, _) in CASES.items():
        if int(i.max()) >= ORACLE_MAX_STRUCTURES:
            continue
        m = ec.Model(h, i)
        lh, off = ec.per_structure_lists(h, i)
        oix = oracle.build_index_from_lists_mt(lh, off, 2)
        assert np.array_equal(m.hashes, oix.hashes()), name
        assert np.array_equal(m.offsets, oix.offsets()), name
        assert np.array_equal(m.value, oix.values()), name
        for k in (0, len(m.hashes) // 2, len(m.hashes) - 1):      # last_ids: the last entry of the oracle's decoded list
            assert int(oix.entries(int(m.hashes[k]))[-1]) == int(m.last_ids[k]), name
        compared += 1
    # the sizes, the alignments, the long list, the duplicate runs and the boundary values up to 0x4000
    assert compared == 6 + 16 + 1 + 3 + 4 * 4, compared


@pytest.mark.parametrize("v", [0, 1, 0x7f, 0x80, 0x3fff, 0x4000, 0x1fffff, 0x200000, 0xfffffff, 0x10000000, 0xffffffff])
def test_model_varint_bytes(v):
    """the model's LEB128 on single postings against the definition, byte by byte"""
    m = ec.Model([9], [v])
    want, x = [], v
    while True:
        want.append((x & 0x7f) | (0x80 if x >> 7 else 0))
        x >>= 7
        if not x:
            break
    assert m.value.tolist() == want and int(ec.varint_len(v)) == len(want) and m.last_ids.tolist() == [v]
