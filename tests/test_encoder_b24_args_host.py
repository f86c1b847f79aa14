"""The argument checks of the test-only entry fdgpu_debug_encode_stream_b24 (include/fdgpu_debug.h), which come before the context is used: with no
context the call is those checks alone, so they run without a device.  tests/test_gpu_encoder_constant_tiles.py drives the encoder through it."""
import ctypes as C

import numpy as np
import pytest

from folddisco_amd import _lib

OK, EINVAL = 0, -1


def _call(h, loc, first_id=0):
    L = _lib.load()
    h = np.ascontiguousarray(h, np.uint32)
    loc = np.ascontiguousarray(loc, np.uint32)
    out = C.c_void_p(1)
    rc = L.fdgpu_debug_encode_stream_b24(None, h.ctypes.data_as(_lib.u32p), loc.ctypes.data_as(_lib.u32p), len(h), first_id, C.byref(out))
    assert out.value is None      # nothing is made without a context
    return rc


GOOD_H = [5, 5, 5 | 1 << 24, 39 << 24 | 0xffffff]
GOOD_ID = [0, 7, 7, (1 << 24) - 1]


def test_a_stream_it_would_encode_passes():
    assert _call(GOOD_H, GOOD_ID) == OK
    assert _call([], []) == OK
    assert _call(GOOD_H, GOOD_ID, first_id=(1 << 32) - (1 << 24) - 1) == OK


@pytest.mark.parametrize("h,loc", [([6, 5], [0, 0]), ([5, 5], [3, 2]), ([1 << 24, 5], [0, 0])], ids=["hash", "id", "bucket"])
def test_unsorted_stream(h, loc):
    assert _call(h, loc) == EINVAL


@pytest.mark.parametrize("h", [40 << 24, 63 << 24 | 5, 1 << 30, 0xffffffff], ids=hex)
def test_bucket_of_forty_or_more(h):
    assert _call([5, h], [0, 0]) == EINVAL


@pytest.mark.parametrize("i", [1 << 24, 0xffffffff], ids=hex)
def test_local_id_of_2_to_the_24_or_more(i):
    assert _call([5, 5], [0, i]) == EINVAL


def test_ids_beyond_32_bits_and_missing_arguments():
    assert _call(GOOD_H, GOOD_ID, first_id=(1 << 32) - (1 << 24)) == EINVAL
    L = _lib.load()
    h = np.zeros(1, np.uint32)
    assert L.fdgpu_debug_encode_stream_b24(None, h.ctypes.data_as(_lib.u32p), h.ctypes.data_as(_lib.u32p), 1, 0, None) == EINVAL
    out = C.c_void_p()
    assert L.fdgpu_debug_encode_stream_b24(None, None, None, 1, 0, C.byref(out)) == EINVAL
