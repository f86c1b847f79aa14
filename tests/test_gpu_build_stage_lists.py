"""The stage list of an index build call (csrc/fd_api_build.hip: ib_choose_form and the ib_* stages), as fdgpu_last_timings reports it with
timing enabled: the stages' names in launch order and the byte figure of each.  bench.py reads exactly this per stage, and every form of the
build — MSD (the default), structure-major with 6-byte elements (FDGPU_MSD=0), 8-byte elements (FDGPU_IDS32=1), an encoding with its own
descriptor (row kernels), --multiple-bins (structure-major, one emit per bin pair) and the wide retry out of both 6-byte forms — has its own.

The literals below were recorded from commit 35fcfcd (the last one whose build was a single function asking `own / msd / else` at every stage)
on the batch this module makes: an empty structure, one of 5 residues (shorter than a tile) and one of 70 (across a 64-residue tile edge), every
residue pair inside the cutoff; for the retry a fourth structure, the third with one CB at 3.0e38 (its CB distances overflow to inf: hashes
beyond 30 bits, which the 6-byte forms cannot hold).  A build that was retried reports the stages of the run that finished, the 8-byte one, and
its index must equal the FDGPU_IDS32=1 build byte for byte."""
import numpy as np
import pytest

from tests import quantiser_edges as qe
from tests.test_gpu_emit_private_slots import _blob, _layout

ENV = ("FDGPU_DTAB", "FDGPU_EXACT", "FDGPU_MSD", "FDGPU_IDS32")
FORMS = {      # name -> (environment, arguments of the build)
    "msd": ({}, {}),
    "ids16": ({"FDGPU_MSD": "0"}, {}),
    "ids32": ({"FDGPU_IDS32": "1"}, {}),
    "own": ({}, {"hash_type": 2}),
    "multiple_bins": ({}, {"multiple_bins": [(16, 4), (8, 3)]}),
}
# recorded from 35fcfcd: (stage, bytes) in launch order
def _sort(passes, hist, scan, scatter):
    return [("rs_hist", hist), ("rs_scan", scan), ("rs_scatter", scatter)] * passes


EXPECTED = {
    "msd": [("frames", 2550), ("pair_count", 9630), ("segment_scan", 1440), ("pair_emit", 31875),
            ("rs_hist", 5305288), ("rs_scan", 10571776), ("rs_scatter", 58200), *_sort(2, 5295588, 10571776, 58200),
            ("encode_sizes", 29100), ("encode_write", 91994)],
    "ids16": [("frames", 8775), ("pair_count", 975), ("segment_scan", 36), ("pair_emit", 31875), *_sort(4, 20424, 2048, 58200),
              ("encode_sizes", 29100), ("encode_write", 91994)],
    "ids32": [("frames", 8775), ("pair_count", 975), ("segment_scan", 36), ("pair_emit", 41575), *_sort(4, 20424, 2048, 77600),
              ("encode_sizes", 38800), ("encode_write", 101694)],
    "own": [("frames", 8775), ("pair_count", 2775), ("pair_emit", 41559), *_sort(4, 20416, 2048, 77568),
            ("encode_sizes", 38784), ("encode_write", 101730)],
    "multiple_bins": [("frames", 8775), ("pair_count", 975), ("segment_scan", 36), ("pair_emit", 60975), *_sort(4, 40848, 4096, 116400),
                      ("encode_sizes", 58200), ("encode_write", 183559)],
}
# with the fourth structure, out of either 6-byte form: the 8-byte build's list
_WIDE = [("frames", 16965), ("pair_count", 1885), ("segment_scan", 48), ("pair_emit", 82805), *_sort(4, 40768, 4096, 154880),
         ("encode_sizes", 77440), ("encode_write", 145054)]
EXPECTED_RETRY = {"msd": _WIDE, "ids16": _WIDE}


def make_batch(with_far=False):
    rng = np.random.Generator(np.random.PCG64(4711))
    d = _layout([(np.zeros((0, 3)), np.zeros(0, np.uint8)), (_blob(rng, 5), rng.integers(0, 20, 5)), (_blob(rng, 70), rng.integers(0, 20, 70))])
    if with_far:
        a = int(d["res_off"][2])
        far = {k: d[k][a:].copy() for k in ("n_xyz", "ca_xyz", "cb_xyz", "aa")}
        far["cb_xyz"][7] = np.float32(3.0e38)
        d = dict(res_off=np.append(d["res_off"], d["res_off"][3] + np.uint64(70)).astype(np.uint64),
                 **{k: np.concatenate([d[k], far[k]]) for k in far})
    return qe.to_packed(d)


def build_with_stages(ctx, monkeypatch, packed, form):
    """-> (exported index, [(stage, bytes)]) of one build call in the given form"""
    import folddisco_amd as fd
    env, kw = FORMS[form]
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ix = fd.FolddiscoIndex.build(ctx, ctx.upload(packed), first_id=3, **kw)
    stages = [(name, nbytes) for name, _, nbytes in ctx.last_timings()]
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return ix.export(), stages


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    c.enable_timing(True)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_stage_list_of_every_form(ctx, monkeypatch, form):
    _, stages = build_with_stages(ctx, monkeypatch, make_batch(), form)
    print(form, stages)
    assert stages == EXPECTED[form]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["msd", "ids16"])
def test_stage_list_of_the_wide_retry(ctx, monkeypatch, form):
    packed = make_batch(with_far=True)
    got, stages = build_with_stages(ctx, monkeypatch, packed, form)
    print(form, stages)
    assert stages == EXPECTED_RETRY[form]
    want, wide = build_with_stages(ctx, monkeypatch, packed, "ids32")
    assert stages == wide      # the retry IS the 8-byte build
    assert got[1].max() >= (1 << 30)
    for a, b, name in zip(got, want, ("values", "hashes", "offsets")):
        assert np.array_equal(a, b), name
