"""Ranked scoring on the hand-made posting lists of scoring_cases.py, at the switches of its dispatch and at the list layouts the tiled kernels depend on,
against the integer model of that module BYTE FOR BYTE (no tolerance: the fixed-point arithmetic is exactly reproducible), with the form that ran
read back through fdgpu_debug_last_count_path after every call.

Per case and first_id (0, 3000, 2^28 - 40,000, 2^32 - 1 - S): the index is loaded, verifies clean where every id is in range, its posting lengths
equal the model's; count_query_batch with top_n = 0 and with every top_n of the case plus 1, 3072 and 3073; for a case of one query count_query as well
(the single entry point: the model's full list and the rows form); for map cases count_query_maps in the
default form and under FDGPU_QT32=0, FDGPU_QT32=0 + FDGPU_QT_STREAM=0 and FDGPU_QTILE=0.  The expected form restates the dispatch's conditions from
the model's units (no zero-unit row, units below 2^32, rows <= 128 / <= 1024 / >= 4096 in one query, fix < 2^27, top_n + 1024 <= 4096).

Map cases sit on the query map of residues B18 .. B24 of tests/golden/query/4CHA.pdb (scoring_cases.MOTIF: the first of the shortest runs of consecutive
residues whose map has at least 160 entries; test_scoring_cases_host.py checks that on the CPU) and, for the mixed batches, of B18 .. B19.
Measured: the module's 69 tests take 10 s on an MI355X, the slowest 0.5 s."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import scoring_cases as sc
from tests.helpers import Q4CHA

pytestmark = pytest.mark.gpu

TILED, SUMS32, STREAM, SLICED, ROWS, PACKED, OVERFLOW = 1, 2, 4, 8, 16, 32, 64
EXTRA_N = (1, 3072, 3073)
ENVS = ({}, {"FDGPU_QT32": "0"}, {"FDGPU_QT32": "0", "FDGPU_QT_STREAM": "0"}, {"FDGPU_QTILE": "0"})


@pytest.fixture(scope="module")
def ctx():
    import folddisco_amd as fd
    c = fd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def motif(ctx):
    """the query structure on the device, the residues of the two motifs, and their maps made without an index: the rows (hash, qi, qj)"""
    import folddisco_amd as fd
    from folddisco_amd import query as fq
    from folddisco_amd import structure as st
    q = st.read_compact_structure(Q4CHA)
    qb = ctx.upload(fd.PackedStructures.concat([q.as_item()]))
    out = dict(qb=qb, idx={}, subs={}, rows={})
    for name, m in (("big", sc.MOTIF), ("small", sc.MOTIF_SMALL)):
        res = fq.parse_query_string(m, q.chains[0])
        out["idx"][name] = [q.get_index(c, r) for c, r, _ in res]
        out["subs"][name] = [s for _, _, s in res]
        qm = fq.make_query_map(ctx, qb, out["idx"][name], out["subs"][name], None, 0.0)
        out["rows"][name] = (qm.hash.copy(), qm.qi.copy(), qm.qj.copy())
    out["slots"] = sc.map_slots(out["rows"]["big"][0], out["rows"]["small"][0])
    assert len(out["rows"]["big"][0]) == sc.MAX_MAP_ROWS
    return out


@functools.lru_cache(maxsize=None)
def _batch_cases(first_id):
    return sc.batch_cases(first_id)


def last_path(ctx):
    f = C.c_uint32(0)
    ctx.check(ctx.L.fdgpu_debug_last_count_path(ctx.h, C.byref(f)))
    return f.value


def expected_path(via, top_n, kept_fix, env):
    """the dispatch of fd_count_query_batch_impl restated: kept_fix = per query the kept rows' idf units"""
    qtile, qt32_env, stream_env = env.get("FDGPU_QTILE") != "0", env.get("FDGPU_QT32") != "0", env.get("FDGPU_QT_STREAM") != "0"
    rows = [len(f) for f in kept_fix]
    nq, max_rows = sum(rows), max(rows)
    packed = all(int(x) < 1 << 27 for f in kept_fix for x in f) and max_rows < 1 << 18
    sums_fit32 = all(int(x) != 0 for f in kept_fix for x in f) and all(sum(int(x) for x in f) < 1 << 32 for f in kept_fix)
    dense = packed and 0 < top_n and top_n + 1024 <= 4096
    sliced = len(rows) == 1 and nq >= 4096
    tiled = dense and not sliced and qtile and max_rows <= 1024
    qt32 = tiled and qt32_env and sums_fit32 and via == "maps" and max_rows <= 128
    big = dense and sliced and qtile
    stream = tiled and (qt32 or (stream_env and via == "maps"))
    return ((TILED if tiled else 0) | (SUMS32 if qt32 else 0) | (STREAM if stream else 0) | (SLICED if big else 0) | (0 if tiled or big else ROWS)
            | (PACKED if packed else 0))


def run_case(ctx, motif, c, first_id, monkeypatch):
    import folddisco_amd as fd
    from folddisco_amd import query as fq
    from folddisco_amd.api import REC_DTYPE
    assert REC_DTYPE == sc.REC
    h, o, v, L = c.index(first_id, motif["slots"][0])
    ix = fd.FolddiscoIndex.load(ctx, h, o, v, sc.S, first_id=first_id)
    if c.in_range:
        rep = ix.verify()
        assert rep.ok, (c, str(rep))
    rows = c.rows(motif["rows"])
    mods = [sc.model_full(L, q, c.total, c.penalty, first_id, sc.S) for q in rows]
    for q, m in zip(rows, mods):
        assert np.array_equal(ix.posting_lengths(q[0]), m[2].astype(np.uint64)), c
    kept_fix = [m[3][m[2] > 0] for m in mods]
    ns = tuple(sorted(set(c.top_ns + EXTRA_N)))
    seen = {}

    def check(got, n, via, env):
        path = last_path(ctx)
        for t, (g, m) in enumerate(zip(got, mods)):
            want = m[0] if n == 0 else sc.rank(m[0], n)
            assert len(g) == len(want) and g.tobytes() == want.tobytes(), (c, first_id, via, n, env, t, hex(path))
        want_path = expected_path(via, n, kept_fix, env)
        assert path & ~OVERFLOW == want_path, (c, first_id, via, n, env, hex(path), hex(want_path))
        if "overflow" in c.claims and n == 50 and path & TILED:          # 1075 equal keys at the cut of a selection that holds 1074
            assert bool(path & OVERFLOW) == c.claims["overflow"], (c, first_id, via, env, hex(path))
        if n > 3072:
            assert not path & (TILED | SLICED)
        seen[(via, n, tuple(sorted(env)))] = path

    for n in (0,) + ns:
        check(fd.count_query_batch(ctx, ix, rows, c.penalty, total_structures=c.total, top_n=n), n, "batch", {})
    if len(rows) == 1:          # the single entry point: the rows form of one query, every touched structure
        got = fd.count_query(ctx, ix, *rows[0], c.penalty, total_structures=c.total, as_array=True)
        assert got.tobytes() == mods[0][0].tobytes(), (c, first_id, "single")
        packed = all(int(x) < 1 << 27 for x in kept_fix[0]) and len(kept_fix[0]) < 1 << 18
        assert last_path(ctx) == ROWS | (PACKED if packed else 0), (c, first_id, "single", hex(last_path(ctx)))
    if c.via == "maps":
        which = {name: k for k, name in enumerate(dict.fromkeys(c.queries))}
        made = fq.make_query_maps(ctx, motif["qb"], [(0, motif["idx"][name], motif["subs"][name]) for name in which], ix, float(c.total))
        qms = [made[which[name]] for name in c.queries]
        for env in ENVS:
            for k in ("FDGPU_QT32", "FDGPU_QT_STREAM", "FDGPU_QTILE"):
                if k in env:
                    monkeypatch.setenv(k, env[k])
                else:
                    monkeypatch.delenv(k, raising=False)
            for n in ns:
                check(fd.count_query_maps(ctx, ix, qms, c.penalty, total_structures=c.total, top_n=n), n, "maps", env)
        for k in ("FDGPU_QT32", "FDGPU_QT_STREAM", "FDGPU_QTILE"):
            monkeypatch.delenv(k, raising=False)
    return seen, kept_fix


def claimed_forms(c, seen, kept_fix):
    """the forms the cases at a switch were built for, named one by one (expected_path above derives them; here they are pinned)"""
    n = c.top_ns[0]
    rows = max(len(f) for f in kept_fix)
    if c.via == "maps":
        d = seen[("maps", n, ())]
        if c.name == "near_wrap":
            assert d & SUMS32 and d & TILED and d & STREAM
        if c.name in ("exact_wrap", "zero_units"):
            assert d & TILED and not d & SUMS32
        if c.name in ("kept128", "mixed128"):
            assert rows == 128 and d & SUMS32
        if c.name in ("kept129", "mixed129"):
            assert rows == 129 and d & TILED and not d & SUMS32
        assert not seen[("maps", n, ("FDGPU_QT32",))] & SUMS32 and seen[("maps", n, ("FDGPU_QTILE",))] & ROWS
        assert not seen[("maps", n, ("FDGPU_QT32", "FDGPU_QT_STREAM"))] & STREAM
        assert not seen[("maps", 3073, ())] & (TILED | SLICED)
    d = seen[("batch", n, ())]
    if c.name == "rows1024":
        assert rows == 1024 and d & TILED and not d & ROWS
    if c.name == "rows1025":
        assert rows == 1025 and d & ROWS and not d & TILED
    if c.name == "rows4095":
        assert rows == 4095 and d & ROWS and not d & SLICED
    if c.name == "rows4096":
        assert rows == 4096 and d & SLICED and not d & (ROWS | TILED)
    if c.name == "total_2_33":
        assert not d & PACKED and d & ROWS
    elif c.cls != "width":
        assert d & PACKED
    if c.name.startswith("ties1075"):
        assert d & OVERFLOW
    if c.name.startswith(("ties1073", "ties1074")):
        assert d & TILED and not d & OVERFLOW
    assert seen[("batch", 0, ())] & ROWS and not seen[("batch", 3073, ())] & (TILED | SLICED)


@pytest.mark.parametrize("cls", sc.CLASSES)
@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_free_rows_equal_the_model(ctx, motif, first_id, cls, monkeypatch):
    cases = [c for c in _batch_cases(first_id) if c.cls == cls]
    assert cases
    for c in cases:
        seen, kept_fix = run_case(ctx, motif, c, first_id, monkeypatch)
        claimed_forms(c, seen, kept_fix)


@pytest.mark.parametrize("cls", [x for x in sc.CLASSES if x != "groups"])
@pytest.mark.parametrize("first_id", sc.FIRST_IDS)
def test_query_maps_equal_the_model(ctx, motif, first_id, cls, monkeypatch):
    cases = [c for c in sc.map_cases(first_id, motif["slots"][1]) if c.cls == cls]
    assert cases
    for c in cases:
        seen, kept_fix = run_case(ctx, motif, c, first_id, monkeypatch)
        claimed_forms(c, seen, kept_fix)


def test_path_flags_before_any_count_call():
    import folddisco_amd as fd
    c = fd.Context(0)
    try:
        assert last_path(c) == 0
        assert c.L.fdgpu_debug_last_count_path(c.h, None) != 0
    finally:
        c.close()
