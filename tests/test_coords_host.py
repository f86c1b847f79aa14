"""Host side of the coordinate store (PREFIX.coords: indexio.CoordStore / write_coords, `python -m folddisco_amd coords`), no GPU: the file
round-trips the ingest's arrays byte for byte, slices and gathers equal numpy's, pieces written through write_coords equal the direct write, every
refusal of the reader is reached, and the commands that use a store refuse before a device is opened."""
import functools
import os
import shutil

import numpy as np
import pytest

from folddisco_amd import indexio, structure
from tests.helpers import SER

SECTIONS = ("res_off", "n_xyz", "ca_xyz", "cb_xyz", "aa", "cb_valid", "resname_std", "chain", "serial")


def _status(argv):
    from folddisco_amd.__main__ import main
    try:
        main(argv)
    except SystemExit as e:
        return 1 if isinstance(e.code, str) else (e.code or 0)
    return 0


@pytest.fixture
def no_device(monkeypatch):
    import folddisco_amd as fd

    def boom(*a, **k):
        raise AssertionError("a device was touched by a host-side command or before its validation ended")
    monkeypatch.setattr(fd, "Context", boom)


def _write_index(prefix, paths, value=b""):
    """index files that are consistent with each other over the given structure files (tids = their paths); no posting is ever decoded here"""
    n = len(paths)
    indexio.save_lookup_py(prefix + ".lookup", paths, np.arange(n, dtype=np.uint64) + 10, np.full(n, 50.0, np.float32))
    indexio.save_type(prefix + ".type", n)
    if value:
        indexio.write_index_files(prefix, np.frombuffer(value, np.uint8), np.array([7], np.uint32), np.array([0, len(value)], np.uint64))
    else:
        indexio.write_index_files(prefix, np.zeros(0, np.uint8), np.zeros(0, np.uint32), np.zeros(1, np.uint64))


def _make_store(tmp, name, paths, value=b""):
    pre = os.path.join(str(tmp), name)
    _write_index(pre, paths, value)
    assert _status(["coords", "-i", pre, "--chunk", "2"]) == 0      # 5 structures in chunks of 2: the chunk seams are inside the data
    return pre


@functools.lru_cache(maxsize=None)
def _reference():
    """the serine peptidases through the per-structure ingest, once per process; callers leave it unchanged"""
    structs, ok = structure.read_compact_structures(SER, threads=2)
    assert ok.all() and len(structs) == 5
    return structs


def _flat(structs):
    off = np.zeros(len(structs) + 1, np.uint64)
    off[1:] = np.cumsum([s.n for s in structs])
    cat = lambda f, dt, w=None: np.concatenate([np.asarray(f(s), dt).reshape((-1, w) if w else (-1,)) for s in structs])
    return dict(res_off=off, n_xyz=cat(lambda s: s.n_xyz, np.float32, 3), ca_xyz=cat(lambda s: s.ca_xyz, np.float32, 3),
                cb_xyz=cat(lambda s: s.cb_xyz, np.float32, 3), aa=cat(lambda s: s.aa, np.uint8), cb_valid=cat(lambda s: s.cb_ok, np.uint8),
                resname_std=cat(lambda s: s.resname_std(), np.uint8), chain=cat(lambda s: s.chain, np.uint8), serial=cat(lambda s: s.serial, np.uint64))


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype.itemsize == b.dtype.itemsize and a.shape == b.shape and a.tobytes() == b.tobytes()


def _arrays_of(ca: indexio.CoordArrays):
    ps = ca.ps
    return dict(res_off=ps.res_off, n_xyz=ps.n_xyz, ca_xyz=ps.ca_xyz, cb_xyz=ps.cb_xyz, aa=ps.aa, cb_valid=ps.cb_valid, resname_std=ca.resname_std,
                chain=ca.chain, serial=ca.serial)


def test_store_round_trips_the_ingest_byte_for_byte(tmp_path):
    pre = _make_store(tmp_path, "ix", SER)
    st = indexio.CoordStore.open(pre + ".coords", check_prefix=pre)
    want = _flat(_reference())
    assert st.n_struct == 5 and st.n_res == int(want["res_off"][-1]) and st.flags == 1
    assert st.stamp == (5, 0, 16) == indexio.index_stamp(pre)
    for name in SECTIONS:
        assert _same_bytes(getattr(st, name), want[name]), name
    # the layout the header implies: 64-byte header, every section on a 64-byte boundary, nothing behind the last
    raw = open(pre + ".coords", "rb").read()
    assert raw[:8] == b"FDCOORD1" and np.frombuffer(raw[8:16], "<u4").tolist() == [1, 1]
    assert np.frombuffer(raw[16:56], "<u8").tolist() == [5, st.n_res, 5, 0, 16] and raw[56:64] == b"\0" * 8
    pos = 64
    for name, dt, per in indexio.COORDS_SECTIONS:
        n = (6 if per is None else per * st.n_res) * np.dtype(dt).itemsize
        assert pos % 64 == 0 and raw[pos:pos + n] == np.ascontiguousarray(want[name]).tobytes(), name
        pos += n
        if name != "serial":
            assert raw[pos:(pos + 63) & ~63] == b"\0" * (((pos + 63) & ~63) - pos)
            pos = (pos + 63) & ~63
    assert pos == len(raw)


def test_read_packed_labels_are_those_of_the_per_structure_ingest():
    out = structure.read_packed(SER, threads=2, labels=True)
    assert len(out) == 6 and len(structure.read_packed(SER, threads=2)) == 5
    want = _flat(_reference())
    for name in ("chain", "resname_std", "serial"):
        assert _same_bytes(out[5][name], want[name]), name


def test_slice_and_select_equal_numpy_gathers(tmp_path):
    st = indexio.CoordStore.open(_make_store(tmp_path, "ix", SER) + ".coords")
    ref = _reference()
    for lo, hi in ((0, 5), (1, 4), (2, 2), (4, 5), (0, 0), (5, 5)):
        got, want = _arrays_of(st.slice(lo, hi)), _flat(ref[lo:hi]) if hi > lo else None
        if want is None:
            assert got["res_off"].tolist() == [0] and all(len(got[n]) == 0 for n in SECTIONS[1:])
            continue
        for name in SECTIONS:
            assert _same_bytes(got[name], want[name]), (lo, hi, name)
    for ids in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [3, 0, 4], [2, 2, 2, 0], [4], []):
        got = _arrays_of(st.select(np.array(ids, np.int64)))
        if not ids:
            assert got["res_off"].tolist() == [0] and all(len(got[n]) == 0 for n in SECTIONS[1:])
            continue
        want = _flat([ref[k] for k in ids])
        for name in SECTIONS:
            assert _same_bytes(got[name], want[name]), (ids, name)
    with pytest.raises(IndexError):
        st.select([5])
    with pytest.raises(IndexError):
        st.slice(3, 6)


def test_lazy_sequence_gives_the_labels_of_compact_structure(tmp_path):
    st = indexio.CoordStore.open(_make_store(tmp_path, "ix", SER) + ".coords")
    ref = _reference()
    for lo, hi in ((0, 5), (1, 4)):
        seq = st.structs(lo, hi)
        assert len(seq) == hi - lo and bool(seq)
        assert _same_bytes(seq.resname_std_all(), np.concatenate([s.resname_std() for s in ref[lo:hi]]))
        for k in range(hi - lo):
            t, s = seq[k], ref[lo + k]
            assert t.n == s.n and _same_bytes(t.ca_xyz, s.ca_xyz)
            assert [f"{chr(int(t.chain[x]))}{int(t.serial[x])}" for x in range(t.n)] == [f"{chr(int(s.chain[x]))}{int(s.serial[x])}" for x in range(s.n)]
        with pytest.raises(IndexError):
            seq[hi - lo]
    assert len(st.structs(2, 2)) == 0 and not st.structs(2, 2) and len(st.structs(2, 2).resname_std_all()) == 0


@pytest.mark.parametrize("case", ["reorder", "remove", "join"])
def test_write_coords_over_pieces_equals_the_direct_write(tmp_path, case):
    a = _make_store(tmp_path, "a", SER)
    sa = indexio.CoordStore.open(a + ".coords", check_prefix=a)
    out = str(tmp_path / "out")
    if case == "reorder":
        ids = np.array([3, 0, 4, 1, 2])
        want = _make_store(tmp_path, "w", [SER[k] for k in ids])
        pieces = [(sa, ids)]
    elif case == "remove":
        ids = np.array([0, 2, 3])
        want = _make_store(tmp_path, "w", [SER[k] for k in ids])
        pieces = [(sa, ids)]
    else:
        b = _make_store(tmp_path, "b", SER[3:] + SER[:1])
        sb = indexio.CoordStore.open(b + ".coords", check_prefix=b)
        want = _make_store(tmp_path, "w", SER + SER[3:] + SER[:1])
        pieces = [(sa, None), (sb, None)]
    indexio.write_coords(out + ".coords", iter(pieces), indexio.index_stamp(want))
    assert open(out + ".coords", "rb").read() == open(want + ".coords", "rb").read()
    assert not any(".tmp" in f for f in os.listdir(tmp_path))      # no temporary file stays
    # raw arrays as a piece: the same bytes again
    wst = indexio.CoordStore.open(want + ".coords")
    indexio.write_coords(out + "2.coords", [wst.slice(0, 1), wst.slice(1, wst.n_struct)], lambda: indexio.index_stamp(want))
    assert open(out + "2.coords", "rb").read() == open(want + ".coords", "rb").read()


def test_pieces_without_cb_valid_contribute_ones_or_no_section(tmp_path):
    from folddisco_amd.api import PackedStructures
    st = indexio.CoordStore.open(_make_store(tmp_path, "ix", SER) + ".coords")
    full = st.slice(0, 2)
    bare = indexio.CoordArrays(PackedStructures(full.ps.res_off, full.ps.n_xyz, full.ps.ca_xyz, full.ps.cb_xyz, full.ps.aa, None), full.chain, full.resname_std,
                               full.serial)
    p = str(tmp_path / "m.coords")
    indexio.write_coords(p, [full, bare], (4, 0, 16))
    m = indexio.CoordStore.open(p)
    n = int(full.ps.res_off[-1])
    assert m.flags == 1 and _same_bytes(m.cb_valid[:n], full.ps.cb_valid) and (np.asarray(m.cb_valid[n:]) == 1).all()
    indexio.write_coords(p, [bare], (2, 0, 16))
    m = indexio.CoordStore.open(p)
    assert m.flags == 0 and m.cb_valid is None and m.slice(0, 2).ps.cb_valid is None and _same_bytes(m.serial, full.serial)


# ---- refusals of the reader, one at a time
def _patched(tmp_path, edit):
    pre = _make_store(tmp_path, "ix", SER)
    raw = bytearray(open(pre + ".coords", "rb").read())
    raw = edit(raw)
    open(pre + ".coords", "wb").write(bytes(raw))
    return pre


def _set_u64(raw, pos, v):
    raw[pos:pos + 8] = np.array([v], "<u8").tobytes()
    return raw


@pytest.mark.parametrize("name,edit,word", [
    ("truncated", lambda r: r[:-1], "truncated"),
    ("header_only", lambda r: r[:40], "shorter than"),
    ("trailing_byte", lambda r: r + b"\0", "trailing"),
    ("res_off_descends", lambda r: _set_u64(r, 64 + 8 * 2, int(np.frombuffer(bytes(r[64 + 8:64 + 16]), "<u8")[0]) - 1), "ascend"),
    ("res_off_first", lambda r: _set_u64(r, 64, 1), "res_off[0]"),
    ("res_off_last", lambda r: _set_u64(r, 64 + 8 * 5, int(np.frombuffer(bytes(r[24:32]), "<u8")[0]) - 1), "res_off[5]"),
    ("magic", lambda r: b"FDCOORD2" + r[8:], "magic"),
    ("version", lambda r: r[:8] + np.array([2], "<u4").tobytes() + r[12:], "version"),
    ("flags", lambda r: r[:12] + np.array([3], "<u4").tobytes() + r[16:], "flag"),
])
def test_reader_refuses_an_inconsistent_store(tmp_path, name, edit, word):
    pre = _patched(tmp_path, edit)
    with pytest.raises(indexio.CoordStoreError) as e:
        indexio.CoordStore.open(pre + ".coords")
    assert word in str(e.value), str(e.value)


@pytest.mark.parametrize("field", [0, 1, 2])
def test_reader_refuses_a_stamp_that_is_off_by_one(tmp_path, field):
    pre = _patched(tmp_path, lambda r: _set_u64(r, 32 + 8 * field, int(np.frombuffer(bytes(r[32 + 8 * field:40 + 8 * field]), "<u8")[0]) + 1))
    indexio.CoordStore.open(pre + ".coords")                     # sound in itself
    with pytest.raises(indexio.CoordStoreError) as e:
        indexio.CoordStore.open(pre + ".coords", check_prefix=pre)
    assert indexio.STAMP_FIELDS[field] in str(e.value)
    assert not any(f in str(e.value) for k, f in enumerate(indexio.STAMP_FIELDS) if k != field)      # the message names the field that mismatches


# ---- the commands
def test_coords_refuses_a_missing_structure_file_and_writes_nothing(tmp_path, capsys, no_device):
    pre = str(tmp_path / "ix")
    _write_index(pre, SER[:2] + [str(tmp_path / f"gone{k}.pdb") for k in range(12)] + SER[2:])
    before = sorted(os.listdir(tmp_path))
    assert _status(["coords", "-i", pre]) == 1
    out = capsys.readouterr().out
    assert "12 of the 17" in out and out.count("gone") == 10 and "gone9.pdb" in out and "gone10.pdb" not in out and "..." in out
    assert sorted(os.listdir(tmp_path)) == before


def test_coords_statuses(tmp_path, capsys, no_device):
    pre = str(tmp_path / "ix")
    assert _status(["coords", "-i", pre]) == 2                   # no index there
    _write_index(pre, SER)
    indexio.save_type(pre + ".type", 4)                          # chunk_size disagrees with the rows of .lookup
    before = sorted(os.listdir(tmp_path))
    assert _status(["coords", "-i", pre]) == 1 and "inconsistent" in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path)) == before
    indexio.save_type(pre + ".type", 5)
    assert _status(["coords", "-i", pre, "-o", str(tmp_path / "elsewhere.bin"), "-t", "2"]) == 0
    assert "[OK]" in capsys.readouterr().out and not os.path.exists(pre + ".coords")
    indexio.CoordStore.open(str(tmp_path / "elsewhere.bin"), check_prefix=pre)
    # tids relative to the index's directory are found the way `query` finds them
    os.makedirs(tmp_path / "rel")
    for p in SER[:2]:
        shutil.copy(p, tmp_path / "rel")
    rel = str(tmp_path / "r")
    _write_index(rel, [os.path.join("rel", os.path.basename(p)) for p in SER[:2]])
    assert _status(["coords", "-i", rel]) == 0
    assert _same_bytes(indexio.CoordStore.open(rel + ".coords").serial, _flat(_reference()[:2])["serial"])


def test_a_skipped_structure_keeps_its_slot_with_no_residues(tmp_path, capsys, no_device):
    bad = str(tmp_path / "unreadable.pdb.gz")
    open(bad, "wb").write(b"this is not gzip")
    pre = _make_store(tmp_path, "ix", [SER[0], bad, SER[1]])
    st = indexio.CoordStore.open(pre + ".coords", check_prefix=pre)
    ref = _reference()
    assert st.n_struct == 3 and np.diff(np.asarray(st.res_off).astype(np.int64)).tolist() == [ref[0].n, 0, ref[1].n]
    assert st.structs()[1].n == 0


def _stale(tmp_path, name="ix"):
    """an index whose store was written before the index files changed: consistent files, a stamp that no longer matches"""
    pre = _make_store(tmp_path, name, SER)
    kept = str(tmp_path / "kept.coords")
    shutil.copy(pre + ".coords", kept)
    _write_index(pre, SER, value=b"\x01\x01\x01")
    assert not indexio.check_index_files(pre)
    return pre


def test_commands_refuse_a_stale_store_before_a_device_is_opened(tmp_path, capsys, no_device):
    pre = _stale(tmp_path)
    rm = str(tmp_path / "rm.txt")
    open(rm, "w").write(SER[1] + "\n")
    files = lambda: {f: os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)}
    before = files()
    for argv in (["update", "-i", pre, "--remove", rm], ["reorder", "-i", pre, "--by", "tid", "--desc"], ["reorder", "-i", pre, "--by", "tid", "--host"],
                 ["query", "-i", pre, "-p", SER[0], "-q", "A1"], ["verify", "-i", pre, "--host"]):
        assert _status(argv) == 1, argv
        out = capsys.readouterr().out
        assert "coordinate store refused" in out and "value file bytes" in out, (argv, out)
        assert files() == before
    # --no-coords does not look at the store: the query goes on to open the device
    with pytest.raises(AssertionError, match="a device was touched"):
        _status(["query", "-i", pre, "-p", SER[0], "-q", "A1", "--no-coords"])


def test_merge_refuses_when_only_some_inputs_have_a_store(tmp_path, capsys, no_device):
    a = _make_store(tmp_path, "a", SER[:3])
    b = str(tmp_path / "b")
    _write_index(b, SER[3:])
    before = sorted(os.listdir(tmp_path))
    for extra in ([], ["--host"]):
        assert _status(["merge", "-i", a, b, "-o", str(tmp_path / "m")] + extra) == 1
        out = capsys.readouterr().out
        assert "only some inputs have a coordinate store" in out and b in out.split("without one:")[1] and a not in out.split("without one:")[1]
    assert sorted(os.listdir(tmp_path)) == before


def test_index_coords_is_refused_under_several_ranks(tmp_path, capsys, monkeypatch, no_device):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    assert _status(["index", "-p", os.path.dirname(SER[0]), "-i", str(tmp_path / "ix"), "--coords"]) == 1
    assert "coords -i PREFIX" in capsys.readouterr().out
    assert os.listdir(tmp_path) == []


def test_verify_adds_one_line_for_a_store(tmp_path, capsys, no_device):
    pre = _make_store(tmp_path, "ix", SER)
    capsys.readouterr()
    assert _status(["verify", "-i", pre, "--host"]) == 0
    with_store = capsys.readouterr().out.splitlines()
    os.remove(pre + ".coords")
    assert _status(["verify", "-i", pre, "--host"]) == 0
    without = capsys.readouterr().out.splitlines()
    assert len(with_store) == len(without) + 1 and with_store[1:] == without and with_store[0].startswith(f"[OK] {pre}.coords: 5 structures")


def test_host_merge_and_reorder_carry_the_store(tmp_path, capsys, no_device):
    """`merge --host` and `reorder --host` open no device: the store they write equals the direct write over the structures in the result's order"""
    a, b = _make_store(tmp_path, "a", SER[:3]), _make_store(tmp_path, "b", SER[3:])
    m = str(tmp_path / "m")
    assert _status(["merge", "-i", b, a, "-o", m, "--host"]) == 0
    want = _make_store(tmp_path, "w", SER[3:] + SER[:3])
    assert open(m + ".coords", "rb").read() == open(want + ".coords", "rb").read()
    indexio.CoordStore.open(m + ".coords", check_prefix=m)
    assert _status(["reorder", "-i", m, "--by", "tid", "--host"]) == 0      # in place: the store is rewritten with the other files
    st = indexio.CoordStore.open(m + ".coords", check_prefix=m)
    order = np.argsort([os.path.basename(p) for p in SER[3:] + SER[:3]], kind="stable")
    assert [t.split("\t")[1] for t in open(m + ".lookup")] == [(SER[3:] + SER[:3])[k] for k in order]
    assert _same_bytes(st.serial, _flat([_reference()[(list(range(3, 5)) + list(range(3)))[k]] for k in order])["serial"])
    # no input has a store: none is written
    for p in (a, b):
        os.remove(p + ".coords")
    assert _status(["merge", "-i", a, b, "-o", str(tmp_path / "n"), "--host"]) == 0 and not os.path.exists(str(tmp_path / "n.coords"))
