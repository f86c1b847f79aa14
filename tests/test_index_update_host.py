"""Host side of the index update (`python -m folddisco_amd update`), no GPU: the .lookup / .type rewrite helpers and the command's
validation, which runs before any device call."""
import os

import numpy as np
import pytest

from folddisco_amd import indexio

TIDS = ["a1", "b2", "c3", "d4", "e5"]
NRES = np.array([120, 0, 77, 4031, 9], np.uint64)
PLDDT = np.array([0.0, 0.0, 91.25, 47.123, 100.0], np.float32)


def _write_index(prefix, db_keys=None, fczdb=False):
    indexio.save_lookup_py(prefix + ".lookup", TIDS, NRES, PLDDT, db_keys)
    kw = dict(input_format="FCZDB", foldcomp_db="some/db") if fczdb else {}
    indexio.save_type(prefix + ".type", len(TIDS), grid_width=15.5, nbin_dist=8, nbin_angle=3, hash_type="FolddiscoAngle", multiple_bins=[(8, 32), (4, 12)], **kw)
    for ext in ("", ".offset"):
        open(prefix + ext, "wb").write(b"\x00" * 16)


@pytest.mark.parametrize("fczdb", [False, True])
def test_lookup_rewrite_keep_all_is_identity(tmp_path, fczdb):
    pre = str(tmp_path / "ix")
    _write_index(pre, db_keys=np.array([40, 7, 1000, 3, 12], np.uint64) if fczdb else None, fczdb=fczdb)
    rows = indexio.read_lookup_rows(pre + ".lookup")
    out = indexio.update_lookup_rows(rows, np.ones(len(rows), bool), keep_db_keys=fczdb)
    assert "".join(out).encode() == open(pre + ".lookup", "rb").read()
    txt = open(pre + ".type").read()
    assert indexio.update_type_text(txt, len(TIDS)) == txt


def test_lookup_rewrite_renumbers_file_built_rows(tmp_path):
    pre = str(tmp_path / "ix")
    _write_index(pre)
    rows = indexio.read_lookup_rows(pre + ".lookup")
    keep = np.array([True, False, True, False, True])
    out = [r.rstrip("\n").split("\t") for r in indexio.update_lookup_rows(rows, keep, keep_db_keys=False)]
    old = [r.rstrip("\n").split("\t") for r in rows]
    assert [r[0] for r in out] == ["0", "1", "2"] and [r[4] for r in out] == ["0", "1", "2"]
    assert [r[1:4] for r in out] == [old[k][1:4] for k in (0, 2, 4)]          # tid, nres, plddt verbatim
    # appended rows continue the numbering in the library writer's format
    add = indexio.lookup_rows(3, ["x9", "y8"], np.array([5, 6], np.uint64), np.array([1.5, 70.0], np.float32))
    assert add == ["3\tx9\t5\t1.5\t3\n", "4\ty8\t6\t70\t4\n"]
    p2 = str(tmp_path / "lib.lookup")
    tids = [old[k][1] for k in (0, 2, 4)] + ["x9", "y8"]
    indexio.save_lookup(p2, tids, np.r_[NRES[[0, 2, 4]], [5, 6]].astype(np.uint64), np.r_[PLDDT[[0, 2, 4]], [1.5, 70.0]].astype(np.float32))
    assert open(p2).read() == "".join("\t".join(r) + "\n" for r in out) + "".join(add)


def test_lookup_rewrite_keeps_foldcomp_db_keys(tmp_path):
    pre = str(tmp_path / "ix")
    _write_index(pre, db_keys=np.array([40, 7, 1000, 3, 12], np.uint64), fczdb=True)
    rows = indexio.read_lookup_rows(pre + ".lookup")
    out = [r.rstrip("\n").split("\t") for r in indexio.update_lookup_rows(rows, np.array([False, True, True, False, True]), keep_db_keys=True)]
    assert [r[0] for r in out] == ["0", "1", "2"] and [r[4] for r in out] == ["7", "1000", "12"]


def test_type_rewrite_changes_chunk_size_only(tmp_path):
    pre = str(tmp_path / "ix")
    _write_index(pre, fczdb=True)
    txt = open(pre + ".type").read()
    new = indexio.update_type_text(txt, 3)
    a, b = txt.splitlines(), new.splitlines()
    assert len(a) == len(b) and [k for k in range(len(a)) if a[k] != b[k]] == [0] and b[0] == "chunk_size = 3"
    cfg = indexio.load_type(pre + ".type")
    cfg2 = dict(cfg, chunk_size=3)
    open(pre + ".type", "w").write(new)
    assert indexio.load_type(pre + ".type") == cfg2


@pytest.fixture
def no_device(monkeypatch):
    import folddisco_amd as fd

    def boom(*a, **k):
        raise AssertionError("a device was touched before the update's validation ended")
    monkeypatch.setattr(fd, "Context", boom)


def _exit_status(argv):
    from folddisco_amd.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(argv)
    return e.value.code


def test_update_validation_before_any_device_call(tmp_path, no_device):
    pre = str(tmp_path / "ix")
    _write_index(pre)
    before = [open(pre + ext, "rb").read() for ext in ("", ".offset", ".lookup", ".type")]
    gone = tmp_path / "gone.txt"
    gone.write_text("b2\n" + "".join(f"zz{k}\n" for k in range(12)))
    code = _exit_status(["update", "-i", pre, "--remove", str(gone)])
    assert isinstance(code, str) and "zz0" in code and "zz9" in code and "zz10" not in code      # exit status 1, the first ten listed
    gone.write_text("\n".join(TIDS) + "\n")
    assert "every structure" in _exit_status(["update", "-i", pre, "--remove", str(gone)])
    assert "-p" in _exit_status(["update", "-i", pre])
    (tmp_path / "empty").mkdir()
    assert "no structures" in _exit_status(["update", "-i", pre, "-p", str(tmp_path / "empty")])
    assert "not found" in _exit_status(["update", "-i", str(tmp_path / "nope"), "-p", str(tmp_path / "empty")])
    assert [open(pre + ext, "rb").read() for ext in ("", ".offset", ".lookup", ".type")] == before
    fc = str(tmp_path / "fc")
    _write_index(fc, db_keys=np.arange(5, dtype=np.uint64), fczdb=True)
    (tmp_path / "add").mkdir()
    open(tmp_path / "add" / "x.pdb", "w").write("END\n")
    assert "Foldcomp" in _exit_status(["update", "-i", fc, "-p", str(tmp_path / "add")])
    assert not [f for f in os.listdir(tmp_path) if "update-tmp" in f]
