"""CPU: the column offsets of the MSD build's mask table (csrc/fd_pair_mask_cols.h: wi_col, one u64 per work item, made once per batch by
fd_build_work_items), compiled for the host with -fsanitize=undefined,address (tools/check_pair_mask_cols.cpp) and compared with a numpy
restatement: a work item is one 64-residue tile of a structure, meets the partners from its first residue to the structure's end, and owns one
column per partner, padded to whole blocks of 64."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    e = str(tmp_path_factory.mktemp("maskcols") / "check_pair_mask_cols")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined",
                           "tools/check_pair_mask_cols.cpp", "-o", e], cwd=ROOT)
    return e


def restate(lengths):
    """wi_col of a batch of structures of these lengths: [work items + 1] first columns, the last entry = the number of columns"""
    cols = []
    for R in lengths:
        for t in range(0, R, 64):
            cols.append(-(-(R - t) // 64) * 64)
    return np.concatenate([[0], np.cumsum(np.asarray(cols, dtype=object))]) if cols else np.array([0], dtype=object)


def _run(exe, lengths):
    out = subprocess.run([exe], input="".join("%d\n" % r for r in lengths), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    head = lines[0].split()
    return int(head[1]), int(head[3]), [int(x) for x in lines[1:] if x]


def test_offsets_equal_the_restatement_at_the_block_edges(exe):
    """lengths 0, 1, 2, 63, 64, 65, 127, 128, 129, 4,200 and 65,535 mixed in one batch, each twice and in two orders: every offset, the number of
    work items, and the last offset = the sum of the padded columns"""
    base = [0, 1, 2, 63, 64, 65, 127, 128, 129, 4200, 65535]
    for lengths in (base, base[::-1], base + base[::-1], [0, 0, 5, 0], []):
        W, total, col = _run(exe, lengths)
        want = restate(lengths)
        assert W == len(want) - 1 == sum(-(-r // 64) for r in lengths)
        assert col == [int(x) for x in want], lengths
        assert total == col[-1] == sum(int(b) - int(a) for a, b in zip(col, col[1:]))
        assert all((b - a) % 64 == 0 and b > a for a, b in zip(col, col[1:]))      # whole blocks, and every work item owns at least one
    # one structure, by hand: 130 residues -> tiles at 0, 64, 128 meet 130, 66, 2 partners -> 192, 128, 64 columns
    assert _run(exe, [130])[2] == [0, 192, 320, 384]


def test_nothing_wraps_at_32_bits(exe):
    """128 structures of 65,535 residues: 131,072 work items and more than 2^32 columns (arithmetic only, no table of that size)"""
    out = subprocess.run([exe, "--big", "128", "65535"], capture_output=True, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stdout + out.stderr[-2000:]
    f = out.stdout.split()
    total, per, tiles = int(f[1]), int(f[3]), int(f[5])
    want = sum(-(-(65535 - t) // 64) * 64 for t in range(0, 65535, 64))
    assert per == want == 33587200 and tiles == 128 * 1024
    assert total == 128 * want and total > 1 << 32
