"""CPU: the posting encoder's rule for one element of a constant tile (csrc/fd_postings.h: fd_const_classify, fd_delta_len), compiled for the host
with -fsanitize=undefined,address and compared with the general rule on full hashes and ids (tools/check_enc_const.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constant_tile_rule_equals_the_general_rule_under_ubsan_and_asan(tmp_path):
    """every pair of neighbouring key words over the top bytes {0, 1, 0x7f, 0xfe, 0xff} and the local ids at and around every varint boundary
    below 2^24 (ids and deltas), 0 and 2^24 - 1, with four first ids up to 2^28 - 1 — the pairs whose top byte rises while the id falls among
    them — and 2^20 random pairs: same head, same value, same length; every delta below 2^24 and 2^20 random ones below 2^31: the length of
    fd_delta_len equals fd_varint_len's (0 for 0)"""
    exe = str(tmp_path / "check_enc_const")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined", "-Itools/host_hip",
                           "tools/check_enc_const.cpp", "-o", exe], cwd=ROOT)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "mismatches: 0" in out.stdout and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    n = int(out.stdout.split("checked ")[1].split()[0])
    assert n >= 4 * 100000
