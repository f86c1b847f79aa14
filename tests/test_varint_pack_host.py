"""CPU: fd_varint_pack (csrc/fd_postings.h), the branch-free register form of a LEB128 varint that the posting encoder appends to its
accumulator, compiled for the host with -fsanitize=undefined and compared with the byte-wise writer fd_put_varint (tools/check_varint_pack.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_varint_pack_equals_the_bytewise_writer_under_ubsan(tmp_path):
    """every v < 2^22, every power of 128 +- 1, 2^32 - 1 and 2^24 random values of all lengths: same bytes, zero above them; a shift by the
    operand's width (the likely mistake in the continuation mask) aborts the program"""
    exe = str(tmp_path / "check_varint_pack")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-Itools/host_hip",
                           "tools/check_varint_pack.cpp", "-o", exe], cwd=ROOT)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "mismatches: 0" in out.stdout and "runtime error" not in out.stderr
    n = int(out.stdout.split("checked ")[1].split()[0])
    assert n >= (1 << 22) + (1 << 24)
