"""Where a pool slot's cold path state lies in the arena (csrc/hip/rt_cold_layout.h), checked without a GPU: tests/cpp/cold_layout_host.cpp
is built with g++ against the header the kernel and the arena's allocation read, and run.  For every traversal 0-6 and pools of 128,
160 and 192 slots it checks that cold_index is injective over fields x slots and below pool_wave_cold_dwords; that the walks keep
field * pool + slot; and, for the flat kernel, that a slot's fields lie in [16 slot, 16 slot + 16), that each of the four groups
(T + last pdf, L + output slot, the NEE term, the remaining-triangle words) shares one 16-byte cell, and that a wave's block is a
multiple of 64 bytes.  The header's own static_asserts state the same facts, so compiling it is part of the test."""
import os
import subprocess

import util


def test_cold_layout_host_program(tmp_path):
    exe = str(tmp_path / "cold_layout_host")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(util.ROOT, "rsoderh-raytracing_amd", "csrc", "hip"),
           os.path.join(util.ROOT, "tests", "cpp", "cold_layout_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    # 7 traversals' fields (14, 14, 13, 14, 24, 41, 13) x (128 + 160 + 192) slots
    assert r.stdout.strip() == "cold layout ok: %d indices" % ((14 + 14 + 13 + 14 + 24 + 41 + 13) * 480)
