"""Which stage a wave of the pool kernel runs next (csrc/hip/rt_pool_pick.h: the maximum over (count << 3) | stage), checked without a
GPU: tests/cpp/pool_pick_host.cpp is built with g++ against the header the kernel reads, and run — a plain executable, once as it
is and once under the address and undefined-behaviour sanitizers.  It compares the pick with a transcription of the scan it replaces
(the fullest stage, ties to the later stage, none if all are empty, never GEN once the work is exhausted) for all count vectors in
{0, 1, 2, 63, 64, 65, 191, 192}^5 with both values of `exhausted`, and for 10^6 random vectors whose sum is at most 192."""
import os
import subprocess

import pytest

import util


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_pool_pick_host_program(tmp_path, sanitize):
    exe = str(tmp_path / "pool_pick_host")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(util.ROOT, "rsoderh-raytracing_amd", "csrc", "hip")]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd += [os.path.join(util.ROOT, "tests", "cpp", "pool_pick_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip() == "pool pick ok: %d vectors" % (2 * 8 ** 5 + 10 ** 6)
