"""rsrt_sincosf (include/rsrt_detmath.h), the fused sine and cosine of one angle the render kernels use, without a GPU: as bits against
the two functions it fuses (tests/cpp/sincos_host.cpp, a stand-alone program: every 37th of all 2^32 inputs, the octant borders, the range
check, the special values) and, through them, against the checker's statement of the contract (oracle.detmath)."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import util

F = np.float32
STRIDE, ULPS = 37, 4096


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """The program's exit status and its output: {set: (checked, mismatches, first failing pattern)}."""
    exe = str(tmp_path_factory.mktemp("sincos") / "sincos_host")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(util.ROOT, "include"),
           os.path.join(util.ROOT, "tests", "cpp", "sincos_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    sets = {}
    for line in r.stdout.splitlines():
        t = line.split()
        assert t[1] == "checked" and t[3] == "mismatches" and t[5] == "first", line
        sets[t[0]] = (int(t[2]), int(t[4]), int(t[6], 16))
    return r.returncode, sets


def test_fused_form_has_the_bits_of_sin_and_cos(report):
    rc, sets = report
    # what the strides give: an empty loop cannot pass
    want = {"stride37": -(-(1 << 32) // STRIDE),                       # 0, 37, 74, ... below 2^32
            "octants": 2 * (ULPS + 1) + 64 * 2 * (2 * ULPS + 1),      # k = 0: +-0 and the 4096 patterns above either; k = 1 .. 64: both signs
            "range": 2 * (2 * ULPS + 1),
            "special": 20}
    assert {k: v[0] for k, v in sets.items()} == want
    for name, (checked, bad, first) in sets.items():
        assert bad == 0, (name, bad, "first failing input %08x" % first)
    assert rc == 0


def test_fused_form_equals_the_checkers_statement(tmp_path):
    """10^4 angles — the integrator's ranges (0 .. 2 pi, -pi .. pi) and the whole accepted range — through the header's rsrt_sincosf
    against oracle.detmath("sin" / "cos", x), the checker's statement of the contract, as uint32."""
    import ctypes as C
    src = tmp_path / "w.cpp"
    src.write_text('#include "rsrt_detmath.h"\nextern "C" void sc(const float *x, int n, float *s, float *c) { for (int i = 0; i < n; i++) rsrt_sincosf(x[i], s + i, c + i); }\n')
    so = str(tmp_path / "libw.so")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(util.ROOT, "include"), str(src), "-o", so],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    L = C.CDLL(so)
    L.sc.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(12)
    xs = np.concatenate([rng.uniform(0.0, 2.0 * np.pi, 4000), rng.uniform(-np.pi, np.pi, 4000), rng.uniform(-8192.0, 8192.0, 2000)]).astype(F)
    s, c = np.zeros_like(xs), np.zeros_like(xs)
    L.sc(xs.ctypes.data, len(xs), s.ctypes.data, c.ctypes.data)
    want_s = np.array([oracle.detmath("sin", float(x)) for x in xs], F)
    want_c = np.array([oracle.detmath("cos", float(x)) for x in xs], F)
    assert len(xs) == 10 ** 4 and np.array_equal(util.bits(s), util.bits(want_s)) and np.array_equal(util.bits(c), util.bits(want_c))
