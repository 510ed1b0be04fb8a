"""include/helib_amd_ckks.hpp between slots, from C++ (tests/cpp/linalg_test.cpp, self-checking: rotate, shift, totalSums,
runningSums, extractRealPart, extractImPart within errorBound of the plaintext maps; hx_mul_add_many called directly
against the sequence it replaces, and its error returns); its decoded rotation agrees with the python class's."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hx():
    try:
        import torch  # noqa: F401   (before this library touches the device: see test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import capi
    if capi.device_count() <= 0:
        pytest.skip("no HIP device: the GPU tests run on an MI355X (pytest -m gpu)")
    return capi


def _vectors(n, B, s):
    i = np.arange(n)
    return np.stack([0.5 * np.cos(s * i + 1.1 * b) + 0.5j * np.sin(0.23 * i + s * b) for b in range(B)])


@pytest.mark.parametrize("m,bits,B", [(256, 300, 1), (1024, 300, 3)])
def test_cpp_slot_methods_and_mul_add_many(hx, m, bits, B, tmp_path):
    from helib_amd import ckks, ctxt as hc, keys as hk
    from tests import ckks_linalg_ref as L
    exe, out = str(tmp_path / "linalg_test"), str(tmp_path / "rot.bin")
    libdir = os.path.join(ROOT, "helib_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "linalg_test.cpp"), "-L" + libdir, "-lhelib_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    r = subprocess.run([exe, str(m), str(bits), str(B), out], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and "linalg_test OK" in r.stdout, r.stdout + r.stderr
    cpp_bound = float(r.stdout.split("errorBound ")[-1].split()[0])
    got_cpp = np.fromfile(out, dtype=np.float64).view(np.complex128).reshape(B, m // 4)
    cc = hc.ChainContext(m, -1, 20, bits=bits, c=3, ckks=True)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=31)
    sk.GenSecKey(maxDegKswitch=2)
    hk.add1DMatrices(sk)
    ea = ckks.EncryptedArrayCx(cc, g)
    a = _vectors(m // 4, B, 0.37)
    ct = ea.encrypt_batch(sk, a)
    ea.rotate(ct, 1)
    got_py = ea.rawDecrypt_batch(ct, sk)
    want = np.stack([L.rotate(x, 1) for x in a])
    assert np.max(np.abs(got_py - want)) <= ckks.errorBound(ct)
    assert np.max(np.abs(got_cpp - want)) <= cpp_bound
    assert np.max(np.abs(got_cpp - got_py)) <= cpp_bound + ckks.errorBound(ct)
