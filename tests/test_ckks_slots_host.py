"""CKKS slot encoding on the host side (no GPU): the numpy restatement of the reference's slot maps (tests/ckks_ref.py)
against the definitions, and PAlgebra's slot order (ith_rep) in helib_amd.hostnt and include/helib_amd_keys.hpp."""
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from helib_amd import hostnt

from tests import ckks_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("m", [16, 32, 64, 128, 256, 512, 1024])
def test_restatement_is_the_direct_evaluation(m):
    """v[m/4-1-i] = f(zeta^-T[i]): the FFT form of CKKS_canonicalEmbedding against an O(n^2) evaluation"""
    rng = np.random.default_rng(m)
    f = rng.uniform(-1, 1, size=(2, m // 2))
    got, want = R.canonical_embedding(f, m), R.direct_embedding(f, m)
    assert np.max(np.abs(got - want)) < 1e-11 * max(1.0, np.max(np.abs(want)))


@pytest.mark.parametrize("m", [16, 64, 1024, 16384])
def test_decode_of_encode_within_the_reference_bound(m):
    """decode(encode(v)) = v up to the rounding: |embedding(round(x)) - embedding(x)|/scale <= err/scale with err the
    reference's encodeRoundingError (src/EaCx.cpp:264-278: noiseBoundForUniform(0.5, phi(m)))"""
    rng = np.random.default_rng(m + 1)
    n = m // 4
    v = rng.uniform(-1, 1, size=(3, n)) + 1j * rng.uniform(-1, 1, size=(3, n))
    scale = 2.0 ** 20
    f = R.embed_in_slots(v, m, scale)
    back = R.canonical_embedding(f.astype(np.float64), m) / scale
    # noiseBoundForUniform(0.5, phi(m)) = scale(=10) * sqrt(phi(m) * 0.25/3)  (src/Context.h)
    err = 10.0 * math.sqrt(m // 2 * 0.25 / 3.0)
    assert np.max(np.abs(back - v)) <= err / scale
    # and unrounded, the two maps are inverse to each other
    x = R.embed_unrounded(v, m, scale)
    assert np.max(np.abs(R.canonical_embedding(x, m) / scale - v)) < 1e-9


def test_fewer_values_than_slots_fill_zeros():
    m = 64
    v = np.arange(1, 6) + 0.5j
    full = np.zeros(m // 4, dtype=np.complex128)
    full[:5] = v
    assert np.array_equal(R.embed_in_slots(v, m, 2.0 ** 10), R.embed_in_slots(full, m, 2.0 ** 10))


def _construction(z):
    """src/PAlgebra.cpp:520-570: exponent vectors over gens in lexicographic order, t = prod g_i^e_i mod m"""
    out = []
    for e in itertools.product(*[range(d) for d in z.ords]):
        t = 1
        for g, k in zip(z.gens, e):
            t = t * pow(g, k, z.m) % z.m
        out.append(t)
    return out


@pytest.mark.parametrize("m", [2 ** k for k in range(4, 18)])
def test_ith_rep_python_follows_the_construction(m):
    z = R.zmstar(m)
    T = z.reps()
    assert len(T) == z.getNSlots() == m // 4
    assert T == _construction(z)
    # one representative per class {t, -t} of Z_m^*; the single generator 3 (what the device tables assume)
    assert sorted(set(T) | {m - t for t in T}) == list(range(1, m, 2))
    assert z.gens == [3] and T == [pow(3, i, m) for i in range(m // 4)]


def test_ith_rep_on_a_two_generator_quotient():
    z = hostnt.ZmStar(21845, 2)   # BGV-style quotient with several generators: the order is still lexicographic
    T = [z.ith_rep(i) for i in range(z.getNSlots())]
    assert T == _construction(z) and len(set(T)) == len(T)
    with pytest.raises(ValueError):
        z.ith_rep(z.getNSlots())


def test_ith_rep_cpp_equals_python(tmp_path):
    exe = str(tmp_path / "ckks_reps_test")
    # ZmStar is header-only: no library to link
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ckks_reps_test.cpp"), "-o", exe])
    for k in range(4, 18):
        m = 2 ** k
        got = [int(x) for x in subprocess.check_output([exe, str(m)]).split()]
        assert got == R.zmstar(m).reps(), m


def test_capi_declares_the_slot_entry_points():
    from helib_amd import capi
    for s in ("hx_ckks_encode", "hx_ckks_embed", "hx_ckks_decode"):
        assert s in capi.SYMBOLS


def test_encrypted_array_refuses_bgv_and_non_power_of_two():
    from helib_amd import capi, ckks

    class Cc:
        ckks, m = False, 1024
    with pytest.raises(ckks.LogicError, match="bad args to CKKS_canonicalEmbedding"):
        ckks.EncryptedArrayCx(Cc(), None)
    Cc.ckks, Cc.m = True, 21845
    with pytest.raises(capi.InvalidArgument, match="only supports m as a power of two"):
        ckks.EncryptedArrayCx(Cc(), None)
