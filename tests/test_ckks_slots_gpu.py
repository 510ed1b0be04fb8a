"""CKKS slot encoding and decoding on the device (hx_ckks_encode / hx_ckks_embed / hx_ckks_decode, helib_amd.ckks)
against the numpy restatement of the reference's maps (tests/ckks_ref.py), the oracle's transforms and the host's
DecryptCKKS path."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import ckks_ref as R

pytestmark = pytest.mark.gpu

MS = [16, 64, 1024, 16384, 32768, 65536, 131072]


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


def _ctx(hx, m, nprimes=3):
    g = O.PrimeGen(60, m)
    primes = [g.next() for _ in range(nprimes)]
    o, c = O.Ctx(m), hx.Context(m)
    for q in primes:
        i = o.add_prime(q)
        c.add_prime(q, o.roots[i])
    return c, o, primes


def _rand_slots(rng, B, n):
    return rng.uniform(-1, 1, size=(B, n)) + 1j * rng.uniform(-1, 1, size=(B, n))


@pytest.mark.parametrize("m,B", [(m, b) for m in MS for b in (1, 3)] + [(65536, 64)])
def test_encode_matches_the_restatement_and_the_oracle_transform(hx, m, B):
    c, o, primes = _ctx(hx, m, 3 if B < 64 else 1)
    rng = np.random.default_rng(m + B)
    v = _rand_slots(rng, B, m // 4)
    scale = 2.0 ** 30
    idx = list(range(len(primes)))
    d, cf = hx.ckksEncode(c, v, scale, idx, coeffs=True)
    x = R.embed_unrounded(v, m, scale)
    want = R.round_away(x).astype(np.int64)
    near_half = np.abs(np.abs(x - np.trunc(x)) - 0.5) < 1e-6
    diff = cf != want
    print(f"m={m} B={B}: {int(near_half.sum())} coefficients within 1e-6 of a half, {int(diff.sum())} differ")
    assert not (diff & ~near_half).any()
    assert np.max(np.abs(cf - want)) <= 1
    rows = d.download()
    for b in range(min(B, 3)):
        res = np.stack([np.mod(cf[b], np.int64(q)).astype(np.uint64) for q in primes])
        assert np.array_equal(rows[:, b], o.fft(idx, res))


@pytest.mark.parametrize("scaling,want", [(2.5, 3), (-2.5, -3), (0.5, 1), (-0.5, -1), (1.5, 2), (0.25, 0)])
def test_encode_rounds_halves_away_from_zero(hx, scaling, want):
    """std::round in CKKS_embedInSlots: every slot 1 encodes the constant polynomial `scaling` (the transform of an
    all-ones vector is exact in floating point), so f_0 lands exactly on a half and every other coefficient on 0"""
    m = 1024
    c, _, _ = _ctx(hx, m, 1)
    _, cf = hx.ckksEncode(c, np.ones((1, m // 4)), scaling, [0], coeffs=True)
    assert cf[0, 0] == want and not cf[0, 1:].any()


def test_encode_with_fewer_values_and_zero_scaling_edge(hx):
    m = 1024
    c, _, _ = _ctx(hx, m, 1)
    v = _rand_slots(np.random.default_rng(1), 2, 37)
    _, cf = hx.ckksEncode(c, v, 2.0 ** 20, [0], coeffs=True)
    assert np.array_equal(cf, R.embed_in_slots(v, m, 2.0 ** 20))
    _, cf0 = hx.ckksEncode(c, v, 0.0, [0], coeffs=True)
    assert not cf0.any()


@pytest.mark.parametrize("m", MS)
def test_embed_matches_the_restatement(hx, m):
    c, _, _ = _ctx(hx, m, 1)
    rng = np.random.default_rng(m)
    f = rng.uniform(-1e6, 1e6, size=(3, m // 2))
    got, want = hx.ckksEmbed(c, f), R.canonical_embedding(f, m)
    assert np.max(np.abs(got - want)) <= 1e-11 * np.max(np.abs(want))


def test_errors(hx):
    from helib_amd import ckks
    from helib_amd import ctxt as hc
    c, _, _ = _ctx(hx, 1024, 1)
    with pytest.raises(hx.HxError, match="overflow in encoding"):
        hx.ckksEncode(c, np.ones((1, 256)), 2.0 ** 70, [0])
    big = hx.Context(1 << 18)
    with pytest.raises(hx.HxError) as e:
        hx.ckksEmbed(big, np.zeros((1, 1 << 17)))
    assert e.value.code == hx.HX_ERR_UNSUPPORTED
    odd = hx.Context(21845)
    with pytest.raises(hx.InvalidArgument, match="only supports m as a power of two"):
        hx.ckksEmbed(odd, np.zeros((1, odd.phim)))
    bgv = hc.ChainContext(1024, 257, 1, bits=60, c=2)
    with pytest.raises(ckks.LogicError, match="bad args to CKKS_canonicalEmbedding"):
        ckks.EncryptedArrayCx(bgv, c)


def _chain(hx, m, bits, precision=20, seed=5, autos=()):
    from helib_amd import ckks, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, -1, precision, bits=bits, c=3, ckks=True)
    g = hx.Context(m)
    o = O.Ctx(m)
    for q in cc.primes:
        i = o.add_prime(q)
        g.add_prime(q, o.roots[i])
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey(maxDegKswitch=2)
    for k in autos:
        sk.GenKeySWmatrix(1, k)
    return cc, g, sk, ckks.EncryptedArrayCx(cc, g)


@pytest.mark.parametrize("m,bits", [(1024, 300), (65536, 1400)])
def test_decode_of_a_product_matches_host_decrypt(hx, m, bits):
    """hx_ckks_decode of a real CKKS product = host decryption (big-integer CRT / ratFactor) + the embedding; at
    bits = 1400 the 24-prime Garner kernel"""
    from helib_amd import ckks
    cc, g, sk, ea = _chain(hx, m, bits)
    rng = np.random.default_rng(2)
    a, b = _rand_slots(rng, 1, m // 4), _rand_slots(rng, 1, m // 4)
    ca, cb = ea.encrypt(sk, a), ea.encrypt(sk, b)
    ca.multiplyBy(cb)
    got = hx.ckksDecode(ckks.innerProduct(sk, ca), ca.lnRatFactor)
    raw = sk.Decrypt(ca)
    f = np.array([float(v) for v in raw]) / math.exp(ca.lnRatFactor)
    want = R.canonical_embedding(f, m)
    assert np.max(np.abs(got - want)) <= 1e-11 * np.max(np.abs(want))
    assert np.max(np.abs(got - a * b)) <= ckks.errorBound(ca)


@pytest.mark.parametrize("m,bits,B", [(1024, 300, 3), (65536, 440, 4), (65536, 1400, 64)])
def test_encrypt_multiply_decrypt_slotwise(hx, m, bits, B):
    from helib_amd import ckks
    cc, g, sk, ea = _chain(hx, m, bits)
    rng = np.random.default_rng(bits + B)
    a, b = _rand_slots(rng, B, m // 4) / math.sqrt(2), _rand_slots(rng, B, m // 4) / math.sqrt(2)
    ca, cb = ea.encrypt_batch(sk, a), ea.encrypt_batch(sk, b)
    s = ca.clone()
    s += cb
    got = ea.rawDecrypt_batch(s, sk)
    assert np.max(np.abs(got - (a + b))) <= ckks.errorBound(s)
    ca.multiplyBy(cb)
    got = ea.rawDecrypt_batch(ca, sk)
    err = np.max(np.abs(got - a * b))
    print(f"m={m} bits={bits} B={B}: max slot error {err:.3e}, errorBound {ckks.errorBound(ca):.3e}")
    assert err <= ckks.errorBound(ca)
    if B > 1:
        return
    # multByConstantCKKS with an encoded constant vector
    k = _rand_slots(rng, 1, m // 4) / math.sqrt(2)
    dk, fk = ea.encode(k, 1.0, idx=sorted(ca.primeSet))
    ca.multByConstantCKKS(dk, 1.0, fk, cc.encodeRoundingError())
    got = ea.rawDecrypt_batch(ca, sk)
    assert np.max(np.abs(got - a * b * k)) <= ckks.errorBound(ca)


def test_batch_of_one_equals_single_encryption(hx):
    from helib_amd import keys as hk
    m = 1024
    cc, g, sk, ea = _chain(hx, m, 300)
    v = _rand_slots(np.random.default_rng(3), 1, m // 4)
    d, f = ea.encode(v)
    sk1 = hk.SecKey(cc, hk.HxBackend(g, cc), seed=99)
    sk2 = hk.SecKey(cc, hk.HxBackend(g, cc), seed=99)
    for s in (sk1, sk2):
        s.pubEncrKey, s.pubEncrKeyNoise, s.skBounds = sk.pubEncrKey, sk.pubEncrKeyNoise, sk.skBounds
    c1 = sk1.CKKSencrypt(d, 1.0, f)
    c2 = sk2.CKKSencryptBatch(d, 1.0, f)
    assert c1.lnRatFactor == c2.lnRatFactor
    for h in ("1", "s"):
        assert np.array_equal(c1.parts[h].download(), c2.parts[h].download())


def test_automorphisms_rotate_and_conjugate_slots(hx):
    from helib_amd import ckks, ctxt as hc
    m = 1024
    T = R.reps(m)
    cc, g, sk, ea = _chain(hx, m, 300, autos=(int(T[1]), m - 1))
    v = _rand_slots(np.random.default_rng(4), 1, m // 4) / 2
    ct = ea.encrypt(sk, v)
    r = ct.clone()
    r.smartAutomorph(int(T[1]))
    got = ea.rawDecrypt(r, sk)
    assert np.max(np.abs(got - np.roll(v[0], 1))) <= ckks.errorBound(r)
    # the hoisted result stays on the ctxt and special primes, scaled by their product P (BasicAutomorphPrecon,
    # src/matmul.cpp:48-184: the caller mod-switches down): decoded with ratFactor * P
    h = hc.BasicAutomorphPrecon(ct).automorph(int(T[1]))
    lnP = cc.logOfProduct(list(cc.specialPrimes))
    hv = hx.ckksDecode(ckks.innerProduct(sk, h), ct.lnRatFactor + lnP)[0]
    assert np.max(np.abs(hv - got)) <= 2 * ckks.errorBound(r)
    c = ct.clone()
    c.smartAutomorph(m - 1)
    assert np.max(np.abs(ea.rawDecrypt(c, sk) - np.conj(v[0]))) <= ckks.errorBound(c)


@pytest.mark.parametrize("vmax,size", [(0.25, -1.0), (3.0, -1.0), (3.0, 4.0)])
def test_encrypt_passes_the_callers_size_to_CKKSencrypt(hx, vmax, size):
    """include/helib/EncryptedArray.h:1252-1266: the encoding factor comes from the values (or the given size), the
    size given by the caller goes to CKKSencrypt unchanged -- the default -1 means ptxtSize = 1 there:
    ratFactor = f * ef, ef = ceil(errorBound * 2^r / (f * ptxtSize)), ptxtMag = roundedSize(ptxtSize)"""
    from helib_amd import ckks
    m = 1024
    cc, g, sk, ea = _chain(hx, m, 300)
    v = _rand_slots(np.random.default_rng(6), 2, m // 4)
    v *= vmax / np.max(np.abs(v))
    ct = ea.encrypt_batch(sk, v, size)
    f = cc.encodeScalingFactor() / (vmax if size < 0 else size)
    ptxtSize = 1.0 if size <= 0 else size
    ef = math.ceil(math.exp(ct.lnNoise) * (1 << cc.r) / (f * ptxtSize))
    assert abs(ct.lnRatFactor - math.log(f * max(ef, 1))) < 1e-12
    assert ct.ptxtMag == (1.0 if ptxtSize <= 1 else float(1 << (math.ceil(ptxtSize) - 1).bit_length()))
    assert np.max(np.abs(ea.rawDecrypt_batch(ct, sk) - v)) <= ckks.errorBound(ct)


def _hip_free_bytes():
    import ctypes as C
    try:
        fn = C.CDLL(None).hipMemGetInfo   # the process's HIP runtime (loaded globally with torch's copy)
    except AttributeError:
        import torch
        return torch.cuda.mem_get_info()[0]
    free, total = C.c_size_t(), C.c_size_t()
    assert fn(C.byref(free), C.byref(total)) == 0
    return free.value


def test_slot_state_is_released_with_the_context(hx):
    """the slot unit's tables and buffers (about 40 MB per context at m = 65536, batch 64) go with the context:
    device memory does not grow over repeated create / encode / destroy"""
    m, B = 65536, 64
    v = _rand_slots(np.random.default_rng(7), B, m // 4)

    def once():
        c, _, _ = _ctx(hx, m, 1)
        d = hx.ckksEncode(c, v, 2.0 ** 20, [0])
        hx.ckksEmbed(c, np.zeros((B, m // 2)))
        d.close()
        c.close()
    once()
    before = _hip_free_bytes()
    for _ in range(8):
        once()
    assert before - _hip_free_bytes() < 96 << 20      # 8 leaked states would be > 300 MB


def _vectors(n, B, s):
    i = np.arange(n)
    return np.stack([0.5 * np.cos(s * i + 1.1 * b) + 0.5j * np.sin(0.23 * i + s * b) for b in range(B)])


@pytest.mark.parametrize("m,bits,B", [(1024, 300, 3), (65536, 440, 2)])
def test_cpp_encrypted_array_agrees_with_the_python_class(hx, m, bits, B, tmp_path):
    """include/helib_amd_ckks.hpp from C++ (tests/cpp/ckks_test.cpp, self-checking: encryptBatch -> multiplyBy ->
    rawDecryptBatch within errorBound, encode / decode, both rawDecrypt forms, CKKSencryptBatch at B = 1 equal word
    for word to CKKSencrypt, LogicError("overflow in encoding")); its decoded product agrees with the python class's
    on the same inputs"""
    import os
    import subprocess
    from helib_amd import ckks
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, out = str(tmp_path / "ckks_test"), str(tmp_path / "prod.bin")
    libdir = os.path.join(root, "helib_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "ckks_test.cpp"), "-L" + libdir, "-lhelib_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    r = subprocess.run([exe, str(m), str(bits), str(B), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ckks_test OK" in r.stdout, r.stdout + r.stderr
    cpp_bound = float(r.stdout.split("errorBound ")[1].split()[0])
    got_cpp = np.fromfile(out, dtype=np.float64).view(np.complex128).reshape(B, m // 4)
    cc, g, sk, ea = _chain(hx, m, bits, seed=31)
    a, b = _vectors(m // 4, B, 0.37), _vectors(m // 4, B, 0.61)
    ca, cb = ea.encrypt_batch(sk, a), ea.encrypt_batch(sk, b)
    ca.multiplyBy(cb)
    got_py = ea.rawDecrypt_batch(ca, sk)
    assert np.max(np.abs(got_py - a * b)) <= ckks.errorBound(ca)
    assert np.max(np.abs(got_cpp - got_py)) <= cpp_bound + ckks.errorBound(ca)
