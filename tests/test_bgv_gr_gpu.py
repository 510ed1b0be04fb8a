"""Galois-ring slots on the device (hx_bgv_gf_create_pr, helib_amd.bgv_gr) against the literal CRT of
tests/intraslot_ref.py where that restatement is quick, and against the CPU-built tables evaluated in python integers
(tests/bgv_gr_tables.TableEncoder) at the largest admitted degree; bgv_pr's integer kernels as an independent witness for
constants; homomorphic operations with real keys.  Everything here is an integer: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_gr_tables as T
from tests import bgv_pr_ref as PR
from tests import intraslot_ref as IR

pytestmark = pytest.mark.gpu


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


def _ctx(hx, m, nprimes=2, bits=60):
    g = hostnt.PrimeGen(bits, m)
    c = hx.Context(m)
    for _ in range(nprimes):
        c.add_prime(g.next())
    return c


def _words(hx, c, idx, coeffs):
    """the device's own forward transform of given coefficients"""
    res = np.stack([np.mod(coeffs, np.int64(c.primes[i])).astype(np.uint64) for i in idx])
    return hx.DoubleCRT(c, list(idx), coeffs.shape[0], res).FFT().download()


# (85, 2, 4): d = 8, 8 slots; (13, 3, 2): odd p; (641, 2, 2): d = 64 = ord_641(2), the largest admitted degree, 10
# slots, phi = 640: the window and the fold cross two 256-coefficient tile edges with a 63-word halo.  The literal CRT is
# the reference for the first two; at d = 64 its Hensel lifting in python integers takes several seconds, so here the
# reference is the CPU-built tables in exact integers, which tests/test_bgv_gr_host.py checks against the literal CRT at
# this very ring (test_tables_at_the_largest_degree_against_the_literal_crt), beside the round trip and the product below.
@pytest.mark.parametrize("m,p,r", [(85, 2, 4), (13, 3, 2), (641, 2, 2)])
def test_encode_embed_decode_every_word(hx, m, p, r):
    from helib_amd import bgv_gr, ctxt as hc
    enc = T.TableEncoder(m, p, r)
    P, n, d, N = enc.P, enc.n, enc.d, enc.phim
    lit = IR.tables(m, p, r) if d < 64 else None
    c = _ctx(hx, m, 2)
    t = hx.BgvGf(c, p, r)
    assert (t.d, t.nslots, t.gens, t.ords, t.G, t.p, t.prime, t.r) == (d, n, enc.t["gens"], enc.t["ords"], enc.G, P, p, r)
    if lit is not None:
        assert t.G == lit.G
    rr, mod = C.c_int(), C.c_uint64()
    assert hx.lib().hx_bgv_gf_space(t.h, C.byref(rr), C.byref(mod)) == 0 and (rr.value, mod.value) == (r, P)
    rng = np.random.default_rng(m + r)
    for B, idx, mul in ((1, [0, 1], 1), (3, [], P + 3), (17, [1], 2 * P + 1)):
        a = rng.integers(-3 * P, 5 * P, size=(B, n, d))            # signed and out of range
        a[0, 0] = -1
        a[B - 1] = P - 1
        want = enc.coeffs(a % P, mul)
        if lit is not None:
            assert np.array_equal(want, lit.encode(a, mul))
        dd, cf = hx.bgvGfEncode(t, a, idx, mul, coeffs=True)
        assert np.array_equal(cf, want)
        if idx:
            assert np.array_equal(dd.download(), _words(hx, c, idx, want))
        f = rng.integers(-2 ** 40, 2 ** 40, size=(B, N))
        assert np.array_equal(hx.bgvGfEmbed(t, f), enc.slots(f))
        if lit is not None:
            assert np.array_equal(hx.bgvGfEmbed(t, f[:1]), lit.decode(f[:1]))
        assert np.array_equal(hx.bgvGfEmbed(t, want), a % P * (mul % P) % P)            # a scalar scales every slot
        assert np.array_equal(hx.bgvGfEmbed(t, hx.bgvGfEncode(t, a, [], 1, coeffs=True)[1]), a % P)
        small = rng.integers(-1000, 1000, size=(B, N))
        res = np.stack([np.mod(small, np.int64(c.primes[i])).astype(np.uint64) for i in (0, 1)])
        acc = hx.DoubleCRT(c, [0, 1], B, res).FFT()
        finv = 5 % P if P > 2 else 1
        assert np.array_equal(hx.bgvGfDecode(t, acc, finv), enc.slots(small * finv))
    # every slot is the same ring: the product of two encodings mod (Phi_m, p^r) decodes to the slot-wise product
    cc = hc.ChainContext(m, p, r, bits=100, c=2)
    ea = bgv_gr.EncryptedArray(cc, None, encoder=enc)
    a, b = rng.integers(0, P, size=(2, 2, n, d))
    ha, hb = (hx.bgvGfEncode(t, v, [], 1, coeffs=True)[1] for v in (a, b))
    phi = [int(x) for x in hostnt.phimx(m)]
    prod = [PR.mulmod([int(x) for x in ha[k]], [int(x) for x in hb[k]], phi, P) for k in range(2)]
    prod = np.array([row + [0] * (N - len(row)) for row in prod], dtype=np.int64)
    assert np.array_equal(hx.bgvGfEmbed(t, prod), ea.mulPlain(a, b))
    # constants: the words of the integer kernels modulo p^r
    crt = hx.BgvCrt(c, p, r)
    k = rng.integers(-4, P + 4, size=(17, n))
    d1, c1 = hx.bgvGfEncode(t, k, [1, 0], 1, coeffs=True)
    d0, c0 = hx.bgvCrtEncode(crt, k, [1, 0], 1, coeffs=True)
    assert np.array_equal(c1, c0) and np.array_equal(d1.download(), d0.download())
    got = hx.bgvGfEmbed(t, c0)
    assert np.array_equal(got[:, :, 0], k % P) and not np.any(got[:, :, 1:])


def test_r1_is_hx_bgv_gf_create(hx):
    m, p = 85, 2
    c = _ctx(hx, m, 2)
    t1, t2 = hx.BgvGf(c, p), hx.BgvGf(c, p, 1)
    h = C.c_void_p()
    assert hx.lib().hx_bgv_gf_create_pr(c.h, p, 1, C.byref(h)) == 0
    rr, mod = C.c_int(), C.c_uint64()
    assert hx.lib().hx_bgv_gf_space(h, C.byref(rr), C.byref(mod)) == 0 and (rr.value, mod.value) == (1, 2)
    hx.lib().hx_bgv_gf_destroy(h)
    a = np.random.default_rng(0).integers(0, 2, size=(3, 8, 8))
    x1, y1 = hx.bgvGfEncode(t1, a, [0, 1], 1, coeffs=True)
    x2, y2 = hx.bgvGfEncode(t2, a, [0, 1], 1, coeffs=True)
    assert np.array_equal(y1, y2) and np.array_equal(x1.download(), x2.download()) and t1.table_bytes == t2.table_bytes


def test_refusals(hx):
    from helib_amd import bgv_gr, ckks, ctxt as hc
    c = _ctx(hx, 13, 2)
    h = C.c_void_p()
    L = hx.lib()
    assert L.hx_bgv_gf_create_pr(c.h, 3, 0, C.byref(h)) == hx.HX_ERR_INVALID
    assert L.hx_bgv_gf_create_pr(c.h, 3, 20, C.byref(h)) == hx.HX_ERR_UNSUPPORTED and b"2^31" in L.hx_last_error()
    assert L.hx_bgv_gf_create_pr(c.h, 13, 2, C.byref(h)) == hx.HX_ERR_INVALID          # p | m
    assert L.hx_bgv_gf_create_pr(c.h, 9, 2, C.byref(h)) == hx.HX_ERR_INVALID           # not a prime
    assert L.hx_bgv_gf_space(None, None, None) == hx.HX_ERR_INVALID
    with pytest.raises(hx.HxError, match="130.*64") as e:                              # ord_131(2) = 130 > 64
        hx.BgvGf(_ctx(hx, 131, 1), 2, 2)
    assert e.value.code == hx.HX_ERR_UNSUPPORTED
    # a matrix over a table with r > 1 is refused in the library as well
    t = hx.BgvGf(c, 3, 2)
    with pytest.raises(hx.HxError, match="r > 1") as e:
        hx.BgvGfMatrix(t, np.zeros((1, 4, 4, 3), dtype=np.uint32), np.zeros(4, dtype=np.int32), np.arange(4, dtype=np.int32))
    assert e.value.code == hx.HX_ERR_UNSUPPORTED
    cc = hc.ChainContext(13, 3, 2, bits=100, c=2)
    ea = bgv_gr.EncryptedArray(cc, c)
    with pytest.raises(ckks.LogicError, match="FindRoots"):
        bgv_gr.EncryptedArray(cc, c, G=[x % 3 for x in ea.getG()])
    assert bgv_gr.EncryptedArray(cc, c, G=ea.getG()).getG() == IR.tables(13, 3, 2).G


# ---- homomorphic operations with real keys: bits = 300, the chain the existing Frobenius tests use at m = 85 ----
@pytest.mark.parametrize("m,p,r", [(85, 2, 4), (13, 3, 2)])
def test_homomorphic_operations_on_galois_ring_slots(hx, m, p, r):
    from helib_amd import bgv_gr, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, r, bits=300, c=3)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=5)
    sk.GenSecKey()
    ea = bgv_gr.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    hk.addFrbMatrices(sk)
    B, n, d, P = 3, ea.size(), ea.getDegree(), p ** r
    rng = np.random.default_rng(m)
    a, b = rng.integers(0, P, size=(2, B, n, d))
    a[0] = 0
    a[0, 0, 1 % d] = 1                                          # the slot X
    ca, cb = ea.encrypt_batch(sk, a), ea.encrypt_batch(sk, b)
    assert np.array_equal(ea.decrypt_batch(ca, sk), a)
    prod = ca.clone()
    prod.multiplyBy(cb)
    assert prod.isCorrect() and np.array_equal(ea.decrypt_batch(prod, sk), ea.mulPlain(a, b))
    one = ea.encrypt(sk, b[:1])
    ea.multByConstant(one, ea.encodePtxt(a[1:2]))
    ea.addConstant(one, ea.encodePtxt(b[2:3]))
    assert np.array_equal(ea.decrypt(one, sk), (ea.mulPlain(b[:1], a[1:2]) + b[2:3])[0] % P)
    rot = cb.clone()
    ea.rotate(rot, 3)
    assert np.array_equal(ea.decrypt_batch(rot, sk), np.roll(b, 3, axis=1))
    tot = cb.clone()
    ea.totalSums(tot)
    assert np.array_equal(ea.decrypt_batch(tot, sk), np.broadcast_to(b.sum(axis=1, keepdims=True) % P, b.shape))
    for j in (1, d - 1, d):
        fr = cb.clone()
        ea.frobeniusAutomorph(fr, j)
        assert np.array_equal(ea.decrypt_batch(fr, sk), ea.frobeniusPlain(b, j)), j
    # a ciphertext at p^(r-1), decoded through the p^r tables
    low = ea.encrypt_batch(sk, b * p % P)
    low.divideByP()
    assert low.ptxtSpace == P // p and np.array_equal(ea.decrypt_batch(low, sk), b % (P // p))
