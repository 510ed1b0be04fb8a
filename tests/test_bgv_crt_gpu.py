"""BGV slots for any d = ord_m(p) on the device (hx_bgv_crt_*, helib_amd.bgv_crt) against the polynomial restatement of
the reference's definitions (tests/bgv_crt_ref.py) and python big-integer sums.  Everything here is an integer: every
comparison is exact."""
import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_crt_ref as R

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


def _check_encode(hx, c, table, ref, a, mul, idx):
    """words (against the device's own forward transform of the reference coefficients) and the zzX"""
    want = ref.encode(a, mul)
    d, cf = hx.bgvCrtEncode(table, a, idx, mul, coeffs=True)
    assert np.array_equal(cf, want)
    if idx:
        res = np.stack([np.mod(want, np.int64(c.primes[i])).astype(np.uint64) for i in idx])
        assert np.array_equal(d.download(), hx.DoubleCRT(c, list(idx), want.shape[0], res).FFT().download())


# ---- (a) encode and decode ----
@pytest.mark.parametrize("m,p", [(51, 2), (85, 2), (105, 2), (31, 3)])
def test_encode_embed_decode_against_the_restatement(hx, m, p):
    ref = R.tables(m, p)
    c = _ctx(hx, m, 3)
    t = hx.BgvCrt(c, p)
    assert (t.d, t.nslots, t.gens, t.ords) == (ref.d, ref.nslots, ref.z.gens, ref.z.signedOrds())
    assert t.table_bytes == 2 * 4 * ref.nslots * ((ref.phim + 3) // 4 * 4)
    rng = np.random.default_rng(m)
    for B in (1, 3, 5):
        a = rng.integers(-3 * p, 5 * p, size=(B, ref.nslots))
        a[0, 0] = -1
        for idx, mul in (([0, 2], 1), ([], 1), ([1], p + 3 if p > 2 else 3)):
            _check_encode(hx, c, t, ref, a, mul, idx)
        f = rng.integers(-2 ** 40, 2 ** 40, size=(B, ref.phim))
        assert np.array_equal(hx.bgvCrtEmbed(t, f), ref.decode(f))
        assert np.array_equal(hx.bgvCrtEmbed(t, ref.encode(a)), a % p)
        # hx_bgv_crt_decode: a polynomial on two primes holding small coefficients, times factor_inv
        idx = [0, 1]
        small = rng.integers(-1000, 1000, size=(B, ref.phim))
        res = np.stack([np.mod(small, np.int64(c.primes[i])).astype(np.uint64) for i in idx])
        acc = hx.DoubleCRT(c, idx, B, res).FFT()
        finv = 2 % p if p > 2 else 1
        assert np.array_equal(hx.bgvCrtDecode(t, acc, finv), ref.decode(small * finv))
    short = hx.bgvCrtEncode(t, [[1]], [], coeffs=True)[1]
    assert np.array_equal(short, ref.encode([[1] + [0] * (ref.nslots - 1)]))


# ---- (b) lazy reduction: the smallest shape where a missed reduction overflows ----
def test_lazy_reduction_at_the_largest_prime(hx):
    m, p = 64, 2147483647
    ref = R.tables(m, p)
    assert (ref.nslots, ref.phim, (1 << 64) // (p * p)) == (16, 32, 4)
    c = _ctx(hx, m, 2)
    t = hx.BgvCrt(c, p)
    rng = np.random.default_rng(7)
    a = np.concatenate([np.full((1, 16), p - 1), rng.integers(0, p, size=(2, 16))])
    want = np.array([[sum(int(x) * e[k] for x, e in zip(row, ref.E)) % p for k in range(32)] for row in a], dtype=object)
    want = np.array([[int(v) - p if int(v) > p // 2 else int(v) for v in row] for row in want], dtype=np.int64)
    assert np.array_equal(hx.bgvCrtEncode(t, a, [], coeffs=True)[1], want)
    assert np.array_equal(want, ref.encode(a))
    f = np.concatenate([np.full((1, 32), p - 1), rng.integers(0, p, size=(2, 32))])
    assert np.array_equal(hx.bgvCrtEmbed(t, f), ref.decode(f))
    assert np.array_equal(hx.bgvCrtEmbed(t, want), a % p)


# ---- (c) d = 1: the existing path, word for word ----
def test_d1_equals_the_transform_path(hx):
    m, p, B = 1024, 12289, 3
    c = _ctx(hx, m, 2)
    t, old = hx.BgvCrt(c, p), hx.BgvSlots(c, p)
    assert (t.d, t.nslots, t.gens, t.ords) == (1, 512, old.gens, old.ords)
    rng = np.random.default_rng(1)
    a = rng.integers(-p, 2 * p, size=(B, 512))
    d1, c1 = hx.bgvCrtEncode(t, a, [0, 1], 77, coeffs=True)
    d0, c0 = hx.bgvEncode(old, a, [0, 1], 77, coeffs=True)
    assert np.array_equal(c1, c0) and np.array_equal(d1.download(), d0.download())
    f = rng.integers(-2 ** 50, 2 ** 50, size=(B, 512))
    assert np.array_equal(hx.bgvCrtEmbed(t, f), hx.bgvEmbed(old, f))


# ---- (d) tile edges: 30 slots, 300 coefficients ----
def test_tile_edges_at_a_middle_ring(hx):
    m, p = 341, 2
    ref = R.tables(m, p)
    assert (ref.phim, ref.d, ref.nslots) == (300, 10, 30)
    c = _ctx(hx, m, 2)
    t = hx.BgvCrt(c, p)
    rng = np.random.default_rng(3)
    a = rng.integers(-4, 5, size=(17, 30))      # two batch tiles, the second with one element
    _check_encode(hx, c, t, ref, a, 1, [1])
    f = rng.integers(-9, 9, size=(17, 300))
    assert np.array_equal(hx.bgvCrtEmbed(t, f), ref.decode(f))


# ---- (e) homomorphic operations ----
def _chain(hx, m, p, bits, seed=5):
    from helib_amd import bgv_crt, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, 1, bits=bits, c=3)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    ea = bgv_crt.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    return cc, g, sk, ea


def _roll(a, ea, i, k):
    shape = [ea.sizeOfDimension(j) for j in range(ea.dimension())]
    return np.roll(a.reshape(-1, *shape), k, axis=1 + i).reshape(a.shape)


@pytest.mark.parametrize("m,p,bits,orders", [(85, 2, 300, [-8]), (119, 2, 300, [2, -2])])
def test_homomorphic_operations_over_non_native_dimensions(hx, m, p, bits, orders):
    from helib_amd import ckks
    cc, g, sk, ea = _chain(hx, m, p, bits)
    ref = R.tables(m, p)
    assert ea.zMStar.signedOrds() == orders and (ea.size(), ea.getDegree()) == (ref.nslots, ref.d)
    B, n = 3, ea.size()
    rng = np.random.default_rng(m)
    a, b, c = rng.integers(0, p, size=(3, B, n))
    a[0, 0], a[0, 1:] = 1, 0
    ca, cb, cx = ea.encrypt_batch(sk, a), ea.encrypt_batch(sk, b), ea.encrypt_batch(sk, c)
    assert np.array_equal(ea.decrypt_batch(ca, sk), a)
    prod = ca.clone()
    prod.multiplyBy(cb)
    prod += cx
    assert np.array_equal(ea.decrypt_batch(prod, sk), (a * b + c) % p)
    e = ea.encodePtxt(b[:1])
    one = ea.encrypt(sk, a[0])
    ea.multByConstant(one, e)
    assert np.array_equal(ea.decrypt(one, sk), a[0] * b[0] % p)
    ea.addConstant(one, ea.encodePtxt(c[:1]))
    assert np.array_equal(ea.decrypt(one, sk), (a[0] * b[0] + c[0]) % p)
    for i in range(ea.dimension()):
        for k in (1, 3, -1):
            ct = ca.clone()
            ea.rotate1D(ct, i, k)
            assert np.array_equal(ea.decrypt_batch(ct, sk), _roll(a, ea, i, k)), (i, k)
        ct = ca.clone()
        ea.shift1D(ct, i, 1)
        assert np.array_equal(ea.decrypt_batch(ct, sk), _roll(a, ea, i, 1) * (ea._coords(i) >= 1)), i
        if not ea.nativeDimension(i):           # lnNoise: the reference's sequence written out
            ord_, z = ea.sizeOfDimension(i), ea.zMStar
            got = ca.clone()
            ea.rotate1D(got, i, 1)
            ct = ca.clone()
            ct.smartAutomorph(z.genToPow(i, 1))
            T = ct.clone()
            T.smartAutomorph(z.genToPow(i, -ord_))
            m1, sz = ea._encodedMask(ea.maskSlots(i, 1), set(ct.primeSet) | set(T.primeSet))
            ct.multByConstant(m1, sz)
            ct += T
            T.multByConstant(m1, sz)
            ct -= T
            assert got.lnNoise == ct.lnNoise and got.primeSet == ct.primeSet
    with pytest.raises(ckks.LogicError, match="non-native"):
        ea.totalSums(ca.clone())


# ---- (f) errors ----
def test_refusals(hx):
    from helib_amd import bgv, ctxt as hc
    c = _ctx(hx, 85, 2)
    for p, code in ((2147483659, hx.HX_ERR_UNSUPPORTED), (5, hx.HX_ERR_INVALID), (15, hx.HX_ERR_INVALID)):
        with pytest.raises(hx.HxError) as e:
            hx.BgvCrt(c, p)
        assert e.value.code == code, p
    with pytest.raises(hx.HxError, match="only d = 1") as e:      # the base class still refuses d > 1
        bgv.EncryptedArray(hc.ChainContext(85, 2, 1, bits=100, c=2), c)
    assert e.value.code == hx.HX_ERR_UNSUPPORTED
    with pytest.raises(hx.HxError, match="only d = 1"):
        hx.BgvSlots(c, 2)
    t = hx.BgvCrt(c, 2)                                           # the device is untouched by the refusals
    assert np.array_equal(hx.bgvCrtEmbed(t, hx.bgvCrtEncode(t, [[1, 0, 1]], [], coeffs=True)[1])[0, :3], [1, 0, 1])
