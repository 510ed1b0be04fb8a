"""BGV slots modulo p^r on the device (hx_bgv_crt_create_pr, hx_scaled_sub, helib_amd.bgv_pr) against the Hensel-lifting
restatement tests/bgv_pr_ref.py, numpy and the unfused call sequences.  Everything here is an integer: every comparison
is exact."""
import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_pr_ref as R

pytestmark = pytest.mark.gpu
PMAX = 46337        # the largest prime whose square is below 2^31


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


# ---- (a) encode / embed / decode ----
@pytest.mark.parametrize("m,p,r,B", [(85, 2, 4, 17), (127, 2, 3, 17), (85, PMAX, 2, 3)])
def test_encode_embed_decode_against_the_restatement(hx, m, p, r, B):
    ref = R.tables(m, p, r)
    P = p ** r
    c = _ctx(hx, m, 3)
    t = hx.BgvCrt(c, p, r)
    assert (t.prime, t.r, t.p) == (p, r, P)
    assert (t.d, t.nslots, t.gens, t.ords) == (ref.d, ref.nslots, ref.z.gens, ref.z.signedOrds())
    rng = np.random.default_rng(m + r)
    a = rng.integers(-2 ** 63, 2 ** 63 - 1, size=(B, ref.nslots), endpoint=True)     # the whole int64 range
    a[0, :4] = [-1, P // 2, -(P // 2), P - 1][:min(4, ref.nslots)]
    for idx, mul in (([0, 2], 1), ([], 1), ([1], P - 3)):
        want = ref.encode(a, mul)
        d, cf = hx.bgvCrtEncode(t, a, idx, mul, coeffs=True)
        assert np.array_equal(cf, want)
        if idx:
            res = np.stack([np.mod(want, np.int64(c.primes[i])).astype(np.uint64) for i in idx])
            assert np.array_equal(d.download(), hx.DoubleCRT(c, list(idx), B, res).FFT().download())
    want = ref.encode(a)
    assert want.max() <= P // 2 and want.min() > -(P // 2) - (P & 1)          # balanced, +P/2 kept at an even modulus
    slots = np.array([[int(x) % P for x in row] for row in a], dtype=np.int64)
    assert np.array_equal(hx.bgvCrtEmbed(t, want), slots)
    f = rng.integers(-2 ** 63, 2 ** 63 - 1, size=(B, ref.phim), endpoint=True)
    assert np.array_equal(hx.bgvCrtEmbed(t, f), ref.decode(f))
    # hx_bgv_crt_decode: a polynomial on two primes holding small coefficients, times factor_inv
    small = rng.integers(-10 ** 6, 10 ** 6, size=(B, ref.phim))
    res = np.stack([np.mod(small, np.int64(c.primes[i])).astype(np.uint64) for i in (0, 1)])
    acc = hx.DoubleCRT(c, [0, 1], B, res).FFT()
    finv = P - 2
    assert np.array_equal(hx.bgvCrtDecode(t, acc, finv), ref.decode([[int(x) * finv for x in row] for row in small]))


def test_create_pr_refusals_and_r1(hx):
    c = _ctx(hx, 85, 2)
    for p, r, code in ((2, 0, hx.HX_ERR_INVALID), (2, -1, hx.HX_ERR_INVALID), (2, 31, hx.HX_ERR_UNSUPPORTED),
                       (46349, 2, hx.HX_ERR_UNSUPPORTED), (15, 2, hx.HX_ERR_INVALID), (5, 2, hx.HX_ERR_INVALID)):
        with pytest.raises(hx.HxError) as e:
            hx.BgvCrt(c, p, r)
        assert e.value.code == code, (p, r)
        if code == hx.HX_ERR_UNSUPPORTED:
            assert "2^31 = 2147483648" in str(e.value)
    with pytest.raises(hx.HxError) as e:
        hx.BgvCrt(c, 15)
    assert e.value.code == hx.HX_ERR_INVALID
    # r = 1 through the new entry is the old table: the same words out of both
    import ctypes as C
    h = C.c_void_p()
    assert hx.lib().hx_bgv_crt_create_pr(c.h, 2, 1, C.byref(h)) == 0
    old = hx.BgvCrt(c, 2)
    new = hx.BgvCrt.__new__(hx.BgvCrt)
    new.context, new.p, new.h, new.nslots = c, 2, h, old.nslots
    a = np.random.default_rng(0).integers(-5, 5, size=(3, old.nslots))
    d0, c0 = hx.bgvCrtEncode(old, a, [0, 1], 1, coeffs=True)
    d1, c1 = hx.bgvCrtEncode(new, a, [0, 1], 1, coeffs=True)
    assert np.array_equal(c0, c1) and np.array_equal(d0.download(), d1.download())
    new.close()


# ---- (b) hx_scaled_sub against the four calls ----
@pytest.mark.parametrize("m,phim", [(85, 64), (127, 126)])
def test_scaled_sub_is_bit_exact_against_the_four_calls(hx, m, phim):
    from helib_amd import ctxt as hc
    cc = hc.ChainContext(m, 2, 1, bits=200, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    assert g.phim == phim
    idx = list(range(len(cc.primes)))            # all chain primes as rows
    qs = [cc.primes[i] for i in idx]
    rng = np.random.default_rng(m)
    special = [0, 1, None]                       # None: q - 1
    for B in (1, 5):
        for parts in (1, 2):
            def rnd():
                return hx.DoubleCRT(g, idx, B, np.stack([rng.integers(0, q, size=(B, phim), dtype=np.uint64) for q in qs]))
            c, t = [rnd() for _ in range(parts)], [rnd() for _ in range(parts)]
            u = [int(rng.integers(0, q)) for q in qs]
            v = [int(rng.integers(0, q)) for q in qs]
            for k in range(min(3, len(qs))):     # 0, 1 and q - 1 in both lists, at different rows
                u[k] = qs[k] - 1 if special[k] is None else special[k]
                v[-1 - k] = qs[-1 - k] - 1 if special[k] is None else special[k]
            want = []
            for x, y in zip(c, t):
                w, y2 = x.copy(), y.copy()
                w.mulConstant(u)
                y2.mulConstant(v)
                w -= y2
                want.append(w.download())
            t_before = [y.download() for y in t]
            c_before = c[0].download()
            hx.scaledSub(c[0], c[1] if parts == 2 else None, t[0], t[1] if parts == 2 else None, u, v)
            for x, w in zip(c, want):
                assert np.array_equal(x.download(), w), (B, parts)
            for y, w in zip(t, t_before):
                assert np.array_equal(y.download(), w)
            # and against python integers: the last row of the first part
            q = qs[-1]
            py = (c_before[-1].astype(object) * u[-1] - t_before[0][-1].astype(object) * v[-1]) % q
            assert np.array_equal(c[0].download()[-1], py.astype(np.uint64))
    # a c that still shares its rows with t (a lazy copy): c takes its own copy, t stays
    t0 = hx.DoubleCRT(g, idx, 2, np.stack([rng.integers(0, q, size=(2, phim), dtype=np.uint64) for q in qs]))
    c0 = t0.copy()
    before = t0.download()
    hx.scaledSub(c0, None, t0, None, [3] * len(qs), [1] * len(qs))
    assert np.array_equal(t0.download(), before)
    assert np.array_equal(c0.download(), np.stack([(before[i].astype(object) * 2 % q).astype(np.uint64) for i, q in enumerate(qs)]))


def test_scaled_sub_refusals_touch_nothing(hx):
    import ctypes as C
    m = 85
    g = _ctx(hx, m, 3)
    other = _ctx(hx, m, 3)
    qs = g.primes
    rng = np.random.default_rng(1)

    def rnd(ctx=g, idx=(0, 1, 2), B=2):
        return hx.DoubleCRT(ctx, list(idx), B, np.stack([rng.integers(0, ctx.primes[i], size=(B, 64), dtype=np.uint64) for i in idx]))
    c0, c1, t0, t1 = rnd(), rnd(), rnd(), rnd()
    keep = [x.download() for x in (c0, c1, t0, t1)]
    ok = np.array([1, 2, 3], dtype=np.uint64)
    L = hx.lib()

    def call(a, b, c, d, u=ok, v=ok):
        def h(x):
            return x.h if x is not None else None
        return L.hx_scaled_sub(h(a), h(b), h(c), h(d), u.ctypes.data_as(C.c_void_p) if u is not None else None,
                               v.ctypes.data_as(C.c_void_p) if v is not None else None)
    INV = hx.HX_ERR_INVALID
    assert call(None, None, t0, None) == INV and call(c0, None, None, None) == INV
    assert call(c0, None, t0, None, u=None) == INV and call(c0, None, t0, None, v=None) == INV
    assert call(c0, c1, t0, None) == INV and b"go together" in L.hx_last_error()
    assert call(c0, None, t0, t1) == INV and b"go together" in L.hx_last_error()
    assert call(c0, None, c0, None) == INV and b"different polys" in L.hx_last_error()
    assert call(c0, c0, t0, t1) == INV and call(c0, c1, t0, t0) == INV and call(c0, c1, t0, c1) == INV
    assert call(c0, None, rnd(other), None) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(c0, None, rnd(B=3), None) == INV and b"batch or prime set" in L.hx_last_error()
    assert call(c0, None, rnd(idx=(0, 1)), None) == INV and call(c0, None, rnd(idx=(0, 2, 1)), None) == INV
    assert call(c0, c1, t0, rnd(B=1)) == INV
    big = np.array([1, qs[1], 3], dtype=np.uint64)
    assert call(c0, None, t0, None, u=big) == INV and b"not reduced" in L.hx_last_error()
    assert call(c0, None, t0, None, v=big) == INV
    with pytest.raises(hx.InvalidArgument, match="one u and one v per prime row"):
        hx.scaledSub(c0, None, t0, None, [1, 2], [1, 2, 3])
    for x, w in zip((c0, c1, t0, t1), keep):
        assert np.array_equal(x.download(), w)
    assert call(c0, c1, t0, t1) == 0             # and the state still works
    assert not np.array_equal(c0.download(), keep[0])


# ---- (c) homomorphic operations ----
def _chain(hx, m, p, r, bits, seed=5):
    from helib_amd import bgv_pr, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, r, bits=bits, c=3)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    ea = bgv_pr.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    return cc, g, sk, ea


def test_encrypt_multiply_add_decrypt_and_divide_by_p(hx):
    cc, g, sk, ea = _chain(hx, 85, 2, 4, 300)
    B, n, P = 3, ea.size(), 16
    rng = np.random.default_rng(85)
    a, b, c = rng.integers(0, P, size=(3, B, n))
    ca, cb, cx = ea.encrypt_batch(sk, a), ea.encrypt_batch(sk, b), ea.encrypt_batch(sk, c)
    assert ca.ptxtSpace == P and np.array_equal(ea.decrypt_batch(ca, sk), a)
    prod = ca.clone()
    prod.multiplyBy(cb)
    prod += cx
    assert np.array_equal(ea.decrypt_batch(prod, sk), (a * b + c) % P)
    one = ea.encrypt(sk, a[0])
    ea.multByConstant(one, ea.encodePtxt(b[:1]))
    ea.addConstant(one, ea.encodePtxt(c[:1]))
    assert np.array_equal(ea.decrypt(one, sk), (a[0] * b[0] + c[0]) % P)
    # divideByP on an encryption of 2 a: a mod 8
    dbl = ea.encrypt_batch(sk, 2 * a)
    dbl.divideByP()
    assert dbl.ptxtSpace == 8 and dbl.effectiveR() == 3
    assert np.array_equal(ea.decrypt_batch(dbl, sk), a % 8)
    dbl.multByP()
    assert dbl.ptxtSpace == 16 and np.array_equal(ea.decrypt_batch(dbl, sk), 2 * (a % 8))


def test_rotate_shift_total_sums(hx):
    cc, g, sk, ea = _chain(hx, 85, 2, 2, 300)
    B, n, P = 2, ea.size(), 4
    a = np.random.default_rng(4).integers(0, P, size=(B, n))
    ca = ea.encrypt_batch(sk, a)
    for k in (1, 3, -2):
        ct = ca.clone()
        ea.rotate(ct, k)
        assert np.array_equal(ea.decrypt_batch(ct, sk), np.roll(a, k, axis=1)), k
    ct = ca.clone()
    ea.shift(ct, 3)
    want = np.zeros_like(a)
    want[:, 3:] = a[:, :-3]
    assert np.array_equal(ea.decrypt_batch(ct, sk), want)
    ct = ca.clone()
    ea.totalSums(ct)
    assert np.array_equal(ea.decrypt_batch(ct, sk), np.repeat(a.sum(axis=1, keepdims=True) % P, n, axis=1))


def _words(ct):
    return {h: p.download() for h, p in ct.parts.items()}


def test_extract_digits_fused_and_unfused(hx):
    from helib_amd import bgv_pr
    cc, g, sk, ea = _chain(hx, 85, 2, 3, 300)
    B, n, P = 4, ea.size(), 8
    a = np.random.default_rng(9).integers(0, P, size=(B, n))
    a[0, :3] = [0, 7, 4]
    ct = ea.encrypt_batch(sk, a)
    fused = bgv_pr.extractDigits(ea, ct, fused=True)
    plain = bgv_pr.extractDigits(ea, ct, fused=False)
    assert len(fused) == len(plain) == 3
    for j, (x, y) in enumerate(zip(fused, plain)):
        assert (x.lnNoise, x.primeSet, x.ptxtSpace, x.intFactor) == (y.lnNoise, y.primeSet, y.ptxtSpace, y.intFactor)
        wx, wy = _words(x), _words(y)
        assert wx.keys() == wy.keys() and all(np.array_equal(wx[h], wy[h]) for h in wx)
        assert x.ptxtSpace == 2 ** (3 - j) and x.bitCapacity() > 0
        assert np.array_equal(ea.decrypt_batch(x, sk), (a >> j) & 1), j
    assert np.array_equal(ea.decrypt_batch(ct, sk), a)
    # one fused step against the two calls, words and bookkeeping
    c1, c2, t = ct.clone(), ct.clone(), ea.encrypt_batch(sk, a % 2)
    c1 -= t
    c1.divideByP()
    c2.subDivideByP(t, fused=True)
    assert (c1.lnNoise, c1.primeSet, c1.ptxtSpace, c1.intFactor) == (c2.lnNoise, c2.primeSet, c2.ptxtSpace, c2.intFactor)
    w1, w2 = _words(c1), _words(c2)
    assert all(np.array_equal(w1[h], w2[h]) for h in w1)
    assert np.array_equal(ea.decrypt_batch(c2, sk), a >> 1)
