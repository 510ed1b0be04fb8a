"""BGV slot encoding and decoding on the device (hx_bgv_*, helib_amd.bgv) for d = ord_m(p) = 1 against the restatement
of the reference's definitions (tests/bgv_slots_ref.py), the oracle's transforms and the host's Encrypt / Decrypt.
Everything here is an integer: every comparison is exact."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import bgv_slots_ref as R

pytestmark = pytest.mark.gpu

# (m, p): p = 1 mod m
SMALL = [(16, 17), (64, 193), (256, 257), (105, 211)]
LARGE = [(32768, 65537), (65536, 65537), (21845, 43691)]


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


@functools.lru_cache(maxsize=None)
def _points(m, p):
    return R.points(m, p)


def _ctx(hx, m, nprimes=2, bits=60):
    g = O.PrimeGen(bits, m)
    primes = [g.next() for _ in range(nprimes)]
    o, c = O.Ctx(m), hx.Context(m)
    for q in primes:
        i = o.add_prime(q)
        c.add_prime(q, o.roots[i])
    return c, o, primes


# ---- 1. may the existing row kernels carry the plaintext prime? ----
@pytest.mark.parametrize("m,p", [(32768, 65537), (1024, 12289), (21845, 43691), (65536, 65537), (16, 17), (105, 211)])
def test_engine_transform_is_exact_for_the_small_prime(hx, m, p):
    """FFT / iFFT of rows modulo p itself, word for word against the oracle's transform (same root)"""
    o, c = O.Ctx(m), hx.Context(m)
    i = o.add_prime(p)
    c.add_prime(p, o.roots[i])
    rng = np.random.default_rng(m)
    B = 3
    x = rng.integers(0, p, size=(1, B, c.phim), dtype=np.uint64)
    x[0, 0, :4] = [0, 1, p - 1, p // 2]
    d = hx.DoubleCRT(c, [0], B, x)
    fwd = d.FFT().download()
    for b in range(B):
        assert np.array_equal(fwd[0, b], o.fft([0], x[:, b])[0]), (m, p, b)
    back = hx.DoubleCRT(c, [0], B, x).iFFT().download()
    for b in range(B):
        assert np.array_equal(back[0, b], o.ifft([0], x[:, b])[0]), (m, p, b)
    assert np.array_equal(d.iFFT().download(), x)


# ---- 2. encode ----
def _check_rows(o, primes, d, cf, B):
    rows = d.download()
    idx = list(range(len(primes)))
    for b in sorted({0, B - 1, B // 2}):
        res = np.stack([np.mod(cf[b], np.int64(q)).astype(np.uint64) for q in primes])
        assert np.array_equal(rows[:, b], o.fft(idx, res)), b


@pytest.mark.parametrize("m,p", SMALL)
@pytest.mark.parametrize("B", [1, 3])
def test_encode_equals_the_literal_crt(hx, m, p, B):
    c, o, primes = _ctx(hx, m)
    t = hx.BgvSlots(c, p)
    assert t.rho == max(R.primitive_roots(m, p))
    z = R.zmstar(m, p)
    assert (t.gens, t.ords) == (z.gens, z.ords)
    n = c.phim
    v = np.random.default_rng(m + B).integers(0, p, size=(B, n))
    d, cf = hx.bgvEncode(t, v, [0, 1], coeffs=True)
    for b in range(B):
        assert np.array_equal(cf[b], R.encode_crt(v[b], m, p)), (m, b)
    assert np.all(np.abs(cf) <= p // 2)
    _check_rows(o, primes, d, cf, B)
    assert np.array_equal(hx.bgvEmbed(t, cf), v)


@pytest.mark.parametrize("m,p,B", [(1024, 12289, 1), (1024, 12289, 3)] +
                         [(m, p, B) for m, p in LARGE for B in (1, 3, 64)])
def test_encode_satisfies_the_defining_property(hx, m, p, B):
    """H(rho^(1/t_i)) = a_i mod p by Horner: at all slots for m = 1024, at 64 sampled slots per element beyond"""
    c, o, primes = _ctx(hx, m, 2 if B < 64 else 1)
    t = hx.BgvSlots(c, p)
    assert t.rho == R.rho_of(m, p)
    n = c.phim
    rng = np.random.default_rng(m + B)
    v = rng.integers(0, p, size=(B, n))
    idx = list(range(len(primes)))
    d, cf = hx.bgvEncode(t, v, idx, coeffs=True)
    assert np.all(np.abs(cf) <= p // 2)           # p odd: (-p/2, p/2)
    pts = _points(m, p)
    which = list(range(n)) if m == 1024 else sorted(set([0, 1, n - 1]) | set(rng.integers(0, n, size=61).tolist()))
    assert np.array_equal(R.decode(cf, m, p, pts, which), v[:, which])
    _check_rows(o, primes, d, cf, B)
    assert np.array_equal(hx.bgvEmbed(t, cf), v)


def test_encode_mul_padding_and_reduction(hx):
    m, p = 1024, 12289
    c, o, primes = _ctx(hx, m)
    t = hx.BgvSlots(c, p)
    rng = np.random.default_rng(7)
    v = rng.integers(0, p, size=(2, c.phim))
    _, cf = hx.bgvEncode(t, v, [0], coeffs=True)
    for mul in (2, p - 1, 5000, p + 3):
        d, cm = hx.bgvEncode(t, v, [0, 1], mul=mul, coeffs=True)
        assert np.array_equal(cm, R.balanced(cf * (mul % p), p))
        _check_rows(o, primes, d, cm, 2)
    # fewer values than slots pad with 0
    short = v[:, :37]
    full = np.zeros_like(v)
    full[:, :37] = short
    assert np.array_equal(hx.bgvEncode(t, short, [], coeffs=True)[1], hx.bgvEncode(t, full, [], coeffs=True)[1])
    empty = hx.bgvEncode(t, np.zeros((2, 0), dtype=np.int64), [], coeffs=True)[1]
    assert not empty.any()
    # negative and >= p inputs reduce; any int64
    wild = v.astype(np.int64) - 5 * p
    wild[0, :4] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1, p]
    want = np.array([[int(x) % p for x in row] for row in wild])
    got = hx.bgvEncode(t, wild, [], coeffs=True)[1]
    assert np.array_equal(hx.bgvEmbed(t, got), want)
    assert np.array_equal(hx.bgvEmbed(t, got + 3 * p), want)      # embed reduces its input as well


@pytest.mark.parametrize("m,p", [(1024, 12289), (105, 211), (32768, 65537)])
def test_slotwise_ring_structure(hx, m, p):
    """encode(a) * encode(b) mod (Phi_m, p), multiplied through the oracle's transform for p, decodes to a*b mod p"""
    c, _, _ = _ctx(hx, m, 1)
    t = hx.BgvSlots(c, p)
    rng = np.random.default_rng(m)
    a, b = rng.integers(0, p, size=(2, 1, c.phim))
    fa, fb = hx.bgvEncode(t, a, [], coeffs=True)[1], hx.bgvEncode(t, b, [], coeffs=True)[1]
    op = O.Ctx(m)
    op.add_prime(p)
    ea, eb = op.fft([0], (fa % p).astype(np.uint64)), op.fft([0], (fb % p).astype(np.uint64))
    prod = op.ifft([0], O.row_op("mul", ea[0], eb[0], p)[None, :])
    assert np.array_equal(hx.bgvEmbed(t, prod.astype(np.int64)), a * b % p)
    assert np.array_equal(hx.bgvEmbed(t, fa + fb), (a + b) % p)


# ---- 3. with real keys ----
def _chain(hx, m, p, bits, seed=5):
    from helib_amd import bgv, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, 1, bits=bits, c=3)
    g = hx.Context(m)
    o = O.Ctx(m)
    for q in cc.primes:
        i = o.add_prime(q)
        g.add_prime(q, o.roots[i])
    nprimes = len(g.primes)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    ea = bgv.EncryptedArray(cc, g)
    assert len(g.primes) == nprimes == len(cc.primes)    # p went to a side context: the chain reads as before
    sk.zMStar = ea.zMStar
    return cc, g, sk, ea


@pytest.mark.parametrize("m,p,bits", [(1024, 12289, 300), (32768, 65537, 950)])
def test_round_trip_and_arithmetic_with_keys(hx, m, p, bits):
    cc, g, sk, ea = _chain(hx, m, p, bits)
    B, n = 8, ea.size()
    assert (ea.getP(), ea.getDegree(), n) == (p, 1, cc.phim)
    rng = np.random.default_rng(m)
    a, b, c = rng.integers(0, p, size=(3, B, n))
    ca, cb, cx = ea.encrypt_batch(sk, a), ea.encrypt_batch(sk, b), ea.encrypt_batch(sk, c)
    assert np.array_equal(ea.decrypt_batch(ca, sk), a)
    ca.multiplyBy(cb)
    ca += cx
    assert np.array_equal(ea.decrypt_batch(ca, sk), (a * b + c) % p)
    # constants
    e = ea.encodePtxt(b[:1])
    ea.multByConstant(cx, e)
    assert np.array_equal(ea.decrypt_batch(cx, sk), c * b[:1] % p)
    ea.addConstant(cx, e)
    assert np.array_equal(ea.decrypt_batch(cx, sk), (c * b[:1] + b[:1]) % p)
    ea.addConstant(ca, e, neg=True)      # after a multiply: intFactor / the prime set's factor are live
    assert np.array_equal(ea.decrypt_batch(ca, sk), (a * b + c - b[:1]) % p)
    one = ea.encrypt(sk, a[0])
    assert np.array_equal(ea.decrypt(one, sk), a[0])


@pytest.mark.parametrize("m,p,bits", [(1024, 12289, 300), (32768, 65537, 950)])
def test_rotate1d_moves_the_coordinate(hx, m, p, bits):
    """After rotate1D(ct, dim, amt) the slot whose coordinate in dim is c + amt holds what the slot with coordinate c
    held.  m = 1024 takes add1DMatrices (255 + 1 matrices).  At m = 32768 dimension 0 has order 8192: the full family
    would be 8191 matrices of about 15 MB each, so there the matrices of exactly the rotations under test are
    generated -- rotate1D is one automorphism either way."""
    from helib_amd import keys as hk
    cc, g, sk, ea = _chain(hx, m, p, bits)
    assert ea.dimension() == 2 and all(ea.nativeDimension(i) for i in range(2))
    assert ea.sizeOfDimension(0) * ea.sizeOfDimension(1) == ea.size()
    cases = [(0, 1), (0, -3), (0, ea.sizeOfDimension(0) + 5), (1, 1), (1, -1)]
    if m == 1024:
        hk.add1DMatrices(sk)
    else:
        for dim, amt in cases:
            sk.GenKeySWmatrix(1, ea.zMStar.genToPow(dim, amt % ea.sizeOfDimension(dim)))
    sk.setKeySwitchMap()
    B, n = 2, ea.size()
    a = np.random.default_rng(3).integers(0, p, size=(B, n))
    slots = np.arange(n)
    for dim, amt in cases:
        ct = ea.encrypt_batch(sk, a)
        ea.rotate1D(ct, dim, amt)
        got = ea.decrypt_batch(ct, sk)
        ord_ = ea.sizeOfDimension(dim)
        stride = n // int(np.prod([ea.sizeOfDimension(i) for i in range(dim + 1)]))
        coord = slots // stride % ord_
        dest = slots + ((coord + amt) % ord_ - coord) * stride     # coordinate c -> c + amt
        want = np.empty_like(a)
        want[:, dest] = a
        assert np.array_equal(got, want), (dim, amt)
        assert ea.coordinate(dim, int(dest[5])) == (ea.coordinate(dim, 5) + amt) % ord_


def test_encrypt_batch_equals_consecutive_encrypts(hx):
    m, p = 1024, 12289
    cc, g, sk, ea = _chain(hx, m, p, 300, seed=11)
    _, _, sk2, _ = _chain(hx, m, p, 300, seed=11)
    B = 3
    v = np.random.default_rng(1).integers(0, p, size=(B, ea.size()))
    polys = ea.encodeCoeffs(v)                      # the host-encoded polynomials
    ct = ea.encrypt_batch(sk, v)
    rows = [ct.parts[h].download() for h in ("1", "s")]
    for b in range(B):
        one = sk2.Encrypt([int(x) for x in polys[b]])
        for k, h in enumerate(("1", "s")):
            assert np.array_equal(one.parts[h].download()[:, 0], rows[k][:, b]), (b, h)
        assert one.lnNoise == ct.lnNoise and one.ptxtSpace == ct.ptxtSpace == p


# ---- 4. errors: argument checks on the host ----
def test_errors(hx):
    from helib_amd import bgv, ckks, ctxt as hc
    big = hx.Context(32768)
    with pytest.raises(hx.HxError, match=r"d = ord_m\(p\) = 8192.*only d = 1") as e:
        hx.BgvSlots(big, 3)
    assert e.value.code == hx.HX_ERR_UNSUPPORTED
    with pytest.raises(hx.InvalidArgument, match="divides m"):
        hx.BgvSlots(big, 2)
    with pytest.raises(hx.InvalidArgument, match="not a prime"):
        hx.BgvSlots(big, 65536)
    c, _, _ = _ctx(hx, 1024)
    t = hx.BgvSlots(c, 12289)
    with pytest.raises(hx.InvalidArgument, match="slot count"):
        hx.bgvEncode(t, np.zeros((1, c.phim + 1), dtype=np.int64), [0])
    other, _, _ = _ctx(hx, 1024)
    foreign = hx.DoubleCRT(other, [0], 1)
    with pytest.raises(hx.InvalidArgument, match="another context"):
        hx.bgvDecode(t, foreign)
    with pytest.raises(hx.InvalidArgument, match="another context"):
        hx._chk(hx.lib().hx_bgv_encode(t.h, None, 1, 0, 1, foreign.h, None))
    with pytest.raises(hx.InvalidArgument, match="null argument"):
        hx._chk(hx.lib().hx_bgv_embed(t.h, None, 1, None))
    mine = hx.DoubleCRT(c, [0], 1)
    with pytest.raises(hx.InvalidArgument, match="bad batch"):
        hx._chk(hx.lib().hx_bgv_encode(t.h, None, 0, 0, 1, mine.h, None))
    assert len(c.primes) == 2
    n = hx.C.c_int()
    hx._chk(hx.lib().hx_ctx_num_primes(c.h, hx.C.byref(n)))
    assert n.value == 2
    with pytest.raises(ckks.LogicError, match="CKKS context"):
        bgv.EncryptedArray(hc.ChainContext(1024, -1, 20, bits=100, c=2, ckks=True), c)
    with pytest.raises(hx.HxError, match="only d = 1") as e:
        bgv.EncryptedArray(hc.ChainContext(1024, 257, 1, bits=100, c=2), c)
    assert e.value.code == hx.HX_ERR_UNSUPPORTED
    with pytest.raises(hx.HxError, match="r > 1") as e:
        bgv.EncryptedArray(hc.ChainContext(1024, 12289, 2, bits=100, c=2), c)
    assert e.value.code == hx.HX_ERR_UNSUPPORTED
    # a ciphertext whose plaintext space is not p
    cc, g, sk, ea = _chain(hx, 1024, 12289, 300)
    ct = ea.encrypt(sk, [1, 2, 3])
    ct.ptxtSpace = 17
    with pytest.raises(ckks.LogicError, match="plaintext space is not p"):
        ea.decrypt(ct, sk)
    ct.ptxtSpace = 12289
    assert np.array_equal(ea.decrypt(ct, sk)[:4], [1, 2, 3, 0])     # the device is untouched by the refusals
