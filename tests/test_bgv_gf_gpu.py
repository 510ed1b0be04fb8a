"""BGV slots in GF(p^d) on the device (hx_bgv_gf_*, helib_amd.bgv_gf) against the restatement of the reference's
definitions (tests/bgv_gf_ref.py), the integer kernels (hx_bgv_crt_*, hx_bgv_*) as an independent witness, and numpy on
[B, nslots, d] slot arrays after homomorphic operations with real keys.  Everything here is an integer: every comparison
is exact."""
import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_gf_ref as GR
from tests import bgv_hypercube_ref as H

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


def _check_encode(hx, c, table, ref, a, mul, idx):
    want = ref.encode(a, mul)
    d, cf = hx.bgvGfEncode(table, a, idx, mul, coeffs=True)
    assert np.array_equal(cf, want)
    if idx:
        assert np.array_equal(d.download(), _words(hx, c, idx, want))


# ---- (a) encode, embed and decode against the restatement ----
# (15, 2): d = 4, 2 slots; (85, 2): d = 8, order -8; (32, 7): odd p, a bad dimension; (31, 3): d = 30, one slot, no
# hypercube; (341, 2): d = 10, phi = 300 -- the window and the fold cross the 256-coefficient tile edge
@pytest.mark.parametrize("m,p", [(15, 2), (85, 2), (32, 7), (13, 3), (31, 3), (341, 2)])
def test_encode_embed_decode_against_the_restatement(hx, m, p):
    ref = GR.tables(m, p)
    n, d = ref.nslots, ref.d
    c = _ctx(hx, m, 2)
    t = hx.BgvGf(c, p)
    assert (t.d, t.nslots, t.gens, t.ords, t.G) == (d, n, ref.z.gens, ref.z.signedOrds(), [int(x) for x in ref.G])
    ld, ldr = (ref.phim + 3) // 4 * 4, (ref.phim + d - 1 + 3) // 4 * 4
    assert t.table_bytes == 4 * (n * (ld + ldr + 2 * d * d) + (d - 1) * ld)
    rng = np.random.default_rng(m)
    for B, idx, mul in ((1, [0, 1], 1), (3, [], p + 3 if p > 2 else 3), (17, [1], 2 * p + 1)):
        a = rng.integers(-3 * p, 5 * p, size=(B, n, d))            # signed and out of range
        a[0, 0] = -1
        _check_encode(hx, c, t, ref, a, mul, idx)
        f = rng.integers(-2 ** 40, 2 ** 40, size=(B, ref.phim))
        assert np.array_equal(hx.bgvGfEmbed(t, f), ref.decode(f))
        assert np.array_equal(hx.bgvGfEmbed(t, ref.encode(a)), a % p)
        # hx_bgv_gf_decode: a polynomial on two primes holding small coefficients, times factor_inv
        small = rng.integers(-1000, 1000, size=(B, ref.phim))
        res = np.stack([np.mod(small, np.int64(c.primes[i])).astype(np.uint64) for i in (0, 1)])
        acc = hx.DoubleCRT(c, [0, 1], B, res).FFT()
        finv = 2 % p if p > 2 else 1
        assert np.array_equal(hx.bgvGfDecode(t, acc, finv), ref.decode(small * finv))
    short = hx.bgvGfEncode(t, [[[0, 1]]], [], coeffs=True)[1]       # missing slots and coefficients are zero
    full = np.zeros((1, n, d), dtype=np.int64)
    full[0, 0, 1] = 1
    assert np.array_equal(short, ref.encode(full))


# ---- (b) lazy reduction, every input word p - 1 ----
# (64, 2^31 - 1): d = 2 and limit = 4: 16 slots x 2 taps pass it eight times; (13, 2^31 - 1): d = 6 > limit, so one
# slot alone passes it, in the per-slot maps (6 terms) as well
@pytest.mark.parametrize("m,d,n", [(64, 2, 16), (13, 6, 2)])
def test_lazy_reduction_at_the_largest_prime(hx, m, d, n):
    p = 2147483647
    ref = GR.tables(m, p)
    assert (ref.d, ref.nslots, (1 << 64) // (p * p)) == (d, n, 4)
    c = _ctx(hx, m, 2)
    t = hx.BgvGf(c, p)
    rng = np.random.default_rng(7)
    a = np.concatenate([np.full((1, n, d), p - 1), rng.integers(0, p, size=(2, n, d))])
    want = ref.encode(a)
    assert np.array_equal(hx.bgvGfEncode(t, a, [], coeffs=True)[1], want)
    f = np.concatenate([np.full((1, ref.phim), p - 1), rng.integers(0, p, size=(2, ref.phim))])
    assert np.array_equal(hx.bgvGfEmbed(t, f), ref.decode(f))
    assert np.array_equal(hx.bgvGfEmbed(t, want), a % p)


# ---- (c) d = 1: the integer paths, word for word ----
def test_d1_equals_the_integer_paths(hx):
    m, p, B = 1024, 12289, 3
    c = _ctx(hx, m, 2)
    t, crt, old = hx.BgvGf(c, p), hx.BgvCrt(c, p), hx.BgvSlots(c, p)
    assert (t.d, t.nslots, t.gens, t.ords) == (1, 512, old.gens, old.ords) and len(t.G) == 2
    rng = np.random.default_rng(1)
    a = rng.integers(-p, 2 * p, size=(B, 512))
    d2, c2 = hx.bgvGfEncode(t, a[:, :, None], [0, 1], 77, coeffs=True)
    d1, c1 = hx.bgvCrtEncode(crt, a, [0, 1], 77, coeffs=True)
    d0, c0 = hx.bgvEncode(old, a, [0, 1], 77, coeffs=True)
    assert np.array_equal(c2, c1) and np.array_equal(c2, c0)
    assert np.array_equal(d2.download(), d1.download()) and np.array_equal(d2.download(), d0.download())
    f = rng.integers(-2 ** 50, 2 ** 50, size=(B, 512))
    got = hx.bgvGfEmbed(t, f)
    assert got.shape == (B, 512, 1)
    assert np.array_equal(got[:, :, 0], hx.bgvCrtEmbed(crt, f)) and np.array_equal(got[:, :, 0], hx.bgvEmbed(old, f))


# ---- (d) a 2-D input means constants, and gives bgv_crt's words ----
@pytest.mark.parametrize("m,p", [(85, 2), (341, 2)])
def test_constants_equal_the_integer_encode(hx, m, p):
    c = _ctx(hx, m, 2)
    t, crt = hx.BgvGf(c, p), hx.BgvCrt(c, p)
    a = np.random.default_rng(m).integers(-4, 5, size=(17, t.nslots))
    d1, c1 = hx.bgvGfEncode(t, a, [1, 0], 1, coeffs=True)
    d0, c0 = hx.bgvCrtEncode(crt, a, [1, 0], 1, coeffs=True)
    assert np.array_equal(c1, c0) and np.array_equal(d1.download(), d0.download())
    got = hx.bgvGfEmbed(t, c0)
    assert np.array_equal(got[:, :, 0], a % p) and not np.any(got[:, :, 1:])


# ---- (e) the measured ring: m = 21845, p = 2, d = 16, 1024 slots, 65 coefficient tiles, two batch tiles ----
def test_full_size_round_trip_and_constants(hx):
    m, p, B = 21845, 2, 17
    c = _ctx(hx, m, 1)
    t, crt = hx.BgvGf(c, p), hx.BgvCrt(c, p)
    assert (t.d, t.nslots, t.ords, c.phim) == (16, 1024, [-128, -8], 16384)
    rng = np.random.default_rng(2)
    a = rng.integers(0, p, size=(B, 1024, 16))
    a[0] = 1
    a[1] = 0
    a[1, 1023, 15] = 1
    cf = hx.bgvGfEncode(t, a, [], coeffs=True)[1]
    assert np.array_equal(hx.bgvGfEmbed(t, cf), a)
    # constants against the integer kernels, both ways
    k = rng.integers(0, p, size=(B, 1024))
    ck = hx.bgvCrtEncode(crt, k, [], coeffs=True)[1]
    assert np.array_equal(hx.bgvGfEncode(t, k, [], coeffs=True)[1], ck)
    got = hx.bgvGfEmbed(t, ck)
    assert np.array_equal(got[:, :, 0], k) and not np.any(got[:, :, 1:])
    # linear over Z_p: the encoding of a sum is the sum of the encodings
    b = rng.integers(0, p, size=(B, 1024, 16))
    assert np.array_equal(hx.bgvGfEncode(t, a + b, [], coeffs=True)[1], (cf + hx.bgvGfEncode(t, b, [], coeffs=True)[1]) % p)


# ---- (f) homomorphic operations with real keys ----
def _chain(hx, m, p, bits, seed=5):
    from helib_amd import bgv_gf, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, 1, bits=bits, c=3)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    ea = bgv_gf.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    (hk.addFrbMatrices if ea.getDegree() <= 8 else hk.addMinimalFrbMatrices)(sk)
    return cc, g, sk, ea


def _roll(a, ea, i, k):
    shape = [ea.sizeOfDimension(j) for j in range(ea.dimension())]
    return np.roll(a.reshape(a.shape[0], *shape, a.shape[2]), k, axis=1 + i).reshape(a.shape)


# (85, 2): d = 8, one non-native dimension; (803, 3): d = 60, odd p (intFactor), two non-native dimensions
@pytest.mark.parametrize("m,p,bits", [(85, 2, 300), (803, 3, 700)])
def test_homomorphic_operations_on_gf_slots(hx, m, p, bits):
    cc, g, sk, ea = _chain(hx, m, p, bits)
    assert ea.zMStar.signedOrds() == H.RINGS[m, p]
    B, n, d = 2, ea.size(), ea.getDegree()
    assert d == {85: 8, 803: 60}[m]
    if m == 85:
        assert ea.getG() == [int(x) for x in GR.tables(m, p).G]
    rng = np.random.default_rng(m)
    a, b, c = rng.integers(0, p, size=(3, B, n, d))
    a[0] = 0
    a[0, 0, 1] = 1                                              # the slot X
    ca, cb = ea.encrypt_batch(sk, a), ea.encrypt_batch(sk, b)
    assert np.array_equal(ea.decrypt_batch(ca, sk), a)
    prod = ca.clone()
    prod.multiplyBy(cb)
    assert np.array_equal(ea.decrypt_batch(prod, sk), ea.mulPlain(a, b))
    prod += ea.encrypt_batch(sk, c)
    assert np.array_equal(ea.decrypt_batch(prod, sk), (ea.mulPlain(a, b) + c) % p)
    one = ea.encrypt(sk, b[:1])
    ea.multByConstant(one, ea.encodePtxt(c[:1]))
    assert np.array_equal(ea.decrypt(one, sk), ea.mulPlain(b[:1], c[:1])[0])
    ea.addConstant(one, ea.encodePtxt(a[:1]))
    assert np.array_equal(ea.decrypt(one, sk), (ea.mulPlain(b[:1], c[:1]) + a[:1])[0] % p)
    # between slots: whole slot values move
    bad = [i for i in range(ea.dimension()) if not ea.nativeDimension(i)][0]
    ct = cb.clone()
    ea.rotate1D(ct, bad, 1)
    assert np.array_equal(ea.decrypt_batch(ct, sk), _roll(b, ea, bad, 1))
    jobs = [("rotate", (3,), np.roll(b, 3, axis=1)), ("shift", (-2,), H.shift(b, -2)),
            ("totalSums", (), H.total_sums(b, p)), ("runningSums", (), H.running_sums(b, p))]
    for op, args, want in jobs:
        res = {}
        for fused in (True, False):                             # the fused and the term-by-term mask paths
            ct = cb.clone()
            getattr(ea, op)(ct, *args, fused=fused)
            assert np.array_equal(ea.decrypt_batch(ct, sk), want), (op, fused)
            res[fused] = ct
        H.same(res[True], res[False], lambda part: part.download())
    # the Frobenius on slots
    fr = cb.clone()
    ea.frobeniusAutomorph(fr, 1)
    want = ea.frobeniusPlain(b, 1)
    assert np.array_equal(ea.decrypt_batch(fr, sk), want) and not np.array_equal(want, b)
    power = b
    for _ in range(p - 1):                                      # alpha^p by p - 1 products
        power = ea.mulPlain(power, b)
    assert np.array_equal(want, power)
    same = cb.clone()
    ea.frobeniusAutomorph(same, d)
    assert np.array_equal(ea.decrypt_batch(same, sk), b) and np.array_equal(ea.frobeniusPlain(b, d), b)


# ---- (g) errors ----
def test_refusals(hx):
    from helib_amd import bgv_gf, ckks, ctxt as hc
    c = _ctx(hx, 85, 2)
    for p, code in ((2147483659, hx.HX_ERR_UNSUPPORTED), (5, hx.HX_ERR_INVALID), (15, hx.HX_ERR_INVALID)):
        with pytest.raises(hx.HxError) as e:
            hx.BgvGf(c, p)
        assert e.value.code == code, p
    with pytest.raises(hx.HxError, match="130.*64") as e:          # ord_131(2) = 130 > 64
        hx.BgvGf(_ctx(hx, 131, 1), 2)
    assert e.value.code == hx.HX_ERR_UNSUPPORTED
    cc = hc.ChainContext(85, 2, 1, bits=100, c=2)
    F = GR.tables(85, 2).F
    with pytest.raises(ckks.LogicError, match="FindRoots"):
        bgv_gf.EncryptedArray(cc, c, G=[int(x) for x in F[1]])
    ea = bgv_gf.EncryptedArray(cc, c, G=[int(x) for x in F[0]])
    t = ea.enc.table                                                # the device is untouched by the refusals
    with pytest.raises(hx.InvalidArgument):
        hx.bgvGfEncode(t, np.zeros((1, 9, 8), dtype=np.int64), [])
    v = np.zeros((1, 8, 8), dtype=np.int64)
    v[0, 3, 5] = 1
    assert np.array_equal(ea.decode(ea.encodeCoeffs(v)), v)
