"""hx_mask_blend against the hx_mul / hx_add / hx_mul / hx_sub sequence it replaces (every word), and
helib_amd.bgv_hypercube -- rotate / shift / sums / MatMul1DExec over non-native dimensions -- with real keys against
numpy on the plaintext slots.  Everything here is an integer: every comparison is exact."""
import numpy as np
import pytest

from oracle import oracle as O
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


def _ctx(hx, m, nprimes=3, bits=60):
    g = O.PrimeGen(bits, m)
    primes = [g.next() for _ in range(nprimes)]
    o, c = O.Ctx(m), hx.Context(m)
    for q in primes:
        i = o.add_prime(q)
        c.add_prime(q, o.roots[i])
    return c, primes


def _rand(rng, primes, idx, batch, n):
    """canonical residues [rows, batch, n] with 0, 1, q - 1 and q - 2 among them"""
    x = np.stack([rng.integers(0, primes[i], size=(batch, n), dtype=np.uint64) for i in idx])
    for r, i in enumerate(idx):
        x[r, :, :4] = [0, primes[i] - 1, 1, primes[i] - 2]
        x[r, -1, -2:] = [primes[i] - 1, 0]
    return x


def _four_calls(c, t, mask):
    """c *= mask; c += t; t *= mask; c -= t"""
    for a, b in zip(c, t):
        a *= mask
        a += b
        b *= mask
        a -= b


def _blend_case(hx, c, primes, rng, parts, batch, mask_batch, superset):
    n = c.phim
    idx = [0, 2] if superset else [0, 1, 2]
    midx = [2, 1, 0] if superset else idx            # more primes than c, in another order
    cd = [_rand(rng, primes, idx, batch, n) for _ in range(parts)]
    td = [_rand(rng, primes, idx, batch, n)[:, ::-1].copy() for _ in range(parts)]
    md = _rand(rng, primes, midx, mask_batch, n)
    mask = hx.DoubleCRT(c, midx, mask_batch, md)
    cs = [hx.DoubleCRT(c, idx, batch, x) for x in cd]
    ts = [hx.DoubleCRT(c, idx, batch, x) for x in td]
    hx.maskBlend(cs[0], cs[1] if parts == 2 else None, ts[0], ts[1] if parts == 2 else None, mask)
    rc = [hx.DoubleCRT(c, idx, batch, x) for x in cd]
    rt = [hx.DoubleCRT(c, idx, batch, x) for x in td]
    _four_calls(rc, rt, mask)
    for a in range(parts):
        got = cs[a].download()
        assert np.array_equal(got, rc[a].download()), (n, parts, batch, mask_batch, superset, a)
        assert np.array_equal(ts[a].download(), td[a]), "t is read only"
        if n <= 64:                                   # and python integers, independent of any kernel
            for r, i in enumerate(idx):
                q = primes[i]
                mrow = md[midx.index(i)]
                for b in range(batch):
                    mb = mrow[b if mask_batch > 1 else 0]
                    want = [(int(x) * int(k) + int(y) - int(y) * int(k)) % q
                            for x, y, k in zip(cd[a][r, b], td[a][r, b], mb)]
                    assert [int(x) for x in got[r, b]] == want
    assert np.array_equal(mask.download(), md)        # the mask is read only


# ---- 1. the kernel against the four-call sequence ----
@pytest.mark.parametrize("m", [85, 119, 1785])
def test_mask_blend_equals_mul_add_mul_sub(hx, m):
    """N = 64; 96 (48 vectors: fewer than one workgroup's threads); 768 (384 vectors: two workgroups, the second
    partial)"""
    c, primes = _ctx(hx, m)
    assert c.phim == {85: 64, 119: 96, 1785: 768}[m]
    rng = np.random.default_rng(m)
    for parts in (1, 2):
        for batch in (1, 3, 5):
            for mask_batch in sorted({1, batch}):
                for superset in (False, True):
                    _blend_case(hx, c, primes, rng, parts, batch, mask_batch, superset)


def test_mask_blend_when_c_is_a_lazy_copy_of_t(hx):
    """hx_poly_copy shares rows until one side is written: c sharing t's rows takes its own copy, and c*m + t - t*m
    is then c unchanged"""
    c, primes = _ctx(hx, 1785)
    rng = np.random.default_rng(2)
    x, md = _rand(rng, primes, [0, 1, 2], 3, c.phim), _rand(rng, primes, [0, 1, 2], 1, c.phim)
    mask = hx.DoubleCRT(c, [0, 1, 2], 1, md)
    t = hx.DoubleCRT(c, [0, 1, 2], 3, x)
    cc, bystander = t.copy(), t.copy()
    hx.maskBlend(cc, None, t, None, mask)
    assert np.array_equal(cc.download(), x) and np.array_equal(t.download(), x)
    assert np.array_equal(bystander.download(), x)


def test_mask_blend_in_a_graph_capture(hx):
    c, primes = _ctx(hx, 1785)
    rng = np.random.default_rng(4)
    n, idx, B = c.phim, [0, 1, 2], 5
    x = [_rand(rng, primes, idx, B, n) for _ in range(4)]
    mask = hx.DoubleCRT(c, idx, 1, _rand(rng, primes, idx, 1, n))
    direct = [hx.DoubleCRT(c, idx, B, v) for v in x]
    hx.maskBlend(direct[0], direct[1], direct[2], direct[3], mask)  # eagerly once
    ops = [hx.DoubleCRT(c, idx, B, v) for v in x]
    c.graphBegin()
    hx.maskBlend(ops[0], ops[1], ops[2], ops[3], mask)
    graph = c.graphEnd()
    for d, v in zip(ops, x):                                         # (nothing ran yet)
        d.upload(v)
    graph.launch()
    for a in range(4):
        assert np.array_equal(ops[a].download(), direct[a].download())
    # fresh operands in the same polys
    y = [_rand(rng, primes, idx, B, n) for _ in range(4)]
    for d, v in zip(ops, y):
        d.upload(v)
    graph.launch()
    rc = [hx.DoubleCRT(c, idx, B, y[0]), hx.DoubleCRT(c, idx, B, y[1])]
    rt = [hx.DoubleCRT(c, idx, B, y[2]), hx.DoubleCRT(c, idx, B, y[3])]
    _four_calls(rc, rt, mask)
    for a in range(2):
        assert np.array_equal(ops[a].download(), rc[a].download())
        assert np.array_equal(ops[2 + a].download(), y[2 + a])
    graph.destroy()


def test_mask_blend_refusals_touch_nothing(hx):
    c, primes = _ctx(hx, 119)
    other, _ = _ctx(hx, 119)
    rng = np.random.default_rng(6)
    n, idx, B = c.phim, [0, 1], 3
    xs = [_rand(rng, primes, idx, B, n) for _ in range(4)]
    c0, c1, t0, t1 = (hx.DoubleCRT(c, idx, B, x) for x in xs)
    md = _rand(rng, primes, [0, 1, 2], 1, n)
    mask = hx.DoubleCRT(c, [0, 1, 2], 1, md)

    def refused(code, match, *args):
        with pytest.raises(hx.HxError, match=match) as e:
            hx._chk(hx.lib().hx_mask_blend(*[a.h if a is not None else None for a in args]))
        assert e.value.code == code, (match, e.value.code)
        for d, x in zip((c0, c1, t0, t1), xs):
            assert np.array_equal(d.download(), x), match
        assert np.array_equal(mask.download(), md), match

    INV, PS = hx.HX_ERR_INVALID, hx.HX_ERR_PRIMESET
    refused(INV, "null argument", None, None, t0, None, mask)
    refused(INV, "null argument", c0, None, None, None, mask)
    refused(INV, "null argument", c0, None, t0, None, None)
    refused(INV, "go together", c0, c1, t0, None, mask)
    refused(INV, "go together", c0, None, t0, t1, mask)
    # aliasing: c and t are distinct handles, and no output is the mask
    refused(INV, "different polys", c0, None, c0, None, mask)
    refused(INV, "different polys", c0, c0, t0, t1, mask)
    refused(INV, "different polys", c0, c1, t0, c0, mask)
    refused(INV, "different polys", c0, c1, t0, t0, mask)
    one = hx.DoubleCRT(c, idx, B, xs[0])
    refused(INV, "also the mask", one, None, t0, None, one)
    refused(INV, "also the mask", c0, one, t0, t1, one)
    # a foreign context
    fk = hx.DoubleCRT(other, idx, B, xs[0])
    fm = hx.DoubleCRT(other, [0, 1, 2], 1)
    refused(INV, "incompatible objects", c0, None, fk, None, mask)
    refused(INV, "incompatible objects", c0, fk, t0, t1, mask)
    refused(INV, "incompatible objects", c0, None, t0, None, fm)
    # shapes: batch, rows, row order
    for bad in (hx.DoubleCRT(c, idx, B + 1), hx.DoubleCRT(c, [0], B), hx.DoubleCRT(c, [1, 0], B), hx.DoubleCRT(c, [0, 1, 2], B)):
        refused(INV, "t0 differs", c0, None, bad, None, mask)
        refused(INV, "c1 differs", c0, bad, t0, t1, mask)
        refused(INV, "t1 differs", c0, c1, t0, bad, mask)
    refused(INV, "neither 1 nor 3", c0, None, t0, None, hx.DoubleCRT(c, [0, 1, 2], 2))
    # a mask missing a prime
    refused(PS, "no row for prime 1", c0, None, t0, None, hx.DoubleCRT(c, [0, 2], 1))
    # more rows than one launch descriptor holds
    from helib_amd import hostnt
    big, gen = hx.Context(85), hostnt.PrimeGen(50, 85)
    for _ in range(161):
        big.add_prime(gen.next())
    wide = [hx.DoubleCRT(big, range(161), 1) for _ in range(3)]
    refused(hx.HX_ERR_UNSUPPORTED, "too many rows", wide[0], None, wide[1], None, wide[2])
    assert not any(w.download().any() for w in wide)
    # an odd number of coefficients: phi(m) is odd for m = 2 only (phi = 1); polys without rows reach the check
    tiny = hx.Context(2)
    assert tiny.phim == 1
    a, b, mk = (hx.DoubleCRT(tiny, [], 1, zero=False) for _ in range(3))
    with pytest.raises(hx.HxError, match="even number of coefficients") as e:
        hx.maskBlend(a, None, b, None, mk)
    assert e.value.code == hx.HX_ERR_UNSUPPORTED
    # and after all that the call still works
    hx.maskBlend(c0, c1, t0, t1, mask)
    rc = [hx.DoubleCRT(c, idx, B, xs[0]), hx.DoubleCRT(c, idx, B, xs[1])]
    rt = [hx.DoubleCRT(c, idx, B, xs[2]), hx.DoubleCRT(c, idx, B, xs[3])]
    _four_calls(rc, rt, mask)
    assert np.array_equal(c0.download(), rc[0].download()) and np.array_equal(c1.download(), rc[1].download())


# ---- 2. end to end with real keys ----
def _chain(hx, m, p, bits, seed=5, minimal=False):
    from helib_amd import bgv_hypercube, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, 1, bits=bits, c=3)
    g = hx.Context(m)
    o = O.Ctx(m)
    for q in cc.primes:
        i = o.add_prime(q)
        g.add_prime(q, o.roots[i])
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    ea = bgv_hypercube.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    (hk.addMinimal1DMatrices if minimal else hk.add1DMatrices)(sk)
    return cc, g, sk, ea


def _rows(part):
    return part.download()


@pytest.mark.parametrize("m,p,bits", [(119, 2, 500), (255, 2, 600), (527, 2, 600), (803, 3, 700), (1785, 2, 700)])
def test_rotate_shift_and_sums_with_keys(hx, monkeypatch, m, p, bits):
    """decrypt_batch after rotate / shift / totalSums / runningSums against numpy, fused (the kernel) and term by
    term: the same plaintext, and the same words and bookkeeping"""
    cc, g, sk, ea = _chain(hx, m, p, bits)
    assert ea.zMStar.signedOrds() == H.RINGS[m, p]
    B, n = 3, ea.size()
    a = np.random.default_rng(m).integers(0, p, size=(B, n))
    a[0] = 0
    a[0, 0] = 1
    calls = []
    real = hx.maskBlend
    monkeypatch.setattr(hx, "maskBlend", lambda *args: (calls.append(1), real(*args))[1])
    fresh = ea.encrypt_batch(sk, a)                    # both paths start from the same words
    jobs = [("rotate", (amt,), np.roll(a, amt, axis=1)) for amt in (1, 2, n // 2 + 1, n - 1, -3)]
    jobs += [("shift", (k,), H.shift(a, k)) for k in (1, -1, n - 1, 1 - n)]
    jobs += [("runningSums", (), H.running_sums(a, p)), ("totalSums", (), H.total_sums(a, p))]
    blends = 0
    for op, args, want in jobs:
        res = {}
        for fused in (True, False):
            del calls[:]
            ct = fresh.clone()
            assert getattr(ea, op)(ct, *args, fused=fused) is ct
            assert np.array_equal(ea.decrypt_batch(ct, sk), want), (op, args, fused)
            assert ct.isCorrect(), (op, args, fused)
            if not fused:
                assert not calls
            blends += len(calls)
            res[fused] = ct
        H.same(res[True], res[False], _rows)
    if p == 2:                                          # (at p = 3 unequal intFactors may leave every blend term by term)
        assert blends > 0


# ---- 3. MatMul1DExec on the device ----
@pytest.mark.parametrize("minimal", [False, True])
@pytest.mark.parametrize("m,p,dim", [(255, 2, 0), (527, 2, 1)])
def test_matmul1d_with_keys(hx, m, p, dim, minimal):
    from helib_amd import bgv_hypercube as bh, bgv_matmul as bm
    cc, g, sk, ea = _chain(hx, m, p, 600, minimal=minimal)
    D = ea.sizeOfDimension(dim)
    assert not ea.nativeDimension(dim)
    rng = np.random.default_rng(m + dim)
    A = rng.integers(0, p, size=(D, D))
    A[0, 0] = 1
    mat = bm.MatMul1D(ea, A, dim)
    ex = bh.MatMul1DExec(ea, mat, minimal=minimal)
    a = rng.integers(0, p, size=(3, ea.size()))
    fresh = ea.encrypt_batch(sk, a)
    res = {}
    for fused in (True, False):
        ct = fresh.clone()
        assert ex.mul(ct, pk=sk, fused=fused) is ct
        assert np.array_equal(ea.decrypt_batch(ct, sk), bm.mulPlain(ea, a, mat)), (m, dim, minimal, fused)
        assert ct.isCorrect()
        res[fused] = ct
    H.same(res[True], res[False], _rows)
