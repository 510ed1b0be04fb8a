"""hx_hoisted_mask_fan on the device against python integers (tests/replicate_ref.hoisted_mask_fan), and
BasicAutomorphPrecon.automorphMasked / replicateAll of real ciphertexts, through the kernel against the calls it replaces.
Everything here is an integer: every comparison is exact.

The shapes of the kernel tests are those of tests/test_hoisted_sum_gpu.py: phi(m) = 36 (less than a wavefront), 64, 126, 1024
through the closed-form gather of a power of two, and 16384 on 2 + 1 rows (64 workgroup columns, through the table
gather); batch 1 (one element per thread), 2, 3 and 5 (a partial group of four, and a second one); one to three digits;
n = 1, 2, 3; for A and B each of: no mask, a mask of batch 1, a mask of the operands' batch -- all nine pairs -- and both
arrays left out; masks and matrices made for exactly the outputs' rows and for two primes more, their rows in reversed
order; and every operand word q - 1 at 60-bit primes with three digits, the largest value both accumulators see."""
import ctypes as C

import numpy as np
import pytest

from tests import replicate_ref as RF
from tests import thin_ref as TR
from tests.test_hoisted_sum_gpu import _digit_block, _frob, _matrix, _psp, _ring, _rnd

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


def _arr(xs, n):
    if xs is None:
        return None
    return (C.c_void_p * max(len(xs), n, 1))(*[getattr(x, "h", None) for x in xs])


def _raw(hx, dg, c0, c1, ks, Ws, A, B, sp, out0, out1, n=None):
    n = len(ks) if n is None else n
    ka = np.array([int(k) for k in ks] or [0], dtype=np.uint64)
    spa = np.array(list(sp) or [0], dtype=np.int32)
    h = lambda x: x.h if x is not None else None                        # noqa: E731
    return hx.lib().hx_hoisted_mask_fan(h(dg), h(c0), h(c1), ka.ctypes.data_as(C.c_void_p), _arr(Ws, n), _arr(A, n), _arr(B, n),
                                        n, spa.ctypes.data_as(C.c_void_p), len(sp), _arr(out0, n), _arr(out1, n))


def _mask(hx, g, rng, midx, allp, kind, B, fill=None):
    """-> (DoubleCRT or None, its rows on the output primes [nall, 1 or B, N] or None)"""
    if kind == "null":
        return None, None
    poly, rows = _rnd(hx, g, rng, midx, B if kind == "per" else 1, fill=fill)
    return poly, rows[[midx.index(i) for i in allp]]


#        m, p, own rows, special rows, batch, digits, extra rows of the matrices and masks, per term (A, B): null / one / per
CASES = [(57, 7, 2, 1, 1, 2, 0, [("one", "one"), ("null", "one")]),
         (85, 2, 3, 2, 3, 3, 0, [("per", "one"), ("one", "per"), ("null", "null")]),
         (127, 2, 2, 1, 2, 1, 2, [("per", "per"), ("null", "per"), ("per", "null")]),
         (2048, 3, 2, 1, 3, 2, 0, [("one", "null"), ("per", "per")]),
         (2048, 5, 3, 1, 5, 2, 2, [("one", "per")]),
         (21845, 2, 2, 1, 2, 2, 0, [("per", "one"), ("null", "per")]),
         (85, 2, 2, 1, 1, 2, 2, None)]


@pytest.mark.parametrize("m,p,L,nsp,B,ndig,extra,kinds", CASES)
def test_kernel_against_python_integers(hx, m, p, L, nsp, B, ndig, extra, kinds):
    g = _ring(hx, m, L + nsp + extra)
    N = g.phim
    n = len(kinds) if kinds is not None else 1
    rng = np.random.default_rng(m + 10 * B + n)
    # with extra rows the operand sits below the matrices' level: it holds primes 1 .. L, the matrices and masks 0 .. L + 1
    own = list(range(1, L + 1)) if extra else list(range(L))
    sp = list(range(L + extra, L + extra + nsp))
    allp = own + sp
    nall = len(allp)
    ks = _frob(m, p)[:n]
    assert len(ks) == n
    dg, dig = _digit_block(hx, g, rng, own, sp, ndig, B)
    c0, r0 = _rnd(hx, g, rng, own, B)
    c1, r1 = _rnd(hx, g, rng, own, B)
    wrows = list(range(L + extra + nsp))[::-1] if extra else allp       # another order, and primes the operand lacks
    Ws, keys = [], []
    for _ in ks:
        W, b, a = _matrix(hx, g, rng, wrows, ndig + (1 if extra else 0))
        sel = [wrows.index(i) for i in allp]
        Ws.append(W)
        keys.append((b[:ndig][:, sel], a[:ndig][:, sel]))
    if kinds is None:
        A = Bm = None
        Ar = Br = [None] * n
    else:
        pa = [_mask(hx, g, rng, wrows, allp, ka, B) for ka, _ in kinds]
        pb = [_mask(hx, g, rng, wrows, allp, kb, B) for _, kb in kinds]
        A, Ar, Bm, Br = [x[0] for x in pa], [x[1] for x in pa], [x[0] for x in pb], [x[1] for x in pb]
    psp = _psp(g, allp, sp)
    want0, want1 = RF.hoisted_mask_fan(m, [g.primes[i] for i in allp], L, psp, dig, r0, r1, ks, keys, Ar, Br)
    # one word by hand: the last term, row 0, element B - 1, word N - 1
    t, q, x = n - 1, g.primes[allp[0]], int(TR.perm(m, ks[-1])[N - 1])
    inner = psp[0] * int(r0[0, B - 1, x]) + sum(int(dig[j, 0, B - 1, x]) * int(keys[t][0][j][0][N - 1]) for j in range(ndig))
    am = 1 if Ar[t] is None else int(Ar[t][0, -1, N - 1])
    bm = 1 if Br[t] is None else int(Br[t][0, -1, N - 1])
    assert int(want0[t][0, B - 1, N - 1]) == (am * (psp[0] * int(r0[0, B - 1, N - 1])) + bm * inner) % q
    out0 = [_rnd(hx, g, rng, [own[0]], B)[0] for _ in range(n)]         # (reshaped and overwritten, not read)
    out1 = [hx.DoubleCRT(g, allp, B) for _ in range(n)]
    assert _raw(hx, dg, c0, c1, ks, Ws, A, Bm, sp, out0, out1) == 0, hx.lib().hx_last_error()
    for t in range(n):
        assert out0[t].getIndexSet() == allp == out1[t].getIndexSet()
        for got, want in ((out0[t].download(), want0[t]), (out1[t].download(), want1[t])):
            assert got.shape == (nall, B, N)
            bad = np.argwhere(got != want)
            assert not len(bad), "term %d: %d words differ, the first at [row, element, word] %s" % (t, len(bad), bad[0])
            assert all((got[r] < g.primes[i]).all() for r, i in enumerate(allp))
    # the inputs and the masks are left as they were
    assert np.array_equal(c0.download(), r0) and np.array_equal(c1.download(), r1)
    assert np.array_equal(dg.download().reshape(dig.shape), dig)
    for polys, rows in ((A, Ar), (Bm, Br)):
        for poly, keep in zip(polys or [], rows):
            if poly is not None:
                assert np.array_equal(poly.download()[[wrows.index(i) for i in allp]], keep)
    # the binding: new outputs; an output that still shares an input's rows (a lazy copy) lets go of them
    o0, o1 = hx.hoistedMaskFan(dg, c0, c1, ks, Ws, A, Bm, sp)
    assert all(o0[t].getIndexSet() == allp and np.array_equal(o0[t].download(), want0[t])
               and np.array_equal(o1[t].download(), want1[t]) for t in range(n))
    lazy = [c0.copy()] + out0[1:]
    assert _raw(hx, dg, c0, c1, ks, Ws, A, Bm, sp, lazy, out1) == 0
    assert np.array_equal(lazy[0].download(), want0[0]) and np.array_equal(c0.download(), r0)
    if m == 85 and B == 3:                                              # the second witness: the calls the kernel replaces
        for t, (k, W) in enumerate(zip(ks, Ws)):
            d2, p0 = dg.copy(), c0.copy()
            d2.automorph(k)
            p0.automorph(k)
            p0.addPrimesAndScale(sp)
            p1 = hx.zerosLike(p0)
            hx.keySwitchDigits(d2, W, p0, p1)
            if Bm[t] is not None:
                p0 *= Bm[t]
                p1 *= Bm[t]
            a0, a1 = c0.copy(), c1.copy()
            if A[t] is not None:
                a0 *= A[t]
                a1 *= A[t]
            a0.addPrimesAndScale(sp)
            a1.addPrimesAndScale(sp)
            a0 += p0
            a1 += p1
            assert np.array_equal(a0.download(), want0[t]) and np.array_equal(a1.download(), want1[t]), t


def test_kernel_takes_the_largest_words(hx):
    """every operand word q - 1 at 60-bit primes, three digits, masks of q - 1: the inner sum is 4 products of (q - 1)^2,
    the outer one 2"""
    m, B, ndig, n = 85, 2, 3, 2
    g = _ring(hx, m, 4)
    assert all(q.bit_length() == 60 for q in g.primes)
    rng = np.random.default_rng(1)
    own, sp = [0, 1, 2], [3]
    allp = own + sp
    dg, dig = _digit_block(hx, g, rng, own, sp, ndig, B, fill="max")
    c0, _ = _rnd(hx, g, rng, own, B, fill="max")
    c1, _ = _rnd(hx, g, rng, own, B, fill="max")
    W, _, _ = _matrix(hx, g, rng, allp, ndig, fill="max")
    A = [_rnd(hx, g, rng, allp, 1, fill="max")[0], _rnd(hx, g, rng, allp, B, fill="max")[0]]
    Bm = [_rnd(hx, g, rng, allp, B, fill="max")[0], _rnd(hx, g, rng, allp, 1, fill="max")[0]]
    psp = _psp(g, allp, sp)
    out0 = [hx.DoubleCRT(g, allp, B) for _ in range(n)]
    out1 = [hx.DoubleCRT(g, allp, B) for _ in range(n)]
    assert _raw(hx, dg, c0, c1, [2, 4], [W, W], A, Bm, sp, out0, out1) == 0, hx.lib().hx_last_error()
    for t in range(n):
        got0, got1 = out0[t].download(), out1[t].download()
        for r, i in enumerate(allp):
            q = g.primes[i]
            own_row = r < len(own)
            in0 = ((psp[r] * (q - 1) if own_row else 0) + ndig * (q - 1) ** 2) % q
            in1 = ndig * (q - 1) ** 2 % q
            pc = psp[r] * (q - 1) % q if own_row else 0
            assert (got0[r] == ((q - 1) * pc + (q - 1) * in0) % q).all(), (t, r)
            assert (got1[r] == ((q - 1) * pc + (q - 1) * in1) % q).all(), (t, r)


def test_refusals_touch_nothing(hx):
    m, B, ndig = 85, 2, 2
    g, other = _ring(hx, m, 5), _ring(hx, m, 5)
    rng = np.random.default_rng(2)
    own, sp = [0, 1], [3]
    allp = own + sp
    dg, dig = _digit_block(hx, g, rng, own, sp, ndig, B)
    c0, r0 = _rnd(hx, g, rng, own, B)
    c1, r1 = _rnd(hx, g, rng, own, B)
    W, b, a = _matrix(hx, g, rng, allp, ndig)
    outs, marks = [], []
    for _ in range(4):
        poly, rows = _rnd(hx, g, rng, allp, B)
        outs.append(poly)
        marks.append(rows)
    out0, out1 = outs[:2], outs[2:]
    mA, rA = _rnd(hx, g, rng, allp, 1)
    mB, rB = _rnd(hx, g, rng, allp, B)
    ks, Ws, A, Bm = [2, 4], [W, W], [mA, None], [mB, mA]
    L = hx.lib()
    INV, UNS, PS = hx.HX_ERR_INVALID, hx.HX_ERR_UNSUPPORTED, hx.HX_ERR_PRIMESET

    def call(dg=dg, c0=c0, c1=c1, ks=ks, Ws=Ws, A=A, Bm=Bm, sp=sp, out0=out0, out1=out1, n=None):
        return _raw(hx, dg, c0, c1, ks, Ws, A, Bm, sp, out0, out1, n)
    null = type("Null", (), {"h": None})()
    for kw in (dict(dg=None), dict(c0=None), dict(c1=None), dict(out0=None), dict(out1=None), dict(Ws=None),
               dict(Ws=[W, null]), dict(out0=[out0[0], null]), dict(out1=[null, out1[1]])):
        assert call(**kw) == INV and b"null" in L.hx_last_error(), kw
    assert L.hx_hoisted_mask_fan(dg.h, c0.h, c1.h, None, _arr(Ws, 2), None, None, 2, None, 0, _arr(out0, 2), _arr(out1, 2)) == INV
    assert call(n=0) == INV and b"at least one term" in L.hx_last_error()
    assert call(ks=[2, 5]) == INV and b"not in Zm*" in L.hx_last_error()                # 5 | 85
    assert call(ks=[2, 85 + 17]) == INV
    oc, _ = _rnd(hx, other, rng, own, B)
    oW = _matrix(hx, other, rng, allp, ndig)[0]
    om, _ = _rnd(hx, other, rng, allp, 1)
    assert call(c1=oc) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(out1=[out1[0], _rnd(hx, other, rng, allp, B)[0]]) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(A=[om, None]) == INV and call(Bm=[mB, om]) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(Ws=[W, oW]) == INV and b"another context" in L.hx_last_error()
    assert call(c1=_rnd(hx, g, rng, own, 3)[0]) == INV and call(c1=_rnd(hx, g, rng, [1, 0], B)[0]) == INV
    assert b"c0 and c1 differ" in L.hx_last_error()
    assert call(dg=_digit_block(hx, g, rng, own, sp, ndig, 3)[0]) == INV and b"batch" in L.hx_last_error()
    assert call(out0=[out0[0], _rnd(hx, g, rng, allp, 1)[0]]) == INV and b"batch" in L.hx_last_error()
    assert call(sp=[4]) == INV and b"digit rows do not match" in L.hx_last_error()       # the block was broken over prime 3
    assert call(sp=[]) == INV and call(sp=[1]) == INV and call(sp=[7]) == INV
    assert call(A=[_rnd(hx, g, rng, allp, 3)[0], None]) == INV and b"neither 1 nor 2" in L.hx_last_error()
    assert call(Bm=[mB, _rnd(hx, g, rng, allp, 3)[0]]) == INV and b"B[1]" in L.hx_last_error()
    assert call(out0=[out0[0], out0[0]]) == INV and call(out0=[out0[0], out1[1]]) == INV
    assert b"two outputs are the same" in L.hx_last_error()
    for kw in (dict(out0=[c0, out0[1]]), dict(out1=[out1[0], dg]), dict(out1=[c1, out1[1]]), dict(out0=[out0[0], mA]),
               dict(out1=[mB, out1[1]])):
        assert call(**kw) == INV and b"also an input or a mask" in L.hx_last_error(), kw
    assert call(Ws=[W, _matrix(hx, g, rng, allp, 1)[0]]) == INV and b"as many columns" in L.hx_last_error()
    assert call(Ws=[W, _matrix(hx, g, rng, [0, 1, 2], ndig)[0]]) == PS and b"prime 3" in L.hx_last_error()
    assert call(A=[_rnd(hx, g, rng, [0, 1, 2], 1)[0], None]) == PS and b"A[0] has no row for prime 3" in L.hx_last_error()
    assert call(Bm=[mB, _rnd(hx, g, rng, [3, 1], B)[0]]) == PS and b"B[1] has no row for prime 0" in L.hx_last_error()
    more = [hx.DoubleCRT(g, allp, B) for _ in range(2 * 257)]
    assert call(ks=[2] * 257, Ws=[W] * 257, A=None, Bm=None, out0=more[:257], out1=more[257:]) == UNS
    assert b"256" in L.hx_last_error()
    empty = [hx.DoubleCRT(g, [], B, zero=False) for _ in range(2)]
    assert call(c0=empty[0], c1=empty[1]) == INV and b"c0 has no rows" in L.hx_last_error()
    # 160 rows and a special prime: one row more than a launch descriptor holds
    big = _ring(hx, m, 161, bits=50)
    wide = [hx.DoubleCRT(big, range(160), B) for _ in range(2)]
    bo = [hx.DoubleCRT(big, [0], B) for _ in range(3)]
    bW = _matrix(hx, big, rng, [0], 1)[0]
    assert call(dg=bo[0], c0=wide[0], c1=wide[1], ks=[2], Ws=[bW], A=None, Bm=None, sp=[160], out0=[bo[1]], out1=[bo[2]]) == UNS
    assert b"too many rows" in L.hx_last_error()
    assert all(x.getIndexSet() == [0] and not x.download().any() for x in bo)
    # an odd number of coefficients: phi(m) is odd for m = 2 only (phi = 1); polys without rows reach the check
    tiny = hx.Context(2)
    assert tiny.phim == 1
    tp = [hx.DoubleCRT(tiny, [], 1, zero=False) for _ in range(5)]
    assert call(dg=tp[0], c0=tp[1], c1=tp[2], ks=[1], Ws=[null], A=None, Bm=None, sp=[], out0=[tp[3]], out1=[tp[4]]) == UNS
    assert b"hx_hoisted_mask_fan needs an even number of coefficients" in L.hx_last_error()
    g.graphBegin()                                                      # a call during a graph capture
    try:
        assert call() == UNS and b"cannot be captured" in L.hx_last_error()
    finally:
        try:
            g.graphEnd().destroy()
        except hx.HxError:
            pass
    for x, keep in zip(outs + [c0, c1, mA, mB], marks + [r0, r1, rA, rB]):
        assert x.getIndexSet() == (own if x in (c0, c1) else allp) and np.array_equal(x.download(), keep)
    assert np.array_equal(dg.download().reshape(dig.shape), dig)
    assert call() == 0, L.hx_last_error()                               # and the context still works
    want0, want1 = RF.hoisted_mask_fan(m, [g.primes[i] for i in allp], 2, _psp(g, allp, sp), dig, r0, r1, ks, [(b, a)] * 2,
                                       [rA, None], [rB, rA])
    for t in range(2):
        assert np.array_equal(out0[t].download(), want0[t]) and np.array_equal(out1[t].download(), want1[t])


# ---- real ciphertexts ----
def _same(x, y):
    wx = {h: (part.getIndexSet(), part.download()) for h, part in x.parts.items()}
    wy = {h: (part.getIndexSet(), part.download()) for h, part in y.parts.items()}
    assert sorted(wx, key=str) == sorted(wy, key=str) == ["1", "s"]
    assert all(wx[h][0] == wy[h][0] and np.array_equal(wx[h][1], wy[h][1]) for h in wx)
    assert (x.lnNoise, x.primeSet, x.ptxtSpace, x.intFactor, x.ptxtMag) == (y.lnNoise, y.primeSet, y.ptxtSpace, y.intFactor, y.ptxtMag)


def _keys(hx, m, p, bits=200, B=3):
    from helib_amd import bgv_gr, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, 1, bits=bits, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=5)
    sk.GenSecKey()
    ea = bgv_gr.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    v = np.random.default_rng(m).integers(0, p, size=(B, ea.size(), ea.getDegree()))
    if not all(ea.nativeDimension(i) for i in range(ea.dimension())):
        v[:, :, 1:] = 0         # a rotation that goes around a non-native dimension applies the Frobenius map: integers stay
    return ea, sk, v


@pytest.fixture
def fan_calls(hx, monkeypatch):
    seen = []
    real = hx.hoistedMaskFan
    monkeypatch.setattr(hx, "hoistedMaskFan", lambda *args: (seen.append(len(args[3])), real(*args))[1])
    return seen


def test_automorph_masked_fused_is_the_sequence(hx, fan_calls):
    from helib_amd import ctxt as hc, replicate as R
    ea, sk, v = _keys(hx, 57, 7)
    ct = ea.encrypt_batch(sk, v)
    ct.multiplyBy(ea.encrypt_batch(sk, v))                              # below the top level
    ct.mulIntFactor(3)
    rng = np.random.default_rng(3)
    enc = [R._encode(ea, rng.integers(0, 2, ea.size())) for _ in range(4)]
    ks = [ea.zMStar.genToPow(0, i) for i in (1, 2, 5)]
    A, B = [enc[0][0], None, enc[1][0]], [enc[2][0], enc[3][0], None]
    sizes = [(enc[0][1], enc[2][1]), (-1.0, -1.0), (enc[1][1], -1.0)]
    seq = hc.BasicAutomorphPrecon(ct).automorphMasked(ks, A, B, sizes, fused=False)
    assert not fan_calls
    one = hc.BasicAutomorphPrecon(ct).automorphMasked(ks, A, B, sizes, fused=True)
    assert fan_calls == [3]
    for x, y in zip(seq, one):
        _same(x, y)


@pytest.mark.parametrize("m,p", [(11, 23), (57, 7)])
def test_replicate_all_in_three_forms(hx, fan_calls, m, p):
    from helib_amd import replicate as R
    ea, sk, v = _keys(hx, m, p)
    ct = ea.encrypt_batch(sk, v)
    ref = R.replicateAll(ea, ct, 64, hoisted=False)
    assert not fan_calls
    seq = R.replicateAll(ea, ct, 64, hoisted=True, fused=False)
    assert not fan_calls
    one = R.replicateAll(ea, ct, 64, hoisted=True, fused=True)
    assert fan_calls and set(fan_calls) <= {1, 2}
    assert len(ref) == len(seq) == len(one) == ea.size()
    for i in range(ea.size()):
        want = R.replicatePlain(v, i, axis=1)
        for form in (ref, seq, one):
            assert form[i].isCorrect() and np.array_equal(ea.decrypt_batch(form[i], sk), want), i
        _same(seq[i], one[i])
