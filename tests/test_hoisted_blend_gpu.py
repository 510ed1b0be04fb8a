"""hx_hoisted_blend on the device against python integers (tests/matmul_full_ref.hoisted_blend), and ctxt.automorphBlend /
matmul_full.MatMulFullExec of real ciphertexts, through the kernel against the calls it replaces.  Everything here is an
integer: every comparison is exact.

The shapes of the kernel tests are those of tests/test_hoisted_sum_gpu.py: phi(m) = 36 (less than a wavefront), 64, 126, 1024
through the closed-form gather of a power of two, and 16384 on 2 + 1 rows (64 workgroup columns, through the table
gather); batch 1 (one element per thread), 2, 3 and 5 (a partial group of four, and a second one); one to three digits;
n = 1, 2, 3; a mask of batch 1 and of the operands' batch; masks and matrices made for exactly the outputs' rows and for
two primes more, their rows in reversed order; and every operand and mask word q - 1 at 60-bit primes with three digits,
the largest value the blend and the accumulators see.

bits of the real chains: tests/test_bgv_hypercube_host.BITS for (527, 2) and (803, 3); (2091, 2) runs at 200 -- on the
CPU oracle the unfused product of a random 32 x 32 matrix decrypts correctly at 100 already, the smallest multiple of 100
(62 bits of capacity left), and the test adds 100 as tests/test_replicate_host.py does."""
import ctypes as C

import numpy as np
import pytest

from tests import matmul_full_ref as MR
from tests import thin_ref as TR
from tests.test_hoisted_sum_gpu import _digit_block, _frob, _matrix, _psp, _ring, _rnd

pytestmark = pytest.mark.gpu

BITS = {(527, 2): 500, (803, 3): 600, (2091, 2): 200}


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


def _raw(hx, dA, a0, a1, dB, b0, b1, ks, Ws, M, sp, out0, out1, n=None):
    n = len(ks) if n is None else n
    ka = np.array([int(k) for k in ks] or [0], dtype=np.uint64)
    spa = np.array(list(sp) or [0], dtype=np.int32)
    h = lambda x: x.h if x is not None else None                        # noqa: E731
    return hx.lib().hx_hoisted_blend(h(dA), h(a0), h(a1), h(dB), h(b0), h(b1), ka.ctypes.data_as(C.c_void_p), _arr(Ws, n),
                                     _arr(M, n), n, spa.ctypes.data_as(C.c_void_p), len(sp), _arr(out0, n), _arr(out1, n))


#        m, p, own rows, special rows, batch, digits, extra rows of the matrices and masks, per term the mask: one / per
CASES = [(57, 7, 2, 1, 1, 2, 0, ["one", "one"]),
         (85, 2, 3, 2, 3, 3, 0, ["per", "one", "per"]),
         (127, 2, 2, 1, 2, 1, 2, ["per", "one", "per"]),
         (2048, 3, 2, 1, 3, 2, 0, ["one", "per"]),
         (2048, 5, 3, 1, 5, 2, 2, ["per"]),
         (21845, 2, 2, 1, 2, 2, 0, ["per", "one"]),
         (85, 2, 2, 1, 1, 2, 2, ["one"])]


@pytest.mark.parametrize("m,p,L,nsp,B,ndig,extra,kinds", CASES)
def test_kernel_against_python_integers(hx, m, p, L, nsp, B, ndig, extra, kinds):
    g = _ring(hx, m, L + nsp + extra)
    N = g.phim
    n = len(kinds)
    rng = np.random.default_rng(m + 10 * B + n)
    # with extra rows the operands sit below the matrices' level: they hold primes 1 .. L, the matrices and masks 0 .. L + 1
    own = list(range(1, L + 1)) if extra else list(range(L))
    sp = list(range(L + extra, L + extra + nsp))
    allp = own + sp
    nall = len(allp)
    ks = _frob(m, p)[:n]
    assert len(ks) == n
    dA, digA = _digit_block(hx, g, rng, own, sp, ndig, B)
    dB, digB = _digit_block(hx, g, rng, own, sp, ndig, B)
    ins = [_rnd(hx, g, rng, own, B) for _ in range(4)]                  # a0, a1, b0, b1
    (a0, ra0), (a1, _), (b0, rb0), (b1, _) = ins
    wrows = list(range(L + extra + nsp))[::-1] if extra else allp       # another order, and primes the operands lack
    sel = [wrows.index(i) for i in allp]
    Ws, keys = [], []
    for _ in ks:
        W, b, a = _matrix(hx, g, rng, wrows, ndig + (1 if extra else 0))
        Ws.append(W)
        keys.append((b[:ndig][:, sel], a[:ndig][:, sel]))
    masks = [_rnd(hx, g, rng, wrows, B if kind == "per" else 1) for kind in kinds]
    M, Mr = [x[0] for x in masks], [x[1][sel] for x in masks]
    psp = _psp(g, allp, sp)
    want0, want1 = MR.hoisted_blend(m, [g.primes[i] for i in allp], L, psp, digA, ra0, digB, rb0, ks, keys, Mr)
    # one word by hand: the last term, row 0, element B - 1, word N - 1
    t, q, x = n - 1, g.primes[allp[0]], int(TR.perm(m, ks[-1])[N - 1])
    X0 = psp[0] * int(ra0[0, B - 1, x]) + sum(int(digA[j, 0, B - 1, x]) * int(keys[t][0][j][0][N - 1]) for j in range(ndig))
    Y0 = psp[0] * int(rb0[0, B - 1, x]) + sum(int(digB[j, 0, B - 1, x]) * int(keys[t][0][j][0][N - 1]) for j in range(ndig))
    mk = int(Mr[t][0, -1, N - 1])
    assert int(want0[t][0, B - 1, N - 1]) == (mk * X0 + Y0 - mk * Y0) % q
    out0 = [_rnd(hx, g, rng, [own[0]], B)[0] for _ in range(n)]         # (reshaped and overwritten, not read)
    out1 = [hx.DoubleCRT(g, allp, B) for _ in range(n)]
    assert _raw(hx, dA, a0, a1, dB, b0, b1, ks, Ws, M, sp, out0, out1) == 0, hx.lib().hx_last_error()
    for t in range(n):
        assert out0[t].getIndexSet() == allp == out1[t].getIndexSet()
        for got, want in ((out0[t].download(), want0[t]), (out1[t].download(), want1[t])):
            assert got.shape == (nall, B, N)
            bad = np.argwhere(got != want)
            assert not len(bad), "term %d: %d words differ, the first at [row, element, word] %s" % (t, len(bad), bad[0])
            assert all((got[r] < g.primes[i]).all() for r, i in enumerate(allp))
    # the inputs and the masks are left as they were
    assert all(np.array_equal(poly.download(), rows) for poly, rows in ins)
    assert np.array_equal(dA.download().reshape(digA.shape), digA) and np.array_equal(dB.download().reshape(digB.shape), digB)
    assert all(np.array_equal(poly.download(), rows) for poly, rows in masks)
    # the binding: new outputs; an output that still shares an input's rows (a lazy copy) lets go of them
    o0, o1 = hx.hoistedBlend(dA, a0, a1, dB, b0, b1, ks, Ws, M, sp)
    assert all(o0[t].getIndexSet() == allp and np.array_equal(o0[t].download(), want0[t])
               and np.array_equal(o1[t].download(), want1[t]) for t in range(n))
    lazy = [b0.copy()] + out0[1:]
    assert _raw(hx, dA, a0, a1, dB, b0, b1, ks, Ws, M, sp, lazy, out1) == 0
    assert np.array_equal(lazy[0].download(), want0[0]) and np.array_equal(b0.download(), rb0)
    if m == 85 and B == 3:                                              # the second witness: the calls the kernel replaces
        for t, (k, W) in enumerate(zip(ks, Ws)):
            res = []
            for dg, c0 in ((dA, a0), (dB, b0)):
                d2, p0 = dg.copy(), c0.copy()
                d2.automorph(k)
                p0.automorph(k)
                p0.addPrimesAndScale(sp)
                p1 = hx.zerosLike(p0)
                hx.keySwitchDigits(d2, W, p0, p1)
                res.append((p0, p1))
            (x0, x1), (y0, y1) = res
            hx.maskBlend(x0, x1, y0, y1, M[t])
            assert np.array_equal(x0.download(), want0[t]) and np.array_equal(x1.download(), want1[t]), t


def test_kernel_takes_the_largest_words(hx):
    """every operand and mask word q - 1 at 60-bit primes, three digits: the blend is (q - 1)(x + q - y) + y with x = y =
    q - 1, a blended word of q - 1, and the sum is 4 products of (q - 1)^2; then x = q - 1 against y = 0, the largest
    product the blend forms, (q - 1)(2 q - 1)"""
    m, B, ndig, n = 85, 2, 3, 2
    g = _ring(hx, m, 4)
    assert all(q.bit_length() == 60 for q in g.primes)
    rng = np.random.default_rng(1)
    own, sp = [0, 1, 2], [3]
    allp = own + sp
    dA, _ = _digit_block(hx, g, rng, own, sp, ndig, B, fill="max")
    ops = [_rnd(hx, g, rng, own, B, fill="max")[0] for _ in range(4)]
    W, _, _ = _matrix(hx, g, rng, allp, ndig, fill="max")
    M = [_rnd(hx, g, rng, allp, 1, fill="max")[0], _rnd(hx, g, rng, allp, B, fill="max")[0]]
    psp = _psp(g, allp, sp)
    zeros, _ = _digit_block(hx, g, rng, own, sp, ndig, B)
    zeros.upload(np.zeros((len(allp) * ndig, B, g.phim), dtype=np.uint64))
    z0 = hx.DoubleCRT(g, own, B)
    for dB, b0, y in ((dA, ops[2], None), (zeros, z0, 0)):
        out0 = [hx.DoubleCRT(g, allp, B) for _ in range(n)]
        out1 = [hx.DoubleCRT(g, allp, B) for _ in range(n)]
        assert _raw(hx, dA, ops[0], ops[1], dB, b0, ops[3], [2, 4], [W, W], M, sp, out0, out1) == 0, hx.lib().hx_last_error()
        for t in range(n):
            got0, got1 = out0[t].download(), out1[t].download()
            for r, i in enumerate(allp):
                q = g.primes[i]
                yy = q - 1 if y is None else y
                z = ((q - 1) * (q - 1) + yy - (q - 1) * yy) % q
                assert (got0[r] == ((psp[r] * z if r < len(own) else 0) + ndig * z * (q - 1)) % q).all(), (t, r)
                assert (got1[r] == ndig * z * (q - 1) % q).all(), (t, r)


def test_refusals_touch_nothing(hx):
    m, B, ndig = 85, 2, 2
    g, other = _ring(hx, m, 5), _ring(hx, m, 5)
    rng = np.random.default_rng(2)
    own, sp = [0, 1], [3]
    allp = own + sp
    dA, digA = _digit_block(hx, g, rng, own, sp, ndig, B)
    dB, digB = _digit_block(hx, g, rng, own, sp, ndig, B)
    (a0, ra0), (a1, ra1), (b0, rb0), (b1, rb1) = [_rnd(hx, g, rng, own, B) for _ in range(4)]
    W, b, a = _matrix(hx, g, rng, allp, ndig)
    outs, marks = [], []
    for _ in range(4):
        poly, rows = _rnd(hx, g, rng, allp, B)
        outs.append(poly)
        marks.append(rows)
    out0, out1 = outs[:2], outs[2:]
    mA, rA = _rnd(hx, g, rng, allp, 1)
    mB, rB = _rnd(hx, g, rng, allp, B)
    ks, Ws, M = [2, 4], [W, W], [mA, mB]
    L = hx.lib()
    INV, UNS, PS = hx.HX_ERR_INVALID, hx.HX_ERR_UNSUPPORTED, hx.HX_ERR_PRIMESET

    def call(dA=dA, a0=a0, a1=a1, dB=dB, b0=b0, b1=b1, ks=ks, Ws=Ws, M=M, sp=sp, out0=out0, out1=out1, n=None):
        return _raw(hx, dA, a0, a1, dB, b0, b1, ks, Ws, M, sp, out0, out1, n)
    null = type("Null", (), {"h": None})()
    for kw in (dict(dA=None), dict(a0=None), dict(a1=None), dict(dB=None), dict(b0=None), dict(b1=None), dict(out0=None),
               dict(out1=None), dict(Ws=None), dict(M=None), dict(Ws=[W, null]), dict(M=[mA, null]),
               dict(out0=[out0[0], null]), dict(out1=[null, out1[1]])):
        assert call(**kw) == INV and b"null" in L.hx_last_error(), kw
    assert L.hx_hoisted_blend(dA.h, a0.h, a1.h, dB.h, b0.h, b1.h, None, _arr(Ws, 2), _arr(M, 2), 2, None, 0, _arr(out0, 2),
                              _arr(out1, 2)) == INV
    assert call(n=0) == INV and b"at least one term" in L.hx_last_error()
    assert call(ks=[2, 5]) == INV and b"not in Zm*" in L.hx_last_error()                # 5 | 85
    assert call(ks=[2, 85 + 17]) == INV
    oc, _ = _rnd(hx, other, rng, own, B)
    oW = _matrix(hx, other, rng, allp, ndig)[0]
    om, _ = _rnd(hx, other, rng, allp, 1)
    assert call(a1=oc) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(b0=oc) == INV and call(dB=_digit_block(hx, other, rng, own, sp, ndig, B)[0]) == INV
    assert b"incompatible objects" in L.hx_last_error()
    assert call(out1=[out1[0], _rnd(hx, other, rng, allp, B)[0]]) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(M=[om, mB]) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(Ws=[W, oW]) == INV and b"another context" in L.hx_last_error()
    assert call(a1=_rnd(hx, g, rng, own, 3)[0]) == INV and call(a1=_rnd(hx, g, rng, [1, 0], B)[0]) == INV
    assert b"a0 and a1 differ" in L.hx_last_error()
    for kw in (dict(b0=_rnd(hx, g, rng, own, 3)[0]), dict(b1=_rnd(hx, g, rng, [1, 0], B)[0]), dict(b0=_rnd(hx, g, rng, [0, 1, 2], B)[0])):
        assert call(**kw) == INV and b"the two operands differ" in L.hx_last_error(), kw
    assert call(dA=_digit_block(hx, g, rng, own, sp, ndig, 3)[0]) == INV and b"batch" in L.hx_last_error()
    assert call(dB=_digit_block(hx, g, rng, own, sp, 1, B)[0]) == INV and b"number of digits" in L.hx_last_error()
    assert call(out0=[out0[0], _rnd(hx, g, rng, allp, 1)[0]]) == INV and b"batch" in L.hx_last_error()
    assert call(sp=[4]) == INV and b"digit rows do not match" in L.hx_last_error()       # the blocks were broken over prime 3
    assert call(dB=_digit_block(hx, g, rng, own, [4], ndig, B)[0]) == INV and b"digit rows do not match" in L.hx_last_error()
    assert call(sp=[]) == INV and call(sp=[1]) == INV and call(sp=[7]) == INV
    assert call(M=[_rnd(hx, g, rng, allp, 3)[0], mB]) == INV and b"neither 1 nor 2" in L.hx_last_error()
    assert call(out0=[out0[0], out0[0]]) == INV and call(out0=[out0[0], out1[1]]) == INV
    assert b"two outputs are the same" in L.hx_last_error()
    for kw in (dict(out0=[a0, out0[1]]), dict(out1=[out1[0], dA]), dict(out1=[b1, out1[1]]), dict(out0=[out0[0], dB]),
               dict(out0=[out0[0], mA]), dict(out1=[mB, out1[1]])):
        assert call(**kw) == INV and b"also an input or a mask" in L.hx_last_error(), kw
    assert call(Ws=[W, _matrix(hx, g, rng, allp, 1)[0]]) == INV and b"as many columns" in L.hx_last_error()
    assert call(Ws=[W, _matrix(hx, g, rng, [0, 1, 2], ndig)[0]]) == PS and b"prime 3" in L.hx_last_error()
    assert call(M=[_rnd(hx, g, rng, [0, 1, 2], 1)[0], mB]) == PS and b"M[0] has no row for prime 3" in L.hx_last_error()
    assert call(M=[mA, _rnd(hx, g, rng, [3, 1], B)[0]]) == PS and b"M[1] has no row for prime 0" in L.hx_last_error()
    more = [hx.DoubleCRT(g, allp, B) for _ in range(2 * 257)]
    assert call(ks=[2] * 257, Ws=[W] * 257, M=[mA] * 257, out0=more[:257], out1=more[257:]) == UNS
    assert b"256" in L.hx_last_error()
    empty = [hx.DoubleCRT(g, [], B, zero=False) for _ in range(4)]
    assert call(a0=empty[0], a1=empty[1], b0=empty[2], b1=empty[3]) == INV and b"a0 has no rows" in L.hx_last_error()
    # 160 rows and a special prime: one row more than a launch descriptor holds
    big = _ring(hx, m, 161, bits=50)
    wide = [hx.DoubleCRT(big, range(160), B) for _ in range(4)]
    bo = [hx.DoubleCRT(big, [0], B) for _ in range(5)]
    bW = _matrix(hx, big, rng, [0], 1)[0]
    assert call(dA=bo[0], a0=wide[0], a1=wide[1], dB=bo[1], b0=wide[2], b1=wide[3], ks=[2], Ws=[bW], M=[bo[2]], sp=[160],
                out0=[bo[3]], out1=[bo[4]]) == UNS
    assert b"too many rows" in L.hx_last_error()
    assert all(x.getIndexSet() == [0] and not x.download().any() for x in bo)
    # an odd number of coefficients: phi(m) is odd for m = 2 only (phi = 1); polys without rows reach the check
    tiny = hx.Context(2)
    assert tiny.phim == 1
    tp = [hx.DoubleCRT(tiny, [], 1, zero=False) for _ in range(9)]
    assert call(dA=tp[0], a0=tp[1], a1=tp[2], dB=tp[3], b0=tp[4], b1=tp[5], ks=[1], Ws=[null], M=[tp[6]], sp=[], out0=[tp[7]],
                out1=[tp[8]]) == UNS
    assert b"hx_hoisted_blend needs an even number of coefficients" in L.hx_last_error()
    g.graphBegin()                                                      # a call during a graph capture
    try:
        assert call() == UNS and b"cannot be captured" in L.hx_last_error()
    finally:
        try:
            g.graphEnd().destroy()
        except hx.HxError:
            pass
    own_ins = (a0, a1, b0, b1)
    for x, keep in zip(outs + [a0, a1, b0, b1, mA, mB], marks + [ra0, ra1, rb0, rb1, rA, rB]):
        assert x.getIndexSet() == (own if x in own_ins else allp) and np.array_equal(x.download(), keep)
    assert np.array_equal(dA.download().reshape(digA.shape), digA) and np.array_equal(dB.download().reshape(digB.shape), digB)
    assert call() == 0, L.hx_last_error()                               # and the context still works
    want0, want1 = MR.hoisted_blend(m, [g.primes[i] for i in allp], 2, _psp(g, allp, sp), digA, ra0, digB, rb0, ks,
                                    [(b, a)] * 2, [rA, rB])
    for t in range(2):
        assert np.array_equal(out0[t].download(), want0[t]) and np.array_equal(out1[t].download(), want1[t])


# ---- real ciphertexts ----
def _same(x, y):
    wx = {h: (part.getIndexSet(), part.download()) for h, part in x.parts.items()}
    wy = {h: (part.getIndexSet(), part.download()) for h, part in y.parts.items()}
    assert sorted(wx, key=str) == sorted(wy, key=str) == ["1", "s"]
    assert all(wx[h][0] == wy[h][0] and np.array_equal(wx[h][1], wy[h][1]) for h in wx)
    assert (x.lnNoise, x.primeSet, x.ptxtSpace, x.intFactor, x.ptxtMag) == (y.lnNoise, y.primeSet, y.ptxtSpace, y.intFactor, y.ptxtMag)


def _keys(hx, m, p, B=3):
    from helib_amd import bgv_hypercube, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, 1, bits=BITS[m, p], c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=5)
    sk.GenSecKey()
    ea = bgv_hypercube.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    assert all(hk.getKSStrategy(sk, i) == hk.HELIB_KSS_FULL for i in range(ea.dimension()))
    return ea, sk, np.random.default_rng(m).integers(0, p, size=(B, ea.size()))


@pytest.fixture
def blend_calls(hx, monkeypatch):
    seen = []
    real = hx.hoistedBlend
    monkeypatch.setattr(hx, "hoistedBlend", lambda *args: (seen.append(len(args[6])), real(*args))[1])
    return seen


def test_automorph_blend_fused_is_the_sequence(hx, blend_calls):
    """(527, 2), dimension 0: native, six coordinates -- the blend of two rotated ciphertexts under masks of dimension 0
    does not depend on what the second operand is, so ct1 is simply another ciphertext, below the top level like ct"""
    from helib_amd import ctxt as hc
    ea, sk, v = _keys(hx, 527, 2)
    ct = ea.encrypt_batch(sk, v)
    ct.multiplyBy(ea.encrypt_batch(sk, v))
    ct.cleanUp()
    ct.modDownToSet(ct.primeSet - {max(ct.primeSet)})              # below the top level
    assert set(ea.cc.ctxtPrimes) > set(ct.primeSet)
    ct1 = ct.clone()
    ct1.smartAutomorph(ea.zMStar.genToPow(1, 1))
    ct1.cleanUp()
    z = ea.zMStar
    offs = [1, 2, 5]
    ks = [z.genToPow(0, i) for i in offs]
    idx = set(ea.cc.ctxtPrimes) | set(ea.cc.specialPrimes)
    enc = [ea._encodedMask(ea.maskSlots(0, i), idx) for i in offs]
    masks, sizes = [mk for mk, _ in enc], [enc[0][1], -1.0, enc[2][1]]
    seq = hc.automorphBlend(hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1), ks, masks, sizes, fused=False)
    assert not blend_calls
    one = hc.automorphBlend(hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1), ks, masks, sizes, fused=True)
    assert blend_calls == [3]
    for x, y in zip(seq, one):
        _same(x, y)


@pytest.mark.parametrize("m,p,terms", [(527, 2, [1]), (2091, 2, [3])])
def test_matmul_full_in_three_forms(hx, blend_calls, monkeypatch, m, p, terms):
    """the four-call sequence (fused=False), the sequence with hx_mask_blend (fused=None with Ctxt.fuseHoistedBlend off:
    EncryptedArray.fuseMaskBlend) and hx_hoisted_blend (fused=True, and fused=None as the switch ships): each against
    mulPlain, and all against the first word for word"""
    from helib_amd import bgv_matmul as bm, ctxt as hc, matmul_full as mf
    ea, sk, v = _keys(hx, m, p)
    assert type(ea).fuseMaskBlend is True
    n = ea.size()
    A = np.random.default_rng(m + 1).integers(0, p, size=(n, n))
    mat = bm.MatMulFull(ea, A)
    ex = mf.MatMulFullExec(ea, mat)
    want = bm.mulPlain(ea, v, mat)
    mb = []
    real = hx.maskBlend
    monkeypatch.setattr(hx, "maskBlend", lambda *args: (mb.append(1), real(*args))[1])
    fresh, out = ea.encrypt_batch(sk, v), {}
    assert hc.Ctxt.fuseHoistedBlend is True
    for form, fused, switch in (("four calls", False, True), ("mask blend", None, False), ("hoisted", True, False),
                                ("as shipped", None, True)):
        monkeypatch.setattr(hc.Ctxt, "fuseHoistedBlend", switch)
        del mb[:], blend_calls[:]
        ct = fresh.clone()
        assert ex.mul(ct, pk=sk, fused=fused) is ct
        assert np.array_equal(ea.decrypt_batch(ct, sk), want) and ct.isCorrect(), form
        assert blend_calls == (terms if form in ("hoisted", "as shipped") else []), form
        assert bool(mb) == (form == "mask blend"), form
        out[form] = ct
    for form in ("mask blend", "hoisted", "as shipped"):
        _same(out["four calls"], out[form])


def test_unequal_int_factors_give_the_sequence(hx, blend_calls):
    """(803, 3): the fused request gives the sequence's ciphertext, whether the key switch left equal intFactors (one
    hx_hoisted_blend) or not (none)"""
    from helib_amd import bgv_matmul as bm, matmul_full as mf
    m, p = 803, 3
    ea, sk, v = _keys(hx, m, p)
    n = ea.size()
    mat = bm.MatMulFull(ea, np.random.default_rng(m + 1).integers(0, p, size=(n, n)))
    ex = mf.MatMulFullExec(ea, mat)
    fresh, out = ea.encrypt_batch(sk, v), {}
    for fused in (False, True):
        ct = fresh.clone()
        ex.mul(ct, pk=sk, fused=fused)
        assert np.array_equal(ea.decrypt_batch(ct, sk), bm.mulPlain(ea, v, mat)) and ct.isCorrect(), fused
        out[fused] = ct
    assert blend_calls in ([], [1])
    _same(out[False], out[True])
