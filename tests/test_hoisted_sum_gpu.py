"""hx_hoisted_automorph_sum on the device against python integers (tests/thin_ref.hoisted_sum), and
BasicAutomorphPrecon.automorphSum / traceMap of a real ciphertext, fused against the loop.  Everything here is an integer:
every comparison is exact.

The shapes of the kernel tests: phi(m) = 36 (less than a wavefront), 64, 126, 1024 through the closed-form gather of a
power of two, and 16384 on 2 + 1 rows (64 workgroup columns, through the table gather); batch 1 (one element per thread),
2, 3 and 5 (a partial group of four, and a second one); one to three digits; n = 1 and the d - 1 powers of p; matrices made
for exactly the operand's rows and for two primes and one digit more, their rows in another order; 85 terms of two digits
with every word q - 1 at 60-bit primes -- the 256 products the accumulators take -- and 86 refused."""
import ctypes as C

import numpy as np
import pytest

from helib_amd import hostnt

from tests import thin_ref as TR

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


def _ring(hx, m, nprimes, bits=60):
    g = hx.Context(m)
    gen = hostnt.PrimeGen(bits, m)
    for _ in range(nprimes):
        g.add_prime(gen.next())
    return g


def _rnd(hx, g, rng, idx, B, fill=None):
    rows = np.stack([np.full((B, g.phim), g.primes[i] - 1, dtype=np.uint64) if fill == "max" else
                     rng.integers(0, g.primes[i], size=(B, g.phim), dtype=np.uint64) for i in idx])
    return hx.DoubleCRT(g, list(idx), B, rows), rows


def _digit_block(hx, g, rng, own, sp, ndig, B, fill=None):
    """a digit block of the shape hx_break_into_digits leaves (ndig digits on own + sp), holding random words"""
    part, _ = _rnd(hx, g, rng, own, B)
    per = -(-len(own) // ndig)
    digits = [own[i:i + per] for i in range(0, len(own), per)]
    assert len(digits) == ndig
    dg = part.breakIntoDigits(digits, sp)
    allp = list(own) + list(sp)
    assert dg.getIndexSet() == allp * ndig
    rows = np.stack([np.full((B, g.phim), g.primes[i] - 1, dtype=np.uint64) if fill == "max" else
                     rng.integers(0, g.primes[i], size=(B, g.phim), dtype=np.uint64) for i in allp * ndig])
    dg.upload(rows)
    return dg, rows.reshape(ndig, len(allp), B, g.phim)


def _matrix(hx, g, rng, row_idx, ndig, fill=None):
    shape = (ndig, len(row_idx), g.phim)
    if fill == "max":
        b = np.stack([np.stack([np.full(g.phim, g.primes[i] - 1, dtype=np.uint64) for i in row_idx])] * ndig)
        a = b.copy()
    else:
        b = np.stack([np.stack([rng.integers(0, g.primes[i], size=g.phim, dtype=np.uint64) for i in row_idx]) for _ in range(ndig)])
        a = np.stack([np.stack([rng.integers(0, g.primes[i], size=g.phim, dtype=np.uint64) for i in row_idx]) for _ in range(ndig)])
    assert b.shape == shape
    return hx.KeySwitch(g, list(row_idx), b, a), b, a


def _raw(hx, dg, c0, c1, ks, Ws, sp, out0, out1, n=None):
    n = len(ks) if n is None else n
    ka = np.array([int(k) for k in ks] or [0], dtype=np.uint64)
    wa = (C.c_void_p * max(len(Ws), 1))(*[getattr(W, "h", None) for W in Ws])
    spa = np.array(list(sp) or [0], dtype=np.int32)
    h = lambda x: x.h if x is not None else None                        # noqa: E731
    return hx.lib().hx_hoisted_automorph_sum(h(dg), h(c0), h(c1), ka.ctypes.data_as(C.c_void_p), wa, n,
                                             spa.ctypes.data_as(C.c_void_p), len(sp), h(out0), h(out1))


def _psp(g, allp, sp):
    out = []
    for i in allp:
        f = 1
        for s in sp:
            f = f * g.primes[s] % g.primes[i]
        out.append(f)
    return out


def _frob(m, p):
    ks, k = [], p % m
    while k != 1:
        ks.append(k)
        k = k * p % m
    return ks


#        m, p, own rows, special rows, batch, digits, n (None: every power of p but 1), the matrices' extra rows and digits
CASES = [(57, 7, 2, 1, 1, 2, None, 0), (85, 2, 3, 2, 3, 3, None, 0), (127, 2, 2, 1, 2, 1, None, 2),
         (2048, 3, 2, 1, 3, 2, 5, 0), (2048, 5, 3, 1, 5, 2, 1, 2), (21845, 2, 2, 1, 2, 2, 3, 0), (85, 2, 2, 1, 1, 2, 1, 2)]


@pytest.mark.parametrize("m,p,L,nsp,B,ndig,n,extra", CASES)
def test_kernel_against_python_integers(hx, m, p, L, nsp, B, ndig, n, extra):
    g = _ring(hx, m, L + nsp + extra)
    N = g.phim
    rng = np.random.default_rng(m + 10 * B + n if n else m)
    # with extra rows the operand sits below the matrices' level: it holds primes 1 .. L, the matrices 0 .. L + 1
    own = list(range(1, L + 1)) if extra else list(range(L))
    sp = list(range(L + extra, L + extra + nsp))
    allp = own + sp
    ks = _frob(m, p)
    ks = ks if n is None else ks[:n]
    assert ks and len(ks) * (ndig + 1) + 1 <= 256
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
    want0, want1 = TR.hoisted_sum(m, [g.primes[i] for i in allp], L, _psp(g, allp, sp), dig, r0, r1, ks, keys)
    # one word by hand: row 0, element B - 1, word N - 1
    q, pm = g.primes[allp[0]], [TR.perm(m, k) for k in ks]
    w = _psp(g, allp, sp)[0] * (int(r0[0, B - 1, N - 1]) + sum(int(r0[0, B - 1, x[N - 1]]) for x in pm))
    w += sum(int(dig[j, 0, B - 1, x[N - 1]]) * int(kb[j][0][N - 1]) for x, (kb, _) in zip(pm, keys) for j in range(ndig))
    assert int(want0[0, B - 1, N - 1]) == w % q
    out0, marked = _rnd(hx, g, rng, [own[0]], B)                        # (reshaped and overwritten, not read)
    out1 = hx.DoubleCRT(g, allp, B)
    assert _raw(hx, dg, c0, c1, ks, Ws, sp, out0, out1) == 0, hx.lib().hx_last_error()
    assert out0.getIndexSet() == allp == out1.getIndexSet()
    for got, want in ((out0.download(), want0), (out1.download(), want1)):
        bad = np.argwhere(got != want)
        assert not len(bad), "%d words differ, the first at [row, element, word] %s" % (len(bad), bad[0])
    assert np.array_equal(c0.download(), r0) and np.array_equal(c1.download(), r1)      # the inputs are left as they were
    assert np.array_equal(dg.download().reshape(dig.shape), dig)
    # the binding: new outputs; an output that still shares an input's rows (a lazy copy) lets go of them
    o0, o1 = hx.hoistedAutomorphSum(dg, c0, c1, ks, Ws, sp)
    assert o0.getIndexSet() == allp and np.array_equal(o0.download(), want0) and np.array_equal(o1.download(), want1)
    lazy = c0.copy()
    assert _raw(hx, dg, c0, c1, ks, Ws, sp, lazy, out1) == 0
    assert np.array_equal(lazy.download(), want0) and np.array_equal(c0.download(), r0)
    if m == 85 and B == 3:                                              # the second witness: the calls the kernel replaces
        acc0, acc1 = c0.copy(), c1.copy()
        acc0.addPrimesAndScale(sp)
        acc1.addPrimesAndScale(sp)
        for k, W in zip(ks, Ws):
            d2, p0 = dg.copy(), c0.copy()
            d2.automorph(k)
            p0.automorph(k)
            p0.addPrimesAndScale(sp)
            p1 = hx.zerosLike(p0)
            hx.keySwitchDigits(d2, W, p0, p1)
            acc0 += p0
            acc1 += p1
        assert np.array_equal(acc0.download(), want0) and np.array_equal(acc1.download(), want1)


def test_kernel_takes_256_products_of_the_largest_words(hx):
    """n = 85 terms of two digits: 1 + 85 + 170 = 256 products in a word of out0, every operand q - 1 at 60-bit primes;
    one term more is refused and leaves the outputs as they were"""
    m, L, nsp, B, ndig, n = 85, 2, 1, 2, 2, 85
    g = _ring(hx, m, L + nsp)
    assert all(q.bit_length() == 60 for q in g.primes)
    rng = np.random.default_rng(1)
    own, sp = [0, 1], [2]
    allp = own + sp
    dg, dig = _digit_block(hx, g, rng, own, sp, ndig, B, fill="max")
    c0, r0 = _rnd(hx, g, rng, own, B, fill="max")
    c1, r1 = _rnd(hx, g, rng, own, B, fill="max")
    W, b, a = _matrix(hx, g, rng, allp, ndig, fill="max")
    ks = (_frob(m, 2) * 13)[:n]
    assert len(ks) == n and n * (ndig + 1) + 1 == 256
    psp = _psp(g, allp, sp)
    out0, out1 = hx.DoubleCRT(g, allp, B), hx.DoubleCRT(g, allp, B)
    assert _raw(hx, dg, c0, c1, ks, [W] * n, sp, out0, out1) == 0, hx.lib().hx_last_error()
    got0, got1 = out0.download(), out1.download()
    for r, i in enumerate(allp):
        q = g.primes[i]
        dd = n * ndig * (q - 1) ** 2
        assert (got0[r] == ((psp[r] * (n + 1) * (q - 1) if r < L else 0) + dd) % q).all()
        assert (got1[r] == ((psp[r] * (q - 1) if r < L else 0) + dd) % q).all()
    assert _raw(hx, dg, c0, c1, ks + ks[:1], [W] * (n + 1), sp, out0, out1) == hx.HX_ERR_UNSUPPORTED
    assert b"256" in hx.lib().hx_last_error()
    assert np.array_equal(out0.download(), got0) and np.array_equal(out1.download(), got1)


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
    out0, m0 = _rnd(hx, g, rng, allp, B)
    out1, m1 = _rnd(hx, g, rng, allp, B)
    ks, Ws = [2, 4], [W, W]
    L = hx.lib()
    INV, UNS, PS = hx.HX_ERR_INVALID, hx.HX_ERR_UNSUPPORTED, hx.HX_ERR_PRIMESET

    def call(dg=dg, c0=c0, c1=c1, ks=ks, Ws=Ws, sp=sp, out0=out0, out1=out1, n=None):
        return _raw(hx, dg, c0, c1, ks, Ws, sp, out0, out1, n)
    null = type("Null", (), {"h": None})()
    for kw in (dict(dg=None), dict(c0=None), dict(c1=None), dict(out0=None), dict(out1=None), dict(Ws=[W, null])):
        assert call(**kw) == INV and b"null" in L.hx_last_error(), kw
    assert L.hx_hoisted_automorph_sum(dg.h, c0.h, c1.h, None, None, 2, None, 0, out0.h, out1.h) == INV
    assert call(n=0) == INV and b"at least one term" in L.hx_last_error()
    assert call(ks=[2, 5]) == INV and b"not in Zm*" in L.hx_last_error()                # 5 | 85
    assert call(ks=[2, 85 + 17]) == INV
    oc, _ = _rnd(hx, other, rng, own, B)
    oW = _matrix(hx, other, rng, allp, ndig)[0]
    assert call(c1=oc) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(out1=_rnd(hx, other, rng, allp, B)[0]) == INV
    assert call(Ws=[W, oW]) == INV and b"another context" in L.hx_last_error()
    assert call(c1=_rnd(hx, g, rng, own, 3)[0]) == INV and call(c1=_rnd(hx, g, rng, [1, 0], B)[0]) == INV
    assert call(dg=_digit_block(hx, g, rng, own, sp, ndig, 3)[0]) == INV and b"batch" in L.hx_last_error()
    assert call(out0=_rnd(hx, g, rng, allp, 1)[0]) == INV and b"batch" in L.hx_last_error()
    assert call(sp=[4]) == INV and b"digit rows do not match" in L.hx_last_error()       # the block was broken over prime 3
    assert call(sp=[]) == INV and call(sp=[1]) == INV and call(sp=[7]) == INV
    assert call(out0=out1) == INV and call(out0=c0) == INV and call(out1=dg) == INV and call(out1=c1) == INV
    assert b"also an input" in L.hx_last_error()
    assert call(Ws=[W, _matrix(hx, g, rng, allp, 1)[0]]) == INV and b"as many columns" in L.hx_last_error()
    assert call(Ws=[W, _matrix(hx, g, rng, [0, 1, 2], ndig)[0]]) == PS and b"prime 3" in L.hx_last_error()
    assert call(ks=[2] * 86, Ws=[W] * 86) == UNS and b"256" in L.hx_last_error()
    empty = [hx.DoubleCRT(g, [], B, zero=False) for _ in range(2)]
    assert call(c0=empty[0], c1=empty[1]) == INV and b"c0 has no rows" in L.hx_last_error()
    # 160 rows and a special prime: one row more than a launch descriptor holds
    big = _ring(hx, m, 161, bits=50)
    wide = [hx.DoubleCRT(big, range(160), B) for _ in range(2)]
    bo = [hx.DoubleCRT(big, [0], B) for _ in range(3)]
    bW = _matrix(hx, big, rng, [0], 1)[0]
    assert call(dg=bo[0], c0=wide[0], c1=wide[1], ks=[2], Ws=[bW], sp=[160], out0=bo[1], out1=bo[2]) == UNS
    assert b"too many rows" in L.hx_last_error()
    assert all(x.getIndexSet() == [0] and not x.download().any() for x in bo)
    g.graphBegin()                                                      # a call during a graph capture
    try:
        assert call() == UNS and b"cannot be captured" in L.hx_last_error()
    finally:
        try:
            g.graphEnd().destroy()
        except hx.HxError:
            pass
    for x, keep in ((out0, m0), (out1, m1), (c0, r0), (c1, r1)):
        assert x.getIndexSet() == (allp if x in (out0, out1) else own) and np.array_equal(x.download(), keep)
    assert call() == 0, L.hx_last_error()                               # and the context still works
    keys = [(b, a)] * 2
    want0, want1 = TR.hoisted_sum(m, [g.primes[i] for i in allp], 2, _psp(g, allp, sp), dig, r0, r1, ks, keys)
    assert np.array_equal(out0.download(), want0) and np.array_equal(out1.download(), want1)


# ---- traceMap and automorphSum of a real ciphertext ----
def _same(x, y):
    wx = {h: (part.getIndexSet(), part.download()) for h, part in x.parts.items()}
    wy = {h: (part.getIndexSet(), part.download()) for h, part in y.parts.items()}
    assert sorted(wx, key=str) == sorted(wy, key=str) == ["1", "s"]
    assert all(wx[h][0] == wy[h][0] and np.array_equal(wx[h][1], wy[h][1]) for h in wx)
    assert (x.lnNoise, x.primeSet, x.ptxtSpace, x.intFactor, x.ptxtMag) == (y.lnNoise, y.primeSet, y.ptxtSpace, y.intFactor, y.ptxtMag)


@pytest.mark.parametrize("m,p,r", [(85, 2, 2), (57, 7, 1)])
def test_trace_map_fused_is_the_loop(hx, monkeypatch, m, p, r):
    from helib_amd import bgv_gr, ctxt as hc, keys as hk, thin_evalmap as TE
    cc = hc.ChainContext(m, p, r, bits=200, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=5)
    sk.GenSecKey()
    ea = bgv_gr.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    hk.addFrbMatrices(sk)
    d = ea.getDegree()
    v = np.random.default_rng(m).integers(0, p ** r, size=(3, ea.size(), d))
    ct = ea.encrypt_batch(sk, v)
    ct.multiplyBy(ea.encrypt_batch(sk, v))                              # below the top level
    if p > 2:
        ct.mulIntFactor(3)
    seen = []
    real = hx.hoistedSum
    monkeypatch.setattr(hx, "hoistedSum", lambda *args: (seen.append(len(args[3])), real(*args))[1])
    ks = [ea.zMStar.genToPow(-1, i) for i in range(1, d)]
    loop = hc.BasicAutomorphPrecon(ct).automorphSum(ks, fused=False)
    assert hc.Ctxt.fuseHoistedSum is True and not seen
    fused = hc.BasicAutomorphPrecon(ct).automorphSum(ks)                # fused=None follows the switch
    assert seen == [d - 1]
    _same(loop, fused)
    a, b = ct.clone(), ct.clone()
    TE.traceMap(ea, a, sk, fused=False)
    TE.traceMap(ea, b, sk)
    assert TE.traceMap.last == "hoisted" and seen == [d - 1, d - 1]
    _same(a, b)
    _same(a, loop)
    want = TE.tracePlain(ea, ea.mulPlain(v, v))
    assert b.isCorrect() and np.array_equal(ea.decrypt_batch(b, sk), want)
