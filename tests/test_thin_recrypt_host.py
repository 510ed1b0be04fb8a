"""Thin recryption on the CPU: helib_amd.thin_evalmap (ThinEvalMap on the plain side and its matrices against a
restatement of the reference's two matrix classes, traceMap on every branch over the oracle backend),
BasicAutomorphPrecon.automorphSum with hx_hoisted_automorph_sum stated in python integers (tests/thin_ref.py) against the
loop it replaces, and the whole thinReCrypt over the oracle backend of tests/recryption_ref.py.  Everything here is an
integer: every comparison is exact.  No GPU.

The chain: on this code thinReCrypt holds (the slots come back, isCorrect(), the capacity grows, a second thinReCrypt after
one more multiplication decrypts) from bits = 300 on, the smallest multiple of 100, at (57, 7, 1), (85, 2, 1) and (85, 2, 2):
at 100 nothing decrypts, at 200 the check of rawModSwitch's noise estimate refuses (57, 7, 1) at once and (85, 2, 2) at the
second recryption.  The tests run at 300 + 100 = 400."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import evalmap_tables as E
from tests import recryption_ref as RR
from tests import thin_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS_MIN, BITS = 300, 400       # see the module docstring


def _ring(m):
    p, rs, mvec, gens, ords = E.ring(m)
    return m, p, rs[-1], mvec, gens, ords


# ---- (a) the thin maps on the plain side ----
@pytest.mark.parametrize("m", [85, 57, 105, 15, 1365])
def test_thin_map_identities(m):
    """m = 85 at 2^4, 57 at 7^2 (d = 3), 105 at 2^3 (d = 12), 15 at 2^4 (the size-1 last dimension), 1365 at 17 (three
    factors)"""
    from helib_amd import evalmap, thin_evalmap as TE
    m, p, r, mvec, gens, ords = _ring(m)
    ea = E.plain_ea(m, p, r, gens, ords)
    n, d, P = ea.size(), ea.getDegree(), ea.P
    rng = np.random.default_rng(m)
    fwd, inv = TE.ThinEvalMap(ea, mvec), TE.ThinEvalMap(ea, mvec, invert=True)
    assert (fwd.matvec_data[-1] is None) == (ea.dimension() < len(mvec)) == (m == 15)
    v = rng.integers(0, P, size=(2, n))
    # 1. the forward map on constants is EvalMap's
    a = fwd.applyPlain(v)
    assert np.array_equal(a, evalmap.EvalMap(ea, mvec).applyPlain(v))
    # 2. inverse after forward is the identity, and leaves constants
    back = inv.applyPlain(a)
    assert np.array_equal(back[:, :, 0], v) and not back[:, :, 1:].any()
    # 3. on any slots the inverse map is coefficient 0 of the packed inverse
    z = rng.integers(0, P, size=(2, n, d))
    thin = inv.applyPlain(z)
    assert np.array_equal(thin[:, :, 0], evalmap.EvalMap(ea, mvec, invert=True).applyPlain(z)[:, :, 0])
    assert not thin[:, :, 1:].any()


def _inverse_mod(M, p, P):
    """the inverse of a square matrix of python integers modulo P = p^r, by Gauss-Jordan with unit pivots"""
    n = len(M)
    w = [[int(x) % P for x in row] + [int(i == j) for j in range(n)] for i, row in enumerate(M)]
    for c in range(n):
        piv = next(i for i in range(c, n) if w[i][c] % p)
        w[c], w[piv] = w[piv], w[c]
        f = pow(w[c][c], -1, P)
        w[c] = [x * f % P for x in w[c]]
        for i in range(n):
            if i != c and w[i][c]:
                g = w[i][c]
                w[i] = [(x - g * y) % P for x, y in zip(w[i], w[c])]
    return [row[n:] for row in w]


@pytest.mark.parametrize("m", [85, 57, 105, 15, 1365])
def test_thin_matrices_are_the_reference_classes(m):
    """ThinStep2Matrix (src/EvalMap.cpp:699-727) and ThinStep1Matrix (:815-885) restated over python integers"""
    from helib_amd import thin_evalmap as TE
    m, p, r, mvec, gens, ords = _ring(m)
    ea = E.plain_ea(m, p, r, gens, ords)
    G, P, d, k = [int(x) for x in ea.G], ea.P, ea.getDegree(), len(mvec)
    fwd, inv = TE.ThinEvalMap(ea, mvec), TE.ThinEvalMap(ea, mvec, invert=True)
    one = [1 % P] + [0] * (d - 1)

    def powers(pt, count):
        out = [one]
        for _ in range(1, count):
            out.append(E.ring_mul(out[-1], pt, G, P))
        return out
    for dim in range(k):
        reps, cof = fwd.reps[dim], m // mvec[dim]
        sz = len(reps)
        pts = [E.eta_pow(rep * cof, G, P) for rep in reps]
        last = dim == k - 1
        # forward: A[i][j] = point_j^i, the last factor's points raised to d
        fpts = [powers(pt, d + 1)[d] for pt in pts] if last else pts
        A = [[powers(pt, sz)[i] for pt in fpts] for i in range(sz)]
        mat = fwd.matvec_data[dim]
        if dim >= ea.dimension():
            assert mat is None and sz == 1
        else:
            assert mat.dim == dim and mat.dense[0].tolist() == A
        if not last:
            # inverse: the inverse over the ring -- A^-1 A = 1
            Ai = inv.matvec_data[dim].dense[0].tolist()
            for i in range(sz):
                for j in range(sz):
                    acc = [0] * d
                    for l in range(sz):
                        acc = [(x + y) % P for x, y in zip(acc, E.ring_mul(Ai[i][l], A[l][j], G, P))]
                    assert acc == (one if i == j else [0] * d), (dim, i, j)
            continue
        # the last factor's inverse: column 0 of every block of the inverted (sz d) x (sz d) matrix, times T^-1
        AA = [[powers(pt, sz * d)[i] for pt in pts] for i in range(sz * d)]
        A1 = [[AA[i][j // d][j % d] for j in range(sz * d)] for i in range(sz * d)]
        A2 = _inverse_mod(A1, p, P)
        tv = []
        for i in range(2 * d - 1):
            t = [0] * d
            for e in range(d):
                t = [(x + y) % P for x, y in zip(t, E.eta_pow(i * p ** e, G, P))]
            assert not any(t[1:])
            tv.append(t[0])
        Tinv = _inverse_mod([[tv[i + j] for j in range(d)] for i in range(d)], p, P)
        W = [[[sum(A2[i * d + i1][j * d] * Tinv[i1][c] for i1 in range(d)) % P for c in range(d)] for j in range(sz)]
             for i in range(sz)]
        mat = inv.matvec_data[dim]
        if dim >= ea.dimension():                       # the product by W[0][0] in every slot, as a block
            blk = [E.ring_mul(E.eta_pow(l, G, P), W[0][0], G, P) for l in range(d)]
            assert mat.dim == ea.dimension() and all(x.tolist() == blk for x in mat.dense[:, 0, 0])
        else:
            assert mat.dim == dim and mat.dense[0].tolist() == W


def test_thin_map_makes_evalmaps_checks():
    from helib_amd import evalmap, thin_evalmap as TE
    m, p, r, mvec, gens, ords = _ring(85)
    ea = E.plain_ea(m, p, r, gens, ords)
    for bad, msg in (((5, 15), "pairwise co-prime"), ((5, 19), "does not match"), ((), "must not be empty"),
                     ((17, 5), "bad inertPrefix|must equal reps")):
        for cls in (TE.ThinEvalMap, evalmap.EvalMap):
            with pytest.raises(evalmap.LogicError, match=msg):
                cls(ea, bad)
    with pytest.raises(evalmap.LogicError, match="bgv_gr.EncryptedArray"):
        TE.ThinEvalMap(object(), mvec)
    with pytest.raises(evalmap.LogicError, match="ThinEvalMap is not built"):      # the old name keeps refusing
        evalmap.ThinEvalMap(ea, mvec)


# ---- (b) traceMap over the oracle backend, every branch ----
@functools.lru_cache(maxsize=None)
def _trace_setup(m, p, r, bits=150):
    from tests import bgv_gr_tables as T
    S = T.Setup(m, p, r, bits=bits)
    S.hs_calls = []
    type(S.be.ops).hoistedSum = TR.oracle_hoisted_sum(S.o, S.hs_calls)
    return S


def _key(S, family, seed=11):
    """a second key over S's chain holding one family of Frobenius matrices"""
    from helib_amd import keys as hk
    sk = hk.SecKey(S.cc, S.be, seed=seed)
    sk.GenSecKey()
    sk.zMStar = S.ea.zMStar
    getattr(hk, family)(sk)
    return sk


TRACE = [(57, 7, 1, "addFrbMatrices", "hoisted", 3), (85, 2, 1, "addFrbMatrices", "hoisted", 8),
         (31, 2, 1, "addMinimalFrbMatrices", "iterative", 5), (105, 2, 1, "addMinimalFrbMatrices", "bsgs", 12),
         (23, 2, 1, "addMinimalFrbMatrices", "bsgs-remainder", 11), (93, 2, 1, "addBSGSFrbMatrices", "doubling", 10)]


@pytest.mark.parametrize("m,p,r,family,branch,d", TRACE)
def test_trace_map_takes_every_branch(m, p, r, family, branch, d):
    from helib_amd import keys as hk, thin_evalmap as TE
    S = _trace_setup(m, p, r)
    ea = S.ea
    assert ea.getDegree() == d
    if branch.startswith("bsgs"):
        g = hk.KSGiantStepSize(d)
        assert g == 4 and (d % g == 0) == (branch == "bsgs") and d - g * (d // g) == (0 if branch == "bsgs" else 3)
    sk = _key(S, family)
    v = S.slots(m)
    ct = ea.encrypt(sk, v)
    assert TE.traceMap(ea, ct, sk) is ct and TE.traceMap.last == branch
    want = TE.tracePlain(ea, v)
    assert not want[:, :, 1:].any() and want[:, :, 0].any()
    assert ct.isCorrect() and np.array_equal(ea.decrypt_batch(ct, sk), want)
    # the trace of a sum of Frobenius images, slot by slot, by the definition
    alt = sum(ea.frobeniusPlain(v, e) for e in range(d)) % ea.P
    assert np.array_equal(want, alt)


# ---- (c) automorphSum: one hoistedSum against the loop ----
def _words(ct):
    return {h: (list(part.idx), part.rows.copy()) for h, part in ct.parts.items()}


def _books(ct):
    return ct.lnNoise, ct.primeSet, ct.ptxtSpace, ct.intFactor, ct.ptxtMag, ct.lnRatFactor


@pytest.mark.parametrize("m,p,r,d", [(57, 7, 1, 3), (85, 2, 1, 8)])
def test_automorph_sum_fused_is_the_loop(m, p, r, d):
    from helib_amd import ctxt as hc, thin_evalmap as TE
    S = _trace_setup(m, p, r)
    ea, sk = S.ea, S.sk
    ct = ea.encrypt(sk, S.slots(3))
    ct.multiplyBy(ea.encrypt(sk, S.slots(4)))                           # below the top level: W is made for more primes
    if p > 2:
        ct.mulIntFactor(3)
    ks = [ea.zMStar.genToPow(-1, i) for i in range(1, d)]
    assert hc.Ctxt.fuseHoistedSum is True                              # profiles/thin_recrypt.json: it won every pair
    del S.hs_calls[:]
    loop = hc.BasicAutomorphPrecon(ct).automorphSum(ks, fused=False)
    assert not S.hs_calls
    fused = hc.BasicAutomorphPrecon(ct).automorphSum(ks)                # fused=None follows the switch
    assert len(S.hs_calls) == 1 and S.hs_calls[0][0] == d - 1
    wl, wf = _words(loop), _words(fused)
    assert sorted(wl, key=str) == sorted(wf, key=str) == ["1", "s"]
    for h in wl:
        assert wl[h][0] == wf[h][0] and np.array_equal(wl[h][1], wf[h][1]), h
    assert _books(loop) == _books(fused)
    assert set(S.cc.specialPrimes) <= fused.primeSet
    # the switch, and traceMap through it
    a, b = ct.clone(), ct.clone()
    try:
        hc.Ctxt.fuseHoistedSum = False
        TE.traceMap(ea, a, sk)
        assert len(S.hs_calls) == 1
    finally:
        hc.Ctxt.fuseHoistedSum = True
    TE.traceMap(ea, b, sk)
    assert len(S.hs_calls) == 2 and _books(a) == _books(b) == _books(loop)
    assert all(np.array_equal(_words(a)[h][1], _words(b)[h][1]) for h in ("1", "s"))


def test_automorph_sum_falls_back():
    from helib_amd import ctxt as hc
    S = _trace_setup(85, 2, 1)
    ea = S.ea
    sk = _key(S, "addBSGSFrbMatrices")                                  # p^1 .. p^3 and p^4: p^5 goes through two matrices
    ct = ea.encrypt(sk, S.slots(5))
    ks = [ea.zMStar.genToPow(-1, i) for i in range(1, 8)]
    assert ct._firstStep(ks[4]) != ks[4]
    del S.hs_calls[:]
    loop = hc.BasicAutomorphPrecon(ct).automorphSum(ks, fused=False)
    fused = hc.BasicAutomorphPrecon(ct).automorphSum(ks, fused=True)
    assert not S.hs_calls and _books(loop) == _books(fused)
    assert all(np.array_equal(_words(loop)[h][1], _words(fused)[h][1]) for h in ("1", "s"))
    direct = hc.BasicAutomorphPrecon(ct).automorphSum(ks[:3], fused=True)       # the matrices that are there: one call
    assert S.hs_calls == [(3, len(hc.BasicAutomorphPrecon(ct).digits))]
    assert _books(direct) == _books(hc.BasicAutomorphPrecon(ct).automorphSum(ks[:3], fused=False))
    # a backend without the op
    ops = type(S.be.ops)
    op = ops.hoistedSum
    del ops.hoistedSum
    try:
        with pytest.raises(RuntimeError, match="no hoistedSum"):
            hc.BasicAutomorphPrecon(ct).automorphSum(ks[:3], fused=True)
        assert _books(hc.BasicAutomorphPrecon(ct).automorphSum(ks[:3])) == _books(direct)   # fused=None: the loop, quietly
    finally:
        ops.hoistedSum = op


# ---- (d) the whole thinReCrypt over the oracle backend ----
@functools.lru_cache(maxsize=None)
def thin_ring(m, r, bits=BITS):
    from helib_amd import recryption as RC
    p, _, mvec, gens, ords = E.ring(m)
    S, rc0 = RR.recrypt_setup(m, p, r, mvec, gens, ords, bits)
    S.hs_calls = []
    type(S.be.ops).hoistedSum = TR.oracle_hoisted_sum(S.o, S.hs_calls)
    rc = RC.ThinRecryptData(S.cc, None, mvec, alsoThick=True, ea=S.ea, ea_boot=rc0.ea_boot, p2dConv=rc0.p2dConv)
    return S, rc


def thin_input(S, seed):
    """thinly packed random slots with the capacity used up -> (ct, want)"""
    ea, sk = S.ea, S.sk
    v = np.random.default_rng(seed).integers(0, ea.P, size=(1, ea.size()))
    want = ea._slots(v)
    ct = ea.encrypt(sk, v)
    while ct.bitCapacity() > 60:
        ct.multiplyBy(ea.encrypt(sk, v))
        want = ea.mulPlain(want, v)
    if S.p > 2:
        ct.mulIntFactor(3)                                              # intFactor != 1: lost and restored
        assert ct.intFactor != 1
    assert not want[:, :, 1:].any() and np.array_equal(ea.decrypt_batch(ct, sk), want)
    return ct, v, want


@pytest.mark.parametrize("m,r", TR.THIN_RINGS)
def test_thin_recrypt_over_the_oracle_backend(m, r):
    """two ciphertexts (the oracle backend holds one batch element each), thinly packed"""
    from helib_amd import recryption as RC, thin_evalmap as TE, timing
    S, rc = thin_ring(m, r)
    ea, sk = S.ea, S.sk
    assert isinstance(rc.coeffToSlot, TE.ThinEvalMap) and rc.coeffToSlot.invert and not rc.slotToCoeff.invert
    assert rc.coeffToSlot.ea is rc.ea_boot and rc.slotToCoeff.ea is ea and rc.firstMap is not None
    for seed in (1, 2):
        ct, v, want = thin_input(S, 10 * m + seed)
        thick = ct.clone()
        before = ct.bitCapacity()
        timing.resetAllTimers()
        stats = {}
        assert RC.thinReCrypt(ct, sk, rc, seed=5, stats=stats) is ct
        assert TE.traceMap.last == "hoisted"
        assert [c[0] for c in S.prep_calls[-2:]] == [0, 1] and all(c[1] <= 3 + len(S.cc.specialPrimes) for c in S.prep_calls)
        assert 0 < stats["raw-mod-switch-noise"][0] <= 1
        for name in ("AAA_slotToCoeff", "AAA_bootKeySwitch", "AAA_coeffToSlot", "AAA_extractDigitsThin"):
            assert timing.getTimerByName(name).numCalls == 1, name
        assert ct.isCorrect() and ct.bitCapacity() > before and ct.ptxtSpace == rc.p2r
        assert np.array_equal(ea.decrypt_batch(ct, sk), want)
        ct.multiplyBy(ea.encrypt(sk, v))                                 # one more multiplication, and again
        want2 = ea.mulPlain(want, v)
        stats = {}
        RC.thinReCrypt(ct, sk, rc, seed=6, stats=stats)
        assert 0 < stats["raw-mod-switch-noise"][0] <= 1
        assert ct.isCorrect() and ct.ptxtSpace == rc.p2r and np.array_equal(ea.decrypt_batch(ct, sk), want2)
        if seed == 1:                                                   # the packed reCrypt on the same thin input
            RC.reCrypt(thick, sk, rc, seed=5)
            assert thick.isCorrect() and np.array_equal(ea.decrypt_batch(thick, sk), want)


def test_thin_recrypt_with_the_fused_sum_is_the_same_ciphertext():
    from helib_amd import ctxt as hc, recryption as RC
    S, rc = thin_ring(85, 1)
    ct, _, want = thin_input(S, 77)
    other = ct.clone()
    del S.hs_calls[:]
    try:
        hc.Ctxt.fuseHoistedSum = False
        RC.thinReCrypt(ct, S.sk, rc, seed=9)
        assert not S.hs_calls
    finally:
        hc.Ctxt.fuseHoistedSum = True
    RC.thinReCrypt(other, S.sk, rc, seed=9)
    assert len(S.hs_calls) == 1 and _books(ct) == _books(other)
    assert all(np.array_equal(_words(ct)[h][1], _words(other)[h][1]) for h in ("1", "s"))
    assert np.array_equal(S.ea.decrypt_batch(other, S.sk), want)


def test_thin_recrypt_refusals():
    from helib_amd import recryption as RC
    S, rc = thin_ring(85, 1)
    ct = S.ea.encrypt(S.sk, S.slots(2)[:, :, 0])
    with pytest.raises(RC.LogicError, match="bootstrappable=True"):
        RC.ThinRecryptData(RR.chain(85, 2, 1, False), None, (5, 17))
    with pytest.raises(RC.LogicError, match="holds no maps"):
        RC.thinReCrypt(ct, S.sk, RC.RecryptData(S.cc, None, rc.mvec))
    dummy = ct.clone()
    del dummy.parts["s"]
    with pytest.raises(RC.LogicError, match="dummy encryption"):
        RC.thinReCrypt(dummy, S.sk, rc)
    sk2 = type(S.sk)(S.cc, S.be, seed=9)
    sk2.GenSecKey()
    with pytest.raises(RC.LogicError, match="No bootstrapping data"):
        RC.thinReCrypt(ct, sk2, rc)
    low = RR.chain(85, 2, 1)
    view = type("View", (), dict(vars(low)))()                          # the chain's fields with e < r
    view.ckks, view.bootstrappable, view.e, view.r = False, True, 1, 2
    with pytest.raises(RC.LogicError, match="rcData.e must be at least alMod.r"):
        RC.ThinRecryptData(view, None, (5, 17))
    empty = ct.clone()
    empty.parts = {}
    assert RC.thinReCrypt(empty, S.sk, rc) is empty


# ---- (z) declarations ----
def test_symbol_is_declared_bound_listed_and_exported():
    from helib_amd import build, capi, keys as hk
    header = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    so = build.build()
    dyn = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    lib = capi.lib()
    assert re.search(r"\bint hx_hoisted_automorph_sum\(", header)
    assert "hx_hoisted_automorph_sum" in capi.SYMBOLS
    assert re.search(r" T hx_hoisted_automorph_sum$", dyn, re.M)
    assert len(lib.hx_hoisted_automorph_sum.argtypes) == 10
    assert "src/matmul.cpp:2878-2887" in header and "n (ndig + 1) + 1 <= 256" in header
    text = subprocess.run(["nm", "-C", so], capture_output=True, text=True, check=True).stdout
    assert "hoisted_sum_kernel" in text and "hoisted_perm_kernel" in text
    assert capi.hoistedSum is capi.hoistedAutomorphSum and hasattr(hk.HxBackend, "hoistedSum")
    with pytest.raises(capi.InvalidArgument, match="are required"):       # the binding refuses before it reaches the library
        capi.hoistedAutomorphSum(None, None, None, [2], [None], [])
    with pytest.raises(capi.InvalidArgument, match="one matrix for each"):
        capi.hoistedAutomorphSum(object(), object(), object(), [2, 4], [object()], [])
