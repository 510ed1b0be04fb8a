"""helib_amd.bgv_hypercube on the host side (no GPU): rotate / shift / runningSums / totalSums and MatMul1DExec over
hypercubes with non-native dimensions, over the oracle backend with a CPU encoder (one vector per ciphertext, two
vectors per case), against numpy on the plaintext slots; the bad-last-dimension branch of rotate against the same
branch written out with the Ctxt primitives; the bookkeeping of the fused blend; the new entry point's declaration.

bits per ring: enough that every sequence here (totalSums is the deepest: one mask product per rotate1D over a bad
dimension and one per split, log2(n) + 1 rotations) still decrypts -- Ctxt.isCorrect is asserted."""
import os
import re
import subprocess

import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_hypercube_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = {(85, 2): 300, (119, 2): 400, (255, 2): 500, (527, 2): 500, (803, 3): 600, (151, 2): 300}


def test_the_rings_are_what_they_are_taken_for():
    for (m, p), ords in H.RINGS.items():
        assert hostnt.ZmStar(m, p).signedOrds() == ords, (m, p)
    assert hostnt.ZmStar(151, 2).signedOrds() == [-10]          # the smallest bad dimension above MIN_THRESH = 8
    assert hostnt.ZmStar(21845, 2).signedOrds() == [-128, -8]


def _vectors(ea, seed):
    """two vectors: a single 1 in slot 0, and random slots"""
    n, p = ea.size(), ea.p
    return [np.eye(1, n, dtype=np.int64), np.random.default_rng(seed).integers(0, p, size=(1, n))]


def _amounts(n, every):
    """every amount in [-n, 2n], or the ends, the wrap-arounds and one amount per coordinate pattern"""
    if every:
        return list(range(-n, 2 * n + 1))
    return sorted({-n, -n + 1, -1, 0, 1, 3, n // 2, n - 1, n, n + 1, 2 * n})


# ---- semantics ----
@pytest.mark.parametrize("m,p", [(119, 2), (255, 2), (527, 2), (803, 3)])
def test_rotate_and_shift_against_numpy(m, p):
    cc, sk, ea = H.setup(m, p, BITS[m, p])
    n = ea.size()
    assert ea.dimension() > 1 and not all(ea.nativeDimension(i) for i in range(ea.dimension()))
    every = n <= 4
    for a in _vectors(ea, m):
        for amt in _amounts(n, every):
            ct = ea.encrypt(sk, a)
            assert ea.rotate(ct, amt) is ct
            assert np.array_equal(ea.decrypt_batch(ct, sk), np.roll(a, amt, axis=1)), ("rotate", amt)
            assert ct.isCorrect()
        ks = range(-n + 1, n) if every else [k for k in _amounts(n, False) if -n < k < n]
        for k in list(ks) + [n, -n, n + 2]:
            ct = ea.encrypt(sk, a)
            assert ea.shift(ct, k) is ct
            got = ea.decrypt_batch(ct, sk)
            assert np.array_equal(got, H.shift(a, k)), ("shift", k)
            if abs(k) >= n:
                assert not got.any()
            else:
                assert ct.isCorrect()


@pytest.mark.parametrize("m,p", [(85, 2), (119, 2), (255, 2), (527, 2), (803, 3)])
def test_sums_against_numpy(m, p):
    cc, sk, ea = H.setup(m, p, BITS[m, p])
    assert (ea.dimension() == 1) == (m == 85)                   # (85, 2): the single-generator path
    for a in _vectors(ea, m + 1):
        ct = ea.encrypt(sk, a)
        assert ea.totalSums(ct) is ct
        assert np.array_equal(ea.decrypt_batch(ct, sk), H.total_sums(a, p))
        assert ct.isCorrect()
        ct = ea.encrypt(sk, a)
        assert ea.runningSums(ct) is ct
        assert np.array_equal(ea.decrypt_batch(ct, sk), H.running_sums(a, p))
        assert ct.isCorrect()


def test_slot_permutation_is_the_automorphism():
    """slotPermutation(k) against the ciphertext automorphism X -> X^k on a bad dimension, wrap-around included: it is
    a permutation, and equal to the roll wherever nothing leaves the end"""
    m, p = 255, 2
    cc, sk, ea = H.setup(m, p, BITS[m, p])
    z = ea.zMStar
    a = np.random.default_rng(5).integers(0, p, size=(1, ea.size()))
    a[0, :4] = [1, 0, 0, 1]
    for amt in (1, 3, -2, -8):
        k = z.genToPow(0, amt)
        perm = ea.slotPermutation(k)
        assert sorted(perm) == list(range(ea.size()))
        ct = ea.encrypt(sk, a)
        ct.smartAutomorph(k)
        assert np.array_equal(ea.decrypt_batch(ct, sk), a[:, perm]), amt
        c = ea._coords(0)
        inside = (c - amt >= 0) & (c - amt < 8)
        roll = np.roll(a.reshape(1, 8, 2), amt, axis=1).reshape(1, -1)
        assert np.array_equal(a[:, perm][:, inside], roll[:, inside])


# ---- the sequence of the bad-last-dimension branch ----
@pytest.mark.parametrize("m,p", [(527, 2), (803, 3)])
def test_bad_last_dimension_branch_by_hand(m, p):
    """rotate by an amount with v != 0 in the (bad) last dimension: the automorphisms issued are those of
    src/EncryptedArray.cpp:227-254, and the words and the bookkeeping equal the branch written out here"""
    from helib_amd import ctxt as hc
    cc, sk, ea = H.setup(m, p, BITS[m, p], seed=6)
    _, sk2, ea2 = H.setup(m, p, BITS[m, p], seed=6)
    z, ref = ea.zMStar, H.tables(m, p)
    o0, o1 = z.ords
    v0, v1 = 2, 1
    amt = v0 * o1 + v1
    a = np.random.default_rng(4).integers(0, p, size=(1, ea.size()))
    ct, bh = ea.encrypt(sk, a), ea2.encrypt(sk2, a)
    seen, real = [], hc.Ctxt.smartAutomorph

    def spy(self, k):
        seen.append(k)
        return real(self, k)
    hc.Ctxt.smartAutomorph = spy
    try:
        ea.rotate(ct, amt)
    finally:
        hc.Ctxt.smartAutomorph = real
    g = z.genToPow
    if z.SameOrd(0):
        want = [g(1, v1), g(1, -o1), g(0, v0), g(0, v0 + 1)]
    else:
        want = [g(1, v1), g(1, -o1), g(0, v0), g(0, -o0), g(0, v0 + 1), g(0, -o0)]
    assert seen == want
    assert np.array_equal(ea.decrypt_batch(ct, sk), np.roll(a, amt, axis=1))
    # by hand
    be = sk2.be

    def const(slots, primes):
        cf = ref.encode(np.asarray(slots).reshape(1, -1), 1)[0]
        return be.fromCoeffs(sorted(primes), [int(x) for x in cf]), be.embeddingLargestCoeff(cf)

    def rotate1d(c, i, v):
        v %= z.ords[i]
        if v == 0:
            return
        c.smartAutomorph(g(i, v))
        if z.SameOrd(i):
            return
        T = c.clone()
        T.smartAutomorph(g(i, -z.ords[i]))
        m1, sz = const(ea2._coords(i) >= v, c.primeSet | T.primeSet)
        c.multByConstant(m1, sz)
        c += T
        T.multByConstant(m1, sz)
        c -= T
    bh.smartAutomorph(g(1, v1))
    tmp = bh.clone()
    tmp.smartAutomorph(g(1, -o1))
    m1, sz = const(ea2._coords(1) >= v1, bh.primeSet | tmp.primeSet)
    bh.multByConstant(m1, sz)
    tmp1 = tmp.clone()
    tmp1.multByConstant(m1, sz)
    tmp -= tmp1
    rotate1d(bh, 0, v0)
    rotate1d(tmp, 0, v0 + 1)
    bh += tmp
    H.same(ct, bh, lambda part: part.rows)
    assert np.array_equal(ea2.decrypt_batch(bh, sk2), np.roll(a, amt, axis=1))


# ---- fused bookkeeping ----
def _ops(calls):
    from oracle.backend import OracleOps

    class Ops(OracleOps):
        """maskBlend / maskSplit / likeUninit made of the oracle's own *=, +=, -="""
        @staticmethod
        def likeUninit(poly):
            q = poly.copy()
            q.rows[:] = 12345
            return q

        @staticmethod
        def maskSplit(k0, k1, t0, t1, mask):
            for k, t in ((k0, t0), (k1, t1)):
                if k is not None:
                    t.rows[:] = k.rows
                    t *= mask
                    k -= t

        @staticmethod
        def maskBlend(c0, c1, t0, t1, mask):
            calls.append(c1 is not None)
            for c, t in ((c0, t0), (c1, t1)):
                if c is not None:
                    t = t.copy()                 # t is read only
                    c *= mask
                    c += t
                    t *= mask
                    c -= t
    return Ops


@pytest.mark.parametrize("m,p", [(119, 2), (255, 2)])
def test_fused_and_termwise_bookkeeping_agree(m, p):
    from helib_amd import ckks
    calls, out = [], {}
    n = hostnt.ZmStar(m, p).getNSlots()
    for fused in (True, False):
        cc, sk, ea = H.setup(m, p, BITS[m, p], seed=2, ops=_ops(calls))
        bad = [i for i in range(ea.dimension()) if not ea.nativeDimension(i)][0]
        a = np.random.default_rng(1).integers(0, p, size=(1, n))
        res = []
        for f, want in ((lambda c: ea.rotate1D(c, bad, 1, fused=fused), None),
                        (lambda c: ea.rotate(c, n - 1, fused=fused), np.roll(a, n - 1, axis=1)),
                        (lambda c: ea.shift(c, 1, fused=fused), H.shift(a, 1)),
                        (lambda c: ea.totalSums(c, fused=fused), H.total_sums(a, p))):
            ct = ea.encrypt(sk, a)
            f(ct)
            if want is not None:
                assert np.array_equal(ea.decrypt_batch(ct, sk), want), fused
            res.append(ct)
        out[fused] = res
        if fused:
            ncalls = len(calls)
    assert len(calls) == ncalls > 0 and all(calls)       # two parts at a time, and only under fused=True
    for x, y in zip(out[True], out[False]):
        H.same(x, y, lambda part: part.rows)
        assert x.ptxtMag == y.ptxtMag
    # a backend without the call cannot be forced; the default follows the class attribute
    cc, sk, ea = H.setup(m, p, BITS[m, p], seed=2)
    assert type(ea).fuseMaskBlend in (True, False)
    with pytest.raises(ckks.LogicError, match="no maskBlend"):
        ea.rotate1D(ea.encrypt(sk, a), bad, 1, fused=True)
    ea.rotate1D(ea.encrypt(sk, a), bad, 1)


def test_unequal_int_factors_go_term_by_term():
    """(803, 3): a pair whose intFactors differ is blended by the four calls under fused=True too (addCtxt rescales),
    and the result is the term-by-term one"""
    m, p = 803, 3
    calls, res = [], {}
    for fused in (True, False):
        cc, sk, ea = H.setup(m, p, BITS[m, p], seed=2, ops=_ops(calls), keys=False)
        a = np.random.default_rng(1).integers(0, p, size=(1, ea.size()))
        ct, T = ea.encrypt(sk, a), ea.encrypt(sk, (a + 1) % p)
        T.intFactor = 2                                     # T now encrypts 2 * (a + 1) ... with factor 2: still a + 1
        for part in T.parts.values():
            part.mulConstant(2)
        mask = ea.maskSlots(0, 2)
        m1, sz = ea._encodedMask(mask, ct.primeSet)
        ea._maskBlend(ct, T, m1, sz, fused=fused)
        assert np.array_equal(ea.decrypt_batch(ct, sk), (a * mask + (a + 1) * (1 - mask)) % p)
        res[fused] = ct
    assert not calls
    H.same(res[True], res[False], lambda part: part.rows)
    # equal factors: fused
    cc, sk, ea = H.setup(m, p, BITS[m, p], seed=2, ops=_ops(calls), keys=False)
    ct, T = ea.encrypt(sk, a), ea.encrypt(sk, (a + 1) % p)
    ea._maskBlend(ct, T, *ea._encodedMask(mask, ct.primeSet), fused=True)
    assert calls == [True]
    assert np.array_equal(ea.decrypt_batch(ct, sk), (a * mask + (a + 1) * (1 - mask)) % p)


# ---- MatMul1D ----
@pytest.mark.parametrize("minimal,keys", [(False, "all"), (True, "minimal"), (True, "all")])
@pytest.mark.parametrize("m,p,dim", [(85, 2, 0), (255, 2, 0), (527, 2, 1), (151, 2, 0)])
def test_matmul1d_against_numpy(m, p, dim, minimal, keys):
    """keys "all": every 1D matrix, the general-automorphism / giant-step form; "minimal": the minimal key set, the
    iterative form.  (151, 2) has D = 10 > 8, so minimal=True there takes baby steps and giant steps (g != 0), iterative
    or not by the keys; the other rings run the g = 0 branches"""
    from helib_amd import bgv_hypercube as bh, bgv_matmul as bm, keys as hk
    cc, sk, ea = H.setup(m, p, BITS[m, p], keys=False)
    (hk.addMinimal1DMatrices if keys == "minimal" else hk.add1DMatrices)(sk)
    D = ea.sizeOfDimension(dim)
    assert not ea.nativeDimension(dim)
    rng = np.random.default_rng(m + dim)
    A = rng.integers(0, p, size=(D, D))
    A[0, 0] = 1
    mat = bm.MatMul1D(ea, A, dim)
    ex = bh.MatMul1DExec(ea, mat, minimal=minimal)
    assert (ex.g != 0) == (minimal and D > 8)
    for a in _vectors(ea, m):
        ct = ea.encrypt(sk, a)
        assert ex.mul(ct, pk=sk) is ct
        assert np.array_equal(ea.decrypt_batch(ct, sk), bm.mulPlain(ea, a, mat)), (m, dim, minimal)
        assert ct.isCorrect()


def test_matmul1d_zero_diagonal_and_refusals():
    from helib_amd import bgv_hypercube as bh, bgv_matmul as bm, ckks
    m, p = 255, 2
    cc, sk, ea = H.setup(m, p, BITS[m, p])
    D = 8
    A = np.random.default_rng(3).integers(0, p, size=(D, D))
    j = np.arange(D)
    A[(j - 3) % D, j] = 0                                   # diagonal 3 is zero
    A[(j - 5) % D, j] = 1
    ex = bh.MatMul1DExec(ea, A, dim=0)
    assert ex.multiplier[3] is None and ex.multiplier1[3] is None
    assert ex.multiplier[5] is not None and ex.multiplier1[5] is not None
    assert ex.multiplier1[0] is None                        # no coordinate lies below 0: poly2 of diagonal 0 is zero
    a = np.random.default_rng(4).integers(0, p, size=(1, ea.size()))
    ct = ea.encrypt(sk, a)
    ex.mul(ct, pk=sk)
    assert np.array_equal(ea.decrypt_batch(ct, sk), bm.mulPlain(ea, a, bm.MatMul1D(ea, A, 0)))
    # the native dimension is the base class's
    nat = bh.MatMul1DExec(ea, np.array([[0, 1], [1, 1]]), dim=1)
    assert nat.native and not hasattr(nat, "multiplier1")
    ct = ea.encrypt(sk, a)
    nat.mul(ct, pk=sk)
    assert np.array_equal(ea.decrypt_batch(ct, sk), bm.mulPlain(ea, a, bm.MatMul1D(ea, np.array([[0, 1], [1, 1]]), 1)))
    # what stays refused
    full = np.eye(ea.size(), dtype=np.int64)
    with pytest.raises(ckks.LogicError, match="out of scope"):
        bh.MatMulFullExec(ea, full)
    with pytest.raises(ckks.LogicError, match="non-native"):
        bm.MatMulFullExec(ea, full)
    with pytest.raises(ckks.LogicError, match="non-native"):
        bm.MatMul1DExec(ea, A, dim=0)


# ---- declarations ----
def test_mask_blend_is_declared_bound_and_exported():
    from helib_amd import bgv_hypercube, capi
    hdr = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    declared = set(re.findall(r"\b(hx_[a-zA-Z0-9_]+)\s*\(", hdr))
    assert "hx_mask_blend" in capi.SYMBOLS and "hx_mask_blend" in declared
    assert "src/EncryptedArray.cpp:120-124" in hdr and "t is\n * read, not written" in hdr
    lib = capi.lib()                      # the cross-compiled library
    assert len(lib.hx_mask_blend.argtypes) == 5
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi._SO], text=True)
    assert re.search(r"\bT hx_mask_blend$", out, re.M)
    assert hasattr(capi, "maskBlend")
    with pytest.raises(capi.InvalidArgument, match="go together"):
        capi.maskBlend(None, None, None, object(), None)
    for f in ("rotate1D", "rotate", "shift", "totalSums", "runningSums", "_maskBlend", "slotPermutation"):
        assert f in vars(bgv_hypercube.EncryptedArray)
