"""helib_amd.matmul_full on the host side (no GPU): MatMulFullExec over hypercubes with non-native dimensions, over the
oracle backend with a CPU encoder (tests/bgv_hypercube_ref.setup), against bgv_matmul.mulPlain; ctxt.automorphBlend with
hx_hoisted_blend stated in python integers (tests/matmul_full_ref.py) against the call sequence it replaces; the
fallbacks; the declarations of the new symbol.  Everything here is an integer: every comparison is exact.

bits per ring are those of tests/test_bgv_hypercube_host.BITS: a full product is at most one rotation with a mask
product along the first dimension and one MatMul1DExec along the last, shallower than the totalSums those figures were
chosen for -- Ctxt.isCorrect is asserted after every product."""
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_hypercube_ref as H
from tests import matmul_full_ref as MR
from tests.test_bgv_hypercube_host import BITS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#  (m, p): phi(m), ord(p), orders, native, dims after MatMulDimComp
CUBES = {(255, 2): (128, 8, (8, 2), (False, True), [1, 0]),
         (119, 2): (96, 24, (2, 2), (True, False), [0, 1]),
         (527, 2): (480, 40, (6, 2), (True, False), [1, 0]),
         (803, 3): (720, 60, (6, 2), (False, False), [1, 0]),
         (2091, 2): (1280, 40, (8, 4), (True, False), [1, 0])}


def dim_order(ords, native):
    """MatMulDimComp (src/matmul.cpp:2084-2098)"""
    return sorted(range(len(ords)), key=lambda i: (ords[i], not native[i]))


def test_the_hypercubes_are_what_they_are_taken_for():
    for (m, p), (phim, ordp, ords, native, dims) in CUBES.items():
        z = hostnt.ZmStar(m, p)
        assert (sum(math.gcd(i, m) == 1 for i in range(m)), z.ordP, tuple(z.ords), tuple(z.native)) == (phim, ordp, ords, native), (m, p)
        assert dim_order(z.ords, z.native) == dims, (m, p)
        assert phim == ordp * z.getNSlots()
    # 2091: the recursion runs along the non-native dimension of four coordinates (three masked terms), 32 slots
    assert hostnt.ZmStar(2091, 2).getNSlots() == 32
    assert hostnt.ZmStar(21845, 2).signedOrds() == [-128, -8]


def setup(m, p, keys="full", op=True, seed=3):
    """-> (cc, sk, ea, calls): tests/bgv_hypercube_ref.setup with hoistedBlend among the backend's ops (op=True);
    calls receives (n, ndig) per call of it.  keys: "full" (add1DMatrices: HELIB_KSS_FULL in every dimension), "minimal"
    (addMinimal1DMatrices: HELIB_KSS_MIN), "bsgs" (addBSGS1DMatrices: HELIB_KSS_BSGS) or None"""
    from oracle.backend import OracleOps
    from helib_amd import keys as hk
    calls = []

    class Ops(OracleOps):
        def __init__(self, o):
            super().__init__(o)
            if op:
                self.hoistedBlend = types.MethodType(MR.oracle_hoisted_blend(o, calls), self)
    cc, sk, ea = H.setup(m, p, BITS[m, p], seed=seed, ops=Ops, keys=False)
    if keys is not None:
        {"full": hk.add1DMatrices, "minimal": hk.addMinimal1DMatrices, "bsgs": hk.addBSGS1DMatrices}[keys](sk)
        want = {"full": hk.HELIB_KSS_FULL, "minimal": hk.HELIB_KSS_MIN, "bsgs": hk.HELIB_KSS_BSGS}[keys]
        assert all(hk.getKSStrategy(sk, i) == want for i in range(ea.dimension()))
    return cc, sk, ea, calls


def matrix(ea, seed, zero=None):
    """a random matrix over all slots with one zero diagonal: the entries (r, s) with coordinates(s) - coordinates(r) =
    zero (default: 1 in every dimension)"""
    from helib_amd import bgv_matmul as bm
    n, ords = ea.size(), ea.zMStar.ords
    A = np.random.default_rng(seed).integers(0, ea.p, size=(n, n))
    A[0, 0] = 1
    st = bm.strides(ords)
    s = np.arange(n)
    c = [s // st[i] % ords[i] for i in range(len(ords))]
    zero = [1] * len(ords) if zero is None else zero
    r = sum((c[i] - zero[i]) % ords[i] * st[i] for i in range(len(ords)))
    A[r, s] = 0
    return A


# ---- semantics ----
@pytest.mark.parametrize("minimal", [False, True])
@pytest.mark.parametrize("keys", ["full", "minimal"])
@pytest.mark.parametrize("m,p", [(119, 2), (255, 2), (527, 2), (803, 3)])
def test_matmul_full_against_numpy(m, p, keys, minimal):
    from helib_amd import bgv_matmul as bm, matmul_full as mf
    cc, sk, ea, calls = setup(m, p, keys)
    assert not all(ea.nativeDimension(i) for i in range(ea.dimension()))
    mat = bm.MatMulFull(ea, matrix(ea, m))
    ex = mf.MatMulFullExec(ea, mat, minimal=minimal)
    assert ex.dims == CUBES[m, p][4]
    assert len(ex.transforms) == ea.sizeOfDimension(ex.dims[0])
    assert sum(t.multiplier[i] is None and getattr(t, "multiplier1", [None] * t.D)[i] is None
               for t in ex.transforms for i in range(t.D)) == 1                 # the zero diagonal
    a = np.random.default_rng(m + 1).integers(0, p, size=(1, ea.size()))
    ct = ea.encrypt(sk, a)
    assert ex.mul(ct, pk=sk) is ct
    assert np.array_equal(ea.decrypt_batch(ct, sk), bm.mulPlain(ea, a, mat)), (m, keys, minimal)
    assert ct.isCorrect()
    if keys == "minimal" or ea.nativeDimension(ex.dims[0]):                     # iterative, or no blend in the recursion
        assert not calls
    elif p == 2:                                                                # (p > 2: unequal intFactors take the sequence)
        assert calls == [(ea.sizeOfDimension(ex.dims[0]) - 1, len(cc.digits))]  # Ctxt.fuseHoistedBlend ships True


@pytest.mark.parametrize("keys", ["bsgs", None])
def test_matmul_full_under_other_strategies(keys):
    """HELIB_KSS_BSGS and no key at all (HELIB_KSS_UNKNOWN): the per-offset sequence over the general precon"""
    from helib_amd import bgv_matmul as bm, matmul_full as mf
    m, p = 527, 2
    cc, sk, ea, calls = setup(m, p, keys or "full")
    mat = bm.MatMulFull(ea, matrix(ea, 7))
    a = np.random.default_rng(8).integers(0, p, size=(1, ea.size()))
    ct = ea.encrypt(sk, a)
    mf.MatMulFullExec(ea, mat).mul(ct, pk=sk if keys else None, fused=None if keys else False)
    assert np.array_equal(ea.decrypt_batch(ct, sk), bm.mulPlain(ea, a, mat))
    assert ct.isCorrect() and not calls


# ---- automorphBlend: one hoistedBlend against the sequence ----
def _words(ct):
    return {h: (list(part.idx), part.rows.copy()) for h, part in ct.parts.items()}


def _books(ct):
    return ct.lnNoise, ct.primeSet, ct.ptxtSpace, ct.intFactor, ct.ptxtMag, ct.lnRatFactor


def _same(xs, ys):
    assert len(xs) == len(ys)
    for x, y in zip(xs, ys):
        wx, wy = _words(x), _words(y)
        assert sorted(wx, key=str) == sorted(wy, key=str) == ["1", "s"]
        for h in wx:
            assert wx[h][0] == wy[h][0] and np.array_equal(wx[h][1], wy[h][1]), h
        assert _books(x) == _books(y)


def _pair(ea, sk, seed, dim, deep=True):
    """-> (ct, ct1, a): a ciphertext below the top level and its copy moved by g^(-ord) along the non-native `dim`"""
    rng = np.random.default_rng(seed)
    a, b = (rng.integers(0, ea.p, size=(1, ea.size())) for _ in range(2))
    ct = ea.encrypt(sk, a)
    if deep:
        ct.multiplyBy(ea.encrypt(sk, b))
        a = a * b % ea.p
        ct.cleanUp()
        ct.modDownToSet(ct.primeSet - {max(ct.primeSet)})
    ct.cleanUp()
    ct1 = ct.clone()
    ct1.smartAutomorph(ea.zMStar.genToPow(dim, -ea.sizeOfDimension(dim)))
    return ct, ct1, a


def _masks(ea, dim, offs):
    idx = set(ea.cc.ctxtPrimes) | set(ea.cc.specialPrimes)
    enc = [ea._encodedMask(ea.maskSlots(dim, i), idx) for i in offs]
    return [mk for mk, _ in enc], [sz for _, sz in enc]


def test_automorph_blend_fused_is_the_sequence():
    """(255, 2): dimension 0 is non-native with 8 coordinates; n = 1, 2, 3, below the top level, the masks on every ctxt
    and special prime.  What comes out is the rotation by i along that dimension"""
    from helib_amd import ctxt as hc
    m, p, dim = 255, 2, 0
    cc, sk, ea, calls = setup(m, p)
    z = ea.zMStar
    ct, ct1, a = _pair(ea, sk, 5, dim)
    pre = hc.BasicAutomorphPrecon(ct)
    assert set(cc.ctxtPrimes) > set(pre.ctxt.primeSet)                          # below the top level
    offs = [1, 2, 5]
    ks = [z.genToPow(dim, i) for i in offs]
    masks, sizes = _masks(ea, dim, offs)
    assert set(masks[0].idx) > set(pre.ctxt.primeSet) | set(cc.specialPrimes)
    sizes[1] = -1.0                                                             # multByConstant's default size
    for n in (1, 2, 3):
        del calls[:]
        seq = hc.automorphBlend(hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1), ks[:n], masks[:n], sizes[:n],
                                fused=False)
        one = hc.automorphBlend(hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1), ks[:n], masks[:n], sizes[:n],
                                fused=True)
        assert calls == [(n, len(pre.digits))]
        _same(seq, one)
        assert set(cc.specialPrimes) <= one[0].primeSet
        for i, x in zip(offs, one):
            want = np.roll(a.reshape(1, 8, 2), i, axis=1).reshape(1, -1)
            assert np.array_equal(ea.decrypt_batch(x, sk), want) and x.isCorrect()
    # the class switch: True as measured; False gives the sequence back
    assert hc.Ctxt.fuseHoistedBlend is True
    del calls[:]
    _same(seq, hc.automorphBlend(hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1), ks, masks, sizes))
    assert len(calls) == 1
    try:
        hc.Ctxt.fuseHoistedBlend = False
        _same(seq, hc.automorphBlend(hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1), ks, masks, sizes))
        assert len(calls) == 1
    finally:
        hc.Ctxt.fuseHoistedBlend = True
    with pytest.raises(ValueError, match="one mask and one size"):
        hc.automorphBlend(pre, pre, ks, masks[:1], None)


def test_automorph_blend_falls_back():
    from helib_amd import ctxt as hc
    # unequal intFactors (803, 3): the sequence, whose addCtxt rescales
    m, p, dim = 803, 3, 0
    cc, sk, ea, calls = setup(m, p)
    z = ea.zMStar
    ct, ct1, a = _pair(ea, sk, 6, dim, deep=False)
    ct1.intFactor = ct1.intFactor * 2 % p                   # ct1 still encrypts what it did: its parts are doubled too
    for part in ct1.parts.values():
        part.mulConstant(2)
    ks = [z.genToPow(dim, 2)]
    masks, sizes = _masks(ea, dim, [2])
    pre, pre1 = hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1)
    assert pre.ctxt.intFactor != pre1.ctxt.intFactor
    seq = hc.automorphBlend(pre, pre1, ks, masks, sizes, fused=False)
    one = hc.automorphBlend(pre, pre1, ks, masks, sizes, fused=True)
    assert not calls
    _same(seq, one)
    assert np.array_equal(ea.decrypt_batch(one[0], sk), np.roll(a.reshape(1, 6, 2), 2, axis=1).reshape(1, -1))
    # a k whose first step is another matrix (the minimal key set has g^1 alone), and the identity
    cc, sk, ea, calls = setup(255, 2, "minimal")
    z = ea.zMStar
    ct, ct1, a = _pair(ea, sk, 7, 0, deep=False)
    k2 = z.genToPow(0, 2)
    assert ct._firstStep(k2) != k2
    masks, sizes = _masks(ea, 0, [2])
    _same(hc.automorphBlend(hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1), [k2], masks, sizes, fused=False),
          hc.automorphBlend(hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1), [k2], masks, sizes, fused=True))
    assert not calls
    k1 = z.genToPow(0, 1)
    pre, pre1 = hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1)
    assert hc._blendFused(pre, pre1, [1], masks, sizes) is None and not calls
    assert hc._blendFused(pre, pre1, [k1], masks, sizes) is not None and calls == [(1, len(pre.digits))]
    # special primes in an operand, a CKKS context, another digit split: not the op's cases
    for which in (0, 1):
        pp = [hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1)]
        pp[which].ctxt.modUpToSet(pp[which].ctxt.primeSet | frozenset(cc.specialPrimes))
        assert hc._blendFused(pp[0], pp[1], [k1], masks, sizes) is None
    pre = hc.BasicAutomorphPrecon(ct)
    pre.ctxt.context = type("View", (), dict(vars(cc), ckks=True))()
    assert hc._blendFused(pre, pre1, [k1], masks, sizes) is None
    pre = hc.BasicAutomorphPrecon(ct)
    pre.digits = pre.digits[:-1] + [pre.digits[-1][:-1]]
    assert hc._blendFused(pre, pre1, [k1], masks, sizes) is None
    assert len(calls) == 1
    # a backend without the op: fused=True raises, fused=None runs the sequence quietly
    cc, sk, ea, calls = setup(255, 2, op=False)
    ct, ct1, a = _pair(ea, sk, 7, 0, deep=False)
    args = ([ea.zMStar.genToPow(0, 1)],) + _masks(ea, 0, [1])
    with pytest.raises(RuntimeError, match="no hoistedBlend"):
        hc.automorphBlend(hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1), *args, fused=True)
    assert hc.Ctxt.fuseHoistedBlend is True
    out = hc.automorphBlend(hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1), *args)
    assert np.array_equal(ea.decrypt_batch(out[0], sk), np.roll(a.reshape(1, 8, 2), 1, axis=1).reshape(1, -1))


def test_a_ckks_ciphertext_takes_the_sequence():
    from oracle import oracle as O
    from oracle.backend import OracleBackend, OracleOps
    from helib_amd import ctxt as hc, keys as hk
    cc = hc.ChainContext(128, -1, 20, bits=200, c=2, ckks=True)
    octx = O.Ctx(128)
    for q in cc.primes:
        octx.add_prime(q)
    calls = []

    class Ops(OracleOps):
        hoistedBlend = MR.oracle_hoisted_blend(octx, calls)
    be = OracleBackend(octx, cc)
    be.ops = Ops(octx)
    sk = hk.SecKey(cc, be, 7)
    sk.GenSecKey()
    sk.GenKeySWmatrix(1, 5)
    f = float(1 << 20)
    ct = sk.CKKSencrypt(np.arange(cc.phim, dtype=np.int64), 1.0, f)
    ct1 = sk.CKKSencrypt(np.arange(cc.phim, dtype=np.int64)[::-1].copy(), 1.0, f)
    mk = be.fromCoeffs(sorted(set(cc.ctxtPrimes) | set(cc.specialPrimes)), [1] + [0] * (cc.phim - 1))
    out = {}
    for fused in (False, True):
        x, = hc.automorphBlend(hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1), [5], [mk], [1.0], fused=fused)
        out[fused] = x
    assert not calls
    for h in out[True].parts:
        assert np.array_equal(out[True].parts[h].rows, out[False].parts[h].rows)


# ---- the whole product through the op ----
@pytest.mark.parametrize("m,p,fuses", [(527, 2, True), (255, 2, False), (803, 3, None)])
def test_matmul_full_counts_its_fused_calls(m, p, fuses):
    """(527, 2) under HELIB_KSS_FULL: the recursion runs along the non-native dimension of two coordinates, so one
    hoistedBlend of one term, and the product is the unfused one word for word.  (255, 2): the recursion runs along
    the native dimension -- no blend at all.  (803, 3): the request reaches automorphBlend; whether the op runs depends
    on the intFactor the key switch left on the moved copy, and where it differs the sequence runs -- either way the
    ciphertext is the sequence's"""
    from helib_amd import bgv_matmul as bm, ctxt as hc, matmul_full as mf
    cc, sk, ea, calls = setup(m, p)
    mat = bm.MatMulFull(ea, matrix(ea, m + 2))
    ex = mf.MatMulFullExec(ea, mat)
    a = np.random.default_rng(m + 3).integers(0, p, size=(1, ea.size()))
    seen, real = [], hc.automorphBlend

    def spy(pre, pre1, *args, **kw):
        seen.append(pre.ctxt.intFactor == pre1.ctxt.intFactor)
        return real(pre, pre1, *args, **kw)
    out, ct0 = {}, ea.encrypt(sk, a)
    hc.automorphBlend = spy
    try:
        for fused in (False, True):
            ct = ct0.clone()
            ex.mul(ct, pk=sk, fused=fused)
            assert np.array_equal(ea.decrypt_batch(ct, sk), bm.mulPlain(ea, a, mat)) and ct.isCorrect()
            out[fused] = ct
    finally:
        hc.automorphBlend = real
    _same([out[False]], [out[True]])
    ndig = len(hc.BasicAutomorphPrecon(ea.encrypt(sk, a)).digits)
    if fuses is True:
        assert seen == [True] and calls == [(1, ndig)]
    elif fuses is False:
        assert not seen and not calls
    else:
        assert len(seen) == 1 and calls == ([(1, ndig)] if seen[0] else [])


def test_unequal_int_factors_are_not_fused_in_the_product():
    """(803, 3) with the moved copy's intFactor made to differ: hoistedBlend is not called, the product is right"""
    from helib_amd import bgv_matmul as bm, ctxt as hc, matmul_full as mf
    m, p = 803, 3
    cc, sk, ea, calls = setup(m, p)
    mat = bm.MatMulFull(ea, matrix(ea, 11))
    ex = mf.MatMulFullExec(ea, mat)
    a = np.random.default_rng(12).integers(0, p, size=(1, ea.size()))
    real = hc.BasicAutomorphPrecon.__init__
    made = []

    def init(self, ct):
        real(self, ct)
        made.append(self)
        if len(made) == 2:                                  # the precon of ct1: the same plaintext under another factor
            self.ctxt.intFactor = self.ctxt.intFactor * 2 % p
            for part in self.ctxt.parts.values():
                part.mulConstant(2)
            self.polyDigits = hc.BasicAutomorphPrecon(self.ctxt).polyDigits
    ct = ea.encrypt(sk, a)
    hc.BasicAutomorphPrecon.__init__ = init
    try:
        ex.mul(ct, pk=sk, fused=True)
    finally:
        hc.BasicAutomorphPrecon.__init__ = real
    assert len(made) >= 2 and not calls
    assert np.array_equal(ea.decrypt_batch(ct, sk), bm.mulPlain(ea, a, mat)) and ct.isCorrect()


# ---- refusals ----
def test_what_stays_refused():
    from helib_amd import bgv_hypercube as bh, bgv_matmul as bm, ckks, matmul_full as mf
    cc, sk, ea, calls = setup(255, 2, keys=None)
    full = np.eye(ea.size(), dtype=np.int64)
    with pytest.raises(ckks.LogicError, match="out of scope"):
        bh.MatMulFullExec(ea, full)
    with pytest.raises(ckks.LogicError, match="non-native"):
        bm.MatMulFullExec(ea, full)
    assert bm.MatMulFullExec.exec1D is bm.MatMul1DExec and mf.MatMulFullExec.exec1D is bh.MatMul1DExec
    view = type("PR", (), {"r": 2, "p": 2})()
    with pytest.raises(ckks.LogicError, match="r > 1"):
        mf.MatMulFullExec(view, full)
    one = type("One", (), {"r": 1, "p": 2, "size": lambda self: 1, "dimension": lambda self: 0})()
    with pytest.raises(ckks.LogicError, match="less than 2"):
        mf.MatMulFullExec(one, np.eye(1, dtype=np.int64))


# ---- declarations ----
def test_symbol_is_declared_bound_listed_and_exported():
    from helib_amd import build, capi, keys as hk
    header = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    so = build.build()
    dyn = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    lib = capi.lib()
    assert re.search(r"\bint hx_hoisted_blend\(", header)
    assert "hx_hoisted_blend" in capi.SYMBOLS
    assert re.search(r" T hx_hoisted_blend$", dyn, re.M)
    assert len(lib.hx_hoisted_blend.argtypes) == 14
    assert "src/matmul.cpp:2174-2204" in header and "src/matmul.cpp:48-184" in header
    text = subprocess.run(["nm", "-C", so], capture_output=True, text=True, check=True).stdout
    assert "hoisted_blend_kernel" in text and "hoisted_perm_kernel" in text
    assert hasattr(hk.HxBackend, "hoistedBlend") and callable(capi.hoistedBlend)
    with pytest.raises(capi.InvalidArgument, match="are required"):         # the binding refuses before it reaches the library
        capi.hoistedBlend(None, None, None, None, None, None, [2], [None], [None], [])
    six = [object()] * 6
    with pytest.raises(capi.InvalidArgument, match="one matrix for each"):
        capi.hoistedBlend(*six, [2, 4], [object()], [object()], [])
    with pytest.raises(capi.InvalidArgument, match="one mask per automorphism"):
        capi.hoistedBlend(*six, [2], [object()], [None], [])
