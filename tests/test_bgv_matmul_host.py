"""BGV matrix products (helib_amd.bgv_matmul: MatMul1DExec, MatMulFullExec) on the host side (no GPU): the control flow
over the oracle backend with a CPU encoder -- the host construction path -- with real keys of each family, held to
numpy on the plaintext slots; the diagonal descriptor against a literal transcription of the reference's
processDiagonal loops; fused against term by term; the new entry points' declarations.  Everything is an integer:
every comparison is exact."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_linalg_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (m, p, orders of the hypercube, bits).  bits = 300 / 400: enough for the reference's bookkeeping to call every
# result below correct (Ctxt.isCorrect and capacity > 0, asserted after each product), the MatMulFullExec under
# minimal keys (chained key switches per rotation) being the deepest
RINGS = [(16, 17, [4, 2], 300), (105, 211, [12, 2, 2], 400)]
FAMILIES = ["add1DMatrices", "addBSGS1DMatrices", "addMinimal1DMatrices"]


def _ords(m, p):
    return list(hostnt.ZmStar(m, p).ords)


def test_the_rings_are_what_they_are_taken_for():
    for m, p, ords, _ in RINGS:
        assert hostnt.is_prime(p) and p % m == 1
        got = _ords(m, p)
        assert got == ords and int(np.prod(got)) == sum(math.gcd(j, m) == 1 for j in range(m)), (m, got)
    assert len(_ords(105, 211)) == 3 and int(np.prod(_ords(105, 211))) == 48 and int(np.prod(_ords(16, 17))) == 8


def _setup(m, p, bits, family=None, seed=3, ops=None):
    from oracle import oracle as O
    from oracle.backend import OracleBackend
    from helib_amd import bgv, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, 1, bits=bits, c=2)
    o = O.Ctx(m)
    for q in cc.primes:
        o.add_prime(q)

    class Backend(OracleBackend):
        def fromCoeffsBatch(self, idx, polys):
            assert len(polys) == 1
            d = self.fromCoeffs(idx, polys[0])
            d.batch = 1
            return d
    be = Backend(o, cc)
    if ops is not None:
        be.ops = ops(o)
    sk = hk.SecKey(cc, be, seed=seed)
    sk.GenSecKey()
    ea = bgv.EncryptedArray(cc, None, encoder=L.HostEncoder(be, m, p))
    sk.zMStar = ea.zMStar
    if family is not None:
        getattr(hk, family)(sk)
    return cc, sk, ea


def _ea_without_keys(m, p):
    from helib_amd import bgv, ctxt as hc
    return bgv.EncryptedArray(hc.ChainContext(m, p, 1, bits=100, c=2), None, encoder=L.HostEncoder(None, m, p))


def _banded(D, rng, p, band=(0, 1)):
    """non-zero only on the diagonals i in `band` and D - 1: A[(j - i) mod D, j]"""
    a = np.zeros((D, D), dtype=np.int64)
    j = np.arange(D)
    for i in set(band) | {D - 1}:
        a[(j - i) % D, j] = rng.integers(1, p, size=D)
    return a


# ---- the descriptor against the reference's loops ----
def _add_coord(ea, i, k, offset):
    """CubeSignature::addCoord (include/helib/hypercube.h:115-131)"""
    ords, st = ea.zMStar.ords, L.strides(ea.zMStar.ords)
    offset %= ords[i]
    c = ea.coordinate(i, k)
    return k + ((c + offset) % ords[i] - c) * st[i]


def _rotate1d_plain(ea, vec, i, offset):
    """EncryptedArrayBase::rotate1D on a vector (include/helib/EncryptedArray.h:382-394)"""
    out = [None] * len(vec)
    for j in range(len(vec)):
        out[_add_coord(ea, i, j, offset)] = vec[j]
    return out


def _process_diagonal1(ea, get, dim, i, p):
    """MatMul1D_derived_impl::processDiagonal1 (src/matmul.cpp:449-504), zero entries and all"""
    D = ea.sizeOfDimension(dim)
    tmp = [get((j - i) % D, j) % p for j in range(D)]
    return [tmp[ea.coordinate(dim, j)] for j in range(ea.size())]


@pytest.mark.parametrize("m,p", [(16, 17), (105, 211)])
def test_descriptor_equals_the_process_diagonal_loops(m, p):
    from helib_amd import bgv_matmul as M, keys as hk
    ea = _ea_without_keys(m, p)
    n, nd = ea.size(), ea.dimension()
    rng = np.random.default_rng(m)
    # 1D matrices: every dimension, every diagonal, every rotation MatMul1DExec_construct asks for (g = 0 and BSGS)
    for dim in range(nd):
        D = ea.sizeOfDimension(dim)
        a = rng.integers(0, p, size=(D, D))
        a[rng.integers(0, D), :] = 0
        mat = M.MatMul1D(ea, a, dim)
        for i in range(D):
            want = _process_diagonal1(ea, lambda r, c: int(a[r, c]), dim, i, p)
            assert mat.processDiagonal(i).tolist() == want, (dim, i)
            for g in (0, hk.KSGiantStepSize(D)):
                amt = -g * (i // g) if g else 0
                rot = _rotate1d_plain(ea, want, dim, amt)           # plaintextAutomorph at d = 1 (:375-389)
                assert M.diagonalSlots(ea, a, dim, mat.offsets(i), dim, amt).tolist() == rot, (dim, i, g)
    # the full matrix: MatMulFullExec_construct::rec_mul (:2035-2075) carrying the index vector through rotate1D
    a = rng.integers(0, p, size=(n, n))
    full = M.MatMulFull(ea, a)
    dims = sorted(range(nd), key=lambda i: ea.sizeOfDimension(i))
    seen = []

    def rec(d, idxes, off):
        if d >= nd - 1:
            last = dims[d]
            D = ea.sizeOfDimension(last)
            helper = M._FullHelper(full, off, last)
            for i in range(D):
                idx1 = _rotate1d_plain(ea, idxes, last, i)            # MatMulFullHelper::processDiagonal (:1998-2024)
                want = [int(a[idx1[j], j]) for j in range(n)]
                assert helper.processDiagonal(i).tolist() == want, (off, i)
                g = hk.KSGiantStepSize(D)
                amt = -g * (i // g)
                assert M.diagonalSlots(ea, a, -1, helper.offsets(i), last, amt).tolist() == \
                    _rotate1d_plain(ea, want, last, amt), (off, i)
                seen.append(tuple(helper.offsets(i)))
            return
        for o in range(ea.sizeOfDimension(dims[d])):
            off1 = list(off)
            off1[dims[d]] = o
            rec(d + 1, _rotate1d_plain(ea, idxes, dims[d], o), off1)
    rec(0, list(range(n)), [0] * nd)
    assert len(set(seen)) == n                                        # phi(m) diagonals, all different


# ---- with real keys ----
def _check(ct, ea, sk, want, what):
    assert np.array_equal(ea.decrypt_batch(ct, sk), want), what
    assert ct.isCorrect() and ct.capacity() > 0, what


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("m,p,ords,bits", RINGS)
def test_matmul_against_numpy(m, p, ords, bits, family):
    from helib_amd import bgv_matmul as M, keys as hk
    cc, sk, ea = _setup(m, p, bits, family)
    n = ea.size()
    rng = np.random.default_rng(m)
    v = rng.integers(0, p, size=(1, n))
    minimal = family == "addMinimal1DMatrices"
    for dim in range(ea.dimension()):
        D = ea.sizeOfDimension(dim)
        assert hk.getKSStrategy(sk, dim) == {"add1DMatrices": hk.HELIB_KSS_FULL, "addBSGS1DMatrices": hk.HELIB_KSS_BSGS,
                                             "addMinimal1DMatrices": hk.HELIB_KSS_MIN}[family]
        for a in (rng.integers(-p, 2 * p, size=(D, D)), _banded(D, rng, p) if D > 3 else None):
            if a is None:
                continue
            mat = M.MatMul1D(ea, a, dim)
            ex = M.MatMul1DExec(ea, mat, minimal=minimal)
            assert not ex.onDevice and ex.dim == dim
            ct = ea.encrypt(sk, v)
            assert ex.mul(ct, pk=sk) is ct
            # the 1D map by hand: along `dim`, independently for every setting of the other coordinates
            x = np.moveaxis(v.reshape([1] + ords), 1 + dim, -1)
            want = np.moveaxis(x @ (a % p) % p, -1, 1 + dim).reshape(1, n)
            assert np.array_equal(M.mulPlain(ea, v, mat), want)
            _check(ct, ea, sk, want, (family, dim))
    a = rng.integers(0, p, size=(n, n))
    ex = M.MatMulFullExec(ea, a, minimal=minimal)
    assert len(ex.transforms) == n // ea.sizeOfDimension(ex.dims[-1])
    assert [ea.sizeOfDimension(i) for i in ex.dims] == sorted(ords)
    ct = ea.encrypt(sk, v)
    assert ex.mul(ct, pk=sk) is ct
    _check(ct, ea, sk, (v @ a) % p, (family, "full"))


def test_banded_matrix_keeps_no_multiplier_for_a_zero_diagonal():
    from helib_amd import bgv_matmul as M
    m, p, ords, bits = RINGS[1]
    cc, sk, ea = _setup(m, p, bits, "add1DMatrices")
    rng = np.random.default_rng(7)
    dim = ords.index(12)
    a = _banded(12, rng, p, band=(0, 2))
    a[a != 0] += p * rng.integers(-1, 2, size=int(np.count_nonzero(a)))        # values outside [0, p)
    a[0, 3] = 3 * p                                                            # and a multiple of p: zero
    for minimal in (False, True):
        ex = M.MatMul1DExec(ea, M.MatMul1D(ea, a, dim), minimal=minimal)
        assert ex.g == (4 if minimal else 0)
        assert [i for i, mm in enumerate(ex.multiplier) if mm is not None] == [0, 2, 11]
        for mm in ex.multiplier:
            assert mm is None or (mm[0].batch == 1 and mm[1] > 0)
    # a callable matrix takes the same path to the same constants
    by_call = M.MatMul1DExec(ea, M.MatMul1D(ea, lambda i, j: int(a[i, j]), dim), minimal=True)
    for x, y in zip(by_call.multiplier, ex.multiplier):
        assert (x is None) == (y is None)
        if x is not None:
            assert x[1] == y[1] and np.array_equal(x[0].rows, y[0].rows)
    # a full matrix that only moves slots along the last dimension of the product: one live transform
    n = ea.size()
    full = np.zeros((n, n), dtype=np.int64)
    full[np.arange(n), np.arange(n)] = rng.integers(1, p, size=n)
    fx = M.MatMulFullExec(ea, full)
    live = [sum(mm is not None for mm in t.multiplier) for t in fx.transforms]
    assert live == [1] + [0] * (len(fx.transforms) - 1)
    v = rng.integers(0, p, size=(1, n))
    ct = ea.encrypt(sk, v)
    fx.mul(ct, pk=sk)
    _check(ct, ea, sk, (v @ full) % p, "diagonal full matrix")


def test_constants_are_what_mult_by_constant_of_the_zzx_builds():
    """multiplier[i] = (DoubleCRT(balanced zzX), embeddingLargestCoeff(zzX)): ConstMultiplier_zzX::upgrade
    (src/matmul.cpp:355-363)"""
    from helib_amd import bgv_matmul as M
    m, p, ords, bits = RINGS[0]
    cc, sk, ea = _setup(m, p, bits)
    a = np.random.default_rng(2).integers(0, p, size=(4, 4))
    for minimal in (False, True):
        ex = M.MatMul1DExec(ea, M.MatMul1D(ea, a, 0), minimal=minimal)
        assert ex.g == 0
        idx = list(cc.ctxtPrimes) + list(cc.specialPrimes)
        for i, (d, size) in enumerate(ex.multiplier):
            zzx = ea.encodeCoeffs(M.diagonalSlots(ea, a, 0, [i, 0], 0, 0))[0]
            assert np.array_equal(d.rows, sk.be.fromCoeffs(idx, zzx).rows)
            assert size == sk.be.embeddingLargestCoeff(zzx)


# ---- fused against term by term ----
def _fused_ops():
    from oracle.backend import OracleOps
    calls = []

    class Ops(OracleOps):
        @staticmethod
        def mulAddMany(out0, out1, consts, in0, in1, accumulate=True):
            calls.append(len(consts))
            for out, ins in ((out0, in0), (out1, in1)):
                if out is None:
                    continue
                if not accumulate:
                    out.rows[:] = 0
                for c, x in zip(consts, ins):
                    t = x.copy()
                    t *= c
                    out += t
    return Ops, calls


@pytest.mark.parametrize("family", FAMILIES)
def test_fused_and_termwise_agree(family):
    """an oracle backend that offers mulAddMany (as copy, *=, += on its own polys): fused=True then runs the host side
    of the fused path and must leave the words and the bookkeeping of fused=False.  m = 105 along the dimension of
    order 12: g = 0 as it stands, BSGS with g = 4 under minimal=True (12 > HELIB_KEYSWITCH_MIN_THRESH); the baby
    steps are hoisted whenever the key's strategy for the dimension is FULL or BSGS."""
    from helib_amd import bgv_matmul as M, linalg
    m, p, ords, bits = RINGS[1]
    Ops, calls = _fused_ops()
    dim = ords.index(12)
    rng = np.random.default_rng(11)
    a = rng.integers(0, p, size=(12, 12))
    v = rng.integers(0, p, size=(1, 48))
    want = np.moveaxis(np.moveaxis(v.reshape([1] + ords), 1 + dim, -1) @ a % p, -1, 1 + dim).reshape(1, 48)
    for minimal in (False, True):
        out = {}
        for fused in (True, False):
            cc, sk, ea = _setup(m, p, bits, family, seed=2, ops=Ops)
            ex = M.MatMul1DExec(ea, M.MatMul1D(ea, a, dim), minimal=minimal)
            assert ex.g == (4 if minimal else 0)
            ct = ea.encrypt(sk, v)
            del calls[:]
            before = linalg.MatMul1DExec.fallbacks
            ex.mul(ct, pk=sk, fused=fused)
            fell = linalg.MatMul1DExec.fallbacks - before
            if not fused:
                assert not calls and fell == 0
            else:
                assert calls
                if ex.g and family != "addMinimal1DMatrices":
                    assert fell == 0 and calls == [4, 4, 4]       # hoisted baby steps: every group fuses
            _check(ct, ea, sk, want, (family, minimal, fused))
            out[fused] = ct
        x, y = out[True], out[False]
        assert (x.lnNoise, x.primeSet, x.intFactor, x.ptxtSpace) == (y.lnNoise, y.primeSet, y.intFactor, y.ptxtSpace)
        assert sorted(x.parts) == sorted(y.parts)
        for h in x.parts:
            assert np.array_equal(x.parts[h].rows, y.parts[h].rows)


# ---- refusals and declarations ----
def test_error_cases():
    from helib_amd import bgv_matmul as M, ckks
    ea = _ea_without_keys(16, 17)
    with pytest.raises(ckks.LogicError):
        M.MatMul1D(ea, np.zeros((4, 4), dtype=np.int64), 2)
    with pytest.raises(ckks.LogicError):
        M.MatMul1D(ea, np.zeros((3, 3), dtype=np.int64), 0)
    with pytest.raises(ckks.LogicError):
        M.MatMulFull(ea, np.zeros((4, 4), dtype=np.int64))
    with pytest.raises(ckks.LogicError):
        M.MatMul1DExec(ea, np.zeros((4, 4), dtype=np.int64))
    ea.zMStar.SameOrd = lambda i: False
    with pytest.raises(ckks.LogicError, match="non-native"):
        M.MatMul1DExec(ea, np.ones((4, 4), dtype=np.int64), dim=0)


def test_diagonal_entry_points_are_declared_bound_and_exported():
    from helib_amd import bgv, capi
    hdr = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    declared = set(re.findall(r"\b(hx_[a-zA-Z0-9_]+)\s*\(", hdr))
    names = ("hx_bgv_matrix_create", "hx_bgv_matrix_destroy", "hx_bgv_encode_diagonals")
    for s in names:
        assert s in capi.SYMBOLS and s in declared, s
    assert re.search(r"typedef struct hx_bgv_diag \{\s*int32_t off\[8\];\s*int32_t rot_dim, rot_amt;\s*\} hx_bgv_diag;", hdr)
    assert "src/matmul.cpp:375-389" in hdr
    lib = capi.lib()                      # the cross-compiled library
    assert len(lib.hx_bgv_matrix_create.argtypes) == 6 and len(lib.hx_bgv_encode_diagonals.argtypes) == 7
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi._SO], text=True)
    for s in names:
        assert re.search(r"\bT %s$" % s, out, re.M), s
    assert re.search(r"bgv_diag_scatter_kernel", subprocess.check_output(["nm", "-C", capi._SO], text=True))
    d = capi.bgvDiags([([1, -2, 3], 2, -5), ([0], -1, 0)])
    assert d.dtype == np.int32 and d.shape == (2, 10)
    assert d[0].tolist() == [1, -2, 3, 0, 0, 0, 0, 0, 2, -5] and d[1].tolist() == [0] * 8 + [-1, 0]
    for f in ("matrix", "encodeDiagonals", "split"):
        assert hasattr(bgv.DeviceEncoder, f)
    assert hasattr(capi, "BgvMatrix") and hasattr(capi, "bgvEncodeDiagonals")
