"""BGV linear-array rotate / shift / totalSums / runningSums (helib_amd.bgv.EncryptedArray) on the host side (no GPU):
the control flow over the oracle backend with a CPU encoder, one vector at a time, against numpy on the plaintext
slots; the masks against a literal restatement of genMaskTable; the noise bookkeeping; the new entry point's
declaration.  The oracle backend has no fused mask split, so the composition runs term by term here, except where a
test hands it one."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_linalg_ref as L
from tests import bgv_slots_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (m, p, bits): one, two, two and three generators
RINGS = [(17, 103, 200), (45, 181, 300), (1024, 12289, 300), (105, 211, 400)]


def test_the_rings_are_what_they_are_taken_for():
    for (m, p, _), ngens in zip(RINGS, (1, 2, 2, 3)):
        assert hostnt.is_prime(p) and p % m == 1
        assert hostnt.ZmStar(m, p).numOfGens() == ngens


def _setup(m, p, bits, amts=(), seed=3, ops=None):
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
    for k in L.needed_automorphisms(ea.zMStar, amts):
        sk.GenKeySWmatrix(1, k)
    sk.setKeySwitchMap()
    return cc, sk, ea


# ---- the CPU encoder and the masks ----
@pytest.mark.parametrize("m,p", [(17, 103), (45, 181)])
def test_host_encoder_equals_the_literal_crt(m, p):
    enc = L.HostEncoder(None, m, p)
    n = enc.V.shape[0]
    a = np.random.default_rng(m).integers(0, p, size=(2, n))
    cf = enc.coeffs(a)
    for b in range(2):
        assert np.array_equal(cf[b], R.encode_crt(a[b], m, p))
    assert np.array_equal(enc.embed(cf), a)


def _ea_without_keys(m, p):
    from helib_amd import bgv, ctxt as hc
    return bgv.EncryptedArray(hc.ChainContext(m, p, 1, bits=100, c=2), None, encoder=L.HostEncoder(None, m, p))


@pytest.mark.parametrize("m,p", [(17, 103), (45, 181), (105, 211)])
def test_mask_slots_against_gen_mask_table(m, p):
    """genMaskTable (src/PAlgebra.cpp:1316-1338) restated literally over the idempotents crtTable[k] =
    encode_crt(unit vector k), as polynomials mod p; maskSlots(i, j) must be their slots"""
    ea = _ea_without_keys(m, p)
    z, n = ea.zMStar, ea.size()
    pts = R.points(m, p)
    crt = [R.encode_crt(np.eye(n, dtype=np.int64)[k], m, p, pts) for k in range(n)]
    for i in range(z.numOfGens()):
        ord_ = z.OrderOf(i)
        table = [None] * (ord_ + 1)
        table[ord_] = np.zeros(n, dtype=np.int64)
        for j in range(ord_ - 1, 0, -1):
            table[j] = table[j + 1].copy()
            for k in range(n):
                if ea.coordinate(i, k) == j:
                    table[j] = (table[j] + crt[k]) % p
        table[0] = np.zeros(n, dtype=np.int64)
        table[0][0] = 1
        for j in range(ord_ + 1):
            slots = ea.maskSlots(i, j)
            assert np.array_equal(R.decode(table[j][None], m, p, pts)[0], slots), (i, j)
            assert np.array_equal(R.balanced(table[j], p), ea.enc.coeffs(slots)[0]), (i, j)
        assert ea.maskSlots(i, 0).all() and not ea.maskSlots(i, ord_).any()
        assert np.array_equal(ea.maskSlots(i, 1), [int(ea.coordinate(i, k) >= 1) for k in range(n)])


def _polymulmod(a, b, m, p):
    """a * b mod (Phi_m, p), coefficient vectors of length phi(m), lowest first"""
    n = len(a)
    prod = np.zeros(m, dtype=np.int64)
    full = np.convolve(a % p, b % p) % p
    for k, c in enumerate(full):                    # mod X^m - 1
        prod[k % m] = (prod[k % m] + c) % p
    phi = np.array([1], dtype=np.int64)             # Phi_m mod p: the product over the primitive roots; monic, degree n
    for r in R.primitive_roots(m, p):
        phi = np.convolve(phi, np.array([(p - r) % p, 1], dtype=np.int64)) % p
    for k in range(m - 1, n - 1, -1):
        c = prod[k]
        if c:
            prod[k - n:k + 1] = (prod[k - n:k + 1] - c * phi) % p
    return prod[:n]


def test_mask_update_is_slotwise():
    """mask * (M[i][v] - M[i][v + 1]) + M[i][v + 1] mod Phi_m (src/EncryptedArray.cpp:280-281) as polynomials against
    EncryptedArray._nextMask on the slots, m = 45 (two generators)"""
    m, p = 45, 181
    ea = _ea_without_keys(m, p)
    enc = ea.enc
    last = ea.dimension() - 1
    for v_last in (1, ea.sizeOfDimension(last) - 1):
        for v in (0, 1, ea.sizeOfDimension(0) - 1):
            mask = ea.maskSlots(last, v_last)
            a, b = ea.maskSlots(0, v), ea.maskSlots(0, v + 1)
            poly = (_polymulmod(enc.coeffs(mask)[0], (enc.coeffs(a)[0] - enc.coeffs(b)[0]) % p, m, p)
                    + enc.coeffs(b)[0]) % p
            want = enc.embed(poly[None])[0]
            got = ea._nextMask(mask, 0, v)
            assert np.array_equal(got, want) and set(np.unique(got)) <= {0, 1}, (v_last, v)


# ---- rotate / shift / sums against numpy ----
@pytest.mark.parametrize("m,p,bits", RINGS)
def test_rotate_and_shift_against_numpy(m, p, bits):
    z = hostnt.ZmStar(m, p)
    n = z.getNSlots()
    amts = L.amounts(z.ords)
    cc, sk, ea = _setup(m, p, bits, amts)
    a = np.random.default_rng(m).integers(0, p, size=(1, n))
    for amt in amts:
        ct = ea.encrypt(sk, a)
        assert ea.rotate(ct, amt) is ct
        assert np.array_equal(ea.decrypt_batch(ct, sk), L.rotate(a, amt)), ("rotate", amt)
        assert ct.isCorrect()
    for k in amts + [-(n - 1), -(n + 3), 2 * n, -2 * n - 1]:
        ct = ea.encrypt(sk, a)
        assert ea.shift(ct, k) is ct
        got = ea.decrypt_batch(ct, sk)
        assert np.array_equal(got, L.shift(a, k)), ("shift", k)
        if abs(k) >= n:
            assert not ct.parts and not got.any()
        else:
            assert ct.isCorrect()


@pytest.mark.parametrize("m,p,bits", [(17, 103, 200), (45, 181, 500), (1024, 12289, 900), (105, 211, 900)])
def test_sums_against_numpy(m, p, bits):
    z = hostnt.ZmStar(m, p)
    n = z.getNSlots()
    sh, rot = L.sums_amounts(n)
    cc, sk, ea = _setup(m, p, bits, sh + rot)
    a = np.random.default_rng(m + 1).integers(0, p, size=(1, n))
    ct = ea.encrypt(sk, a)
    assert ea.totalSums(ct) is ct
    assert np.array_equal(ea.decrypt_batch(ct, sk), L.total_sums(a, p))
    assert ct.isCorrect()
    ct = ea.encrypt(sk, a)
    assert ea.runningSums(ct) is ct
    assert np.array_equal(ea.decrypt_batch(ct, sk), L.running_sums(a, p))
    assert ct.isCorrect()


def test_shift1d_cases():
    m, p = 45, 181
    z = hostnt.ZmStar(m, p)
    ords, st = z.ords, L.strides(z.ords)
    cases = [(i, k) for i in range(2) for k in (1, -1, ords[i] - 1, 1 - ords[i])]
    cc, sk, ea = _setup(m, p, 300, [st[i] * (k % ords[i]) for i, k in cases])
    n = ea.size()
    a = np.random.default_rng(8).integers(1, p, size=(1, n))
    coords = [np.arange(n) // st[i] % ords[i] for i in range(2)]
    for i, k in cases:
        ct = ea.encrypt(sk, a)
        ea.shift1D(ct, i, k)
        want = np.zeros_like(a)
        ok = (coords[i] + k >= 0) & (coords[i] + k < ords[i])        # what does not fall off the end
        want[:, (np.arange(n) + k * st[i])[ok]] = a[:, ok]
        assert np.array_equal(ea.decrypt_batch(ct, sk), want), (i, k)
    for k in (ords[0], -ords[0], ords[0] + 2):                       # |k| >= ord clears
        ct = ea.encrypt(sk, a)
        ct.intFactor = 5
        ea.shift1D(ct, 0, k)
        assert not ct.parts and ct.intFactor == 1 and ct.lnNoise == -math.inf
        assert ct.primeSet == frozenset(cc.ctxtPrimes)
        other = ea.encrypt(sk, a)
        ct += other                                                  # Ctxt::addCtxt into an empty ciphertext copies
        assert np.array_equal(ea.decrypt_batch(ct, sk), a) and ct.lnNoise == other.lnNoise


# ---- bookkeeping ----
def test_noise_after_rotate_by_hand():
    """rotate in two dimensions (m = 45), both coordinates of the amount non-zero, replayed with the Ctxt primitives
    the reference's text names (src/EncryptedArray.cpp:209-283) and a mask polynomial made by the literal CRT: the
    same words and the same lnNoise; at the split, tmp.lnNoise = lnNoise + ln(size) and the difference carries the
    sum of both bounds (Ctxt::multByConstant src/Ctxt.cpp:1832-1856, Ctxt::addCtxt :1405-1556)"""
    from helib_amd import ctxt as hc
    m, p = 45, 181
    z = hostnt.ZmStar(m, p)
    st = L.strides(z.ords)
    amt = 2 * st[0] + 1
    cc, sk, ea = _setup(m, p, 300, [amt], seed=6)
    _, sk2, ea2 = _setup(m, p, 300, [amt], seed=6)
    a = np.random.default_rng(4).integers(0, p, size=(1, ea.size()))
    ct, by_hand = ea.encrypt(sk, a), ea2.encrypt(sk2, a)
    ea.rotate(ct, amt)
    # by hand
    v1, v0 = 1, 2
    by_hand.smartAutomorph(z.genToPow(1, v1))
    slots = np.array([int(ea.coordinate(1, k) >= v1) for k in range(ea.size())])
    poly = R.encode_crt(slots, m, p)
    size = sk2.be.embeddingLargestCoeff(poly)
    before = by_hand.lnNoise
    tmp = by_hand.clone()
    tmp.multByConstant(sk2.be.fromCoeffs(sorted(tmp.primeSet), poly), size)
    by_hand -= tmp
    assert math.isclose(tmp.lnNoise, before + math.log(size), rel_tol=1e-12)
    assert math.isclose(by_hand.lnNoise, math.log(math.exp(before) + math.exp(before) * size), rel_tol=1e-12)
    tmp.smartAutomorph(z.genToPow(0, v0))
    by_hand.smartAutomorph(z.genToPow(0, v0 + 1))
    by_hand += tmp
    assert ct.lnNoise == by_hand.lnNoise and ct.primeSet == by_hand.primeSet
    assert (ct.intFactor, ct.ptxtSpace) == (by_hand.intFactor, by_hand.ptxtSpace)
    for h in ("1", "s"):
        assert np.array_equal(ct.parts[h].rows, by_hand.parts[h].rows)
    assert np.array_equal(ea.decrypt_batch(ct, sk), L.rotate(a, amt))
    # the split on its own
    ct = ea.encrypt(sk, a)
    before = ct.lnNoise
    mask = ea.maskSlots(1, 1)
    tmp = ea._maskSplit(ct, mask)
    size = ea._encodedMask(mask, ct.primeSet)[1]
    assert math.isclose(size, sk.be.embeddingLargestCoeff(R.encode_crt(mask, m, p)), rel_tol=1e-12)
    assert tmp.lnNoise == before + hc._ln(size) and ct.lnNoise == hc.logaddexp(before, tmp.lnNoise)
    assert np.array_equal(ea.decrypt_batch(tmp, sk), a * mask) and np.array_equal(ea.decrypt_batch(ct, sk), a * (1 - mask))


def test_fused_and_termwise_bookkeeping_agree_on_the_host():
    """an oracle backend that offers maskSplit / likeUninit (as copy, *=, -= on its own polys): fused=True then runs
    the host side of the fused path, and must leave what fused=False leaves; the plain oracle backend refuses
    fused=True"""
    from oracle.backend import OracleOps
    from helib_amd import ckks
    calls = []

    class Ops(OracleOps):
        @staticmethod
        def likeUninit(poly):
            q = poly.copy()
            q.rows[:] = 12345
            return q

        @staticmethod
        def maskSplit(k0, k1, t0, t1, mask):
            calls.append(k1 is not None)
            for k, t in ((k0, t0), (k1, t1)):
                if k is not None:
                    t.rows[:] = k.rows
                    t *= mask
                    k -= t
    m, p = 105, 211
    z = hostnt.ZmStar(m, p)
    amt = sum(L.strides(z.ords)) * 2 + 1
    sh, rot = L.sums_amounts(z.getNSlots())
    out = {}
    for fused in (True, False):
        cc, sk, ea = _setup(m, p, 400, [amt, -amt] + rot[:2] + sh[:2], seed=2, ops=Ops)
        a = np.random.default_rng(1).integers(0, p, size=(1, ea.size()))
        res = []
        for op, arg in (("rotate", amt), ("shift", amt), ("shift", -amt)):
            ct = ea.encrypt(sk, a)
            getattr(ea, op)(ct, arg, fused=fused)
            want = L.rotate(a, arg) if op == "rotate" else L.shift(a, arg)
            assert np.array_equal(ea.decrypt_batch(ct, sk), want), (op, arg, fused)
            res.append(ct)
        out[fused] = res
        if fused:
            ncalls = len(calls)
    assert len(calls) == ncalls > 0 and all(calls)       # two parts at a time, and only under fused=True
    for x, y in zip(out[True], out[False]):
        assert (x.lnNoise, x.primeSet, x.intFactor, x.ptxtSpace) == (y.lnNoise, y.primeSet, y.intFactor, y.ptxtSpace)
        assert sorted(x.parts) == sorted(y.parts)
        for h in x.parts:
            assert np.array_equal(x.parts[h].rows, y.parts[h].rows)
    # the default follows the class switch; a backend without the call cannot be forced
    cc, sk, ea = _setup(m, p, 400, [amt], seed=2)
    ct = ea.encrypt(sk, a)
    with pytest.raises(ckks.LogicError, match="cannot be fused"):
        ea.rotate(ct, amt, fused=True)
    ea.rotate(ea.encrypt(sk, a), amt)                    # fused=None: term by term here


def test_mask_cache_is_bounded_and_reused():
    m, p = 45, 181
    cc, sk, ea = _setup(m, p, 300)
    idx = frozenset(cc.ctxtPrimes)
    first = ea._encodedMask(ea.maskSlots(0, 1), idx)
    assert ea._encodedMask(ea.maskSlots(0, 1), idx) is first
    assert ea._encodedMask(ea.maskSlots(0, 1), frozenset(list(idx)[:1])) is not first
    rng = np.random.default_rng(0)
    for _ in range(ea.MASK_CACHE + 5):
        ea._encodedMask(rng.integers(0, 2, size=ea.size()), idx)
    assert len(ea._masks) == ea.MASK_CACHE
    assert ea._encodedMask(ea.maskSlots(0, 1), idx) is not first      # it was the oldest: gone


def test_error_cases():
    from helib_amd import capi
    m, p = 45, 181
    cc, sk, ea = _setup(m, p, 300)
    a = np.arange(ea.size())
    ct = ea.encrypt(sk, a)
    for bad in (-1, 2):
        with pytest.raises(capi.InvalidArgument):
            ea.shift1D(ct, bad, 1)
        with pytest.raises(capi.InvalidArgument):
            ea.maskSlots(bad, 0)
    with pytest.raises(capi.InvalidArgument):
        ea.maskSlots(0, ea.sizeOfDimension(0) + 1)
    with pytest.raises(LookupError):                  # no key-switching matrices were generated
        ea.rotate(ct, 1)
    with pytest.raises(capi.InvalidArgument, match="go together"):
        capi.maskSplit(None, None, None, object(), None)
    assert np.array_equal(ea.decrypt(ct, sk), a)      # the refusals left the ciphertext alone


# ---- declarations ----
def test_mask_split_is_declared_bound_and_exported():
    from helib_amd import capi
    hdr = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    declared = set(re.findall(r"\b(hx_[a-zA-Z0-9_]+)\s*\(", hdr))
    assert "hx_mask_split" in capi.SYMBOLS and "hx_mask_split" in declared
    assert "src/EncryptedArray.cpp:270-274" in hdr and "HX_NO_MASK_SPLIT" in hdr
    lib = capi.lib()                      # the cross-compiled library
    assert len(lib.hx_mask_split.argtypes) == 5
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi._SO], text=True)
    assert re.search(r"\bT hx_mask_split$", out, re.M)
    sw = open(os.path.join(ROOT, "helib_amd", "csrc", "switches.h")).read()
    assert 'on("HX_NO_MASK_SPLIT")' in sw
    from helib_amd import bgv
    for f in ("maskSlots", "shift1D", "rotate", "shift", "totalSums", "runningSums"):
        assert hasattr(bgv.EncryptedArray, f)
    assert hasattr(capi, "maskSplit")
