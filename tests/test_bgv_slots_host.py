"""BGV slots on the host side (no GPU): the restatement of the reference's definitions (tests/bgv_slots_ref.py) against
itself and brute force, helib_amd.bgv.EncryptedArray's control flow and PubKey.EncryptBatch's sample order over the
oracle backend with an injected CPU encoder, and the new entry points' declarations."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_slots_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hx_bgv_slots_create", "hx_bgv_slots_destroy", "hx_bgv_slots_info", "hx_bgv_encode", "hx_bgv_decode", "hx_bgv_embed"]


@pytest.mark.parametrize("m,p", [(16, 17), (16, 97), (64, 193), (256, 257), (105, 211), (45, 181)])
def test_literal_crt_has_the_defining_property(m, p):
    pts = R.points(m, p)
    n = len(pts)
    assert n == sum(1 for j in range(m) if math.gcd(j, m) == 1) and len(set(pts)) == n
    rng = np.random.default_rng(m)
    a = rng.integers(0, p, size=n)
    H = R.encode_crt(a, m, p, pts)
    assert H.shape == (n,) and np.all(np.abs(H) <= p // 2)
    assert np.array_equal(R.decode(H[None], m, p, pts)[0], a)
    # linear, and the idempotent of slot i is 1 there and 0 elsewhere
    unit = np.zeros(n, dtype=np.int64)
    unit[3] = 1
    assert np.array_equal(R.decode(R.encode_crt(unit, m, p, pts)[None], m, p, pts)[0], unit)
    short = R.encode_crt(a[:5], m, p, pts)
    assert np.array_equal(R.decode(short[None], m, p, pts)[0], np.concatenate([a[:5], np.zeros(n - 5, dtype=np.int64)]))


@pytest.mark.parametrize("m,p", [(16, 17), (16, 97), (64, 193), (105, 211), (45, 181), (1024, 12289)])
def test_rho_and_the_factors_against_brute_force(m, p):
    roots = R.primitive_roots(m, p)
    assert len(roots) == len(R.points(m, p))
    # poly_comp orders X - a by the constant coefficient p - a as a residue: the smallest factor has the largest root
    rho = R.rho_of(m, p)
    assert rho == max(roots) and (p - rho) % p == min((p - a) % p for a in roots)
    # factor i has the root r with r^t_i = rho (X^(1/t_i) mod F_0), and the roots are a permutation of all of them
    z = R.zmstar(m, p)
    pts = R.points(m, p, z)
    assert sorted(pts) == sorted(roots)
    assert all(pow(r, z.ith_rep(i), p) == rho for i, r in enumerate(pts))
    assert pts[0] == rho


def test_slot_permutation_against_the_transform_order():
    """slot i sits at the row position of k / t_i mod m when the transform evaluates at zeta^j, j in Z_m^* ascending,
    and rho = zeta^k -- for a zeta that is NOT rho"""
    m, p = 64, 193
    z = R.zmstar(m, p)
    rho = R.rho_of(m, p)
    zeta = next(a for a in R.primitive_roots(m, p) if a != rho)
    units = [j for j in range(m) if math.gcd(j, m) == 1]
    k = next(j for j in units if pow(zeta, j, p) == rho)
    pts = R.points(m, p, z)
    for i in range(z.getNSlots()):
        pos = units.index(k * pow(z.ith_rep(i), -1, m) % m)
        assert pow(zeta, units[pos], p) == pts[i]


# ---- EncryptedArray over the oracle backend with a CPU encoder ----
class _Batch:
    """B batch-1 oracle polys behind the few DoubleCRT methods EncryptBatch and Ctxt use"""

    def __init__(self, polys):
        self.polys, self.batch = polys, len(polys)

    def getIndexSet(self):
        return self.polys[0].getIndexSet()

    def copy(self):
        return _Batch([x.copy() for x in self.polys])

    def _each(self, other, op):
        others = other.polys if isinstance(other, _Batch) else [other] * self.batch
        for x, y in zip(self.polys, others if len(others) == self.batch else others * self.batch):
            op(x, y)
        return self

    def __iadd__(self, o):
        return self._each(o, lambda x, y: x.__iadd__(y))

    def __isub__(self, o):
        return self._each(o, lambda x, y: x.__isub__(y))

    def __imul__(self, o):
        return self._each(o, lambda x, y: x.__imul__(y))

    def mulConstant(self, c):
        for x in self.polys:
            x.mulConstant(c)
        return self


class _CpuEncoder:
    """the encoder's members over tests/bgv_slots_ref.py and the oracle backend"""

    def __init__(self, be, m, p):
        self.be, self.m, self.p = be, m, p
        self.pts = R.points(m, p)
        self.calls = []

    def encode(self, v, mul, idx, coeffs=False):
        self.calls.append(("encode", int(mul), list(idx)))
        cf = np.stack([R.balanced(R.encode_crt(row, self.m, self.p, self.pts) * (mul % self.p), self.p) for row in v])
        d = _Batch([self.be.fromCoeffs(idx, row) for row in cf]) if idx else None
        return (d, cf) if coeffs else d

    def embed(self, coeffs):
        return R.decode(coeffs, self.m, self.p, self.pts)

    def decode(self, acc, factor_inv):
        self.calls.append(("decode", int(factor_inv)))
        polys = acc.polys if isinstance(acc, _Batch) else [acc]
        cf = np.array([[int(x) % self.p * factor_inv % self.p for x in self.be.toPoly(q)] for q in polys])
        return self.embed(cf)

    def norm(self, coeffs):
        return np.array([self.be.embeddingLargestCoeff(row) for row in np.atleast_2d(coeffs)])


def _setup(m=64, p=193, seed=3):
    from oracle import oracle as O
    from oracle.backend import OracleBackend
    from helib_amd import bgv, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, 1, bits=120, c=2)
    o = O.Ctx(m)
    for q in cc.primes:
        o.add_prime(q)

    class Backend(OracleBackend):
        def fromCoeffsBatch(self, idx, polys):
            return _Batch([self.fromCoeffs(idx, c) for c in polys])
    be = Backend(o, cc)
    sk = hk.SecKey(cc, be, seed=seed)
    sk.GenSecKey()
    enc = _CpuEncoder(be, m, p)
    return cc, sk, bgv.EncryptedArray(cc, None, encoder=enc), enc


def test_encrypted_array_geometry_and_refusals():
    from helib_amd import bgv, capi, ckks, ctxt as hc
    cc, sk, ea, enc = _setup()
    assert (ea.size(), ea.getP(), ea.getDegree()) == (32, 193, 1)
    z = hostnt.ZmStar(64, 193)
    assert ea.dimension() == z.numOfGens() == 2
    assert [ea.sizeOfDimension(i) for i in range(2)] == z.ords and all(ea.nativeDimension(i) for i in range(2))
    assert [ea.coordinate(0, k) * z.ords[1] + ea.coordinate(1, k) for k in range(32)] == list(range(32))
    with pytest.raises(ckks.LogicError):
        bgv.EncryptedArray(hc.ChainContext(64, -1, 20, bits=100, c=2, ckks=True), None, encoder=enc)
    for ctx, what in [(hc.ChainContext(64, 17, 1, bits=100, c=2), r"d = ord_m\(p\) = 4"),
                      (hc.ChainContext(64, 193, 2, bits=100, c=2), "r > 1")]:
        with pytest.raises(capi.HxError, match=what) as e:
            bgv.EncryptedArray(ctx, None, encoder=enc)
        assert e.value.code == capi.HX_ERR_UNSUPPORTED
    with pytest.raises(capi.InvalidArgument, match="more values than slots"):
        ea.encode(np.zeros(33, dtype=np.int64))


def test_encrypt_batch_draws_in_the_order_of_consecutive_encrypts():
    cc, sk, ea, enc = _setup(seed=9)
    _, sk2, ea2, _ = _setup(seed=9)
    p, B = 193, 3
    v = np.random.default_rng(2).integers(-p, 2 * p, size=(B, ea.size()))
    ct = ea.encrypt_batch(sk, v)
    Q = cc.productOfPrimes(list(cc.ctxtPrimes)) % p
    assert enc.calls[-1] == ("encode", Q, list(cc.ctxtPrimes))
    polys = ea2.encodeCoeffs(v)
    for b in range(B):
        one = sk2.Encrypt([int(x) for x in polys[b]])
        for h in ("1", "s"):
            assert np.array_equal(one.parts[h].rows, ct.parts[h].polys[b].rows), (b, h)
        assert one.lnNoise == ct.lnNoise and ct.ptxtSpace == p
    # and it decrypts: the factor handed to the decoder is (Q * intFactor)^-1 mod p
    got = ea.decrypt_batch(ct, sk)
    assert enc.calls[-1] == ("decode", pow(Q, -1, p))
    assert np.array_equal(got, v % p)
    ct.ptxtSpace = 17
    from helib_amd import ckks
    with pytest.raises(ckks.LogicError, match="plaintext space is not p"):
        ea.decrypt_batch(ct, sk)


def test_constants_and_rotation_control_flow():
    cc, sk, ea, enc = _setup(seed=4)
    p, n = 193, ea.size()
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, p, size=(2, 1, n))
    ct = ea.encrypt(sk, a[0])
    e = ea.encodePtxt(b)
    assert np.array_equal(ea.decode(e.poly), b) and e.ptxtSpace == p
    ln0 = ct.lnNoise
    ea.multByConstant(ct, e)
    assert math.isclose(ct.lnNoise, ln0 + math.log(enc.norm(e.poly)[0]))
    assert np.array_equal(ea.decrypt(ct, sk), (a * b % p)[0])
    ea.addConstant(ct, e)
    Q = cc.productOfPrimes(sorted(ct.primeSet)) % p * ct.intFactor % p
    assert ("encode", Q, sorted(ct.primeSet)) in enc.calls      # the scaling happens in the plaintext space
    assert np.array_equal(ea.decrypt(ct, sk), ((a * b + b) % p)[0])
    ea.addConstant(ct, e, neg=True)
    assert np.array_equal(ea.decrypt(ct, sk), (a * b % p)[0])
    # rotate1D: one automorphism by g_i^amt, amt taken modulo the order
    seen = []

    class Spy:
        parts = True

        def smartAutomorph(self, k):
            seen.append(k)
            return self
    z = ea.zMStar
    ea.rotate1D(Spy(), 0, 3)
    ea.rotate1D(Spy(), 0, -1)
    ea.rotate1D(Spy(), 1, z.ords[1] + 1)
    ea.rotate1D(Spy(), 1, 0)
    assert seen == [pow(z.gens[0], 3, 64), pow(z.gens[0], z.ords[0] - 1, 64), z.gens[1] % 64]
    from helib_amd import capi
    with pytest.raises(capi.InvalidArgument):
        ea.rotate1D(Spy(), 2, 1)


# ---- declarations ----
def test_new_symbols_are_declared_bound_and_exported():
    from helib_amd import capi
    hdr = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    declared = set(re.findall(r"\b(hx_[a-zA-Z0-9_]+)\s*\(", hdr))
    for s in NEW:
        assert s in capi.SYMBOLS and s in declared, s
    lib = capi.lib()                      # the cross-compiled library
    for s in NEW:
        assert hasattr(lib, s) and getattr(lib, s).argtypes is not None, s
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi._SO], text=True)
    for s in NEW:
        assert re.search(r"\bT %s$" % s, out, re.M), s
    for f in ("bgvEncode", "bgvDecode", "bgvEmbed", "BgvSlots"):
        assert hasattr(capi, f)
    import helib_amd.bgv as bgv
    assert hasattr(bgv, "EncryptedArray") and hasattr(capi.lib(), "hx_poly_rem")
