"""What the helib_amd.bgv_hypercube tests share: the oracle-backend setup with a CPU encoder (as
tests/test_bgv_crt_host.py's, with the new class and an optional ops class), and the numpy truth on slot vectors."""
import functools

import numpy as np

from tests import bgv_crt_ref as R

# (m, p): signed orders -- the smallest ring of each shape (hostnt.ZmStar)
RINGS = {(85, 2): [-8], (119, 2): [2, -2], (527, 2): [6, -2], (255, 2): [-8, 2], (803, 3): [-6, -2],
         (1785, 2): [-8, 2, 2]}


@functools.lru_cache(maxsize=None)
def tables(m, p):
    return R.tables(m, p)


def setup(m, p, bits, seed=3, ops=None, keys=True):
    """-> (cc, sk, ea): helib_amd.bgv_hypercube.EncryptedArray over the oracle backend, one vector per ciphertext"""
    from oracle import oracle as O
    from oracle.backend import OracleBackend
    from helib_amd import bgv_hypercube, ctxt as hc, keys as hk
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
    ref = tables(m, p)

    class Enc:
        def dims(self):
            return ref.z.gens, ref.z.signedOrds()

        def encode(self, v, mul, idx, coeffs=False):
            cf = ref.encode(v, mul)
            d = None
            if idx:
                assert cf.shape[0] == 1, "the CPU backend takes one vector at a time"
                d = be.fromCoeffs(idx, [int(x) for x in cf[0]])
                d.batch = 1
            return (d, cf) if coeffs else d

        def embed(self, coeffs):
            return ref.decode(coeffs)

        def decode(self, acc, factor_inv):
            return ref.decode([[int(x) % p * factor_inv % p for x in be.toPoly(acc)]])

        def norm(self, coeffs):
            return np.array([be.embeddingLargestCoeff(row) for row in np.atleast_2d(coeffs)])
    sk = hk.SecKey(cc, be, seed=seed)
    sk.GenSecKey()
    ea = bgv_hypercube.EncryptedArray(cc, None, encoder=Enc())
    sk.zMStar = ea.zMStar
    if keys:
        hk.add1DMatrices(sk)
    return cc, sk, ea


def shift(a, k):
    """slot j -> slot j + k, zeros come in"""
    a = np.atleast_2d(a)
    n, out = a.shape[1], np.zeros_like(np.atleast_2d(a))
    if 0 <= k < n:
        out[:, k:] = a[:, :n - k]
    elif -n < k < 0:
        out[:, :n + k] = a[:, -k:]
    return out


def total_sums(a, p):
    a = np.atleast_2d(a)
    return np.repeat(a.sum(axis=1, keepdims=True) % p, a.shape[1], axis=1)


def running_sums(a, p):
    return np.cumsum(np.atleast_2d(a), axis=1) % p


def same(x, y, rows):
    """equal bookkeeping and equal words; rows(part) -> the words as an array"""
    assert (x.lnNoise, x.primeSet, x.intFactor, x.ptxtSpace) == (y.lnNoise, y.primeSet, y.intFactor, y.ptxtSpace)
    assert sorted(x.parts, key=str) == sorted(y.parts, key=str)
    for h in x.parts:
        assert np.array_equal(rows(x.parts[h]), rows(y.parts[h])), h
