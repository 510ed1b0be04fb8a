"""Restatement of the default EncryptedArray's slot maps (G = X, r = 1) for any d = ord_m(p): polynomial arithmetic
over Z_p on coefficient arrays, written from the reference's definitions.  No extension field, no roots of unity, no
traces: it shares no method with helib_amd/csrc/bgv_crt.h.

  factors of Phi_m mod p   equal-degree splitting by random gcds (Cantor-Zassenhaus; the trace map for p = 2), the
                           factors ordered by poly_comp (src/PAlgebra.cpp:67-81): F_0 the smallest
  factor i                 gcd(F_0(X^t_i), Phi_m), t_i = ith_rep(i): the reference's own sanity formula (:734-743)
  encode                   the literal CRT: sum_i a_i * crtCoeffs_i * (Phi_m / F_i), crtCoeffs_i = (Phi_m / F_i mod
                           F_i)^-1 mod F_i (:750-756, 1007-1045); balanced into (-p/2, p/2] (for p = 2 the reference
                           draws the sign of a 1 at random, src/zzX.cpp:139-154; the project always takes +1)
  decode                   slot i = the constant term of H mod F_i
Coefficients are lowest first; p < 2^31, so a product of two fits an int64."""
import functools
import math
import random

import numpy as np

from helib_amd import hostnt


def _trim(a):
    n = len(a)
    while n and a[n - 1] == 0:
        n -= 1
    return a[:n]


def prem(a, g, p):
    """a mod the monic g"""
    a = np.array(a, dtype=np.int64) % p
    dg = len(g) - 1
    for i in range(len(a) - 1, dg - 1, -1):
        c = int(a[i])
        if c:
            a[i - dg:i + 1] = (a[i - dg:i + 1] - c * g) % p
    return _trim(a[:dg])


def pdiv(a, g, p):
    """the quotient of a by the monic g"""
    a = np.array(a, dtype=np.int64) % p
    dg = len(g) - 1
    q = np.zeros(max(len(a) - dg, 1), dtype=np.int64)
    for i in range(len(a) - 1, dg - 1, -1):
        c = int(a[i])
        q[i - dg] = c
        if c:
            a[i - dg:i + 1] = (a[i - dg:i + 1] - c * g) % p
    return q


def pmul(a, b, p):
    out = np.zeros(len(a) + len(b) - 1 if len(a) and len(b) else 0, dtype=np.int64)
    for i, c in enumerate(a):
        c = int(c)
        if c:
            out[i:i + len(b)] = (out[i:i + len(b)] + c * b) % p
    return out


def monic(a, p):
    a = _trim(np.array(a, dtype=np.int64) % p)
    return a * pow(int(a[-1]), -1, p) % p if len(a) else a


def pgcd(a, b, p):
    a, b = _trim(np.array(a, dtype=np.int64) % p), _trim(np.array(b, dtype=np.int64) % p)
    while len(b):
        b = monic(b, p)
        a, b = b, prem(a, b, p)
    return monic(a, p)


def pinv(a, f, p):
    """a^-1 mod the monic f (extended Euclid)"""
    r0, r1 = np.array(f, dtype=np.int64), _trim(np.array(a, dtype=np.int64) % p)
    s0, s1 = np.zeros(0, dtype=np.int64), np.array([1], dtype=np.int64)
    while len(r1) > 1:
        lead = pow(int(r1[-1]), -1, p)
        r1, s1 = r1 * lead % p, s1 * lead % p
        q = pdiv(r0, r1, p)
        r0, r1 = r1, prem(r0, r1, p)
        qs = pmul(q, s1, p)
        n = max(len(s0), len(qs))
        s2 = (np.pad(s0, (0, n - len(s0))) - np.pad(qs, (0, n - len(qs)))) % p
        s0, s1 = s1, _trim(s2)
    assert len(r1) == 1, "not invertible"
    return prem(s1 * pow(int(r1[0]), -1, p) % p, f, p)


def ppowmod(a, e, f, p):
    r, a = np.array([1], dtype=np.int64), prem(a, f, p)
    while e:
        if e & 1:
            r = prem(pmul(r, a, p), f, p)
        a = prem(pmul(a, a, p), f, p)
        e >>= 1
    return r


def split(f, d, p, rng):
    """the monic irreducible factors, all of degree d, of the monic squarefree f"""
    if len(f) - 1 == d:
        return [f]
    while True:
        a = np.array([rng.randrange(p) for _ in range(len(f) - 1)], dtype=np.int64)
        if p == 2:
            t, x = np.zeros(0, dtype=np.int64), prem(a, f, p)
            for _ in range(d):
                n = max(len(t), len(x))
                t = (np.pad(t, (0, n - len(t))) + np.pad(x, (0, n - len(x)))) % p
                x = prem(pmul(x, x, p), f, p)
            t = _trim(t)
        else:
            t = ppowmod(a, (p ** d - 1) // 2, f, p)
            t = np.pad(t, (0, max(0, 1 - len(t))))
            t[0] = (t[0] - 1) % p
            t = _trim(t)
        if not len(t):
            continue
        g = pgcd(f, t, p)
        if 1 < len(g) < len(f):
            return split(g, d, p, rng) + split(pdiv(f, g, p), d, p, rng)


def poly_key(f):
    """poly_comp for polynomials of one degree: the first differing coefficient from the constant one up decides"""
    return tuple(int(x) for x in f)


class Tables:
    """m, p, d, nslots, phim, z (hostnt.ZmStar), phi (Phi_m mod p), F[i] (monic, d + 1 words), E[i] (the idempotents,
    phim python ints each)"""

    def __init__(self, m, p):
        self.m, self.p = m, p
        self.z = hostnt.ZmStar(m, p)
        self.d, self.nslots = self.z.ordP, self.z.getNSlots()
        self.phi = np.array(hostnt.phimx(m), dtype=np.int64) % p
        self.phim = len(self.phi) - 1
        assert self.nslots * self.d == self.phim
        d, phi = self.d, self.phi
        F0 = min(split(phi, d, p, random.Random(m * 1000003 + p)), key=poly_key)
        # X^e mod Phi_m for every e < m, then F_0(X^t) as a sum of those
        xp = [np.array([1], dtype=np.int64)]
        for _ in range(m - 1):
            xp.append(prem(np.concatenate([[0], xp[-1]]), phi, p))
        self.F = []
        for i in range(self.nslots):
            t = self.z.ith_rep(i)
            comp = np.zeros(self.phim, dtype=np.int64)
            for j, c in enumerate(F0):
                x = xp[t * j % m]
                comp[:len(x)] = (comp[:len(x)] + int(c) * x) % p
            self.F.append(pgcd(phi, comp, p))
            assert len(self.F[-1]) == d + 1
        assert poly_key(self.F[0]) == poly_key(F0)
        self.E = []
        for f in self.F:
            rest = pdiv(phi, f, p)
            e = pmul(pinv(prem(rest, f, p), f, p), rest, p)
            self.E.append([int(x) for x in np.pad(e, (0, self.phim - len(e)))])

    def balanced(self, x):
        p = self.p
        return np.array([[(int(v) % p) - p if (int(v) % p) > p // 2 else int(v) % p for v in row] for row in np.atleast_2d(x)],
                        dtype=np.int64)

    def encode(self, a, mul=1):
        """slots [B, <= nslots] (any integers) -> balanced(mul * H mod p) [B, phim], in python integers"""
        p = self.p
        out = []
        for row in np.atleast_2d(np.asarray(a, dtype=object)):
            h = [0] * self.phim
            for i, v in enumerate(row):
                v = int(v) % p
                if v:
                    h = [x + v * e for x, e in zip(h, self.E[i])]
            out.append([x % p * (mul % p) % p for x in h])
        return self.balanced(out)

    def decode(self, coeffs):
        """polynomials [B, phim] (any integers) -> slots [B, nslots] in [0, p)"""
        p = self.p
        out = []
        for row in np.atleast_2d(np.asarray(coeffs, dtype=object)):
            h = np.array([int(x) % p for x in row], dtype=np.int64)
            rems = [prem(h, f, p) for f in self.F]
            out.append([int(r[0]) if len(r) else 0 for r in rems])
        return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def tables(m, p):
    return Tables(m, p)


def phi_of(m):
    return sum(1 for j in range(m) if math.gcd(j, m) == 1)
