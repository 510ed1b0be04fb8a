"""Restatement of EncryptedArray(context, G) with G = F_0 (slots in GF(p^d) = Z_p[X] / G, r = 1) from the definitions,
on top of tests/bgv_crt_ref.py's polynomial arithmetic over Z_p.  No sliding window, no fold, no per-slot matrices: it
shares no method with helib_amd/csrc/bgv_gf.h.

  encode   the literal CRT: H = sum_i c_i * E_i mod Phi_m with c_i = alpha_i(X^(t_i)) mod F_i (Horner in Z_p[X] / F_i),
           E_i the idempotent of factor i, t_i = ith_rep(i); balanced into (-p/2, p/2]
  decode   slot i = (H mod F_i)(X^(1/t_i)) mod G (Horner in Z_p[X] / G)
  mul / frobenius   in Z_p[X] / G: the product, and alpha -> alpha^(p^j) by square and multiply
Slots are [B, nslots, d], coefficients lowest first; a [B, nslots] array means constants."""
import functools

import numpy as np

from tests import bgv_crt_ref as R


def padd(a, b, p):
    n = max(len(a), len(b))
    return (np.pad(np.asarray(a, dtype=np.int64), (0, n - len(a))) + np.pad(np.asarray(b, dtype=np.int64), (0, n - len(b)))) % p


def compose(a, x, f, p):
    """a(x) mod f, a given by its coefficients (Horner)"""
    r = np.zeros(0, dtype=np.int64)
    for c in reversed([int(v) % p for v in a]):
        r = R.prem(padd(R.pmul(r, x, p), [c], p), f, p)
    return r


class GfTables:
    def __init__(self, m, p):
        self.base = b = R.tables(m, p)
        self.m, self.p, self.d, self.nslots, self.phim, self.z = m, p, b.d, b.nslots, b.phim, b.z
        self.F, self.G = b.F, b.F[0]
        X = np.array([0, 1], dtype=np.int64)
        self.t = [b.z.ith_rep(i) for i in range(self.nslots)]
        self.xt = [R.ppowmod(X, t, f, p) for t, f in zip(self.t, self.F)]        # X^(t_i) mod F_i
        self.y = [R.ppowmod(X, pow(t, -1, m), self.G, p) for t in self.t]       # X^(1/t_i) mod G

    def slots(self, a):
        """[B, <= nslots] constants or [B, <= nslots, <= d] -> object array [B, nslots, d]"""
        a = np.asarray(a, dtype=object)
        if a.ndim == 2:
            a = a[:, :, None]
        out = np.zeros((a.shape[0], self.nslots, self.d), dtype=object)
        out[:, :a.shape[1], :a.shape[2]] = a
        return out

    def encode(self, a, mul=1):
        """-> balanced(mul * H mod p) [B, phim]"""
        p, b = self.p, self.base
        out = []
        for row in self.slots(a):
            h = np.zeros(0, dtype=np.int64)
            for i, alpha in enumerate(row):
                c = compose(alpha, self.xt[i], self.F[i], p)
                if len(c):
                    h = padd(h, R.pmul(c, np.array(b.E[i], dtype=np.int64), p), p)
            h = R.prem(h, b.phi, p)
            h = np.pad(h, (0, self.phim - len(h)))
            out.append([int(x) * (mul % p) % p for x in h])
        return b.balanced(out)

    def decode(self, coeffs):
        """polynomials [B, phim] (any integers) -> slots [B, nslots, d] in [0, p)"""
        p = self.p
        out = []
        for row in np.atleast_2d(np.asarray(coeffs, dtype=object)):
            h = np.array([int(x) % p for x in row], dtype=np.int64)
            vals = []
            for i, f in enumerate(self.F):
                v = compose(R.prem(h, f, p), self.y[i], self.G, p)
                vals.append(np.pad(v, (0, self.d - len(v))))
            out.append(vals)
        return np.array(out, dtype=np.int64)

    def _each(self, a, fn):
        a = self.slots(a)
        out = np.zeros(a.shape, dtype=np.int64)
        for b in range(a.shape[0]):
            for i in range(a.shape[1]):
                v = fn(b, i, np.array([int(x) % self.p for x in a[b, i]], dtype=np.int64))
                out[b, i, :len(v)] = v
        return out

    def mul(self, a, b):
        b = self.slots(b)
        return self._each(a, lambda bb, i, x: R.prem(R.pmul(x, np.array([int(v) % self.p for v in b[bb, i]], dtype=np.int64),
                                                            self.p), self.G, self.p))

    def frobenius(self, a, j):
        return self._each(a, lambda bb, i, x: R.ppowmod(x, self.p ** j, self.G, self.p) if np.any(x) else x[:0])


@functools.lru_cache(maxsize=None)
def tables(m, p):
    return GfTables(m, p)
