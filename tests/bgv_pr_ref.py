"""Restatement of the default EncryptedArray's slot maps (G = X) modulo p^r, r >= 1, in python integers: the r > 1 branch
of PAlgebraModDerived's constructor (src/PAlgebra.cpp:757-763 over PAlgebraLift, :840-881) by Hensel's lemma on
polynomials.  It starts from tests/bgv_crt_ref.py's factors and idempotents modulo p and shares no method with
helib_amd/csrc/bgv_crt.h: no Galois ring, no roots of unity, no traces.

  factor i      F_i mod p lifted one power of p at a time: with G = Phi_m / F, delta = (Phi_m - F G) / p^k mod p and
                t = G^-1 mod (F, p), the next F is F + p^k (t delta mod F); the next G is the exact quotient Phi_m / F
  idempotent i  e <- 3 e^2 - 2 e^3 mod (Phi_m, p^(2^k)): if e^2 = e mod p^j then the new e is idempotent mod p^(2j) and
                reduces to the old one, so from E_i mod p it reaches the E_i mod p^r of the lifted factors
  R[i][k]       the constant term of X^k mod F_i, by multiplying by X and reducing k times
  encode        sum_i a_i E_i mod p^r, times mul, balanced into (-p^r/2, p^r/2]: at an even modulus the reference draws
                the sign of a coefficient equal to p^r/2 at random (src/zzX.cpp:122-137); the project keeps +p^r/2
  decode        slot i = sum_k h_k R[i][k] mod p^r, reduced mod p^k for a ciphertext whose space is p^k
Coefficients are lowest first.

Beside the tables, the two references the host and the device tests share: scaled_sub (hx_scaled_sub's words) and replay
(the digit extraction loop on plain integers)."""
import functools

import numpy as np

from helib_amd import hostnt

from tests import bgv_crt_ref as R1


def _mul(a, b, P):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] += x * y
    return [v % P for v in out]


def _divmod(a, f, P):
    """(quotient, remainder) of a by the monic f modulo P"""
    a = [v % P for v in a]
    df = len(f) - 1
    q = [0] * max(len(a) - df, 1)
    for i in range(len(a) - 1, df - 1, -1):
        c = a[i]
        if c:
            q[i - df] = c
            for j in range(df + 1):
                a[i - df + j] = (a[i - df + j] - c * f[j]) % P
    return q, a[:df]


def mulmod(a, b, f, P):
    return _divmod(_mul(a, b, P), f, P)[1]


class Tables:
    """m, p, r, P = p^r, d, nslots, phim, z; phi (Phi_m over the integers), F[i] (d + 1 ints), E[i], Rt[i] (phim ints)"""

    def __init__(self, m, p, r):
        base = R1.tables(m, p)
        self.base, self.m, self.p, self.r, self.P = base, m, p, r, p ** r
        self.z, self.d, self.nslots, self.phim = base.z, base.d, base.nslots, base.phim
        self.phi = [int(c) for c in hostnt.phimx(m)]
        phi, P, n = self.phi, self.P, self.phim
        self.F = []
        for f1 in base.F:
            F = [int(c) for c in f1]
            G1 = R1.pdiv(np.array(phi, dtype=np.int64) % p, np.array(F, dtype=np.int64), p)
            t = [int(c) for c in R1.pinv(R1.prem(G1, np.array(F, dtype=np.int64), p), np.array(F, dtype=np.int64), p)]
            pk = p
            for _ in range(1, r):
                G, rem = _divmod(phi, F, pk)
                assert not any(rem)
                nxt = pk * p
                prod = _mul(F, G, nxt)
                delta = [((phi[i] - prod[i]) % nxt) // pk for i in range(n + 1)]
                u = _divmod(_mul(t, delta, p), [c % p for c in F], p)[1]
                F = [(c + pk * (u[i] if i < len(u) else 0)) % nxt for i, c in enumerate(F)]
                pk = nxt
            assert not any(_divmod(phi, F, P)[1]) and F[-1] == 1
            self.F.append(F)
        self.E = []
        for e1 in base.E:
            e, j = [int(c) for c in e1], 1
            while j < r:
                j = min(2 * j, r)
                pj = p ** j
                e2 = mulmod(e, e, phi, pj)
                e3 = mulmod(e2, e, phi, pj)
                e = [(3 * x - 2 * y) % pj for x, y in zip(e2, e3)]
            self.E.append(e)
        self.Rt = []
        for F in self.F:
            d, cur, row = self.d, [1] + [0] * (self.d - 1), []
            for _ in range(n):
                row.append(cur[0])
                top = cur[d - 1]
                cur = [(-top * F[0]) % P] + [(cur[i - 1] - top * F[i]) % P for i in range(1, d)]
            self.Rt.append(row)
        self._E = np.array(self.E, dtype=object)
        self._R = np.array(self.Rt, dtype=object)

    def balanced(self, x, P=None):
        P = self.P if P is None else P
        return np.array([[(int(v) % P) - P if (int(v) % P) > P // 2 else int(v) % P for v in row]
                         for row in np.atleast_2d(np.asarray(x, dtype=object))], dtype=np.int64)

    def encode(self, a, mul=1):
        """slots [B, <= nslots] (any integers) -> balanced(mul * H mod p^r) [B, phim]"""
        P = self.P
        a = np.atleast_2d(np.asarray(a, dtype=object))
        a = np.array([[int(v) % P for v in row] + [0] * (self.nslots - len(row)) for row in a], dtype=object)
        return self.balanced(a.dot(self._E) % P * (mul % P) % P)

    def decode(self, coeffs, k=None):
        """polynomials [B, phim] (any integers) -> slots [B, nslots] in [0, p^k) (k = None: r)"""
        Pk = self.P if k is None else self.p ** k
        h = np.atleast_2d(np.asarray(coeffs, dtype=object))
        h = np.array([[int(v) % self.P for v in row] for row in h], dtype=object)
        return np.array(h.dot(self._R.T) % Pk, dtype=np.int64)

    def worst_sums(self):
        """(encode, decode): the largest sums a kernel that never reduced would have to hold when every input word is
        p^r - 1 -- max over the coefficients k of sum_i (p^r - 1) E[i][k], max over the slots i of
        sum_k (p^r - 1) R[i][k].  Above 2^64 a dropped or late reduction of the 64-bit accumulator wraps."""
        top = self.P - 1
        return top * int(max(self._E.sum(axis=0))), top * int(max(self._R.sum(axis=1)))

    def kernel_replay(self, kind, x, drop=False, late=0):
        """What a 64-bit accumulator gives for x = slots ("encode": [B, nslots] -> [B, phim]) or coefficients ("decode":
        [B, phim] -> [B, nslots]) when it counts as bgv_crt_encode_kernel / bgv_crt_decode_kernel do: terms four at a
        time in steps of 16 slots / 32 coefficients (the padding of the last step counts down as well), left = limit at
        the start, left -= 4 after every four terms and, once left < 4, a reduction mod p^r and left = limit + late.
        drop: the reduction inside the loop never happens.  The sums wrap modulo 2^64; the result is reduced once at the
        end, so with drop = False and late = 0 it is the residue encode / decode start from.  A modulus that divides
        2^64 keeps its residue through a wrap: there no miscount can show."""
        P, M = self.P, (1 << 64) - 1
        limit = min((1 << 64) // (P * P), 0xffffffff)
        T, step = (self._E, 16) if kind == "encode" else (self._R.T, 32)      # [terms, outputs]
        x = np.array([[int(v) % P for v in row] for row in np.atleast_2d(np.asarray(x, dtype=object))], dtype=object)
        acc = np.zeros((x.shape[0], T.shape[1]), dtype=object)
        left = limit
        for g in range(0, (T.shape[0] + step - 1) // step * step, 4):
            if g < T.shape[0]:
                acc = (acc + x[:, g:g + 4].dot(T[g:g + 4])) & M
            left -= 4
            if left < 4:
                if not drop:
                    acc = acc % P
                left = limit + late
        return np.array(acc % P, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def tables(m, p, r):
    return Tables(m, p, r)


def scaled_sub(c_rows, t_rows, u, v, qs):
    """hx_scaled_sub in python integers: row i of the result is (c_rows[i] * u[i] - t_rows[i] * v[i]) mod qs[i], word for
    word, as an object array of the shape of c_rows (row i may have any shape)"""
    c = np.asarray(c_rows).astype(object)
    t = np.asarray(t_rows).astype(object)
    assert c.shape == t.shape and len(c) == len(u) == len(v) == len(qs)
    out = np.empty_like(c)
    for i, q in enumerate(qs):
        out[i] = (c[i] * int(u[i]) - t[i] * int(v[i])) % int(q)
    return out


def replay(a, p, r):
    """the loop of src/extractDigits.cpp:90-124 on plain integers: [(values, modulus)]"""
    P = p ** r
    dig = []
    for i in range(r):
        tmp, M = np.array([int(x) % P for x in a], dtype=object), P
        for j in range(i):
            v, Mj = dig[j]
            v = v ** p % Mj
            dig[j] = (v, Mj)
            assert Mj == M
            tmp = tmp - v
            assert not any(int(x) % p for x in tmp)
            M //= p
            tmp = np.array([int(x) // p % M for x in tmp], dtype=object)
        dig.append((tmp, M))
    return dig
