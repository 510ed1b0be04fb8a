"""Python-integer restatement of Galois-ring slots (EncryptedArray(context, G), G the Hensel lift of F_0, plaintext space
p^r) and of the normal-basis passage of src/intraSlot.cpp, shared by the host and the device tests.  It starts from
tests/bgv_pr_ref.py's Hensel-lifted factors and idempotents and shares no method with helib_amd/csrc/bgv_gf.h,
helib_amd/bgv_gr.py or helib_amd/intraslot.py: no sliding window, no fold, no per-slot matrices, no trace, no Gram matrix.

  encode   the literal CRT: H = sum_i c_i E_i mod (Phi_m, p^r), c_i = alpha_i(X^(t_i)) mod F_i (Horner), balanced
  decode   slot i = (H mod F_i)(X^(1/t_i)) mod G (Horner in Z_(p^r)[X] / G)
  mul / sigma     the product in Z_(p^r)[X] / G and alpha -> alpha(X^p) mod G
  first_normal    the module's rule restated: X^k first, then the 0/1 polynomials in increasing integer order, the
                  first whose conjugates have a non-zero determinant mod p (Laplace-free: fraction-free elimination
                  over Z_p)
  coords   the normal-basis coordinates of alpha by solving sum_i c_i sigma^i(theta) = alpha (Gauss-Jordan, unit pivots)
  circulant       hx_mul_add_circulant word for word: out[i] = sum_j c[(i + j) mod d] in[j] mod q
Slots are lists / arrays [B, nslots, d], coefficients lowest first."""
import functools

import numpy as np

from tests import bgv_pr_ref as PR


def compose(a, x, f, P):
    """a(x) mod (f, P), a given by its coefficients (Horner); lists of python integers, len(f) - 1 words out"""
    d = len(f) - 1
    r = [0] * d
    for c in reversed([int(v) % P for v in a]):
        r = PR.mulmod(r, x, f, P)
        r = (r + [0] * d)[:d]
        r[0] = (r[0] + c) % P
    return r


def powmod(x, e, f, P):
    d = len(f) - 1
    r = [1 % P] + [0] * (d - 1)
    b = (list(x) + [0] * d)[:d]
    while e:
        if e & 1:
            r = (PR.mulmod(r, b, f, P) + [0] * d)[:d]
        b = (PR.mulmod(b, b, f, P) + [0] * d)[:d]
        e >>= 1
    return r


def xmod(f, P):
    """X mod f"""
    d = len(f) - 1
    return [(-f[0]) % P] if d == 1 else [0, 1] + [0] * (d - 2)


class _Lifted:
    """the members of bgv_pr_ref.Tables that GrTables reads, over factors and idempotents lifted earlier (from_golden)"""

    def __init__(self, m, p, r, F, E):
        from helib_amd import hostnt
        self.z = hostnt.ZmStar(m, p)
        self.P = p ** r
        self.d, self.nslots, self.phim = self.z.ordP, self.z.getNSlots(), len(E[0])
        self.phi = [int(c) for c in hostnt.phimx(m)]
        self.F, self.E = [list(map(int, f)) for f in F], [list(map(int, e)) for e in E]
        assert len(self.F) == len(self.E) == self.nslots and all(len(f) == self.d + 1 for f in self.F)
        for f in self.F:                                  # what was stored are monic factors of Phi_m modulo p^r
            assert f[-1] == 1 and not any(PR._divmod(self.phi, f, self.P)[1])

    balanced = PR.Tables.balanced


class GrTables:
    def __init__(self, m, p, r, lifted=None):
        self.base = b = PR.tables(m, p, r) if lifted is None else _Lifted(m, p, r, *lifted)
        self.m, self.p, self.r, self.P = m, p, r, p ** r
        self.d, self.nslots, self.phim, self.z = b.d, b.nslots, b.phim, b.z
        self.F, self.G = b.F, b.F[0]
        P = self.P
        self.t = [b.z.ith_rep(i) for i in range(self.nslots)]
        self.xt = [powmod(xmod(f, P), t, f, P) for t, f in zip(self.t, self.F)]            # X^(t_i) mod F_i
        self.y = [powmod(xmod(self.G, P), pow(t, -1, m), self.G, P) for t in self.t]      # X^(1/t_i) mod G
        self.xp = powmod(xmod(self.G, P), p, self.G, P)                                    # X^p mod G

    def slots(self, a):
        a = np.asarray(a, dtype=object)
        if a.ndim == 2:
            a = a[:, :, None]
        out = np.zeros((a.shape[0], self.nslots, self.d), dtype=object)
        out[:, :a.shape[1], :a.shape[2]] = a
        return out

    def encode(self, a, mul=1):
        """-> balanced(mul * H mod p^r) [B, phim]"""
        P, b, n = self.P, self.base, self.phim
        out = []
        for row in self.slots(a):
            h = [0] * n
            for i, alpha in enumerate(row):
                c = compose(alpha, self.xt[i], self.F[i], P)
                if any(c):
                    t = PR.mulmod(c, b.E[i], b.phi, P)
                    h = [(x + (t[k] if k < len(t) else 0)) % P for k, x in enumerate(h)]
            out.append([x * (mul % P) % P for x in h])
        return b.balanced(out)

    def decode(self, coeffs, k=None):
        """polynomials [B, phim] (any integers) -> slots [B, nslots, d] in [0, p^k) (k = None: r)"""
        P = self.P
        Pk = P if k is None else self.p ** k
        out = []
        for row in np.atleast_2d(np.asarray(coeffs, dtype=object)):
            h = [int(x) % P for x in row]
            vals = []
            for i, f in enumerate(self.F):
                rem = PR._divmod(h, f, P)[1]
                vals.append([x % Pk for x in compose(rem, self.y[i], self.G, P)])
            out.append(vals)
        return np.array(out, dtype=np.int64)

    def mul1(self, x, y):
        d = self.d
        return (PR.mulmod([int(v) % self.P for v in x], [int(v) % self.P for v in y], self.G, self.P) + [0] * d)[:d]

    def sigma1(self, x, j=1):
        x = [int(v) % self.P for v in x]
        for _ in range(j % self.d):
            x = compose(x, self.xp, self.G, self.P)
        return x

    def _each(self, a, fn):
        a = self.slots(a)
        return np.array([[fn(b, i, a[b, i]) for i in range(a.shape[1])] for b in range(a.shape[0])], dtype=np.int64)

    def mul(self, a, b):
        b = self.slots(b)
        return self._each(a, lambda bb, i, x: self.mul1(x, b[bb, i]))

    def sigma(self, a, j=1):
        return self._each(a, lambda bb, i, x: self.sigma1(x, j))

    # ---- the normal basis ----
    def conjugates(self, theta):
        rows = [[int(v) % self.P for v in theta]]
        for _ in range(1, self.d):
            rows.append(self.sigma1(rows[-1]))
        return rows

    def first_normal(self):
        """the rule, by brute force: (theta, CB)"""
        d = self.d
        cands = [[1 if i == k else 0 for i in range(d)] for k in range(d)] + [[(n >> i) & 1 for i in range(d)] for n in range(1, 1 << d)]
        for theta in cands:
            CB = self.conjugates(theta)
            if det_mod(CB, self.p):
                return theta, CB
        raise AssertionError("no normal element among the 0/1 polynomials")

    def coords(self, CB, alpha):
        """c with sum_i c_i CB[i] = alpha mod p^r"""
        d, P = self.d, self.P
        A = [[CB[i][j] for i in range(d)] + [int(alpha[j]) % P] for j in range(d)]     # columns are the conjugates
        for c in range(d):
            piv = next(r for r in range(c, d) if A[r][c] % self.p)
            A[c], A[piv] = A[piv], A[c]
            inv = pow(A[c][c], -1, P)
            A[c] = [x * inv % P for x in A[c]]
            for r in range(d):
                if r != c and A[r][c]:
                    f = A[r][c]
                    A[r] = [(x - f * y) % P for x, y in zip(A[r], A[c])]
        return [A[j][d] for j in range(d)]


def det_mod(M, p):
    """the determinant of a square integer matrix modulo the prime p"""
    M = [[int(x) % p for x in row] for row in M]
    n, det = len(M), 1
    for c in range(n):
        piv = next((r for r in range(c, n) if M[r][c]), None)
        if piv is None:
            return 0
        if piv != c:
            M[c], M[piv] = M[piv], M[c]
            det = -det
        det = det * M[c][c] % p
        inv = pow(M[c][c], -1, p)
        for r in range(c + 1, n):
            f = M[r][c] * inv % p
            if f:
                M[r] = [(x - f * y) % p for x, y in zip(M[r], M[c])]
    return det % p


@functools.lru_cache(maxsize=None)
def tables(m, p, r):
    return GrTables(m, p, r)


def from_golden(path):
    """GrTables over the lifted factors F and idempotents E stored in a JSON file {"m", "p", "r", "F", "E"} (what
    tables(m, p, r) computes, written once by tests/golden/make_intraslot_golden.py: at d = 64 the lifting takes seconds)"""
    import json
    with open(path) as fh:
        g = json.load(fh)
    return GrTables(g["m"], g["p"], g["r"], lifted=(g["F"], g["E"]))


def circulant(c_rows, in_rows, qs, nout):
    """hx_mul_add_circulant in python integers.  c_rows[t], in_rows[j]: arrays [rows, ...] (row r modulo qs[r]; a
    constant broadcasts against an input) -> nout object arrays of the inputs' shape"""
    d = len(c_rows)
    assert len(in_rows) == d and 1 <= nout <= d
    c = [np.asarray(x).astype(object) for x in c_rows]
    x = [np.asarray(v).astype(object) for v in in_rows]
    out = []
    for i in range(nout):
        acc = np.zeros(x[0].shape, dtype=object)
        for j in range(d):
            acc = acc + c[(i + j) % d] * x[j]
        for r, q in enumerate(qs):
            acc[r] = acc[r] % int(q)
        out.append(acc)
    return out
