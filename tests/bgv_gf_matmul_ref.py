"""Restatement of the linear maps on GF(p^d) slots from the definitions, on tests/bgv_gf_ref.py's literal CRT and
tests/bgv_crt_ref.py's polynomial arithmetic over Z_p.  No tables of its own: no Frobenius matrices, no inverse of the
Moore matrix, no slot permutation.

  linpoly_solve    the C with sum_k C[k] (X^j)^(p^k) = L[j] mod G for every j, found by solving that system of d^2
                   equations over Z_p directly (small d)
  linpoly_holds    whether a given C satisfies those d equations (any d; the solution is unique)
  automorph        encode literally, substitute X -> X^k modulo Phi_m and p on the polynomial, decode literally
  mul_block / mul_gf   mul(PlaintextArray, BlockMatMul1D / MatMul1D) as plain loops over breakIndexByDim"""
import numpy as np

from tests import bgv_crt_ref as R
from tests import bgv_gf_ref as GR


def _pad(v, d):
    v = np.asarray(v, dtype=np.int64)
    return np.pad(v, (0, d - len(v)))


def _pow_basis(ref):
    """P[k][j] = (X^j)^(p^k) mod G as d coefficients"""
    p, d, G = ref.p, ref.d, ref.G
    X = np.array([0, 1], dtype=np.int64)
    out = []
    for k in range(d):
        xk = R.ppowmod(X, p ** k, G, p) if d > 1 else R.prem(X, G, p)
        out.append([_pad(R.ppowmod(xk, j, G, p) if j else [1], d) for j in range(d)])
    return out


def _fmul(a, b, ref):
    return _pad(R.prem(R.pmul(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), ref.p), ref.G, ref.p), ref.d)


def linpoly_holds(ref, C, L):
    p, d = ref.p, ref.d
    P = _pow_basis(ref)
    for j in range(d):
        s = np.zeros(d, dtype=object)
        for k in range(d):
            s = (s + _fmul(C[k], P[k][j], ref)) % p
        if [int(x) for x in s] != [int(x) % p for x in L[j]]:
            return False
    return True


def linpoly_solve(ref, L):
    """unknowns C[k][c]; equation (j, e): sum_(k, c) C[k][c] [X^e](X^c P[k][j] mod G) = L[j][e]"""
    p, d = ref.p, ref.d
    P = _pow_basis(ref)
    n = d * d
    A = [[0] * (n + 1) for _ in range(n)]
    for j in range(d):
        for k in range(d):
            for c in range(d):
                col = _fmul(np.eye(d, dtype=np.int64)[c], P[k][j], ref)
                for e in range(d):
                    A[j * d + e][k * d + c] = int(col[e])
        for e in range(d):
            A[j * d + e][n] = int(L[j][e]) % p
    for c in range(n):
        piv = next(r for r in range(c, n) if A[r][c])
        A[c], A[piv] = A[piv], A[c]
        inv = pow(A[c][c], -1, p)
        A[c] = [x * inv % p for x in A[c]]
        for r in range(n):
            if r != c and A[r][c]:
                f = A[r][c]
                A[r] = [(x - f * y) % p for x, y in zip(A[r], A[c])]
    return np.array([[A[k * d + c][n] for c in range(d)] for k in range(d)], dtype=np.int64)


def automorph(ref, a, k):
    """slots [B, n, d] -> the slots of H(X^k) mod (Phi_m, p)"""
    m, p = ref.m, ref.p
    out = []
    for h in ref.encode(a):
        g = np.zeros(m, dtype=np.int64)
        for i, c in enumerate(h):
            g[i * k % m] = (g[i * k % m] + int(c)) % p
        r = R.prem(g, ref.base.phi, p)
        out.append(_pad(r, ref.phim))
    return ref.decode(np.array(out))


def break_index(ords, s, dim):
    """CubeSignature::breakIndexByDim -> (the index of the other coordinates, the coordinate along dim)"""
    if dim == len(ords):
        return s, 0
    lo = 1
    for x in ords[dim + 1:]:
        lo *= x
    hi = lo * ords[dim]
    return s % lo + s // hi * lo, s % hi // lo


def _mul(ref, v, A, dim, entry):
    ords = ref.z.ords
    n, d, p = ref.nslots, ref.d, ref.p
    D = 1 if dim == len(ords) else ords[dim]
    A = np.asarray(A)
    where = {break_index(ords, s, dim): s for s in range(n)}
    out = np.zeros(v.shape, dtype=np.int64)
    for b in range(v.shape[0]):
        for k in range(n // D):
            for j in range(D):
                acc = np.zeros(d, dtype=object)
                for i in range(D):
                    acc = (acc + entry(v[b, where[k, i]], A[k][i][j] if A.ndim == 5 else A[i][j])) % p
                out[b, where[k, j]] = [int(x) for x in acc]
    return out


def mul_block(ref, v, A, dim):
    """A [D, D, d, d] or [n / D, D, D, d, d]: the coefficient row vector of a slot times the d x d block"""
    p = ref.p
    return _mul(ref, np.asarray(v), A, dim,
                lambda x, a: np.array([sum(int(x[l]) * int(a[l][c]) for l in range(ref.d)) % p for c in range(ref.d)], dtype=object))


def mul_gf(ref, v, A, dim):
    """A [D, D, d]: the product in Z_p[X] / G"""
    return _mul(ref, np.asarray(v), A, dim, lambda x, a: _fmul(x, a, ref))


tables = GR.tables
