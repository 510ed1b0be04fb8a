"""Restatement of EncryptedArray's slot maps for d = ord_m(p) = 1 (p = 1 mod m, r = 1) in python integers / numpy,
written from the reference's definitions and independent of any transform:

  factors of Phi_m mod p   X - a over the primitive m-th roots of unity a; factor 0 is the smallest by poly_comp
                           (src/PAlgebra.cpp:67-81: constant coefficient p - a first, as residues in [0, p)), i.e.
                           F_0 = X - rho with rho the LARGEST primitive m-th root
  factor i                 the minimal polynomial of X^(1/t_i) mod F_0, t_i = ith_rep(i) (:726-733): X - rho^(1/t_i mod m)
  encode                   CRT_reconstruct (:750-756, 1007-1045): sum_i a_i * E_i, E_i = prod_(j != i) F_j *
                           (prod_(j != i) F_j mod F_i)^-1, then balanced_zzX (src/EncryptedArray.cpp:438-447)
  decode                   slot i = H mod F_i = H(rho^(1/t_i))
"""
import math

import numpy as np

from helib_amd import hostnt


def primitive_roots(m, p):
    """every element of order exactly m in Z_p^*, by its definition (p - 1 candidates: small p only)"""
    assert (p - 1) % m == 0
    fac = [q for q in range(2, m + 1) if m % q == 0 and hostnt.is_prime(q)]
    return [a for a in range(1, p) if pow(a, m, p) == 1 and all(pow(a, m // q, p) != 1 for q in fac)]


def rho_of(m, p):
    """the largest primitive m-th root of unity mod p, without listing Z_p: the powers z^j, gcd(j, m) = 1, of one"""
    fac = [q for q in range(2, m + 1) if m % q == 0 and hostnt.is_prime(q)]
    g = 2
    while True:
        z = pow(g, (p - 1) // m, p)
        if all(pow(z, m // q, p) != 1 for q in fac):
            break
        g += 1
    best, x = 0, 1
    for j in range(1, m):
        x = x * z % p
        if math.gcd(j, m) == 1 and x > best:
            best = x
    return best


def zmstar(m, p):
    return hostnt.ZmStar(m, p)


def points(m, p, z=None):
    """the root of F_i for every slot i"""
    z = z or zmstar(m, p)
    rho = rho_of(m, p)
    return [pow(rho, pow(z.ith_rep(i), -1, m), p) for i in range(z.getNSlots())]


def balanced(x, p):
    x = np.asarray(x, dtype=np.int64) % p
    return np.where(x > p // 2, x - p, x)


def _polymul(a, b, p):
    return np.convolve(a, b) % p        # coefficients < p < 2^20 and short polynomials: no overflow in int64


def encode_crt(a, m, p, pts=None):
    """the literal CRT with idempotents (small m): a[nslots] -> balanced coefficients [phi(m)]"""
    pts = pts or points(m, p)
    n = len(pts)
    a = [int(x) % p for x in a] + [0] * (n - len(a))
    F = [np.array([(p - r) % p, 1], dtype=np.int64) for r in pts]       # X - r, lowest coefficient first
    H = np.zeros(n, dtype=np.int64)
    for i in range(n):
        prod = np.array([1], dtype=np.int64)
        for j in range(n):
            if j != i:
                prod = _polymul(prod, F[j], p)
        rem = horner(prod[None, :], [pts[i]], p)[0, 0]                   # prod mod F_i
        H = (H + prod * (a[i] * pow(int(rem), -1, p) % p)) % p
    return balanced(H, p)


def horner(coeffs, x, p):
    """coeffs[B, n] (any sign) evaluated at the points x[P] mod p -> [B, P] (p < 2^31)"""
    c = np.asarray(coeffs, dtype=np.int64) % p
    x = np.asarray(x, dtype=np.int64).reshape(1, -1)
    acc = np.zeros((c.shape[0], x.shape[1]), dtype=np.int64)
    for k in range(c.shape[1] - 1, -1, -1):
        acc = (acc * x + c[:, k:k + 1]) % p
    return acc


def decode(coeffs, m, p, pts=None, which=None):
    """slots [B, len(which)] of the polynomials coeffs[B, phi(m)]"""
    pts = pts or points(m, p)
    which = range(len(pts)) if which is None else which
    return horner(coeffs, [pts[i] for i in which], p)
