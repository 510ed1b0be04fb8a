"""What the BGV linear-array tests (tests/test_bgv_linalg_host.py, tests/test_bgv_linalg_gpu.py) share: the plaintext
maps the ciphertext operations are held to -- numpy on the slots, never the code under test -- the amounts to move by,
the automorphisms those amounts need matrices for, and a CPU encoder for the host test."""
import numpy as np

from tests import bgv_slots_ref as R


# ---- truth ----
def rotate(a, amt):
    return np.roll(a, amt, axis=1)              # slot j moves to slot j + amt mod n


def shift(a, k):
    """slot j moves to slot j + k, zeros come in"""
    n = a.shape[1]
    out = np.zeros_like(a)
    if 0 <= k < n:
        out[:, k:] = a[:, :n - k]
    elif -n < k < 0:
        out[:, :n + k] = a[:, -k:]
    return out


def total_sums(a, p):
    return np.repeat(a.sum(axis=1, keepdims=True) % p, a.shape[1], axis=1)


def running_sums(a, p):
    return np.cumsum(a, axis=1) % p


# ---- amounts ----
def strides(ords):
    s = [1] * len(ords)
    for i in range(len(ords) - 2, -1, -1):
        s[i] = s[i + 1] * ords[i + 1]
    return s


def amounts(ords):
    """0, +-1, n - 1, n, -n, n + 3, and for every dimension i an amount whose coordinate in i is 0 and one whose
    coordinate is ord_i - 1 (so that v + 1 wraps), the other coordinates being 1"""
    n = int(np.prod(ords))
    st = strides(ords)
    out = [0, 1, -1, n - 1, n, -n, n + 3]
    for i in range(len(ords)):
        for c in (0, ords[i] - 1):
            out.append(sum(st[j] * (c if j == i else 1 % ords[j]) for j in range(len(ords))))
    return list(dict.fromkeys(out))


def needed_automorphisms(z, amts):
    """every k whose matrix rotate / shift by one of amts goes through: g_i^v and g_i^(v + 1), v the coordinate of the
    amount in dimension i"""
    n, st, need = z.getNSlots(), strides(z.ords), set()
    for amt in amts:
        for i, d in enumerate(z.ords):
            v = amt % n // st[i] % d
            need |= {z.genToPow(i, v), z.genToPow(i, (v + 1) % d)}
    return sorted(need - {1})


def sums_amounts(n):
    """the shifts of runningSums and the rotations of totalSums (src/EncryptedArray.cpp:695-736) for n slots"""
    sh, s = [], 1
    while s < n:
        sh.append(s)
        s *= 2
    rot, e = [], 1
    for i in range(n.bit_length() - 2, -1, -1):
        rot.append(e)
        e *= 2
        if (n >> i) & 1:
            rot.append(e)
            e += 1
    return sh, rot


# ---- a CPU encoder ----
def inverse_mod(A, p):
    """Gauss-Jordan over Z_p (p < 2^31)"""
    n = A.shape[0]
    M = np.concatenate([A % p, np.eye(n, dtype=np.int64)], axis=1)
    for c in range(n):
        r = c + int(np.nonzero(M[c:, c])[0][0])
        M[[c, r]] = M[[r, c]]
        M[c] = M[c] * pow(int(M[c, c]), -1, p) % p
        f = M[:, c].copy()
        f[c] = 0
        M = (M - f[:, None] * M[c][None, :]) % p
    return M[:, n:]


class HostEncoder:
    """the encoder's members (helib_amd.bgv.DeviceEncoder) on the CPU for one vector at a time: H is the interpolation
    polynomial through (root of F_i, a_i), i.e. the inverse of the Vandermonde matrix of the roots applied to the
    slots -- CRT_reconstruct's result without its idempotents, which cost n^3"""

    def __init__(self, be, m, p):
        self.be, self.m, self.p = be, m, p
        pts = R.points(m, p)
        n = len(pts)
        self.V = np.ones((n, n), dtype=np.int64)
        for k in range(1, n):
            self.V[:, k] = self.V[:, k - 1] * np.array(pts, dtype=np.int64) % p
        self.Vinv = inverse_mod(self.V, p)

    def coeffs(self, v, mul=1):
        n = self.V.shape[0]
        a = np.zeros((np.atleast_2d(v).shape[0], n), dtype=np.int64)
        a[:, :np.atleast_2d(v).shape[1]] = np.atleast_2d(v) % self.p
        return R.balanced((self.Vinv @ a.T % self.p).T * (mul % self.p), self.p)

    def encode(self, v, mul, idx, coeffs=False):
        cf = self.coeffs(v, mul)
        d = None
        if idx:
            assert cf.shape[0] == 1, "the CPU backend takes one vector at a time"
            d = self.be.fromCoeffs(idx, cf[0])
            d.batch = 1
        return (d, cf) if coeffs else d

    def embed(self, coeffs):
        return (self.V @ (np.atleast_2d(coeffs) % self.p).T % self.p).T

    def decode(self, acc, factor_inv):
        cf = np.array([[int(x) % self.p * factor_inv % self.p for x in self.be.toPoly(acc)]], dtype=np.int64)
        return self.embed(cf)

    def norm(self, coeffs):
        return np.array([self.be.embeddingLargestCoeff(row) for row in np.atleast_2d(coeffs)])
