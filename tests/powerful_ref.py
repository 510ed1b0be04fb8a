"""TEST INFRASTRUCTURE: the powerful basis in python integers, straight from the definition (src/powerful.cpp:22-244 of the
reference): index maps, and schoolbook long division by the cyclotomic polynomial.  The ground truth of
tests/test_evalmap_host.py and tests/test_evalmap_gpu.py; it imports nothing of helib_amd.powerful and does not use the
binomial form of Phi_n for a division."""
import functools
from math import gcd

import numpy as np


def divisors(n):
    return [d for d in range(1, n + 1) if n % d == 0]


def phi(n):
    return sum(1 for j in range(1, n + 1) if gcd(j, n) == 1)


def _divexact(a, b):
    """a / b over the integers, b monic, coefficients lowest first; the remainder must be zero"""
    a, out = list(a), [0] * (len(a) - len(b) + 1)
    for i in range(len(a) - len(b), -1, -1):
        c = a[i + len(b) - 1]
        out[i] = c
        for j, x in enumerate(b):
            a[i + j] -= c * x
    assert not any(a)
    return out


@functools.lru_cache(maxsize=None)
def cyclotomic(n):
    """Phi_n over the integers, lowest coefficient first: (x^n - 1) / prod_(d | n, d < n) Phi_d"""
    f = [-1] + [0] * (n - 1) + [1]
    for d in divisors(n):
        if d < n:
            f = _divexact(f, cyclotomic(d))
    return tuple(f)


def poly_rem(a, f, q):
    """a mod the monic f, modulo q, by schoolbook long division -> deg f words.  q = None: over the integers (the
    conversions are Z-linear, so one division over Z reduced modulo q serves every modulus q)"""
    df = len(f) - 1
    # one row operation per quotient word; numpy only carries the row (int64 where no product can leave it, python
    # integers otherwise)
    dt = np.int64 if q is not None and q * max(abs(x) for x in f) < 2 ** 62 else object
    a, fv = np.array([int(x) if q is None else int(x) % q for x in a], dtype=dt), np.array(f, dtype=dt)
    for i in range(len(a) - 1, df - 1, -1):
        c = a[i]
        if c:
            a[i - df:i + 1] = a[i - df:i + 1] - c * fv if q is None else (a[i - df:i + 1] - c * fv) % q
    return ([int(x) for x in a] + [0] * df)[:df]


def binomials(n):
    """(num, den), sorted: Phi_n = prod_(e in num) (x^e - 1) / prod_(e in den) (x^e - 1) without the factor x^n - 1,
    e = n / s over the squarefree s | n, s > 1, with mu(s) = +1 / -1"""
    primes = [q for q in divisors(n) if q > 1 and all(q % t for t in range(2, q))]
    num, den = [], []
    for mask in range(1, 1 << len(primes)):
        s, bits = 1, 0
        for i, q in enumerate(primes):
            if mask >> i & 1:
                s, bits = s * q, bits + 1
        (den if bits % 2 else num).append(n // s)
    return sorted(num), sorted(den)


class Indexes:
    """PowerfulTranslationIndexes: m, phim, phivec, polyToCubeMap, cubeToPolyMap, shortToLongMap"""

    def __init__(self, mvec):
        self.mvec = mvec = [int(x) for x in mvec]
        k = self.k = len(mvec)
        m = 1
        for x in mvec:
            m *= x
        self.m, self.phivec = m, [phi(x) for x in mvec]
        self.phim = 1
        for x in self.phivec:
            self.phim *= x
        inv = [pow(m // mi % mi, -1, mi) if mi > 1 else 0 for mi in mvec]

        def index(coords, sig):
            j = 0
            for c, n in zip(coords, sig):
                j = j * n + c
            return j
        self.polyToCubeMap = [index([(i % mi) * iv % mi for mi, iv in zip(mvec, inv)], mvec) for i in range(m)]
        self.cubeToPolyMap = [0] * m
        for i, j in enumerate(self.polyToCubeMap):
            self.cubeToPolyMap[j] = i
        self.shortToLongMap = []
        for i in range(self.phim):
            coords, rest = [], i
            for n in reversed(self.phivec):
                coords.append(rest % n)
                rest //= n
            self.shortToLongMap.append(index(coords[::-1], mvec))
        self.shortToExp = [self.cubeToPolyMap[j] for j in self.shortToLongMap]
        assert sorted(self.polyToCubeMap) == list(range(m))
        for i in range(m):                                  # i = sum_d i_d (m / m_d) mod m
            coords, rest = [], self.polyToCubeMap[i]
            for n in reversed(mvec):
                coords.append(rest % n)
                rest //= n
            assert sum(c * (m // mi) for c, mi in zip(coords[::-1], mvec)) % m == i


@functools.lru_cache(maxsize=None)
def indexes(mvec):
    return Indexes(mvec)


def poly_to_powerful(F, mvec, q):
    """PowerfulConversion::polyToPowerful: phi(m) coefficients -> the cube of phi(m) words, all modulo q"""
    ix = indexes(tuple(mvec))
    cube = [0] * ix.m
    for i, x in enumerate(F):
        cube[ix.polyToCubeMap[i]] = int(x) if q is None else int(x) % q
    stride = ix.m
    for d, (n, ph) in enumerate(zip(ix.mvec, ix.phivec)):   # recursiveReduce: every hypercolumn of dimension d
        stride //= n
        f = cyclotomic(n)
        for base in range(ix.m):
            if base // stride % n:
                continue
            col = [cube[base + k * stride] for k in range(n)]
            rem = poly_rem(col, f, q) + [0] * (n - ph)
            for k in range(n):
                cube[base + k * stride] = rem[k]
    return [cube[j] for j in ix.shortToLongMap]


def powerful_to_poly(cube, mvec, q):
    """PowerfulConversion::powerfulToPoly"""
    ix = indexes(tuple(mvec))
    tmp = [0] * ix.m
    for i, x in enumerate(cube):
        tmp[ix.shortToExp[i]] = int(x) if q is None else int(x) % q
    return poly_rem(tmp, cyclotomic(ix.m), q)


# ---- the factorisations of the device tests, and what their reductions consist of ----
# (mvec, the prime p of the chain whose rows tests/test_evalmap_gpu.py converts): the first six are squarefree and odd;
# then a prime power with e = 3 in a per-factor dimension, the factor 4 (m = 20: p = 3), e = 5, the factor 8 beside a
# composite one (m = 120: p = 7), and four factors with a prime power among them (m = 4095)
DEVICE_MVECS = [((3, 5), 2), ((3, 35), 2), ((7, 3, 65), 2), ((17, 257), 2), ((7, 3, 221), 2), ((31,), 2),
                ((9, 5), 2), ((4, 5), 3), ((25, 3), 2), ((8, 15), 7), ((7, 5, 9, 13), 2)]
MANY_ITEMS = [(3, 5), (7, 3, 221)]                          # converted with more items than the kernel has workgroups


def reductions(mvec):
    """the reductions modulo a cyclotomic polynomial that the two conversions make, from their definition:
    (direction, n, phi(n), stride, nouter) -- to_powerful reduces, for each factor i, the fibres of length m_i and stride
    prod_(j > i) m_j whose earlier coordinates are below their phi(m_j) (prod_(j < i) phi(m_j) x stride of them) modulo
    Phi_(m_i); to_poly reduces one fibre of length m modulo Phi_m"""
    ix = indexes(tuple(mvec))
    out, stride, nouter = [], ix.m, 1
    for n, ph in zip(ix.mvec, ix.phivec):
        stride //= n
        out.append(("to_powerful", n, ph, stride, nouter))
        nouter *= ph
    return out + [("to_poly", ix.m, ix.phim, 1, 1)]


def remainder_steps(n):
    """the steps of one remainder modulo Phi_n = prod_(e in num) (x^e - 1) / prod_(e in den) (x^e - 1) / (x^n - 1)^-1 of a
    fibre of n words, as (half, op, e, L): the quotient from the reversed top n - phi(n) words, times the binomials of den
    and divided by those of num; then quotient times Phi_n on phi(n) words, times num and divided by den, and one
    subtraction.  A binomial whose e is not below L leaves the L words alone and is no step."""
    num, den = binomials(n)
    ph = phi(n)
    Lq = n - ph
    return ([("quotient", "REV", 0, Lq)] + [("quotient", "MUL", e, Lq) for e in den if e < Lq] +
            [("quotient", "DIV", e, Lq) for e in num if e < Lq] + [("remainder", "REVW", n - 1 - ph, ph)] +
            [("remainder", "MUL", e, ph) for e in num if e < ph] + [("remainder", "DIV", e, ph) for e in den if e < ph] +
            [("remainder", "SUB", 0, ph)])
