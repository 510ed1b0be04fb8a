"""Planted boundary integers for the exact RNS kernels, and what those kernels must return for them, from python
integers alone (helper of test_rns_boundary_host.py / test_rns_boundary_gpu.py).

The kernels between two transforms (rns_kernels.h, rns_mfma_kernels.hip, the single-prime prep store of
ntt_kernels.hip) are exact except for decisions taken per coefficient on the INTEGER the residues stand for: the
centring compare against (P-1)/2, the HPS quotient floor(z) / frac(z) > 1/2 from a double-precision sum with its
redo list inside hps_eps of 0, 1/2 and 1, and the tie dm == ptxtSpace/2 at an even plaintext space.  Uniform
residues never land there, so the values are planted: planted() lists them by class, hps_front() restates the
device's trust rule so that the classes provably sit on the intended side of the default threshold, the builders
put them into polynomials (coefficients first, uniform filler behind, batch element 1 rotated), and the want_*
functions state addPrimes / scaleDownToSet / breakIntoDigits / toPoly on python integers."""
import math
import os
import random
import re
from fractions import Fraction
from functools import reduce

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES_H = os.path.join(ROOT, "helib_amd", "csrc", "switches.h")
CLASSES = ("zero", "half", "inside_eps", "outside_eps", "single_y", "thirds")
ROTATE = 37       # batch element 1 = element 0 rotated by this many coefficients
MIN_FILLER = 16   # uniform coefficients behind the planted ones, at least


def default_hps_eps(path=SWITCHES_H):
    """Switches::hps_eps as switches.h initialises it (1.0 / (double)(1u << K)); a form this cannot parse fails."""
    with open(path) as f:
        text = f.read()
    found = re.findall(r"double\s+hps_eps\s*=\s*1\.0\s*/\s*\(double\)\s*\(\s*1u\s*<<\s*(\d+)\s*\)\s*;", text)
    assert len(found) == 1, "switches.h: the initialiser of Switches::hps_eps is not in the form this helper parses"
    return 1.0 / float(1 << int(found[0]))


def prod(xs):
    return reduce(lambda a, b: a * b, xs, 1)


def centre(x, P):
    """x in [0, P) -> the representative in [-(P-1)/2, (P-1)/2] (P odd)"""
    return x - P if x > (P - 1) // 2 else x


def hps_front(ps, x, eps):
    """hps_front of rns_kernels.h in python doubles (as tests/test_oracle_rns.py restates it): y_k = x (P/p_k)^-1 mod
    p_k, z = sum_k double(y_k) * double(1/p_k), v = floor(z), neg = frac(z) > 1/2, the value sum_k y_k (P/p_k) -
    (v + neg) P.  Returns (trusted, value_if_trusted == x centred, neg_if_trusted == (x > (P-1)/2))."""
    P = prod(ps)
    z, s = 0.0, 0
    for p in ps:
        Pk = P // p
        y = (x % p) * pow(Pk % p, -1, p) % p
        z += float(y) * (1.0 / float(p))
        s += y * Pk
    fl = math.floor(z)
    f = z - fl
    neg = f > 0.5
    trusted = not (f < eps or f > 1.0 - eps or abs(f - 0.5) < eps)
    return trusted, s - (int(fl) + (1 if neg else 0)) * P == centre(x, P), neg == (x > (P - 1) // 2)


def planted(ps, ptxt):
    """[(class, x)], x in [0, P): see the module docstring and CLASSES.  No value is listed twice within a class."""
    P = prod(ps)
    h = (P - 1) // 2
    out = []

    def add(cls, vals):
        seen = set()
        for v in vals:
            v %= P
            if v not in seen:
                seen.add(v)
                out.append((cls, v))

    # zero: 0, +-1, +-2; +-1 is the tie dm == ptxt/2 at ptxt = 2 and +-2, +-6 (x P^-1 mod 4 == 2: P is odd) at ptxt = 4,
    # +-ptxt/2 and +-3 ptxt/2 at any other even ptxt
    z = [0, 1, -1, 2, -2, 6, -6]
    if ptxt > 1 and ptxt % 2 == 0:
        z += [ptxt // 2, -(ptxt // 2), 3 * (ptxt // 2), -3 * (ptxt // 2)]
    add("zero", z)
    add("half", [h + d for d in (-2, -1, 0, 1, 2, 3)])           # (P-1)/2 and (P+1)/2, each with two neighbours outwards
    add("inside_eps", [b + s * (P >> k) for b in (0, h) for k in (40, 31) for s in (1, -1)])
    add("outside_eps", [b + s * (P >> k) for b in (0, h) for k in (29, 27) for s in (1, -1)])
    add("single_y", [(P // p) * j for p in ps for j in (1, 2, p - 1)])
    add("thirds", [P // 3 + d for d in (-1, 0, 1)])
    return out


def classes_present(values, ps, ptxt):
    """the classes of planted(ps, ptxt) of which at least one value occurs in `values` (integers mod P)"""
    have = {v % prod(ps) for v in values}
    return {cls for cls, x in planted(ps, ptxt) if x in have}


def class_of(x, ps, ptxt):
    """the classes a value belongs to ('' for filler): for assertion messages"""
    return "/".join(sorted({cls for cls, v in planted(ps, ptxt) if v == x % prod(ps)}))


def _chunks(items, N):
    """items dealt round-robin into the fewest lists of at most N - MIN_FILLER, so that every class (classes are
    contiguous runs of at least as many items as there are lists) occurs in every list"""
    cap = N - MIN_FILLER
    k = -(-len(items) // cap)
    return [items[c::k] for c in range(k)]


def _batch(coef):
    """batch element 0 and the same coefficients rotated by ROTATE positions"""
    N = len(coef)
    return [coef, [coef[(i - ROTATE) % N] for i in range(N)]]


def extension_inputs(ps, ptxt, N, seed):
    """polynomials (one per chunk of the planted list, each [2][N] integers in [0, P)) whose coefficients ARE the
    planted values, uniform filler behind them"""
    P = prod(ps)
    rng = random.Random(seed)
    out = []
    for ch in _chunks(planted(ps, ptxt), N):
        coef = [x for _, x in ch] + [rng.randrange(P) for _ in range(N - len(ch))]
        out.append(_batch(coef))
    return out


def scale_down_inputs(drop_ps, keep_ps, ptxt, N, seed):
    """c = delta + P r mod Q, delta the centred planted value modulo the dropped primes' product P and r uniform in
    [0, Q/P): the dropped rows stand for delta, the kept rows are not trivial"""
    P, K = prod(drop_ps), prod(keep_ps)
    rng = random.Random(seed)
    out = []
    for ch in _chunks(planted(drop_ps, ptxt), N):
        xs = [x for _, x in ch] + [rng.randrange(P) for _ in range(N - len(ch))]
        out.append(_batch([(centre(x, P) + P * rng.randrange(K)) % (P * K) for x in xs]))
    return out


def digit_inputs(digit_ps, which, N, seed):
    """x = d_0 + P_0 (d_1 + P_1 (d_2 ...)) mod Q with the planted values (centred) as digit `which` and uniform centred
    values as the others: a later digit is then what the fix-up digits[j] -= digits[i]; digits[j] /= P_i leaves"""
    Pd = [prod(d) for d in digit_ps]
    Q = prod(Pd)
    rng = random.Random(seed)
    out = []
    for ch in _chunks(planted(digit_ps[which], 4), N):
        coef = []
        for i in range(N):
            v = 0
            for j in range(len(Pd) - 1, -1, -1):
                if j == which and i < len(ch):
                    d = centre(ch[i][1], Pd[j])
                else:
                    d = rng.randrange(-((Pd[j] - 1) // 2), (Pd[j] - 1) // 2 + 1)
                v = v * Pd[j] + d
            coef.append(v % Q)
        out.append(_batch(coef))
    return out


def residue_rows(coef, ps):
    """[len(ps)][N] words: the coefficients (any integers) modulo each prime"""
    return np.array([[v % p for v in coef] for p in ps], dtype=np.uint64)


def eval_rows(ctx, idx, batch):
    """[len(idx)][len(batch)][N] rows in evaluation form (through the oracle context's forward transform)"""
    ps = [ctx.primes[i] for i in idx]
    return np.stack([ctx.fft(idx, residue_rows(coef, ps)) for coef in batch], axis=1)


# ---- what the operations return, on python integers (src/DoubleCRT.cpp:479-599, 925-1113, 1464-1516) ----
def want_to_poly(coef, ps):
    P = prod(ps)
    return [centre(v % P, P) for v in coef]


def want_add_primes(coef, src_ps, tgt_ps):
    """coefficient-domain rows of the centred value on the new primes"""
    return residue_rows(want_to_poly(coef, src_ps), tgt_ps)


def want_digits(coef, own_ps, digits, all_ps):
    """digits: lists of positions in own_ps.  ([ndig][len(all_ps)][N] coefficient-domain words, [ndig][N] digit / P_d,
    [ndig][N] the digits themselves)"""
    cur = want_to_poly(coef, own_ps)
    rows, frac, digs = [], [], []
    for d in digits:
        P = prod(own_ps[i] for i in d)
        dig = [centre(v % P, P) for v in cur]
        cur = [(v - r) // P for v, r in zip(cur, dig)]
        rows.append(residue_rows(dig, all_ps))
        frac.append([float(Fraction(r, P)) for r in dig])
        digs.append(dig)
    return np.stack(rows), np.array(frac), digs


def want_scale_down(coef, own_ps, drop, ptxt):
    """drop: positions in own_ps.  delta = c mod P centred, made divisible by ptxt by subtracting P * balanced(delta
    P^-1 mod ptxt) with the tie dm == ptxt/2 going to the sign of delta (as test_scale_down_matches_python states
    it); the kept rows of (c - delta) / P in coefficient domain, in own_ps order, and fdelta = delta / P."""
    drop_ps = [own_ps[i] for i in drop]
    keep_ps = [p for i, p in enumerate(own_ps) if i not in drop]
    P = prod(drop_ps)
    delta = want_to_poly(coef, drop_ps)
    if ptxt > 1:
        Pinv = pow(P % ptxt, -1, ptxt)
        fixed = []
        for v in delta:
            dm = v % ptxt
            if dm != 0:
                dm = dm * Pinv % ptxt
                if dm > ptxt // 2 or (ptxt % 2 == 0 and dm == ptxt // 2 and v < 0):
                    dm -= ptxt
                v -= P * dm
            assert v % ptxt == 0
            fixed.append(v)
        delta = fixed
    assert all((c - d) % P == 0 for c, d in zip(coef, delta))
    rows = []
    for q in keep_ps:
        Pq = pow(P % q, -1, q)
        rows.append([((c - d) % q) * Pq % q for c, d in zip(coef, delta)])
    return np.array(rows, dtype=np.uint64), np.array([float(Fraction(d, P)) for d in delta])


# ---- the prime chains of the boundary tests (recipes of tests/test_gpu_parity.py) ----
def many_source_chain(O, n, m):
    """n 60-bit sources, then six 60-bit, three 56-bit and two 45-bit targets (_many_source_extension_cases).  At n = 1
    the generator's first two primes are passed over: for them double(P - 1) * double(1 / P) stays below 1.0, and the
    one-term sum then has no lane with a right value and a wrong sign, which test_rns_boundary_host.py asks of every n."""
    g60, g56, g45 = O.PrimeGen(60, m), O.PrimeGen(56, m), O.PrimeGen(45, m)
    if n == 1:
        g60.next(), g60.next()
    return [g60.next() for _ in range(n + 6)] + [g56.next() for _ in range(3)] + [g45.next() for _ in range(2)]


def mixed_chain(O, m):
    """a 38-bit prime that is not of Proth form, five 60-bit and two 56-bit ones (test_proth_form_of_the_fast_rns_kernels)"""
    q38 = O.PrimeGen(38, m).next()
    assert q38 & 0xffffffff != 1 and q38 >> 32
    g60, g56 = O.PrimeGen(60, m), O.PrimeGen(56, m)
    return [q38] + [g60.next() for _ in range(5)] + [g56.next() for _ in range(2)]
