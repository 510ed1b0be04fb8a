"""Plain references for the integer kernels of the CKKS slot unit (helib_amd/csrc/ckks_slots.h), standard library and
numpy only (prime_sets alone asks the oracle's PrimeGen for primes):

  crt_exact / crt_model / crt_rel_bound     ckks_crt_double_kernel: centred CRT value / ratFactor
  residues_exact                            ckks_residues_kernel: int64 coefficient -> canonical residues
  embed_ld / encode_unrounded_ld            the two slot maps of tests/ckks_ref.py from their definitions, in longdouble
  fft_abs_bound                             forward error of the device's radix-2 transforms

and the planted inputs the tests of tests/test_ckks_planted_host.py / test_ckks_planted_gpu.py share, so that the CPU
file can hold exactly the cases the GPU file asserts to their conditions."""
import decimal
import functools
import math
import random

import numpy as np

LD = np.longdouble
NS = (1, 2, 8, 9, 16, 17, 32, 33, 64)       # both sides of every dispatch edge of ckks_crt_double_kernel<8/16/32/64>
KINDS = ("60", "mixed")
NEIGHBOURS = ("half_lo", "half_hi")         # (Q - 1)/2 and (Q + 1)/2: magnitude only (see the host file)
RANGE_LO, RANGE_HI = 2.0 ** -1000, 2.0 ** 1020


def _prod(xs):
    p = 1
    for x in xs:
        p *= int(x)
    return p


# ---------------------------------------------------------------------------------------------------------------
# the CRT kernel
# ---------------------------------------------------------------------------------------------------------------
def crt_exact(values, qs, ln_rat):
    """centred value / exp(ln_rat) as the nearest double: v mod Q, v > Q/2 -> v - Q in exact integers (the host's
    Decrypt), exp of the very double the call passes evaluated with `decimal` at 80 digits (a result beyond the
    double range comes back as inf, below it as 0)"""
    Q = _prod(qs)
    with decimal.localcontext() as c:
        c.prec = 80
        c.Emax, c.Emin = 10 ** 9, -10 ** 9
        R = decimal.Decimal(float(ln_rat)).exp()
        out = []
        for v in values:
            v = int(v) % Q
            if 2 * v > Q:
                v -= Q
            out.append(float(decimal.Decimal(v) / R))
    return np.array(out, dtype=np.float64)


def crt_exact_ld(values, qs, ln_rat):
    """crt_exact kept to longdouble precision (25 digits through a string): the input of embed_ld"""
    Q = _prod(qs)
    with decimal.localcontext() as c:
        c.prec = 80
        c.Emax, c.Emin = 10 ** 9, -10 ** 9
        R = decimal.Decimal(float(ln_rat)).exp()
        out = []
        for v in values:
            v = int(v) % Q
            if 2 * v > Q:
                v -= Q
            out.append(LD(format(decimal.Decimal(v) / R, ".25E")))
    return np.array(out, dtype=LD)


def _ld_of_int(q):
    """a 64-bit integer as a longdouble, exactly (two 32-bit halves)"""
    q = int(q)
    return LD(q >> 32) * LD(4294967296.0) + LD(q & 0xffffffff)


def crt_weights(qs, ln_rat):
    """hx_ckks_decode's weight table wm_k 2^we_k = P_k / ratFactor: long double log, floor, exp2"""
    wm, we = [], []
    run = -LD(float(ln_rat))
    ln2 = np.log(LD(2))
    for q in qs:
        l2 = run / ln2
        e = np.floor(l2)
        wm.append(float(np.exp2(l2 - e)))
        we.append(int(e))
        run = run + np.log(_ld_of_int(q))
    return wm, we


def crt_digits(v, qs):
    """Garner's mixed-radix digits of 0 <= v < Q: v = a_0 + a_1 q_0 + a_2 q_0 q_1 + ..."""
    a = []
    for q in qs:
        v, r = divmod(v, int(q))
        a.append(r)
    return a


def crt_model(values, qs, ln_rat):
    """The kernel's own double arithmetic restated: exact digits, frac = value/Q by Horner in doubles, the sign from
    frac > 0.5, then sum d_k wm_k 2^we_k over the non-zero digits (of Q - 1 - value, plus the weight of 1, when
    negative).  Returns (results, fracs, digits).  CPU only: it proves the conditions on the planted inputs and is
    never the expected value of a device assertion."""
    Q = _prod(qs)
    wm, we = crt_weights(qs, ln_rat)
    res, fracs, digs = [], [], []
    with np.errstate(over="ignore", under="ignore"):
        for v in values:
            a = crt_digits(int(v) % Q, qs)
            frac = 0.0
            for ak, q in zip(a, qs):
                frac = (frac + float(ak)) / float(q)
            neg = frac > 0.5
            acc = float(np.ldexp(wm[0], we[0])) if neg else 0.0
            for k, q in enumerate(qs):
                d = int(q) - 1 - a[k] if neg else a[k]
                if d:
                    acc += float(np.ldexp(np.float64(float(d) * wm[k]), we[k]))
            res.append(-acc if neg else acc)
            fracs.append(frac)
            digs.append(a)
    return np.array(res, dtype=np.float64), np.array(fracs, dtype=np.float64), digs


def crt_rel_bound(n, lnQ, ln_rat):
    """Relative error of a correct ckks_crt_double_kernel against crt_exact, for results in the normal double range:

        (n + 4) 2^-52 + (n + 1) (lnQ + |ln_rat| + 1) 2^-62.

    The kernel returns +-sum_k d_k w_k over at most n + 1 terms (the `+ 1` of the negative branch included), every term
    non-negative, so the relative error of the sum is at most the largest relative error of a term plus that of the
    additions: nothing cancels and nothing amplifies.
      * a term fl(fl(d_k) wm_k) 2^we_k carries the digit's rounding to a double (d_k < 2^60: 2^-53), the rounding of
        wm_k = fl(exp2l(..)) to a double (2^-53) and one product rounding (2^-53); ldexp is exact in the normal range.
        Together < 3 * 2^-53 (1 + 2^-52) < 2^-51.
      * n additions into the running sum: each 2^-53 of the partial sum, which never exceeds the total: n 2^-53.
      * the division by crt_exact's own rounding to the nearest double: 2^-53.
        First part: 2^-51 + n 2^-53 + 2^-53 + second-order terms < (n + 4) 2^-52.
      * the weight's exponent: log2 w_k = (sum_(j<k) ln q_j - ln_rat) / ln 2 is a long-double sum of k + 1 <= n + 1
        terms, each logl rounded (2^-64 relative of a term of size <= 42), each partial sum rounded (2^-64 of a
        magnitude <= lnQ + |ln_rat|), the division by ln 2, floor (exact) and exp2l (2^-63): an absolute error in
        ln w_k of at most (n + 1)(lnQ + |ln_rat| + 1) 2^-63 with every rounding counted twice over, which is the
        relative error of w_k; doubled once more for the slack between e^x - 1 and x:
        (n + 1)(lnQ + |ln_rat| + 1) 2^-62.
    The bound comes from the formats alone; a device result outside it is a finding, not a reason to widen it."""
    return (n + 4) * 2.0 ** -52 + (n + 1) * (lnQ + abs(ln_rat) + 1.0) * 2.0 ** -62


def lnQ_of(qs):
    return sum(math.log(int(q)) for q in qs)


def ln_rats(qs):
    """ln(ratFactor) of the decode cases: 1, sqrt(Q), Q / e^30, and an everyday factor"""
    lnQ = lnQ_of(qs)
    return [0.0, 0.5 * lnQ, lnQ - 30.0, 37.123456789]


def planted_values(qs):
    """named integers modulo Q = prod(qs), each in [0, Q): the inputs where the kernel's branches part.  (At small n
    several names fall on one integer -- q_0 q_1 = Q = 0 at n = 2, say; every name is kept, so every n has 40.)"""
    qs = [int(q) for q in qs]
    Q = _prod(qs)
    top = _prod(qs[:-1])
    big = 1 << (100 if Q.bit_length() - 3 >= 100 else Q.bit_length() - 3)
    d = (Q >> 48) + 1
    v = {"zero": 0}
    for name, x in (("1", 1), ("5", 5), ("q0", qs[0]), ("q0q1", _prod(qs[:2])), ("top", top), ("big", big),
                    ("third", Q // 3)):
        v["+" + name] = x
        v["-" + name] = -x
    v["Q-top"] = Q - top
    v["half-d"] = Q // 2 - d
    v["half+1+d"] = Q // 2 + 1 + d
    v["half_lo"] = (Q - 1) // 2
    v["half_hi"] = (Q + 1) // 2
    rng = random.Random(0xCC55 + len(qs))
    for i in range(20):
        v["u%02d" % i] = rng.randrange(Q)
    return {k: x % Q for k, x in v.items()}


@functools.lru_cache(maxsize=None)
def prime_sets(m):
    """{(n, kind): primes} for n in NS: kind "60" = n 60-bit primes, kind "mixed" = sizes cycling 60, 60, 48, 36 bits,
    all from the oracle's PrimeGen(bits, m) in its order (the sets of a kind are prefixes of one another)"""
    from oracle import oracle as O
    gens = {b: O.PrimeGen(b, m) for b in (60, 48, 36)}
    nmax = max(NS)
    p60 = [gens[60].next() for _ in range(nmax)]
    mixed, it60 = [], iter(p60)
    for k in range(nmax):
        b = (60, 60, 48, 36)[k % 4]
        mixed.append(next(it60) if b == 60 else gens[b].next())
    out = {}
    for n in NS:
        out[(n, "60")] = tuple(p60[:n])
        out[(n, "mixed")] = tuple(mixed[:n])
    return out


def in_range(exact):
    """the asserted cases: the exact result is a normal double well inside the range (or exactly 0, from the value 0)"""
    a = np.abs(exact)
    return (a >= RANGE_LO) & (a <= RANGE_HI)


def decode_cases(qs, ln_rat):
    """(names, values, exact, asserted) of one decode case: what the device test uploads and what it may skip --
    decided from the exact result alone, never from what the device returns"""
    pv = planted_values(qs)
    names = list(pv)
    vals = [pv[k] for k in names]
    exact = crt_exact(vals, qs, ln_rat)
    keep = in_range(exact) | np.array([v == 0 for v in vals])      # (a name that falls on 0 mod Q: exactly 0.0)
    return names, vals, exact, keep


def expected_skips(n, li):
    """How many of the 40 planted values of a decode case lie outside [2^-1000, 2^1020] after the division, by
    (n, index into ln_rats): none up to 17 primes (Q < 2^1020); from 32 primes on the 10 small values (+-1, +-5,
    +-q0, +-q0q1, +-2^100) at Q/e^30 -- one quarter -- and the 29 values of the size of Q at ratFactor 1 and
    e^37.12, where only the small ones fit a double; at 64 primes and sqrt(Q) everything but 0 is either above
    2^1020 or below 2^-1000."""
    if n < 32:
        return 0
    if li == 2:
        return 10
    if li == 1:
        return 39 if n == 64 else 0
    return 29


# ---------------------------------------------------------------------------------------------------------------
# the residues kernel
# ---------------------------------------------------------------------------------------------------------------
def residues_exact(coef, qs):
    """canonical residues [len(qs), *coef.shape] (uint64) of python-integer coefficients"""
    c = np.asarray(coef).astype(object)
    return np.stack([np.asarray(c % int(q), dtype=object).astype(np.uint64) for q in qs])


RESIDUE_BITS = (60, 60, 48, 36, 30)


@functools.lru_cache(maxsize=None)
def residue_primes(m):
    from oracle import oracle as O
    gens = {b: O.PrimeGen(b, m) for b in set(RESIDUE_BITS)}
    return tuple(gens[b].next() for b in RESIDUE_BITS)


def residue_scalings(qs):
    """signed scalings s (|s| a double) whose constant polynomial round(s) the encode test plants: coefficient 0 is s
    exactly.  Every quotient class of red64 on every prime size, exact negative multiples, and INT64_MIN."""
    q48, q36, q30 = int(qs[2]), int(qs[3]), int(qs[4])
    k36 = (1 << 53) // q36 - 1          # k q < 2^53: a double holds it exactly
    k30 = (1 << 53) // q30 - 1
    mags = [1 << 62, (1 << 63) - 1024, (1 << 60) + (1 << 20), 17 * q48, q48, k36 * q36, 3 * q36, q36,
            k30 * q30, 5 * q30, q30, q36 << 10]
    out = []
    for a in mags:
        out += [a, -a]
    out.append(-(1 << 63))
    return out


LARGE_CASES = ((1024, 3), (65536, 2))


def large_encode_case(m, B):
    """slots in the unit box and the scaling that puts max |unrounded coefficient| at 0.9 * 2^62 (tests/ckks_ref.py's
    double transform decides the scaling; it is an input, not an expectation)"""
    from tests import ckks_ref as R
    rng = np.random.default_rng(m + B)
    v = rng.uniform(-1, 1, size=(B, m // 4)) + 1j * rng.uniform(-1, 1, size=(B, m // 4))
    scaling = 0.9 * 2.0 ** 62 / float(np.max(np.abs(R.embed_unrounded(v, m, 1.0, _reps(m)))))
    return v, scaling


# ---------------------------------------------------------------------------------------------------------------
# the slot maps in longdouble
# ---------------------------------------------------------------------------------------------------------------
_PI = LD("3.14159265358979323846264338327950288419716939937510")


@functools.lru_cache(maxsize=None)
def _zeta(m):
    """(cos, sin)(2 pi j / m), j < m, in longdouble; the angle reduced to the first octant so that every entry is
    good to a few 2^-64"""
    j = np.arange(m, dtype=np.int64)
    o = m // 8
    r = j % (2 * o)                               # position within the quadrant
    fold = r > o
    a = np.where(fold, 2 * o - r, r).astype(LD) * (2 * _PI / LD(m))      # in [0, pi/4]
    c, s = np.cos(a), np.sin(a)
    c, s = np.where(fold, s, c), np.where(fold, c, s)                    # angle in [0, pi/2)
    quad = (j // (2 * o)) % 4
    cc = np.select([quad == 0, quad == 1, quad == 2, quad == 3], [c, -s, -c, s])
    ss = np.select([quad == 0, quad == 1, quad == 2, quad == 3], [s, c, -s, -c])
    return cc, ss


def _reps(m):
    """PAlgebra's T for m = 2^k, p = -1: T[i] = 3^i mod m (tests/test_ckks_slots_host.py holds it to ZmStar)"""
    T, t = [], 1
    for _ in range(m // 4):
        T.append(t)
        t = t * 3 % m
    return np.array(T, dtype=np.int64)


def slot_root(m):
    """j(s): slot s holds f(W^(2j+1)), W = exp(2 pi i/m): 2j + 1 = m - T[m/4-1-s]"""
    T = _reps(m)
    return (m - T[::-1] - 1) // 2


def _edges(m):
    """the first and the last output index s + S k' of every sub-transform of the device's split (H <= 8192)"""
    N = m // 2
    S = max(1, N // 8192)
    return sorted({s for s in range(S)} | {N - S + s for s in range(S)})


def sample_slots(m, count=64, seed=11):
    """slots of a fixed sample: every slot whose root is the first or the last output of a sub-transform (of each
    conjugate pair of outputs one is a slot), and `count` more from a fixed seed; all slots up to N = 2048"""
    N = m // 2
    if N <= 2048:
        return np.arange(N // 2)
    j = slot_root(m)
    edge = set(_edges(m))
    hit = [s for s in range(N // 2) if int(j[s]) in edge or N - 1 - int(j[s]) in edge]
    rnd = np.random.default_rng(seed).choice(N // 2, size=count, replace=False)
    return np.array(sorted(set(hit) | set(int(x) for x in rnd)), dtype=np.int64)


def sample_coeffs(m, count=64, seed=12):
    """coefficient indices of a fixed sample: the first and last of every sub-transform and `count` more"""
    N = m // 2
    if N <= 2048:
        return np.arange(N)
    rnd = np.random.default_rng(seed).choice(N, size=count, replace=False)
    return np.array(sorted(set(_edges(m)) | set(int(x) for x in rnd)), dtype=np.int64)


def embed_ld(f, m, slots=None):
    """canonical embedding from its definition, v[s] = f(zeta^-T[m/4-1-s]) = sum_k f_k zeta^(-T k), in longdouble:
    (re, im), each [B, len(slots)] -- all slots for N <= 2048 (the O(N^2) form), else sample_slots(m), O(N) each"""
    f = np.atleast_2d(np.asarray(f)).astype(LD)
    N = m // 2
    slots = sample_slots(m) if slots is None else np.asarray(slots)
    T = _reps(m)[m // 4 - 1 - slots]
    c, s = _zeta(m)
    k = np.arange(N, dtype=np.int64)
    re = np.empty((f.shape[0], len(slots)), dtype=LD)
    im = np.empty_like(re)
    for i, t in enumerate(T):
        e = (-(int(t) * k)) % m
        re[:, i] = (f * c[e]).sum(axis=1)
        im[:, i] = (f * s[e]).sum(axis=1)
    return re, im


def encode_unrounded_ld(v, m, scaling, nslots=None, coeffs=None):
    """the values CKKS_embedInSlots rounds, from the definition in tests/ckks_ref.py with the FFT written out:
    buf[T>>1] = conj(v), buf[(m-T)>>1] = v, f_k = Re(zeta^-k sum_j buf_j zeta^(-2jk)) scaling/N
        = (scaling/N) sum_i 2 Re(v_(m/4-1-i) zeta^(k T_i))        over the slots given (the first nslots columns of v),
    in longdouble, [B, len(coeffs)] -- all coefficients for N <= 2048, else sample_coeffs(m)"""
    v = np.atleast_2d(np.asarray(v, dtype=np.complex128))
    ns = v.shape[1] if nslots is None else nslots
    N = m // 2
    coeffs = sample_coeffs(m) if coeffs is None else np.asarray(coeffs)
    out = np.zeros((v.shape[0], len(coeffs)), dtype=LD)
    if ns == 0:
        return out
    T = _reps(m)[m // 4 - 1 - np.arange(ns)]          # slot s <-> T[m/4-1-s]
    vr, vi = v[:, :ns].real.astype(LD), v[:, :ns].imag.astype(LD)
    c, s = _zeta(m)
    scale = LD(float(scaling)) / LD(N)
    for i, k in enumerate(coeffs):
        e = (int(k) * T) % m
        out[:, i] = 2 * (vr * c[e] - vi * s[e]).sum(axis=1) * scale
    return out


def fft_abs_bound(N, l1):
    """Worst-case absolute forward error of one output of the device's N-point transforms, l1 = the l1 norm of the
    transform's input:  (8 log2 N + 16) 2^-53 l1.

    Every output is a sum over the inputs of x_n times a product of log2 N twiddles, so |output| <= l1 and the error
    propagates linearly: an error made at one level is carried on by factors of modulus <= 1 (+ their own errors).
    A radix-2 butterfly in doubles (u = 2^-53) with a twiddle correctly rounded from long double (relative error
    mu <= u (1 + 2^-10) per component, so about u in modulus) computes one complex product (four products, two
    additions: relative error gamma_4 of a quantity bounded by sqrt 2 |a| |w|), and one complex addition (u): per
    level the error relative to the running l1 bound grows by
        eta = mu + gamma_4 (sqrt 2 + mu)  ~  u + 4 u * 1.4143  ~  6.7 u   (Higham, Accuracy and Stability, 24.1),
    taken as 8 u.  log2 N levels give 8 log2 N u l1, first order; the second-order remainder at N = 2^16 is
    (128 u)^2 / 2, far below one unit of the 16.  The 16 u cover what is not a butterfly level: the folded load of the
    first log2 S levels as ONE S-term sum per point (S <= 8: S products and S - 1 additions with table twiddles,
    <= (S + 2) u instead of 8 log2 S u, so the levels already counted are not exceeded by more than 2 u), the final
    twist by W^k with its real part (3 u), the multiplication by the scale (u), and crt- or caller-side roundings of
    the inputs to doubles (u), with room to spare."""
    return (8.0 * math.log2(N) + 16.0) * 2.0 ** -53 * np.asarray(l1, dtype=np.float64)
