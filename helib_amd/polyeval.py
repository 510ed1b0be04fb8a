"""Polynomial evaluation on BGV ciphertexts (src/polyEval.cpp) and what the reference builds on it (src/extractDigits.cpp):

  DynamicCtxtPowers   the powers of a ciphertext, formed on demand at depth ceil(log2 e) (:18-29); the class lives in
                      helib_amd.ctxt, where Ctxt.power uses it
  polyEval            a plaintext polynomial (python integers, lowest coefficient first) on an encrypted x (:129-389):
                      baby steps and giant steps, Paterson-Stockmeyer with the depth kept at ceil(log2 deg)
  polyEvalCtxt        an encrypted polynomial on an encrypted x (:60-126)
  buildDigitPolynomial, compute_a_vals, compute_magic_poly     the digit polynomials of src/extractDigits.cpp:28-56,
                      131-214, in python integers
  extractDigits       src/extractDigits.cpp:70-129 for any p (square, cube, or polyEval of the digit polynomial)
  extendExtractDigits src/extractDigits.cpp:225-308

Every leaf of polyEval is simplePolyEval (:223-255), sum_i f_i X^i + f_0 over the baby steps: it goes through
Ctxt.linearCombination, which is the reference's call sequence or, fused, one hx_lin_comb.  Nothing here imports
oracle/."""
import math

from .ckks import LogicError
from .ctxt import Ctxt, DynamicCtxtPowers

__all__ = ["DynamicCtxtPowers", "polyEval", "polyEvalCtxt", "buildDigitPolynomial", "compute_a_vals",
           "compute_magic_poly", "extractDigits", "extendExtractDigits"]


# ---- integer polynomials as lists, lowest coefficient first ----
def _norm(f):
    f = list(f)
    while f and f[-1] == 0:
        f.pop()
    return f


def _deg(f):
    return len(f) - 1


def _coeff(f, i):
    return f[i] if 0 <= i < len(f) else 0


def _set(f, i, v):
    """SetCoeff(f, i, v) -> the normalised polynomial"""
    f = list(f) + [0] * (i + 1 - len(f))
    f[i] = v
    return _norm(f)


def _divrem_monic(a, b):
    """DivRem over the integers by a monic b: a = c b + s with deg s < deg b"""
    if not b or b[-1] != 1:
        raise ValueError("DivRem: the divisor is not monic")
    s, db = list(a), _deg(b)
    c = [0] * max(len(a) - db, 0)
    for i in range(len(s) - 1, db - 1, -1):
        t = s[i]
        if t:
            c[i - db] = t
            for j in range(db + 1):
                s[i - db + j] -= t * b[j]
    return _norm(c), _norm(s[:db])


def _npt(n):
    """NTL::NextPowerOfTwo: the least k with 2^k >= n"""
    return max(n - 1, 0).bit_length()


def _divc(a, b):
    return -(-a // b)


class _Eval:
    """one polyEval call: the switches and the counters its steps share"""

    def __init__(self, x, fused, stats):
        self.x, self.fused, self.stats = x, fused, stats
        if stats is not None:
            stats.setdefault("mults", 0)
            stats.setdefault("powers", set())
            stats.setdefault("leaves", 0)

    def mul(self, a, b):
        a.multiplyBy(b)
        if self.stats is not None:
            self.stats["mults"] += 1

    def empty(self):
        return self.x._emptyLike()

    def simple(self, poly, baby):
        """simplePolyEval (:223-255)"""
        d = _deg(poly)
        if d < 0:
            return self.empty()
        if d > baby.size():
            raise ValueError("BabyStep has not enough powers (required more than deg(poly))")
        P = baby.getPower(1).ptxtSpace
        bal = lambda c: c % P - P if c % P > P // 2 else c % P           # noqa: E731
        terms = [(baby.getPower(i), bal(poly[i])) for i in range(1, d + 1)]
        if self.stats is not None:
            self.stats["leaves"] += 1
        if not terms:
            ret = self.empty()
            ret.addScalar(bal(poly[0]))
            return ret
        return Ctxt.linearCombination(terms, bal(poly[0]), self.fused)

    def paterson(self, poly, k, t, delta, baby, giant):
        """PatersonStockmeyer (:261-307): poly monic of degree k (2t - 1) + delta, t a power of two"""
        if _deg(poly) <= baby.size():
            return self.simple(poly, baby)
        r, q = _norm(poly[:k * t]), _norm(poly[k * t:])
        r = _set(r, _deg(q), _coeff(r, _deg(q)) - 1)                     # r' = r - X^deg(q)
        c, s = _divrem_monic(r, q)                                       # r' = c q + s
        if not (not c or _deg(c) < k - delta):
            raise ValueError("Nonzero c has not degree smaller than k - delta")
        s = _set(s, _deg(q), 1)                                          # s' = s + X^deg(q)
        P = baby.getPower(1).ptxtSpace
        c, s = _norm([v % P for v in c]), _norm([v % P for v in s])
        ret = self.paterson(q, k, t // 2, delta, baby, giant)            # poly = (c + X^(k t)) q + s'
        tmp = self.simple(c, baby)
        tmp += giant.getPower(t)
        self.mul(ret, tmp)
        ret += self.paterson(s, k, t // 2, delta, baby, giant)
        return ret

    def degPowerOfTwo(self, poly, k, baby, giant):
        """degPowerOfTwo (:311-338): k (2^e + 1) > deg(poly) > k (2^e - 1)"""
        if _deg(poly) <= baby.size():
            return self.simple(poly, baby)
        n = 1 << _npt(_deg(poly) // k)
        r, q = _norm(poly[:(n - 1) * k]), _norm(poly[(n - 1) * k:])
        r = _set(r, (n - 1) * k, 1)                                      # monic, degree k (2^e - 1)
        q = _set(q, 0, _coeff(q, 0) - 1)
        ret = self.paterson(r, k, n // 2, 0, baby, giant)
        tmp = self.simple(q, baby)
        i = 1
        while i < n:                                                     # times X^(k (n - 1)) at the least depth
            g = giant.getPower(i)
            if tmp.parts:
                self.mul(tmp, g)
            i *= 2
        ret += tmp
        return ret

    def recursive(self, poly, k, baby, giant):
        """recursivePolyEval (:340-389): poly monic"""
        d = _deg(poly)
        if d <= baby.size():
            return self.simple(poly, baby)
        delta, n = d % k, _divc(d, k)
        t = 1 << _npt(n)
        if n == t:
            return self.degPowerOfTwo(poly, k, baby, giant)
        if n == t - 1 and delta == 0:
            return self.paterson(poly, k, t // 2, delta, baby, giant)
        t //= 2
        u = d - k * (t - 1)                                              # poly = (q - 1) X^u + (X^u + r), deg r < u
        r, q = _norm(poly[:u]), _norm(poly[u:])
        q = _set(q, 0, _coeff(q, 0) - 1)
        r = _set(r, u, 1)
        ret = self.paterson(q, k, t // 2, 0, baby, giant)
        tmp = giant.getPower(u // k).clone()
        if delta != 0:
            self.mul(tmp, baby.getPower(delta))
        self.mul(ret, tmp)
        ret += self.recursive(r, k, baby, giant)
        return ret


def polyEval(x, poly, k=0, fused=None, stats=None):
    """polyEval(ret, ZZX poly, x, k) (src/polyEval.cpp:129-220): -> a new ciphertext holding sum_i poly[i] x^i, the
    plaintext space that of x.  k: the number of baby steps (<= 0: about sqrt(deg / 2), a power of two, with the
    heuristic of :151-158).  fused: how every simplePolyEval runs (Ctxt.linearCombination).  stats: a dict that
    receives "mults" (ciphertext products), "powers" (the set of (name, e) formed, name "baby" or "giant") and "leaves"
    (simplePolyEval calls)."""
    if x.context.ckks:
        raise LogicError("polyEval: BGV only (the reference's simplePolyEval works modulo the plaintext space)")
    ev = _Eval(x, fused, stats)
    poly = _norm([int(c) for c in poly])
    d = _deg(poly)
    if d <= 2:
        if d < 1:
            ret = ev.empty()
            ret.addScalar(_coeff(poly, 0))
            return ret
        return ev.simple(poly, DynamicCtxtPowers(x, d, stats, "baby"))
    if k <= 0:
        kk = int(math.sqrt(d / 2.0))
        k = 1 << _npt(kk)
        if (k == 16 and d > 167) or (k > 16 and k > 1.44 * kk):          # k >> kk: a smaller power of two
            k //= 2
    n = _divc(d, k)
    baby = DynamicCtxtPowers(x, k, stats, "baby")
    x2k = baby.getPower(k)
    if n == 1 << _npt(n):                                                # deg(p) > k (2^e - 1)
        return ev.degPowerOfTwo(poly, k, baby, DynamicCtxtPowers(x2k, n // 2, stats, "giant"))
    # otherwise make poly monic of a degree divisible by k, then recurse
    p = x.ptxtSpace
    top = poly[-1]
    invertible = math.gcd(top % p, p) == 1
    topInv = pow(top % p, -1, p) if invertible else 0
    extra = 0
    if n * k != d or not invertible:                                     # add a term extra * X^(n k)
        top = topInv = 1
        extra = (1 - _coeff(poly, n * k)) % p
        poly = _set(poly, n * k, 1)
    t = _divc(n, 2) if extra == 0 else n
    giant = DynamicCtxtPowers(x2k, t, stats, "giant")
    if top != 1:
        poly = _norm([c * topInv % p for c in poly])
    ret = ev.recursive(poly, k, baby, giant)
    if top != 1:
        ret.multByScalar(top)
    if extra != 0:                                                       # subtract the added term back
        topTerm = giant.getPower(n).clone()
        topTerm.multByScalar(extra)
        ret -= topTerm
    return ret


def polyEvalCtxt(polyCts, x):
    """polyEval(ret, Vec<Ctxt> poly, x) (src/polyEval.cpp:60-126): sum_i polyCts[i] x^i for encrypted coefficients, by
    the powers x^(2^i) and p0(X) + (p1(X) + p2(X) X^d) X^d with every piece split recursively at powers of two"""
    if x.context.ckks:
        raise LogicError("polyEval: BGV only")
    n = len(polyCts)
    if n == 0:
        ret = x.clone()
        ret.clear()
        return ret
    if n == 1:
        return polyCts[0].clone()
    logD = _npt(_divc(n, 3))
    d = 1 << logD
    if not d <= n - 1 < 3 * d:
        raise ValueError("Poly degree not in [d, 3d)")
    powers = [x.clone()]
    for i in range(1, logD + 1):                                         # powers[i] = x^(2^i)
        c = powers[i - 1].clone()
        c.square()
        powers.append(c)

    def rec(cts):
        if len(cts) <= 1:
            if not cts:
                e = x.clone()
                e.clear()
                return e
            return cts[0].clone()
        lg = _npt(len(cts)) - 1
        h = 1 << lg
        tmp = rec(cts[h:])
        ret = rec(cts[:h])
        tmp.multiplyBy(powers[lg])
        ret += tmp
        return ret
    ret = rec(polyCts[d:2 * d])                                          # p1(X)
    if n > 2 * d:                                                        # p2(X)
        tmp = rec(polyCts[2 * d:])
        tmp.multiplyBy(powers[logD])
        ret += tmp
    ret.multiplyBy(powers[logD])                                         # (p1(X) + p2(X) X^d) X^d
    ret += rec(polyCts[:d])                                              # p0(X)
    return ret


# ---- the digit polynomials (src/extractDigits.cpp:28-56, 131-214) ----
def buildDigitPolynomial(p, e):
    """A polynomial of degree p with poly(z0 + p^t z1) = z0 mod p^(t+1) for every t < e and balanced z0
    (src/extractDigits.cpp:28-56): x^p + poly'(x) with poly'(z0) = z0 - z0^p mod p^e interpolated at the p balanced
    residues.  Lowest coefficient first; [] when there is nothing to do (p < 2 or e <= 1)."""
    from . import hostnt
    if p < 2 or e <= 1:
        return []
    p2e = p ** e
    xs = [-(p // 2) + j for j in range(p)]
    ys = [z - pow(z % p2e, p, p2e) for z in xs]
    poly = hostnt.interpolateMod(xs, ys, p, e)
    if _deg(poly) >= p:
        raise RuntimeError("Interpolation error.  Degree too high.")
    return _set(poly, p, 1)


def _mul_trunc(a, b, n, mod):
    out = [0] * n
    for i, x in enumerate(a[:n]):
        if x:
            for j, y in enumerate(b[:n - i]):
                out[i + j] = (out[i + j] + x * y) % mod
    return out


def compute_a_vals(p, e):
    """a[m] = a(m) / m! of Chen and Han for m = p .. (e-1)(p-1)+1 (src/extractDigits.cpp:131-167): the coefficients of
    p (x+1)^p / ((x+1)^p - x^p) modulo p^(2e), each divided by m! with the common power of p taken out first; a list of
    length (e-1)(p-1)+2 whose entries below p are 0"""
    pe, p2e = p ** e, p ** (2 * e)
    n = (e - 1) * (p - 1) + 2
    xp1 = [math.comb(p, i) % p2e for i in range(p + 1)]                  # (x + 1)^p
    den = list(xp1)
    den[p] = (den[p] - 1) % p2e                                          # (x + 1)^p - x^p: constant term 1
    den = (den + [0] * n)[:n]
    inv = [0] * n                                                        # InvTrunc
    inv[0] = pow(den[0], -1, p2e)
    for i in range(1, n):
        inv[i] = -inv[0] * sum(den[j] * inv[i - j] for j in range(1, i + 1)) % p2e
    poly = [c * p % p2e for c in _mul_trunc(xp1, inv, n, p2e)]
    a = [0] * n
    m_fac = 1
    for m in range(2, p):
        m_fac = m_fac * m % p2e
    for m in range(p, n):
        m_fac = m_fac * m % p2e
        c = poly[m]
        d = math.gcd(m_fac, p2e)
        if d == 0 or d > pe or c % d != 0:
            raise RuntimeError("cannot divide")
        a[m] = (c // d) % pe * pow((m_fac // d) % pe, -1, pe) % pe
    return a


def compute_magic_poly(p, e):
    """Chen and Han's polynomial G with G(x) = (x mod p) modulo p^e, (x mod p) in [0, 1] for p = 2 and balanced
    otherwise (src/extractDigits.cpp:169-214); coefficients in [0, p^e), lowest first"""
    a = compute_a_vals(p, e)
    pe = p ** e
    n = (e - 1) * (p - 1) + 2

    def times_x_minus(f, m):                                             # f (X - m)
        out = [0] * (len(f) + 1)
        for i, c in enumerate(f):
            out[i + 1] = (out[i + 1] + c) % pe
            out[i] = (out[i] - m * c) % pe
        return out
    poly, term = [0], [1]
    for m in range(p):
        term = times_x_minus(term, m)
    for m in range(p, n):
        poly = [(_coeff(poly, i) + _coeff(term, i) * a[m]) % pe for i in range(max(len(poly), len(term)))]
        term = times_x_minus(term, m)
    if p % 2 == 1:                                                       # poly(X + (p - 1) / 2)
        h = (p - 1) // 2
        poly2 = [0]
        for c in reversed(poly):
            poly2 = times_x_minus(poly2, -h)
            poly2[0] = (poly2[0] + c) % pe
        poly = poly2
    out = [(-c) % pe for c in poly] + [0] * max(0, 2 - len(poly))
    out[1] = (out[1] + 1) % pe                                           # X - poly
    return _norm(out)


# ---- digit extraction ----
def _raise_to_p(d, p, x2p, fused):
    """"in spirit" d = d^p: square, cube, or the digit polynomial"""
    if p == 2:
        d.square()
    elif p == 3:
        d.cube()
    else:
        r = polyEval(d, x2p, fused=fused)
        r.lnNoise  # noqa: B018 -- complete r's deferred noise updates on r itself before d takes its fields over
        d.__dict__.update(r.__dict__)


def extractDigits(ea, ct, r=0, fused=None):
    """extractDigits (src/extractDigits.cpp:70-129) for any p: the slots of ct hold integers mod p^rr, rr =
    ct.effectiveR(); -> digits, a list of r ciphertexts (r <= 0 or r > rr: rr), digits[j] with plaintext space
    p^(rr - j) and, in every slot, a value congruent mod p to digit j of the slot's expansion in base p (digits in
    [0, p) for p = 2, balanced otherwise).  For p <= 3 the steps are those of helib_amd.bgv_pr.extractDigits; for
    p > 3 digits[j] goes through polyEval of buildDigitPolynomial(p, r).  fused: Ctxt.subDivideByP's and
    Ctxt.linearCombination's."""
    if ct.context is not ea.cc:
        raise LogicError("extractDigits: the ciphertext belongs to another context than the EncryptedArray")
    if ct.context.ckks:
        raise LogicError("extractDigits: BGV only")
    p = ea.p
    rr = ct.effectiveR()
    if r <= 0 or r > rr:
        r = rr
    x2p = buildDigitPolynomial(p, r) if p > 3 else None
    digits = []
    for i in range(r):
        tmp = ct.clone()
        for j in range(i):
            _raise_to_p(digits[j], p, x2p, fused)
            tmp.subDivideByP(digits[j], fused)
        digits.append(tmp)
    return digits


def extendExtractDigits(ea, ct, r, e, fused=None):
    """extendExtractDigits (src/extractDigits.cpp:225-308): the slots of ct hold integers mod p^(r+e); -> digits, r
    ciphertexts, digits[j] holding digit j of every slot itself (not only a value congruent to it mod p) in the space
    p^(e+r-j): round i forms digits0[i] as extractDigits does and digits[i] = G_(e+r-i)(digits0[i]) with Chen and
    Han's polynomial, and subtracts whichever of digits[j], digits0[j]^p has the larger capacity."""
    if ct.context is not ea.cc:
        raise LogicError("extendExtractDigits: the ciphertext belongs to another context than the EncryptedArray")
    if ct.context.ckks:
        raise LogicError("extendExtractDigits: BGV only")
    if r < 1 or e < 1:
        raise ValueError("extendExtractDigits: r and e are at least 1")
    p = ea.p
    x2p = buildDigitPolynomial(p, r) if p > 3 else None
    G = [compute_magic_poly(p, e + r - i) for i in range(r)]
    digits, digits0 = [], []
    for i in range(r):
        tmp = ct.clone()
        for j in range(i):
            if digits[j].capacity() >= digits0[j].capacity():            # digits[j] is the better one: use it as it is
                tmp.subDivideByP(digits[j], fused)
            else:
                _raise_to_p(digits0[j], p, x2p, fused)
                tmp.subDivideByP(digits0[j], fused)
        digits0.append(tmp)
        digits.append(polyEval(tmp, G[i], fused=fused))
    return digits
