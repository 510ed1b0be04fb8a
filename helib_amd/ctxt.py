"""Host-side mirror of the reference's ciphertext bookkeeping for this path (BGV):

  ChainContext  -- Context::buildModChain (src/Context.cpp:728-1073): small / ctxt / special
                   primes, digits, and ModuliSizes (src/primeChain.cpp:68-335)
  Ctxt          -- the orchestration rows of SURVEY.md 8(a): modUpToSet / modDownToSet /
                   bringToSet (src/Ctxt.cpp:346-562), dropSmallAndSpecialPrimes (:589-662),
                   tensorProduct bookkeeping (:1563-1608), computeIntervalForMul (:1610-1656),
                   multLowLvl / multiplyBy (:1681-1774), reLinearize / keySwitchPart (:720-842),
                   addCtxt for equal prime sets (:1540-1553)

The polynomial work is delegated to a backend (`ops`): on the GPU that is helib_amd.capi
(DoubleCRT parts resident in HBM, possibly a batch of independent ciphertexts sharing this
bookkeeping).  The class itself is pure control flow + floating-point noise estimates, exactly the
part SURVEY.md keeps on the host (risk R3).  Added noise follows the reference's default
branches when the backend can measure it (Ctxt.measure, power-of-two m on the GPU): the mod-switch
noise is sum_parts embeddingLargestCoeff(delta/diffProd) * skBound^power (src/Ctxt.cpp:466-530)
and the key-switch noise is W.noiseBound * sum_digits embeddingLargestCoeff(digit)
(src/DoubleCRT.cpp:530-545, src/Ctxt.cpp:828-841), both norms evaluated on the device (SURVEY
row N1).  A batch of ciphertexts behind one Ctxt shares one bound: the maximum over the batch.
Otherwise (general m, or Ctxt.measure = False) the reference's own alternative branches are used:
modSwitchAddedNoiseBound() (src/Ctxt.cpp:546-559 `#else`) and noiseBoundForUniform per digit
(src/DoubleCRT.cpp:520-529 `#if 0`).  Noise bounds are kept as natural logarithms (NTL::xdouble
in the reference) -- only their logs are ever compared.
"""
import math
from functools import reduce
from helib_amd import timing

from . import hostnt

HELIB_SP_NBITS = 60
LN2 = math.log(2.0)


def phi(m):
    r, x, p = m, m, 2
    while p * p <= x:
        if x % p == 0:
            while x % p == 0:
                x //= p
            r -= r // p
        p += 1
    if x > 1:
        r -= r // x
    return r


def _divc(a, b):
    return -(-a // b)


def handle_powers(handle):
    """(powerOfS, powerOfX) of a part key: "1", "s", "s2", ("s", k) = s(X^k), ("s^", r) = s^r,
    ("s^", r, k) = s^r(X^k)  (SKHandle, include/helib/Ctxt.h:74-170)."""
    if handle == "1":
        return 0, 1
    if handle == "s":
        return 1, 1
    if handle == "s2":
        return 2, 1
    if handle[0] == "s":
        return 1, int(handle[1])
    return int(handle[1]), (int(handle[2]) if len(handle) > 2 else 1)


def handle_of(powerOfS, powerOfX=1):
    if powerOfS == 0:
        return "1"
    if powerOfX == 1:
        return {1: "s", 2: "s2"}.get(powerOfS, ("s^", powerOfS))
    return ("s", powerOfX) if powerOfS == 1 else ("s^", powerOfS, powerOfX)


def handle_mul(h1, h2):
    """SKHandle::mul (include/helib/Ctxt.h:140-165): powers of s add; the automorphism amounts must
    agree unless one side is the constant handle."""
    (s1, x1), (s2, x2) = handle_powers(h1), handle_powers(h2)
    if s1 == 0:
        return h2
    if s2 == 0:
        return h1
    if x1 != x2:
        raise ValueError("cannot multiply parts under different automorphisms")
    return handle_of(s1 + s2, x1)


def _powerOfS(handle):
    return handle_powers(handle)[0]


def polyNormBnd(m):
    """calcPolyNormBnd (src/PAlgebra.cpp:215-434): the ring constant c_M.  1 for a power of two,
    2 cot(pi/(2u))/u when the odd part of m is a power of one prime u; otherwise, with m replaced by
    the radical of its odd part, the maximal absolute row sum of the inverse of the Vandermonde matrix
    of the primitive m-th roots x_j: row i of column j is q_i(x_j) / Phi_m'(x_j) with the Horner
    prefixes q_0 = 1, q_i = q_(i-1) x_j + a_(n-i) of Phi_m (:360-372).  |Phi_m'(x_j)| = prod_i |x_i -
    x_j| is taken as exp of a sum of logarithms (the reference keeps a frexp-normalised running
    product, :300-357); the sums over i for all j at once are one cyclic correlation."""
    import numpy as np
    while m % 2 == 0:
        m //= 2
    if m == 1:
        return 1.0
    fac, r, d = [], m, 3
    while r > 1:
        if r % d == 0:
            fac.append(d)
            while r % d == 0:
                r //= d
        d += 2
    if len(fac) == 1:
        u = fac[0]
        return 2.0 / math.tan(math.pi / (2.0 * u)) / u
    m = 1
    for u in fac:
        m *= u
    phi_coef = np.array(hostnt.phimx(m)[:-1], dtype=np.float64)      # a_0 .. a_(n-1): without the leading 1
    n = len(phi_coef)
    res = np.array([i for i in range(1, m) if math.gcd(i, m) == 1])
    assert len(res) == n
    k = np.arange(m, dtype=np.longdouble)
    x = (np.cos(2 * np.pi * k / m)[res] + 1j * np.sin(2 * np.pi * k / m)[res]).astype(np.complex128)
    # ln |Phi'(x_j)| = sum over units i != j of ln(2 sin(pi |i - j| / m)): correlation of the unit
    # indicator with the table of logarithms (dist 0 counts as 1, as dist_tab[0] = 1 does)
    logd = np.zeros(m)
    logd[1:] = np.log(2.0 * np.sin(np.pi * k[1:] / m).astype(np.float64))
    ind = np.zeros(m)
    ind[res] = 1.0
    corr = np.fft.irfft(np.fft.rfft(logd) * np.conj(np.fft.rfft(ind)), m)   # corr[t] = sum_s ind[s] logd[s+t]
    # sum_i logd[(res_i - res_j) mod m] = sum_s ind[s] logd[(s - res_j) mod m] = corr[-res_j]
    inv_prod = np.exp(-corr[(-res) % m])
    norm_col = np.empty(n)
    q = np.ones(n, dtype=np.complex128)
    norm_col[0] = inv_prod.sum()
    for i in range(1, n):
        q = q * x + phi_coef[n - i]
        norm_col[i] = float(np.dot(np.abs(q), inv_prod))
    return float(norm_col.max())


def _ln(x):
    return math.log(x) if x > 0 else -math.inf


def logaddexp(a, b):
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    hi, lo = (a, b) if a >= b else (b, a)
    return hi + math.log1p(math.exp(lo - hi))


class ModuliSizes:
    """src/primeChain.cpp:68-335"""

    def __init__(self, context):
        self.iFFT_cost = 0 if context.pow2 else 20
        sizes = [(0.0, frozenset())]
        for i in context.smallPrimes:
            sq = math.log(context.primes[i])
            sizes += [(s + sq, st | {i}) for s, st in sizes]
        base = list(sizes)
        interval, isz = set(), 0.0
        for i in context.ctxtPrimes:
            interval.add(i)
            isz += math.log(context.primes[i])
            fs = frozenset(interval)
            sizes += [(s + isz, st | fs) for s, st in base]
        sizes.sort(key=lambda e: (e[0], sorted(e[1])))
        self.sizes = sizes
        self._keys = [s for s, _ in sizes]

    def _cost(self, frm, to):
        if self.iFFT_cost == 0:
            return 100 * len(to - frm)
        return 100 * len(to - frm) + self.iFFT_cost * len(frm - to)

    def getSet4Size(self, low, high, from1, from2=None, reverse=False):
        import bisect
        from1 = frozenset(from1)
        from2 = frozenset(from2) if from2 is not None else None
        cost = (lambda s: self._cost(from1, s)) if from2 is None else \
               (lambda s: self._cost(from1, s) + self._cost(from2, s))
        idx = bisect.bisect_left(self._keys, low)
        best, best_cost = -1, None
        ii = idx
        n = len(self.sizes)
        while ii < n and self.sizes[ii][0] <= high:
            c = cost(self.sizes[ii][1])
            if best_cost is None or c <= best_cost:
                best, best_cost = ii, c
            ii += 1
        w = "window1" if from2 is None else "window2"         # src/primeChain.cpp:207-208, 288-289
        timing.STATS_UPDATE(w + "-out", best == -1)
        timing.STATS_UPDATE(w + "-nchoices", ii - idx)
        if best == -1:
            if reverse:
                if ii < n:
                    ub = self.sizes[ii][0] + LN2
                    i = ii
                    while i < n and self.sizes[i][0] <= ub:
                        c = cost(self.sizes[i][1])
                        if best_cost is None or c < best_cost:
                            best, best_cost = i, c
                        i += 1
            elif idx > 0:
                lb = self.sizes[idx - 1][0] - LN2
                i = idx - 1
                while i >= 0 and self.sizes[i][0] >= lb:
                    c = cost(self.sizes[i][1])
                    if best_cost is None or c < best_cost:
                        best, best_cost = i, c
                    i -= 1
        if best == -1:
            return frozenset()
        return self.sizes[best][1]


MIN_SK_HWT = 120     # include/helib/Context.h:34


def lweEstimateSecurity(n, log2AlphaInv, hwt):
    """src/Context.cpp:34-72: security ~ slope * n / log2(1/alpha) + const, slope and constant interpolated
    between the fitted Hamming weights 120, 150, ..., 450 (dense keys: 3.8, -20); never negative"""
    if hwt < 0 or 0 < hwt < MIN_SK_HWT:
        return 0.0
    hw = [120, 150, 180, 210, 240, 270, 300, 330, 360, 390, 420, 450]
    sl = [2.4, 2.67, 2.83, 3.0, 3.1, 3.3, 3.3, 3.35, 3.4, 3.45, 3.5, 3.55]
    cn = [19, 13, 10, 6, 3, 1, -3, -4, -5, -7, -10, -12]
    if hwt == 0:
        slope, const = 3.8, -20.0
    else:
        i = (hwt - 120) // 30
        if i < len(hw) - 1:
            a = (hwt - hw[i]) / (hw[i + 1] - hw[i])
            slope, const = sl[i] + a * (sl[i + 1] - sl[i]), cn[i] + a * (cn[i + 1] - cn[i])
        else:
            slope, const = sl[-1], float(cn[-1])
    return max(0.0, slope * n / log2AlphaInv + const)


BOOT_DFLT_SK_HWT = 120     # include/helib/Context.h:33-35 (MIN_SK_HWT): the default Hamming weight of a bootstrappable secret key


def _compute_fudge(p2ePrime, p2e):
    """compute_fudge (src/recryption.cpp:155-198): the v coefficients are not quite uniform"""
    eps = 0.0
    if p2ePrime > 1:
        eps = 1.0 / (float(p2ePrime) * float(p2ePrime)) if p2ePrime % 2 == 0 else 1.0 / float(p2e)
    return 1.0 + eps


def setAE(context):
    """RecryptData::setAE (src/recryption.cpp:200-256) -> (e, ePrime): the pair with the smallest e - e' such that
    p^e >= 2 (fudge p^e' + 2 p^r + 2) boundForRecryption, p^e + 1 < 2^30."""
    coeff_bound = context.boundForRecryption()
    p, r = context.p, context.r
    frstTerm = 2 * p ** r + 2
    e_bnd, p2e_bnd = 0, 1
    while p2e_bnd <= ((1 << 30) - 2) // p:
        e_bnd += 1
        p2e_bnd *= p
    ePrime, e = 0, r + 1
    while e <= e_bnd and p ** e < frstTerm * coeff_bound * 2:
        e += 1
    if e > e_bnd:
        raise RuntimeError("setAE: cannot find suitable e")
    ePrimeTry = 1
    while ePrimeTry <= e_bnd:
        p2ePrimeTry = p ** ePrimeTry
        eTry = max(r + 1, ePrimeTry + 1)
        while eTry <= e_bnd and eTry - ePrimeTry < e - ePrime:
            p2eTry = p ** eTry
            if p2eTry >= (p2ePrimeTry * _compute_fudge(p2ePrimeTry, p2eTry) + frstTerm) * coeff_bound * 2:
                break
            eTry += 1
        if eTry <= e_bnd and eTry - ePrimeTry < e - ePrime:
            e, ePrime = eTry, ePrimeTry
        ePrimeTry += 1
    return e, ePrime


class ChainContext:
    """ContextBuilder<BGV>().m(m).p(p).r(r).bits(bits).c(c) -> buildModChain; with ckks=True
    ContextBuilder<CKKS>().m(m).precision(r).bits(bits).c(c): p = -1, plaintext space 1, r = the
    precision in bits (include/helib/Context.h:1040-1130).  bootstrappable=True is .bootstrappable(true)
    (Context::buildModChain's willBeBootstrappable, src/Context.cpp:1037-1073; ignored for CKKS): skHwt = 0 becomes
    BOOT_DFLT_SK_HWT, setAE fixes e and ePrime, and the special primes are sized for the plaintext space
    p^(r + e - e') of the encrypted recryption key."""

    def __init__(self, m, p, r=1, bits=300, c=3, stdev=3.2, scale=10.0, skHwt=0, resolution=3,
                 bitsInSpecialPrimes=0, ckks=False, bootstrappable=False):
        self.ckks = bool(ckks)
        self.bootstrappable = bool(bootstrappable) and not self.ckks
        self.e = self.ePrime = 0
        if self.ckks:
            p = -1
        self.m, self.p, self.r = m, p, r
        self.ptxtSpace = 1 if self.ckks else p ** r
        self.phim = phi(m)
        self.pow2 = (m & (m - 1)) == 0
        self.stdev, self.scale, self.hwt = stdev, scale, skHwt
        if bits <= 0:      # Context::buildModChain (src/Context.cpp:1044-1046): InvalidArgument
            raise ValueError("Cannot initialise modulus chain with nBits < 1")
        if skHwt < 0:
            raise ValueError("invalid skHwt parameter")
        if skHwt == 0 and self.bootstrappable:     # src/Context.cpp:1054-1058
            self.hwt = BOOT_DFLT_SK_HWT
        self.primes = []
        self.smallPrimes, self.ctxtPrimes, self.specialPrimes = [], [], []
        pSize = self._ctxtPrimeSize(bits)
        self._addSmallPrimes(resolution, pSize)
        self._addCtxtPrimes(bits, pSize)
        self._addSpecialPrimes(c, bitsInSpecialPrimes)
        self.modSizes = ModuliSizes(self)

    # ---- size and security of the chain (include/helib/Context.h:857-889, src/Context.cpp:34-72) ----
    def bitSizeOfQ(self):
        """ceil(log2 of the product of the ctxt and special primes)"""
        return int(math.ceil(self.logOfProduct(list(self.ctxtPrimes) + list(self.specialPrimes)) / LN2))

    def securityLevel(self):
        """Context::securityLevel: lweEstimateSecurity(phi(m), log2(Q / stdev'), hwt) -- the reference's
        affine fits to the LWE estimator, by Hamming weight of the secret key (0 = dense)."""
        s = self.stdev if self.pow2 else self.stdev * math.sqrt(self.m)
        log2AlphaInv = (self.logOfProduct(list(self.ctxtPrimes) + list(self.specialPrimes)) - math.log(s)) / LN2
        return lweEstimateSecurity(self.phim, log2AlphaInv, self.hwt)

    # ---- chain construction (src/Context.cpp:728-1035) ----
    @staticmethod
    def _bit_loss():
        return -math.log1p(-1.0 / (1 << hostnt.PrimeGen.B)) / LN2

    def _ctxtPrimeSize(self, nBits):
        bit_loss = self._bit_loss()
        nPrimes = int(math.ceil(nBits / (HELIB_SP_NBITS - bit_loss)))
        t = HELIB_SP_NBITS
        while 10 * (t - 1) >= 9 * HELIB_SP_NBITS and (t - 1) >= 30 and \
                ((t - 1) - bit_loss) * nPrimes >= nBits:
            t -= 1
        return t

    def _add(self, q, where):
        assert q not in self.primes, "Prime q is already in the prime chain"
        self.primes.append(q)
        where.append(len(self.primes) - 1)

    def _addSmallPrimes(self, resolution, cpSize):
        if resolution < 1 or resolution > 10:
            resolution = 3
        sizes = []
        if cpSize >= 54:
            smallest = _divc(2 * cpSize, 3)
        elif cpSize >= 45:
            smallest = _divc(7 * cpSize, 10)
        else:
            smallest = _divc(11 * cpSize, 15)
            sizes.append(smallest)
        sizes += [smallest, smallest]
        delta = resolution
        while cpSize - delta > smallest:
            sizes.append(cpSize - delta)
            delta *= 2
        if cpSize - 3 * resolution > smallest:
            sizes.append(cpSize - 3 * resolution)
        if resolution == 1 and cpSize - 11 > smallest:
            sizes.append(cpSize - 11)
        sizes.sort()
        last, gen = 0, None
        for sz in sizes:
            if sz != last:
                gen = hostnt.PrimeGen(sz, self.m)
            self._add(gen.next(), self.smallPrimes)
            last = sz

    def _addCtxtPrimes(self, nBits, targetSize):
        gen = hostnt.PrimeGen(targetSize, self.m)
        bitlen = 0.0
        while bitlen < nBits - 0.5:
            q = gen.next()
            self._add(q, self.ctxtPrimes)
            bitlen += math.log2(q)

    def _addSpecialPrimes(self, nDgts, bitsInSpecialPrimes):
        n = len(self.ctxtPrimes)
        nDgts = max(1, min(nDgts, n))
        digits = []
        if nDgts > 1:
            remaining = list(self.ctxtPrimes)
            for dgt in range(nDgts - 1):
                card = _divc(len(remaining), nDgts - dgt)
                digits.append(remaining[:card])
                remaining = remaining[card:]
            if remaining:
                digits.append(remaining)
        else:
            digits = [list(self.ctxtPrimes)]
        self.digits = digits
        maxDigitLog = max(self.logOfProduct(d) for d in digits)
        nDgts = len(digits)
        if bitsInSpecialPrimes:
            nBits = bitsInSpecialPrimes
        else:
            h = self.phim / 2.0 if self.hwt == 0 else self.hwt
            log_phim = max(math.log(self.phim), 1.0)
            p2e = self.ptxtSpace
            if self.bootstrappable:   # bigger p^e for bootstrapping (src/Context.cpp:884-894)
                self.e, self.ePrime = setAE(self)
                p2e *= self.p ** (self.e - self.ePrime)
            if self.ckks:   # a smaller noise estimate, to protect precision (src/Context.cpp:957-965)
                nBits = (maxDigitLog + math.log(self.stdev) + math.log(nDgts) - 0.5 * math.log(h)) / LN2
            elif self.pow2:
                nBits = (maxDigitLog + math.log(p2e) + math.log(self.stdev) + 0.5 * math.log(12.0) +
                         math.log(nDgts) - 0.5 * math.log(log_phim) - 2 * math.log(self.p) -
                         math.log(h)) / LN2
            else:
                nBits = (maxDigitLog + math.log(self.m) + math.log(p2e) + math.log(self.stdev) +
                         0.5 * math.log(12.0) + math.log(nDgts) - 0.5 * log_phim -
                         0.5 * math.log(log_phim) - 2 * math.log(self.p) - math.log(h)) / LN2
        nBits = max(nBits, 1.0)
        bit_loss = self._bit_loss()
        nPrimes = int(math.ceil(nBits / (HELIB_SP_NBITS - bit_loss)))
        t = HELIB_SP_NBITS
        while (t - 1) >= 0.55 * HELIB_SP_NBITS and (t - 1) >= 30 and \
                ((t - 1) - bit_loss) * nPrimes >= nBits:
            t -= 1
        gen = hostnt.PrimeGen(t, self.m)
        while nPrimes > 0:
            q = gen.next()
            if q in self.primes:
                continue
            self._add(q, self.specialPrimes)
            nPrimes -= 1

    # ---- recryption parameters (include/helib/Context.h:616-638) ----
    def stdDevForRecryption(self):
        """Context::stdDevForRecryption: sqrt(phi(m) / m * skHwt * 2^k / 3) / 2, k the number of prime factors of m
        (PAlgebra::getNFactors, src/PAlgebra.cpp:513-515)"""
        k, n, f = 0, self.m, 2
        while f * f <= n:
            if n % f == 0:
                k += 1
                while n % f == 0:
                    n //= f
            f += 1
        k += 1 if n > 1 else 0
        return math.sqrt(self.phim / float(self.m) * float(self.hwt) * float(1 << k) / 3.0) * 0.5

    def boundForRecryption(self):
        """Context::boundForRecryption: a high-probability bound on |w0 + w1 s| in the powerful basis"""
        return 0.5 + self.scale * self.stdDevForRecryption()

    # ---- helpers ----
    def logOfPrime(self, i):
        return math.log(self.primes[i])

    def logOfProduct(self, s):
        return sum(math.log(self.primes[i]) for i in s)

    def productOfPrimes(self, s):
        return reduce(lambda a, b: a * b, (self.primes[i] for i in s), 1)

    def noiseBoundForUniform(self, magBound, degBound):
        return self.scale * math.sqrt(degBound / 3.0) * magBound

    def encodeRoundingError(self):
        """EncryptedArrayCx::encodeRoundingError (include/helib/EncryptedArray.h:1287-1297)"""
        return self.noiseBoundForUniform(0.5, self.phim)

    def encodeScalingFactor(self, precision=-1, roundErr=-1.0):
        """EncryptedArrayCx::encodeScalingFactor (include/helib/EncryptedArray.h:1299-1312): the factor CKKS
        plaintexts are scaled by before rounding -- ceil(precision * roundErr) rounded up to a power of two, with
        precision defaulting to 2^r of ContextBuilder<CKKS>::precision(r).  (m = 65536: 2^11 at precision(1),
        2^30 at precision(20).)"""
        if precision <= 0:
            precision = 1 << self.r
        if roundErr < 0:
            roundErr = self.encodeRoundingError()
        f = int(math.ceil(precision * roundErr))
        return 1 << max(f - 1, 0).bit_length()       # NTL::NextPowerOfTwo

    def noiseBoundForMod(self, modulus, degBound):
        var = modulus * modulus / 12.0 + (1.0 / 6.0 if modulus % 2 == 0 else 0.0)
        return self.scale * math.sqrt(degBound * var)

    # sample*Bounded return values (src/sample.cpp:260-267, 342-396, 445-463)
    def skBound(self):
        if self.hwt > 0:
            return math.sqrt(self.hwt * math.log(self.phim))
        return math.sqrt(self.phim * math.log(self.phim) / 2.0)

    def gaussBound(self):
        eff = math.sqrt(self.phim * math.log(self.phim)) if self.pow2 else \
            math.sqrt(self.m * math.log(self.phim))
        st = self.stdev if self.pow2 else self.stdev * math.sqrt(self.m)
        return st * eff

    def freshNoiseBound(self):
        """noiseBound of PubKey::Encrypt output (src/keys.cpp:395-475)."""
        p = self.ptxtSpace
        e = self.gaussBound() * p
        pk_noise = e                                   # RLWE1: bound *= p
        r_bound = math.sqrt(self.phim * math.log(self.phim) / 2.0)
        return r_bound * pk_noise + e + e * self.skBound() + self.noiseBoundForMod(p, self.phim)


class Ctxt:
    """BGV ciphertext: parts keyed by secret-key handle ("1", "s", "s2")."""
    safety = LN2  # src/Ctxt.cpp:39
    measure = True  # measured added noise (the reference's default) when the backend supports it
    lazyTensor = True  # multiplyBy leaves the tensor product to the mod-switch / key-switch kernels (tests A/B this)

    def __init__(self, context, ops, ksw=None, ksw_ptxtSpace=None, ksw_noise=None):
        self.context, self.ops = context, ops
        self._meas = bool(Ctxt.measure and hasattr(ops, "supportsNorms") and ops.supportsNorms(context.m))
        self._ln = -math.inf
        self._pending = []     # deferred noise updates waiting for norms still on the device
        self.ksw_auto = {}     # k -> key-switching matrix from s(X^k) to s (PubKey::getKeySWmatrix)
        self.ksw_pow = {}      # r -> key-switching matrix from s^r to s, r >= 3 (r = 2 is self.ksw)
        self.ksw_map = None    # PubKey::keySwitchMap: k -> first step n on the way to X -> X^k (0: none)
        self.parts = {}
        # multiplyBy only (as the C++ host's Ctxt::pendingTensor): the tensor product's bookkeeping is done, its
        # data not yet -- the four operand parts wait here while `parts` holds the three product handles with no
        # storage; the mod-switch or the key switch that follows forms the product inside its own kernels
        # (ops.tensorBringToSet / ops.mulRelin), anything else calls _materializeTensor() first
        self._pendT = None
        self._like = None      # a part this ciphertext once held: the shape (batch, device) of a part it is yet to gain
        self.primeSet = frozenset()
        self.ptxtSpace = context.ptxtSpace
        self.intFactor = 1
        # CKKS (src/Ctxt.h: ptxtMag, ratFactor): |plaintext| bound and ln of the scaling factor
        self.ptxtMag, self.lnRatFactor = 1.0, 0.0
        self.ksw, self.ksw_ptxtSpace = ksw, ksw_ptxtSpace or context.ptxtSpace
        self.ksw_lnNoise = ksw_noise if ksw_noise is not None else \
            math.log(context.gaussBound() * context.ptxtSpace)

    @classmethod
    def fresh(cls, context, ops, c0, c1, ksw=None, **kw):
        c = cls(context, ops, ksw, **kw)
        c.parts = {"1": c0, "s": c1}
        c.primeSet = frozenset(context.ctxtPrimes)
        c.lnNoise = math.log(context.freshNoiseBound())
        return c

    def clear(self):
        """Ctxt::clear (include/helib/Ctxt.h:1347-1354): an empty ciphertext on the ctxt primes"""
        like = self._pendT[0] if self._pendT is not None else next(iter(self.parts.values()), None)
        if like is not None:
            self._like = like
        self._pending, self._pendT = [], None
        self.parts = {}
        self.primeSet = frozenset(self.context.ctxtPrimes)
        self._ln = -math.inf
        self.intFactor = 1
        self.ptxtMag, self.lnRatFactor = 1.0, 0.0

    def clone(self):
        self._materializeTensor()
        c = Ctxt(self.context, self.ops, self.ksw, self.ksw_ptxtSpace, self.ksw_lnNoise)
        c.parts = {h: p.copy() for h, p in self.parts.items()}
        c.primeSet, c.ptxtSpace = self.primeSet, self.ptxtSpace
        c.lnNoise, c.intFactor = self.lnNoise, self.intFactor
        c.ptxtMag, c.lnRatFactor = self.ptxtMag, self.lnRatFactor
        c.ksw_auto = self.ksw_auto
        c.ksw_pow = self.ksw_pow
        c.ksw_map = self.ksw_map
        c._like = self._like
        return c

    def assign(self, other):
        """*this = other for a ciphertext of the same context and keys: this object takes over other's parts and
        bookkeeping (other must not be used afterwards); other's deferred noise updates are completed first, since
        they are bound to it"""
        other.lnNoise  # noqa: B018
        self.__dict__.update(other.__dict__)
        return self

    def _emptyLike(self):
        """Ctxt tmp(pubKey, ptxtSpace): an empty ciphertext under this one's keys, in its plaintext space"""
        c = Ctxt(self.context, self.ops, self.ksw, self.ksw_ptxtSpace, self.ksw_lnNoise)
        c.ptxtSpace = self.ptxtSpace
        c.ksw_auto, c.ksw_pow, c.ksw_map = self.ksw_auto, self.ksw_pow, self.ksw_map
        c._like = self._pendT[0] if self._pendT is not None else next(iter(self.parts.values()), self._like)
        c.primeSet = frozenset(self.context.ctxtPrimes)
        return c

    # ---- noise estimate: ln(noiseBound) ----
    # Measured norms are read back lazily: an operation enqueues its kernels, registers how the
    # norms will enter the estimate, and returns; the estimate is completed (waiting only for the
    # norm kernels, hx_norms_flush) when somebody reads it -- normally the next prime-set
    # decision, by which time more work is already queued behind on the GPU.
    @property
    def lnNoise(self):
        if self._pending:
            if hasattr(self.ops, "normsFlush") and self.parts:
                some = self._pendT[0] if self._pendT is not None else next(iter(self.parts.values()))
                self.ops.normsFlush(some)
            todo, self._pending = self._pending, []
            for fn in todo:
                fn()
        return self._ln

    @lnNoise.setter
    def lnNoise(self, v):
        if self._pending:
            self.lnNoise  # noqa: B018 -- complete earlier updates first, in order
        self._ln = v

    def _defer(self, fn):
        if self._meas:
            self._pending.append(fn)
        else:
            fn()

    def _materializeTensor(self):
        """the pending tensor product's data, now (Ctxt::tensorProduct's DoubleCRT work, src/Ctxt.cpp:1576-1597)"""
        if self._pendT is None:
            return
        t, self._pendT = self._pendT, None
        t0, t1, t2 = self.ops.tensorProduct(*t)
        self.parts = {"1": t0, "s": t1, "s2": t2}

    # ---- bookkeeping ----
    def logOfPrimeSet(self):
        return self.context.logOfProduct(self.primeSet)

    def modSwitchAddedNoiseBound(self):
        h = self.context.skBound()
        added = sum(h ** _powerOfS(k) for k in self.parts)
        return added * self.context.noiseBoundForUniform(self.ptxtSpace / 2.0, self.context.phim)

    # ---- prime-set maintenance ----
    @timing.timed
    def modUpToSet(self, s):
        diff = sorted(frozenset(s) - self.primeSet)
        if not diff:
            return
        self._materializeTensor()
        for p in self.parts.values():
            p.addPrimesAndScale(diff)
        self.lnNoise += self.context.logOfProduct(diff)
        self.lnRatFactor += self.context.logOfProduct(diff)   # "If CKKS, the rational factor grows" (:366)
        self.primeSet = self.primeSet | frozenset(diff)

    @timing.timed
    def modDownToSet(self, s):
        inter = self.primeSet & frozenset(s)
        if not inter:
            raise RuntimeError(f"modDownToSet called from {sorted(self.primeSet)} to {sorted(s)}")
        diff = self.primeSet - inter
        if not diff:
            return
        added = Ctxt._modDownParts([self], sorted(inter))[0]
        logdiff = self.context.logOfProduct(diff)
        self.lnRatFactor -= logdiff                              # ratFactor /= f (:533, :553)
        bound = math.log(self.modSwitchAddedNoiseBound()) if timing.fhe_stats else None

        def update():
            add = _ln(added())
            if bound is not None:   # src/Ctxt.cpp:535-537: added noise over its a-priori bound
                timing.STATS_UPDATE("mod-switch-added-noise", math.exp(add - bound))
            self._ln = logaddexp(self._ln - logdiff, add)
        self._defer(update)
        self.primeSet = inter

    @staticmethod
    def _modDownParts(cts, keep, add=()):
        """The polynomial work of modDownToSet (after a mod-up by `add`, if given) on all parts of
        ciphertexts that share one prime set, in one backend call where the backend has one.
        Returns, per ciphertext, a function giving its added noise: measured, sum over parts of
        embeddingLargestCoeff(fdelta) * h^power (src/Ctxt.cpp:495-527) -- to be called once the
        norms have been read back (Ctxt.lnNoise does) -- else the bound."""
        a = cts[0]
        ops, meas, ptxt = a.ops, a._meas, a.ptxtSpace
        kw = {"norms": True, "defer": True} if meas else {}
        pend = None
        if len(cts) == 1 and a._pendT is not None:   # the tensor product is formed inside this mod-switch
            pend, a._pendT = a._pendT, None
        else:
            for c in cts:
                c._materializeTensor()
        parts = [p for c in cts for p in c.parts.values()]
        if pend is not None:
            res = ops.tensorBringToSet(*pend, list(add), keep, ptxt, **kw)
            outs, norms = res if meas else (res, None)
            a.parts = {"1": outs[0], "s": outs[1], "s2": outs[2]}
        elif add and hasattr(ops, "bringToSetMulti"):
            norms = ops.bringToSetMulti(parts, add, keep, ptxt, **kw)
        elif add:
            for p in parts:
                p.addPrimesAndScale(list(add))
            norms = [p.scaleDownToSet(keep, ptxt, **({"norms": True} if meas else {})) for p in parts]
        elif hasattr(ops, "scaleDownToSetMulti"):
            norms = ops.scaleDownToSetMulti(parts, keep, ptxt, **kw)
        else:
            norms = [p.scaleDownToSet(keep, ptxt, **({"norms": True} if meas else {})) for p in parts]
        if not meas:
            return [c.modSwitchAddedNoiseBound for c in cts]
        h = a.context.skBound()
        out, k = [], 0
        for c in cts:
            keys = list(c.parts)
            out.append(lambda k0=k, keys=keys: sum(float(max(norms[k0 + i])) * h ** _powerOfS(key)
                                                   for i, key in enumerate(keys)))
            k += len(keys)
        return out

    @timing.timed
    def bringToSet(self, s):
        s = frozenset(s) if s else frozenset([self.context.ctxtPrimes[0]])
        if hasattr(self.ops, "bringToSetMulti") or self._pendT is not None:
            Ctxt._bringManyToSet([self], s)
            return
        self.modUpToSet(s)
        self.modDownToSet(s)

    @staticmethod
    def _bringManyToSet(cts, s):
        """bringToSet(s) = modUpToSet(s); modDownToSet(s) for ciphertexts that sit on one prime
        set, with the polynomial work of all their parts in one backend call (the mod-up scaling
        is folded into the mod-down kernels on the GPU).  Bookkeeping as in src/Ctxt.cpp:346-562."""
        a = cts[0]
        add = sorted(s - a.primeSet)
        up = a.primeSet | frozenset(add)
        inter = up & s
        if not inter:
            raise RuntimeError(f"modDownToSet called from {sorted(up)} to {sorted(s)}")
        diff = up - inter
        if not add and not diff:
            return
        if not diff:        # a pure mod-up: no mod-switch kernel to form a pending product in
            for c in cts:
                c._materializeTensor()
        added = Ctxt._modDownParts(cts, sorted(inter), add=add or ())
        for c, ad in zip(cts, added):
            c.lnNoise += c.context.logOfProduct(add)
            c.lnRatFactor += c.context.logOfProduct(add) - c.context.logOfProduct(diff)
            c.primeSet = up
            if diff:
                logdiff = c.context.logOfProduct(diff)
                c._defer(lambda c=c, ad=ad, logdiff=logdiff:
                         setattr(c, "_ln", logaddexp(c._ln - logdiff, _ln(ad()))))
                c.primeSet = inter

    @staticmethod
    def _bringBothToSet(a, b, s):
        """bringToSet(s) on two ciphertexts that sit on the same prime set: identical arithmetic
        and bookkeeping to calling it on each, with one batched mod-switch for all parts."""
        s = frozenset(s) if s else frozenset([a.context.ctxtPrimes[0]])
        a.modUpToSet(s)
        b.modUpToSet(s)
        inter = a.primeSet & s
        if not inter:
            raise RuntimeError(f"modDownToSet called from {sorted(a.primeSet)} to {sorted(s)}")
        diff = a.primeSet - inter
        if not diff:
            return
        added = Ctxt._modDownParts([a, b], sorted(inter))
        logdiff = a.context.logOfProduct(diff)
        for c, ad in zip((a, b), added):
            c.lnRatFactor -= logdiff
            c._defer(lambda c=c, ad=ad: setattr(c, "_ln", logaddexp(c._ln - logdiff, _ln(ad()))))
            c.primeSet = inter

    @timing.timed
    def dropSmallAndSpecialPrimes(self):
        ctx = self.context
        small, ctp = frozenset(ctx.smallPrimes), frozenset(ctx.ctxtPrimes)
        if not (self.primeSet & small):
            self.modDownToSet(ctp)
            return
        target = set(self.primeSet & ctp)
        dropping = self.primeSet - target
        log_dropping = ctx.logOfProduct(dropping)
        log_msn = math.log(self.modSwitchAddedNoiseBound()) + 3 * LN2
        comp = 0.0
        if self.lnNoise - log_dropping + comp < log_msn:
            for i in sorted(ctp - target):
                target.add(i)
                comp += ctx.logOfPrime(i)
                if self.lnNoise - log_dropping + comp >= log_msn:
                    break
        self.bringToSet(target)

    # ---- arithmetic ----
    # ---- size / correctness accessors (include/helib/Ctxt.h:1291-1325, src/Ctxt.cpp:116-127) ----
    def lnTotalNoiseBound(self):
        """ln of totalNoiseBound(): for CKKS ptxtMag*ratFactor + noiseBound, else noiseBound"""
        if self.context.ckks:
            return logaddexp(_ln(self.ptxtMag) + self.lnRatFactor, self.lnNoise)
        return self.lnNoise

    def capacity(self):
        """log2 of the modulus over the TOTAL noise bound (at least 1)"""
        return (self.logOfPrimeSet() - max(self.lnTotalNoiseBound(), 0.0)) / LN2

    def bitCapacity(self):
        return int(self.capacity())

    def isCorrect(self):
        """totalNoiseBound * polyNormBnd <= 0.48 Q: would this ciphertext decrypt without errors?"""
        return self.lnTotalNoiseBound() + math.log(polyNormBnd(self.context.m)) <= \
            math.log(0.48) + self.logOfPrimeSet()

    def frobeniusAutomorph(self, j):
        """Ctxt::frobeniusAutomorph (src/Ctxt.cpp:2526-2545): X -> X^(p^j) for BGV (j mod ord(p));
        for CKKS complex conjugation when j is odd (X -> X^(m-1))."""
        if not self.parts or j == 0:
            return
        ctx = self.context
        if ctx.ckks:
            if j & 1:
                self.smartAutomorph(ctx.m - 1)
            return
        d, x = 1, ctx.p % ctx.m
        while x != 1:
            x = x * ctx.p % ctx.m
            d += 1
        j %= d
        if j:
            self.smartAutomorph(pow(ctx.p, j, ctx.m))

    def mulIntFactor(self, e):
        """Ctxt::mulIntFactor (src/Ctxt.cpp:331-340)"""
        if e == 1:
            return
        self.intFactor = self.intFactor * e % self.ptxtSpace
        bal = e - self.ptxtSpace if e > self.ptxtSpace // 2 else e
        for p in self.parts.values():
            p.mulConstant(bal)
        self.lnNoise = self.lnNoise + math.log(abs(bal))

    def effectiveR(self):
        """Ctxt::effectiveR (src/Ctxt.cpp:103-114): the r with ptxtSpace = p^r"""
        p = self.context.p
        r, p2r = 1, p
        while r < HELIB_SP_NBITS:
            if p2r == self.ptxtSpace:
                return r
            if p2r > self.ptxtSpace:
                break
            r, p2r = r + 1, p2r * p
        raise RuntimeError("ctxt.ptxtSpace is not of the form p^r")

    def divideByP(self):
        """Ctxt::divideByP (src/Ctxt.cpp:2415-2435): for a ciphertext whose plaintext is 0 mod p -- every part times
        p^-1 mod Q (Q the product of the prime set), the noise and the plaintext space divided by p, intFactor reduced
        to the new space.  The reference's two asserts are errors here."""
        if not self.parts:
            return self
        p = self.context.p
        if self.ptxtSpace % p != 0:
            raise RuntimeError("p must divide ptxtSpace")
        if self.ptxtSpace <= p:
            raise RuntimeError("ptxtSpace must be strictly greater than p")
        self._materializeTensor()
        pInverse = pow(p, -1, self.context.productOfPrimes(self.primeSet))
        for part in self.parts.values():
            part.mulConstant(pInverse)
        self.lnNoise = self.lnNoise - math.log(p)
        self.ptxtSpace //= p
        self.intFactor %= self.ptxtSpace
        return self

    def reducePtxtSpace(self, newPtxtSpace):
        """Ctxt::reducePtxtSpace (src/Ctxt.cpp:576-584): the plaintext space becomes its gcd with newPtxtSpace"""
        g = math.gcd(self.ptxtSpace, int(newPtxtSpace))
        if g <= 1:
            raise RuntimeError("New and old plaintext spaces are coprime")
        self.ptxtSpace = g
        self.intFactor %= g
        return self

    def multByP(self, e=1):
        """Ctxt::multByP (include/helib/Ctxt.h:1216-1221): the plaintext space grows to p^(r+e), then
        multByConstant(p^e)"""
        p2e = self.context.p ** e
        self.ptxtSpace *= p2e
        return self.multByScalar(p2e)

    fuseScaledSub = False  # fused=None: the two calls until hx_scaled_sub has been measured as the faster form

    def subDivideByP(self, other, fused=None):
        """*this -= other; this->divideByP() -- the inner step of extractDigits (src/extractDigits.cpp:106-107).
        Fused: addCtxt's own preparation (_alignForAdd: the plaintext spaces' gcd, the union of the prime sets, the
        intFactor pair e1, e2), then one ops.scaledSub (hx_scaled_sub) with u = balanced(e1) / p and
        v = balanced(e2) / p modulo every prime in place of mulIntFactor on both sides, the subtraction and the
        product by p^-1 mod Q; the bookkeeping of the two calls is done here, float operation for float operation.  It
        applies when both sides hold the canonical parts {1, s} or the same single part and divideByP's conditions
        hold; otherwise, and with fused=False, the two calls run as they are.  fused=True insists on a backend with
        scaledSub; fused=None follows Ctxt.fuseScaledSub.  The words, lnNoise, primeSet, ptxtSpace and intFactor are
        the same either way; `other` is left as it was either way."""
        has = hasattr(self.ops, "scaledSub")
        if fused and not has:
            raise RuntimeError("Ctxt::subDivideByP: fused=True, but this backend has no scaledSub")
        want = (Ctxt.fuseScaledSub if fused is None else fused) and has
        ctx = self.context
        p = ctx.p
        g = math.gcd(self.ptxtSpace, other.ptxtSpace)
        can = (want and not ctx.ckks and other is not self and self.parts and other.parts
               and g % p == 0 and g > p)
        if can:
            self._materializeTensor()
            other._materializeTensor()
            hs = list(self.parts)
            can = sorted(hs) == sorted(other.parts) and (len(hs) == 1 or sorted(hs) == ["1", "s"])
        if not can:
            self -= other
            return self.divideByP()
        o, _, e1, e2 = self._alignForAdd(other)
        idx = self.parts[hs[0]].getIndexSet()
        if any(self.parts[h].getIndexSet() != idx or o.parts[h].getIndexSet() != idx for h in hs):
            # the kernel pairs rows by position: two sides whose rows stand in different orders (a digit that came out
            # of polyEval) take the two calls, which find nothing left to align
            self -= other
            return self.divideByP()
        P = self.ptxtSpace
        bal = lambda e: e - P if e > P // 2 else e                     # noqa: E731  (mulIntFactor's)
        pInverse = pow(p, -1, ctx.productOfPrimes(self.primeSet))
        u = [bal(e1) * pInverse % ctx.primes[i] for i in idx]
        v = [bal(e2) * pInverse % ctx.primes[i] for i in idx]
        if len(hs) == 2:
            self.ops.scaledSub(self.parts["1"], self.parts["s"], o.parts["1"], o.parts["s"], u, v)
        else:
            self.ops.scaledSub(self.parts[hs[0]], None, o.parts[hs[0]], None, u, v)
        oln = o.lnNoise
        if e2 != 1:                                                    # o.mulIntFactor(e2): the bound alone
            oln = oln + math.log(abs(bal(e2)))
        if e1 != 1:                                                    # self.mulIntFactor(e1)
            self.intFactor = self.intFactor * e1 % P
            self.lnNoise = self.lnNoise + math.log(abs(bal(e1)))
        self.ptxtMag += o.ptxtMag                                      # the subtraction
        self.lnNoise = logaddexp(self.lnNoise, oln)
        self.lnNoise = self.lnNoise - math.log(p)                      # divideByP
        self.ptxtSpace //= p
        self.intFactor %= self.ptxtSpace
        return self

    def negate(self):
        for p in self.parts.values():
            p.Negate()

    @staticmethod
    def equalizeRationalFactors(c1, c2):
        """Ctxt::equalizeRationalFactors (src/Ctxt.cpp:1212-1356): scale both CKKS ciphertexts by
        small integers (continued-fraction convergents of the ratio of their factors) until they
        share one factor, stopping as soon as the discretisation error is within sqrt(2) of the
        error the sum has anyway.  Computed relative to the smaller factor, so plain doubles do
        (the reference's xdouble carries the same 53 bits)."""
        big, small = (c1, c2) if c1.lnRatFactor > c2.lnRatFactor else (c2, c1)
        base = small.lnRatFactor
        x = math.exp(big.lnRatFactor - base)
        r = c1.context.r
        denomBound = 1 << (r + 1)
        epsilon = 0.125 / denomBound
        a = int(math.floor(x + epsilon))
        xi = x - a
        prevDenom, denom = 0, 1
        numer = int(math.floor(denom * x + 0.5))
        m1, of1, oe1 = big.ptxtMag, x, math.exp(big.lnNoise - base)
        m2, of2, oe2 = small.ptxtMag, 1.0, math.exp(small.lnNoise - base)
        target = oe1 / of1 + oe2 / of2

        def calc_err(f, f1, e1, f2, e2):
            return m1 * abs(f1 / f - 1.0) + m2 * abs(f2 / f - 1.0) + (e1 + e2) / f
        while True:
            f1, e1 = of1 * denom, oe1 * denom
            f2, e2 = of2 * numer, oe2 * numer
            err1, err2 = calc_err(f1, f1, e1, f2, e2), calc_err(f2, f1, e1, f2, e2)
            if err1 < err2:
                f, fe1, fe2, err = f1, e1, e2 + m2 * abs(f2 - f1), err1
            else:
                f, fe1, fe2, err = f2, e1 + m1 * abs(f2 - f1), e2, err2
            if err < math.sqrt(2.0) * target or xi <= 0:
                break
            xi = 1.0 / xi
            ai = int(math.floor(xi + epsilon))
            xi -= ai
            tmpDenom = denom * ai + prevDenom
            if tmpDenom > denomBound:
                break
            prevDenom, denom = denom, tmpDenom
            numer = int(math.floor(denom * x + 0.5))
        if denom != 1:
            for p in big.parts.values():
                p.mulConstant(denom)
        if numer != 1:
            for p in small.parts.values():
                p.mulConstant(numer)
        big.lnRatFactor = small.lnRatFactor = math.log(f) + base
        big.lnNoise, small.lnNoise = _ln(fe1) + base, _ln(fe2) + base

    @timing.timed
    def addCtxt(self, other, negative=False):
        """Ctxt::addCtxt (src/Ctxt.cpp:1405-1556): plaintext spaces reduced to their gcd (BGV),
        both operands mod-switched UP to the union of their prime sets, CKKS factors equalised,
        BGV intFactors harmonised by the (e1, e2) of least noise along the extended Euclidean
        sequence, then the parts added handle by handle."""
        if not other.parts:
            return
        if not self.parts:
            c = other.clone()
            self.__dict__.update(c.__dict__)
            if negative:
                self.negate()
            return
        o, owned, e1, e2 = self._alignForAdd(other)
        if e2 != 1:
            if not owned:
                o = other.clone()
            o.mulIntFactor(e2)
        if e1 != 1:
            self.mulIntFactor(e1)
        for h, p in o.parts.items():
            if h in self.parts:
                if negative:
                    self.parts[h] -= p
                else:
                    self.parts[h] += p
            else:
                self.parts[h] = p.copy()
                if negative:
                    self.parts[h].Negate()
        self.ptxtMag += o.ptxtMag
        self.lnNoise = logaddexp(self.lnNoise, o.lnNoise)

    def _alignForAdd(self, other):
        """addCtxt up to the sum itself (src/Ctxt.cpp:1428-1526), both sides with parts: the plaintext spaces' gcd,
        the union of the prime sets, the CKKS factors, and the (e1, e2) that harmonise the BGV intFactors, not yet
        applied.  -> (o, owned, e1, e2): o is `other`, or (owned) a clone where it had to change."""
        ctx = self.context
        o = other
        owned = False

        def own():
            nonlocal o, owned
            if not owned:
                o, owned = other.clone(), True
            return o
        if ctx.ckks:
            if self.ptxtSpace != 1 or other.ptxtSpace != 1:
                raise ValueError("Plaintext spaces incompatible")
        else:
            g = math.gcd(self.ptxtSpace, other.ptxtSpace)
            if g <= 1:
                raise ValueError("New and old plaintext spaces are coprime")
            self.ptxtSpace = g
            self.intFactor %= g
            if other.ptxtSpace != g:
                own().ptxtSpace = g
                o.intFactor %= g
        if o.primeSet - self.primeSet:
            self.modUpToSet(self.primeSet | o.primeSet)
        if self.primeSet - o.primeSet:
            own().modUpToSet(self.primeSet)
        if ctx.ckks:
            Ctxt.equalizeRationalFactors(self, own())
        e1 = e2 = 1
        if not ctx.ckks and self.intFactor != o.intFactor:
            e1, e2 = Ctxt._intFactorPair(ctx.p, self.ptxtSpace, self.intFactor, self.lnNoise, o.intFactor, o.lnNoise)
        return o, owned, e1, e2

    @staticmethod
    def _intFactorPair(p, P, f1, ln1, f2, ln2):
        """the (e1, e2) with e1 f1 = e2 f2 mod P of least noise along the extended Euclidean sequence of P and f2 / f1
        (src/Ctxt.cpp:1474-1526); ln1, ln2 the two sides' ln(noiseBound)"""
        ratio = f2 * pow(f1, -1, P) % P
        bal = lambda e: abs(e - P if e > P // 2 else e)                 # noqa: E731
        norm = lambda a, b: logaddexp(ln1 + _ln(bal(a)), ln2 + _ln(bal(b)))  # noqa: E731
        r0, t0, r1, t1 = P, 0, ratio, 1
        e1, e2 = r1, t1
        best = norm(e1, e2)
        while r1 != 0:
            q = r0 // r1
            r0, r1, t0, t1 = r1, r0 % r1, t1, t0 - t1 * q
            a, b = r1 % P, t1 % P
            if a % p != 0:
                cand = norm(a, b)
                if cand < best:
                    e1, e2, best = a, b, cand
        assert e1 * f1 % P == e2 * f2 % P
        assert math.gcd(e1, P) == 1 and math.gcd(e2, P) == 1
        return e1, e2

    @staticmethod
    def computeIntervalForMul(c1, c2):
        cap1 = c1.logOfPrimeSet() - max(c1.lnNoise, 0.0)
        cap2 = c2.logOfPrimeSet() - max(c2.lnNoise, 0.0)
        adn1 = math.log(c1.modSwitchAddedNoiseBound())
        adn2 = math.log(c2.modSwitchAddedNoiseBound())
        if c1.context.ckks:     # the opposite end: keep n*q'/q above the added noise (:1637-1651)
            lo = max(cap1 + adn1, cap2 + adn2) + Ctxt.safety
            return lo, lo + 4 * LN2
        hi = min(cap1 + adn1, cap2 + adn2) - Ctxt.safety
        return hi - 4 * LN2, hi

    @timing.timed
    def multLowLvl(self, other, destructive=False, lazyTensor=False):
        o = other if destructive else other.clone()
        ckks = self.context.ckks
        if ckks:
            assert self.ptxtSpace == 1 and o.ptxtSpace == 1, "Plaintext spaces incompatible"
        else:
            g = math.gcd(self.ptxtSpace, o.ptxtSpace)
            assert g > 1, "Plaintext spaces are co-prime"
            self.ptxtSpace = o.ptxtSpace = g
            self.intFactor %= g
            o.intFactor %= g
        lo, hi = Ctxt.computeIntervalForMul(self, o)
        common = self.context.modSizes.getSet4Size(lo, hi, self.primeSet, o.primeSet, ckks)
        if self.primeSet == o.primeSet and hasattr(self.ops, "bringToSetMulti"):
            Ctxt._bringManyToSet([self, o], frozenset(common) if common else
                                 frozenset([self.context.ctxtPrimes[0]]))
        elif self.primeSet == o.primeSet and hasattr(self.ops, "scaleDownToSetMulti"):
            Ctxt._bringBothToSet(self, o, common)   # same result, the 4 parts share the launches
        else:
            self.bringToSet(common)
            o.bringToSet(common)
        self._tensorProduct(o, lazyTensor)

    def _tensorProduct(self, o, lazy=False):
        if self.ptxtSpace > 2:
            q = self.context.productOfPrimes(self.primeSet) % self.ptxtSpace
            self.intFactor = self.intFactor * o.intFactor % self.ptxtSpace * q % self.ptxtSpace
        if set(self.parts) == {"1", "s"} and set(o.parts) == {"1", "s"}:
            four = (self.parts["1"], self.parts["s"], o.parts["1"], o.parts["s"])
            if lazy and Ctxt.lazyTensor and hasattr(self.ops, "tensorBringToSet"):
                # the product's data is left to the kernels that consume it (include/helib_amd_ctxt.hpp, pendingTensor)
                self._pendT = four
                self.parts = {"1": None, "s": None, "s2": None}
            else:
                t0, t1, t2 = self.ops.tensorProduct(*four)
                self.parts = {"1": t0, "s": t1, "s2": t2}
        else:   # any parts (src/Ctxt.cpp:1576-1597): all pairwise products, accumulated by handle
            new = {}
            for h1, p1 in self.parts.items():
                for h2, p2 in o.parts.items():
                    h = handle_mul(h1, h2)
                    t = p1.copy()
                    t *= p2
                    if h in new:
                        new[h] += t
                    else:
                        new[h] = t
            self.parts = new
        if self.context.ckks:   # totalNoiseBound = factor*ptxt + noiseBound on both sides (:1600-1606)
            n1, n2 = self.lnNoise, o.lnNoise
            self.lnNoise = logaddexp(logaddexp(n1 + _ln(o.ptxtMag) + o.lnRatFactor,
                                               n2 + _ln(self.ptxtMag) + self.lnRatFactor), n1 + n2)
            self.lnRatFactor += o.lnRatFactor
            self.ptxtMag *= o.ptxtMag
        else:
            self.lnNoise = self.lnNoise + o.lnNoise

    @timing.timed
    def reLinearize(self):
        """Ctxt::reLinearize (src/Ctxt.cpp:720-786) for the shapes of this path: (1, s, s^2) after a
        multiplication, or (1, [s,] s(X^k)) after an automorphism."""
        other = [h for h in self.parts if h not in ("1", "s")]
        if not other:
            return
        if len(other) > 1:
            self._materializeTensor()
            return self._reLinearizeMany(other)
        hnd = other[0]
        W = self._matrixFor(hnd)
        ctx = self.context
        self.dropSmallAndSpecialPrimes()
        self._relin_CKKS_adjust()
        sp = list(ctx.specialPrimes)
        # No mod-switch consumed a pending tensor product (a fresh CKKS product, a product at a level that needs
        # none): at the full level the key switch takes the operands themselves (ops.mulRelin = hx_mul_relin);
        # otherwise the product is formed now.
        pend = None
        if self._pendT is not None:
            cp = list(ctx.ctxtPrimes)
            if (hasattr(self.ops, "mulRelin") and self._pendT[0].getIndexSet() == cp and frozenset(cp) == self.primeSet
                    and list(getattr(W, "row_idx", ())) == cp + sp):
                pend, self._pendT = self._pendT, None
            else:
                self._materializeTensor()
        logProd = ctx.logOfProduct(sp)
        self.lnRatFactor += logProd                              # CKKS factor after mod-up (:757)
        # digits of the context restricted to the current prime set (src/DoubleCRT.cpp:485-493)
        digits = [[i for i in d if i in self.primeSet] for d in ctx.digits]
        digits = [d for d in digits if d]
        if self.ptxtSpace > 1:   # g == 1 for CKKS
            self.ptxtSpace = math.gcd(self.ptxtSpace, self.ksw_ptxtSpace)
            self.intFactor %= self.ptxtSpace
        kw = {"norms": True, "defer": True} if self._meas else {}
        if pend is not None:
            res = self.ops.mulRelin(*pend, W, digits, **kw)
        else:
            res = self.ops.reLinearize(self.parts["1"], self.parts.get("s"), self.parts[hnd], W, digits, sp, **kw)
        o0, o1 = res[0], res[1]

        # noise: scaled parts + key-switch added noise (src/Ctxt.cpp:746, 827-841)
        def update():
            added = -math.inf
            for k, d in enumerate(digits):
                bnd = math.log(ctx.noiseBoundForUniform(0.5, ctx.phim)) + ctx.logOfProduct(d)
                if self._meas:   # norm_val = embeddingLargestCoeff(digit) (src/DoubleCRT.cpp:538-545)
                    nb = _ln(float(max(res[2][k]))) + ctx.logOfProduct(d)
                    if timing.fhe_stats:   # (src/DoubleCRT.cpp:547-548)
                        timing.STATS_UPDATE("break-into-digits-ratio", math.exp(nb - bnd))
                else:            # high-probability bound (src/DoubleCRT.cpp:520-529)
                    nb = bnd
                added = logaddexp(added, nb + self.ksw_lnNoise)
            if timing.fhe_stats:           # (src/Ctxt.cpp:833-835): added noise over the ciphertext's own
                timing.STATS_UPDATE("KS-noise-ratio", math.exp(added - (self._ln + logProd)))
            self._ln = logaddexp(self._ln + logProd, added)

        self.parts = {"1": o0, "s": o1}
        self.primeSet = self.primeSet | frozenset(sp)
        self._defer(update)

    def switchToKey(self, ks):
        """Ctxt::reLinearize(keyID) (src/Ctxt.cpp:720-786, as src/recryption.cpp:434 calls it) for a canonical
        ciphertext: the s part is key-switched by ks, a keys.KeySwitchInfo from this key to another one, and the
        result, parts "1" and "s", is relative to THAT key.  The mod-up, the digits and the noise are reLinearize's."""
        self._materializeTensor()
        if set(self.parts) - {"1", "s"}:
            raise RuntimeError("switchToKey takes a ciphertext in canonical form")
        if "s" not in self.parts:
            return self
        ctx = self.context
        self.dropSmallAndSpecialPrimes()
        sp = list(ctx.specialPrimes)
        logProd = ctx.logOfProduct(sp)
        digits = [[i for i in d if i in self.primeSet] for d in ctx.digits]
        digits = [d for d in digits if d]
        self.ptxtSpace = math.gcd(self.ptxtSpace, ks.ptxtSpace)
        self.intFactor %= self.ptxtSpace
        res = self.ops.reLinearize(self.parts["1"], None, self.parts["s"], ks.W, digits, sp)
        added = -math.inf
        for d in digits:   # the high-probability bound on a digit (src/DoubleCRT.cpp:520-529)
            added = logaddexp(added, math.log(ctx.noiseBoundForUniform(0.5, ctx.phim)) + ctx.logOfProduct(d) +
                              math.log(ks.noiseBound))
        ln = logaddexp(self.lnNoise + logProd, added)
        self.parts = {"1": res[0], "s": res[1]}
        self.primeSet = self.primeSet | frozenset(sp)
        self.lnNoise = ln
        return self

    def replicated(self, batch):
        """this ciphertext with every part repeated over `batch` elements (a part of batch 1 is broadcast into a zeroed
        part of the wanted batch): what `ctxt = recryptEkey` needs when the constants that follow are batched"""
        c = self.clone()
        for h, part in list(c.parts.items()):
            have = getattr(part, "batch", 1)
            if have == batch:
                continue
            if have != 1:
                raise RuntimeError("replicated: a part holds %d elements, not 1" % have)
            wide = type(part)(part.context, part.getIndexSet(), batch)
            wide += part
            c.parts[h] = wide
        return c

    def _matrixFor(self, hnd):
        """PubKey::getKeySWmatrix for the part's handle; LogicError in the reference when absent"""
        sp_, xp_ = handle_powers(hnd)
        if (sp_, xp_) == (2, 1):
            W = self.ksw
        elif sp_ == 1:
            W = self.ksw_auto.get(xp_)
        elif xp_ == 1:
            W = self.ksw_pow.get(sp_)
        else:
            W = None
        if W is None:
            raise LookupError(f"no key-switching matrices for s^{sp_}(X^{xp_})")
        return W

    def _reLinearizeMany(self, other):
        """Ctxt::reLinearize with several non-canonical parts (after multiplyBy2: s^2 and s^3):
        parts 1 and s are scaled by P, every other part goes through keySwitchPart -- break into
        digits, key-switch with its own matrix, accumulate (src/Ctxt.cpp:720-842)."""
        ctx = self.context
        mats = {h: self._matrixFor(h) for h in other}
        self.dropSmallAndSpecialPrimes()
        self._relin_CKKS_adjust()
        sp = list(ctx.specialPrimes)
        logProd = ctx.logOfProduct(sp)
        self.lnRatFactor += logProd
        digits = [[i for i in d if i in self.primeSet] for d in ctx.digits]
        digits = [d for d in digits if d]
        if self.ptxtSpace > 1:
            self.ptxtSpace = math.gcd(self.ptxtSpace, self.ksw_ptxtSpace)
            self.intFactor %= self.ptxtSpace
        part0 = self.parts["1"]
        part0.addPrimesAndScale(sp)
        if "s" in self.parts:
            part1 = self.parts["s"]
            part1.addPrimesAndScale(sp)
        else:
            part1 = self.ops.zerosLike(part0)
        added = -math.inf
        for h in other:
            if self._meas:
                dg, nrm = self.ops.breakIntoDigits(self.parts[h], digits, sp, norms=True)
            else:
                dg, nrm = self.ops.breakIntoDigits(self.parts[h], digits, sp), None
            self.ops.keySwitchDigits(dg, mats[h], part0, part1)
            for k, d in enumerate(digits):
                nb = _ln(float(max(nrm[k]))) if nrm is not None else \
                    math.log(ctx.noiseBoundForUniform(0.5, ctx.phim))
                added = logaddexp(added, nb + ctx.logOfProduct(d) + self.ksw_lnNoise)
        self.lnNoise = logaddexp(self.lnNoise + logProd, added)
        self.parts = {"1": part0, "s": part1}
        self.primeSet = self.primeSet | frozenset(sp)

    @timing.timed
    def multiplyBy2(self, other1, other2):
        """Ctxt::multiplyBy2 (src/Ctxt.cpp:1776-1828): the product of three ciphertexts with ONE
        relinearisation at the end (parts up to s^3), multiplying in the order of their capacities."""
        if not self.parts:
            return
        for o in (other1, other2):
            if not o.parts:
                c = o.clone()
                self.__dict__.update(c.__dict__)
                return
        cap, cap1, cap2 = self.capacity(), other1.capacity(), other2.capacity()
        if cap < cap1 and cap < cap2:
            tmp = other1.clone()
            tmp.multLowLvl(other2)
            self.multLowLvl(tmp, destructive=True)
            self.reLinearize()
            return
        first, second = (other2, other1) if (cap < cap2 or cap1 < cap2) else (other1, other2)
        second = second.clone() if second is self else second
        self.multLowLvl(first if first is not self else first.clone())
        self.multLowLvl(second)
        self.reLinearize()

    @timing.timed
    def square(self):
        """Ctxt::square: multiplyBy(*this)"""
        self.multiplyBy(self.clone())

    def cube(self):
        """Ctxt::cube: multiplyBy2(*this, *this)"""
        self.multiplyBy2(self.clone(), self.clone())

    def power(self, e):
        """Ctxt::power (src/polyEval.cpp:392-414): repeated squaring for a power of two, otherwise
        DynamicCtxtPowers (:18-29): X^e = X^(e-k) * X^k with k the largest power of two below e, every
        power computed once -- the multiplication depth stays at ceil(log2 e)."""
        if e < 1:
            raise ValueError("Cannot raise a ctxt to a non positive exponent")
        if e == 1:
            return self
        if e & (e - 1) == 0:
            for _ in range(e.bit_length() - 1):
                self.square()
            return self
        r = DynamicCtxtPowers(self, e).getPower(e)
        self.__dict__.update(r.__dict__)
        return self

    def _relin_CKKS_adjust(self):
        """Ctxt::relin_CKKS_adjust (src/Ctxt.cpp:664-717): if the noise is below what the special
        primes were sized for, scale the ciphertext (and its factor) up by an integer."""
        ctx = self.context
        if not ctx.ckks:
            return
        h = ctx.phim / 2.0 if ctx.hwt == 0 else float(ctx.hwt)
        log_phim = max(math.log(ctx.phim), 1.0)
        gamma = 8.0 * int(ctx.scale) * math.sqrt(ctx.phim * log_phim * h / 12.0)
        if math.log(gamma) > self.lnNoise:
            self._materializeTensor()
            xf = int(math.ceil(math.exp(math.log(gamma) - self.lnNoise)))
            for p in self.parts.values():
                p.mulConstant(xf)
            self.lnNoise = self.lnNoise + math.log(xf)
            self.lnRatFactor += math.log(xf)

    # ---- rotations ----
    def automorph(self, k):
        """Ctxt::automorph (src/Ctxt.cpp:2437-2457): F(X) -> F(X^k) on every part; the part that
        pointed at s now points at s(X^k).  No change in the noise bound."""
        m = self.context.m
        k %= m
        if math.gcd(k, m) != 1:
            raise ValueError("k must be in Zm*")
        if k == 1:
            return self
        assert "s2" not in self.parts, "relinearise before an automorphism"
        new = {}
        for h, p in self.parts.items():
            p.automorph(k)
            if h == "1":
                new[h] = p
            else:
                j = (1 if h == "s" else h[1]) * k % m
                new["s" if j == 1 else ("s", j)] = p
        self.parts = new
        return self

    def _firstStep(self, k):
        """PubKey::getNextKSWmatrix(k).fromKey.getPowerOfX(): k itself when there is a matrix for it
        and no map was set, otherwise the first edge of the BFS path (PubKey::setKeySwitchMap)."""
        if self.ksw_map is not None:
            amt = self.ksw_map[k]
            if amt == 0 or amt not in self.ksw_auto:
                raise LookupError(f"no key-switching matrices for k={k}")   # LogicError in the reference
            return amt
        if k not in self.ksw_auto:
            raise LookupError(f"no key-switching matrices for k={k}")
        return k

    @timing.timed
    def smartAutomorph(self, k):
        """Ctxt::smartAutomorph (src/Ctxt.cpp:2462-2515): re-linearise, then walk the path of
        available matrices -- automorph(amt), reLinearize, k <- k * amt^-1 -- until k = 1."""
        m = self.context.m
        k %= m
        if k == 1 or not self.parts:
            return self
        if math.gcd(k, m) != 1:
            raise ValueError("k must be in Zm*")
        self._firstStep(k)          # isReachable, before anything is touched
        self.reLinearize()          # canonical form first
        while k != 1:
            amt = self._firstStep(k)
            self.automorph(amt)
            self.reLinearize()
            k = k * pow(amt, -1, m) % m
        return self

    def complexConj(self):
        """Ctxt::complexConj (src/Ctxt.cpp:2517-2523): smartAutomorph(-1)"""
        return self.smartAutomorph(self.context.m - 1)

    @timing.timed
    def multiplyBy(self, other):
        self.multLowLvl(other, lazyTensor=True)
        self.reLinearize()
        self._materializeTensor()
        return self

    # ---- plaintext constants ----
    def multByConstant(self, dcrt, size=-1.0):
        """Ctxt::multByConstant(const DoubleCRT&, double size) (src/Ctxt.cpp:1832-1856), BGV: every
        part times the constant (Mul with matchIndexSets=false: dcrt may live on more primes);
        size < 0: the bound for coefficients uniform in [-ptxtSpace/2, ptxtSpace/2]."""
        if not self.parts:
            return self
        if size < 0.0:
            size = self.context.noiseBoundForMod(self.ptxtSpace, self.context.phim)
        for p in self.parts.values():
            p *= dcrt
        self.lnNoise = self.lnNoise + _ln(size)
        return self

    def multByScalar(self, c):
        """Ctxt::multByConstant(const ZZ& / long / double / xdouble) (src/Ctxt.cpp:2033-2110).
        BGV: c mod ptxtSpace = c1 * d with d = gcd(c, ptxtSpace); the ciphertext is multiplied by the
        balanced d only and the unit c1 goes into intFactor (its inverse).  CKKS: no polynomial work
        at all -- ptxtMag *= |c|, ratFactor /= |c|, a sign flips the parts."""
        if not self.parts:
            return self
        if self.context.ckks:
            c = float(c)
            if c == 1.0:
                return self
            if c == 0.0:
                self.parts = {}
                return self
            self.ptxtMag *= abs(c)
            self.lnRatFactor -= math.log(abs(c))
            if c < 0:
                self.negate()
            return self
        if isinstance(c, float):
            raise TypeError("multByConstant(double) not supported for BGV")     # LogicError in the reference
        P = self.ptxtSpace
        c0 = int(c) % P
        if c0 == 1:
            return self
        if c0 == 0:
            self.parts = {}
            return self
        d = math.gcd(c0, P)
        self.intFactor = self.intFactor * pow(c0 // d, -1, P) % P
        if d == 1:
            return self
        cc = d - P if d > P // 2 else d
        self.lnNoise = self.lnNoise + math.log(abs(cc))
        for p in self.parts.values():
            p.mulConstant(cc)
        return self

    def __iadd__(self, other):       # Ctxt::operator+=
        self.addCtxt(other)
        return self

    def __isub__(self, other):       # Ctxt::operator-=
        self.addCtxt(other, negative=True)
        return self

    def __imul__(self, other):       # Ctxt::operator*= (ciphertext): multiplyBy
        self.multiplyBy(other)
        return self

    def multByConstantCKKS(self, dcrt, size, factor, roundingErr):
        """Ctxt::multByConstantCKKS(const DoubleCRT&, size, factor, roundingErr) (src/Ctxt.cpp:1905-
        1938): dcrt encodes a constant of magnitude <= size scaled by `factor` with encoding error
        <= roundingErr (the reference takes absent values from EncryptedArrayCx, which is out of
        scope here: they are arguments).  noise' = noise*factor*size + roundingErr*ratFactor*ptxtMag +
        noise*roundingErr; ptxtMag *= size; ratFactor *= factor."""
        if not self.parts:
            return self
        if size <= 0:
            size = 1.0
        if factor <= 0 or roundingErr < 0:
            raise ValueError("factor and roundingErr are the encoder's: pass them")
        n = self.lnNoise
        self.lnNoise = logaddexp(logaddexp(n + math.log(factor) + math.log(size),
                                           _ln(roundingErr) + self.lnRatFactor + _ln(self.ptxtMag)),
                                 n + _ln(roundingErr))
        self.ptxtMag *= size
        self.lnRatFactor += math.log(factor)
        for p in self.parts.values():
            p *= dcrt
        return self

    def addConstantCKKS(self, dcrt, size, factor):
        """Ctxt::addConstantCKKS(const DoubleCRT&, size, factor) (src/Ctxt.cpp:951-1045): the constant
        (scaled by `factor`) is multiplied by round(ratFactor / factor) and added to the part of 1;
        ptxtMag += size, noiseBound += 0.5.  The reference mod-switches up (addSomePrimes) when the
        rounded ratio is off by more than 2^-precision; here that case is an error."""
        if size <= 0:
            size = 1.0
        if factor <= 0:
            raise ValueError("factor is the encoder's: pass it")
        x = math.exp(self.lnRatFactor - math.log(factor))
        ratio = int(math.floor(x + 0.5))
        if ratio < 1 or abs(ratio / x - 1.0) * (1 << self.context.r) > 1.0:
            raise RuntimeError("addConstantCKKS: ratFactor / factor is too far from an integer "
                               "(the reference would call addSomePrimes here)")
        self.ptxtMag += size
        self.lnNoise = logaddexp(self.lnNoise, math.log(0.5))
        if "1" not in self.parts:
            raise RuntimeError("Ctxt::addPart: no part pointing at 1")
        if ratio == 1:
            self.parts["1"] += dcrt
        else:
            tmp = dcrt.copy()
            tmp.mulConstant(ratio)
            self.parts["1"] += tmp
        return self

    def addConstant(self, dcrt, size=-1.0):
        """Ctxt::addConstant(const DoubleCRT&, double size) (src/Ctxt.cpp:896-935), BGV: the
        constant is scaled by f = balRem(intFactor * Q mod ptxtSpace) and added to the part of 1."""
        ctx = self.context
        if size < 0.0:
            size = ctx.noiseBoundForMod(self.ptxtSpace, ctx.phim)
        f = 1
        if self.ptxtSpace > 2:
            p = self.ptxtSpace
            f = ctx.productOfPrimes(self.primeSet) % p * self.intFactor % p
            if f > p // 2:                      # balRem: into (-p/2, p/2]
                f -= p
        self.lnNoise = logaddexp(self.lnNoise, _ln(size * abs(f)))
        if "1" not in self.parts:
            raise RuntimeError("Ctxt::addPart: no part pointing at 1")   # (an empty ctxt in the reference)
        if f == 1:
            self.parts["1"] += dcrt
        else:
            tmp = dcrt.copy()
            tmp.mulConstant(f)
            self.parts["1"] += tmp
        return self

    def _constFactor(self):
        """f = balRem(intFactor * Q mod ptxtSpace): what a constant is scaled by before it is added (src/Ctxt.cpp:2163-2168)"""
        f = 1
        if self.ptxtSpace > 2:
            p = self.ptxtSpace
            f = self.context.productOfPrimes(self.primeSet) % p * self.intFactor % p
            if f > p // 2:
                f -= p
        return f

    def addScalar(self, c, neg=False):
        """Ctxt::addConstant(const ZZ&, bool neg) (src/Ctxt.cpp:2264-2282), BGV: c reduced to its balanced residue cc
        (0: nothing to do), then addConstant of the constant polynomial cc on the prime set with size |cc|: the noise
        bound grows by |cc f| and cc f goes to the part pointing at 1, f as in addConstant.  A ciphertext without that
        part -- an empty one after clear() -- gains it, as Ctxt::addSignedPart does."""
        if self.context.ckks:
            raise TypeError("addScalar is the BGV branch of Ctxt::addConstant(ZZ)")
        P = self.ptxtSpace
        cc = int(c) % P
        if cc > P // 2:
            cc -= P
        if cc == 0:
            return self
        self._materializeTensor()
        f = self._constFactor()
        self.lnNoise = logaddexp(self.lnNoise, _ln(float(abs(cc)) * abs(f)))
        v = -cc * f if neg else cc * f
        part = self.parts.get("1")
        if part is not None and hasattr(part, "addConstant"):
            part.addConstant(v)
            return self
        like = part if part is not None else next(iter(self.parts.values()), self._like)
        if like is None or not hasattr(self.ops, "constantLike"):
            raise RuntimeError("Ctxt::addPart: no part pointing at 1, and nothing to shape one after")
        idx = like.getIndexSet() if self.parts else sorted(self.primeSet)
        cst = self.ops.constantLike(like, idx, v)
        if part is not None:
            part += cst
        else:
            self.parts["1"] = cst
        return self

    fuseLinComb = False  # fused=None: the call sequence until hx_lin_comb has been measured as the faster form
    # fused=None in BasicAutomorphPrecon.automorphSum: one hx_hoisted_automorph_sum wherever it applies.  True because the
    # fused form won every alternated pair against the loop (tools/bench_thin_recrypt.py, profiles/thin_recrypt.json,
    # DESIGN 3.9p); set it to False to get the loop back
    fuseHoistedSum = True
    # fused=None in Ctxt.innerProduct: the loop until hx_tensor_sum has been measured as the faster form in every pair
    # of tools/bench_binary_arith.py
    fuseTensorSum = False
    # fused=None in table_lookup.tableLookup's lazy form: one hx_table_tensor_sum.  True because the kernel and the
    # whole lookup through it won every alternated pair against l x hx_mul_add_many and one hx_tensor_sum
    # (tools/bench_table_lookup.py, profiles/table_lookup.json); set it to False to get those calls back
    fuseTableSum = True
    # fused=None in BasicAutomorphPrecon.automorphMasked: the call sequence until hx_hoisted_mask_fan has been measured
    # as the faster form in every pair of tools/bench_replicate.py
    fuseHoistedFan = False
    # fused=None in automorphBlend (and so in matmul_full.MatMulFullExec.mul): one hx_hoisted_blend wherever it applies.
    # True because the kernel won every alternated pair against the sequence with hx_mask_blend, in the stage alone and
    # in the whole product, with the same words (tools/bench_matmul_full.py, profiles/matmul_full.json); set
    # it to False to get the sequence back
    fuseHoistedBlend = True

    @staticmethod
    def innerProduct(v1, v2, fused=None):
        """sum_i v1[i] * v2[i] with the low-level product and ONE relinearisation at the end (innerProduct,
        src/Ctxt.cpp:2878-2893), as a new ciphertext.  fused=False is the reference's loop.  Fused: every pair's
        multLowLvl runs as in the loop -- the prime-set decision, the mod-switch of the operands, the bookkeeping, the
        measured norms -- but leaves its tensor product pending; when every pair is two canonical two-part ciphertexts
        and the n products ended on one prime set (rows in one order) with one ptxtSpace and one intFactor, which is
        when addCtxt would add the parts as they are, one ops.tensorSum (hx_tensor_sum) forms the three parts of the
        sum, and lnNoise and ptxtMag are combined in the loop's order by addCtxt's formulas.  In every other case (CKKS
        among them: addCtxt equalises rational factors) the products are formed and added as the loop adds them.  Then
        reLinearize() as it is.  fused=True insists on a backend with tensorSum; fused=None follows
        Ctxt.fuseTensorSum.  Words, lnNoise, primeSet, ptxtSpace, intFactor and ptxtMag are the same either way."""
        n = min(len(v1), len(v2))
        if n <= 0:
            raise ValueError("innerProduct of empty vectors")
        has = hasattr(v1[0].ops, "tensorSum")
        if fused and not has:
            raise RuntimeError("Ctxt::innerProduct: fused=True, but this backend has no tensorSum")
        if not ((Ctxt.fuseTensorSum if fused is None else fused) and has) or n == 1:
            return innerProduct(v1, v2)
        prods = []
        for i in range(n):
            tmp = v1[i].clone()
            tmp.multLowLvl(v2[i], lazyTensor=True)
            prods.append(tmp)
        result = prods[0]
        pend = [c._pendT for c in prods]
        one = (not result.context.ckks and all(t is not None for t in pend)
               and all(c.primeSet == result.primeSet and c.ptxtSpace == result.ptxtSpace
                       and c.intFactor == result.intFactor for c in prods[1:]))
        if one:
            rows = pend[0][0].getIndexSet()
            one = all(t[0].getIndexSet() == rows for t in pend[1:])
        if not one:
            for c in prods:
                c._materializeTensor()
            for c in prods[1:]:
                result.addCtxt(c)
        else:
            # the launch first: reading lnNoise waits for the mod-switches' norms, and the device works meanwhile
            t0, t1, t2 = result.ops.tensorSum(*[[t[j] for t in pend] for j in range(4)])
            for c in prods[1:]:    # addCtxt's bookkeeping (src/Ctxt.cpp:1554-1555), while the operands still say where
                result.ptxtMag += c.ptxtMag                       # the deferred norms live
                result.lnNoise = logaddexp(result.lnNoise, c.lnNoise)
            for c in prods:
                c._pendT = None
            result.parts = {"1": t0, "s": t1, "s2": t2}
        result.reLinearize()
        return result

    @staticmethod
    def linearCombination(terms, free=0, fused=None):
        """sum_t c_t * ct_t + free for terms = [(ct, integer)]: the loop of simplePolyEval (src/polyEval.cpp:227-253) --
        ret.clear(); per term tmp = ct; tmp.multByConstant(c); ret += tmp; then ret.addConstant(free) -- as a new
        ciphertext.  Fused: the same steps on the bookkeeping alone (the plaintext spaces' gcd, the union of the prime
        sets, _alignForAdd's (e1, e2), lnNoise, ptxtMag and intFactor, float operation for float operation), collecting
        per term the integers the steps would have multiplied into its words -- the balanced gcd of multByScalar, the
        product of the added primes whenever a side is modded up, bal(e2) on the new term and bal(e1) on everything
        before it -- then one ops.linComb (hx_lin_comb) with those products reduced modulo every output prime.  It
        applies to a BGV context when every surviving term holds the canonical parts {1, s}, or all hold the same single
        part, at most 256 of them, on a backend with linComb; otherwise, and with fused=False, the sequence runs as it
        is.  fused=True insists on a backend with linComb; fused=None follows Ctxt.fuseLinComb.  Words, lnNoise,
        primeSet, ptxtSpace, intFactor and ptxtMag are the same either way; the terms are left as they were."""
        if not terms:
            raise ValueError("linearCombination of no terms")
        first = terms[0][0]
        has = hasattr(first.ops, "linComb")
        if fused and not has:
            raise RuntimeError("Ctxt::linearCombination: fused=True, but this backend has no linComb")
        want = (Ctxt.fuseLinComb if fused is None else fused) and has
        if want:
            ret = Ctxt._linCombFused(terms, free)
            if ret is not None:
                return ret
        ret = first._emptyLike()
        for ct, c in terms:
            tmp = ct.clone()
            tmp.multByScalar(c)
            ret += tmp
        ret.addScalar(free)
        return ret

    @staticmethod
    def _linCombFused(terms, free):
        """linearCombination's fused form, or None where it does not apply (nothing has been touched then)"""
        first = terms[0][0]
        ctx = first.context
        if ctx.ckks:
            return None
        live = []                                        # (ct, c mod its space), the terms multByScalar leaves with parts
        for ct, c in terms:
            if isinstance(c, float):
                raise TypeError("multByConstant(double) not supported for BGV")
            ct._materializeTensor()
            if ct.parts and int(c) % ct.ptxtSpace != 0:
                live.append((ct, int(c) % ct.ptxtSpace))
        if not live or len(live) > 256:
            return None
        hs = sorted(live[0][0].parts, key=str)
        if not (hs == ["1", "s"] or len(hs) == 1):
            return None
        for ct, _ in live:
            if sorted(ct.parts, key=str) != hs:
                return None
            ix = ct.parts[hs[0]].getIndexSet()
            if any(ct.parts[h].getIndexSet() != ix for h in hs[1:]):
                return None
        # the running sum's bookkeeping, and per term the integer its words are multiplied by
        mult = []
        P = ps = fac = ln = mag = idx = None
        for ct, c0 in live:
            tP, tf, tln, tmag, tps, m = ct.ptxtSpace, ct.intFactor, ct.lnNoise, ct.ptxtMag, ct.primeSet, 1
            if c0 != 1:                                                   # multByScalar
                d = math.gcd(c0, tP)
                tf = tf * pow(c0 // d, -1, tP) % tP
                if d != 1:
                    cc = d - tP if d > tP // 2 else d
                    tln = tln + math.log(abs(cc))
                    m *= cc
            if P is None:                                                 # ret += tmp into the empty ret
                P, ps, fac, ln, mag = tP, tps, tf, tln, tmag
                idx = ct.parts[hs[0]].getIndexSet()
                mult.append(m)
                continue
            g = math.gcd(P, tP)                                           # _alignForAdd
            if g <= 1:
                raise ValueError("New and old plaintext spaces are coprime")
            P, fac = g, fac % g
            if tP != g:
                tf %= g
            up = sorted(tps - ps)
            if up:                                                        # the sum is modded up
                ln = ln + ctx.logOfProduct(up)
                ps = ps | frozenset(up)
                idx = idx + up
                prod = ctx.productOfPrimes(up)
                mult = [x * prod for x in mult]
            up = sorted(ps - tps)
            if up:                                                        # the term is modded up
                tln = tln + ctx.logOfProduct(up)
                m *= ctx.productOfPrimes(up)
            e1 = e2 = 1
            if fac != tf:
                e1, e2 = Ctxt._intFactorPair(ctx.p, P, fac, ln, tf, tln)
            bal = lambda e: e - P if e > P // 2 else e                    # noqa: E731  (mulIntFactor's)
            if e2 != 1:                                                   # o.mulIntFactor(e2)
                m *= bal(e2)
                tln = tln + math.log(abs(bal(e2)))
            if e1 != 1:                                                   # self.mulIntFactor(e1)
                fac = fac * e1 % P
                mult = [x * bal(e1) for x in mult]
                ln = ln + math.log(abs(bal(e1)))
            mag += tmag                                                   # the sum
            ln = logaddexp(ln, tln)
            mult.append(m)
        cc = int(free) % P                                                # addScalar
        if cc > P // 2:
            cc -= P
        addend = None
        if cc != 0:
            if hs != ["1", "s"] and hs != ["1"]:
                return None
            f = 1
            if P > 2:
                f = ctx.productOfPrimes(ps) % P * fac % P
                if f > P // 2:
                    f -= P
            ln = logaddexp(ln, _ln(float(abs(cc)) * abs(f)))
            addend = [cc * f % ctx.primes[i] for i in idx]
        w = [[x % ctx.primes[i] for i in idx] for x in mult]
        in0 = [ct.parts[hs[0]] for ct, _ in live]
        in1 = [ct.parts[hs[1]] for ct, _ in live] if len(hs) == 2 else None
        out0, out1 = first.ops.linComb(in0, in1, idx, w, addend)
        ret = live[0][0]._emptyLike()
        ret.parts = {hs[0]: out0}
        if len(hs) == 2:
            ret.parts[hs[1]] = out1
        ret.ptxtSpace, ret.primeSet, ret.intFactor, ret.ptxtMag = P, ps, fac, mag
        ret.lnNoise = ln
        return ret

    fuseCirculant = False  # fused=None: the call sequence until hx_mul_add_circulant has been measured as the faster form

    @staticmethod
    def circulantCombination(cts, consts, n=None, size=-1.0, fused=None):
        """out[i] = sum_j consts[(i + j) mod d] * cts[j] for i < n <= d = len(cts) = len(consts), as n new ciphertexts:
        the loop of unpack (src/intraSlot.cpp:107-116) -- out[i] = cts[0]; out[i].multByConstant(consts[i]); then per
        j >= 1 tmp = cts[j]; tmp.multByConstant(consts[(i + j) mod d]); out[i] += tmp.  consts are DoubleCRTs on a
        superset of every term's primes, `size` their multByConstant size (< 0: the default bound).
        Fused: the same steps once on parts that hold no rows and only record the integers the steps would have
        multiplied into each term's words (bal(e2) on the new term and bal(e1) on everything before it when addCtxt
        harmonises the intFactors; the mod-ups are exact scalings too) -- every out[i] has the same bookkeeping, the
        constants differing in their words alone -- then per term at most one mod-up to the union of the prime sets and
        one product by its integer, and one ops.mulAddCirculant (hx_mul_add_circulant) for the d^2 multiply-adds.  Exact
        sums modulo a prime do not depend on their order: words, lnNoise, primeSet, ptxtSpace, intFactor and ptxtMag are
        those of the sequence.  It applies to a BGV context when every term holds the canonical parts {1, s}, or all the
        same single part, d <= 64, on a backend with mulAddCirculant; otherwise, and with fused=False, the sequence
        runs as it is.  fused=True insists on such a backend; fused=None follows Ctxt.fuseCirculant.  The terms are left
        as they were."""
        d = len(cts)
        if d < 1 or len(consts) != d:
            raise ValueError("circulantCombination takes d >= 1 ciphertexts and d constants")
        n = d if n is None else int(n)
        if not 1 <= n <= d:
            raise ValueError("circulantCombination: 1 <= n <= d")
        has = hasattr(cts[0].ops, "mulAddCirculant")
        if fused and not has:
            raise RuntimeError("Ctxt::circulantCombination: fused=True, but this backend has no mulAddCirculant")
        if (Ctxt.fuseCirculant if fused is None else fused) and has:
            out = Ctxt._circulantFused(cts, consts, n, size)
            if out is not None:
                return out
        out = []
        for i in range(n):
            u = cts[0].clone()
            u.multByConstant(consts[i], size)
            for j in range(1, d):
                tmp = cts[j].clone()
                tmp.multByConstant(consts[(i + j) % d], size)
                u += tmp
            out.append(u)
        return out

    @staticmethod
    def _circulantFused(cts, consts, n, size):
        """circulantCombination's fused form, or None where it does not apply (nothing has been touched then)"""
        d, ctx, ops = len(cts), cts[0].context, cts[0].ops
        if ctx.ckks or d > 64:
            return None
        for ct in cts:
            ct._materializeTensor()
        hs = sorted(cts[0].parts, key=str)
        if not (hs == ["1", "s"] or len(hs) == 1):
            return None
        for ct in cts:
            if sorted(ct.parts, key=str) != hs:
                return None
            ix = ct.parts[hs[0]].getIndexSet()
            if any(ct.parts[h].getIndexSet() != ix for h in hs[1:]):
                return None

        class Track:
            """a part without rows: term -> the integer its words have been multiplied by so far"""

            def __init__(self, mult):
                self.mult = dict(mult)

            def copy(self):
                return Track(self.mult)

            def __imul__(self, o):                       # a constant: its words are the kernel's to multiply in
                if isinstance(o, (int, float, complex)):
                    raise _NotTracked("*= number")
                return self

            def __getattr__(self, name):                 # anything else the sequence might do needs the rows
                raise _NotTracked(name)

            def mulConstant(self, c):
                self.mult = {j: m * int(c) for j, m in self.mult.items()}
                return self

            def addPrimesAndScale(self, s):              # exact: done on the term's own rows below
                return self

            def __iadd__(self, o):
                for j, m in o.mult.items():
                    self.mult[j] = self.mult.get(j, 0) + m
                return self

        def shadow(j):
            ct = cts[j]
            c = Ctxt(ctx, ops, ct.ksw, ct.ksw_ptxtSpace, ct.ksw_lnNoise)
            c.primeSet, c.ptxtSpace, c.intFactor = ct.primeSet, ct.ptxtSpace, ct.intFactor
            c.lnNoise, c.ptxtMag, c.lnRatFactor = ct.lnNoise, ct.ptxtMag, ct.lnRatFactor
            c.parts = {h: Track({j: 1}) for h in hs}
            return c
        try:
            su = shadow(0)
            su.multByConstant(None, size)
            for j in range(1, d):
                tmp = shadow(j)
                tmp.multByConstant(None, size)
                su += tmp
        except _NotTracked:
            return None
        mult = su.parts[hs[0]].mult
        union = su.primeSet
        terms = []
        for j, ct in enumerate(cts):
            m = mult[j]
            if ct.primeSet != union or m != 1:
                ct = ct.clone()
                ct.modUpToSet(union)
                for p in ct.parts.values():
                    p.mulConstant(m)
            terms.append(ct)
        idx = terms[0].parts[hs[0]].getIndexSet()
        if any(t.parts[h].getIndexSet() != idx for t in terms for h in hs):
            return None                                   # the rows of the terms are in different orders
        make = getattr(ops, "likeUninit", None) or ops.zerosLike
        outs = [[make(terms[0].parts[h]) for _ in range(n)] for h in hs]
        ops.mulAddCirculant(outs[0], outs[1] if len(hs) == 2 else None, list(consts), [t.parts[hs[0]] for t in terms],
                            [t.parts[hs[1]] for t in terms] if len(hs) == 2 else None)
        res = []
        for i in range(n):
            c = cts[0]._emptyLike()
            c.parts = {h: outs[k][i] for k, h in enumerate(hs)}
            c.primeSet, c.ptxtSpace, c.intFactor = su.primeSet, su.ptxtSpace, su.intFactor
            c.ptxtMag, c.lnRatFactor = su.ptxtMag, su.lnRatFactor
            c.lnNoise = su.lnNoise
            res.append(c)
        return res

    def cleanUp(self):
        """Ctxt::cleanUp (src/Ctxt.cpp:788-797)"""
        self.reLinearize()
        ctx = self.context
        if self.primeSet & (frozenset(ctx.specialPrimes) | frozenset(ctx.smallPrimes)):
            self.dropSmallAndSpecialPrimes()
        return self


class _NotTracked(Exception):
    """a step of the call sequence that Ctxt._circulantFused's row-less parts cannot record: the sequence runs instead"""


class DynamicCtxtPowers:
    """DynamicCtxtPowers (include/helib/polyEval.h:59-130, src/polyEval.cpp:18-29): the powers of one ciphertext,
    computed when first asked for -- X^e = X^(e-k) * X^k with k the largest power of two below e -- so every power is
    formed once and X^e sits at depth ceil(log2 e).  stats, if given, counts the products in stats["mults"] and
    records (name, e) in stats["powers"]."""

    def __init__(self, x, nPowers, stats=None, name=""):
        if nPowers < 1:
            raise ValueError("Zero or negative nPowers")
        self.v = [None] * nPowers
        self.v[0] = x.clone()
        self.stats, self.name = stats, name

    def size(self):
        return len(self.v)

    def wasComputed(self, e):
        return 1 <= e <= len(self.v) and self.v[e - 1] is not None

    def getPower(self, e):
        if e < 1 or e > len(self.v):
            raise IndexError("DynamicCtxtPowers: power %d of %d" % (e, len(self.v)))
        if self.v[e - 1] is None:
            k = 1 << ((e - 1).bit_length() - 1)      # NextPowerOfTwo(e) - 1
            c = self.getPower(e - k).clone()
            c.multiplyBy(self.getPower(k))
            self.v[e - 1] = c
            if self.stats is not None:
                self.stats["mults"] += 1
                self.stats["powers"].add((self.name, e))
        return self.v[e - 1]


class BasicAutomorphPrecon:
    """Hoisting (src/matmul.cpp:48-184): break the `s` part of a ciphertext into digits ONCE, then
    every automorphism rotates the digits (a permutation of evaluation rows, hx_automorph on the
    whole digit block) and key-switches them with the matrix of that automorphism -- no inverse
    transform, no basis extension and no forward transforms per rotation.  As in the reference the
    matrix for k itself must be available (the generator-tree walk of PubKey::getNextKSWmatrix is
    key management and stays with the caller)."""

    def __init__(self, ct):
        self.ctxt = ct.clone()
        self.polyDigits, self.lnNoise = None, 0.0
        c = self.ctxt
        if len(c.parts) <= 1:
            return
        c.cleanUp()
        assert set(c.parts) == {"1", "s"}, "Ciphertext is not in canonical form"
        ctx = c.context
        sp = list(ctx.specialPrimes)
        digits = [[i for i in d if i in c.primeSet] for d in ctx.digits]
        self.digits = [d for d in digits if d]
        if c._meas:
            self.polyDigits, nrm = c.ops.breakIntoDigits(c.parts["s"], self.digits, sp, norms=True)
        else:
            self.polyDigits, nrm = c.ops.breakIntoDigits(c.parts["s"], self.digits, sp), None
        # addedNoise = breakIntoDigits' return value * max over the matrices' noise bounds
        # (src/matmul.cpp:91-97); noise = ctxt.noise * P + addedNoise (:99-112)
        added = -math.inf
        for k, d in enumerate(self.digits):
            nb = _ln(float(max(nrm[k]))) if nrm is not None else math.log(ctx.noiseBoundForUniform(0.5, ctx.phim))
            added = logaddexp(added, nb + ctx.logOfProduct(d))
        added += c.ksw_lnNoise
        self.lnNoise = logaddexp(c.lnNoise + ctx.logOfProduct(sp), added)

    def automorph(self, k):
        c = self.ctxt
        ctx = c.context
        k %= ctx.m
        if k == 1 or not c.parts:
            return c.clone()
        if math.gcd(k, ctx.m) != 1:
            raise ValueError("k must be in Zm*")
        sp = list(ctx.specialPrimes)
        res = Ctxt(ctx, c.ops, c.ksw, c.ksw_ptxtSpace, c.ksw_lnNoise)
        res.ksw_auto = c.ksw_auto
        res.ptxtSpace, res.intFactor = c.ptxtSpace, c.intFactor
        res.primeSet = c.primeSet | frozenset(sp)
        if ctx.ckks:                   # src/matmul.cpp:139-143: the factor grows with the special primes
            res.ptxtMag = c.ptxtMag
            res.lnRatFactor = c.lnRatFactor + ctx.logOfProduct(sp)
        part0 = c.parts["1"].copy()
        part0.automorph(k)
        part0.addPrimesAndScale(sp)
        res.ksw_map = c.ksw_map
        if len(c.parts) == 1:        # only the constant part: nothing to key-switch (:145-151)
            res.parts = {"1": part0}
            res.lnNoise = c.lnNoise + ctx.logOfProduct(sp)
            return res
        amt = c._firstStep(k)          # first key-switching matrix on the way to k (:153-162)
        W = c.ksw_auto[amt]
        if amt != k:                   # the constant part was rotated by k above: redo it by amt
            part0 = c.parts["1"].copy()
            part0.automorph(amt)
            part0.addPrimesAndScale(sp)
        dg = self.polyDigits.copy()
        dg.automorph(amt)
        part1 = c.ops.zerosLike(part0)
        c.ops.keySwitchDigits(dg, W, part0, part1)
        res.parts = {"1": part0, "s": part1}
        res.lnNoise = self.lnNoise
        res.ksw_map = c.ksw_map
        if amt != k:                   # more automorphisms to do: the usual smartAutomorph (:177-181)
            res.smartAutomorph(k * pow(amt, -1, ctx.m) % ctx.m)
        return res

    def automorphSum(self, ks, fused=None):
        """The ciphertext plus its images under the automorphisms ks, as a new ciphertext: the hoisted loop of traceMap
        (src/matmul.cpp:2878-2887), acc = ctxt; acc += *precon.automorph(k) for every k.  Fused: one ops.hoistedSum
        (hx_hoisted_automorph_sum) over the digit block, with the loop's bookkeeping -- the mod-up of acc by the special
        primes at the first sum, then logaddexp per term -- float operation for float operation.  It applies to a BGV
        ciphertext with the parts {1, s} when every k has a matrix of its own (_firstStep(k) = k) and the terms fit the
        kernel's accumulators; otherwise, and with fused=False, the loop runs as it is.  fused=True insists on a backend
        with hoistedSum; fused=None follows Ctxt.fuseHoistedSum.  Words, lnNoise, primeSet, ptxtSpace, intFactor and the
        part handles are the same either way."""
        c = self.ctxt
        has = hasattr(c.ops, "hoistedSum")
        if fused and not has:
            raise RuntimeError("BasicAutomorphPrecon::automorphSum: fused=True, but this backend has no hoistedSum")
        if (Ctxt.fuseHoistedSum if fused is None else fused) and has:
            ret = self._sumFused(ks)
            if ret is not None:
                return ret
        acc = c.clone()
        for k in ks:
            acc += self.automorph(k)
        return acc

    def _sumFused(self, ks):
        """automorphSum's fused form, or None where it does not apply (nothing has been touched then)"""
        c = self.ctxt
        ctx = c.context
        sp = list(ctx.specialPrimes)
        if ctx.ckks or self.polyDigits is None or set(c.parts) != {"1", "s"} or c.primeSet & frozenset(sp):
            return None
        ks = [k % ctx.m for k in ks]
        if not ks or any(k == 1 or math.gcd(k, ctx.m) != 1 or c._firstStep(k) != k for k in ks):
            return None
        if len(ks) * (len(self.digits) + 1) + 1 > 256:          # the accumulators of hx_hoisted_automorph_sum
            return None
        out0, out1 = c.ops.hoistedSum(self.polyDigits, c.parts["1"], c.parts["s"], ks, [c.ksw_auto[k] for k in ks], sp)
        res = Ctxt(ctx, c.ops, c.ksw, c.ksw_ptxtSpace, c.ksw_lnNoise)
        res.ksw_auto, res.ksw_pow, res.ksw_map, res._like = c.ksw_auto, c.ksw_pow, c.ksw_map, c._like
        res.ptxtSpace, res.intFactor = c.ptxtSpace, c.intFactor
        res.parts = {"1": out0, "s": out1}
        logProd = ctx.logOfProduct(sorted(sp))
        ln, mag = c.lnNoise + logProd, c.ptxtMag                # acc.modUpToSet at the first sum
        for _ in ks:                                            # addCtxt: equal spaces, prime sets and intFactors
            mag += res.ptxtMag                                  # (a term's ptxtMag is the constructor's)
            ln = logaddexp(ln, self.lnNoise)
        res.ptxtMag, res.lnRatFactor = mag, c.lnRatFactor + logProd
        res.lnNoise = ln
        res.primeSet = c.primeSet | frozenset(sp)
        return res

    def automorphMasked(self, ks, A, B, sizes, fused=None):
        """For every t the ciphertext A[t] * ctxt + B[t] * precon.automorph(ks[t]), as a list of new ciphertexts: an
        inner node of replicateAll's recursion (src/replicate.cpp:432-483) with both rotations taken from this one digit
        decomposition.  A[t], B[t]: constants as Ctxt.multByConstant takes them (DoubleCRTs that may live on more
        primes), None for no product; sizes[t] = (size of A[t], size of B[t]), a negative size being multByConstant's
        default.  Unfused, per term: r = automorph(k); r.multByConstant(B, sizeB); a = ctxt.clone();
        a.multByConstant(A, sizeA); a += r.  Fused: one ops.hoistedMaskFan (hx_hoisted_mask_fan) for all terms, with that
        sequence's bookkeeping float operation for float operation.  It applies where _sumFused applies (BGV, the parts
        {1, s}, every k with a matrix of its own, no special primes in the operand); otherwise, and with fused=False,
        the sequence runs.  fused=True insists on a backend with hoistedMaskFan; fused=None follows Ctxt.fuseHoistedFan.
        Words, lnNoise, primeSet, ptxtSpace, intFactor, ptxtMag and the part handles are the same either way."""
        c = self.ctxt
        n = len(ks)
        A = [None] * n if A is None else list(A)
        B = [None] * n if B is None else list(B)
        sizes = [(-1.0, -1.0)] * n if sizes is None else list(sizes)
        if not len(A) == len(B) == len(sizes) == n:
            raise ValueError("automorphMasked: one A, one B and one pair of sizes per automorphism")
        has = hasattr(c.ops, "hoistedMaskFan")
        if fused and not has:
            raise RuntimeError("BasicAutomorphPrecon::automorphMasked: fused=True, but this backend has no hoistedMaskFan")
        if (Ctxt.fuseHoistedFan if fused is None else fused) and has:
            ret = self._maskedFused(ks, A, B, sizes)
            if ret is not None:
                return ret
        out = []
        for k, a_t, b_t, (sa, sb) in zip(ks, A, B, sizes):
            r = self.automorph(k)
            if b_t is not None:
                r.multByConstant(b_t, sb)
            a = c.clone()
            if a_t is not None:
                a.multByConstant(a_t, sa)
            a += r
            out.append(a)
        return out

    def _maskedFused(self, ks, A, B, sizes):
        """automorphMasked's fused form, or None where it does not apply (nothing has been touched then)"""
        c = self.ctxt
        ctx = c.context
        sp = list(ctx.specialPrimes)
        if ctx.ckks or self.polyDigits is None or set(c.parts) != {"1", "s"} or c.primeSet & frozenset(sp):
            return None
        ks = [k % ctx.m for k in ks]
        if not ks or len(ks) > 256 or any(k == 1 or math.gcd(k, ctx.m) != 1 or c._firstStep(k) != k for k in ks):
            return None
        out0, out1 = c.ops.hoistedMaskFan(self.polyDigits, c.parts["1"], c.parts["s"], ks, [c.ksw_auto[k] for k in ks],
                                          A, B, sp)
        logProd = ctx.logOfProduct(sorted(sp))
        defSize = ctx.noiseBoundForMod(c.ptxtSpace, ctx.phim)   # multByConstant's size < 0
        res = []
        for t in range(len(ks)):
            x = Ctxt(ctx, c.ops, c.ksw, c.ksw_ptxtSpace, c.ksw_lnNoise)
            x.ksw_auto, x.ksw_pow, x.ksw_map, x._like = c.ksw_auto, c.ksw_pow, c.ksw_map, c._like
            x.ptxtSpace, x.intFactor = c.ptxtSpace, c.intFactor
            x.parts = {"1": out0[t], "s": out1[t]}
            sa, sb = sizes[t]
            lr = self.lnNoise                                   # r = automorph(k)
            if B[t] is not None:                                # r.multByConstant(B, sizeB)
                lr = lr + _ln(defSize if sb < 0.0 else sb)
            la = c.lnNoise                                      # a = ctxt.clone(); a.multByConstant(A, sizeA)
            if A[t] is not None:
                la = la + _ln(defSize if sa < 0.0 else sa)
            la += logProd                                       # a += r: a.modUpToSet, then addCtxt's sums
            x.ptxtMag, x.lnRatFactor = c.ptxtMag + x.ptxtMag, c.lnRatFactor + logProd
            x.lnNoise = logaddexp(la, lr)
            x.primeSet = c.primeSet | frozenset(sp)
            res.append(x)
        return res


def automorphBlend(pre, pre1, ks, masks, sizes, fused=None):
    """For every t the ciphertext m * pre.automorph(k) + pre1.automorph(k) - m * pre1.automorph(k), k = ks[t], m =
    masks[t], as a list of new ciphertexts: the inner step of MatMulFullExec::rec_mul along a non-native dimension
    (src/matmul.cpp:2186-2200) over the two BasicAutomorphPrecon of ctxt and of ctxt moved by g^(-ord).  masks[t]: a
    constant as Ctxt.multByConstant takes it (a DoubleCRT that may live on more primes); sizes[t]: its size, negative for
    multByConstant's default.  Unfused, per term: tmp = pre.automorph(k); tmp1 = pre1.automorph(k);
    tmp.multByConstant(m, sz); tmp += tmp1; tmp1.multByConstant(m, sz); tmp -= tmp1.  Fused: one ops.hoistedBlend
    (hx_hoisted_blend) for all terms, with that sequence's bookkeeping float operation for float operation.  It applies
    to two BGV precons with digits and the parts {1, s} on one prime set without special primes, with the same digit
    split, ptxtSpace and intFactor (at p > 2 the key switch that made pre1's ciphertext can leave another intFactor, and
    addCtxt then rescales), every k other than 1 with a matrix of its own, n <= 256; otherwise, and with fused=False, the
    sequence runs.  fused=True insists on a backend with hoistedBlend; fused=None follows Ctxt.fuseHoistedBlend.  Words,
    lnNoise, primeSet, ptxtSpace, intFactor, ptxtMag and the part handles are the same either way."""
    n = len(ks)
    masks, sizes = list(masks), [-1.0] * n if sizes is None else list(sizes)
    if not len(masks) == len(sizes) == n or any(mk is None for mk in masks):
        raise ValueError("automorphBlend: one mask and one size per automorphism")
    c = pre.ctxt
    has = hasattr(c.ops, "hoistedBlend")
    if fused and not has:
        raise RuntimeError("automorphBlend: fused=True, but this backend has no hoistedBlend")
    if (Ctxt.fuseHoistedBlend if fused is None else fused) and has:
        ret = _blendFused(pre, pre1, ks, masks, sizes)
        if ret is not None:
            return ret
    out = []
    for k, mk, sz in zip(ks, masks, sizes):
        tmp, tmp1 = pre.automorph(k), pre1.automorph(k)
        tmp.multByConstant(mk, sz)
        tmp += tmp1
        tmp1.multByConstant(mk, sz)
        tmp -= tmp1
        out.append(tmp)
    return out


def _blendFused(pre, pre1, ks, masks, sizes):
    """automorphBlend's fused form, or None where it does not apply (nothing has been touched then)"""
    c, c1 = pre.ctxt, pre1.ctxt
    ctx = c.context
    sp = list(ctx.specialPrimes)
    if ctx.ckks or c1.context is not ctx or pre.polyDigits is None or pre1.polyDigits is None:
        return None
    if set(c.parts) != {"1", "s"} or set(c1.parts) != {"1", "s"} or c.primeSet != c1.primeSet or c.primeSet & frozenset(sp):
        return None
    if pre.digits != pre1.digits or c.ptxtSpace != c1.ptxtSpace or c.intFactor != c1.intFactor:
        return None
    if c.ksw_auto is not c1.ksw_auto or c.ksw_map is not c1.ksw_map:
        return None
    ks = [k % ctx.m for k in ks]
    if not ks or len(ks) > 256 or any(k == 1 or math.gcd(k, ctx.m) != 1 or c._firstStep(k) != k for k in ks):
        return None
    out0, out1 = c.ops.hoistedBlend(pre.polyDigits, c.parts["1"], c.parts["s"], pre1.polyDigits, c1.parts["1"],
                                    c1.parts["s"], ks, [c.ksw_auto[k] for k in ks], masks, sp)
    defSize = ctx.noiseBoundForMod(c.ptxtSpace, ctx.phim)       # multByConstant's size < 0
    res = []
    for t in range(len(ks)):
        x = Ctxt(ctx, c.ops, c.ksw, c.ksw_ptxtSpace, c.ksw_lnNoise)
        x.ksw_auto, x.ksw_pow, x.ksw_map, x._like = c.ksw_auto, c.ksw_pow, c.ksw_map, c._like
        x.ptxtSpace, x.intFactor = c.ptxtSpace, c.intFactor
        x.parts = {"1": out0[t], "s": out1[t]}
        lsz = _ln(defSize if sizes[t] < 0.0 else sizes[t])
        mag1 = x.ptxtMag                                        # (an automorph's ptxtMag is the constructor's)
        ln = pre.lnNoise + lsz                                  # tmp.multByConstant(m, sz)
        x.ptxtMag += mag1                                       # tmp += tmp1
        ln = logaddexp(ln, pre1.lnNoise)
        ln1 = pre1.lnNoise + lsz                                # tmp1.multByConstant(m, sz): the bound alone
        x.ptxtMag += mag1                                       # tmp -= tmp1
        x.lnNoise = logaddexp(ln, ln1)
        x.primeSet = c.primeSet | frozenset(sp)
        res.append(x)
    return res


# ---------------------------------------------------------------------------------------------
# products of many ciphertexts (src/Ctxt.cpp:2803-2904)
# ---------------------------------------------------------------------------------------------
def _split(n):
    """n1 = the highest power of two below n (n/2 <= n1 < n): NumBits(n - 1) = l, n1 = 2^(l-1)"""
    return 1 << ((n - 1).bit_length() - 1)


def incrementalProduct(v):
    """For i = n-1 .. 0: v[i] = prod_{j <= i} v[j], depth log n and (n log n)/2 products, in place."""
    def rec(lo, n):
        if n <= 1:
            return
        n1 = _split(n)
        rec(lo, n1)
        rec(lo + n1, n - n1)
        for i in range(lo + n1, lo + n):
            v[i].multiplyBy(v[lo + n1 - 1])
    rec(0, len(v))


def totalProduct(v):
    """prod_i v[i] in depth log n with n-1 products (triples through multiplyBy2); a new Ctxt."""
    def rec(lo, n):
        out = v[lo].clone()
        if n == 2:
            out.multiplyBy(v[lo + 1])
        elif n == 3:
            out.multiplyBy2(v[lo + 1], v[lo + 2])
        elif n > 3:
            n1 = _split(n)
            out = rec(lo, n1)
            out.multiplyBy(rec(lo + n1, n - n1))
        return out
    if not v:
        raise ValueError("totalProduct of an empty vector")
    return rec(0, len(v))


def innerProduct(v1, v2):
    """sum_i v1[i] * v2[i] with the low-level product and ONE relinearisation at the end"""
    n = min(len(v1), len(v2))
    if n <= 0:
        raise ValueError("innerProduct of empty vectors")
    result = v1[0].clone()
    result.multLowLvl(v2[0])
    for i in range(1, n):
        tmp = v1[i].clone()
        tmp.multLowLvl(v2[i])
        result.addCtxt(tmp)
    result.reLinearize()
    return result
