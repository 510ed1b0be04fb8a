"""Recryption (src/recryption.cpp of the reference): PubKey::reCrypt (:367-545) over this library.

  ChainContext(bootstrappable=True) helib_amd.ctxt: cc.e, cc.ePrime (RecryptData::setAE, :200-256), skHwt 120, the
                                    special primes sized for p^(r + e - e')
  SecKey.genRecryptData(rc)         helib_amd.keys (src/keys.cpp:1678-1713): the second key, the matrix from key 0 to
                                    it, recryptEkey
  RecryptData(cc, g, mvec, gens, ords, maps=True)
                                    (:270-351) e, e', q = p^e + 1, p^e', the PowerfulDCRT of mvec; with maps the array
                                    over p^(e - e' + r) (arrayAt), unpackSlotEncoding, firstMap, secondMap
  arrayAt(cc, g, r)                 bgv_gr.EncryptedArray over the chain at an exponent of the caller's choosing
  rawModSwitch(ct, rc, seed)        per part: p2dConv.coefficientCube (copy, iFFT, dcrtToPowerful), ops.recryptPrep
                                    (hx_recrypt_prep: Ctxt::rawModSwitch, src/Ctxt.cpp:2949-3049, newMakeDivisible,
                                    :73-136, and the division by p^e', :495-497, in one kernel), p2dConv.fromCube
                                    (powerfulToDCRT, FFT) -> the two constants zzParts[0], zzParts[1] as DoubleCRTs in
                                    evaluation form on the primes of the encrypted recryption key, and the scaled-noise
                                    estimate noiseBound q / Q.  Nothing leaves the device.
  preProcess(ct, rc, seed)          rawModSwitch behind the check reCrypt makes on its noise estimate (:440-463):
                                    LogicError, as the non-debug reference, with the "raw-mod-switch-noise" sample
  extractDigitsThin(ea, ct, botHigh, r, ePrime)
                                    the digit extraction on thinly packed slots (:793-909), both branches with the
                                    reference's cost rule (useChenHan), over polyeval.extractDigits / extendExtractDigits
  extractDigitsPacked(rc, ct, botHigh, r, ePrime)
                                    (:646-720) intraslot.unpack, extractDigitsThin on each of the d, X^i in every slot
  reCrypt(ct, pk, rc, seed)         the whole operation, inside the reference's named timers

The reference goes powerful -> polynomial basis after the mod-switch, back for newMakeDivisible and to the polynomial
basis again before it divides; the conversions are integer-linear and inverse to each other on integers this small, so
the kernel does all the per-coefficient steps on the cube and the cube is converted once (include/helib_amd.h has the
argument).  Its ties are NTL::RandomBnd(2); here they are a counter-based function of `seed` (recrypt_core.h), so a
call is reproducible from its seed.

What a backend supplies: ops.recryptPrep(poly, out_set, q, p, p2r, p2ePrime, seed, part) on coefficient rows
(helib_amd.capi's on the device; the tests' oracle backend states it in Python integers), and the conversions through
the p2dConv object RecryptData is given or builds.

  ThinRecryptData(cc, g, mvec, gens, ords, alsoThick=False)
                                    (:773-787) RecryptData with coeffToSlot / slotToCoeff, the two
                                    helib_amd.thin_evalmap.ThinEvalMap; the packed maps only with alsoThick
  thinReCrypt(ct, pk, rc, seed)     (:940-1128) for slots that hold integers modulo p^r: drop to three primes,
                                    slotToCoeff, the shared tail of preProcess, coeffToSlot (with traceMap),
                                    extractDigitsThin once -- inside the reference's named timers

Not built: packedRecrypt, the dummy-ciphertext branch of reCrypt and thinReCrypt (helib_amd.evalmap.reCrypt keeps its
refusal).  Nothing here imports oracle/."""
import copy
import math

import numpy as np

from . import intraslot, polyeval, powerful, timing
from .ckks import LogicError

HELIB_MIN_CAP_FRAC = 2.0 / 3.0      # include/helib/recryption.h:112: the fraction of the capacity the noise may take


class RecryptData:
    """The parameters of recryption for one bootstrappable chain and one factorisation of m (RecryptData::init,
    src/recryption.cpp:270-314): e, ePrime, skHwt from the chain; q = p^e + 1; p2ePrime = p^e'; p2dConv, the
    PowerfulDCRT of mvec over the capi.Context g holding the chain's primes (None: no device, parameters only)."""

    def __init__(self, cc, g, mvec, gens=None, ords=None, ea=None, ea_boot=None, p2dConv=None, maps=False):
        if getattr(cc, "ckks", False) or not getattr(cc, "bootstrappable", False):
            raise LogicError("RecryptData: the chain was not built with bootstrappable=True (e and e' are not set)")
        self.cc, self.g = cc, g
        self.mvec = [int(x) for x in mvec]
        m = 1
        for x in self.mvec:
            m *= x
        if m != cc.m:
            raise LogicError("Cyclotomic polynomial mismatch: the factors multiply to %d, m = %d" % (m, cc.m))
        self.gens, self.ords = gens, ords
        self.skHwt, self.e, self.ePrime = cc.hwt, cc.e, cc.ePrime
        self.p, self.r = cc.p, cc.r
        self.p2r = cc.p ** cc.r
        self.q = cc.p ** cc.e + 1
        self.p2ePrime = cc.p ** cc.ePrime
        if self.e < self.r:
            raise LogicError("rcData.e must be at least alMod.r")
        self.p2dConv = p2dConv if p2dConv is not None else (powerful.PowerfulDCRT(g, self.mvec) if g is not None else None)
        self.ea, self.ea_boot = ea, ea_boot
        self.unpackSlotEncoding = self.firstMap = self.secondMap = None
        if maps or ea is not None or ea_boot is not None:
            self.buildMaps()

    def buildMaps(self):
        """the rest of RecryptData::init (:309-350): the array over p^(e - e' + r), the constants of unpack, firstMap =
        EvalMap(ea_boot, mvec, invert, normal basis) and secondMap = EvalMap(ea, mvec).  An array that was not handed
        in is built on the device over gens / ords."""
        from . import evalmap
        if self.ea is None:
            self.ea = arrayAt(self.cc, self.g, self.r, gens=self.gens, ords=self.ords)
        if self.ea_boot is None:
            self.ea_boot = arrayAt(self.cc, self.g, self.e - self.ePrime + self.r, gens=self.gens, ords=self.ords)
        self.unpackSlotEncoding = intraslot.buildUnpackSlotEncoding(self.ea_boot)
        self.firstMap = evalmap.EvalMap(self.ea_boot, self.mvec, invert=True, normal_basis=True)
        self.secondMap = evalmap.EvalMap(self.ea, self.mvec)
        return self


def arrayAt(cc, g, r, encoder=None, gens=None, ords=None):
    """bgv_gr.EncryptedArray over the chain cc with slots modulo p^r for an r of the caller's choosing (the class takes
    its exponent from the context it is built over: it is built over a view of cc at that r and then pointed back at
    cc, whose primes and keys it works with)"""
    from . import bgv_gr
    view = copy.copy(cc)
    view.r, view.ptxtSpace = int(r), cc.p ** int(r)
    ea = bgv_gr.EncryptedArray(view, g, encoder=encoder, gens=gens, ords=ords) if encoder is None else \
        bgv_gr.EncryptedArray(view, g, encoder=encoder)
    ea.cc = cc
    return ea


def rawModSwitch(ct, rc, seed, out_set=None):
    """-> ([z0, z1], noise_est).  ct: a canonical ciphertext (parts "1" and one more) whose prime set is what reCrypt
    leaves, at most three ciphertext primes and the special primes; it is not changed.  out_set: the primes of the
    encrypted recryption key (default: the chain's ciphertext primes, where PubKey::Encrypt puts it).  z_i is part i
    mod-switched to q, made divisible by p^e' and divided, row t holding it modulo prime t, in evaluation form."""
    cc = rc.cc
    if rc.p2dConv is None:
        raise LogicError("rawModSwitch: this RecryptData was made without a device context")
    ct._materializeTensor()
    p2r = ct.ptxtSpace
    if p2r <= 1:
        raise LogicError("Plaintext space must be greater than 1 for mod switching")
    if math.gcd(rc.q, p2r) != 1:
        raise LogicError("New modulus and current plaintext space must be co-prime")
    if rc.p2r % p2r != 0:
        raise LogicError("ptxtSpace must divide p^r when bootstrapping")
    handles = list(ct.parts)
    if len(handles) != 2 or handles[0] != "1":
        raise LogicError("Exactly 2 parts required for mod-switching in thin bootstrapping (the parts are %s)" % (handles,))
    out_set = sorted(cc.ctxtPrimes) if out_set is None else list(out_set)
    seed = int(seed)
    zz = []
    for i, h in enumerate(handles):
        cube = rc.p2dConv.coefficientCube(ct.parts[h])          # "The ciphertext *this is not affected"
        z = ct.ops.recryptPrep(cube, out_set, rc.q, rc.p, p2r, rc.p2ePrime, seed, i)
        rc.p2dConv.fromCube(z)
        zz.append(z)
    noise_est = math.exp(ct.lnNoise + math.log(rc.q) - cc.logOfProduct(ct.primeSet))
    return zz, noise_est


def normBnd(m):
    """PAlgebra::getNormBnd (src/PAlgebra.cpp:521-525): the product of 2 cot(pi / (2 u)) / u over the prime factors u of m"""
    out, n, u = 1.0, m, 2
    while u * u <= n:
        if n % u == 0:
            out *= 2.0 / math.tan(math.pi / (2.0 * u)) / u
            while n % u == 0:
                n //= u
        u += 1
    if n > 1:
        out *= 2.0 / math.tan(math.pi / (2.0 * n)) / n
    return out


def preProcess(ct, rc, seed, out_set=None, stats=None):
    """rawModSwitch with the check that reCrypt makes on its estimate (src/recryption.cpp:440-463): -> [z0, z1], or a
    LogicError when noise_est * normBnd exceeds HELIB_MIN_CAP_FRAC p^r boundForRecryption.  The estimate is read before
    any device work, so a refused ciphertext costs nothing."""
    noise_est = math.exp(ct.lnNoise + math.log(rc.q) - rc.cc.logOfProduct(ct.primeSet))
    checkNoise(rc.cc, noise_est, rc.p2r, normBnd(rc.cc.m), stats)
    return rawModSwitch(ct, rc, seed, out_set)[0]


def checkNoise(cc, noise_est, p2r, normBnd, stats=None):
    """the bound of src/recryption.cpp:443-463 on rawModSwitch's estimate: noise_est * normBnd (PAlgebra::getNormBnd)
    against HELIB_MIN_CAP_FRAC p^r boundForRecryption -> the ratio; above 1 a LogicError, as the non-debug reference.
    stats: a dict that takes the HELIB_STATS_UPDATE("raw-mod-switch-noise") sample."""
    noise_rat = noise_est * normBnd / (HELIB_MIN_CAP_FRAC * p2r * cc.boundForRecryption())
    if stats is not None:
        stats.setdefault("raw-mod-switch-noise", []).append(noise_rat)
    if noise_rat > 1:
        raise LogicError("rawModSwitch scaled noise exceeds bound: %f" % noise_rat)
    return noise_rat


def useChenHan(p, botHigh, r):
    """the cost rule of extractDigitsThin (src/recryption.cpp:806-832): the degree of Chen and Han's technique is
    p^(bot-1) (p-1) r, that of the basic one p^(bot-1) p^r, or p^(bot-1) p^(r-1) when p = 2 gives a bit for free"""
    if r <= 1:
        return False
    chen_han_cost = math.log(p - 1) + math.log(r)
    basic_cost = (r - 1) * math.log(p) if (p == 2 and r > 2 and botHigh + r > 2) else r * math.log(p)
    thresh = 1.75 if p == 2 else 1.5
    return basic_cost > thresh * chen_han_cost


def extractDigitsThin(ea, ct, botHigh, r, ePrime, force_chen_han=0, fused=None):
    """extractDigitsThin (src/recryption.cpp:793-909), in place: the slots of ct hold integers z modulo p^(botHigh + r);
    afterwards they hold, modulo p^r, -(z rounded to a multiple of p^botHigh) / p^botHigh, plus p^e' times the r - e'
    lowest digits of z when r > e'.  force_chen_han: the reference's fhe_force_chen_han (> 0: Chen and Han's branch,
    < 0: the basic one, 0: the cost rule)."""
    p = ea.p
    p2r = p ** r
    topHigh = botHigh + r - 1
    unpacked = ct.clone()
    unpacked.cleanUp()
    chen_han = useChenHan(p, botHigh, r)
    if force_chen_han:
        chen_han = force_chen_han > 0
    if chen_han:
        scratch = polyeval.extendExtractDigits(ea, unpacked, botHigh, r, fused=fused)
        for j in range(botHigh):
            unpacked -= scratch[j]
            unpacked.divideByP()
    else:
        if p == 2 and r > 2 and topHigh + 1 > 2:
            topHigh -= 1                            # for p = 2 we sometimes get a bit for free
        scratch = polyeval.extractDigits(ea, unpacked, topHigh + 1, fused=fused)
        if topHigh >= len(scratch):
            raise LogicError("extractDigitsThin: %d digits were asked for, %d came" % (topHigh + 1, len(scratch)))
        unpacked = scratch[topHigh].clone()
        for j in range(topHigh - 1, botHigh - 1, -1):
            unpacked.multByP()
            unpacked += scratch[j]
    if p == 2 and botHigh > 0:                      # for p = 2, subtract also the previous bit
        unpacked += scratch[botHigh - 1]
    unpacked.negate()
    if r > ePrime:                                  # add in digits from the bottom part, if any
        topLow = r - 1 - ePrime
        tmp = scratch[topLow].clone()
        for j in range(topLow - 1, -1, -1):
            tmp.multByP()
            tmp += scratch[j]
        if ePrime > 0:
            tmp.multByP(ePrime)
        unpacked += tmp
    unpacked.reducePtxtSpace(p2r)                   # our plaintext space is now mod p^r
    return ct.assign(unpacked)


def extractDigitsPacked(rc, ct, botHigh, r, ePrime, fused=None):
    """extractDigitsPacked (src/recryption.cpp:646-720), in place: unpack the d normal-basis coordinates of every slot
    (intraslot.unpack over the array at p^(e - e' + r)), extractDigitsThin on each, and repack with X^i in every slot of
    the array at p^r."""
    ea2, d = rc.ea, rc.ea.getDegree()
    with timing.NTIMER_START("unpack"):
        ct.cleanUp()
        unpacked = intraslot.unpack(rc.ea_boot, ct, rc.unpackSlotEncoding, fused=fused)
    for u in unpacked:
        extractDigitsThin(rc.ea_boot, u, botHigh, r, ePrime, fused=fused)
    with timing.NTIMER_START("repack"):
        out = unpacked[0]
        for i in range(1, d):
            x2i = np.zeros((1, ea2.size(), d), dtype=np.int64)
            x2i[0, :, i] = 1
            ea2.multByConstant(unpacked[i], ea2.encodePtxt(x2i))
            out += unpacked[i]
    return ct.assign(out)


def _bootKeySwitch(ct, pk, rc, seed, stats):
    """what reCrypt and thinReCrypt share (src/recryption.cpp:420-502, :1012-1099), in place: canonical form, at most
    three ciphertext primes, the switch to the recryption key, preProcess and the product with recryptEkey (the
    intFactor is lost here: the callers restore it)"""
    cc = rc.cc
    if set(ct.parts) - {"1", "s"}:                      # make sure that this ciphertext is in canonical form
        ct.reLinearize()
        ct.dropSmallAndSpecialPrimes()
    s3 = ct.primeSet - frozenset(cc.specialPrimes)
    if not s3 <= frozenset(cc.ctxtPrimes):
        raise LogicError("prime set is messed up")
    if len(s3) > 3:                                     # leave only the first three ciphertext primes
        first = min(s3)
        s3 = s3 & frozenset(range(first, first + 3))
    ct.modDownToSet(s3)
    ct.switchToKey(pk.keySwitchingTo[(1, 1, 0, pk.recryptKeyID)])
    zz = preProcess(ct, rc, seed, sorted(pk.recryptEkey.primeSet), stats)
    batch = getattr(zz[0], "batch", 1)
    new = pk.recryptEkey.replicated(batch)              # NOTE: here we lose the intFactor; it is restored by the caller
    # the reference measures embeddingLargestCoeff of each constant on the host; the constants stay on the device
    # here, so the size is the high-probability bound for coefficients of magnitude |w| <= (q / 2 + q p^e' / 2) / p^e'
    bound = cc.noiseBoundForUniform(rc.q / (2.0 * rc.p2ePrime) + rc.q / 2.0, cc.phim)
    new.multByConstant(zz[1], bound)
    new.addConstant(zz[0], bound)
    return ct.assign(new)


def _checked(ct, pk, rc, have_maps, who):
    """the checks at the head of reCrypt and thinReCrypt -> (ptxtSpace, intFactor), or None for an empty ciphertext"""
    if not ct.parts:
        return None
    if pk.recryptKeyID < 0:
        raise LogicError("No bootstrapping data")
    if not have_maps:
        raise LogicError("%s: this RecryptData holds no maps (%s)" % (who, "RecryptData(..., maps=True)" if who == "reCrypt"
                                                                      else "ThinRecryptData"))
    ct._materializeTensor()
    if set(ct.parts) == {"1"}:
        raise LogicError("%s: a dummy encryption (one part pointing at 1) is not handled" % who)
    if rc.p2r % ct.ptxtSpace != 0:
        raise LogicError("ptxtSpace must divide p^r when bootstrapping")
    return ct.ptxtSpace, ct.intFactor


def reCrypt(ct, pk, rc, seed=None, stats=None):
    """PubKey::reCrypt (src/recryption.cpp:367-545), in place.  pk: the key holding genRecryptData's results and the
    matrices the two EvalMaps walk through; rc: a RecryptData with its maps; seed: of the tie bits (None: 64 bits from
    the key's sampler)."""
    head = _checked(ct, pk, rc, rc.firstMap is not None, "reCrypt")
    if head is None:
        return ct
    ptxtSpace, intFactor = head
    if seed is None:
        seed = int(pk.sampler.rng.integers(0, 1 << 62))
    ct.dropSmallAndSpecialPrimes()
    with timing.NTIMER_START("AAA_preProcess"):
        _bootKeySwitch(ct, pk, rc, seed, stats)
    with timing.NTIMER_START("AAA_LinearTransform1"):
        rc.firstMap.apply(ct, pk=pk)
    with timing.NTIMER_START("AAA_extractDigitsPacked"):
        extractDigitsPacked(rc, ct, rc.e - rc.ePrime, rc.r, rc.ePrime)
    with timing.NTIMER_START("AAA_LinearTransform2"):
        rc.secondMap.apply(ct, pk=pk)
    if intFactor != 1:
        ct.intFactor = ct.intFactor * intFactor % ptxtSpace
    return ct


THIN_RECRYPT_NLEVELS = 3        # src/recryption.cpp:989: the ciphertext primes kept before the first linear map


class ThinRecryptData(RecryptData):
    """ThinRecryptData::init (src/recryption.cpp:773-787): RecryptData -- with the packed maps only when alsoThick is set
    -- and the two thin maps, coeffToSlot = ThinEvalMap(ea_boot, mvec, invert) over the array at p^(e - e' + r) and
    slotToCoeff = ThinEvalMap(ea, mvec).  The arrays are handed in, or built on the device over gens / ords."""

    def __init__(self, cc, g, mvec, gens=None, ords=None, alsoThick=False, ea=None, ea_boot=None, p2dConv=None, minimal=False):
        from . import thin_evalmap
        RecryptData.__init__(self, cc, g, mvec, gens=gens, ords=ords, p2dConv=p2dConv)
        self.ea, self.ea_boot = ea, ea_boot
        if alsoThick:
            self.buildMaps()
        if self.ea is None:
            self.ea = arrayAt(cc, g, self.r, gens=gens, ords=ords)
        if self.ea_boot is None:
            self.ea_boot = arrayAt(cc, g, self.e - self.ePrime + self.r, gens=gens, ords=ords)
        self.coeffToSlot = thin_evalmap.ThinEvalMap(self.ea_boot, self.mvec, invert=True, minimal=minimal)
        self.slotToCoeff = thin_evalmap.ThinEvalMap(self.ea, self.mvec, minimal=minimal)


def thinReCrypt(ct, pk, rc, seed=None, stats=None):
    """PubKey::thinReCrypt (src/recryption.cpp:940-1128), in place, for a ciphertext whose slots hold integers modulo
    p^r.  pk: the key holding genRecryptData's results, the matrices the two ThinEvalMaps walk through and those of the
    Frobenius (traceMap); rc: a ThinRecryptData; seed: of the tie bits (None: 64 bits from the key's sampler)."""
    cc = rc.cc
    head = _checked(ct, pk, rc, getattr(rc, "coeffToSlot", None) is not None, "thinReCrypt")
    if head is None:
        return ct
    ptxtSpace, intFactor = head
    if seed is None:
        seed = int(pk.sampler.rng.integers(0, 1 << 62))
    ct.dropSmallAndSpecialPrimes()
    first = min(cc.ctxtPrimes)                          # drop to a low level before the first linear map
    ct.bringToSet(frozenset(range(first, min(max(cc.ctxtPrimes), first + THIN_RECRYPT_NLEVELS - 1) + 1)))
    with timing.NTIMER_START("AAA_slotToCoeff"):
        rc.slotToCoeff.apply(ct, pk=pk)
    with timing.NTIMER_START("AAA_bootKeySwitch"):
        _bootKeySwitch(ct, pk, rc, seed, stats)
    with timing.NTIMER_START("AAA_coeffToSlot"):
        rc.coeffToSlot.apply(ct, pk=pk)
    with timing.NTIMER_START("AAA_extractDigitsThin"):
        extractDigitsThin(rc.ea_boot, ct, rc.e - rc.ePrime, rc.r, rc.ePrime)
    if intFactor != 1:
        ct.intFactor = ct.intFactor * intFactor % ptxtSpace
    return ct
