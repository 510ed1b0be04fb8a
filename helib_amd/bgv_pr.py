"""The default-constructed EncryptedArray (G = X) for the plaintext space p^r, r >= 1, any d = ord_m(p): a slot holds an
integer mod p^r.  The factors of Phi_m are found and ordered modulo p and Hensel-lifted (the r > 1 branch of
PAlgebraModDerived's constructor, src/PAlgebra.cpp:757-763 over PAlgebraLift, :840-881); the maps are bgv_crt's two
matrices taken modulo p^r (helib_amd/csrc/bgv_crt.h, hx_bgv_crt_create_pr), so the geometry, the order of the slots and
the kernels are those of r = 1, and at r = 1 the class is helib_amd.bgv_hypercube.EncryptedArray word for word.

  encode / decode / encrypt[_batch] / encodePtxt / multByConstant / addConstant
                      bgv's bodies with the modulus p^r where they say p; slot vectors are int64 [B, nslots]
  decrypt[_batch]     a ciphertext whose space is p^k, 1 <= k <= r (after Ctxt.divideByP, or inside extractDigits), is
                      decoded through the p^r tables and its slots reduced mod p^k: the tables mod p^k are the p^k tables
  rotate1D / rotate / shift / shift1D / totalSums / runningSums     inherited from bgv_hypercube with the 0/1 masks
                      encoded mod p^r, non-native dimensions included
  extractDigits       src/extractDigits.cpp:70-129 for p = 2 (square) and p = 3 (cube): digits[j] holds, mod p^(r-j), a
                      value congruent mod p to digit j of every slot; its inner step tmp -= digits[j]; tmp.divideByP() is
                      Ctxt.subDivideByP, one hx_scaled_sub with fused=True

Out of scope, refused with LogicError and a message: helib_amd.bgv_matmul and bgv_gf_matmul over this class at r > 1,
p > 3 in this module's extractDigits (helib_amd.polyeval has polyEval,
buildDigitPolynomial, an extractDigits for any p and extendExtractDigits).  Slots with d > 1 coefficients at r > 1 --
the Galois ring Z_(p^r)[X] / G -- are helib_amd.bgv_gr (helib_amd.bgv_gf stays at r = 1 and refuses).  Nothing here
imports oracle/."""
import numpy as np

from . import bgv, bgv_crt, bgv_hypercube, capi, hostnt
from . import ctxt as hc
from .ckks import LogicError, innerProduct


class PrEncoder(bgv_crt.CrtEncoder):
    """slot vectors mod p^r <-> polynomials on the device through the lifted CRT tables (hx_bgv_crt_create_pr)"""

    def __init__(self, hxctx, p, r):
        self.g = hxctx
        self.table = capi.BgvCrt(hxctx, p, r)


class EncryptedArray(bgv_hypercube.EncryptedArray):
    """context: a BGV helib_amd.ctxt.ChainContext with gcd(p, m) = 1 and any r >= 1 with p^r < 2^31; hxctx: the
    capi.Context holding its primes.  self.p is the prime, self.P = p^r the modulus of the slots."""

    def __init__(self, context, hxctx, encoder=None):
        if getattr(context, "ckks", False):
            raise LogicError("EncryptedArray: a CKKS context takes EncryptedArrayCx")
        self.cc, self.g = context, hxctx
        self.m, self.p, self.r = context.m, context.p, int(getattr(context, "r", 1))
        self.P = self.p ** self.r
        if self.r < 1 or context.ptxtSpace != self.P:
            raise LogicError("EncryptedArray: the context's plaintext space is not p^r")
        self.enc = encoder if encoder is not None else PrEncoder(hxctx, self.p, self.r)
        dims = getattr(self.enc, "dims", None)
        gens, ords = dims() if dims is not None else ((), ())
        self.zMStar = hostnt.ZmStar(self.m, self.p, gens, ords)
        if gens and any((o > 0) != nat for o, nat in zip(ords, self.zMStar.native)):
            raise LogicError("EncryptedArray: the encoder's signed orders disagree with the generators")

    def getPPowR(self):
        return self.P

    def _slots(self, v):
        a = np.asarray(v)
        if a.dtype == object or a.dtype.kind not in "iu" or a.dtype == np.uint64:
            a = np.array([int(x) % self.P for x in a.reshape(-1)], dtype=np.int64).reshape(a.shape)
        return super()._slots(a)

    def decode(self, coeffs):
        """EncryptedArray::decode of plaintext polynomials [B, phi(m)] -> int64 slots [B, nslots] in [0, p^r)"""
        c = np.asarray(coeffs)
        if c.dtype == object:
            c = np.array([int(x) % self.P for x in c.reshape(-1)], dtype=np.int64).reshape(c.shape)
        return self.enc.embed(np.atleast_2d(c.astype(np.int64)))

    # ---- encryption: bgv.py's checks against p (bgv.py:181-206) are against p^r, or a p^k below it ----
    def encrypt_batch(self, pk, vs):
        if pk.ptxtSpace != self.P:
            raise LogicError("EncryptedArray.encrypt: the key's plaintext space is not p^r")
        idx = list(self.cc.ctxtPrimes)
        return pk.EncryptBatch(self.encode(vs, idx, mul=self.cc.productOfPrimes(idx) % self.P))

    def _spaceOf(self, ct):
        """p^k, the ciphertext's space, 1 <= k <= r"""
        try:
            k = ct.effectiveR()
        except RuntimeError:
            k = 0
        if not 1 <= k <= self.r:
            raise LogicError("EncryptedArray: the ciphertext's plaintext space is not p^k with 1 <= k <= r")
        return ct.ptxtSpace

    def decrypt_batch(self, ct, sk):
        """SecKey::Decrypt + decode -> int64 [B, nslots] in [0, p^k), p^k the ciphertext's space.  The factor of
        src/keys.cpp:1388-1405 is inverted mod p^k; the polynomial is reduced and decoded mod p^r, which commutes with
        the reduction of the slots mod p^k."""
        Pk = self._spaceOf(ct)
        acc = innerProduct(sk, ct)
        if acc is None:
            return np.zeros((1, self.size()), dtype=np.int64)
        factor = self.cc.productOfPrimes(sorted(ct.primeSet)) % Pk * ct.intFactor % Pk
        return self.enc.decode(acc, pow(factor, -1, Pk)) % Pk

    # ---- the EncodedPtxt interface ----
    def encodePtxt(self, v):
        v = self._slots(v)
        return bgv.EncodedPtxt(self, v, self.encodeCoeffs(v), self.P)

    def _space(self, ct, eptxt):
        # the reference reduces both spaces to their gcd (src/Ctxt.cpp:1988-1990, 2200-2202); the constant is encoded
        # mod p^r here, so a ciphertext below p^r would need the encoder at p^k
        if ct.ptxtSpace != eptxt.ptxtSpace:
            raise LogicError("EncryptedArray: the ciphertext's plaintext space is not the constant's p^r")

    def addConstant(self, ct, eptxt, neg=False):
        """Ctxt::addConstant(const EncodedPtxt_BGV&, neg) (src/Ctxt.cpp:2187-2224) with f = intFactor * Q mod p^r"""
        self._space(ct, eptxt)
        P = self.P
        primes = sorted(ct.primeSet)
        f = self.cc.productOfPrimes(primes) % P * ct.intFactor % P if P > 2 else 1
        dcrt, poly = self.enc.encode(eptxt.v, f, primes, coeffs=True)
        ct.lnNoise = hc.logaddexp(ct.lnNoise, hc._ln(float(np.max(self.enc.norm(poly)))))
        if "1" not in ct.parts:
            raise RuntimeError("Ctxt::addPart: no part pointing at 1")
        if neg:
            ct.parts["1"] -= dcrt
        else:
            ct.parts["1"] += dcrt
        return ct

    def _nextMask(self, mask, i, v):
        hi = self.maskSlots(i, v + 1)
        return (mask * (self.maskSlots(i, v) - hi) + hi) % self.P


def extractDigits(ea, ct, r=0, fused=None):
    """extractDigits (src/extractDigits.cpp:70-129) for p = 2 and p = 3: the slots of ct hold integers mod p^rr,
    rr = ct.effectiveR(); -> digits, a list of r ciphertexts (r <= 0 or r > rr: rr), digits[j] with plaintext space
    p^(rr - j) and, in every slot, a value congruent mod p to digit j of the slot's expansion in base p (digits in
    [0, p) for p = 2, balanced for p = 3).  Round i starts from ct and, for j < i, raises digits[j] to the p-th power in
    place (square / cube) and does tmp -= digits[j]; tmp.divideByP() -- Ctxt.subDivideByP(digits[j], fused).  p > 3 is
    refused here: helib_amd.polyeval.extractDigits takes any p."""
    if ct.context is not ea.cc:
        raise LogicError("extractDigits: the ciphertext belongs to another context than the EncryptedArray")
    p = ea.p
    if p > 3:
        raise LogicError("extractDigits: p = %d > 3 needs polyEval and buildDigitPolynomial "
                         "(src/extractDigits.cpp:28-56, 99), which are not built" % p)
    rr = ct.effectiveR()
    if r <= 0 or r > rr:
        r = rr
    digits = []
    for i in range(r):
        tmp = ct.clone()
        for j in range(i):
            if p == 2:
                digits[j].square()
            else:
                digits[j].cube()
            tmp.subDivideByP(digits[j], fused)
        digits.append(tmp)
    return digits
