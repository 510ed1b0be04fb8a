"""EncryptedArrayCx (include/helib/EncryptedArray.h:1150-1330, src/EaCx.cpp) over the device: CKKS slot vectors --
numpy complex128 arrays of shape [B, m/4] (B independent vectors: a batch) -- go into ciphertexts and come back out.

  encode / decode     CKKS_embedInSlots / CKKS_canonicalEmbedding (src/norms.cpp:495-615) on the device
                      (helib_amd.capi.ckksEncode / ckksEmbed: hx_ckks_encode / hx_ckks_embed)
  encrypt[_batch]     EncryptedArrayCx::encrypt (include/helib/EncryptedArray.h:1252-1266): encode with the factor
                      of encode(zzX&, ...) (src/EaCx.cpp:324-349), then PubKey.CKKSencrypt of the encoded DoubleCRT
  rawDecrypt[_batch]  src/EaCx.cpp:62-86: the secret-key inner product, then hx_ckks_decode (the division by
                      ratFactor and the embedding on the device; one download)

Slot order is PAlgebra's (ith_rep, src/PAlgebra.cpp:520-570): slot s holds the value at zeta^-T[m/4-1-s].
Out of scope: EncryptedArrayCx::decrypt, which adds noise against the Li-Micciancio attack
(src/Ctxt.cpp:3051-3115) from a PRG stream that cannot be reproduced here -- only rawDecrypt is offered.

Between slots (this file; the matrix product is helib_amd/linalg.py, re-exported here):
  rotate / shift      src/EaCx.cpp:142-236          totalSums / runningSums   src/EncryptedArray.cpp:695-735
  extractRealPart / extractImPart   src/EaCx.cpp:419-447
  encodePtxt / multByConstant / addConstant   the EncodedPtxt interface (src/EaCx.cpp:238-278, src/Ctxt.cpp:2001-2030,
                      :2226-2260)
Nothing here imports oracle/."""
import math

import numpy as np

from . import capi
from . import ctxt as hc
from . import hostnt


class DeviceEncoder:
    """slot vectors -> DoubleCRT on the device (hx_ckks_encode).  An EncryptedArrayCx can be given another object
    with these three members (tests drive the host control flow over a CPU backend that way)."""
    max_batch = 64

    def __init__(self, hxctx):
        self.g = hxctx

    def encode(self, v, scaling, idx):
        return capi.ckksEncode(self.g, v, scaling, idx)

    def split(self, poly):
        return capi.splitBatch(poly)


class EncodedPtxt:
    """EncodedPtxt_CKKS (include/helib/EncodedPtxt.h): the encoded slots with mag, scale and err -- the three
    numbers Ctxt.multByConstantCKKS / addConstant ask for.  The reference keeps the zzX and expands it to the
    ciphertext's primes when it is used (FatEncodedPtxt::expand); here the DoubleCRT is kept, and re-encoded from
    the slots if a ciphertext lives on primes it lacks."""

    def __init__(self, ea, v, dcrt, mag, scale, err):
        self.ea, self.v, self.dcrt, self.mag, self.scale, self.err = ea, v, dcrt, mag, scale, err

    def expand(self, primeSet, exact=False):
        have = self.dcrt.getIndexSet()
        want = sorted(primeSet)
        if (have == want) if exact else set(want) <= set(have):
            return self.dcrt
        return self.ea.enc.encode(self.v, self.scale, want)


class LogicError(RuntimeError):
    """helib::LogicError"""


class EncryptedArrayCx:
    """context: a CKKS helib_amd.ctxt.ChainContext; hxctx: the capi.Context holding its primes."""

    def __init__(self, context, hxctx, encoder=None):
        if not getattr(context, "ckks", False):
            raise LogicError("bad args to CKKS_canonicalEmbedding")   # src/norms.cpp:505
        if context.m & (context.m - 1):
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "CKKS scheme only supports m as a power of two.")
        self.cc, self.g = context, hxctx
        self.m = context.m
        self.enc = encoder if encoder is not None else DeviceEncoder(hxctx)
        self.zMStar = hostnt.ZmStar(self.m, -1)

    def size(self):
        return self.m // 4

    def _slots(self, v):
        v = np.asarray(v, dtype=np.complex128)
        v = v.reshape(1, -1) if v.ndim == 1 else v
        if v.shape[1] > self.size():
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "more values than slots")
        return v

    def encodeScalingFactor(self, precision=-1):
        return float(self.cc.encodeScalingFactor(precision))

    def factor(self, v, useThisSize=-1.0, precision=-1):
        """the factor of encode(zzX&, array, useThisSize, precision) (src/EaCx.cpp:324-349): encodeScalingFactor /
        size, size = the largest |v| when not given (at least 1 if that is 0); one factor for the whole batch"""
        if useThisSize < 0:
            useThisSize = max(useThisSize, float(np.max(np.abs(v))) if v.size else 0.0)
        if useThisSize <= 0:
            useThisSize = 1.0
        return self.encodeScalingFactor(precision) / useThisSize

    def encode(self, v, useThisSize=-1.0, precision=-1, idx=None, coeffs=False):
        """-> (DoubleCRT over idx (default: the ctxt primes) in evaluation form, factor); coeffs=True adds the
        int64 coefficients [B, phi(m)].  HxError on "overflow in encoding"."""
        v = self._slots(v)
        f = self.factor(v, useThisSize, precision)
        idx = list(self.cc.ctxtPrimes) if idx is None else list(idx)
        if not coeffs:
            return self.enc.encode(v, f, idx), f
        r = capi.ckksEncode(self.g, v, f, idx, coeffs=True)
        return r[0], f, r[1]

    def encodeCoeffs(self, v, scaling):
        """CKKS_embedInSlots alone: the zzX [B, phi(m)] of v scaled by `scaling`"""
        return capi.ckksEncode(self.g, self._slots(v), scaling, [], coeffs=True)[1]

    def decode(self, coeffs, scaling):
        """EncryptedArrayCx::decode (src/EaCx.cpp:385-395): canonicalEmbedding(f) / scaling"""
        if not scaling > 0:
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "Scaling must be positive to decode")
        return capi.ckksEmbed(self.g, np.atleast_2d(np.asarray(coeffs, dtype=np.float64))) / scaling

    def encrypt(self, pk, v, useThisSize=-1.0, precision=-1):
        """EncryptedArrayCx::encrypt (include/helib/EncryptedArray.h:1252-1266) of one vector"""
        v = self._slots(v)
        if v.shape[0] != 1:
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "encrypt takes one vector: use encrypt_batch")
        return self.encrypt_batch(pk, v, useThisSize, precision)

    def encrypt_batch(self, pk, vs, useThisSize=-1.0, precision=-1):
        """B vectors -> one batched Ctxt: the encoding factor from the largest |v| of the batch unless useThisSize is
        given, useThisSize itself passed on as CKKSencrypt's ptxtSize; samples in the order of B consecutive
        encryptions, one ef (PubKey.CKKSencryptBatch)"""
        vs = self._slots(vs)
        dcrt, f = self.encode(vs, useThisSize, precision)
        # the caller's size goes to CKKSencrypt unchanged (include/helib/EncryptedArray.h:1264-1266): the default
        # -1 means ptxtSize = 1 there, whatever factor the encoding took from the values
        return pk.CKKSencryptBatch(dcrt, useThisSize, f)

    def rawDecrypt_batch(self, ct, sk):
        """src/EaCx.cpp:62-86 for every element of a batched Ctxt -> complex [B, m/4]"""
        acc = innerProduct(sk, ct)
        if acc is None:
            return np.zeros((1, self.size()), dtype=np.complex128)
        return capi.ckksDecode(acc, ct.lnRatFactor)

    def rawDecrypt(self, ct, sk, real=False):
        """complex slots (real=True: their real parts, EncryptedArrayCx's `project`) of a batch-1 Ctxt"""
        v = self.rawDecrypt_batch(ct, sk)[0]
        return v.real.copy() if real else v

    # ---- the EncodedPtxt interface ----
    def defaultErr(self):
        """include/helib/EncryptedArray.h:1315-1329"""
        return self.cc.noiseBoundForUniform(0.5, self.cc.phim)

    def defaultScale(self, err, prec=-1):
        """include/helib/EncryptedArray.h:1331-1349: 2^(r + ceil(log2(err))), err at least 1"""
        err = max(err, 1.0)
        r = self.cc.r if prec < 0 else prec
        _, e = math.frexp(1.0 / err)
        return math.ldexp(1.0, r - e + 1)

    def encodePtxt(self, v, mag=-1.0, prec=-1, idx=None):
        """EncryptedArrayCx::encode(EncodedPtxt&, array, mag, prec) (src/EaCx.cpp:238-278): mag = Norm(v) unless
        given, err = defaultErr(), scale = defaultScale(err, prec) -- neither depends on the data."""
        v = self._slots(v)
        if mag < 0:
            mag = float(np.max(np.abs(v))) if v.size else 0.0
        err = self.defaultErr()
        scale = self.defaultScale(err, prec)
        idx = list(self.cc.ctxtPrimes) if idx is None else list(idx)
        return EncodedPtxt(self, v, self.enc.encode(v, scale, idx), mag, scale, err)

    def multByConstant(self, ct, eptxt):
        """Ctxt::multByConstant(const EncodedPtxt&) (src/Ctxt.cpp:1952-1958, 2001-2030)"""
        if not ct.parts:
            return ct
        return ct.multByConstantCKKS(eptxt.expand(ct.primeSet), eptxt.mag, eptxt.scale, eptxt.err)

    def addConstant(self, ct, eptxt, neg=False):
        """Ctxt::addConstant(const FatEncodedPtxt_CKKS&, neg) (src/Ctxt.cpp:2226-2260): a ciphertext whose only
        part is the constant, with the constant's mag, scale and err, goes through addCtxt -- which equalises the
        factors"""
        tmp = hc.Ctxt(ct.context, ct.ops, ct.ksw, ct.ksw_ptxtSpace, ct.ksw_lnNoise)
        tmp.ksw_auto, tmp.ksw_pow, tmp.ksw_map = ct.ksw_auto, ct.ksw_pow, ct.ksw_map
        tmp.primeSet = ct.primeSet
        tmp.ptxtMag, tmp.lnRatFactor, tmp.lnNoise = eptxt.mag, math.log(eptxt.scale), math.log(eptxt.err)
        tmp.parts = {"1": eptxt.expand(ct.primeSet, exact=True)}
        ct.addCtxt(tmp, negative=neg)
        return ct

    # ---- between slots ----
    def _amount(self, amt):
        """amt % ord with C++ rules, then into [0, ord)"""
        ord_ = self.size()
        amt = int(math.fmod(amt, ord_))
        return amt + ord_ if amt < 0 else amt

    def rotate(self, ct, amt):
        """EncryptedArrayCx::rotate = rotate1D(ctxt, 0, amt) (src/EaCx.cpp:142-164, 222-228): slot j moves to slot
        (j + amt) mod size"""
        amt = self._amount(amt)
        if amt == 0:
            return ct
        return ct.smartAutomorph(self.zMStar.genToPow(0, amt))

    def shift(self, ct, k):
        """EncryptedArrayCx::shift = shift1D(ctxt, 0, k) (src/EaCx.cpp:166-221, 229-235): the slots that would wrap
        around are cleared by the encoded 0/1 mask first, then the rotation; |k| >= size clears the ciphertext"""
        ord_ = self.size()
        if k <= -ord_ or k >= ord_:
            ct.parts = {}
            return ct
        amt = self._amount(k)
        if amt == 0:
            return ct
        val = self.zMStar.genToPow(0, amt - ord_ if k < 0 else amt)
        j = np.arange(ord_)
        mask = ((j + k < ord_) & (j + k >= 0)).astype(np.complex128)
        self.multByConstant(ct, self.encodePtxt(mask))
        return ct.smartAutomorph(val)

    def totalSums(self, ct):
        """totalSums (src/EncryptedArray.cpp:707-735): every slot <- the sum of all slots"""
        n = self.size()
        if n == 1:
            return ct
        orig = ct.clone()
        e = 1
        for i in range(n.bit_length() - 2, -1, -1):
            tmp1 = ct.clone()
            self.rotate(tmp1, e)
            ct += tmp1
            e *= 2
            if (n >> i) & 1:
                tmp2 = orig.clone()
                self.rotate(tmp2, e)
                ct += tmp2
                e += 1
        return ct

    def runningSums(self, ct):
        """runningSums (src/EncryptedArray.cpp:695-705): slot j <- the sum of slots 0..j"""
        n, shamt = self.size(), 1
        while shamt < n:
            tmp = ct.clone()
            self.shift(tmp, shamt)
            ct += tmp
            shamt *= 2
        return ct

    def extractRealPart(self, ct):
        """src/EaCx.cpp:419-425: (c + conj(c)) * 0.5"""
        tmp = ct.clone()
        tmp.complexConj()
        ct += tmp
        return ct.multByScalar(0.5)

    def extractImPart(self, ct):
        """src/EaCx.cpp:432-447: (conj(c) - c) * i * 0.5, i encoded as encodei does (:368-372: size 1)"""
        tmp = ct.clone()
        ct.complexConj()
        ct -= tmp
        if not ct.parts:
            return ct
        di, f = self.encode(np.full(self.size(), 1j), 1.0, idx=sorted(ct.primeSet))
        ct.multByConstantCKKS(di, 1.0, f, self.cc.encodeRoundingError())
        return ct.multByScalar(0.5)


def innerProduct(sk, ct):
    """sum over the parts of part * s^r(X^t) (SecKey::Decrypt, src/keys.cpp:1327-1386), batched parts times the
    key rows broadcast over the batch; evaluation form"""
    acc = None
    for handle, part in ct.parts.items():
        term = part.copy()
        if handle != "1":
            sPower, xPower = hc.handle_powers(handle)
            term *= sk._keyRows(part.getIndexSet(), sPower, xPower)
        if acc is None:
            acc = term
        else:
            acc += term
    return acc


def errorBound(ct):
    """Ctxt::errorBound: noiseBound / ratFactor"""
    return math.exp(ct.lnNoise - ct.lnRatFactor)


from .linalg import MatMul1D_CKKS, MatMul1DExec  # noqa: E402,F401
