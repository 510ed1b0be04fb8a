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
Nothing here imports oracle/."""
import math

import numpy as np

from . import capi
from . import ctxt as hc


class LogicError(RuntimeError):
    """helib::LogicError"""


class EncryptedArrayCx:
    """context: a CKKS helib_amd.ctxt.ChainContext; hxctx: the capi.Context holding its primes."""

    def __init__(self, context, hxctx):
        if not getattr(context, "ckks", False):
            raise LogicError("bad args to CKKS_canonicalEmbedding")   # src/norms.cpp:505
        if context.m & (context.m - 1):
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "CKKS scheme only supports m as a power of two.")
        self.cc, self.g = context, hxctx
        self.m = context.m

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
        r = capi.ckksEncode(self.g, v, f, idx, coeffs=coeffs)
        return (r[0], f, r[1]) if coeffs else (r, f)

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
