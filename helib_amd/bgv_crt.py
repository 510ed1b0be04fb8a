"""The default-constructed EncryptedArray (G = X, include/helib/EncryptedArray.h) for any d = ord_m(p) at r = 1: Phi_m
mod p has nslots = phi(m) / d factors of degree d and a slot holds an integer mod p.  helib_amd.bgv.EncryptedArray
covers d = 1 through the engine's transform for the prime p; here the maps are two matrices modulo p
(helib_amd/csrc/bgv_crt.h) and two matrix-product kernels (bgv_crt.hip), so p = 2 and the other small plaintext primes
of the reference's rings work.

  encode / decode / encrypt[_batch] / decrypt[_batch] / encodePtxt / multByConstant / addConstant / shift1D
                      inherited unchanged; slot vectors are [B, nslots]
  rotate1D            a native dimension (and dc=True on any): one automorphism; a non-native one the reference's masked
                      branch (src/EncryptedArray.cpp:99-124): ct*m + T - T*m with T the copy moved by g^-ord
  rotate / shift / totalSums / runningSums, and helib_amd.bgv_matmul, over a hypercube with a non-native dimension
                      raise LogicError: their masked loops (src/EncryptedArray.cpp:221-264) are not built

Out of scope: p^r with r > 1 (refused here; integer slots mod p^r: helib_amd.bgv_pr.  Slots in GF(p^d), G = F_0:
helib_amd.bgv_gf).  Nothing here imports oracle/."""
import numpy as np

from . import bgv, capi, hostnt
from .ckks import LogicError


class CrtEncoder:
    """slot vectors <-> polynomials on the device through the CRT tables (hx_bgv_crt_*): DeviceEncoder's members
    without matrix / encodeDiagonals"""

    def __init__(self, hxctx, p):
        self.g = hxctx
        self.table = capi.BgvCrt(hxctx, p)

    def dims(self):
        """(gens, signed ords) of the hypercube of Z_m^* / <p>"""
        return self.table.gens, self.table.ords

    def encode(self, v, mul, idx, coeffs=False):
        return capi.bgvCrtEncode(self.table, v, idx, mul, coeffs=coeffs)

    def split(self, poly):
        return capi.splitBatch(poly)

    def embed(self, coeffs):
        return capi.bgvCrtEmbed(self.table, coeffs)

    def decode(self, acc, factor_inv):
        return capi.bgvCrtDecode(self.table, acc, factor_inv)

    def norm(self, coeffs):
        """embeddingLargestCoeff of every zzX [B, phi(m)]"""
        return capi.embeddingLargestCoeff(self.g, np.asarray(coeffs, dtype=np.float64))


class EncryptedArray(bgv.EncryptedArray):
    """context: a BGV helib_amd.ctxt.ChainContext with gcd(p, m) = 1 and r = 1 (any d); hxctx: the capi.Context holding
    its primes.  rotate, shift, totalSums, runningSums and the matrix products of helib_amd.bgv_matmul raise LogicError
    when a dimension they would cross is not native."""

    def __init__(self, context, hxctx, encoder=None):
        if getattr(context, "ckks", False):
            raise LogicError("EncryptedArray: a CKKS context takes EncryptedArrayCx")
        self.cc, self.g = context, hxctx
        self.m, self.p = context.m, context.p
        if getattr(context, "r", 1) != 1 or context.ptxtSpace != self.p:
            raise capi.HxError(capi.HX_ERR_UNSUPPORTED,
                               "BGV slots: plaintext space p^r with r > 1 (Hensel lifting) is not built")
        self.enc = encoder if encoder is not None else CrtEncoder(hxctx, self.p)
        dims = getattr(self.enc, "dims", None)
        gens, ords = dims() if dims is not None else ((), ())
        self.zMStar = hostnt.ZmStar(self.m, self.p, gens, ords)
        if gens and any((o > 0) != nat for o, nat in zip(ords, self.zMStar.native)):
            raise LogicError("EncryptedArray: the encoder's signed orders disagree with the generators")

    def size(self):
        return self.zMStar.getNSlots()

    def getDegree(self):
        return self.zMStar.ordP

    def rotate1D(self, ct, i, amt, dc=False):
        """EncryptedArray::rotate1D (src/EncryptedArray.cpp:65-125): the slot whose coordinate in dimension i is c moves
        to coordinate c + amt (mod the order).  dc ("don't care"): one automorphism on any dimension -- what falls off
        the end of a non-native dimension is then not what wraps around."""
        if not 0 <= i < self.dimension():
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "i must be between 0 and dimension()")
        ord_ = self.sizeOfDimension(i)
        amt %= ord_
        if amt == 0:
            return ct
        if dc or self.nativeDimension(i):
            return ct.smartAutomorph(self.zMStar.genToPow(i, amt))
        # the non-native rotation (:99-124)
        ct.smartAutomorph(self.zMStar.genToPow(i, amt))          # ct = rho_i^amt(original)
        T = ct.clone()
        T.smartAutomorph(self.zMStar.genToPow(i, -ord_))         # T = rho_i^(amt - ord)(original)
        if not ct.parts:
            return ct
        m1, sz = self._encodedMask(self.maskSlots(i, amt), set(ct.primeSet) | set(T.primeSet))
        ct.multByConstant(m1, sz)                                # ct*m1 + T - T*m1
        ct += T
        T.multByConstant(m1, sz)
        ct -= T
        return ct

    def _nativeOnly(self, what):
        if not all(self.nativeDimension(i) for i in range(self.dimension())):
            raise LogicError("EncryptedArray::%s over a non-native dimension is not built" % what)

    def rotate(self, ct, amt, fused=None):
        self._nativeOnly("rotate")
        return super().rotate(ct, amt, fused)

    def shift(self, ct, k, fused=None):
        self._nativeOnly("shift")
        return super().shift(ct, k, fused)

    def runningSums(self, ct, fused=None):
        self._nativeOnly("runningSums")
        return super().runningSums(ct, fused)

    def totalSums(self, ct, fused=None):
        self._nativeOnly("totalSums")
        return super().totalSums(ct, fused)
