"""EncryptedArray(context, G) with G = F_0, the first factor of Phi_m mod p (include/helib/EncryptedArray.h over the
G = F_0 branches of PAlgebraModDerived, src/PAlgebra.cpp:1064-1067, 1096-1100, 1168-1186, 1243-1278): every slot is an
element of GF(p^d) = Z_p[X] / G, d = ord_m(p), r = 1.  helib_amd.bgv_crt / bgv_hypercube keep one integer mod p per slot
(G = X); here a slot vector is an int64 array [B, nslots, d], the d coefficients of a slot lowest first.

  encode / decode / encrypt[_batch] / decrypt[_batch] / encodePtxt / multByConstant / addConstant
                      on GF slots, through helib_amd.capi.bgvGf* (hx_bgv_gf_*: helib_amd/csrc/bgv_gf.h, bgv_gf.hip)
  a [B, nslots] array means constants in the slots, and encodes to exactly the words bgv_crt gives: masks,
                      maskSlots, _encodedMask, _maskSplit and _maskBlend are inherited as they are
  rotate1D / rotate / shift / shift1D / runningSums / totalSums     inherited from bgv_hypercube: they move whole slot
                      values (np.roll / zero fill along axis 1, sums coefficient-wise mod p), non-native dimensions
                      included
  frobeniusAutomorph  Ctxt::frobeniusAutomorph (keys: helib_amd.keys.addFrbMatrices): slot alpha -> alpha^(p^j) mod G
  mulPlain / frobeniusPlain     the plain-side truths: the slot-wise product mod (G, p) and alpha -> alpha^(p^j)

The members that know a slot is an element of Z_p[X] / G -- the check of G, _slots, the Frobenius, the plain side -- and
the encoder are helib_amd.slot_ring's (SlotRing, SlotEncoder) with the modulus P = p; this module adds the constructor.

Out of scope, refused with a message: a G other than F_0 (a root of G in Z_p[X] / F_0 would have to be found: the
reference's FindRoots branch of mapToSlots, src/PAlgebra.cpp:1116-1186), deg G < d, d > 64, and p^r with r > 1, which is
helib_amd.bgv_gr (slots in the Galois ring Z_(p^r)[X] / G; unpack / repack over either class: helib_amd.intraslot).  Linearized
polynomials, MatMul1D with GF entries and BlockMatMul1D over these slots are helib_amd.bgv_gf_matmul (helib_amd.bgv_matmul
takes integer matrices of two axes).  Nothing here imports oracle/."""
from . import bgv_hypercube, capi, slot_ring
from .ckks import LogicError


class GfEncoder(slot_ring.SlotEncoder):
    """GF(p^d) slot vectors <-> polynomials on the device (hx_bgv_gf_*): CrtEncoder's members, and G"""

    def __init__(self, hxctx, p):
        super().__init__(hxctx, capi.BgvGf(hxctx, p))


class EncryptedArray(slot_ring.SlotRing, bgv_hypercube.EncryptedArray):
    """context: a BGV helib_amd.ctxt.ChainContext with gcd(p, m) = 1 and r = 1; hxctx: the capi.Context holding its
    primes; G: None for F_0, or F_0's coefficients (constant first, any representatives mod p).  An injected encoder has
    GfEncoder's members (encode takes [B, nslots, d] or, for constants, [B, nslots]) and G.  self.P = self.p is the
    modulus of the slots."""

    _otherG = ("EncryptedArray: G is not F_0, the first factor of Phi_m mod p; another G needs a root of G "
               "in Z_p[X] / F_0 (the reference's FindRoots branch of mapToSlots), which is not built")

    def __init__(self, context, hxctx, G=None, encoder=None):
        if getattr(context, "ckks", False):
            raise LogicError("EncryptedArray: a CKKS context takes EncryptedArrayCx")
        if getattr(context, "r", 1) != 1 or context.ptxtSpace != context.p:
            raise capi.HxError(capi.HX_ERR_UNSUPPORTED,
                               "BGV slots: plaintext space p^r with r > 1 (Hensel lifting) is not built")
        super().__init__(context, hxctx, encoder=encoder if encoder is not None else GfEncoder(hxctx, context.p))
        self.P = self.p
        self._initRing(G)
