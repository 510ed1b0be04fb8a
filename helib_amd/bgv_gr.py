"""EncryptedArray(context, G) for the plaintext space p^r, r >= 1, with G the Hensel lift of F_0, the first factor of
Phi_m mod p: every slot is an element of the Galois ring Z_(p^r)[X] / G, d = deg G = ord_m(p).  It is the array
RecryptData::init builds over p^(e - e' + r) (src/recryption.cpp:310-343).  helib_amd.bgv_pr keeps one integer mod p^r per
slot (G = X) and helib_amd.bgv_gf an element of GF(p^d) at r = 1; both classes take the members that know the ring of a
slot, and their encoder, from helib_amd.slot_ring (SlotRing, SlotEncoder), here with the modulus P = p^r over the tables
of hx_bgv_gf_create_pr (helib_amd/csrc/bgv_gf.h: bgv_gf's formulas modulo p^r on the lifted factors of bgv_crt.h, the
per-slot map inverted with unit pivots); this module adds the constructor.  A slot vector is an int64 array
[B, nslots, d] in [0, p^r), the d coefficients of a slot lowest first.

  encode / decode / encrypt[_batch] / encodePtxt / multByConstant / addConstant
                      bgv_pr's bodies on Galois-ring slots, through helib_amd.capi.bgvGf* on a table with r
  a [B, nslots] array means constants in the slots, and encodes to exactly the words bgv_pr gives
  decrypt[_batch]     a ciphertext whose space is p^k, 1 <= k <= r (after Ctxt.divideByP), is decoded through the p^r
                      tables and its slots reduced mod p^k, as bgv_pr does: the tables mod p^k are the p^k tables
  rotate1D / rotate / shift / shift1D / runningSums / totalSums     inherited from bgv_hypercube with the 0/1 masks encoded
                      mod p^r (bgv_pr._nextMask); they move whole slot values
  frobeniusAutomorph  Ctxt::frobeniusAutomorph: sigma: X -> X^p is a ring automorphism of Z_(p^r)[X] / G because it fixes
                      the lifted F_0 (it permutes the Teichmueller roots of F_0); slot alpha(X) -> alpha(X^(p^j)) mod G
  mulPlain / frobeniusPlain     the plain-side truths: the product in Z_(p^r)[X] / G and alpha -> sigma^j(alpha)
  getG / getDegree / getPPowR

At r = 1 the class gives helib_amd.bgv_gf.EncryptedArray's words.  Unpacking a slot into its d normal-basis
coordinates and back is helib_amd.intraslot.

Out of scope, refused with a message: a G other than the lifted F_0, d > 64, p^r >= 2^31, and every product of
helib_amd.bgv_matmul / bgv_gf_matmul over this class at r > 1 (their _modPOnly / _check refuse an array with r > 1;
helib_amd.bgv_gr_matmul has the linear maps on these slots).
Nothing here imports oracle/."""
from . import bgv_pr, capi, slot_ring
from .ckks import LogicError

MAX_D = 64                  # hxc::GF_MAX_D: the device kernels stage d - 1 <= 63 words of halo
MAX_MODULUS = 1 << 31       # hxc::CRT_MAX_P: the tables hold 32-bit words


class GrEncoder(slot_ring.SlotEncoder):
    """Galois-ring slot vectors <-> polynomials on the device (hx_bgv_gf_* on a table of hx_bgv_gf_create_pr); G is the
    lifted F_0, d + 1 integers in [0, p^r).  gens / ords: the hypercube of the slots follows these generators
    (capi.BgvGf), as ContextBuilder.gens().ords() chooses it in the reference"""

    def __init__(self, hxctx, p, r, gens=None, ords=None):
        super().__init__(hxctx, capi.BgvGf(hxctx, p, r, gens=gens, ords=ords))

    def encodeGathered(self, matrix, descs, maps, mul, idx, coeffs=False, flags_only=False):
        """the constants of a capi.BgvGfMatrix gathered, twisted and encoded without leaving the device
        (hx_bgv_gf_encode_gathered); flags_only: the non-zero flags alone"""
        return capi.bgvGfEncodeGathered(self.table, matrix, descs, maps, idx, mul, coeffs=coeffs, flags_only=flags_only)


class EncryptedArray(slot_ring.SlotRing, bgv_pr.EncryptedArray):
    """context: a BGV helib_amd.ctxt.ChainContext with gcd(p, m) = 1 and any r >= 1 with p^r < 2^31; hxctx: the
    capi.Context holding its primes; G: None for the lifted F_0, or its coefficients (constant first, any
    representatives mod p^r).  An injected encoder has GrEncoder's members (encode takes [B, nslots, d] or, for constants,
    [B, nslots]) and G.  self.p is the prime, self.P = p^r the modulus of the slots.  gens / ords: the generators of the
    slot hypercube and their orders (helib_amd.evalmap needs a hypercube that follows a factorisation of m); they go to
    the encoder this class builds, so they exclude an injected one."""

    _otherG = ("EncryptedArray: G is not the Hensel lift of F_0, the first factor of Phi_m mod p; another G "
               "needs a root of G in Z_(p^r)[X] / F_0 (the reference's FindRoots branch of mapToSlots), "
               "which is not built")

    def __init__(self, context, hxctx, G=None, encoder=None, gens=None, ords=None):
        p, r = context.p, int(getattr(context, "r", 1))
        if not getattr(context, "ckks", False):
            if r >= 1 and p ** r >= MAX_MODULUS:
                raise LogicError("EncryptedArray: p^r = %d^%d is not below 2^31 (the tables hold 32-bit words)" % (p, r))
            d, x = 1, p % context.m
            while x != 1 % context.m:
                x, d = x * p % context.m, d + 1
            if d > MAX_D:
                raise LogicError("EncryptedArray: d = ord_m(p) = %d: Galois-ring slots are built for d <= %d" % (d, MAX_D))
        if (gens is not None or ords is not None) and encoder is not None:
            raise LogicError("EncryptedArray: gens / ords choose the hypercube of the encoder this class builds; an injected "
                             "encoder brings its own through dims()")
        super().__init__(context, hxctx, encoder=encoder if encoder is not None else GrEncoder(hxctx, p, r, gens, ords))
        self._initRing(G)
