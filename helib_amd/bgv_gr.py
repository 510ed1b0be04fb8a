"""EncryptedArray(context, G) for the plaintext space p^r, r >= 1, with G the Hensel lift of F_0, the first factor of
Phi_m mod p: every slot is an element of the Galois ring Z_(p^r)[X] / G, d = deg G = ord_m(p).  It is the array
RecryptData::init builds over p^(e - e' + r) (src/recryption.cpp:310-343).  helib_amd.bgv_pr keeps one integer mod p^r per
slot (G = X) and helib_amd.bgv_gf an element of GF(p^d) at r = 1; this class has bgv_gf's members with the modulus p^r
where they say p, over the tables of hx_bgv_gf_create_pr (helib_amd/csrc/bgv_gf.h: bgv_gf's formulas modulo p^r on the
lifted factors of bgv_crt.h, the per-slot map inverted with unit pivots).  A slot vector is an int64 array
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
import numpy as np

from . import bgv_pr, capi
from .ckks import LogicError

MAX_D = 64                  # hxc::GF_MAX_D: the device kernels stage d - 1 <= 63 words of halo
MAX_MODULUS = 1 << 31       # hxc::CRT_MAX_P: the tables hold 32-bit words


class GrEncoder:
    """Galois-ring slot vectors <-> polynomials on the device (hx_bgv_gf_* on a table of hx_bgv_gf_create_pr):
    bgv_gf.GfEncoder's members, and G (the lifted F_0, d + 1 integers in [0, p^r)).  gens / ords: the hypercube of the
    slots follows these generators (capi.BgvGf), as ContextBuilder.gens().ords() chooses it in the reference"""

    def __init__(self, hxctx, p, r, gens=None, ords=None):
        self.g = hxctx
        self.table = capi.BgvGf(hxctx, p, r, gens=gens, ords=ords)
        self.G = list(self.table.G)

    def dims(self):
        """(gens, signed ords) of the hypercube of Z_m^* / <p>"""
        return self.table.gens, self.table.ords

    def encode(self, v, mul, idx, coeffs=False):
        return capi.bgvGfEncode(self.table, v, idx, mul, coeffs=coeffs)

    def encodeGathered(self, matrix, descs, maps, mul, idx, coeffs=False, flags_only=False):
        """the constants of a capi.BgvGfMatrix gathered, twisted and encoded without leaving the device
        (hx_bgv_gf_encode_gathered); flags_only: the non-zero flags alone"""
        return capi.bgvGfEncodeGathered(self.table, matrix, descs, maps, idx, mul, coeffs=coeffs, flags_only=flags_only)

    def split(self, poly):
        return capi.splitBatch(poly)

    def embed(self, coeffs):
        return capi.bgvGfEmbed(self.table, coeffs)

    def decode(self, acc, factor_inv):
        return capi.bgvGfDecode(self.table, acc, factor_inv)

    def norm(self, coeffs):
        """embeddingLargestCoeff of every zzX [B, phi(m)]"""
        return capi.embeddingLargestCoeff(self.g, np.asarray(coeffs, dtype=np.float64))


class EncryptedArray(bgv_pr.EncryptedArray):
    """context: a BGV helib_amd.ctxt.ChainContext with gcd(p, m) = 1 and any r >= 1 with p^r < 2^31; hxctx: the
    capi.Context holding its primes; G: None for the lifted F_0, or its coefficients (constant first, any
    representatives mod p^r).  An injected encoder has GrEncoder's members (encode takes [B, nslots, d] or, for constants,
    [B, nslots]) and G.  self.p is the prime, self.P = p^r the modulus of the slots.  gens / ords: the generators of the
    slot hypercube and their orders (helib_amd.evalmap needs a hypercube that follows a factorisation of m); they go to
    the encoder this class builds, so they exclude an injected one."""

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
        P, d = self.P, self.zMStar.ordP
        self.G = [int(x) % P for x in self.enc.G]
        if len(self.G) != d + 1 or self.G[d] != 1:
            raise LogicError("EncryptedArray: the encoder's G is not monic of degree d = %d" % d)
        if G is not None:
            g = [int(x) % P for x in G]
            while g and g[-1] == 0:
                g.pop()
            if len(g) - 1 < d:
                raise LogicError("EncryptedArray: deg G = %d < d = %d is not built (only G = F_0, of degree d)" % (len(g) - 1, d))
            if g != self.G:
                raise LogicError("EncryptedArray: G is not the Hensel lift of F_0, the first factor of Phi_m mod p; another G "
                                 "needs a root of G in Z_(p^r)[X] / F_0 (the reference's FindRoots branch of mapToSlots), "
                                 "which is not built")
        self._G = np.array(self.G[:d], dtype=np.int64)
        self._frob = None

    def getG(self):
        return list(self.G)

    def getDegree(self):
        return self.zMStar.ordP

    def _slots(self, v):
        """-> int64 [B, nslots, d].  One axis: one vector of constants; two: [B, <= nslots] constants; three:
        [B, <= nslots, <= d]; what is missing is zero."""
        a = np.asarray(v)
        if a.dtype == object or a.dtype.kind not in "iu" or a.dtype == np.uint64:
            a = np.array([int(x) % self.P for x in a.reshape(-1)], dtype=np.int64).reshape(a.shape)
        a = a.astype(np.int64)
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim == 2:
            a = a[:, :, None]
        n, d = self.size(), self.getDegree()
        if a.ndim != 3 or a.shape[1] > n or a.shape[2] > d:
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "more values than slots, or more coefficients than d")
        out = np.zeros((a.shape[0], n, d), dtype=np.int64)
        out[:, :a.shape[1], :a.shape[2]] = a
        return out

    def decrypt_batch(self, ct, sk):
        """SecKey::Decrypt + decode -> int64 [B, nslots, d] in [0, p^k), p^k the ciphertext's space (k <= r)"""
        out = super().decrypt_batch(ct, sk)
        return out if out.ndim == 3 else self._slots(out)

    def frobeniusAutomorph(self, ct, j):
        """EncryptedArray::frobeniusAutomorph: every slot alpha -> sigma^j(alpha) = alpha(X^(p^j)) mod G, by
        Ctxt::frobeniusAutomorph (X -> X^(p^j) maps Phi_m's lifted factor F_i to itself, so it acts slot by slot, and the
        slot maps are ring maps); j counts mod d"""
        ct.frobeniusAutomorph(j % self.getDegree())
        return ct

    # ---- the plain side ----
    def _mul(self, a, b):
        """the product in Z_(p^r)[X] / G along the last axis of two arrays [..., d] with entries in [0, p^r)"""
        P, d = self.P, self.getDegree()
        w = np.zeros(np.broadcast_shapes(a.shape, b.shape)[:-1] + (2 * d - 1,), dtype=np.int64)
        for l in range(d):                                  # every product is below p^2r < 2^62 and reduced at once
            w[..., l:l + d] = (w[..., l:l + d] + a[..., l:l + 1] * b % P) % P
        for k in range(2 * d - 2, d - 1, -1):               # X^k = -X^(k - d) (G - X^d)
            w[..., k - d:k] = (w[..., k - d:k] - w[..., k:k + 1] * self._G % P) % P
        return np.ascontiguousarray(w[..., :d])

    def mulPlain(self, a, b):
        """the slot-wise product in Z_(p^r)[X] / G -> int64 [B, nslots, d]"""
        return self._mul(self._slots(a) % self.P, self._slots(b) % self.P)

    def _frobenius(self):
        """row l = X^(l p) mod G: sigma(alpha) = sum_l alpha_l X^(l p), sigma fixing the coefficients.  (At r > 1 sigma is
        not alpha -> alpha^p: that map is not additive modulo p^2.)"""
        if self._frob is None:
            P, p, d = self.P, self.p, self.getDegree()
            one, x = np.zeros((1, 1, d), dtype=np.int64), np.zeros((1, 1, d), dtype=np.int64)
            one[0, 0, 0] = 1
            if d == 1:
                x[0, 0, 0] = -self.G[0] % P                 # X mod the linear G
            else:
                x[0, 0, 1] = 1
            xp, e = one, p                                  # X^p by square and multiply
            while e:
                if e & 1:
                    xp = self._mul(xp, x)
                x = self._mul(x, x)
                e >>= 1
            rows, cur = [], one
            for _ in range(d):
                rows.append(cur[0, 0])
                cur = self._mul(cur, xp)
            self._frob = np.stack(rows)
        return self._frob

    def frobeniusPlain(self, a, j):
        """every slot alpha -> sigma^j(alpha) = alpha(X^(p^j)) mod G -> int64 [B, nslots, d]"""
        a, P, d = self._slots(a) % self.P, self.P, self.getDegree()
        F = self._frobenius()
        for _ in range(j % d):
            nxt = np.zeros_like(a)
            for l in range(d):
                nxt = (nxt + a[:, :, l:l + 1] * F[l] % P) % P
            a = nxt
        return a
