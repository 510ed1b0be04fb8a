"""EncryptedArray (include/helib/EncryptedArray.h, src/EncryptedArray.cpp, src/PAlgebra.cpp) over the device for BGV
with d = ord_m(p) = 1 and r = 1: the plaintext prime p = 1 mod m splits Phi_m into phi(m) linear factors, a slot is an
integer mod p, and slot vectors -- numpy int64 arrays of shape [B, phi(m)] (B independent vectors: a batch) -- go into
ciphertexts and come back out.

  maps                F_0 = X - rho, rho the largest primitive m-th root of unity mod p (the smallest factor by
                      poly_comp, src/PAlgebra.cpp:67-81); F_i = X - rho^(1/t_i mod m), t_i = zMStar.ith_rep(i)
                      (:726-733); encode(a) = balanced(H), H of degree < phi(m) with H(rho^(1/t_i)) = a_i mod p
                      (CRT_reconstruct, src/EncryptedArray.cpp:438-447); decode: slot i = H(rho^(1/t_i)) mod p
  encode / decode     helib_amd.capi.bgvEncode / bgvEmbed (hx_bgv_encode / hx_bgv_embed): the engine's transform for
                      the prime p between a scatter and a lift kernel
  encrypt[_batch]     encode with the factor Q mod p of PubKey::Encrypt's balanced_MulMod (src/keys.cpp:358-488) folded
                      in, then PubKey.EncryptBatch
  decrypt[_batch]     the secret-key inner product, then hx_bgv_decode (toPoly + PolyRed on the device, the factor of
                      SecKey::Decrypt, the transform mod p; one download)
  rotate1D            every dimension is native at d = 1: one automorphism (src/EncryptedArray.cpp:65-97)
  encodePtxt / multByConstant / addConstant   the EncodedPtxt interface (src/Ctxt.cpp:1952-2000, 2187-2224)
  maskSlots           maskTable[i][j] (PAlgebraModDerived::genMaskTable, src/PAlgebra.cpp:1316-1338) as its 0/1 slot
                      vector; a mask is encoded by the device encoder when it is used and kept in a small cache
  shift1D / rotate / shift                    the linear array over the hypercube (src/EncryptedArray.cpp:130-174,
                      181-285, 288-355): per dimension below the last one  tmp = ct * mask; ct -= tmp  -- copy /
                      multByConstant / -= or, fused=True, one device call for the parts (capi.maskSplit: hx_mask_split,
                      DESIGN 3.9d); the words and the bookkeeping (lnNoise, primeSet, intFactor, ptxtSpace) are the same
                      either way, fused=None follows EncryptedArray.fuseMaskSplit
  totalSums / runningSums                     src/EncryptedArray.cpp:695-736
  matrix products     helib_amd.bgv_matmul: MatMul1DExec / MatMulFullExec over rotate1D, with the diagonals read out of a
                      device-resident matrix (DeviceEncoder.matrix / encodeDiagonals: hx_bgv_encode_diagonals)

Out of scope: d > 1 (helib_amd.bgv_crt, bgv_hypercube and bgv_gf cover it) and p^r with r > 1 (helib_amd.bgv_pr) --
refused with HX_ERR_UNSUPPORTED.  Nothing here imports
oracle/."""
import collections
import math

import numpy as np

from . import capi
from . import ctxt as hc
from . import hostnt
from .ckks import LogicError, innerProduct
from .linalg import _like


class DeviceEncoder:
    """slot vectors <-> polynomials on the device (hx_bgv_*).  An EncryptedArray can be given another object with these
    members (tests drive the host control flow over a CPU backend that way)."""

    def __init__(self, hxctx, p):
        self.g = hxctx
        self.table = capi.BgvSlots(hxctx, p)

    def dims(self):
        """(gens, ords) of Z_m^*'s hypercube, as the device tables order the slots"""
        return self.table.gens, self.table.ords

    def encode(self, v, mul, idx, coeffs=False):
        return capi.bgvEncode(self.table, v, idx, mul, coeffs=coeffs)

    max_batch = 64      # diagonals per encodeDiagonals call: the scratch is max_batch transforms mod p

    def matrix(self, a, dim=-1):
        """a plaintext matrix on the device: [phi(m), phi(m)] by slot (dim = -1) or [D, D] by the coordinate in
        dimension dim"""
        return capi.BgvMatrix(self.table, a, dim)

    def encodeDiagonals(self, matrix, diags, idx=None, coeffs=False):
        """diags: [(off, rot_dim, rot_amt)] -> (DoubleCRT batch len(diags) over idx, zzX or None, non-zero flags);
        idx = None: the flags alone"""
        return capi.bgvEncodeDiagonals(self.table, matrix, diags, idx, coeffs=coeffs)

    def split(self, poly):
        return capi.splitBatch(poly)

    def embed(self, coeffs):
        return capi.bgvEmbed(self.table, coeffs)

    def decode(self, acc, factor_inv):
        return capi.bgvDecode(self.table, acc, factor_inv)

    def norm(self, coeffs):
        """embeddingLargestCoeff of every zzX [B, phi(m)]"""
        return capi.embeddingLargestCoeff(self.g, np.asarray(coeffs, dtype=np.float64))


class EncodedPtxt:
    """EncodedPtxt_BGV (include/helib/EncodedPtxt.h): the zzX of the encoded slots with its plaintext space.  The
    slots are kept as well: the reference expands the zzX to a ciphertext's primes when it is used
    (FatEncodedPtxt::expand); here that is one more encode on the device."""

    def __init__(self, ea, v, poly, ptxtSpace):
        self.ea, self.v, self.poly, self.ptxtSpace = ea, v, poly, ptxtSpace


class EncryptedArray:
    """context: a BGV helib_amd.ctxt.ChainContext with p = 1 mod m and r = 1; hxctx: the capi.Context holding its
    primes."""

    def __init__(self, context, hxctx, encoder=None):
        if getattr(context, "ckks", False):
            raise LogicError("EncryptedArray: a CKKS context takes EncryptedArrayCx")
        self.cc, self.g = context, hxctx
        self.m, self.p = context.m, context.p
        if getattr(context, "r", 1) != 1 or context.ptxtSpace != self.p:
            raise capi.HxError(capi.HX_ERR_UNSUPPORTED,
                               "BGV slots: plaintext space p^r with r > 1 (Hensel lifting) is not built")
        if math.gcd(self.p, self.m) == 1 and self.p % self.m != 1 % self.m:
            d, x = 1, self.p % self.m
            while x != 1:
                x, d = x * self.p % self.m, d + 1
            raise capi.HxError(capi.HX_ERR_UNSUPPORTED, "d = ord_m(p) = %d for p = %d, m = %d: only d = 1 (p = 1 mod m, "
                               "slots in Z_p) is built" % (d, self.p, self.m))
        self.enc = encoder if encoder is not None else DeviceEncoder(hxctx, self.p)
        dims = getattr(self.enc, "dims", None)
        gens, ords = dims() if dims is not None else ((), ())
        self.zMStar = hostnt.ZmStar(self.m, self.p, gens, ords)

    # ---- geometry ----
    def size(self):
        return self.cc.phim

    def dimension(self):
        return self.zMStar.numOfGens()

    def sizeOfDimension(self, i):
        return self.zMStar.OrderOf(i)

    def nativeDimension(self, i):
        return self.zMStar.SameOrd(i)

    def getP(self):
        return self.p

    def getDegree(self):
        return 1

    def coordinate(self, i, k):
        """PAlgebra::coordinate: the exponent of generator i in slot k"""
        for d in self.zMStar.ords[i + 1:]:
            k //= d
        return k % self.zMStar.ords[i]

    def _slots(self, v):
        a = np.asarray(v)
        if a.dtype == object or a.dtype.kind not in "iu" or a.dtype == np.uint64:
            a = np.array([int(x) % self.p for x in a.reshape(-1)], dtype=np.int64).reshape(a.shape)
        a = a.astype(np.int64)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        if a.ndim != 2 or a.shape[1] > self.size():
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "more values than slots")
        return a

    # ---- encode / decode ----
    def encode(self, v, idx=None, coeffs=False, mul=1):
        """-> DoubleCRT over idx (default: the ctxt primes) in evaluation form holding balanced(mul * H mod p);
        coeffs=True: (DoubleCRT, int64 coefficients [B, phi(m)])"""
        idx = list(self.cc.ctxtPrimes) if idx is None else list(idx)
        return self.enc.encode(self._slots(v), mul, idx, coeffs=coeffs)

    def encodeCoeffs(self, v, mul=1):
        """the zzX alone, [B, phi(m)]"""
        return self.enc.encode(self._slots(v), mul, [], coeffs=True)[1]

    def decode(self, coeffs):
        """EncryptedArray::decode of plaintext polynomials [B, phi(m)] -> int64 slots [B, phi(m)] in [0, p)"""
        c = np.asarray(coeffs)
        if c.dtype == object:
            c = np.array([int(x) % self.p for x in c.reshape(-1)], dtype=np.int64).reshape(c.shape)
        return self.enc.embed(np.atleast_2d(c.astype(np.int64)))

    # ---- encryption ----
    def encrypt(self, pk, v):
        v = self._slots(v)
        if v.shape[0] != 1:
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "encrypt takes one vector: use encrypt_batch")
        return self.encrypt_batch(pk, v)

    def encrypt_batch(self, pk, vs):
        """B vectors -> one batched Ctxt, element b being what PubKey.Encrypt gives for the encoding of vs[b] (the
        samples in the order of B consecutive calls): the plaintext term balanced(ptxt * Q mod p) comes from the
        encoder"""
        if pk.ptxtSpace != self.p:
            raise LogicError("EncryptedArray.encrypt: the key's plaintext space is not p")
        idx = list(self.cc.ctxtPrimes)
        return pk.EncryptBatch(self.encode(vs, idx, mul=self.cc.productOfPrimes(idx) % self.p))

    def decrypt_batch(self, ct, sk):
        """SecKey::Decrypt + decode for every element of a batched Ctxt -> int64 [B, phi(m)] in [0, p)"""
        if ct.ptxtSpace != self.p:
            raise LogicError("EncryptedArray.decrypt: the ciphertext's plaintext space is not p")
        acc = innerProduct(sk, ct)
        if acc is None:
            return np.zeros((1, self.size()), dtype=np.int64)
        factor = self.cc.productOfPrimes(sorted(ct.primeSet)) % self.p * ct.intFactor % self.p   # src/keys.cpp:1388-1405
        return self.enc.decode(acc, pow(factor, -1, self.p))

    def decrypt(self, ct, sk):
        return self.decrypt_batch(ct, sk)[0]

    # ---- the EncodedPtxt interface ----
    def encodePtxt(self, v):
        """EncryptedArray::encode(EncodedPtxt&, array): the zzX and the plaintext space"""
        v = self._slots(v)
        return EncodedPtxt(self, v, self.encodeCoeffs(v), self.p)

    def _space(self, ct, eptxt):
        if ct.ptxtSpace != eptxt.ptxtSpace:   # the reference reduces the plaintext space to the gcd: 1 for a prime
            raise LogicError("EncryptedArray: the ciphertext's plaintext space is not p")

    def multByConstant(self, ct, eptxt):
        """Ctxt::multByConstant(const EncodedPtxt&) (src/Ctxt.cpp:1958-2000): the zzX expanded to the ciphertext's
        primes, its size embeddingLargestCoeff(zzX) (FatEncodedPtxt_BGV)"""
        if not ct.parts:
            return ct
        self._space(ct, eptxt)
        size = float(np.max(self.enc.norm(eptxt.poly)))
        return ct.multByConstant(self.enc.encode(eptxt.v, 1, sorted(ct.primeSet)), size)

    def addConstant(self, ct, eptxt, neg=False):
        """Ctxt::addConstant(const EncodedPtxt_BGV&, neg) (src/Ctxt.cpp:2187-2224): the constant is scaled by
        f = intFactor * Q mod p in the plaintext space -- balanced(f * zzX mod p), here the encoder's `mul` -- and
        the noise grows by that polynomial's embeddingLargestCoeff"""
        self._space(ct, eptxt)
        p = self.p
        primes = sorted(ct.primeSet)
        f = self.cc.productOfPrimes(primes) % p * ct.intFactor % p if p > 2 else 1
        dcrt, poly = self.enc.encode(eptxt.v, f, primes, coeffs=True)
        ct.lnNoise = hc.logaddexp(ct.lnNoise, hc._ln(float(np.max(self.enc.norm(poly)))))
        if "1" not in ct.parts:
            raise RuntimeError("Ctxt::addPart: no part pointing at 1")
        if neg:
            ct.parts["1"] -= dcrt
        else:
            ct.parts["1"] += dcrt
        return ct

    # ---- between slots ----
    def rotate1D(self, ct, i, amt):
        """EncryptedArray::rotate1D (src/EncryptedArray.cpp:65-97) on a native dimension: the slot whose coordinate
        in dimension i is c moves to coordinate c + amt (mod the order)"""
        if not 0 <= i < self.dimension():
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "i must be between 0 and dimension()")
        ord_ = self.sizeOfDimension(i)
        amt %= ord_
        if amt == 0:
            return ct
        return ct.smartAutomorph(self.zMStar.genToPow(i, amt))

    # ---- masks ----
    MASK_CACHE = 32     # encoded masks kept per EncryptedArray (least recently used goes first)
    fuseMaskSplit = False  # fused=None: term by term until hx_mask_split has been measured as the faster form

    def _coords(self, i):
        """PAlgebra::coordinate(i, k) for every slot k"""
        stride = 1
        for d in self.zMStar.ords[i + 1:]:
            stride *= d
        return np.arange(self.size(), dtype=np.int64) // stride % self.zMStar.ords[i]

    def maskSlots(self, i, j):
        """maskTable[i][j] (genMaskTable, src/PAlgebra.cpp:1316-1338) as slots: 1 where coordinate(i, k) >= j -- all
        ones for j = 0, all zeros for j = OrderOf(i).  The table's polynomial is the encoding of this vector (a sum of
        the idempotents crtTable[k])."""
        if not 0 <= i < self.dimension():
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "i must be between 0 and dimension()")
        if not 0 <= j <= self.sizeOfDimension(i):
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "j must be between 0 and the order of dimension i")
        return (self._coords(i) >= j).astype(np.int64)

    def _nextMask(self, mask, i, v):
        """mask * (maskTable[i][v] - maskTable[i][v + 1]) + maskTable[i][v + 1]  (mod Phi_m)
        (src/EncryptedArray.cpp:280-281, 344-345): products mod Phi_m are slot-wise, so it is done on the slots"""
        hi = self.maskSlots(i, v + 1)
        return (mask * (self.maskSlots(i, v) - hi) + hi) % self.p

    def _encodedMask(self, mask, primeSet):
        """(DoubleCRT(balanced_zzX(mask)) on primeSet, embeddingLargestCoeff of that zzX -- the size
        Ctxt::multByConstant(const zzX&) takes, src/Ctxt.cpp:1872-1882).  Cached by (mask bytes, prime set), at most
        MASK_CACHE entries: totalSums asks for the same few masks at every step."""
        cache = self.__dict__.setdefault("_masks", collections.OrderedDict())
        idx = sorted(primeSet)
        key = (mask.tobytes(), tuple(idx))
        hit = cache.get(key)
        if hit is not None:
            cache.move_to_end(key)
            return hit
        dcrt, poly = self.enc.encode(mask.reshape(1, -1), 1, idx, coeffs=True)
        hit = cache[key] = (dcrt, float(np.max(self.enc.norm(poly))))
        while len(cache) > self.MASK_CACHE:
            cache.popitem(last=False)
        return hit

    def _multByMask(self, ct, mask):
        """ctxt.multByConstant(balanced_zzX(mask))"""
        if ct.parts:
            ct.multByConstant(*self._encodedMask(mask, ct.primeSet))
        return ct

    def _maskSplit(self, ct, mask, fused=None):
        """tmp = ctxt; tmp.multByConstant(mask_poly); ctxt -= tmp  (src/EncryptedArray.cpp:270-274, 334-338) -> tmp.
        Fused: one capi.maskSplit per pair of parts, and the bookkeeping of the three calls done here --
        multByConstant's lnNoise + ln(size) on tmp, addCtxt's noise and ptxtMag sums on ctxt (same prime set, plaintext
        space and intFactor on both sides, so addCtxt changes nothing else).  It needs parts and a backend with
        maskSplit (the scheme is BGV and the mask is encoded on ct's own prime set by construction); fused=True
        insists on it, fused=False goes term by term."""
        if not ct.parts:
            return ct.clone()
        ct._materializeTensor()
        can = hasattr(ct.ops, "maskSplit")
        if fused and not can:
            raise LogicError("EncryptedArray: fused=True, but the mask split cannot be fused here")
        if not ((self.fuseMaskSplit if fused is None else fused) and can):
            tmp = ct.clone()
            self._multByMask(tmp, mask)
            ct -= tmp
            return tmp
        dcrt, size = self._encodedMask(mask, ct.primeSet)
        keep = list(ct.parts.items())
        take = {h: ct.ops.likeUninit(p) for h, p in keep}
        for a in range(0, len(keep), 2):
            (h0, k0), (h1, k1) = keep[a], keep[a + 1] if a + 1 < len(keep) else (None, None)
            ct.ops.maskSplit(k0, k1, take[h0], take[h1] if k1 is not None else None, dcrt)
        tmp = _like(ct, take)
        tmp.lnNoise = tmp.lnNoise + hc._ln(size)
        ct.ptxtMag += tmp.ptxtMag
        ct.lnNoise = hc.logaddexp(ct.lnNoise, tmp.lnNoise)
        return tmp

    # ---- the linear array ----
    def shift1D(self, ct, i, k):
        """EncryptedArray::shift1D (src/EncryptedArray.cpp:130-174): k positions along dimension i with zero fill"""
        if not 0 <= i < self.dimension():
            raise capi.InvalidArgument(capi.HX_ERR_INVALID,
                                       "i must be non-negative and less than the PAlgebra's generator count")
        ord_ = self.sizeOfDimension(i)
        if k <= -ord_ or k >= ord_:
            ct.clear()
            return ct
        amt = k % ord_                       # in [1, ord - 1]
        if amt == 0:
            return ct
        mask = self.maskSlots(i, ord_ - amt)
        if k < 0:
            val = self.zMStar.genToPow(i, amt - ord_)
        else:
            mask = 1 - mask
            val = self.zMStar.genToPow(i, amt)
        self._multByMask(ct, mask)           # zero out slots where mask = 0
        return ct.smartAutomorph(val)

    def rotate(self, ct, amt, fused=None):
        """EncryptedArray::rotate (src/EncryptedArray.cpp:181-285): slot j moves to slot j + amt mod nslots"""
        ngens = self.dimension()
        if ngens == 1:                       # simple case: just one generator
            return self.rotate1D(ct, 0, amt)
        amt %= self.size()                   # in [1, nslots - 1]
        if amt == 0:
            return ct
        # one dimension at a time
        i = ngens - 1
        v = self.coordinate(i, amt)
        mask = self.maskSlots(i, v)
        # :221-264 fold a non-native last dimension's own mask into the loop.  At d = 1 <p> is trivial, every
        # generator has the same order in Z_m^* / <p> as in Z_m^* (SameOrd), and that branch cannot be reached.
        if not self.nativeDimension(i):
            raise LogicError("EncryptedArray::rotate: a non-native dimension at d = 1")
        self.rotate1D(ct, i, v)
        for i in range(i - 1, -1, -1):
            v = self.coordinate(i, amt)
            tmp = self._maskSplit(ct, mask, fused)      # tmp: the slots in which mask = 1; ct: those with mask = 0
            self.rotate1D(tmp, i, v)
            self.rotate1D(ct, i, v + 1)
            ct += tmp
            if i > 0:
                mask = self._nextMask(mask, i, v)
        return ct

    def shift(self, ct, k, fused=None):
        """EncryptedArray::shift (src/EncryptedArray.cpp:288-355): slot j moves to slot j + k, zeros come in"""
        ngens = self.dimension()
        if ngens == 1:
            return self.shift1D(ct, 0, k)
        n = self.size()
        if k <= -n or k >= n:                # an all-zero ciphertext
            return ct.multByScalar(0)
        amt = k % n                          # in [1, nslots - 1]
        if amt == 0:
            return ct
        i = ngens - 1
        v = self.coordinate(i, amt)
        mask = self.maskSlots(i, v)
        self.rotate1D(ct, i, v)
        for i in range(i - 1, -1, -1):
            v = self.coordinate(i, amt)
            tmp = self._maskSplit(ct, mask, fused)
            if i > 0:
                self.rotate1D(ct, i, v + 1)
                self.rotate1D(tmp, i, v)
                ct += tmp
                mask = self._nextMask(mask, i, v)
            else:
                if k < 0:
                    v -= self.sizeOfDimension(0)
                self.shift1D(tmp, 0, v)
                self.shift1D(ct, 0, v + 1)   # may leave ct empty: += then copies tmp (Ctxt::addCtxt, src/Ctxt.cpp:1420-1426)
                ct += tmp
        return ct

    def runningSums(self, ct, fused=None):
        """runningSums (src/EncryptedArray.cpp:695-706): slot j <- sum of slots 0 .. j"""
        n = self.size()
        shamt = 1
        while shamt < n:
            tmp = ct.clone()
            self.shift(tmp, shamt, fused=fused)
            ct += tmp                        # ct = ct + (ct >> shamt)
            shamt *= 2
        return ct

    def totalSums(self, ct, fused=None):
        """totalSums (src/EncryptedArray.cpp:708-736): every slot <- the sum of all slots; the recursion follows the
        bits of n, which need not be a power of two"""
        n = self.size()
        if n == 1:
            return ct
        orig = ct.clone()
        e = 1
        for i in range(n.bit_length() - 2, -1, -1):
            tmp1 = ct.clone()
            self.rotate(tmp1, e, fused=fused)
            ct += tmp1                       # ct = ct + (ct >>> e)
            e *= 2
            if (n >> i) & 1:
                tmp2 = orig.clone()
                self.rotate(tmp2, e, fused=fused)
                ct += tmp2                   # ct = ct + (orig >>> e)
                e += 1
        return ct
