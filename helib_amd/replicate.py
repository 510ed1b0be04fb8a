"""Replication of slots: the reference's replicate.h family (src/replicate.cpp) over helib_amd.ctxt.Ctxt.

  replicate(ea, ct, pos)                   slot `pos` in every slot, in place (:26-38): one unit-selector mask, then replicate0
  replicate0(ea, ct, pos)                  the same for a ciphertext that is zero outside slot `pos` (:43-76): shift-and-add
                                           along every dimension, O(log nslots) rotations
  replicateAll(ea, ct, handler, recBound=64, repAux=None)
                                           all nslots replications at O(1) amortised rotations each, handed one by one to
                                           handler.handle (:353-683): one dimension at a time, blocks of 2^k slots replicated
                                           by shift-and-add (replicateOneBlock), then the recursion that halves them
                                           (recursiveReplicateDim), then the leftover slots of the dimension
  replicateAll(ea, ct, recBound=64)        the same, returning the list of ea.size() ciphertexts (:702-711)
  replicateAllOrig(ea, ct, handler, repAux=None)
                                           the recursion over the linear array, with EncryptedArray.rotate (:130-255)
  ReplicateHandler, RepAux, RepAuxDim      the handler's interface and the mask caches, reusable across calls
  replicatePlain(a, i, axis=-1)            on slot arrays (:737-740)

recBound is the reference's: positive, blocks of min(~log dSize, 2^recBound) slots where the heuristic of :554-562 says
so; 0, no recursion; negative, blocks of min(2^-recBound, 2^n).  Rotations along a non-native dimension are the
reference's "don't care" rotations, one automorphism each: what wraps lands on slots that are zero or are masked later.
An exception raised by the handler propagates: that is how a caller stops early.

It works over every BGV array class whose slots move as whole values (bgv, bgv_crt, bgv_hypercube, bgv_pr, bgv_gf,
bgv_gr); a CKKS array is refused.  Masks are encoded by the array's own mask encoder (_encodedMask) on the chain's
ciphertext and special primes, once per RepAuxDim.

hoisted (replicateAll only; None follows the module switch hoistNodes): an inner node of recursiveReplicateDim,
    masked = ct M;  left = masked + rho^+e(masked);  rest = ct - masked;  right = rest + rho^-e(rest)
costs two key switches, each with its own digit decomposition.  Since sigma_k(ct M) = sigma_k(ct) sigma_k(M),
    left = M ct + sigma_k+(M) rho^+e(ct),   right = (1 - M) ct + sigma_k-(1 - M) rho^-e(ct),
both from ONE BasicAutomorphPrecon of ct: BasicAutomorphPrecon.automorphMasked with n = 2 (n = 1 where the right half is
not needed, and at the leaf that fills positions past the extent), one hx_hoisted_mask_fan where Ctxt.fuseHoistedFan says
so.  The images sigma(M) are DoubleCRT.automorph of the encoded masks, cached in RepAuxDim beside them.  A node whose
rotation amount has no key-switching matrix of its own keeps the reference's form.  The hoisted form gives the same slots
in other words, with a slightly different noise estimate: the masks multiply after the key switch instead of before it,
and 1 - M is encoded on its own.  replicateAllOrig, replicate and replicate0 have the reference's form only.

There is no C++ twin of this module.  Nothing here imports oracle/."""
import numpy as np

from . import ctxt as hc
from .ckks import LogicError

# hoisted=None in replicateAll: the reference's form until the hoisted one has been measured ahead of it in every pair of
# tools/bench_replicate.py, with every output correct and its capacity within 2 bits
hoistNodes = False


class OutOfRangeError(IndexError):
    """helib::OutOfRangeError (assertInRange)"""


class ReplicateHandler:
    """ReplicateHandler (include/helib/replicate.h): handle receives every replicated ciphertext; earlyStop(d, k, prodDim)
    returning True hands over the partially replicated ciphertext at dimension d, block size 2^k (k = -1: before the
    dimension is begun), prodDim the product of the dimensions up to d"""

    def handle(self, ct):
        raise NotImplementedError

    def earlyStop(self, d, k, prodDim):
        return False


class _Table:
    """a vector that grows on access: tab(i) of the reference's RepAux, None where nothing is stored yet"""

    def __init__(self):
        self.v = []

    def get(self, i):
        return self.v[i] if i < len(self.v) else None

    def put(self, i, x):
        while len(self.v) <= i:
            self.v.append(None)
        self.v[i] = x
        return x


class RepAux:
    """RepAux: the masks of replicateAllOrig, (DoubleCRT, size) by level"""

    def __init__(self):
        self._tab = _Table()

    def tab(self, i):
        return self._tab.get(i)

    def setTab(self, i, x):
        return self._tab.put(i, x)


class RepAuxDim:
    """RepAuxDim: the masks of replicateAll, (DoubleCRT, size) by (dimension, level) -- tab for the recursion, tab1 for
    the range selections of replicateAllNextDim -- and, for the hoisted form, fan(d, i): the (A, B, sizes) lists of one
    node's automorphMasked"""

    def __init__(self):
        self._tab, self._tab1, self._fan = {}, {}, {}

    def _of(self, where, d):
        return where.setdefault(d, _Table())

    def tab(self, d, i):
        return self._of(self._tab, d).get(i)

    def setTab(self, d, i, x):
        return self._of(self._tab, d).put(i, x)

    def tab1(self, d, i):
        return self._of(self._tab1, d).get(i)

    def setTab1(self, d, i, x):
        return self._of(self._tab1, d).put(i, x)

    def fan(self, d, i):
        return self._of(self._fan, d).get(i)

    def setFan(self, d, i, x):
        return self._of(self._fan, d).put(i, x)


def NumBits(n):
    """NTL::NumBits of a non-negative integer"""
    return int(n).bit_length()


def GreatestPowerOfTwo(n):
    """the greatest k with 2^k <= n (:82-93)"""
    if n <= 0:
        raise ValueError("Cannot take log of negative number")
    return int(n).bit_length() - 1


def _check(ea):
    if getattr(getattr(ea, "cc", None), "ckks", False) or not hasattr(ea, "_encodedMask"):
        raise LogicError("replicate is built for the BGV array classes, where whole slot values move; a CKKS array is refused")


def _fullPrimes(ea):
    return list(ea.cc.ctxtPrimes) + list(ea.cc.specialPrimes)


def _encode(ea, mask):
    """FatEncodedPtxt(mask, fullPrimes): (DoubleCRT on the ciphertext and special primes, the size multByConstant takes)"""
    return ea._encodedMask(np.asarray(mask, dtype=np.int64), _fullPrimes(ea))


def _mul(ct, enc):
    if ct.parts:
        ct.multByConstant(*enc)
    return ct


def _rangeMask(ea, lo, hi):
    """SelectRange (:96-114) as slots"""
    n = ea.size()
    if not 0 <= lo <= hi:
        raise ValueError("Ill-formed interval")
    if hi > n:
        raise ValueError("Interval exceeds number of slots")
    i = np.arange(n)
    return ((i >= lo) & (i < hi)).astype(np.int64)


def _rangeMaskDim(ea, lo, hi, d):
    """SelectRangeDim (:263-289) as slots"""
    if not 0 <= d < ea.dimension():
        raise OutOfRangeError("dimension d must be within [0, ea.dimension())")
    if not 0 <= lo <= hi:
        raise ValueError("Ill-formed interval")
    if hi > ea.sizeOfDimension(d):
        raise LogicError("Interval exceeds dimension of d")
    c = ea._coords(d)
    return ((c >= lo) & (c < hi)).astype(np.int64)


def _dcAmount(ea, d, amt):
    """the element of Z_m^* of rotate1D(ctxt, d, amt, dontCare = true), or 1 for no move"""
    amt %= ea.sizeOfDimension(d)
    return ea.zMStar.genToPow(d, amt) if amt else 1


def _rotateDC(ea, ct, d, amt):
    """EncryptedArray::rotate1D with the don't-care flag (src/EncryptedArray.cpp:84-90): one automorphism, native or not"""
    k = _dcAmount(ea, d, amt)
    if k != 1:
        ct.smartAutomorph(k)
    return ct


def replicate(ea, ct, pos):
    """slot `pos` of ct in every slot, in place (:26-38)"""
    _check(ea)
    n = ea.size()
    if not 0 <= pos < n:
        raise OutOfRangeError("replication failed (pos must be in [0, nSlots))")
    mask = np.zeros(n, dtype=np.int64)
    mask[pos] = 1                                        # encodeUnitSelector
    if ct.parts:
        ct.multByConstant(*ea._encodedMask(mask, ct.primeSet))
    return replicate0(ea, ct, pos)


def replicate0(ea, ct, pos):
    """ct is zero outside slot `pos`, which ends up in every slot (:43-76)"""
    _check(ea)
    for d in range(ea.dimension()):
        if not ea.nativeDimension(d):
            _rotateDC(ea, ct, d, -ea.coordinate(d, pos))
        orig = ct.clone()
        sz = ea.sizeOfDimension(d)
        e = 1
        for j in range(NumBits(sz) - 2, -1, -1):         # bits k-2 down to 0
            tmp = ct.clone()
            _rotateDC(ea, tmp, d, e)
            ct += tmp
            e *= 2
            if (sz >> j) & 1:
                _rotateDC(ea, ct, d, 1)
                ct += orig
                e += 1
    return ct


# ---------------------------------------------------------------------------------------------
# the recursion over the linear array (:124-255)
# ---------------------------------------------------------------------------------------------
def _recursiveReplicate(ea, ct, n, k, pos, limit, aux, handler):
    if pos >= limit:
        return
    nSlots = ea.size()
    if k == 0:
        if (1 << n) >= nSlots:
            handler.handle(ct)
            return
        # replicate to fill positions [2^n, nSlots)
        enc = aux.tab(0) or aux.setTab(0, _encode(ea, _rangeMask(ea, 0, nSlots - (1 << n))))
        tmp = _mul(ct.clone(), enc)
        ea.rotate(tmp, 1 << n)
        tmp += ct
        handler.handle(tmp)
        return
    k -= 1
    enc = aux.tab(k + 1)
    if enc is None:
        i = np.arange(nSlots)
        enc = aux.setTab(k + 1, _encode(ea, ((i < (1 << n)) & ((i >> k) & 1 == 0)).astype(np.int64)))
    masked = _mul(ct.clone(), enc)
    left = masked.clone()
    ea.rotate(left, 1 << k)
    left += masked
    _recursiveReplicate(ea, left, n, k, pos, limit, aux, handler)
    del left
    pos += 1 << k
    if pos >= limit:
        return
    right = ct.clone()
    right -= masked
    masked = right.clone()
    ea.rotate(masked, -(1 << k))
    right += masked
    _recursiveReplicate(ea, right, n, k, pos, limit, aux, handler)


def replicateAllOrig(ea, ct, handler, repAux=None):
    """replicateAllOrig (:225-255)"""
    _check(ea)
    ct = ct.clone()
    ct.cleanUp()
    nSlots = ea.size()
    n = GreatestPowerOfTwo(nSlots)
    ct1 = ct.clone()
    if (1 << n) < nSlots:
        _mul(ct1, _encode(ea, _rangeMask(ea, 0, 1 << n)))
    aux = repAux if repAux is not None else RepAux()
    _recursiveReplicate(ea, ct1, n, n, 0, 1 << n, aux, handler)
    if (1 << n) < nSlots:
        ct1 = ct.clone()
        _mul(ct1, _encode(ea, _rangeMask(ea, 1 << n, nSlots)))
        ea.rotate(ct1, -(1 << n))
        _recursiveReplicate(ea, ct1, n, n, 1 << n, nSlots, aux, handler)


# ---------------------------------------------------------------------------------------------
# one dimension at a time (:257-683)
# ---------------------------------------------------------------------------------------------
def _replicateOneBlock(ea, ct, pos, blockSize, d):
    """ct is zero outside the block [pos blockSize, (pos + 1) blockSize) of dimension d, which is replicated over
    [0, floor(dSize / blockSize) blockSize) (:309-350)"""
    dSize = ea.sizeOfDimension(d)
    # the block moves to position 0, except in a native dimension that the block size divides
    if pos != 0 and (not ea.nativeDimension(d) or dSize % blockSize != 0):
        _rotateDC(ea, ct, d, -pos * blockSize)
    sz = dSize // blockSize
    if sz == 1:
        return
    e = 1
    orig = ct.clone()
    for j in range(NumBits(sz) - 2, -1, -1):
        tmp = ct.clone()
        _rotateDC(ea, tmp, d, e * blockSize)
        ct += tmp
        e *= 2
        if (sz >> j) & 1:
            _rotateDC(ea, ct, d, blockSize)
            ct += orig
            e += 1


class _Run:
    """what one replicateAll carries down its recursion"""

    def __init__(self, ea, recBound, aux, handler, hoisted, fused):
        self.ea, self.recBound, self.aux, self.handler, self.hoisted, self.fused = ea, recBound, aux, handler, hoisted, fused

    def _direct(self, ct, ks):
        """every amount has a key-switching matrix of its own, and the ciphertext is one BasicAutomorphPrecon takes"""
        if not self.hoisted or not ct.parts or ct.context.ckks:
            return False
        try:
            return all(k != 1 and ct._firstStep(k) == k for k in ks)
        except LookupError:
            return False

    def _nodeMask(self, d, extent, k):
        """the mask at index k + 1: coordinates below the extent whose bit k is 0 (:440-452)"""
        aux, ea = self.aux, self.ea
        enc = aux.tab(d, k + 1)
        if enc is None:
            c = ea._coords(d)
            enc = aux.setTab(d, k + 1, _encode(ea, ((c < extent) & ((c >> k) & 1 == 0)).astype(np.int64)))
        return enc

    def _nodeFan(self, d, extent, k, kp, km):
        """(A, B, sizes) of a hoisted node: A = (M, 1 - M), B = (sigma_k+(M), sigma_k-(1 - M))"""
        hit = self.aux.fan(d, k + 1)
        if hit is None:
            ea = self.ea
            m, sm = self._nodeMask(d, extent, k)
            c = ea._coords(d)
            w, sw = _encode(ea, 1 - ((c < extent) & ((c >> k) & 1 == 0)).astype(np.int64))
            mp, wm = m.copy(), w.copy()
            mp.automorph(kp)
            wm.automorph(km)
            # (an automorphism permutes the canonical embedding: the images have the sizes of the masks)
            hit = self.aux.setFan(d, k + 1, ([m, w], [mp, wm], [(sm, sm), (sw, sw)]))
        return hit

    def recursive(self, ct, d, extent, k, pos, limit, dimProd):
        """recursiveReplicateDim (:372-496)"""
        if pos >= limit:
            return
        ea, aux, handler = self.ea, self.aux, self.handler
        dSize = ea.sizeOfDimension(d)
        if k == 0:                                       # last level in this dimension: blocks of size 1
            if extent >= dSize:
                return self.nextDim(ct, d + 1, dimProd)
            # replicate to fill positions [extent, dSize)
            enc = aux.tab(d, 0) or aux.setTab(d, 0, _encode(ea, _rangeMaskDim(ea, 0, dSize - extent, d)))
            kr = _dcAmount(ea, d, extent)
            if self._direct(ct, [kr]):
                hit = aux.fan(d, 0)
                if hit is None:
                    img = enc[0].copy()
                    img.automorph(kr)
                    hit = aux.setFan(d, 0, (None, [img], [(-1.0, enc[1])]))
                tmp = hc.BasicAutomorphPrecon(ct).automorphMasked([kr], *hit, fused=self.fused)[0]
            else:
                tmp = _mul(ct.clone(), enc)
                _rotateDC(ea, tmp, d, extent)
                tmp += ct
            return self.nextDim(tmp, d + 1, dimProd)
        if handler.earlyStop(d, k, dimProd):
            handler.handle(ct)
            return
        k -= 1
        e = 1 << k
        needRight = pos + e < limit
        kp, km = _dcAmount(ea, d, e), _dcAmount(ea, d, -e)
        if self._direct(ct, [kp, km] if needRight else [kp]):
            A, B, sizes = self._nodeFan(d, extent, k, kp, km)
            nt = 2 if needRight else 1
            halves = hc.BasicAutomorphPrecon(ct).automorphMasked([kp, km][:nt], A[:nt], B[:nt], sizes[:nt], fused=self.fused)
            self.recursive(halves[0], d, extent, k, pos, limit, dimProd)
            if needRight:
                self.recursive(halves[1], d, extent, k, pos + e, limit, dimProd)
            return
        masked = _mul(ct.clone(), self._nodeMask(d, extent, k))
        left = masked.clone()
        _rotateDC(ea, left, d, e)
        left += masked
        self.recursive(left, d, extent, k, pos, limit, dimProd)
        del left
        pos += e
        if pos >= limit:
            return
        right = ct.clone()
        right -= masked
        masked = right.clone()
        _rotateDC(ea, masked, d, -e)
        right += masked
        self.recursive(right, d, extent, k, pos, limit, dimProd)

    def nextDim(self, ct, d, dimProd):
        """replicateAllNextDim (:498-660)"""
        ea, aux, handler, recBound = self.ea, self.aux, self.handler, self.recBound
        if d < 0:
            raise ValueError("dimension must be non-negative")
        if d >= ea.dimension() or handler.earlyStop(d, -1, dimProd):
            handler.handle(ct)
            return
        dSize = ea.sizeOfDimension(d)
        dimProd *= dSize
        n = GreatestPowerOfTwo(dSize)
        if recBound >= 0:                                # the heuristic bound (:554-562)
            k = 0
            if dSize > 2 and dimProd * NumBits(dSize) > ea.size() // 8:
                k = min(NumBits(NumBits(dSize)) - 1, n, recBound)
        else:
            k = min(-recBound, n)
        blockSize = 1 << k
        numBlocks = dSize // blockSize
        extent = numBlocks * blockSize
        ct1 = ct.clone()
        if extent < dSize:                               # only the slots [0, extent) of this dimension
            enc = aux.tab1(d, 0) or aux.setTab1(d, 0, _encode(ea, _rangeMaskDim(ea, 0, extent, d)))
            _mul(ct1, enc)
        if numBlocks == 1:
            self.recursive(ct1, d, extent, k, 0, extent, dimProd)
        else:
            for pos in range(numBlocks):
                ct2 = ct1.clone()
                if ct2.parts:                            # SelectRangeDim on the ciphertext: encoded on its own primes
                    ct2.multByConstant(*ea._encodedMask(_rangeMaskDim(ea, pos * blockSize, (pos + 1) * blockSize, d),
                                                        ct2.primeSet))
                _replicateOneBlock(ea, ct2, pos, blockSize, d)
                self.recursive(ct2, d, extent, k, 0, extent, dimProd)
        if extent < dSize:                               # the leftover slots
            ct1 = ct.clone()
            enc = aux.tab1(d, 1) or aux.setTab1(d, 1, _encode(ea, _rangeMaskDim(ea, extent, dSize, d)))
            _mul(ct1, enc)
            _rotateDC(ea, ct1, d, -extent)
            _replicateOneBlock(ea, ct1, 0, blockSize, d)
            self.recursive(ct1, d, extent, k, extent, dSize, dimProd)


class _Collector(ReplicateHandler):
    """ExplicitReplicator (:690-699)"""

    def __init__(self):
        self.v = []

    def handle(self, ct):
        self.v.append(ct.clone())


def replicateAll(ea, ct, handler=None, recBound=64, repAux=None, hoisted=None, fused=None):
    """replicateAll (:666-683), and with no handler (or recBound in its place, as the reference's second overload takes
    it) the list of ea.size() ciphertexts (:702-711).  hoisted: see the module docstring; fused is handed to
    automorphMasked (None: Ctxt.fuseHoistedFan)."""
    _check(ea)
    if handler is not None and not hasattr(handler, "handle"):
        handler, recBound = None, int(handler)
    collect = handler is None
    if collect:
        handler = _Collector()
    hoisted = hoistNodes if hoisted is None else bool(hoisted)
    ct = ct.clone()
    ct.cleanUp()
    aux = repAux if repAux is not None else RepAuxDim()
    _Run(ea, recBound, aux, handler, hoisted, fused).nextDim(ct, 0, 1)
    return handler.v if collect else None


def replicatePlain(a, i, axis=-1):
    """replicate on a plaintext array (:717-740): slot i in every slot, `axis` being the slot axis of a"""
    a = np.asarray(a)
    n = a.shape[axis]
    if not 0 <= i < n:
        raise OutOfRangeError("Attempted to access out-of-range data")
    return np.repeat(np.take(a, [i], axis=axis), n, axis=axis)
