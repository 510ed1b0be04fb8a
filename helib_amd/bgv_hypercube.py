"""The linear array and MatMul1D over a hypercube with non-native ("bad") dimensions: generators whose order in
Z_m^* / <p> differs from their order in Z_m^*, the case of m = 21845, p = 2 (signed orders -128, -8) and of the
reference's bootstrapping rings.  helib_amd.bgv_crt.EncryptedArray and helib_amd.bgv_matmul refuse there; the classes
below derive from them and restate the reference's masked paths.

  EncryptedArray.rotate1D   as bgv_crt's (src/EncryptedArray.cpp:99-124), the tail ct*m1 + T - T*m1 through _maskBlend:
                      term by term (multByConstant, +=, multByConstant, -=) or, fused, one capi.maskBlend
                      (hx_mask_blend) per pair of parts with the bookkeeping of the four calls done here;
                      the words and lnNoise / ptxtMag are the same either way.  fused=None follows fuseMaskBlend.
  rotate              src/EncryptedArray.cpp:181-285 in full, the bad-last-dimension branch (:223-264) included
  shift / runningSums / totalSums   helib_amd.bgv.EncryptedArray's bodies (the reference's own, :288-355, 695-736, call
                      only rotate1D, shift1D and rotate, which resolve here)
  MatMul1DExec        a non-native `dim`: two lists of constants (MatMul1DExec_construct, src/matmul.cpp:644-688 with
                      ALT_MATMUL = 1) and MatMul1DExec::mul's non-native branches (:1058-1142, 1253-1285, 1300-1317); a
                      native `dim` is the base class's

Out of scope, refused with a message that says so: MatMulFullExec over a hypercube with a non-native dimension
(src/matmul.cpp:2157-2250; this module's class keeps refusing, the product is helib_amd.matmul_full.MatMulFullExec),
BlockMatMul*, p^r with r > 1 (integer slots mod p^r: helib_amd.bgv_pr, which derives from
the class below).  Nothing here imports oracle/."""
import contextlib
import os
import time

import numpy as np

from . import bgv, bgv_crt, bgv_matmul, capi
from . import ctxt as hc
from . import keys as hk
from . import linalg
from .ckks import LogicError


class EncryptedArray(bgv_crt.EncryptedArray):
    """bgv_crt.EncryptedArray with nothing refused for non-nativeness"""

    fuseMaskBlend = True   # fused=None: hx_mask_blend, the faster form in all three alternated pairs measured

    def _maskBlend(self, ct, T, m1, sz, fused=None):
        """ct = ct*m1 + T - T*m1 (src/EncryptedArray.cpp:120-124).  Fused: one capi.maskBlend per pair of parts, then
        what the four calls do to the bookkeeping -- multByConstant's lnNoise + ln(sz) on ct and on T, the two addCtxt
        steps' noise and ptxtMag sums -- which is all they do when both sides have the same part handles, prime set,
        plaintext space and intFactor.  Otherwise (at p > 2 the two key switches can leave different intFactors, and
        addCtxt then rescales) the four calls run as they are.  T's parts are left alone by the fused form; T is dead in
        every caller."""
        ct._materializeTensor()
        T._materializeTensor()
        has = hasattr(ct.ops, "maskBlend")
        if fused and not has:
            raise LogicError("EncryptedArray: fused=True, but this backend has no maskBlend")
        want = self.fuseMaskBlend if fused is None else fused
        can = (has and list(ct.parts) == list(T.parts) and ct.primeSet == T.primeSet
               and ct.ptxtSpace == T.ptxtSpace and ct.intFactor == T.intFactor)
        if not (want and can):
            ct.multByConstant(m1, sz)
            ct += T
            T.multByConstant(m1, sz)
            ct -= T
            return ct
        hs = list(ct.parts)
        for a in range(0, len(hs), 2):
            h0, h1 = hs[a], hs[a + 1] if a + 1 < len(hs) else None
            ct.ops.maskBlend(ct.parts[h0], ct.parts[h1] if h1 is not None else None,
                             T.parts[h0], T.parts[h1] if h1 is not None else None, m1)
        ct.lnNoise = ct.lnNoise + hc._ln(sz)                     # ct.multByConstant(m1, sz)
        ct.ptxtMag += T.ptxtMag                                  # ct += T
        ct.lnNoise = hc.logaddexp(ct.lnNoise, T.lnNoise)
        T.lnNoise = T.lnNoise + hc._ln(sz)                       # T.multByConstant(m1, sz): the bound alone
        ct.ptxtMag += T.ptxtMag                                  # ct -= T
        ct.lnNoise = hc.logaddexp(ct.lnNoise, T.lnNoise)
        return ct

    def rotate1D(self, ct, i, amt, dc=False, fused=None):
        """bgv_crt.EncryptedArray.rotate1D with the tail of the non-native branch through _maskBlend"""
        if not 0 <= i < self.dimension():
            raise capi.InvalidArgument(capi.HX_ERR_INVALID, "i must be between 0 and dimension()")
        ord_ = self.sizeOfDimension(i)
        amt %= ord_
        if amt == 0:
            return ct
        if dc or self.nativeDimension(i):
            return ct.smartAutomorph(self.zMStar.genToPow(i, amt))
        ct.smartAutomorph(self.zMStar.genToPow(i, amt))          # ct = rho_i^amt(original)
        T = ct.clone()
        T.smartAutomorph(self.zMStar.genToPow(i, -ord_))         # T = rho_i^(amt - ord)(original)
        if not ct.parts:
            return ct
        m1, sz = self._encodedMask(self.maskSlots(i, amt), set(ct.primeSet) | set(T.primeSet))
        return self._maskBlend(ct, T, m1, sz, fused)

    def rotate(self, ct, amt, fused=None):
        """EncryptedArray::rotate (src/EncryptedArray.cpp:181-285): slot j moves to slot j + amt mod nslots"""
        ngens = self.dimension()
        if ngens == 1:                       # simple case: just one generator
            return self.rotate1D(ct, 0, amt, fused=fused)
        amt %= self.size()                   # in [1, nslots - 1]
        if amt == 0:
            return ct
        i = ngens - 1
        v = self.coordinate(i, amt)
        mask = self.maskSlots(i, v)
        if self.nativeDimension(i) or v == 0:
            self.rotate1D(ct, i, v, fused=fused)
        else:
            # a bad last dimension (:223-264): its rotate1D shares the mask of the loop below, which saves a
            # multiplication by a constant -- ct keeps the slots with mask = 1, tmp those with mask = 0
            ord_ = self.sizeOfDimension(i)
            ct.smartAutomorph(self.zMStar.genToPow(i, v))        # ct = rho_i^v(original)
            tmp = ct.clone()
            tmp.smartAutomorph(self.zMStar.genToPow(i, -ord_))   # tmp = rho_i^(v - ord)(original)
            if ct.parts:
                if ct.primeSet == tmp.primeSet:                  # m1 is then the mask on tmp's own primes
                    m1, sz = self._encodedMask(mask, ct.primeSet)
                    ct.multByConstant(m1, sz)
                    self._maskSplit(tmp, mask, fused)            # tmp1 = tmp * m1; tmp -= tmp1
                else:
                    m1, sz = self._encodedMask(mask, set(ct.primeSet) | set(tmp.primeSet))
                    ct.multByConstant(m1, sz)
                    tmp1 = tmp.clone()
                    tmp1.multByConstant(m1, sz)
                    tmp -= tmp1
            # the next generator's rotation before the two are combined
            i -= 1
            v = self.coordinate(i, amt)
            self.rotate1D(ct, i, v, fused=fused)
            self.rotate1D(tmp, i, v + 1, fused=fused)
            ct += tmp
            if i <= 0:
                return ct                    # no more generators
            mask = self._nextMask(mask, i, v)
        for i in range(i - 1, -1, -1):
            v = self.coordinate(i, amt)
            tmp = self._maskSplit(ct, mask, fused)      # tmp: the slots in which mask = 1; ct: those with mask = 0
            self.rotate1D(tmp, i, v, fused=fused)
            self.rotate1D(ct, i, v + 1, fused=fused)
            ct += tmp
            if i > 0:
                mask = self._nextMask(mask, i, v)
        return ct

    @contextlib.contextmanager
    def _blending(self, fused):
        """bgv.EncryptedArray's bodies call rotate1D(ct, i, v) without `fused`: that call then follows this choice"""
        if fused is None:
            yield
            return
        had, old = "fuseMaskBlend" in self.__dict__, self.__dict__.get("fuseMaskBlend")
        self.fuseMaskBlend = bool(fused)
        try:
            yield
        finally:
            if had:
                self.fuseMaskBlend = old
            else:
                del self.fuseMaskBlend

    # bgv_crt's overrides of these refuse a non-native dimension and stay as they are: the bodies are bgv's
    def shift(self, ct, k, fused=None):
        with self._blending(fused):
            return bgv.EncryptedArray.shift(self, ct, k, fused)

    def runningSums(self, ct, fused=None):
        with self._blending(fused):
            return bgv.EncryptedArray.runningSums(self, ct, fused)

    def totalSums(self, ct, fused=None):
        with self._blending(fused):
            return bgv.EncryptedArray.totalSums(self, ct, fused)

    # ---- plaintext automorphisms on integer slots ----
    def _cosets(self):
        """element of Z_m^* -> the slot whose representative lies in its coset of <p>"""
        idx = self.__dict__.get("_coset")
        if idx is None:
            m, p = self.m, self.p % self.m
            idx = self._coset = {}
            for j, t in enumerate(self.zMStar.reps()):
                for _ in range(self.zMStar.ordP):
                    idx[t] = j
                    t = t * p % m
        return idx

    def slotPermutation(self, k):
        """The automorphism X -> X^k of the plaintext ring on integer slots: the encoding of a becomes the encoding of
        a[perm].  Slot j reads the encoded polynomial at rho^(1/t_j); after the automorphism that is its value at
        rho^(k/t_j), a root of the factor of the slot whose representative is t_j / k up to a power of p, and an integer
        mod p is fixed by the Frobenius.  Along a non-native dimension this need not be a roll: g^ord lies in <p> times
        the group of the earlier generators, so what leaves at one end may arrive in another row of the hypercube."""
        m = self.m
        kinv = pow(k, -1, m)
        cos = self._cosets()
        return np.array([cos[t * kinv % m] for t in self.zMStar.reps()], dtype=np.int64)


class MatMul1DExec(bgv_matmul.MatMul1DExec):
    """multiplier[i] / multiplier1[i]: None, or (DoubleCRT of batch 1, size), for the part of diagonal i at coordinates
    >= i / < i of a non-native dimension (vec / vec1 of MatMul1DExec_construct)"""

    def __init__(self, ea, mat, minimal=False, dim=None, device_diagonals=None):
        bgv_matmul._modPOnly(ea, "MatMul1DExec")
        if not isinstance(mat, (bgv_matmul.MatMul1D, bgv_matmul._FullHelper)):
            if dim is None:
                raise LogicError("MatMul1DExec: a bare matrix needs its dimension (or pass a MatMul1D)")
            mat = bgv_matmul.MatMul1D(ea, mat, dim)
        dim = mat.getDim()
        if not 0 <= dim < ea.dimension():
            raise LogicError("Matrix dimension not in [0, ea.dimension())")
        self.native = ea.nativeDimension(dim)
        if self.native:
            super().__init__(ea, mat, minimal, device_diagonals=device_diagonals)
            return
        if not hasattr(ea, "slotPermutation"):
            raise LogicError("MatMul1DExec: a non-native dimension takes helib_amd.bgv_hypercube.EncryptedArray")
        self.ea, self.mat, self.minimal, self.dim = ea, mat, minimal, dim
        self.D = D = ea.sizeOfDimension(dim)
        bsgs = D > hk.HELIB_KEYSWITCH_THRESH or (minimal and D > hk.HELIB_KEYSWITCH_MIN_THRESH)
        self.g = g = hk.KSGiantStepSize(D) if bsgs else 0
        self.times = {"construct": 0.0, "baby": 0.0, "muladd": 0.0, "giant": 0.0}
        self.sync = None
        self.fused = os.environ.get("HX_MATMUL_TERMWISE", "0") in ("", "0")
        self.onDevice = False            # the diagonals are split by the mask and permuted on the host
        t0 = time.perf_counter()
        z = ea.zMStar
        # src/matmul.cpp:644-688: poly1 = diag * maskTable[dim][i], poly2 = diag - poly1 (products mod Phi_m are
        # slot-wise); vec[i] = poly1 moved by rho^(-g k), vec1[i] = poly2 moved by rho^(DD - g k), k = i / g (g = 0:
        # no move and DD = D), each move the plaintext automorphism X -> X^(gen^amt)
        self.multiplier, self.multiplier1 = [None] * D, [None] * D
        vecs, where = [], []
        for i in range(D):
            diag = mat.slots(mat.offsets(i)) % ea.p
            if not np.any(diag):                                  # IsZero(poly): neither list gets a multiplier
                continue
            poly1 = diag * ea.maskSlots(dim, i)
            poly2 = diag - poly1
            k = i // g if g else 1
            for lst, v, amt in ((self.multiplier, poly1, -g * k), (self.multiplier1, poly2, (0 if g else D) - g * k)):
                if np.any(v):                                     # build_ConstMultiplier: nothing for a zero polynomial
                    vecs.append(v[ea.slotPermutation(z.genToPow(dim, amt))] if amt else v)
                    where.append((lst, i))
        # baby steps that were hoisted stay on the ctxt and special primes: the constants live on both
        cc = ea.cc
        idx = list(cc.ctxtPrimes) + list(cc.specialPrimes)
        enc = ea.enc
        step = max(1, int(getattr(enc, "max_batch", 1)))
        split = getattr(enc, "split", lambda poly: [poly])
        for lo in range(0, len(vecs), step):
            poly, cf = enc.encode(np.stack(vecs[lo:lo + step]), 1, idx, coeffs=True)
            sizes = enc.norm(cf)
            for (lst, i), d, sz in zip(where[lo:lo + step], split(poly), sizes):
                lst[i] = (d, float(sz))
        self._tick("construct", t0)

    def _steps(self, ct, n, strategy):
        """GenBabySteps(v, ctxt, dim, clean = false) (src/matmul.cpp:926-969) for j < n"""
        z = self.ea.zMStar
        if n == 1:
            return [ct.clone()]
        if strategy != hk.HELIB_KSS_UNKNOWN:
            precon = hc.BasicAutomorphPrecon(ct)
            return [precon.automorph(z.genToPow(self.dim, j)) for j in range(n)]
        ct0 = linalg._cleanUp(ct.clone())
        out = []
        for j in range(n):
            out.append(ct0.clone())
            if j:
                out[j].smartAutomorph(z.genToPow(self.dim, j))
        return out

    def _chain(self, start, n):
        """start, then each step the one before moved by gen^1 and cleaned up"""
        out, cur = [start], start
        for _ in range(1, n):
            cur = cur.clone()
            cur.smartAutomorph(self.ea.zMStar.genToPow(self.dim, 1))
            linalg._cleanUp(cur)
            out.append(cur)
        return out

    def mul(self, ct, pk=None, strategy=None, fused=None):
        """MatMul1DExec::mul; a non-native dimension takes the branches of src/matmul.cpp:1058-1142 (g != 0) and
        :1253-1285, 1300-1317 (g = 0)"""
        if self.native:
            return super().mul(ct, pk=pk, strategy=strategy, fused=fused)
        fused = self.fused if fused is None else fused
        if strategy is None:
            strategy = hk.getKSStrategy(pk, self.dim) if pk is not None else hk.HELIB_KSS_UNKNOWN
        z, D, g, M, M1, dim = self.ea.zMStar, self.D, self.g, self.multiplier, self.multiplier1, self.dim
        linalg._cleanUp(ct)
        iterative = strategy == hk.HELIB_KSS_MIN

        def pairs(lo, hi, a, b):
            """MulAdd(x, vec[i], a[..]); MulAdd(x, vec1[i], b[..]) for i in [lo, hi), in that order"""
            out = []
            for i in range(lo, hi):
                out += [(M[i], a[i - lo]), (M1[i], b[i - lo])]
            return out
        if g != 0:
            h = -(-D // g)
            t0 = time.perf_counter()
            ct1 = ct.clone()
            ct1.smartAutomorph(z.genToPow(dim, -D))
            if iterative:
                baby, baby1 = self._chain(ct.clone(), g), self._chain(ct1, g)
            else:
                baby, baby1 = self._steps(ct, g, strategy), self._steps(ct1, g, strategy)
            self._tick("baby", t0)
            acc = linalg._empty(ct)
            if iterative:
                for k in range(h - 1, -1, -1):
                    if k < h - 1 and acc.parts:
                        t0 = time.perf_counter()
                        acc.smartAutomorph(z.genToPow(dim, g))
                        linalg._cleanUp(acc)
                        self._tick("giant", t0)
                    self._group(acc, pairs(g * k, min(g * k + g, D), baby, baby1), fused)
            else:
                for k in range(h):
                    inner = linalg._empty(ct)
                    self._group(inner, pairs(g * k, min(g * k + g, D), baby, baby1), fused)
                    if not inner.parts:
                        continue
                    t0 = time.perf_counter()
                    if k > 0:
                        inner.smartAutomorph(z.genToPow(dim, g * k))
                    acc += inner
                    self._tick("giant", t0)
        else:
            t0 = time.perf_counter()
            live = [i for i in range(D) if M[i] is not None or M1[i] is not None]
            if iterative:
                rot = dict(enumerate(self._chain(ct.clone(), live[-1] + 1))) if live else {}
            else:
                precon = bgv_matmul._generalAutomorphPrecon(self.ea, ct, dim, strategy)
                rot = {i: precon(i) for i in live}
            self._tick("baby", t0)
            acc, acc1 = linalg._empty(ct), linalg._empty(ct)
            self._group(acc, [(M[i], rot[i]) for i in live], fused)
            self._group(acc1, [(M1[i], rot[i]) for i in live], fused)
            t0 = time.perf_counter()
            if acc1.parts:
                acc1.smartAutomorph(z.genToPow(dim, -D))
            acc += acc1
            self._tick("giant", t0)
        ct.__dict__.update(acc.__dict__)
        return ct


class MatMulFullExec(bgv_matmul.MatMulFullExec):
    """bgv_matmul.MatMulFullExec; a hypercube with a non-native dimension is refused: the reference's recursion through
    the masked rotations (src/matmul.cpp:2157-2250) is not built here -- helib_amd.matmul_full.MatMulFullExec has it"""

    def __init__(self, ea, mat, minimal=False, device_diagonals=None):
        bgv_matmul._modPOnly(ea, "MatMulFullExec")
        if not all(ea.nativeDimension(i) for i in range(ea.dimension())):
            raise LogicError("MatMulFullExec over a hypercube with a non-native dimension is out of scope "
                             "(src/matmul.cpp:2157-2250 is not built); MatMul1DExec works along one dimension")
        super().__init__(ea, mat, minimal, device_diagonals=device_diagonals)
