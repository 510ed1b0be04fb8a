"""MatMulFullExec over a hypercube with non-native ("bad") dimensions: an encrypted slot vector times a plaintext matrix
over all slots, (v @ A) % p, on rings such as m = 21845, p = 2 (signed orders -128, -8) where
helib_amd.bgv_matmul.MatMulFullExec and helib_amd.bgv_hypercube.MatMulFullExec refuse.

  construction   bgv_matmul.MatMulFullExec's (MatMulDimComp, src/matmul.cpp:2084-2098, and rec_mul, :2035-2075) with
                 helib_amd.bgv_hypercube.MatMul1DExec along the last dimension, native or not
  _rec_mul       the native branches are the base class's; a non-native dimension before the last takes the reference's
                 recursion through masked rotations (:2174-2204, and :2216-2246 under HELIB_KSS_MIN): with ct1 = ct moved
                 by g^(-ord), offset i > 0 recurses on rho^i(ct) m + rho^i(ct1) - rho^i(ct1) m, m = maskTable[dim][i]

The strategy of a dimension is read from the key as the base class reads it (keys.getKSStrategy): add1DMatrices, and
addSome1DMatrices for an order up to its bound, give HELIB_KSS_FULL -- a matrix for every power of the generator --,
addBSGS1DMatrices HELIB_KSS_BSGS, addMinimal1DMatrices HELIB_KSS_MIN, no key HELIB_KSS_UNKNOWN.  Under HELIB_KSS_FULL both
rotations of every offset come from two digit decompositions (BasicAutomorphPrecon of ct and of ct1), and the blend of
up to CHUNK offsets is one device call where ctxt.automorphBlend's fused form applies (hx_hoisted_blend).

`fused` in mul: False, every step term by term (the blend as multByConstant, +=, multByConstant, -=); None, the classes'
switches (EncryptedArray.fuseMaskBlend for the blend alone, Ctxt.fuseHoistedBlend for the hoisted blend); True, the
hoisted blend wherever it applies, hx_mask_blend elsewhere.  It reaches the products along the last dimension unchanged.

Out of scope, refused or left to the classes that refuse: matrices with GF(p^d) or Galois-ring entries, BlockMatMulFull*,
p^r with r > 1, CKKS.  Nothing here imports oracle/."""
from . import bgv_hypercube, bgv_matmul
from . import ctxt as hc
from . import keys as hk


class MatMulFullExec(bgv_matmul.MatMulFullExec):
    """bgv_matmul.MatMulFullExec with nothing refused for non-nativeness"""

    exec1D = bgv_hypercube.MatMul1DExec
    CHUNK = 8          # offsets blended by one automorphBlend: bounds the outputs held at once

    def _blend(self, tmp, tmp1, dim, i, fused):
        """tmp = tmp*m1 + tmp1 - tmp1*m1 with m1 the mask of (dim, i) on the union of the prime sets (:2189-2200)"""
        if not tmp.parts:
            return tmp
        ea = self.ea
        m1, sz = ea._encodedMask(ea.maskSlots(dim, i), set(tmp.primeSet) | set(tmp1.primeSet))
        return ea._maskBlend(tmp, tmp1, m1, sz, fused)

    def _rec_mul(self, acc, ct, d, idx, pk, fused):
        ea = self.ea
        if d >= ea.dimension() - 1 or ea.nativeDimension(self.dims[d]):
            return super()._rec_mul(acc, ct, d, idx, pk, fused)
        dim = self.dims[d]
        sdim, z = ea.sizeOfDimension(dim), ea.zMStar
        strategy = hk.getKSStrategy(pk, dim) if pk is not None else hk.HELIB_KSS_UNKNOWN
        ct1 = ct.clone()
        ct1.smartAutomorph(z.genToPow(dim, -sdim))
        idx = self._rec_mul(acc, ct, d + 1, idx, pk, fused)                    # offset 0: ct itself
        if strategy == hk.HELIB_KSS_MIN:                                       # iterative (:2216-2246)
            sh, sh1 = ct.clone(), ct1
            for i in range(1, sdim):
                sh.smartAutomorph(z.genToPow(dim, 1))
                sh1.smartAutomorph(z.genToPow(dim, 1))
                idx = self._rec_mul(acc, self._blend(sh.clone(), sh1.clone(), dim, i, fused), d + 1, idx, pk, fused)
            return idx
        if strategy == hk.HELIB_KSS_FULL and ct.parts and (hc.Ctxt.fuseHoistedBlend if fused is None else fused):
            pre, pre1 = hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1)
            primes = set(pre.ctxt.primeSet) | set(pre1.ctxt.primeSet) | set(ea.cc.specialPrimes)
            for lo in range(1, sdim, self.CHUNK):
                offs = range(lo, min(lo + self.CHUNK, sdim))
                masks = [ea._encodedMask(ea.maskSlots(dim, i), primes) for i in offs]
                for tmp in hc.automorphBlend(pre, pre1, [z.genToPow(dim, i) for i in offs], [mk for mk, _ in masks],
                                             [sz for _, sz in masks], fused=fused):
                    idx = self._rec_mul(acc, tmp, d + 1, idx, pk, fused)
            return idx
        precon = bgv_matmul._generalAutomorphPrecon(ea, ct, dim, strategy)
        precon1 = bgv_matmul._generalAutomorphPrecon(ea, ct1, dim, strategy)
        for i in range(1, sdim):
            idx = self._rec_mul(acc, self._blend(precon(i), precon1(i), dim, i, fused), d + 1, idx, pk, fused)
        return idx
