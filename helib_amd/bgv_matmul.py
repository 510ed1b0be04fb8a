"""MatMul1D / MatMul1DExec and MatMulFull / MatMulFullExec (src/matmul.cpp) for BGV over helib_amd.bgv.EncryptedArray
(d = 1, every dimension native): a plaintext matrix times the slot vector of a (batched) ciphertext,

  MatMulFull   w[j] = sum_i A[i, j] * v[i] mod p, i.e. (v @ A) % p            (src/matmul.cpp:2766-2806)
  MatMul1D     the same along one dimension of the hypercube, independently for every setting of the other
               coordinates                                                     (:2620-2672)

mul is the CKKS class's (helib_amd.linalg.MatMul1DExec.mul: MatMul1DExec::mul, native branches, :973-1110, 1226-1252,
1286-1299) along the matrix's own dimension, with Ctxt.multByConstant(DoubleCRT, size) as the multiply: the inner loop
runs through hx_mul_add_many under the same shadow-bookkeeping rule, and counts in MatMul1DExec.fallbacks when it
cannot.

Constants.  Diagonal i of the product along dimension `dim` is a slot vector; it is rotated by -g * floor(i / g) along
`dim` (build_ConstMultiplier, :375-389) and kept as ConstMultiplier_DoubleCRT (:329-364): the DoubleCRT of its balanced
zzX and embeddingLargestCoeff of that zzX -- the words and the size multByConstant(zzX) would build on the fly.  One
descriptor (off, rot_dim, rot_amt) names a diagonal for both shapes of matrix (diagonalSlots below is the formula):

  device path   the dense matrix goes to the device once (DeviceEncoder.matrix), the descriptors go in chunks, the
                diagonals are gathered there (hx_bgv_encode_diagonals) and split into constants with hx_poly_extract
  host path     numpy gathers each diagonal, ea.enc.encode encodes it: a callable matrix, an encoder without
                encodeDiagonals, or device_diagonals=False

Both give the same words and sizes.  Out of scope: BlockMatMul*, multipleTransforms, non-native dimensions, d > 1.
Nothing here imports oracle/."""
import os
import time

import numpy as np

from . import ctxt as hc
from . import keys as hk
from . import linalg
from .ckks import LogicError


def strides(ords):
    """slot = sum_i coordinate_i * stride_i, the last dimension fastest (PAlgebra::coordinate)"""
    s = [1] * len(ords)
    for i in range(len(ords) - 2, -1, -1):
        s[i] = s[i + 1] * ords[i + 1]
    return s


def diagonalSlots(ea, a, dim, off, rot_dim=-1, rot_amt=0):
    """The slot vector of one diagonal of the dense matrix a (hx_bgv_diag in numpy).  Slot s has coordinates c; s0 is s
    with c[rot_dim] replaced by c[rot_dim] - rot_amt (plaintextAutomorph at d = 1).  dim = -1, a full matrix by slot:
    a[r, s0] with r the slot of coordinates c_i(s0) - off[i]; dim = i, a D x D matrix by the coordinate in dimension i:
    a[c_i(s0) - off[i], c_i(s0)].  Every difference is taken modulo the order of its dimension."""
    ords = ea.zMStar.ords
    st = strides(ords)
    s = np.arange(ea.size(), dtype=np.int64)
    c = [s // st[i] % ords[i] for i in range(len(ords))]
    if rot_dim >= 0:
        c[rot_dim] = (c[rot_dim] - rot_amt) % ords[rot_dim]
    if dim >= 0:
        return a[(c[dim] - off[dim]) % ords[dim], c[dim]] % ea.p
    s0 = sum(c[i] * st[i] for i in range(len(ords)))
    r = sum((c[i] - off[i]) % ords[i] * st[i] for i in range(len(ords)))
    return a[r, s0] % ea.p


def _modPOnly(ea, what):
    """the matrix products are built for slots mod p: over helib_amd.bgv_pr.EncryptedArray at r > 1 the diagonals
    would have to be reduced, gathered and encoded mod p^r"""
    if getattr(ea, "r", 1) != 1:
        raise LogicError("%s over slots mod p^r with r > 1 (helib_amd.bgv_pr) is not built" % what)


class _Matrix:
    """a plaintext matrix of one of the two shapes: dense integers, or a callable get(i, j) read out once"""

    def __init__(self, ea, mat, dim, side):
        _modPOnly(ea, type(self).__name__)
        self.ea, self.dim = ea, dim
        self.callable = callable(mat)
        if self.callable:
            self.get = mat
            mat = [[int(mat(i, j)) % ea.p for j in range(side)] for i in range(side)]
        a = np.asarray(mat)
        if a.dtype == object or a.dtype.kind not in "iu" or a.dtype == np.uint64:
            a = np.array([int(x) % ea.p for x in a.reshape(-1)], dtype=np.int64).reshape(a.shape)
        self.dense = np.ascontiguousarray(a, dtype=np.int64)
        if self.dense.shape != (side, side):
            raise LogicError("matrix of shape %s where %d x %d is taken" % (self.dense.shape, side, side))
        if not self.callable:
            self.get = lambda i, j: int(self.dense[i, j])
        self._handle = None

    def handle(self, enc):
        """the matrix on the device: uploaded once, shared by every MatMul1DExec built from it"""
        if self._handle is None:
            self._handle = enc.matrix(self.dense, self.dim)
        return self._handle

    def slots(self, off, rot_dim=-1, rot_amt=0):
        return diagonalSlots(self.ea, self.dense, self.dim, off, rot_dim, rot_amt)


class MatMul1D(_Matrix):
    """MatMul1D_derived (include/helib/matmul.h): a D x D matrix for dimension `dim` of the hypercube, D =
    ea.sizeOfDimension(dim), as a dense integer array or a callable get(i, j)"""

    def __init__(self, ea, mat, dim):
        if not 0 <= dim < ea.dimension():
            raise LogicError("Matrix dimension not in [0, ea.dimension())")
        super().__init__(ea, mat, dim, ea.sizeOfDimension(dim))

    def getDim(self):
        return self.dim

    def offsets(self, i):
        off = [0] * self.ea.dimension()
        off[self.dim] = i
        return off

    def processDiagonal(self, i):
        """MatMul1D_derived_impl::processDiagonal1 (src/matmul.cpp:449-504): diag[j] = get((c - i) mod D, c), c the
        coordinate of slot j in the matrix's dimension; as slots mod p"""
        return self.slots(self.offsets(i))


class MatMulFull(_Matrix):
    """MatMulFull_derived: a phi(m) x phi(m) matrix indexed by slot"""

    def __init__(self, ea, mat):
        super().__init__(ea, mat, -1, ea.size())


class _FullHelper:
    """MatMulFullHelper (src/matmul.cpp:1980-2028): the 1D view of a full matrix along `dim` once the index vector has
    been rotated by off[i] along every earlier dimension i (rec_mul, :2060-2072)"""

    def __init__(self, full, off, dim):
        self.ea, self.full, self.off, self.dim = full.ea, full, list(off), dim
        self.callable = full.callable

    def getDim(self):
        return self.dim

    def handle(self, enc):
        return self.full.handle(enc)

    def offsets(self, i):
        off = list(self.off)
        off[self.dim] = i
        return off

    def slots(self, off, rot_dim=-1, rot_amt=0):
        return self.full.slots(off, rot_dim, rot_amt)

    def processDiagonal(self, i):
        """MatMulFullHelper::processDiagonal (:1998-2024): pmat[j] = get(idxes[j], j), idxes the accumulated rotate1D
        of the identity"""
        return self.slots(self.offsets(i))


class MatMul1DExec(linalg.MatMul1DExec):
    """multiplier[i] is None for a zero diagonal, else (DoubleCRT of batch 1, size)"""

    deviceDiagonals = True     # device_diagonals=None: gather the diagonals on the device when the encoder can
    FLAG_CHUNK = 4096          # descriptors per flags-only call (40 B each; no scratch rows)

    def __init__(self, ea, mat, minimal=False, dim=None, device_diagonals=None):
        _modPOnly(ea, "MatMul1DExec")
        if not isinstance(mat, (MatMul1D, _FullHelper)):
            if dim is None:
                raise LogicError("MatMul1DExec: a bare matrix needs its dimension (or pass a MatMul1D)")
            mat = MatMul1D(ea, mat, dim)
        self.ea, self.mat, self.minimal = ea, mat, minimal
        self.dim = dim = mat.getDim()
        if not 0 <= dim < ea.dimension():
            raise LogicError("Matrix dimension not in [0, ea.dimension())")
        if not ea.nativeDimension(dim):
            raise LogicError("MatMul1DExec: a non-native dimension at d = 1")
        self.D = D = ea.sizeOfDimension(dim)
        # src/matmul.cpp:866-872
        bsgs = D > hk.HELIB_KEYSWITCH_THRESH or (minimal and D > hk.HELIB_KEYSWITCH_MIN_THRESH)
        self.g = g = hk.KSGiantStepSize(D) if bsgs else 0
        self.times = {"construct": 0.0, "baby": 0.0, "muladd": 0.0, "giant": 0.0}
        self.sync = None
        self.fused = os.environ.get("HX_MATMUL_TERMWISE", "0") in ("", "0")
        t0 = time.perf_counter()
        # MatMul1DExec_construct, native branch (:626-643): diagonal i rotated by -g * floor(i / g) (0 when g = 0)
        self.rotation = [(-g * (i // g)) if g else 0 for i in range(D)]
        self.multiplier = [None] * D
        # hoisted rotations (the g = 0 form) stay on the ctxt and special primes: their constants must too
        cc = ea.cc
        idx = list(cc.ctxtPrimes) + (list(cc.specialPrimes) if g == 0 else [])
        enc = ea.enc
        want = self.deviceDiagonals if device_diagonals is None else device_diagonals
        self.onDevice = bool(want and not mat.callable and hasattr(enc, "encodeDiagonals"))
        step = max(1, int(getattr(enc, "max_batch", 1)))
        split = getattr(enc, "split", lambda poly: [poly])
        descs = [(mat.offsets(i), dim, self.rotation[i]) for i in range(D)]
        if self.onDevice:
            a = mat.handle(enc)
            live = []
            for lo in range(0, D, self.FLAG_CHUNK):
                nz = enc.encodeDiagonals(a, descs[lo:lo + self.FLAG_CHUNK])[2]
                live += [lo + int(k) for k in np.nonzero(nz)[0]]
            for lo in range(0, len(live), step):
                where = live[lo:lo + step]
                poly, cf, _ = enc.encodeDiagonals(a, [descs[i] for i in where], idx, coeffs=True)
                sizes = enc.norm(cf)
                for i, d, sz in zip(where, split(poly), sizes):
                    self.multiplier[i] = (d, float(sz))
        else:
            vecs, live = [], []
            for i in range(D):
                v = mat.slots(*descs[i])
                if np.any(v):                             # IsZero(poly): no multiplier (:369-372); a rotation keeps it
                    vecs.append(v)
                    live.append(i)
            for lo in range(0, len(live), step):
                poly, cf = enc.encode(np.stack(vecs[lo:lo + step]), 1, idx, coeffs=True)
                sizes = enc.norm(cf)
                for i, d, sz in zip(live[lo:lo + step], split(poly), sizes):
                    self.multiplier[i] = (d, float(sz))
        self._tick("construct", t0)

    @staticmethod
    def _mulAdd(x, a, b):
        """MulAdd (src/matmul.cpp:391-399) with ConstMultiplier_DoubleCRT::mul (:338)"""
        tmp = b.clone()
        tmp.multByConstant(*a)
        x += tmp


def _generalAutomorphPrecon(ea, ct, dim, strategy):
    """buildGeneralAutomorphPrecon (src/matmul.cpp:186-312) -> i |-> the ciphertext rotated by i along dim"""
    z = ea.zMStar
    if strategy == hk.HELIB_KSS_FULL:
        precon = hc.BasicAutomorphPrecon(ct)
        return lambda i: precon.automorph(z.genToPow(dim, i))
    if strategy == hk.HELIB_KSS_BSGS:
        g = hk.KSGiantStepSize(z.ordP if dim == -1 else z.OrderOf(dim))     # dim = -1: the Frobenius (:211)
        p0, pre = hc.BasicAutomorphPrecon(ct), {}

        def bsgs(i):
            k = i // g
            if k not in pre:
                pre[k] = hc.BasicAutomorphPrecon(p0.automorph(z.genToPow(dim, g * k)))
            return pre[k].automorph(z.genToPow(dim, i % g))
        return bsgs
    ct0 = linalg._cleanUp(ct.clone())

    def plain(i):
        r = ct0.clone()
        if i:
            r.smartAutomorph(z.genToPow(dim, i))
        return r
    return plain


class MatMulFullExec:
    """MatMulFullExec (src/matmul.cpp:2030-2273): one MatMul1DExec along the last dimension of `dims` per setting of
    the offsets in the dimensions before it"""

    exec1D = MatMul1DExec      # the product along the last dimension (helib_amd.matmul_full: one that takes a non-native one)

    def __init__(self, ea, mat, minimal=False, device_diagonals=None):
        _modPOnly(ea, "MatMulFullExec")
        mat = mat if isinstance(mat, MatMulFull) else MatMulFull(ea, mat)
        self.ea, self.mat, self.minimal = ea, mat, minimal
        nd = ea.dimension()
        if ea.size() < 2 or nd < 1:
            raise LogicError("Number of slots is less than 2")
        # MatMulDimComp (:2084-2098): small dimensions first, native before non-native among equals
        self.dims = sorted(range(nd), key=lambda i: (ea.sizeOfDimension(i), not ea.nativeDimension(i)))
        self.transforms = []

        def rec(d, off):
            if d >= nd - 1:
                self.transforms.append(self.exec1D(ea, _FullHelper(mat, off, self.dims[d]), minimal,
                                                   device_diagonals=device_diagonals))
                return
            for o in range(ea.sizeOfDimension(self.dims[d])):
                off1 = list(off)
                off1[self.dims[d]] = o
                rec(d + 1, off1)
        rec(0, [0] * nd)

    def _rec_mul(self, acc, ct, d, idx, pk, fused):
        ea = self.ea
        if d >= ea.dimension() - 1:
            tmp = ct.clone()
            self.transforms[idx].mul(tmp, pk=pk, fused=fused)
            acc += tmp
            return idx + 1
        dim = self.dims[d]
        sdim = ea.sizeOfDimension(dim)
        if not ea.nativeDimension(dim):
            raise LogicError("MatMulFullExec: a non-native dimension at d = 1")
        strategy = hk.getKSStrategy(pk, dim) if pk is not None else hk.HELIB_KSS_UNKNOWN
        if strategy != hk.HELIB_KSS_MIN:
            precon = _generalAutomorphPrecon(ea, ct, dim, strategy)
            for i in range(sdim):
                idx = self._rec_mul(acc, precon(i), d + 1, idx, pk, fused)
        else:
            sh = ct.clone()
            for offset in range(sdim):
                if offset > 0:
                    sh.smartAutomorph(ea.zMStar.genToPow(dim, 1))
                idx = self._rec_mul(acc, sh, d + 1, idx, pk, fused)
        return idx

    def mul(self, ct, pk=None, fused=None):
        """MatMulFullExec::mul (:2254-2273); the strategies are read from the key `pk` per dimension"""
        if self.ea.size() < 2:
            raise LogicError("Number of slots is less than 2")
        linalg._cleanUp(ct)
        acc = linalg._empty(ct)
        self._rec_mul(acc, ct, 0, 0, pk, fused)
        ct.__dict__.update(acc.__dict__)
        return ct


# ---- plaintext truth ----
def mulPlain(ea, v, mat):
    """mul(PlaintextArray, MatMul1D / MatMulFull) (src/matmul.cpp:2620-2672, 2766-2806) on slots v[B, phi(m)]"""
    v = np.atleast_2d(np.asarray(v, dtype=np.int64)) % ea.p
    a = mat.dense % ea.p
    if ea.p * ea.p * a.shape[0] >= 2 ** 63:      # the sums would leave int64
        v, a = v.astype(object), a.astype(object)
    if mat.dim < 0:
        return np.array(v @ a % ea.p, dtype=np.int64)
    ords = ea.zMStar.ords
    x = np.moveaxis(v.reshape([v.shape[0]] + list(ords)), 1 + mat.dim, -1)
    w = np.moveaxis(x @ a % ea.p, -1, 1 + mat.dim)
    return np.array(w.reshape(v.shape), dtype=np.int64)
