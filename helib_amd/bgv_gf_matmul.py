"""Linear maps on slots in GF(p^d) over helib_amd.bgv_gf.EncryptedArray (G = F_0, r = 1, d <= 64, p < 2^31):

  buildLinPolyCoeffs / applyLinPolyLL / applyLinPoly1 / applyLinPolyMany
                      linearized polynomials (src/EncryptedArray.cpp:740-879, src/NumbTh.cpp:1099-1111): a Z_p-linear map
                      of a slot is alpha -> sum_k C[k] alpha^(p^k)
  slotAutomorph / automorphPlain      the plaintext automorphism X -> X^k on GF slots: a permutation of the slots and a
                      power of the Frobenius in every slot
  MatMul1D / MatMul1DExec             a D x D matrix with entries in GF(p^d) along one dimension, native or not
                      (MatMul1D_derived, src/matmul.cpp:449-688); mul is bgv_matmul's / bgv_hypercube's, unchanged
  BlockMatMul1D / BlockMatMul1DExec   a D x D matrix of d x d blocks over Z_p, one or n / D transforms
                      (src/matmul.cpp:1324-1976), the reference's size-1 dimension dim = ea.dimension() included
  mulPlain            the plain-side truth of both (src/matmul.cpp:2620-2672, 2705-2756)

Constants.  Every constant of an exec is "slot s takes Frob^e(value at slot src[s]), or zero": the value is coefficient k
of the linearized polynomial of the block its source slot reads on diagonal i (or the GF entry itself), and (src, e) is a
plaintext automorphism (slotAutomorph) behind a mask.  build_ConstMultiplier(poly, -1, -j), (poly, dim, -i), the masked
halves and (poly1, dim, D) of the reference are all of this form.

  device path   the matrix goes to the device once (capi.BgvGfMatrix: for blocks hx_bgv_gf_matrix_create forms every
                entry's coefficients with one product against the flat table, bgv_gf_linpoly_kernel); the descriptors go
                in chunks through capi.bgvGfGather (bgv_gf_gather_kernel) and ea.enc.encode
  host path     numpy does both, then ea.enc.encode: a callable matrix, an injected encoder, device_diagonals=False

Both give the same words and sizes.  The arithmetic -- the tables, the linearized polynomials, the slot automorphisms,
the plain-side products, one constant on the host -- lives in helib_amd.slot_ring, which reads the modulus from the
array (ea.P); the functions here are this module's check of the array in front of it.  What is this module's own is the
matrices, the constants of an exec (_Maps, _constants) and the execs; helib_amd.bgv_gr_matmul subclasses them over
helib_amd.bgv_gr.EncryptedArray.  Refused with a message: BlockMatMulFull*, MatMulFull with GF entries,
multipleTransforms for the GF-entry MatMul1D, r > 1 (bgv_gf.EncryptedArray refuses it).  Nothing here imports oracle/."""
import os
import time

import numpy as np

from . import bgv_gf, bgv_hypercube, bgv_matmul, capi, slot_ring
from . import keys as hk
from . import linalg
from .ckks import LogicError

GATHER_CHUNK = 64      # descriptors per gather call: 64 n d words of scratch


def _check(ea):
    if getattr(ea, "r", 1) != 1:
        raise LogicError("linear maps on GF(p^d) slots at p^r with r > 1 (helib_amd.bgv_pr holds integers) are not built")
    if not isinstance(ea, bgv_gf.EncryptedArray):
        raise LogicError("linear maps on GF(p^d) slots take helib_amd.bgv_gf.EncryptedArray")


def linPolyMatrix(ea):
    """(M, K) as int64 [d, d, d]: M[i][j] = (X^j)^(p^i) mod G and its inverse over GF(p^d)"""
    _check(ea)
    t = slot_ring._tables(ea)
    return t.frob.copy(), t.K.copy()


def linPolyTable(ea):
    """the flat d^2 x d^2 table over Z_p with C = E T"""
    _check(ea)
    return slot_ring._tables(ea).flat()


def buildLinPolyCoeffs(ea, L):
    """EncryptedArrayDerived::buildLinPolyCoeffs: L [..., d, d], row j the coefficients of the image of X^j -> C
    [..., d, d], row k the coefficients of C[k] = sum_j L[j] K[j][k]; the map is alpha -> sum_k C[k] alpha^(p^k)"""
    _check(ea)
    return slot_ring.buildLinPolyCoeffs(ea, L)


def linPolyFlat(ea, E):
    """buildLinPolyCoeffs through the flat table: what the device computes"""
    _check(ea)
    return slot_ring.linPolyFlat(ea, E)


def evalLinPoly(ea, C, a):
    """sum_k C[k] alpha^(p^k) slot by slot: C [d, d] (one map) or [nslots, d, d], a slots -> [B, nslots, d]"""
    _check(ea)
    return slot_ring.evalLinPoly(ea, C, a)


# ---- plaintext automorphisms ----
def slotAutomorph(ea, k):
    """X -> X^k on GF slots -> (perm, frob): the new slot j is Frob^frob[j] of the old slot perm[j]
    (slot_ring.slotAutomorph has the derivation)"""
    _check(ea)
    return slot_ring.slotAutomorph(ea, k)


def automorphPlain(ea, a, k):
    """the slots of the plaintext with X -> X^k applied -> int64 [B, nslots, d]"""
    _check(ea)
    return slot_ring.automorphPlain(ea, a, k)


# ---- the matrices ----
def _geometry(ea, dim):
    """(D, blk [n], col [n]): PAlgebra::breakIndexByDim of every slot; dim = ea.dimension() is the size-1 dimension"""
    n = ea.size()
    s = np.arange(n, dtype=np.int64)
    if dim == ea.dimension():
        return 1, s, np.zeros(n, dtype=np.int64)
    D = ea.sizeOfDimension(dim)
    st = bgv_matmul.strides(ea.zMStar.ords)[dim]
    return D, s % st + s // (st * D) * st, s % (st * D) // st


def _ints(a, P):
    """any integers -> contiguous int64 in [0, P)"""
    a = np.asarray(a)
    if a.dtype == object or a.dtype.kind not in "iu" or a.dtype == np.uint64:
        a = np.array([int(x) % P for x in a.reshape(-1)], dtype=np.int64).reshape(a.shape)
    return np.ascontiguousarray(a.astype(np.int64) % P)


class _GfMatrix:
    block = False
    ring = False               # the device matrix is built over a table of any r (capi.BgvGfMatrix(ring=True))

    # what a module over another class of array replaces: its check
    _checkArray = staticmethod(lambda ea: _check(ea))

    def getDim(self):
        return self.dim

    def multipleTransforms(self):
        return self.multiple

    def handle(self, enc):
        """the matrix on the device: uploaded (and, for blocks, turned into coefficients) once"""
        if self._handle is None:
            self._handle = capi.BgvGfMatrix(enc.table, self.dense, self.blk if self.multiple else np.zeros_like(self.blk), self.col,
                                            ring=self.ring)
        return self._handle

    def values(self):
        """[nb, D, D, K, d]: what a slot can hold -- K = d coefficients of every block's linearized polynomial, or K = 1"""
        if self._values is None:
            self._values = (slot_ring.buildLinPolyCoeffs(self.ea, self.dense) if self.block
                            else self.dense[:, :, :, None, :])
        return self._values

    def slotValues(self, i, k):
        """processDiagonal: slot s -> coefficient k of the entry [(c - i) mod D, c] of its transform, [n, d]"""
        b = self.blk if self.multiple else 0
        return self.values()[b, (self.col - i) % self.D, self.col, k]


class MatMul1D(_GfMatrix):
    """MatMul1D_derived with entries in GF(p^d): A [D, D, d], a [D, D] integer matrix (constants), or a callable
    get(i, j) -> d coefficients (or an integer)"""

    def __init__(self, ea, A, dim):
        self._checkArray(ea)
        if not 0 <= dim < ea.dimension():
            raise LogicError("Matrix dimension not in [0, ea.dimension())")
        self.ea, self.dim, self.multiple, d = ea, dim, False, ea.getDegree()
        self.D, self.blk, self.col = _geometry(ea, dim)
        self.callable = callable(A)
        if self.callable:
            rows = [[np.atleast_1d(_ints(A(i, j), ea.P)) for j in range(self.D)] for i in range(self.D)]
            A = [[np.pad(x, (0, d - len(x))) for x in r] for r in rows]
        a = _ints(A, ea.P)
        if a.ndim >= 4:
            raise LogicError("MatMul1D with GF entries: multipleTransforms (%d axes) is not built; BlockMatMul1D takes one "
                             "matrix per transform" % a.ndim)
        if a.ndim == 2:
            a = a[:, :, None]
        if a.ndim != 3 or a.shape[:2] != (self.D, self.D) or a.shape[2] > d:
            raise LogicError("matrix of shape %s where [%d, %d, %d] is taken" % (a.shape, self.D, self.D, d))
        self.dense = np.zeros((1, self.D, self.D, d), dtype=np.int64)
        self.dense[0, :, :, :a.shape[2]] = a
        self._handle = self._values = None


class BlockMatMul1D(_GfMatrix):
    """BlockMatMul1D_derived: A [D, D, d, d] (one transform) or [n / D, D, D, d, d] (multipleTransforms), entry [i, j]
    the d x d matrix over Z_p a slot's coefficient vector is multiplied by (row vector times matrix).  0 <= dim <=
    ea.dimension(); dim = ea.dimension() is a dimension of size 1: D = 1 and one block per slot, [n, 1, 1, d, d]."""
    block = True

    def __init__(self, ea, A, dim):
        self._checkArray(ea)
        if not 0 <= dim <= ea.dimension():
            raise LogicError("Matrix dimension not in [0, ea.dimension()]")
        self.ea, self.dim, d, n = ea, dim, ea.getDegree(), ea.size()
        self.D, self.blk, self.col = _geometry(ea, dim)
        self.callable = callable(A)
        if self.callable:
            raise LogicError("BlockMatMul1D takes a dense array")
        a = _ints(A, ea.P)
        self.multiple = a.ndim == 5
        if dim == ea.dimension() and not self.multiple:
            raise LogicError("BlockMatMul1D along the size-1 dimension takes one block per slot: [%d, 1, 1, %d, %d]" % (n, d, d))
        want = ((n // self.D,) if self.multiple else ()) + (self.D, self.D, d, d)
        if a.shape != want:
            raise LogicError("matrix of shape %s where %s is taken" % (a.shape, want))
        self.dense = a if self.multiple else a[None]
        self._handle = self._values = None


def BlockMatMulFull(*args, **kwargs):
    raise LogicError("BlockMatMulFull / BlockMatMulFullExec are not built: BlockMatMul1DExec works along one dimension")


BlockMatMulFullExec = BlockMatMulFull


def MatMulFull(*args, **kwargs):
    raise LogicError("MatMulFull with GF entries is not built: helib_amd.bgv_matmul.MatMulFull takes integer matrices, "
                     "MatMul1DExec here works along one dimension")


MatMulFullExec = MatMulFull


def mulPlain(ea, v, mat):
    """mul(PlaintextArray, MatMul1D / BlockMatMul1D) on slots v -> int64 [B, nslots, d]: along mat's dimension and for
    every transform k, w[k][j] = sum_i v[k][i] * A_k[i][j] -- the product in Z_p[X] / G for a GF entry, the coefficient
    row vector times the d x d block for a block entry"""
    _check(ea)
    return slot_ring.mulPlain(ea, v, mat)


# ---- the constants of an exec ----
class _Maps:
    """the (source slot, Frobenius exponent) maps of an exec, each kept once: the automorphism X -> X^k behind a mask"""

    def __init__(self, ea):
        self.ea, self.rows, self.index = ea, [], {}

    def add(self, k, mask=None):
        perm, frob = slot_ring.slotAutomorph(self.ea, k)
        src = perm if mask is None else np.where(np.asarray(mask)[perm] != 0, perm, -1)
        row = np.stack([src, np.where(src >= 0, frob, 0)], axis=1).astype(np.int32)
        key = row.tobytes()
        if key not in self.index:
            self.index[key] = len(self.rows)
            self.rows.append(row)
        return self.index[key]


hostConstant = slot_ring.hostConstant


def _constants(ea, mat, reqs, maps, idx, device, fused=False):
    """reqs [(i, k, map)] -> [None for a zero constant | (DoubleCRT of batch 1 on idx, size)].  fused (device only): the
    constants never leave the device -- enc.encodeGathered gives the flags of a chunk, then the live descriptors go
    through it in the encoder's batches: max_batch if the encoder names one, 16 for the device encoders
    (slot_ring.SlotEncoder), else one"""
    enc = ea.enc
    step = max(1, int(getattr(enc, "max_batch", 16 if isinstance(enc, slot_ring.SlotEncoder) else 1)))
    split = getattr(enc, "split", lambda poly: [poly])
    out = [None] * len(reqs)
    table = np.stack(maps.rows) if maps.rows else None
    handle = mat.handle(enc) if device else None
    for lo in range(0, len(reqs), GATHER_CHUNK):
        chunk = reqs[lo:lo + GATHER_CHUNK]
        if device and fused:
            descs = np.array(chunk, dtype=np.int32)
            nz = enc.encodeGathered(handle, descs, table, 1, idx, flags_only=True)
        elif device:
            slots, nz = capi.bgvGfGather(handle, np.array(chunk, dtype=np.int32), table)
        else:
            slots = np.stack([slot_ring.hostConstant(ea, mat, i, k, maps.rows[mp]) for i, k, mp in chunk])
            nz = slots.reshape(len(chunk), -1).any(axis=1)
        live = [int(t) for t in np.nonzero(nz)[0]]
        for a in range(0, len(live), step):
            where = live[a:a + step]
            if device and fused:
                poly, cf, _ = enc.encodeGathered(handle, descs[where], table, 1, idx, coeffs=True)
            else:
                poly, cf = enc.encode(slots[where], 1, idx, coeffs=True)
            for t, dcrt, sz in zip(where, split(poly), enc.norm(cf)):
                out[lo + t] = (dcrt, float(sz))
    return out


def _onDevice(ea, mat, device_diagonals, default):
    want = default if device_diagonals is None else device_diagonals
    return bool(want and not mat.callable and isinstance(getattr(ea.enc, "table", None), capi.BgvGf))


class MatMul1DExec(bgv_hypercube.MatMul1DExec):
    """MatMul1DExec for a matrix with GF entries: the constants of bgv_matmul.MatMul1DExec (native dimension) and of
    bgv_hypercube.MatMul1DExec (non-native: multiplier / multiplier1), with the plaintext automorphisms of GF slots; mul
    is theirs"""

    _Matrix = MatMul1D         # the matrix class a bare array is wrapped in

    def _consts(self, reqs, maps, idx):
        return _constants(self.ea, self.mat, reqs, maps, idx, self.onDevice)

    def __init__(self, ea, mat, minimal=False, dim=None, device_diagonals=None):
        if not isinstance(mat, self._Matrix):
            if dim is None:
                raise LogicError("MatMul1DExec: a bare matrix needs its dimension (or pass a MatMul1D)")
            mat = self._Matrix(ea, mat, dim)
        self.ea, self.mat, self.minimal = ea, mat, minimal
        self.dim = dim = mat.getDim()
        self.native = ea.nativeDimension(dim)
        self.D = D = mat.D
        bsgs = D > hk.HELIB_KEYSWITCH_THRESH or (minimal and D > hk.HELIB_KEYSWITCH_MIN_THRESH)
        self.g = g = hk.KSGiantStepSize(D) if bsgs else 0
        self.times = {"construct": 0.0, "baby": 0.0, "muladd": 0.0, "giant": 0.0}
        self.sync = None
        self.fused = os.environ.get("HX_MATMUL_TERMWISE", "0") in ("", "0")
        self.onDevice = _onDevice(ea, mat, device_diagonals, self.deviceDiagonals)
        t0 = time.perf_counter()
        z, cc, maps, reqs = ea.zMStar, ea.cc, _Maps(ea), []
        if self.native:
            # MatMul1DExec_construct, native branch (src/matmul.cpp:626-643): diagonal i moved by rho^(-g floor(i / g))
            self.rotation = [(-g * (i // g)) if g else 0 for i in range(D)]
            reqs = [(i, 0, maps.add(z.genToPow(dim, self.rotation[i]))) for i in range(D)]
            idx = list(cc.ctxtPrimes) + (list(cc.specialPrimes) if g == 0 else [])
            self.multiplier = self._consts(reqs, maps, idx)
        else:
            # :644-688: vec[i] = (diag * mask_i) moved by rho^(-g k), vec1[i] = (diag - diag * mask_i) moved by
            # rho^(DD - g k), k = i / g (g = 0: no move and DD = D)
            for i in range(D):
                k, mask = (i // g if g else 1), ea.maskSlots(dim, i)
                reqs.append((i, 0, maps.add(z.genToPow(dim, -g * k), mask)))
                reqs.append((i, 0, maps.add(z.genToPow(dim, (0 if g else D) - g * k), 1 - mask)))
            both = self._consts(reqs, maps, list(cc.ctxtPrimes) + list(cc.specialPrimes))
            self.multiplier, self.multiplier1 = both[0::2], both[1::2]
        self._tick("construct", t0)


class BlockMatMul1DExec(bgv_matmul.MatMul1DExec):
    """BlockMatMul1DExec (src/matmul.cpp:1514-1976).  vec / vec1 hold None or (DoubleCRT of batch 1, size), indexed as
    the reference: [i * d + j] for strategy +1 (D >= d, the Frobenius factored out), [i + j * D] for strategy -1"""

    _Matrix = BlockMatMul1D

    def _consts(self, reqs, maps, idx):
        return _constants(self.ea, self.mat, reqs, maps, idx, self.onDevice)

    def __init__(self, ea, mat, minimal=False, dim=None, device_diagonals=None):
        if not isinstance(mat, self._Matrix):
            if dim is None:
                raise LogicError("BlockMatMul1DExec: a bare matrix needs its dimension (or pass a BlockMatMul1D)")
            mat = self._Matrix(ea, mat, dim)
        self.ea, self.mat, self.minimal = ea, mat, minimal
        self.dim = dim = mat.getDim()
        self.D, self.d = D, d = mat.D, ea.getDegree()
        self.native = True if dim == ea.dimension() else ea.nativeDimension(dim)
        self.strategy = +1 if D >= d else -1
        self.times = {"construct": 0.0, "baby": 0.0, "muladd": 0.0, "giant": 0.0}
        self.sync = None
        self.fused = os.environ.get("HX_MATMUL_TERMWISE", "0") in ("", "0")
        self.onDevice = _onDevice(ea, mat, device_diagonals, self.deviceDiagonals)
        t0 = time.perf_counter()
        z, cc, maps = ea.zMStar, ea.cc, _Maps(ea)
        m = ea.m
        where, reqs, reqs1 = [], [], []
        for i in range(D):
            mask = None if self.native else ea.maskSlots(dim, i)
            for j in range(d):
                if self.strategy == +1:
                    # build_ConstMultiplier(poly[j], -1, -j) (:1569); non-native (:1587-1601): sigma^-j first, then the
                    # mask; the second half moved by rho^D
                    where.append(i * d + j)
                    k0, k1 = z.genToPow(-1, -j), z.genToPow(-1, -j) * (1 if self.native else z.genToPow(dim, D)) % m
                else:
                    # build_ConstMultiplier(poly[j], dim, -i) (:1618); non-native (:1636-1647): poly1 by rho^-i, poly2
                    # by rho^(D - i)
                    where.append(i + j * D)
                    k0, k1 = z.genToPow(dim, -i), (1 if self.native else z.genToPow(dim, D - i))
                reqs.append((i, j, maps.add(k0, mask)))
                if not self.native:
                    reqs1.append((i, j, maps.add(k1, 1 - mask)))
        # the rotated ciphertexts come from a hoisting precon, on the ctxt and special primes: the constants live on both
        idx = list(cc.ctxtPrimes) + list(cc.specialPrimes)
        got = self._consts(reqs + reqs1, maps, idx)
        self.vec, self.vec1 = [None] * (D * d), ([None] * (D * d) if not self.native else None)
        for t, at in enumerate(where):
            self.vec[at] = got[t]
            if not self.native:
                self.vec1[at] = got[len(reqs) + t]
        self._tick("construct", t0)

    def mul(self, ct, pk=None, fused=None):
        """BlockMatMul1DExec::mul (:1697-1976) as one thread runs it: par_buf_sz = 1, iterative1 unless the strategy of
        dim1 is HELIB_KSS_FULL, iterative0 on HELIB_KSS_MIN.  Every accumulator's MulAdd sequence -- the rotations of
        dim0 in order -- is one group (hx_mul_add_many when the bookkeeping allows it)."""
        fused = self.fused if fused is None else fused
        ea, z, D, d, dim = self.ea, self.ea.zMStar, self.D, self.d, self.dim
        linalg._cleanUp(ct)
        (d0, dim0, d1, dim1) = (D, dim, d, -1) if self.strategy == +1 else (d, -1, D, dim)

        def strat(x):
            return hk.getKSStrategy(pk, x) if pk is not None else hk.HELIB_KSS_UNKNOWN
        iterative0 = strat(dim0) == hk.HELIB_KSS_MIN
        iterative1 = strat(dim1) != hk.HELIB_KSS_FULL
        lists = [self.vec] + ([] if self.native else [self.vec1])
        t0 = time.perf_counter()
        if iterative0:
            rot, sh = [], ct.clone()
            for i in range(d0):
                if i > 0:
                    sh = sh.clone()
                    sh.smartAutomorph(z.genToPow(dim0, 1))
                    linalg._cleanUp(sh)
                rot.append(sh)
        else:
            precon = bgv_matmul._generalAutomorphPrecon(ea, ct, dim0, strat(dim0))
            live = {i for i in range(d0) if any(v[i * d1 + j] is not None for v in lists for j in range(d1))}
            rot = [precon(i) if i in live else None for i in range(d0)]
        self._tick("baby", t0)
        sums = []
        for v in lists:
            acc = [linalg._empty(ct) for _ in range(d1)]
            for j in range(d1):
                self._group(acc[j], [(v[i * d1 + j], rot[i]) for i in range(d0) if v[i * d1 + j] is not None], fused)
            t0 = time.perf_counter()
            if iterative1:
                total = acc[d1 - 1]
                for j in range(d1 - 2, -1, -1):
                    if total.parts:
                        total.smartAutomorph(z.genToPow(dim1, 1))
                        linalg._cleanUp(total)
                    total += acc[j]
            else:
                total = linalg._empty(ct)
                for j in range(d1):
                    if j > 0 and acc[j].parts:
                        acc[j].smartAutomorph(z.genToPow(dim1, j))
                    total += acc[j]
            sums.append(total)
            self._tick("giant", t0)
        out = sums[0]
        if not self.native:
            t0 = time.perf_counter()
            if sums[1].parts:
                sums[1].smartAutomorph(z.genToPow(dim, -D))
            out += sums[1]
            self._tick("giant", t0)
        ct.__dict__.update(out.__dict__)
        return ct


# ---- linearized polynomials on ciphertexts ----
applyLinPolyLL = slot_ring.applyLinPolyLL


def applyLinPoly1(ea, ct, C):
    """the same map in every slot (:802-821): C [d, d] from buildLinPolyCoeffs"""
    _check(ea)
    return slot_ring.applyLinPoly1(ea, ct, C)


def applyLinPolyMany(ea, ct, Cvec):
    """another map in every slot (:826-850): Cvec [nslots, d, d], row i from buildLinPolyCoeffs for slot i"""
    _check(ea)
    return slot_ring.applyLinPolyMany(ea, ct, Cvec)
