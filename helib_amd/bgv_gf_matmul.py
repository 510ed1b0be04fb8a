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

Both give the same words and sizes.  The bodies are private helpers that take the modulus of the slot words and the
tables (_evalLinPolyMod, _frobEachMod, _mulPlainMod, _hostConstantMod, _constants, the hooks of _GfMatrix and of the exec
classes): helib_amd.bgv_gr_matmul runs them modulo p^r over helib_amd.bgv_gr.EncryptedArray.  Refused with a message: BlockMatMulFull*, MatMulFull with GF entries,
multipleTransforms for the GF-entry MatMul1D, r > 1 (bgv_gf.EncryptedArray refuses it).  Nothing here imports oracle/."""
import os
import time

import numpy as np

from . import bgv, bgv_gf, bgv_hypercube, bgv_matmul, capi
from . import ctxt as hc
from . import keys as hk
from . import linalg
from .ckks import LogicError

GATHER_CHUNK = 64      # descriptors per gather call: 64 n d words of scratch


# ---- arithmetic modulo p ----
def _matmod(a, b, p):
    """a @ b mod p for non-negative int64 arrays below p, through Python integers when the sums could leave int64"""
    if p * p * max(1, a.shape[-1]) < 2 ** 63:
        return a @ b % p
    return np.array((a.astype(object) @ b.astype(object)) % p, dtype=np.int64)


def _invmod(a, p):
    """the inverse of a square matrix over Z_p (Gauss-Jordan on Python integers); LogicError when singular"""
    n = a.shape[0]
    w = np.concatenate([a.astype(object) % p, np.eye(n, dtype=object)], axis=1)
    for c in range(n):
        piv = next((r for r in range(c, n) if w[r, c]), None)
        if piv is None:
            raise LogicError("a singular matrix modulo p")
        if piv != c:
            w[[c, piv]] = w[[piv, c]]
        w[c] = w[c] * pow(int(w[c, c]), -1, p) % p
        for r in range(n):
            if r != c and w[r, c]:
                w[r] = (w[r] - w[r, c] * w[c]) % p
    return np.array(w[:, n:], dtype=np.int64)


class _Tables:
    """frob[e][l] = X^(l p^e) mod G; M[i][j] = (X^j)^(p^i) = frob[i][j] (buildLinPolyMatrix); K = M^-1 over the field,
    K[j][k] = beta_j^(p^k) with beta the dual basis of the powers of X under the trace (M is a Moore matrix: (K M)[j][j'] =
    sum_k (beta_j X^j')^(p^k) = Tr(beta_j X^j')); beta = the inverse of the Gram matrix Tr(X^(i + j)) over Z_p"""

    def __init__(self, ea):
        p, d = ea.p, ea.getDegree()
        F1 = ea._frobenius() % p
        self.frob = np.zeros((d, d, d), dtype=np.int64)
        self.frob[0] = np.eye(d, dtype=np.int64)
        for e in range(1, d):
            self.frob[e] = _matmod(self.frob[e - 1], F1, p)
        tr = self.frob[:, :, 0].sum(axis=0) % p                     # Tr(X^l) = sum_e [X^0](X^(l p^e)), l < d
        pw, x = [], np.zeros((1, 1, d), dtype=np.int64)
        x[0, 0, 0] = 1
        step = np.zeros((1, 1, d), dtype=np.int64)
        if d > 1:
            step[0, 0, 1] = 1
        for _ in range(2 * d - 1):                                  # X^s mod G, s <= 2 d - 2
            pw.append(x[0, 0])
            x = ea._mul(x, step) if d > 1 else x
        trs = _matmod(np.stack(pw), tr[:, None], p)[:, 0]
        gram = np.array([[trs[i + j] for j in range(d)] for i in range(d)], dtype=np.int64)
        beta = _invmod(gram, p)
        self.K = np.stack([np.stack([_matmod(beta[j][None, :], self.frob[k], p)[0] for k in range(d)]) for j in range(d)])
        self._T = None
        self.ea = ea

    def flat(self):
        """T[(j, b)][(k, c)] = [X^c](X^b K[j][k] mod G), [d^2, d^2]"""
        if self._T is None:
            d = self.K.shape[0]
            eye = np.eye(d, dtype=np.int64)
            T = np.stack([self.ea._mul(eye[:, None, :], self.K[j][None, :, :]) for j in range(d)])      # [j, b, k, c]
            self._T = np.ascontiguousarray(T.reshape(d * d, d * d))
        return self._T


def _tables(ea):
    t = ea.__dict__.get("_linpoly")
    if t is None:
        t = ea.__dict__["_linpoly"] = _Tables(ea)
    return t


def _check(ea):
    if getattr(ea, "r", 1) != 1:
        raise LogicError("linear maps on GF(p^d) slots at p^r with r > 1 (helib_amd.bgv_pr holds integers) are not built")
    if not isinstance(ea, bgv_gf.EncryptedArray):
        raise LogicError("linear maps on GF(p^d) slots take helib_amd.bgv_gf.EncryptedArray")


def linPolyMatrix(ea):
    """(M, K) as int64 [d, d, d]: M[i][j] = (X^j)^(p^i) mod G and its inverse over GF(p^d)"""
    _check(ea)
    t = _tables(ea)
    return t.frob.copy(), t.K.copy()


def linPolyTable(ea):
    """the flat d^2 x d^2 table over Z_p with C = E T"""
    _check(ea)
    return _tables(ea).flat()


def buildLinPolyCoeffs(ea, L):
    """EncryptedArrayDerived::buildLinPolyCoeffs: L [..., d, d], row j the coefficients of the image of X^j -> C
    [..., d, d], row k the coefficients of C[k] = sum_j L[j] K[j][k]; the map is alpha -> sum_k C[k] alpha^(p^k)"""
    _check(ea)
    p, d = ea.p, ea.getDegree()
    L = np.asarray(L, dtype=np.int64) % p
    if L.ndim < 2 or L.shape[-2:] != (d, d):
        raise LogicError("buildLinPolyCoeffs takes [..., d, d] with d = %d" % d)
    K = _tables(ea).K
    Lf = L.reshape(-1, d, d)
    C = np.zeros_like(Lf)
    for k in range(d):
        C[:, k, :] = ea._mul(Lf, K[None, :, k, :]).sum(axis=1) % p
    return C.reshape(L.shape)


def linPolyFlat(ea, E):
    """buildLinPolyCoeffs through the flat table: what the device computes"""
    _check(ea)
    d = ea.getDegree()
    E = np.asarray(E, dtype=np.int64) % ea.p
    return _matmod(E.reshape(-1, d * d), linPolyTable(ea), ea.p).reshape(E.shape)


def evalLinPoly(ea, C, a):
    """sum_k C[k] alpha^(p^k) slot by slot: C [d, d] (one map) or [nslots, d, d], a slots -> [B, nslots, d]"""
    return _evalLinPolyMod(ea, C, a, ea.p)


def _evalLinPolyMod(ea, C, a, p):
    """evalLinPoly with the modulus p of the slot words (ea.frobeniusPlain is sigma^k)"""
    a, d = ea._slots(a) % p, ea.getDegree()
    C = np.asarray(C, dtype=np.int64) % p
    C = np.broadcast_to(C, (ea.size(), d, d)) if C.ndim == 2 else C
    out = np.zeros_like(a)
    for k in range(d):
        out = (out + ea._mul(ea.frobeniusPlain(a, k), C[None, :, k, :])) % p
    return out


# ---- plaintext automorphisms ----
def slotAutomorph(ea, k):
    """X -> X^k on GF slots -> (perm, frob): the new slot j is Frob^frob[j] of the old slot perm[j].  Slot j reads the
    plaintext at zeta^(1 / t_j) (zeta = X mod G, t_j = reps()[j]); after the automorphism that is its value at
    zeta^(k / t_j) = zeta^(p^e / t_i) for the slot i whose coset holds t_j / k, with t_i k = t_j p^e (mod m), and H(y^(p^e))
    = H(y)^(p^e) over Z_p."""
    _check(ea)
    return _slotAutomorph(ea, k)


def _slotAutomorph(ea, k):
    """slotAutomorph for any array with bgv_gf's geometry (ea.p the prime): over Z_(p^r) the same holds with sigma^e for
    the e-th power of the Frobenius, because sigma fixes the lifted F_0"""
    m = ea.m
    k %= m
    cache = ea.__dict__.setdefault("_slotAut", {})
    if k not in cache:
        kinv, p, d = pow(k, -1, m), ea.p % m, ea.getDegree()
        log = {pow(p, e, m): e for e in range(d)}
        cos, reps = ea._cosets(), ea.zMStar.reps()
        perm = np.array([cos[t * kinv % m] for t in reps], dtype=np.int64)
        frob = np.array([log[reps[i] * k % m * pow(t, -1, m) % m] for i, t in zip(perm, reps)], dtype=np.int64)
        cache[k] = (perm, frob)
    return cache[k]


def _frobEach(ea, a, e):
    """slot s of a [B, n, d] -> its Frob^e[s]"""
    return _frobEachMod(a, e, _tables(ea).frob, ea.p)


def _frobEachMod(a, e, fr, p):
    """_frobEach over the tables fr = frob [d, d, d] modulo p"""
    out = a.copy()
    for x in np.unique(e):
        if x:
            w = e == x
            out[:, w] = _matmod(a[:, w], fr[x], p)
    return out


def automorphPlain(ea, a, k):
    """the slots of the plaintext with X -> X^k applied -> int64 [B, nslots, d]"""
    perm, frob = slotAutomorph(ea, k)
    return _frobEach(ea, (ea._slots(a) % ea.p)[:, perm], frob)


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


def _ints(ea, a):
    return _intsMod(a, ea.p)


def _intsMod(a, p):
    a = np.asarray(a)
    if a.dtype == object or a.dtype.kind not in "iu" or a.dtype == np.uint64:
        a = np.array([int(x) % p for x in a.reshape(-1)], dtype=np.int64).reshape(a.shape)
    return np.ascontiguousarray(a.astype(np.int64) % p)


class _GfMatrix:
    block = False
    ring = False               # the device matrix is built over a table of any r (capi.BgvGfMatrix(ring=True))

    # what a module over another ring of slots replaces: the check of the array, the modulus of the words, the
    # linearized-polynomial coefficients of the blocks
    _checkArray = staticmethod(lambda ea: _check(ea))

    @staticmethod
    def _modulus(ea):
        return ea.p

    def _coeffs(self, dense):
        return buildLinPolyCoeffs(self.ea, dense)

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
            self._values = self._coeffs(self.dense) if self.block else self.dense[:, :, :, None, :]
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
        p = self._modulus(ea)
        if self.callable:
            rows = [[np.atleast_1d(_intsMod(A(i, j), p)) for j in range(self.D)] for i in range(self.D)]
            A = [[np.pad(x, (0, d - len(x))) for x in r] for r in rows]
        a = _intsMod(A, p)
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
        a = _intsMod(A, self._modulus(ea))
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
    return _mulPlainMod(ea, v, mat, ea.p)


def _mulPlainMod(ea, v, mat, p):
    """mulPlain with the modulus p of the slot words (ea._mul is the product of the slots' ring)"""
    v, d, D = ea._slots(v) % p, ea.getDegree(), mat.D
    B, n = v.shape[0], ea.size()
    order = np.argsort(mat.blk * D + mat.col, kind="stable")           # slot of (transform, coordinate)
    x = v[:, order].reshape(B, n // D, D, d)
    A = mat.dense if mat.multiple else np.broadcast_to(mat.dense, (n // D,) + mat.dense.shape[1:])
    w = np.zeros_like(x)
    if mat.block:
        xo, Ao = (x.astype(object), A.astype(object)) if p * p * d >= 2 ** 63 else (x, A)
        terms = (xo[:, :, :, None, None, :] @ Ao[None])[..., 0, :] % p                     # [B, k, i, j, c]
        w = np.array(terms.sum(axis=2) % p, dtype=np.int64)
    else:
        for j in range(D):
            w[:, :, j] = ea._mul(x.reshape(B, -1, d), A[:, :, j].reshape(1, -1, d)).reshape(B, n // D, D, d).sum(axis=2) % p
    out = np.zeros_like(v)
    out[:, order] = w.reshape(B, n, d)
    return out


# ---- the constants of an exec ----
class _Maps:
    """the (source slot, Frobenius exponent) maps of an exec, each kept once: the automorphism X -> X^k behind a mask"""

    def __init__(self, ea):
        self.ea, self.rows, self.index = ea, [], {}

    def add(self, k, mask=None):
        perm, frob = _slotAutomorph(self.ea, k)
        src = perm if mask is None else np.where(np.asarray(mask)[perm] != 0, perm, -1)
        row = np.stack([src, np.where(src >= 0, frob, 0)], axis=1).astype(np.int32)
        key = row.tobytes()
        if key not in self.index:
            self.index[key] = len(self.rows)
            self.rows.append(row)
        return self.index[key]


def hostConstant(ea, mat, i, k, row):
    """one constant on the host: slot s = Frob^e(coefficient k of the entry the slot src[s] reads on diagonal i)"""
    return _hostConstantMod(mat, i, k, row, _tables(ea).frob, ea.p)


def _hostConstantMod(mat, i, k, row, fr, p):
    """hostConstant over the tables fr = frob [d, d, d] modulo p"""
    src, e = row[:, 0].astype(np.int64), row[:, 1].astype(np.int64)
    val = mat.slotValues(i, k)
    out = np.where((src >= 0)[:, None], val[np.maximum(src, 0)], 0)
    return _frobEachMod(out[None], e, fr, p)[0]


def _constants(ea, mat, reqs, maps, idx, device, fused=False, const=None, batch=None):
    """reqs [(i, k, map)] -> [None for a zero constant | (DoubleCRT of batch 1 on idx, size)].  const(i, k, row): one
    constant on the host (default hostConstant).  fused (device only): the constants never leave the device --
    enc.encodeGathered gives the flags of a chunk, then the live descriptors go through it in the encoder's batches.
    batch: constants per encode call for an encoder that is no GfEncoder and names no max_batch (None: one)"""
    enc = ea.enc
    step = max(1, int(getattr(enc, "max_batch", (batch or 16) if isinstance(enc, bgv_gf.GfEncoder) or batch else 1)))
    split = getattr(enc, "split", lambda poly: [poly])
    out = [None] * len(reqs)
    table = np.stack(maps.rows) if maps.rows else None
    handle = mat.handle(enc) if device else None
    if const is None:
        def const(i, k, row):
            return hostConstant(ea, mat, i, k, row)
    for lo in range(0, len(reqs), GATHER_CHUNK):
        chunk = reqs[lo:lo + GATHER_CHUNK]
        if device and fused:
            descs = np.array(chunk, dtype=np.int32)
            nz = enc.encodeGathered(handle, descs, table, 1, idx, flags_only=True)
        elif device:
            slots, nz = capi.bgvGfGather(handle, np.array(chunk, dtype=np.int32), table)
        else:
            slots = np.stack([const(i, k, maps.rows[mp]) for i, k, mp in chunk])
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
def applyLinPolyLL(ct, encodedC):
    """applyLinPolyLL (src/EncryptedArray.cpp:855-870): encodedC[j] is an EncodedPtxt (bgv_gf.EncryptedArray.encodePtxt)
    holding C[j] of every slot's map, or (DoubleCRT, size); the Frobenius keys come from keys.addFrbMatrices"""
    def times(c, k):
        if isinstance(k, bgv.EncodedPtxt):
            k.ea.multByConstant(c, k)
        else:
            c.multByConstant(*k)
    linalg._cleanUp(ct)
    tmp = ct.clone()
    times(ct, encodedC[0])
    for j in range(1, len(encodedC)):
        tmp1 = tmp.clone()
        tmp1.frobeniusAutomorph(j)
        times(tmp1, encodedC[j])
        ct += tmp1
    return ct


def applyLinPoly1(ea, ct, C):
    """the same map in every slot (:802-821): C [d, d] from buildLinPolyCoeffs"""
    _check(ea)
    return _applyLinPoly1(ea, ct, C)


def _applyLinPoly1(ea, ct, C):
    d = ea.getDegree()
    C = np.asarray(C, dtype=np.int64)
    if C.shape != (d, d):
        raise LogicError("ea's degree does not match the size of C")
    return applyLinPolyLL(ct, [ea.encodePtxt(np.broadcast_to(C[j], (1, ea.size(), d))) for j in range(d)])


def applyLinPolyMany(ea, ct, Cvec):
    """another map in every slot (:826-850): Cvec [nslots, d, d], row i from buildLinPolyCoeffs for slot i"""
    _check(ea)
    return _applyLinPolyMany(ea, ct, Cvec)


def _applyLinPolyMany(ea, ct, Cvec):
    d = ea.getDegree()
    Cvec = np.asarray(Cvec, dtype=np.int64)
    if Cvec.shape != (ea.size(), d, d):
        raise LogicError("Number of slots does not match size of Cvec, or an entry's size is unequal to the degree of ea")
    return applyLinPolyLL(ct, [ea.encodePtxt(Cvec[None, :, j, :]) for j in range(d)])
