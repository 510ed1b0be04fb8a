"""Linear maps on Galois-ring slots over helib_amd.bgv_gr.EncryptedArray: slots in Z_P[X] / G, P = p^r with any r >= 1, G
the Hensel lift of F_0, d <= 64, P < 2^31.  The interface is helib_amd.bgv_gf_matmul's with P where that module says p,
and the bodies are that module's private helpers, which take the modulus:

  linPolyMatrix / linPolyTable / buildLinPolyCoeffs / evalLinPoly / applyLinPolyLL / applyLinPoly1 / applyLinPolyMany
                      linearized polynomials over the ring (buildLinPolyCoeffs with ppsolve, src/EncryptedArray.cpp:740-879):
                      a Z_P-linear map of a slot is alpha -> sum_k C[k] sigma^k(alpha), sigma: X -> X^p.  The Moore matrix
                      of sigma is inverted mod P through the trace-dual basis (helib_amd.intraslot._Tables)
  slotAutomorph / automorphPlain      the plaintext automorphism X -> X^k: a permutation of the slots and a power of sigma
                      in every slot -- H(y^(p^e)) = sigma^e(H(y)) holds over Z_P because sigma fixes the lifted F_0
  MatMul1D / MatMul1DExec             a D x D matrix with ring entries [D, D, d] along one dimension, native or not
                      (src/matmul.cpp:449-688); a [D, D] integer matrix means constants
  BlockMatMul1D / BlockMatMul1DExec   d x d blocks over Z_P, one or n / D transforms, the size-1 dimension included
                      (src/matmul.cpp:1324-1976); mul is the existing classes', unchanged
  mulPlain            the plain-side truth of both

Constants reach the encode by one of three paths, all with identical words and sizes:

  host          numpy gathers and twists, ea.enc.encode: device_diagonals=False, a callable matrix, an injected encoder
  device        capi.BgvGfMatrix(ring=True) once (hx_bgv_gr_matrix_create: for blocks every entry's coefficients by
                bgv_gf_linpoly_kernel modulo P), capi.bgvGfGather per chunk, the slot arrays hop to the host and back
                into ea.enc.encode
  fused         fused=True: the same matrix, and hx_bgv_gf_encode_gathered (bgv_gf_gather_map_kernel: gather, sigma^e and
                the per-slot map in one pass, feeding the encode on the device) -- flags only per chunk first, then the
                live descriptors.  fused=None follows the class attribute fuseConstants wherever the device path runs
                and the encoder has encodeGathered.  The attribute is True: measured at m = 21845, p^r = 4, the fused
                path won every alternated pair against the device path (profiles/bgv_gr_matmul.json).  fused=True on
                an encoder without encodeGathered, or where the device path cannot run, raises LogicError

Refused with a message: MatMulFull and BlockMatMulFull* with ring entries, multipleTransforms for the ring-entry MatMul1D,
an array that is not bgv_gr.EncryptedArray.  EvalMap over these execs is helib_amd.evalmap.EvalMap (the name here keeps
raising, as it did before that module existed).  Nothing here imports oracle/."""
import numpy as np

from . import bgv_gf_matmul as GM
from . import bgv_gr, intraslot
from .ckks import LogicError

applyLinPolyLL = GM.applyLinPolyLL
CONSTANT_BATCH = 16        # constants per encode call (bgv_gf.GfEncoder's figure)


def _check(ea):
    if not isinstance(ea, bgv_gr.EncryptedArray):
        raise LogicError("linear maps on Galois-ring slots take helib_amd.bgv_gr.EncryptedArray")


class _Tables:
    """intraslot._Tables (frob, K over Z_P) and the flat table T[(j, b)][(k, c)] = [X^c](X^b K[j][k] mod G) beside them"""

    def __init__(self, ea):
        t = intraslot._tables(ea)
        self.ea, self.frob, self.K, self._T = ea, t.frob, t.K, None

    def flat(self):
        if self._T is None:
            d = self.K.shape[0]
            eye = np.eye(d, dtype=np.int64)
            T = np.stack([self.ea._mul(eye[:, None, :], self.K[j][None, :, :]) for j in range(d)])      # [j, b, k, c]
            self._T = np.ascontiguousarray(T.reshape(d * d, d * d))
        return self._T


def _tables(ea):
    t = ea.__dict__.get("_gr_linpoly")
    if t is None:
        t = ea.__dict__["_gr_linpoly"] = _Tables(ea)
    return t


def linPolyMatrix(ea):
    """(M, K) as int64 [d, d, d]: M[i][j] = sigma^i(X^j) mod G and its inverse over the ring"""
    _check(ea)
    t = _tables(ea)
    return t.frob.copy(), t.K.copy()


def linPolyTable(ea):
    """the flat d^2 x d^2 table over Z_P with C = E T"""
    _check(ea)
    return _tables(ea).flat()


def buildLinPolyCoeffs(ea, L):
    """EncryptedArrayDerived::buildLinPolyCoeffs over the ring: helib_amd.intraslot.buildLinPolyCoeffs"""
    _check(ea)
    return intraslot.buildLinPolyCoeffs(ea, L)


def linPolyFlat(ea, E):
    """buildLinPolyCoeffs through the flat table: what the device computes"""
    _check(ea)
    d = ea.getDegree()
    E = np.asarray(E, dtype=np.int64) % ea.P
    return GM._matmod(E.reshape(-1, d * d), linPolyTable(ea), ea.P).reshape(E.shape)


def evalLinPoly(ea, C, a):
    """sum_k C[k] sigma^k(alpha) slot by slot: C [d, d] (one map) or [nslots, d, d], a slots -> [B, nslots, d]"""
    _check(ea)
    return GM._evalLinPolyMod(ea, C, a, ea.P)


def slotAutomorph(ea, k):
    """X -> X^k on ring slots -> (perm, frob): the new slot j is sigma^frob[j] of the old slot perm[j]"""
    _check(ea)
    return GM._slotAutomorph(ea, k)


def automorphPlain(ea, a, k):
    """the slots of the plaintext with X -> X^k applied -> int64 [B, nslots, d]"""
    perm, frob = slotAutomorph(ea, k)
    return GM._frobEachMod((ea._slots(a) % ea.P)[:, perm], frob, _tables(ea).frob, ea.P)


class _GrHooks:
    ring = True
    _checkArray = staticmethod(_check)

    @staticmethod
    def _modulus(ea):
        return ea.P

    def _coeffs(self, dense):
        return intraslot.buildLinPolyCoeffs(self.ea, dense)


class MatMul1D(_GrHooks, GM.MatMul1D):
    """MatMul1D_derived with entries in Z_P[X] / G: A [D, D, d], a [D, D] integer matrix (constants), or a callable
    get(i, j) -> d coefficients (or an integer)"""


class BlockMatMul1D(_GrHooks, GM.BlockMatMul1D):
    """BlockMatMul1D_derived over Z_P: A [D, D, d, d] or [n / D, D, D, d, d] (multipleTransforms); dim = ea.dimension()
    is the size-1 dimension, [n, 1, 1, d, d]"""


def BlockMatMulFull(*args, **kwargs):
    raise LogicError("BlockMatMulFull / BlockMatMulFullExec over Galois-ring slots are not built: BlockMatMul1DExec works "
                     "along one dimension")


BlockMatMulFullExec = BlockMatMulFull


def MatMulFull(*args, **kwargs):
    raise LogicError("MatMulFull with ring entries is not built: MatMul1DExec here works along one dimension")


MatMulFullExec = MatMulFull


def EvalMap(*args, **kwargs):
    raise LogicError("EvalMap is not built: it needs the powerful-basis tables on top of BlockMatMul1D and MatMul1D")


def mulPlain(ea, v, mat):
    """mul(PlaintextArray, MatMul1D / BlockMatMul1D) on slots v -> int64 [B, nslots, d] modulo P"""
    _check(ea)
    return GM._mulPlainMod(ea, v, mat, ea.P)


def hostConstant(ea, mat, i, k, row):
    """one constant on the host: slot s = sigma^e(coefficient k of the entry the slot src[s] reads on diagonal i)"""
    return GM._hostConstantMod(mat, i, k, row, _tables(ea).frob, ea.P)


_Maps = GM._Maps


def _constants(ea, mat, reqs, maps, idx, device, fused=False):
    return GM._constants(ea, mat, reqs, maps, idx, device, fused=fused, const=lambda i, k, row: hostConstant(ea, mat, i, k, row),
                         batch=CONSTANT_BATCH if isinstance(ea.enc, bgv_gr.GrEncoder) else None)


class _GrExec:
    # fused=None: fuse the constants wherever the device path runs and the encoder has encodeGathered.  True because the
    # fused path won every alternated pair against the device path with the host hop (tools/bench_bgv_gr_matmul.py,
    # profiles/bgv_gr_matmul.json); set it to False to get that path back
    fuseConstants = True

    def _consts(self, reqs, maps, idx):
        can = self.onDevice and hasattr(self.ea.enc, "encodeGathered")
        if self._fused and not self.onDevice:
            raise LogicError("fused=True: the constants are fused on the device only (a dense matrix, device_diagonals "
                             "not False, an encoder over capi.BgvGf)")
        fused = bool(self.fuseConstants and can) if self._fused is None else bool(self._fused)
        self.fusedConstants = fused
        return _constants(self.ea, self.mat, reqs, maps, idx, self.onDevice, fused)

    def _start(self, ea, fused):
        _check(ea)
        self._fused = fused
        if fused and not hasattr(ea.enc, "encodeGathered"):
            raise LogicError("fused=True, but this encoder has no encodeGathered")


class MatMul1DExec(_GrExec, GM.MatMul1DExec):
    """MatMul1DExec for a matrix with ring entries; fused: how the constants are formed (the top of this module)"""
    _Matrix = MatMul1D

    def __init__(self, ea, mat, minimal=False, dim=None, device_diagonals=None, fused=None):
        self._start(ea, fused)
        GM.MatMul1DExec.__init__(self, ea, mat, minimal, dim, device_diagonals)


class BlockMatMul1DExec(_GrExec, GM.BlockMatMul1DExec):
    """BlockMatMul1DExec over Z_P; vec / vec1 as helib_amd.bgv_gf_matmul.BlockMatMul1DExec; fused: how the constants
    are formed (the top of this module)"""
    _Matrix = BlockMatMul1D

    def __init__(self, ea, mat, minimal=False, dim=None, device_diagonals=None, fused=None):
        self._start(ea, fused)
        GM.BlockMatMul1DExec.__init__(self, ea, mat, minimal, dim, device_diagonals)


def applyLinPoly1(ea, ct, C):
    """the same map in every slot: C [d, d] from buildLinPolyCoeffs"""
    _check(ea)
    return GM._applyLinPoly1(ea, ct, C)


def applyLinPolyMany(ea, ct, Cvec):
    """another map in every slot: Cvec [nslots, d, d], row i from buildLinPolyCoeffs for slot i"""
    _check(ea)
    return GM._applyLinPolyMany(ea, ct, Cvec)
