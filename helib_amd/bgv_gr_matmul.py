"""Linear maps on Galois-ring slots over helib_amd.bgv_gr.EncryptedArray: slots in Z_P[X] / G, P = p^r with any r >= 1, G
the Hensel lift of F_0, d <= 64, P < 2^31.  The interface is helib_amd.bgv_gf_matmul's.  The arithmetic lives in
helib_amd.slot_ring, which reads the modulus from the array; the functions here are this module's check of the array in
front of it, and the matrix and exec classes are bgv_gf_matmul's over hx_bgv_gr_matrix_create, with the fused constants:

  linPolyMatrix / linPolyTable / buildLinPolyCoeffs / evalLinPoly / applyLinPolyLL / applyLinPoly1 / applyLinPolyMany
                      linearized polynomials over the ring (buildLinPolyCoeffs with ppsolve, src/EncryptedArray.cpp:740-879):
                      a Z_P-linear map of a slot is alpha -> sum_k C[k] sigma^k(alpha), sigma: X -> X^p.  The Moore matrix
                      of sigma is inverted mod P through the trace-dual basis (helib_amd.slot_ring._Tables)
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
from . import bgv_gf_matmul as GM
from . import bgv_gr, slot_ring
from .ckks import LogicError

applyLinPolyLL = slot_ring.applyLinPolyLL


def _check(ea):
    if not isinstance(ea, bgv_gr.EncryptedArray):
        raise LogicError("linear maps on Galois-ring slots take helib_amd.bgv_gr.EncryptedArray")


def linPolyMatrix(ea):
    """(M, K) as int64 [d, d, d]: M[i][j] = sigma^i(X^j) mod G and its inverse over the ring"""
    _check(ea)
    t = slot_ring._tables(ea)
    return t.frob.copy(), t.K.copy()


def linPolyTable(ea):
    """the flat d^2 x d^2 table over Z_P with C = E T"""
    _check(ea)
    return slot_ring._tables(ea).flat()


def buildLinPolyCoeffs(ea, L):
    """EncryptedArrayDerived::buildLinPolyCoeffs over the ring: L [..., d, d], row j the image of X^j -> C [..., d, d]"""
    _check(ea)
    return slot_ring.buildLinPolyCoeffs(ea, L)


def linPolyFlat(ea, E):
    """buildLinPolyCoeffs through the flat table: what the device computes"""
    _check(ea)
    return slot_ring.linPolyFlat(ea, E)


def evalLinPoly(ea, C, a):
    """sum_k C[k] sigma^k(alpha) slot by slot: C [d, d] (one map) or [nslots, d, d], a slots -> [B, nslots, d]"""
    _check(ea)
    return slot_ring.evalLinPoly(ea, C, a)


def slotAutomorph(ea, k):
    """X -> X^k on ring slots -> (perm, frob): the new slot j is sigma^frob[j] of the old slot perm[j]"""
    _check(ea)
    return slot_ring.slotAutomorph(ea, k)


def automorphPlain(ea, a, k):
    """the slots of the plaintext with X -> X^k applied -> int64 [B, nslots, d]"""
    _check(ea)
    return slot_ring.automorphPlain(ea, a, k)


class _GrHooks:
    ring = True                # hx_bgv_gr_matrix_create
    _checkArray = staticmethod(_check)


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
    return slot_ring.mulPlain(ea, v, mat)


hostConstant = slot_ring.hostConstant
_Maps = GM._Maps
_constants = GM._constants


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
        return GM._constants(self.ea, self.mat, reqs, maps, idx, self.onDevice, fused)

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
    return slot_ring.applyLinPoly1(ea, ct, C)


def applyLinPolyMany(ea, ct, Cvec):
    """another map in every slot: Cvec [nslots, d, d], row i from buildLinPolyCoeffs for slot i"""
    _check(ea)
    return slot_ring.applyLinPolyMany(ea, ct, Cvec)
