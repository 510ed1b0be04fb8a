"""The passage between a slot and its d coordinates (src/intraSlot.cpp) over helib_amd.bgv_gf.EncryptedArray (r = 1) or
helib_amd.bgv_gr.EncryptedArray (any r): a slot alpha of Z_(p^r)[X] / G is written on the normal basis
theta, sigma(theta), ..., sigma^(d-1)(theta), sigma: X -> X^p, alpha = sum_i c_i sigma^i(theta), and

  unpack      one ciphertext -> d ciphertexts, slot s of the i-th holding c_i of slot s as a constant (:78-117)
  repack      the way back: sum_i unpacked[i] * (sigma^i(theta) in every slot) (:171-196)

The normal basis is what makes unpack cheap: sigma shifts the coordinates cyclically, c_(i+1)(sigma(alpha)) = c_i(alpha),
so c_i(alpha) = c_0(sigma^-i(alpha)); with c_0 written as the linearized polynomial sum_k C[k] sigma^k this is
c_i(alpha) = sum_k C[k] sigma^(k-i)(alpha) = sum_j C[(i + j) mod d] sigma^j(alpha): every coordinate is a sum over the
same d Frobenius images of the ciphertext, the d constants rotated (:108-115).  That loop is Ctxt.circulantCombination:
the call sequence or, fused, one hx_mul_add_circulant.

  normalBasisMatrices(ea, normal_element=None) -> (CB, CBi)     EncryptedArrayDerived::initNormalBasisMatrix
                      (src/EncryptedArray.cpp:488-550): CB[i] = the coordinates of sigma^i(theta), CBi its inverse mod
                      p^r (ppInvert: here Gauss-Jordan with unit pivots)
  buildLinPolyCoeffs(ea, L) / applyLinPolyPlain(ea, C, a)       EncryptedArrayDerived::buildLinPolyCoeffs (:740-790)
                      and the map it describes, over the Galois ring: helib_amd.slot_ring's behind this module's check
  buildUnpackSlotEncoding(ea)       :34-60
  unpack / unpackMany / repack / repackMany                     :78-160, :171-230
  packConstant / packConstants / unpackSlots                    :242-372
  unpackPlain / repackPlain         the plain-side truths

The normal element.  The reference draws theta from NTL's generator seeded with 1 until its conjugates are independent
mod p; that stream cannot be reproduced without NTL, so the rule here is deterministic: the candidates are X^k for
k = 0 .. d-1, then the polynomials with coefficients in {0, 1} in increasing order of the integer sum_i b_i 2^i (bit i
the coefficient of X^i), n = 1, 2, 3, ...; the first whose conjugates are independent mod p is taken.  A normal basis
exists over every finite field, and normality mod p is decided by the residues mod p, of which the {0, 1} polynomials
cover all for p = 2; for p > 2 the search is not proven to end among them.  It tries at most MAX_CANDIDATES 0/1
polynomials (normal elements are dense: a failure that late means the rule does not suit the ring) and then raises
LogicError (pass normal_element= then).  normal_element= injects a theta, for example the one of a genuine HElib run; one that is
not normal is refused.  Any normal theta gives a valid unpack / repack pair; the coordinates depend on it.

The arithmetic of a slot (the product mod G, sigma, matrices mod p^r, the inverse Moore matrix) is helib_amd.slot_ring.
Keys: helib_amd.keys.addFrbMatrices.  Nothing here imports oracle/."""
import numpy as np

from . import bgv_gf, bgv_gr, slot_ring
from . import ctxt as hc
from .ckks import LogicError
from .slot_ring import _invmod, _matmod, _tables  # noqa: F401  (_tables: the tests read frob and K through this module)


def _check(ea):
    if not isinstance(ea, (bgv_gf.EncryptedArray, bgv_gr.EncryptedArray)):
        raise LogicError("intraslot takes helib_amd.bgv_gf.EncryptedArray or helib_amd.bgv_gr.EncryptedArray")


# ---- the normal basis ----
def _conjugates(ea, theta):
    P, d = ea.P, ea.getDegree()
    S = ea._frobenius()                                             # sigma(alpha) = alpha S as row vectors
    rows = [np.asarray(theta, dtype=np.int64) % P]
    for _ in range(1, d):
        rows.append(_matmod(rows[-1][None, :], S, P)[0])
    return np.stack(rows)


MAX_CANDIDATES = 4096       # 0/1 polynomials tried after the d powers of X, each costing one d x d elimination


def _candidates(d):
    for k in range(d):
        yield [1 if i == k else 0 for i in range(d)]
    for n in range(1, min(1 << d, MAX_CANDIDATES + 1)):
        yield [(n >> i) & 1 for i in range(d)]


def normalBasisMatrices(ea, normal_element=None):
    """-> (CB, CBi), int64 [d, d] over Z_(p^r): CB[i] = the coordinates of sigma^i(theta), CBi = CB^-1.  theta is
    normal_element (d integers, lowest coefficient first; LogicError when its conjugates are dependent mod p) or the
    first normal candidate of the module's rule: X^0, ..., X^(d-1), then the {0, 1} polynomials in increasing integer
    order.  The rule's result is cached on ea."""
    _check(ea)
    p, P, d = ea.p, ea.P, ea.getDegree()
    if normal_element is not None:
        theta = [int(x) % P for x in normal_element]
        if len(theta) > d:
            raise LogicError("normalBasisMatrices: the normal element has more than d = %d coefficients" % d)
        theta += [0] * (d - len(theta))
        CB = _conjugates(ea, theta)
        CBi = _invmod(CB, p, P)
        if CBi is None:
            raise LogicError("normalBasisMatrices: the conjugates of the given element are dependent mod p: it is not normal")
        return CB, CBi
    got = ea.__dict__.get("_normal_basis")
    if got is None:
        for theta in _candidates(d):
            CB = _conjugates(ea, theta)
            CBi = _invmod(CB, p, P)
            if CBi is not None:
                got = ea.__dict__["_normal_basis"] = (CB, CBi)
                break
        else:
            raise LogicError("normalBasisMatrices: no normal element among the powers of X and the first %d 0/1 polynomials "
                             "(p = %d, d = %d): pass normal_element=" % (min((1 << d) - 1, MAX_CANDIDATES), p, d))
    return got[0].copy(), got[1].copy()


# ---- linearized polynomials over the Galois ring ----
def buildLinPolyCoeffs(ea, L):
    """EncryptedArrayDerived::buildLinPolyCoeffs over Z_(p^r)[X] / G: L [..., d, d], row j the coefficients of the image
    of X^j -> C [..., d, d], row k the coefficients of C[k]; the Z_(p^r)-linear map is alpha -> sum_k C[k] sigma^k(alpha)"""
    _check(ea)
    return slot_ring.buildLinPolyCoeffs(ea, L)


def applyLinPolyPlain(ea, C, a):
    """sum_k C[k] sigma^k(alpha) in every slot of a: C [d, d], a slots -> int64 [B, nslots, d]"""
    return slot_ring.evalLinPoly(ea, C, a)


# ---- the plain side ----
def unpackPlain(ea, a, normal_element=None):
    """slots a [B, nslots, d] -> int64 [B, nslots, d]: the normal-basis coordinates c_i of every slot (alpha CBi)"""
    _check(ea)
    P = ea.P
    CBi = normalBasisMatrices(ea, normal_element)[1]
    return _matmod(ea._slots(a) % P, CBi, P)


def repackPlain(ea, c, normal_element=None):
    """coordinates c [B, nslots, <= d] -> the slots sum_i c_i sigma^i(theta) (c CB)"""
    _check(ea)
    P = ea.P
    CB = normalBasisMatrices(ea, normal_element)[0]
    return _matmod(ea._slots(c) % P, CB, P)


def _int2Poly(ea, CB, data, nbits):
    d = ea.getDegree()
    if not 0 <= nbits <= d:
        raise LogicError("Not enough capacity in slots or nbits less than 0 (0 <= nbits <= d = %d)" % d)
    P = ea.P
    acc = np.zeros(d, dtype=np.int64)
    for i in range(nbits):
        if (int(data) >> i) & 1:
            acc = (acc + CB[i]) % P
    return acc


def packConstant(ea, data, nbits, normal_element=None):
    """packConstant (:242-320): the low nbits bits of data, bit i on sigma^i(theta), in every slot -> the zzX
    [1, phi(m)]"""
    _check(ea)
    CB = normalBasisMatrices(ea, normal_element)[0]
    poly = _int2Poly(ea, CB, data, nbits)
    return ea.encodeCoeffs(np.broadcast_to(poly, (1, ea.size(), ea.getDegree())))


def packConstants(ea, data, nbits, normal_element=None):
    """packConstants (:288-330): another integer in every slot -> the zzX [1, phi(m)]"""
    _check(ea)
    if len(data) != ea.size():
        raise LogicError("Cannot encode when data size is different to number of slots")
    CB = normalBasisMatrices(ea, normal_element)[0]
    return ea.encodeCoeffs(np.stack([_int2Poly(ea, CB, x, nbits) for x in data])[None])


def unpackSlots(ea, a, normal_element=None):
    """unpackSlots (:339-372): slots a (one vector) -> one integer per slot, bit j set when coordinate j is non-zero"""
    c = unpackPlain(ea, a, normal_element)[0]
    return [sum(1 << j for j in range(c.shape[1]) if c[i, j]) for i in range(c.shape[0])]


# ---- unpack / repack ----
def buildUnpackSlotEncoding(ea, normal_element=None):
    """buildUnpackSlotEncoding (:34-60): the d constants of the linearized polynomial of alpha -> c_0(alpha), the first
    normal coordinate (LM[j] = CBi[j][0]), C[j] in every slot, as EncodedPtxts"""
    _check(ea)
    d = ea.getDegree()
    CBi = normalBasisMatrices(ea, normal_element)[1]
    L = np.zeros((d, d), dtype=np.int64)
    L[:, 0] = CBi[:, 0]
    C = buildLinPolyCoeffs(ea, L)
    return [ea.encodePtxt(np.broadcast_to(C[j], (1, ea.size(), d))) for j in range(d)]


def unpack(ea, ct, unpackSlotEncoding, n=None, fused=None):
    """unpack (:78-117): -> n <= d ciphertexts (default d), slot s of out[i] holding c_i of slot s of ct as a constant.
    frob[j] = ct; frob[j].frobeniusAutomorph(j); frob[j].cleanUp(); then out[i] = sum_j frob[j] * C[(i + j) mod d] by
    Ctxt.circulantCombination: the reference's sequence or, with fused=True, one hx_mul_add_circulant with the same
    words, lnNoise, primeSet, ptxtSpace, intFactor and ptxtMag.  fused=None follows Ctxt.fuseCirculant; fused=True on
    a backend without mulAddCirculant raises LogicError.  The constants are expanded to the union of the prime sets of
    the Frobenius images (the reference expands them to ct's)."""
    _check(ea)
    d = ea.getDegree()
    n = d if n is None else int(n)
    if len(unpackSlotEncoding) != d or not 1 <= n <= d:
        raise LogicError("unpack takes the d = %d constants of buildUnpackSlotEncoding and 1 <= n <= d" % d)
    if ct.context is not ea.cc:
        raise LogicError("unpack: the ciphertext belongs to another context than the EncryptedArray")
    if fused and not hasattr(ct.ops, "mulAddCirculant"):
        raise LogicError("unpack: fused=True, but this backend has no mulAddCirculant")
    if not ct.parts:
        return [ct.clone() for _ in range(n)]
    frob = []
    for j in range(d):
        f = ct.clone()
        f.frobeniusAutomorph(j)
        f.cleanUp()
        frob.append(f)
    primes = sorted(frozenset().union(*[f.primeSet for f in frob]))
    consts = [ea.enc.encode(e.v, 1, primes) for e in unpackSlotEncoding]
    return hc.Ctxt.circulantCombination(frob, consts, n, fused=fused)


def unpackMany(ea, packed, unpackSlotEncoding, num, fused=None):
    """the list overload (:137-160): num <= len(packed) * d ciphertexts, d from each packed one in turn and the rest from
    the last one used"""
    d = ea.getDegree()
    if len(packed) * d < num:
        raise LogicError("Not enough ciphertexts. (Packed size * d < unpacked size)")
    out, idx = [], 0
    while num > 0:
        k = min(d, num)
        out += unpack(ea, packed[idx], unpackSlotEncoding, k, fused)
        idx += 1
        num -= k
    return out


def repack(ea, unpacked, normal_element=None):
    """repack (:171-196): sum_i unpacked[i] * (sigma^i(theta) in every slot) as a new ciphertext, i < len(unpacked) <= d;
    each product is Ctxt::multByConstant(zzX), of size embeddingLargestCoeff.  The sum runs through hx_mul_add_many when
    the terms share a prime set and its bookkeeping needs no data, and as the reference's sequence otherwise."""
    _check(ea)
    d = ea.getDegree()
    if not 1 <= len(unpacked) <= d:
        raise LogicError("repack takes between 1 and d = %d ciphertexts" % d)
    CB = normalBasisMatrices(ea, normal_element)[0]
    first = unpacked[0]
    ret = first._emptyLike()
    live = [(i, u) for i, u in enumerate(unpacked) if u.parts]
    if not live:
        return ret
    primes = sorted(frozenset().union(*[u.primeSet for _, u in live]))
    terms = []
    for i, u in live:
        e = ea.encodePtxt(np.broadcast_to(CB[i], (1, ea.size(), d)))
        ea._space(u, e)
        size = float(np.max(ea.enc.norm(e.poly)))
        terms.append((ea.enc.encode(e.v, 1, primes), size, u))
    if hasattr(first.ops, "mulAddMany") and len({u.primeSet for _, _, u in terms}) == 1 and _repackFused(ret, terms):
        return ret
    for c, size, u in terms:
        tmp = u.clone()
        tmp.multByConstant(c, size)
        ret += tmp
    return ret


def _repackFused(ret, terms):
    """one hx_mul_add_many for the sum when the sequence's bookkeeping needs no data; False (ret untouched) otherwise"""
    from . import linalg
    ops = terms[0][2].ops
    handles = set(terms[0][2].parts)
    if handles not in ({"1"}, {"1", "s"}) or any(set(u.parts) != handles for _, _, u in terms):
        return False
    idx = terms[0][2].parts["1"].getIndexSet()
    if any(u.parts[h].getIndexSet() != idx for _, _, u in terms for h in handles):
        return False
    sx = linalg._shadow(ret)
    try:
        for c, size, u in terms:
            tmp = linalg._shadow(u)
            tmp.multByConstant(c, size)
            sx += tmp
    except linalg._NeedsData:
        return False
    two = "s" in handles
    like = terms[0][2]
    ret.parts = {h: ops.zerosLike(like.parts[h]) for h in sorted(handles)}
    ops.mulAddMany(ret.parts["1"], ret.parts["s"] if two else None, [c for c, _, _ in terms],
                   [u.parts["1"] for _, _, u in terms], [u.parts["s"] for _, _, u in terms] if two else None,
                   accumulate=False)
    ret.primeSet, ret.ptxtSpace, ret.intFactor = sx.primeSet, sx.ptxtSpace, sx.intFactor
    ret.lnNoise, ret.ptxtMag, ret.lnRatFactor = sx.lnNoise, sx.ptxtMag, sx.lnRatFactor
    return True


def repackMany(ea, unpacked, normal_element=None):
    """the list overload (:210-230): -> ceil(len(unpacked) / d) ciphertexts, d unpacked ones into each"""
    d = ea.getDegree()
    return [repack(ea, unpacked[k:k + d], normal_element) for k in range(0, len(unpacked), d)]
