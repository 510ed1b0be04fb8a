"""Comparison of integers held as encrypted bits (src/binaryCompare.cpp) over helib_amd.ctxt.Ctxt, BGV with plaintext
space 2.  Numbers are python lists of Ctxt, lowest bit first, as in helib_amd.binary_arith.

  compareTwoNumbers(a, b, twosComplement=False, cmp_only=False) -> (max, min, mu, ni), or (mu, ni) with cmp_only:
      mu = (a > b), ni = (a < b), max and min the larger and the smaller number, slot by slot.  As in the reference the
      longer operand plays b: when a is the longer one, mu and ni say how b compares with a.
  runningSums, compProducts, compEqGt    its stages

Not built: packedRecrypt.  Where the reference would recrypt and cannot, it raises LogicError("not enough levels for
comparison"); so does this.  Nothing here imports oracle/."""
from .binary_arith import BPL_ESTIMATE, _invalid, _multiplyBy, checkBits, findMinBitCapacity, ptr2nonNull, vecCopy
from .ckks import LogicError


def runningSums(v):
    """v[i] = sum_{j >= i} v[j], in place (:31-36)"""
    for i in range(len(v) - 1, 0, -1):
        v[i - 1] += v[i]


def _slice(start, size, frm, sz=-1):
    """CtPtrs_slice of a slice (include/helib/PtrVector.h:281-300): (start, size) of the part from `frm`, sz long"""
    frm = max(frm, 0)
    if sz == 0 or frm >= size:
        return start + frm, 0
    if sz < 0 or sz > size - frm:
        sz = size - frm
    return start + frm, sz


def compProducts(e, g, es=None, gs=None):
    """e*[i] = prod_{j >= i} e[j] and g*[i] = e*[i+1] g[i], in place; of the e*[i] only e*[0] and those the g*[i]
    need are computed (:43-95).  es, gs: (start, size) of the slices worked on (default: all)"""
    e0, n = es if es is not None else (0, len(e))
    g0, gn = gs if gs is not None else (0, len(g))
    if n <= 1:
        return
    ell = (n - 1).bit_length() - 1       # n/2 <= 2^ell < n
    n1 = n - (1 << ell)                  # in [1, n/2]
    compProducts(e, g, _slice(e0, n, 0, n1), _slice(g0, gn, 0, n1))
    compProducts(e, g, _slice(e0, n, n1, n - n1), _slice(g0, gn, n1, n - n1))
    # the first product of the second part into every product of the first
    for i in range(1 + n1):
        if i == 0:
            _multiplyBy(e[e0], e[e0 + n1])
        elif i - 1 < gn:
            _multiplyBy(g[g0 + i - 1], e[e0 + n1])


def compEqGt(a, b):
    """-> (aeqb, agtb): aeqb[i] = (a == b from bit i up), agtb[i] = (a > b from bit i up); len(b) >= len(a) (:99-165)"""
    aSize = len(a)
    aeqb, agtb = [], []
    for i in range(len(b)):
        eq = b[i].clone()
        eq.addScalar(1)                  # b + 1
        if i < aSize:
            gt = eq.clone()
            eq += a[i]                   # a + b + 1
            _multiplyBy(gt, a[i])        # a (b + 1)
            agtb.append(gt)
        aeqb.append(eq)
    compProducts(aeqb, agtb)
    runningSums(agtb)
    return aeqb, agtb


def compareTwoNumbers(aa, bb, twosComplement=False, cmp_only=False):
    checkBits(aa, bb)
    a, b = (aa, bb) if len(bb) >= len(aa) else (bb, aa)
    aSize, bSize = len(a), len(b)
    if any(c is None for c in a) or any(c is None for c in b):
        raise _invalid("compareTwoNumbers takes numbers without null bits")
    if aSize < 1:
        like = ptr2nonNull(b)
        if like is None:
            raise _invalid("compareTwoNumbers of two empty numbers")
        mu, ni = like._emptyLike(), like._emptyLike()
        ni.addScalar(1)
        return (mu, ni) if cmp_only else (vecCopy(b), [], mu, ni)
    # (with NumBits(bSize + 1) + 2 levels or fewer the reference recrypts first)
    if findMinBitCapacity(a, b) < (bSize.bit_length() + 1) * BPL_ESTIMATE:       # the bare minimum
        raise LogicError("not enough levels for comparison")
    e, ag = compEqGt(a, b)
    mu = ag[0].clone()                   # a > b
    ni = ag[0].clone()
    ni.addScalar(1)                      # a <= b
    ni += e[0]                           # a < b
    if twosComplement:                   # inverted iff the sign bits differ
        for c in [mu, ni] + ag:
            c += aa[-1]
            c += bb[-1]
    if cmp_only:
        return mu, ni
    mx, mn = [], []
    for i in range(aSize):
        hi = a[i].clone()
        hi -= b[i]
        _multiplyBy(hi, ag[i])           # (a - b) [a > b]
        lo = hi.clone()
        hi += b[i]
        lo -= a[i]
        mx.append(hi)
        mn.append(lo)
    mx += vecCopy(b[aSize:])
    return mx, mn, mu, ni
