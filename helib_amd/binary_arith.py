"""Binary arithmetic on encrypted bits (src/binaryArith.cpp) over helib_amd.ctxt.Ctxt, BGV with plaintext space 2.

A number is a python list, lowest bit first, of Ctxt or None (the reference's null pointer); an empty ciphertext (no
parts) is the constant 0.  A matrix of numbers is a list of lists.  Functions return new lists and leave their inputs as
they were, except addManyNumbers, which works in place on `numbers` as the reference does.  Every slot of every batch
element is one independent number (bit-sliced: numbers[i] holds bit i of all of them).

  AddDAG                                   the plan of addTwoNumbers: init's rules word for word (:211-320), apply with
                                           getCtxt's parent-reuse order (:323-423)
  addTwoNumbers, addManyNumbers, multTwoNumbers (multByNegative), negateBinary, subtractBinary
  three4Two / binaryCond                   take lazy=None, which follows the module flag lazyCarry: the carry
                                           u v + (u + v) w and the conditional cond t + (cond + 1) f as ONE
                                           Ctxt.innerProduct -- one relinearisation instead of two; the slots are the
                                           same, the words are not
  bitwiseXOR / Or / And / Not, binaryMask, concatBinaryNums, splitBinaryNums, leftBitwiseShift, bitwiseRotate
  fifteenOrLess4Four (seven4Three, fifteen4Four), longToBitVector, decryptBinaryNums, encryptBinaryNums

Not built: packedRecrypt and the unpackSlotEncoding argument.  Where the reference would recrypt, these functions raise
what it raises when it cannot: LogicError("not enough levels for addition DAG") and the InvalidArgument of
addManyNumbers below 3 BPL.  Nothing here imports oracle/."""
import sys

import numpy as np

from . import capi
from .ckks import LogicError
from .ctxt import Ctxt, incrementalProduct

BPL_ESTIMATE = 30   # src/binaryArith.cpp:32; Context::BPL() is 30 as well (include/helib/Context.h:743)
LONG_MAX = sys.maxsize
# lazy=None in three4Two, binaryCond and the callers that pass it down: the reference's two multiplyBy until the
# one-relinearisation form has been measured ahead in every pair of tools/bench_binary_arith.py
lazyCarry = False


def _invalid(msg):
    return capi.InvalidArgument(capi.HX_ERR_INVALID, msg)


def _lazy(lazy):
    return lazyCarry if lazy is None else bool(lazy)


# ---- CtPtrs over python lists (include/helib/PtrVector.h, CtPtrs.h) ----
def isSet(v, i):
    return 0 <= i < len(v) and v[i] is not None


def isEmpty(c):
    """a null pointer or Ctxt::isEmpty"""
    return c is None or not c.parts


def ptr2nonNull(v):
    for c in v:
        if isinstance(c, list):
            c = ptr2nonNull(c)
        if c is not None:
            return c
    return None


def checkBits(*numbers):
    """every ciphertext of the numbers holds bits: plaintext space 2"""
    for v in numbers:
        for c in (v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(c, (list, tuple)):
                checkBits(c)
            elif c is not None and (c.context.ckks or c.ptxtSpace != 2):
                raise _invalid("binary arithmetic takes ciphertexts with plaintext space 2 (this one has %s)"
                               % ("CKKS" if c.context.ckks else c.ptxtSpace))


def findMinBitCapacity(*numbers):
    lvl = LONG_MAX
    for v in numbers:
        for c in v:
            if isinstance(c, list):
                lvl = min(lvl, findMinBitCapacity(c))
            elif not isEmpty(c):
                lvl = min(lvl, c.bitCapacity())
    return lvl


def _copy(c, like=None):
    """*dst = *src; a null source gives an empty ciphertext where there is something to shape it after"""
    if c is not None:
        return c.clone()
    return like._emptyLike() if like is not None else None


def vecCopy(v, sizeLimit=0):
    n = len(v)
    if 0 < sizeLimit < n:
        n = sizeLimit
    like = ptr2nonNull(v)
    return [_copy(v[i], like) for i in range(n)]


def _multiplyBy(x, y):
    """x.multiplyBy(y) with the reference's empty cases (src/Ctxt.cpp:1685-1692): 0 * y = 0, x * 0 = 0"""
    if not x.parts:
        return x
    if isEmpty(y):
        x.clear()
        return x
    return x.multiplyBy(y)


def longToBitVector(num, bitSize):
    if bitSize < 0:
        raise _invalid("bitSize must be non-negative.")
    return [(int(num) >> i) & 1 for i in range(bitSize)]


# ---- the addition DAG (src/binaryArith.cpp:43-455) ----
class DAGnode:
    def __init__(self, idx, isQ, level, childrenLeft=0, parent1=None, parent2=None):
        self.idx, self.isQ, self.level, self.childrenLeft = idx, isQ, level, childrenLeft
        self.parent1, self.parent2, self.ct = parent1, parent2, None

    def nodeName(self):
        return "%s(%d,%d)" % ("Q" if self.isQ else "P", self.idx[0], self.idx[1])


def defaultPmiddle(delta):
    return 1 << (delta.bit_length() - 1)


def defaultQmiddle(delta):
    delta = (2 * delta + 2) // 3
    return 1 << (delta.bit_length() - 1)


class AddDAG:
    """p[i,j] = prod_{t=j..i} (a[t] + b[t]), q[i,j] = a[j] b[j] prod_{t=j+1..i} (a[t] + b[t]); every internal node is
    the product of two parents, chosen to keep its level as high as possible and then the number of nodes that must be
    computed as low as possible.  level: the planner's estimate of the bit capacity, BPL_ESTIMATE per product."""

    def __init__(self, a, b):
        self.init(a, b)

    def findP(self, i, j):
        return self.p.get((i, j))

    def findQ(self, i, j):
        return self.q.get((i, j))

    def lowLvl(self):
        if self.aSize < 1:
            return 0
        return self.findQ(self.bSize - 1, 0).level

    def init(self, aa, bb):
        a, b = (aa, bb) if len(bb) >= len(aa) else (bb, aa)
        self.aSize, self.bSize = aSize, bSize = len(a), len(b)
        if aSize < 1:
            raise _invalid("a must not be empty")
        p, q = self.p, self.q = {}, {}

        def lvlOf(v, i):
            return v[i].bitCapacity() if isSet(v, i) and v[i].parts else LONG_MAX
        for i in range(bSize):
            lvl = lvlOf(b, i)
            if i < aSize:
                aLvl = lvlOf(a, i)
                lvl = min(lvl, aLvl)
                if lvl == LONG_MAX or aLvl == LONG_MAX:      # either a[i] or b[i] is empty
                    q[i, i] = DAGnode((i, i), True, LONG_MAX, 1)
                else:
                    q[i, i] = DAGnode((i, i), True, lvl - 1, 1)
            p[i, i] = DAGnode((i, i), False, lvl, 1)

        def product(p1, p2):
            if p1.level == LONG_MAX or p2.level == LONG_MAX:    # a parent is empty
                return LONG_MAX
            return min(p1.level, p2.level) - BPL_ESTIMATE
        # p[i,j] for bSize > i > j >= 0
        for delta in range(1, bSize):
            for i in range(bSize - 1, delta - 1, -1):
                j = i - delta
                mid = i - defaultPmiddle(delta)          # a "good default"
                prnt2, prnt1 = p[i, mid + 1], p[mid, j]
                maxLvl = product(prnt1, prnt2)
                maxN = min(prnt1.childrenLeft, prnt2.childrenLeft)
                for m in range(j, i):                    # the middle point maximising the level, then childrenLeft
                    if m == mid:
                        continue
                    p2, p1 = p[i, m + 1], p[m, j]
                    lvl = product(p1, p2)
                    n = min(p1.childrenLeft, p2.childrenLeft)
                    if lvl > maxLvl or (lvl == maxLvl and n > maxN):
                        maxLvl, maxN, prnt1, prnt2 = lvl, n, p1, p2
                p[i, j] = DAGnode((i, j), False, maxLvl, 0, prnt1, prnt2)
                prnt1.childrenLeft += 1
                prnt2.childrenLeft += 1
        # q[i,j] for bSize > i > j >= 0, j < aSize
        for delta in range(1, bSize):
            for i in range(bSize - 1, delta - 1, -1):
                j = i - delta
                if j >= aSize:
                    continue
                maxLvl = maxN = 0
                mid = i - defaultQmiddle(delta)
                prnt2, prnt1 = p[i, mid + 1], q.get((mid, j))
                if prnt1 is not None:
                    maxLvl = product(prnt1, prnt2)
                    maxN = prnt2.childrenLeft
                for m in range(j, i):
                    if m == mid:
                        continue
                    p2, p1 = p[i, m + 1], q.get((m, j))
                    if p1 is None:
                        continue
                    lvl = product(p1, p2)
                    n = p2.childrenLeft
                    if lvl > maxLvl or (lvl == maxLvl and n > maxN):
                        maxLvl, maxN, prnt1, prnt2 = lvl, n, p1, p2
                if prnt1 is None:
                    continue                             # cannot create the node
                q[i, j] = DAGnode((i, j), True, maxLvl, 1, prnt1, prnt2)
                prnt1.childrenLeft += 1
                prnt2.childrenLeft += 1

    def apply(self, aa, bb, sizeLimit=0):
        """the sum, sizeLimit bits of it (0: bSize + 1).  A plan is applied once: it counts its nodes' children down."""
        a, b = (aa, bb) if len(bb) >= len(aa) else (bb, aa)
        if self.aSize != len(a) or self.bSize != len(b):
            raise LogicError("DAG applied to wrong vectors")
        if sizeLimit == 0:
            sizeLimit = self.bSize + 1
        like = ptr2nonNull(b)
        if like is None:
            raise _invalid("ct_ptr must not be null")
        total = [like._emptyLike() for _ in range(sizeLimit)]
        for i in range(sizeLimit):
            if i < self.bSize:
                self._addCtxtFromNode(total[i], self.findP(i, i), a, b, like)
            for j in range(min(i - 1, self.aSize - 1), -1, -1):
                node = self.findQ(i - 1, j)
                if node is not None:
                    self._addCtxtFromNode(total[i], node, a, b, like)
        return total

    def _addCtxtFromNode(self, c, node, a, b, like):
        c += self._getCtxt(node, a, b, like)
        node.childrenLeft -= 1
        if node.childrenLeft == 0:
            node.ct = None

    def _getCtxt(self, node, a, b, like):
        if node.ct is not None:
            return node.ct
        if node.parent1 is not None and node.parent2 is not None:      # an internal node
            c1 = self._getCtxt(node.parent1, a, b, like)
            node.parent1.childrenLeft -= 1
            n1 = node.parent1.childrenLeft
            c2 = self._getCtxt(node.parent2, a, b, like)
            node.parent2.childrenLeft -= 1
            n2 = node.parent2.childrenLeft
            zero = not c1.parts or not c2.parts                        # the product is zero if a parent is
            if n1 == 0:                                                # reuse parent1's ciphertext
                node.parent1.ct = None
                node.ct = c1
                if zero:
                    c1.clear()
                else:
                    c1.multiplyBy(c2)
                if n2 == 0:
                    node.parent2.ct = None
            elif n2 == 0:                                              # reuse parent2's
                node.parent2.ct = None
                node.ct = c2
                if zero:
                    c2.clear()
                else:
                    c2.multiplyBy(c1)
            else:
                if zero:
                    node.ct = like._emptyLike()
                else:
                    node.ct = c2.clone()
                    node.ct.multiplyBy(c1)
        else:                                                          # a source: a[i] * b[i] or a[i] + b[i]
            i, j = node.idx
            bi = b[i] if isSet(b, i) and b[i].parts else None
            aj = a[j] if isSet(a, j) and a[j].parts else None
            if node.isQ:
                if bi is not None and aj is not None:
                    node.ct = bi.clone()
                    node.ct.multiplyBy(aj)
                else:
                    node.ct = like._emptyLike()
            else:
                node.ct = bi.clone() if bi is not None else like._emptyLike()
                if aj is not None:
                    node.ct += aj
        return node.ct


def addTwoNumbers(lhs, rhs, sizeLimit=0):
    """lhs + rhs, sizeLimit bits of it (0: one more than the longer input) (src/binaryArith.cpp:644-676)"""
    checkBits(lhs, rhs)
    if len(lhs) < 1:
        return vecCopy(rhs, sizeLimit)
    if len(rhs) < 1:
        return vecCopy(lhs, sizeLimit)
    plan = AddDAG(lhs, rhs)
    if plan.lowLvl() < BPL_ESTIMATE:     # (the reference recrypts here and plans again)
        raise LogicError("not enough levels for addition DAG")
    return plan.apply(lhs, rhs, sizeLimit)


def negateBinary(number):
    """-number in two's complement (src/binaryArith.cpp:680-697): flip the bits, add one"""
    checkBits(number)
    like = ptr2nonNull(number)
    if like is None:
        return list(number)
    flipped = vecCopy(number)
    for bit in flipped:
        bit.addScalar(1)
    negation = vecCopy(flipped)
    negation[0].addScalar(1)
    incrementalProduct(flipped)          # the carry bits
    for i in range(1, len(flipped)):
        negation[i] += flipped[i - 1]
    return negation


def subtractBinary(lhs, rhs):
    """lhs - rhs modulo 2^size (src/binaryArith.cpp:700-718)"""
    if len(lhs) != len(rhs):
        raise _invalid("Size of lhs and rhs must be the same.")
    return addTwoNumbers(lhs, negateBinary(rhs), len(lhs))


# ---- 3-for-2 (src/binaryArith.cpp:720-875) ----
def _three4TwoBits(u, v, w, like, lazy):
    """bits u, v, w (null or empty: zero) -> (lsb, msb, the number of outputs that are not identically zero) with
    lsb + 2 msb = u + v + w.  lazy: the carry as one inner product."""
    live = [c for c in (u, v, w) if not isEmpty(c)]      # the empty ones go to the end
    if not live:
        return like._emptyLike(), like._emptyLike(), 0
    if len(live) == 1:
        return live[0].clone(), like._emptyLike(), 1
    u, v = live[0], live[1]
    lsb = u.clone()
    lsb += v                             # u + v
    if len(live) == 2:
        msb = u.clone()
        msb.multiplyBy(v)
        return lsb, msb, 2
    w = live[2]
    if lazy:                             # u v + (u + v) w under one key switch
        msb = Ctxt.innerProduct([u, lsb], [v, w])
    else:
        msb = u.clone()
        msb.multiplyBy(v)                # u v
        tmp = lsb.clone()
        tmp.multiplyBy(w)                # (u + v) w
        msb += tmp
    lsb += w                             # u + v + w
    return lsb, msb, 2


def orderBySize(a, b, c):
    """the three numbers from the shortest to the longest, ties as the reference breaks them (:721-741)"""
    if len(a) <= len(b):
        if len(b) <= len(c):
            return a, b, c
        return (a, c, b) if len(a) <= len(c) else (c, a, b)
    if len(a) <= len(c):
        return b, a, c
    return (b, c, a) if len(b) <= len(c) else (c, b, a)


def three4Two(u, v, w, sizeLimit=0, lazy=None):
    """Bits (Ctxt or None) -> (lsb, msb, count); numbers (lists) -> (lsb, msb) with lsb + 2 msb = u + v + w, msb already
    shifted: msb[0] is an empty ciphertext."""
    lazy = _lazy(lazy)
    if not isinstance(u, list):
        like = ptr2nonNull([u, v, w])
        if like is None:
            raise _invalid("three4Two of three null pointers")
        checkBits([u, v, w])
        return _three4TwoBits(u, v, w, like, lazy)
    checkBits(u, v, w)
    p1, p2, p3 = orderBySize(u, v, w)
    if len(p3) <= 0:
        return [], []
    if len(p1) <= 0:
        return vecCopy(p2, sizeLimit), vecCopy(p3, sizeLimit)
    if sizeLimit == 0:
        sizeLimit = len(p3) + 1
    like = ptr2nonNull(p3) or ptr2nonNull(p2) or ptr2nonNull(p1)
    if like is None:
        raise _invalid("three4Two of numbers without a ciphertext")
    lsbSize = min(sizeLimit, len(p3))
    msbSize = lsbSize
    if len(p2) == len(p3) and lsbSize < sizeLimit:
        msbSize += 1                     # a possible carry out of the last position
    lsb = [like._emptyLike() for _ in range(lsbSize)]
    msb = [like._emptyLike() for _ in range(msbSize)]
    for i in range(msbSize - 1):
        if i < len(p1):
            lsb[i], msb[i + 1], _ = _three4TwoBits(p1[i], p2[i], p3[i], like, lazy)
        elif i < len(p2):
            lsb[i], msb[i + 1], _ = _three4TwoBits(p2[i], p3[i], None, like, lazy)
        elif isSet(p3, i):
            lsb[i] = p3[i].clone()
    if msbSize == lsbSize:               # the last position has no carry out: its LSB alone
        for p in (p1, p2, p3):
            if isSet(p, lsbSize - 1):
                lsb[lsbSize - 1] += p[lsbSize - 1]
    return lsb, msb


def addManyNumbers(numbers, sizeLimit=0, lazy=None):
    """the sum of the numbers by 3-for-2 until two are left (src/binaryArith.cpp:895-966).  Works in place: the lists of
    `numbers` are overwritten with intermediate results."""
    checkBits(numbers)
    like = ptr2nonNull(numbers)
    if len(numbers) < 1 or like is None:
        return []
    if len(numbers) == 1:
        return vecCopy(numbers[0])
    nums = list(numbers)
    while len(nums) > 2:
        if findMinBitCapacity(nums) < 3 * BPL_ESTIMATE:      # (the reference recrypts here)
            raise _invalid("unpackSlotEncoding must not be null")
        nTriples = len(nums) // 3
        out = nums[3 * nTriples:]
        for i in range(nTriples):
            x, y = three4Two(nums[3 * i], nums[3 * i + 1], nums[3 * i + 2], sizeLimit, lazy)
            nums[3 * i][:] = x
            nums[3 * i + 1][:] = y
            out += [nums[3 * i], nums[3 * i + 1]]
        nums = out
    return addTwoNumbers(nums[0], nums[1], sizeLimit)


def multByNegative(a, b, sizeLimit=0, lazy=None):
    """a positive a by a b in two's complement: the rows of the product are sign-extended (:969-1022)"""
    resSize = len(a) + len(b)
    if 0 < sizeLimit < resSize:
        resSize = sizeLimit
    like = ptr2nonNull(a)
    nNums = min(len(a), resSize)
    numbers = [[like._emptyLike() for _ in range(resSize)] for _ in range(nNums)]
    for i in range(nNums):
        for j in range(i, resSize):
            if j < i + len(b) and isSet(a, i) and a[i].parts and isSet(b, j - i) and b[j - i].parts:
                numbers[i][j] = b[j - i].clone()
                numbers[i][j].multiplyBy(a[i])
    for i in range(nNums):
        for j in range(i + len(b), resSize):
            numbers[i][j] = numbers[i][i + len(b) - 1].clone()      # sign extension
    return addManyNumbers(numbers, resSize, lazy)


def multTwoNumbers(lhs, rhs, rhsTwosComplement=False, sizeLimit=0, lazy=None):
    """lhs * rhs (src/binaryArith.cpp:1027-1122): the pairwise bit products summed by addManyNumbers.  The one-bit edge
    cases return the other operand's bits times that bit; where the reference's loops run one position past the copy
    (and, for a one-bit rhs, multiply lhs itself), this multiplies the copy's own bits and leaves the inputs alone."""
    checkBits(lhs, rhs)
    lhsSize, rhsSize = len(lhs), len(rhs)
    resSize = lhsSize + rhsSize
    if 0 < sizeLimit < resSize:
        resSize = sizeLimit
    if ptr2nonNull(lhs) is None or ptr2nonNull(rhs) is None:
        return []
    if lhsSize == 1:
        if isEmpty(lhs[0]):
            return []
        product = vecCopy(rhs, resSize)
        for bit in product:
            _multiplyBy(bit, lhs[0])
        return product
    if rhsTwosComplement:
        return multByNegative(lhs, rhs, sizeLimit, lazy)
    if rhsSize == 1:
        if isEmpty(rhs[0]):
            return []
        product = vecCopy(lhs, resSize)
        for bit in product:
            _multiplyBy(bit, rhs[0])
        return product
    like = ptr2nonNull(lhs)
    longer = max(lhsSize, rhsSize)
    nNums = min(rhsSize, resSize)
    numbers = [[like._emptyLike() for _ in range(min(i + longer, resSize))] for i in range(nNums)]
    for i in range(nNums):
        for j in range(i, len(numbers[i])):
            if isSet(lhs, j - i) and lhs[j - i].parts and isSet(rhs, i) and rhs[i].parts:
                numbers[i][j] = lhs[j - i].clone()
                numbers[i][j].multiplyBy(rhs[i])
    return addManyNumbers(numbers, resSize, lazy)


# ---- masks, conditionals, bit-wise operations (src/binaryArith.cpp:502-641) ----
def binaryMask(bits, mask):
    checkBits(bits, [mask])
    out = vecCopy(bits)
    for bit in out:
        _multiplyBy(bit, mask)
    return out


def binaryCond(cond, trueValue, falseValue, lazy=None):
    """cond ? trueValue : falseValue, bit by bit: cond t + (cond + 1) f.  lazy: each bit as one
    innerProduct([cond, cond + 1], [t_i, f_i])."""
    checkBits([cond], trueValue, falseValue)
    if len(trueValue) != len(falseValue):
        raise _invalid("trueValue and falseValue must have the same size.")
    negated = cond.clone()
    negated.addScalar(1)
    if not _lazy(lazy):
        out = binaryMask(trueValue, cond)
        falseCopy = binaryMask(falseValue, negated)
        for o, f in zip(out, falseCopy):
            o += f
        return out
    out = []
    for t, f in zip(trueValue, falseValue):
        if isEmpty(t) or isEmpty(f) or not cond.parts:       # a zero operand: nothing to sum under one key switch
            o = _copy(t, cond)
            _multiplyBy(o, cond)
            g = _copy(f, cond)
            _multiplyBy(g, negated)
            o += g
        else:
            o = Ctxt.innerProduct([cond, negated], [t, f])
        out.append(o)
    return out


def concatBinaryNums(a, b):
    return vecCopy(a) + vecCopy(b)


def splitBinaryNums(number, leftSize):
    """-> (the low leftSize bits, the rest)"""
    if not 0 <= leftSize <= len(number):
        raise _invalid("Output sizes must sum to input.size()")
    return vecCopy(number[:leftSize]), vecCopy(number[leftSize:])


def leftBitwiseShift(number, shamt):
    if shamt < 0:
        raise _invalid("Shift amount must be positive.")
    like = ptr2nonNull(number)
    n = len(number)
    if like is None:
        return list(number)
    return [like._emptyLike() for _ in range(min(shamt, n))] + vecCopy(number[:max(n - shamt, 0)])


def bitwiseRotate(number, rotamt):
    n = len(number)
    if n == 0:
        return []
    like = ptr2nonNull(number)
    return [_copy(number[(i - rotamt) % n], like) for i in range(n)]


def bitwiseXOR(lhs, rhs):
    checkBits(lhs, rhs)
    if len(lhs) != len(rhs):
        raise _invalid("lhs and rhs must be the same size.")
    out = vecCopy(lhs)
    for o, r in zip(out, rhs):
        if r is not None:
            o += r
    return out


def bitwiseAnd(lhs, rhs):
    """rhs: a number, or a list of 0 / 1 (the mask form)"""
    checkBits(lhs)
    if len(lhs) != len(rhs):
        raise _invalid("lhs and rhs must be the same size.")
    out = vecCopy(lhs)
    if all(isinstance(x, (int, np.integer)) for x in rhs):
        for o, keep in zip(out, rhs):
            if not keep:
                o.clear()
        return out
    checkBits(rhs)
    for o, r in zip(out, rhs):
        _multiplyBy(o, r)
    return out


def bitwiseOr(lhs, rhs):
    """a OR b = a b + a + b"""
    out = bitwiseAnd(lhs, rhs)
    for o, l, r in zip(out, lhs, rhs):
        if l is not None:
            o += l
        if r is not None:
            o += r
    return out


def bitwiseNot(number):
    checkBits(number)
    out = vecCopy(number)
    for o in out:
        o.addScalar(1)
    return out


# ---- counters (src/binaryArith.cpp:1124-1342) ----
def seven4Three(bits, sizeLimit, like, lazy=None):
    """seven bits -> [c1, d1, d2], their sum in three bits (bits past sizeLimit are not computed)"""
    lazy = _lazy(lazy)
    t = lambda u, v, w: _three4TwoBits(u, v, w, like, lazy)[:2]     # noqa: E731
    b1, b2 = t(bits[0], bits[1], bits[2])
    b3, b4 = t(bits[3], bits[4], bits[5])
    c1, c2 = t(bits[6], b1, b3)
    out = [c1, c2, like._emptyLike()]
    if sizeLimit < 2:
        return out
    c3 = b2.clone()
    c3 += b4                             # b2 ^ b4
    c4 = b2.clone()
    _multiplyBy(c4, b4)                  # b2 b4
    d2 = c2.clone()
    out[1] += c3                         # d1 = c2 ^ c3
    if sizeLimit < 3:
        return out
    _multiplyBy(d2, c3)
    d2 += c4                             # d2 = c4 ^ c2 c3
    out[2] = d2
    return out


def fifteen4Four(bits, sizeLimit, like, lazy=None):
    """fifteen bits -> [d1, e1, f1, f2], their sum in four bits"""
    lazy = _lazy(lazy)
    t = lambda u, v, w: _three4TwoBits(u, v, w, like, lazy)[:2]     # noqa: E731
    out = [like._emptyLike() for _ in range(4)]
    b1, b2 = t(bits[0], bits[1], bits[2])
    b3, b4 = t(bits[3], bits[4], bits[5])
    b5, b6 = t(bits[6], bits[7], bits[8])
    c1, c2 = t(b1, b3, b5)
    c3, c4 = t(b2, b4, b6)
    b7, b8 = t(bits[9], bits[10], bits[11])
    b9, b10 = t(bits[12], bits[13], bits[14])
    out[0], d2 = t(b7, b9, c1)
    if sizeLimit < 2:
        return out
    d3, d4 = t(b8, b10, c2)
    out[1], e2 = t(c3, d2, d3)
    if sizeLimit < 3:
        return out
    e3 = c4.clone()
    e3 += d4                             # c4 ^ d4
    e4 = d4
    _multiplyBy(e4, c4)                  # c4 d4
    f1 = e2.clone()
    f1 += e3                             # e2 ^ e3
    out[2] = f1
    if sizeLimit < 4:
        return out
    _multiplyBy(e2, e3)
    e4 += e2                             # f2 = e4 ^ e2 e3
    out[3] = e4
    return out


def fifteenOrLess4Four(bits, sizeLimit=4, lazy=None):
    """up to fifteen bits (Ctxt or None) -> (four bits holding their sum, how many of them are not identically zero)"""
    checkBits(bits)
    if len(bits) > 15:
        raise _invalid("fifteenOrLess4Four takes at most 15 bits")
    like = ptr2nonNull(bits)
    if like is None:
        raise _invalid("fifteenOrLess4Four of null pointers only")
    live = [c for c in bits if c is not None]
    if len(live) > 7:
        return fifteen4Four(list(bits) + [None] * (15 - len(bits)), sizeLimit, like, lazy), 4
    live += [None] * (7 - len(live))
    if sum(c is not None for c in live) > 3:
        return seven4Three(live, sizeLimit, like, lazy) + [like._emptyLike()], 3
    lsb, msb, n = _three4TwoBits(live[0], live[1], live[2], like, _lazy(lazy))
    return [lsb, msb, like._emptyLike(), like._emptyLike()], n


# ---- encryption and decryption of bit-sliced numbers ----
def encryptBinaryNums(ea, sk, values, bitSize):
    """values: integers [B, nslots] (negative ones in two's complement) -> bitSize ciphertexts, lowest bit first"""
    v = np.atleast_2d(np.asarray(values, dtype=np.int64))
    return [ea.encrypt_batch(sk, (v >> i) & 1) for i in range(bitSize)]


def decryptBinaryNums(numbers, sk, ea, twosComplement=False, allSlots=True):
    """-> the integers [B, nslots] (src/binaryArith.cpp:1353-1377); allSlots=False: the slots of index 0 in the last
    dimension only"""
    offset = 1 if allSlots else ea.sizeOfDimension(ea.dimension() - 1)
    total = None
    for i, c in enumerate(numbers):
        if isEmpty(c):
            continue
        slots = np.asarray(ea.decrypt_batch(c, sk), dtype=np.int64)[:, ::offset] << i
        if total is None:
            total = np.zeros_like(slots)
        if twosComplement and i == len(numbers) - 1:
            total -= slots
        else:
            total += slots
    if total is None:
        total = np.zeros((1, ea.size() // offset), dtype=np.int64)
    return total
