"""helib_amd.binary_arith and helib_amd.binary_compare on the host (no GPU), over the oracle backend: the loop forms (the
oracle has no tensorSum).  m = 105, p = 2, bits = 600, c = 3: fresh capacity 589 bits, a product costs about 8 measured
bits, the planner charges 30 per level regardless, so 600 bits leaves room for 8-bit operands.  A bit is the constant
polynomial 0 or 1 (products and sums of constants are constants), so a number is one integer per run; the slot-wise runs
are in test_binary_arith_gpu.py."""
import numpy as np
import pytest

M, BITS, C_COLS = 105, 600, 3


class _Setup:
    def __init__(self, p=2, r=1, seed=3):
        from oracle import oracle as O
        from oracle.backend import OracleBackend, OracleOps, OPoly
        from helib_amd import ctxt as hc, keys as hk
        cc = self.cc = hc.ChainContext(M, p, r, bits=BITS, c=C_COLS)
        o = O.Ctx(M)
        for q in cc.primes:
            o.add_prime(q)

        class Ops(OracleOps):
            """the oracle's ops with capi.constantLike stated in python integers"""

            def constantLike(self, poly, idx, num):
                return OPoly(o, idx, np.array([[int(num) % o.primes[i]] * o.N for i in idx], dtype=np.uint64))
        be = self.be = OracleBackend(o, cc)
        be.ops = Ops(o)
        self.sk = hk.SecKey(cc, be, seed=seed)
        self.sk.GenSecKey()
        sk, phim, P = self.sk, cc.phim, p ** r

        class ConstEA:
            """one slot: the constant coefficient"""

            def size(self):
                return 1

            def encrypt_batch(self, pk, vs):
                return pk.Encrypt([int(np.asarray(vs).reshape(-1)[0]) % P] + [0] * (phim - 1))

            def decrypt_batch(self, ct, key):
                f = [int(x) % P for x in key.Decrypt(ct)]
                assert not any(f[1:]), "not a constant polynomial"
                return np.array([[f[0]]], dtype=np.int64)
        self.ea = ConstEA()
        # four fresh encryptions of each bit; numbers are put together from them (nothing below changes its inputs)
        self.pool = [[self.ea.encrypt_batch(sk, [[b]]) for _ in range(4)] for b in (0, 1)]

    def num(self, value, nbits, shift=0):
        return [self.pool[(value >> i) & 1][(i + shift) % 4] for i in range(nbits)]

    def dec(self, number, twos=False):
        from helib_amd import binary_arith as ba
        for c in number:
            assert c is None or not c.parts or c.isCorrect()
        return int(ba.decryptBinaryNums(number, self.sk, self.ea, twos)[0, 0])

    def bit(self, c):
        return self.dec([c])


@pytest.fixture(scope="module")
def s():
    return _Setup()


def _signed(v, n):
    v &= (1 << n) - 1
    return v - (1 << n) if v >> (n - 1) else v


def test_setup_capacity_and_helpers(s):
    from helib_amd import binary_arith as ba
    cap = s.pool[1][0].bitCapacity()
    assert 580 <= cap <= 600
    assert ba.longToBitVector(11, 5) == [1, 1, 0, 1, 0] and ba.longToBitVector(5, 0) == []
    with pytest.raises(ba.capi.InvalidArgument):
        ba.longToBitVector(1, -1)
    x = ba.encryptBinaryNums(s.ea, s.sk, [[-3]], 4)
    assert len(x) == 4 and s.dec(x) == 13 and s.dec(x, twos=True) == -3
    assert s.dec([]) == 0 and s.dec([None, s.pool[1][0]]) == 2
    assert ba.BPL_ESTIMATE == 30


# ---- the planner ----
def test_add_dag_levels(s):
    """Two fresh n-bit inputs of capacity C.  Sources: p(i,i) = a[i] + b[i] costs nothing (level C), q(i,i) = a[i] b[i]
    is charged 1 (level C - 1); every internal node is min(parents) - 30.
      n = 1: lowLvl = q(0,0) = C - 1.
      n = 2: q(1,0) = p(1,1) q(0,0) = min(C, C - 1) - 30 = C - 31.
      n = 3: q(2,0) = p(2,1) q(0,0) = min(C - 30, C - 1) - 30 = C - 60 (the other split, p(2,2) q(1,0), gives C - 61).
      n = 4: p(3,1) is C - 60 whichever way it is split, so q(3,0) is C - 90 through p(3,1) q(0,0) and through
             p(3,3) q(2,0), but p(3,2) q(1,0) = min(C - 30, C - 31) - 30 = C - 61."""
    from helib_amd import binary_arith as ba
    cap = min(c.bitCapacity() for row in s.pool for c in row)
    assert all(c.bitCapacity() == cap for row in s.pool for c in row)
    for n, cost in ((1, 1), (2, 31), (3, 60), (4, 61)):
        dag = ba.AddDAG(s.num(5, n), s.num(3, n))
        assert dag.lowLvl() == cap - cost, n
        assert dag.findQ(n - 1, 0).level == dag.lowLvl()
    dag = ba.AddDAG(s.num(5, 4), s.num(3, 4))
    assert (dag.findQ(3, 0).parent1.idx, dag.findQ(3, 0).parent2.idx) == ((1, 0), (3, 2))
    assert dag.findP(3, 1).level == cap - 60 and dag.findP(1, 0).level == cap - 30 and dag.findQ(2, 2).level == cap - 1
    assert ba.defaultPmiddle(5) == 4 and ba.defaultQmiddle(5) == 4 and ba.defaultQmiddle(4) == 2


def test_add_dag_shape(s):
    from helib_amd import binary_arith as ba
    for aSize, bSize in ((2, 5), (3, 3), (1, 4), (6, 7)):
        dag = ba.AddDAG(s.num(1, bSize), s.num(1, aSize))       # the shorter one plays a whichever side it is on
        assert (dag.aSize, dag.bSize) == (aSize, bSize)
        for i in range(bSize):
            for j in range(i + 1):
                assert dag.findP(i, j) is not None
                assert (dag.findQ(i, j) is not None) == (j < aSize), (i, j)
        for table, first in ((dag.p, False), (dag.q, True)):
            for (i, j), node in table.items():
                assert node.isQ == first and node.idx == (i, j)
                if i == j:
                    assert node.parent1 is None and node.parent2 is None
                    continue
                # the span j..i is the disjoint union of the parents': parent1 the low part (a q for a q), parent2 a p
                (i1, j1), (i2, j2) = node.parent1.idx, node.parent2.idx
                assert j1 == j and i2 == i and j2 == i1 + 1 and j <= i1 < i
                assert node.parent1.isQ == first and not node.parent2.isQ
                assert node.level == min(node.parent1.level, node.parent2.level) - 30
    with pytest.raises(ba.capi.InvalidArgument, match="must not be empty"):
        ba.AddDAG([], s.num(1, 2))


# ---- addition ----
def test_add_two_numbers_all_pairs_of_2_and_3_bits(s):
    from helib_amd import binary_arith as ba
    for a in range(4):
        for b in range(8):
            x, y = s.num(a, 2), s.num(b, 3, shift=1)
            got = ba.addTwoNumbers(x, y) if (a + b) & 1 else ba.addTwoNumbers(y, x)
            assert len(got) == 4 and s.dec(got) == a + b, (a, b)
    assert s.dec(s.num(3, 2)) == 3 and s.dec(s.num(5, 3, shift=1)) == 5        # the inputs are as they were


def test_add_two_numbers_5_bits_size_limits_and_holes(s):
    from helib_amd import binary_arith as ba
    rng = np.random.default_rng(7)
    for a, b in [(31, 31), (0, 0), (21, 10)] + [tuple(int(v) for v in rng.integers(0, 32, 2)) for _ in range(3)]:
        got = ba.addTwoNumbers(s.num(a, 5), s.num(b, 5, shift=2))
        assert len(got) == 6 and s.dec(got) == a + b, (a, b)
        assert min(c.bitCapacity() for c in got if c.parts) > 400
    x, y = s.num(13, 4), s.num(7, 3)
    for limit, size in ((2, 2), (4, 4), (5, 5), (7, 7), (0, 5)):
        got = ba.addTwoNumbers(x, y, limit)
        assert len(got) == size and s.dec(got) == 20 % (1 << size), limit
    # an empty side: the other one, cut to the limit
    assert s.dec(ba.addTwoNumbers([], x)) == 13 and s.dec(ba.addTwoNumbers(x, [])) == 13
    assert s.dec(ba.addTwoNumbers([], x, 2)) == 1 and ba.addTwoNumbers([], []) == []
    # a null pointer and an empty ciphertext are zero bits
    empty = s.pool[0][0]._emptyLike()
    assert not empty.parts
    holes = [s.pool[1][0], None, empty, s.pool[1][1]]           # 9
    assert s.dec(ba.addTwoNumbers(holes, x)) == 22 and s.dec(ba.addTwoNumbers(y, holes)) == 16
    dag = ba.AddDAG(holes, x)
    assert dag.findQ(1, 1).level == ba.LONG_MAX and dag.findP(1, 1).level == s.pool[1][0].bitCapacity()


def test_add_many_numbers(s):
    from helib_amd import binary_arith as ba
    cases = [[(5, 3), (2, 2), (7, 4)], [(1, 1), (6, 3), (3, 2), (9, 4)],
             [(3, 2), (1, 1), (7, 3), (2, 2), (15, 4), (0, 1), (5, 3)]]
    for case in cases:
        numbers = [s.num(v, n, shift=k) for k, (v, n) in enumerate(case)]
        total = ba.addManyNumbers(numbers)
        assert s.dec(total) == sum(v for v, _ in case), case
    numbers = [s.num(v, n) for v, n in cases[2]]
    assert s.dec(ba.addManyNumbers(numbers, 3)) == sum(v for v, _ in cases[2]) % 8
    assert ba.addManyNumbers([]) == [] and ba.addManyNumbers([[None], [None]]) == []
    assert s.dec(ba.addManyNumbers([s.num(6, 3)])) == 6
    # the 3-for-2 step alone, numbers and bits
    lsb, msb = ba.three4Two(s.num(5, 3), s.num(3, 2), s.num(7, 3))
    assert s.dec(lsb) + s.dec(msb) == 15 and not msb[0].parts
    for u in range(8):
        bits = [s.pool[(u >> k) & 1][k] if u != 5 or k else None for k in range(3)]
        lo, hi, n = ba.three4Two(*bits)
        want = bin(u).count("1") - (1 if u == 5 else 0)
        assert s.bit(lo) + 2 * s.bit(hi) == want and n == min(sum(b is not None for b in bits), 2)


# ---- products ----
def test_mult_two_numbers(s):
    from helib_amd import binary_arith as ba
    rng = np.random.default_rng(11)
    pairs = [(7, 7), (0, 5), (5, 6)] + [tuple(int(v) for v in rng.integers(0, 8, 2)) for _ in range(2)]
    for a, b in pairs:
        got = ba.multTwoNumbers(s.num(a, 3), s.num(b, 3, shift=1))
        assert len(got) == 6 and s.dec(got) == a * b, (a, b)
        assert min(c.bitCapacity() for c in got if c.parts) > 300
    for a, b in [(7, 4), (7, 7), (3, 5), (5, 1), (0, 6)]:          # rhs in two's complement: 4 is -4, 7 is -1, 5 is -3
        got = ba.multTwoNumbers(s.num(a, 3), s.num(b, 3, shift=1), rhsTwosComplement=True)
        assert len(got) == 6 and s.dec(got, twos=True) == a * _signed(b, 3), (a, b)
    # a product of unequal sizes, either way round, and one cut by sizeLimit
    assert s.dec(ba.multTwoNumbers(s.num(13, 4), s.num(3, 2))) == 39
    assert s.dec(ba.multTwoNumbers(s.num(3, 2), s.num(13, 4))) == 39
    got = ba.multTwoNumbers(s.num(7, 3), s.num(6, 3), sizeLimit=4)
    assert len(got) == 4 and s.dec(got) == 42 % 16
    # one-bit operands on either side
    for bit in (0, 1):
        left = ba.multTwoNumbers(s.num(bit, 1), s.num(5, 3))
        right = ba.multTwoNumbers(s.num(5, 3), s.num(bit, 1))
        assert len(left) == 3 and len(right) == 3 and s.dec(left) == 5 * bit == s.dec(right)
    assert s.dec(ba.multTwoNumbers(s.num(1, 1), s.num(6, 3), rhsTwosComplement=True), twos=True) == -2
    empty = s.pool[0][0]._emptyLike()
    assert ba.multTwoNumbers([empty], s.num(5, 3)) == [] and ba.multTwoNumbers(s.num(5, 3), [empty]) == []
    assert ba.multTwoNumbers([None, None], s.num(5, 3)) == []
    assert s.dec(s.num(5, 3)) == 5


def test_negate_and_subtract_all_3_bit_values(s):
    from helib_amd import binary_arith as ba
    for a in range(8):
        got = ba.negateBinary(s.num(a, 3))
        assert len(got) == 3 and s.dec(got) == (-a) % 8 and s.dec(got, twos=True) == _signed(-a, 3)
    for a in range(8):
        for b in (a, (a + 3) % 8, 7 - a):
            got = ba.subtractBinary(s.num(a, 3), s.num(b, 3, shift=1))
            assert len(got) == 3 and s.dec(got) == (a - b) % 8, (a, b)
    with pytest.raises(ba.capi.InvalidArgument):
        ba.subtractBinary(s.num(1, 3), s.num(1, 2))


def test_bitwise_cond_shift_rotate_concat_split(s):
    from helib_amd import binary_arith as ba
    a, b, n = 0b1100, 0b1010, 4
    x, y = s.num(a, n), s.num(b, n, shift=1)
    assert s.dec(ba.bitwiseXOR(x, y)) == a ^ b and s.dec(ba.bitwiseAnd(x, y)) == a & b
    assert s.dec(ba.bitwiseOr(x, y)) == a | b and s.dec(ba.bitwiseNot(x)) == ~a & 15
    assert s.dec(ba.bitwiseAnd(x, [1, 0, 1, 1])) == a & 0b1101 and s.dec(ba.bitwiseAnd(x, [0, 0, 0, 0])) == 0
    for bit in (0, 1):
        mask = s.pool[bit][3]
        assert s.dec(ba.binaryMask(x, mask)) == a * bit
        assert s.dec(ba.binaryCond(mask, x, y)) == (a if bit else b)
    for k in range(6):
        assert s.dec(ba.leftBitwiseShift(x, k)) == (a << k) & 15
    for k in (-5, -1, 0, 1, 2, 3, 4, 7):
        r = k % n
        assert s.dec(ba.bitwiseRotate(x, k)) == ((a << r) | (a >> (n - r))) & 15, k
    both = ba.concatBinaryNums(x, s.num(5, 3))
    assert len(both) == 7 and s.dec(both) == a + (5 << 4)
    low, high = ba.splitBinaryNums(both, 2)
    assert (len(low), len(high)) == (2, 5) and s.dec(low) == both_value(a, 5) % 4 and s.dec(high) == both_value(a, 5) >> 2
    assert s.dec(x) == a and s.dec(y) == b
    with pytest.raises(ba.capi.InvalidArgument):
        ba.bitwiseXOR(x, y[:3])
    with pytest.raises(ba.capi.InvalidArgument):
        ba.leftBitwiseShift(x, -1)


def both_value(a, hi):
    return a + (hi << 4)


@pytest.mark.parametrize("count", [1, 3, 7, 8, 15])
def test_fifteen_or_less_4_four_against_popcount(s, count):
    from helib_amd import binary_arith as ba
    rng = np.random.default_rng(count)
    for trial in range(2):
        bits = [1] * count if trial == 0 else [int(v) for v in rng.integers(0, 2, count)]
        ins = [s.pool[b][k % 4] for k, b in enumerate(bits)]
        if count == 8:                   # null pointers among fifteen
            ins = ins[:3] + [None] * 4 + ins[3:] + [None] * 3
        out, n = ba.fifteenOrLess4Four(ins)
        assert len(out) == 4 and s.dec(out) == sum(bits), bits
        assert n == (4 if count > 7 else 3 if count > 3 else min(count, 2))
    if count == 15:
        out, _ = ba.fifteenOrLess4Four([s.pool[1][k % 4] for k in range(15)], sizeLimit=2)
        assert s.dec(out[:2]) == 15 % 4
        with pytest.raises(ba.capi.InvalidArgument):
            ba.fifteenOrLess4Four([s.pool[1][0]] * 16)


# ---- comparison ----
@pytest.mark.parametrize("twos", [False, True])
def test_compare_all_pairs_of_3_bit_values(s, twos):
    from helib_amd import binary_compare as bc
    for a in range(8):
        for b in range(8):
            va, vb = (_signed(a, 3), _signed(b, 3)) if twos else (a, b)
            mx, mn, mu, ni = bc.compareTwoNumbers(s.num(a, 3), s.num(b, 3, shift=1), twosComplement=twos)
            got = (s.dec(mx, twos), s.dec(mn, twos), s.bit(mu), s.bit(ni))
            assert got == (max(va, vb), min(va, vb), int(va > vb), int(va < vb)), (a, b)
    assert s.dec(s.num(5, 3)) == 5


def test_compare_unequal_sizes_cmp_only_and_empty(s):
    from helib_amd import binary_arith as ba, binary_compare as bc
    for a, b in [(3, 9), (3, 2), (2, 18), (3, 3), (0, 31)]:
        mx, mn, mu, ni = bc.compareTwoNumbers(s.num(a, 2), s.num(b, 5))
        assert (len(mx), len(mn)) == (5, 2)
        assert (s.dec(mx), s.dec(mn), s.bit(mu), s.bit(ni)) == (max(a, b), min(a, b), int(a > b), int(a < b)), (a, b)
        # the longer operand plays b whichever side it is on: mu then says b > a in the caller's names
        mx, mn, mu, ni = bc.compareTwoNumbers(s.num(b, 5), s.num(a, 2))
        assert (s.dec(mx), s.dec(mn), s.bit(mu), s.bit(ni)) == (max(a, b), min(a, b), int(a > b), int(a < b)), (a, b)
        mu, ni = bc.compareTwoNumbers(s.num(a, 2), s.num(b, 5), cmp_only=True)
        assert (s.bit(mu), s.bit(ni)) == (int(a > b), int(a < b))
    mx, mn, mu, ni = bc.compareTwoNumbers([], s.num(6, 3))
    assert s.dec(mx) == 6 and mn == [] and not mu.parts and s.bit(ni) == 1
    mu, ni = bc.compareTwoNumbers(s.num(6, 3), [], cmp_only=True)
    assert not mu.parts and s.bit(ni) == 1
    v = [s.pool[1][0].clone(), s.pool[0][0].clone(), s.pool[1][1].clone()]
    bc.runningSums(v)
    assert [s.bit(c) for c in v] == [0, 1, 1]
    assert ba.findMinBitCapacity(v, [None]) == min(c.bitCapacity() for c in v)


# ---- the one-relinearisation forms ----
def test_lazy_forms_decrypt_alike(s, monkeypatch):
    from helib_amd import binary_arith as ba
    from helib_amd.ctxt import Ctxt
    calls = []
    real = Ctxt.innerProduct
    monkeypatch.setattr(Ctxt, "innerProduct", staticmethod(lambda *a, **k: (calls.append(len(a[0])), real(*a, **k))[1]))
    for u in range(8):
        bits = [s.pool[(u >> k) & 1][k] for k in range(3)]
        lo, hi, _ = ba.three4Two(*bits, lazy=True)
        assert lo.isCorrect() and hi.isCorrect() and s.bit(lo) + 2 * s.bit(hi) == bin(u).count("1")
    assert calls == [2] * 8
    ref = ba.three4Two(*[s.pool[1][k] for k in range(3)], lazy=False)[1]
    assert len(calls) == 8 and abs(ref.bitCapacity() - hi.bitCapacity()) <= 2
    x, y = s.num(5, 3), s.num(2, 3, shift=1)
    for bit in (0, 1):
        got = ba.binaryCond(s.pool[bit][3], x, y, lazy=True)
        assert s.dec(got) == (5 if bit else 2)
    assert len(calls) == 8 + 6
    got = ba.multTwoNumbers(s.num(7, 3), s.num(5, 3, shift=1), lazy=True)
    assert s.dec(got) == 35 and len(calls) > 14
    n = len(calls)
    monkeypatch.setattr(ba, "lazyCarry", True)                    # the module flag is what lazy=None follows
    assert s.dec(ba.addManyNumbers([s.num(3, 2), s.num(3, 2, shift=1), s.num(3, 2, shift=2)])) == 9
    assert len(calls) > n
    with pytest.raises(RuntimeError, match="no tensorSum"):
        real([s.pool[1][0]] * 2, [s.pool[1][1]] * 2, fused=True)
    same = real([s.pool[1][0], s.pool[1][2]], [s.pool[1][1], s.pool[0][3]])      # 1 * 1 + 1 * 0
    assert s.bit(same) == 1


def test_inner_product_fused_bookkeeping_over_a_stated_tensor_sum():
    """Ctxt.innerProduct(fused=True) over the oracle's ops with tensorSum stated as the calls it replaces: the kernel path
    is taken once for pairs on one level and not at all for mixed levels, and words and bookkeeping are the loop's"""
    from helib_amd.ctxt import Ctxt
    t = _Setup(seed=4)
    hits = []

    class Ops(type(t.be.ops)):
        def tensorSum(self, a0, a1, b0, b1):
            hits.append(len(a0))
            acc = self.tensorProduct(a0[0], a1[0], b0[0], b1[0])
            for k in range(1, len(a0)):
                for x, y in zip(acc, self.tensorProduct(a0[k], a1[k], b0[k], b1[k])):
                    x += y
            return tuple(acc)
    ops = Ops(t.be.o)
    x = [c.clone() for c in t.pool[1] + t.pool[0]]
    for c in x:
        c.ops = ops

    def state(ct):
        return ({h: (list(p.idx), p.rows.tolist()) for h, p in ct.parts.items()}, ct.lnNoise, ct.primeSet, ct.ptxtSpace,
                ct.intFactor, ct.ptxtMag)
    v1, v2 = [x[0], x[1], x[4]], [x[2], x[1], x[3]]              # 1 * 1 + 1 * 1 + 0 * 1, the middle pair a square
    loop = Ctxt.innerProduct(v1, v2, fused=False)
    assert not hits and state(Ctxt.innerProduct(v1, v2)) == state(loop) and not hits
    fused = Ctxt.innerProduct(v1, v2, fused=True)
    assert hits == [3] and state(fused) == state(loop) and set(fused.parts) == {"1", "s"}
    assert t.bit(fused) == 0 and fused.isCorrect()
    p1, p2 = x[0].clone(), x[2].clone()
    p1.multiplyBy(x[1])
    p2.multiplyBy(x[3])
    del hits[:]
    loop = Ctxt.innerProduct([x[0], p1], [x[5], p2], fused=False)
    fused = Ctxt.innerProduct([x[0], p1], [x[5], p2], fused=True)
    assert not hits and state(fused) == state(loop) and t.bit(fused) == 1
    one = Ctxt.innerProduct([x[0]], [x[1]], fused=True)          # a single pair: nothing to sum, the loop
    assert not hits and t.bit(one) == 1
    with pytest.raises(ValueError):
        Ctxt.innerProduct([], [], fused=True)


# ---- refusals ----
@pytest.fixture(scope="module")
def ground(s):
    """an encryption of 1 squared until the planner's estimate for two bits falls below 30: capacity below 60"""
    g = s.pool[1][0].clone()
    n = 0
    while g.bitCapacity() >= 60:
        g.multiplyBy(g.clone())
        n += 1
    assert n > 30 and g.isCorrect() and s.bit(g) == 1
    return g


def test_level_errors(s, ground):
    from helib_amd import binary_arith as ba, binary_compare as bc
    from helib_amd.ckks import LogicError
    low = [ground, ground]
    assert ba.AddDAG(low, s.num(3, 2)).lowLvl() == ground.bitCapacity() - 31 < 30
    with pytest.raises(LogicError, match="not enough levels for addition DAG"):
        ba.addTwoNumbers(low, s.num(3, 2))
    with pytest.raises(LogicError, match="not enough levels for comparison"):
        bc.compareTwoNumbers(low, s.num(3, 2))
    with pytest.raises(ba.capi.InvalidArgument, match="unpackSlotEncoding must not be null"):
        ba.addManyNumbers([list(low), s.num(3, 2), s.num(1, 2)])
    # one bit is still within reach: lowLvl = capacity - 1
    if ground.bitCapacity() > 30:
        assert s.dec(ba.addTwoNumbers([ground], s.num(1, 1))) == 2


def test_other_plaintext_spaces_are_refused():
    from helib_amd import binary_arith as ba, binary_compare as bc
    t = _Setup(p=2, r=2)
    x = [t.pool[1][0], t.pool[0][0]]
    assert x[0].ptxtSpace == 4
    for call in (lambda: ba.addTwoNumbers(x, x), lambda: ba.multTwoNumbers(x, x), lambda: ba.bitwiseNot(x),
                 lambda: ba.addManyNumbers([x, x, x]), lambda: bc.compareTwoNumbers(x, x),
                 lambda: ba.binaryCond(x[0], x, x), lambda: ba.three4Two(x[0], x[0], x[1])):
        with pytest.raises(ba.capi.InvalidArgument, match="plaintext space 2"):
            call()
