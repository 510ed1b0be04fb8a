"""helib_amd.table_lookup on the host (no GPU), over the oracle backend: the default form and the lazy form through plain
ops (the oracle has neither mulAddMany nor tensorSum).  The setting is test_binary_arith_host.py's: m = 105, p = 2,
bits = 600, an index bit is the constant polynomial 0 or 1.  A table entry is any polynomial with 0 / 1 coefficients (the
"slots" of the stand-in EncryptedArray are the coefficients themselves), so a lookup decrypts to a whole polynomial.

Capacity left (printed by test_capacity_left_by_both_forms; fresh bits have 589): after a 3-bit lookup 565 bits in the
default form and 565 in the lazy one, after a 5-bit lookup 555 and 554: the lazy form relinearises a sum whose noise
bound is the sum of the pairs' bounds, which costs it at most a bit here, and saves 7 and 31 key switches."""
import math

import numpy as np
import pytest

from tests import table_lookup_ref as R
from tests import test_binary_arith_host as BAH


class _Batch:
    """what a batched encode returns over the oracle: one poly per table entry"""

    def __init__(self, items):
        self.items, self.batch = items, len(items)


class _PolyEA:
    """the table side of an EncryptedArray whose slots are the phi(m) coefficients: encodeCoeffs is the identity"""

    def __init__(self, s):
        self.cc, be = s.cc, s.be
        phim = s.cc.phim
        outer = self
        self.encodes = []

        class Enc:
            def encode(self, v, mul, idx, coeffs=False):
                v = np.atleast_2d(v)
                outer.encodes.append((v.shape[0], tuple(idx)))
                assert mul == 1
                d = _Batch([be.fromCoeffs(list(idx), [int(x) for x in row]) for row in v]) if idx else None
                return (d, v) if coeffs else d

            def split(self, poly):
                return list(poly.items)

            def norm(self, coeffs):
                return np.array([be.embeddingLargestCoeff([float(x) for x in row]) for row in np.atleast_2d(coeffs)])
        self.enc = Enc()
        self.phim = phim

    def size(self):
        return self.phim

    def getDegree(self):
        return 1

    def _slots(self, v):
        v = np.asarray(v, dtype=np.int64)
        assert v.ndim == 2 and v.shape[1] == self.phim
        return v

    def encodeCoeffs(self, v):
        return self._slots(v)


@pytest.fixture(scope="module")
def s():
    return BAH._Setup()


@pytest.fixture(scope="module")
def pea(s):
    return _PolyEA(s)


def _table(s, size, seed):
    t = np.random.default_rng(seed).integers(0, 2, size=(size, s.cc.phim))
    t[0] = 0                                             # an all-zero entry: size 0, a product that vanishes
    t[size - 1] = 1
    return t


def _poly(s, ct):
    assert ct.isCorrect()
    return np.array([int(x) % 2 for x in s.sk.Decrypt(ct)])


# ---- the split ----
def test_split_rule_against_the_hand_derived_table():
    from helib_amd import table_lookup as tl
    assert {n: tl.splitSizes(n) for n in range(1, 17)} == R.SPLIT
    assert R.SPLIT[3] == (4, 2) and R.SPLIT[4] == (4, 4) and R.SPLIT[5] == (16, 2) and R.SPLIT[8] == (16, 16)
    assert R.SPLIT[9] == (256, 2) and R.SPLIT[16] == (256, 256)
    assert all(k * l == 1 << n for n, (k, l) in R.SPLIT.items())


# ---- computeAllProducts ----
@pytest.mark.parametrize("nBits,size", [(1, None), (2, None), (3, None), (5, None), (2, 3), (3, 5), (3, 7)])
def test_compute_all_products_are_the_indicators(s, nBits, size):
    """product j decrypts to [index == j] for every index; a ragged size forms only the first `size` of them"""
    from helib_amd import table_lookup as tl
    n = size or 1 << nBits
    for index in range(1 << nBits):
        bits = s.num(index, nBits, shift=index)
        before = [c.lnNoise for c in bits]
        products = tl.computeAllProducts(bits, size)
        assert len(products) == n
        got = [s.bit(c) for c in products]
        assert got == [int(j == index) for j in range(n)], (index, got)
        assert [c.lnNoise for c in bits] == before and s.dec(bits) == index       # the inputs are as they were


def test_compute_all_products_sizes_and_extra_bits(s):
    from helib_amd import table_lookup as tl
    bits = s.num(5, 4)
    assert tl.computeAllProducts([], None) == []
    out = tl.computeAllProducts(bits, 4)                 # NumBits(3) = 2: the two high bits are ignored
    assert len(out) == 4 and [s.bit(c) for c in out] == [0, 1, 0, 0]
    out = tl.computeAllProducts(bits[:1], 4)             # one bit, four outputs: the last two stay empty
    assert [bool(c.parts) for c in out] == [True, True, False, False] and [s.bit(c) for c in out[:2]] == [0, 1]
    with pytest.raises(tl.capi.InvalidArgument, match="2\\^16"):
        tl.computeAllProducts(s.num(0, 17))


def _counting(monkeypatch):
    from helib_amd.ctxt import Ctxt
    seen = {"multiplyBy": 0, "reLinearize": 0}
    for name in seen:
        real = getattr(Ctxt, name)

        def wrap(self, *a, _real=real, _name=name, **kw):
            seen[_name] += 1
            return _real(self, *a, **kw)
        monkeypatch.setattr(Ctxt, name, wrap)
    return seen


@pytest.mark.parametrize("nBits", [3, 5])
def test_multiplication_counts(s, pea, monkeypatch, nBits):
    """default: one multiplyBy per product of every level (1 + 8 at 3 bits, 1 + 1 + 16 + 32 at 5), each with its own
    relinearisation; lazy: the last level is ONE relinearisation (1 + 1 and 1 + 1 + 16 + 1)"""
    from helib_amd import table_lookup as tl
    total, last = R.counts(nBits)
    assert (total, last) == {3: (9, 8), 5: (50, 32)}[nBits]
    table = tl.LookupTable.fromSlots(pea, _table(s, 1 << nBits, nBits))
    bits = s.num(5, nBits)
    seen = _counting(monkeypatch)
    tl.tableLookup(pea, table, bits, lazy=False)
    assert seen == {"multiplyBy": total, "reLinearize": total}
    seen.update(multiplyBy=0, reLinearize=0)
    tl.tableLookup(pea, table, bits, lazy=True)
    assert seen == {"multiplyBy": total - last, "reLinearize": total - last + 1}


# ---- buildLookupTable ----
def test_build_lookup_table_against_direct_evaluation():
    """f = 1 / (x + 1) with the reference test's parameters (scale_out = 1 - nbits_out), unsigned and signed inputs:
    x = -1 is an infinity (saturation at the top), signed outputs saturate at both ends, and a NaN gives 0"""
    from tests import bgv_gr_tables as GR
    from helib_amd import intraslot, table_lookup as tl
    g = GR.Setup(85, 2, 1, gf=True)
    ea = g.ea
    assert ea.getDegree() == 8 and ea.size() == 8

    def f(x):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.float64(1.0) / np.float64(x + 1.0))
    for nbits_in, sign_in, nbits_out, sign_out in ((4, 0, 8, 0), (4, 1, 8, 0), (3, 1, 5, 1)):
        want = R.table_values(f, nbits_in, 0, sign_in, nbits_out, 1 - nbits_out, sign_out)
        assert tl.tableValues(f, nbits_in, 0, sign_in, nbits_out, 1 - nbits_out, sign_out) == want
        if not sign_in:
            assert want[:4] == [2 ** (nbits_out - 1), 2 ** (nbits_out - 2), round(2 ** (nbits_out - 1) / 3), 2 ** (nbits_out - 3)]
        else:
            assert want[(1 << nbits_in) - 1] == ((1 << (nbits_out - 1)) - 1 if sign_out else (1 << nbits_out) - 1)    # x = -1
        T = tl.buildLookupTable(ea, f, nbits_in, 0, sign_in, nbits_out, 1 - nbits_out, sign_out)
        assert len(T) == 1 << nbits_in and T.zzX.shape == (1 << nbits_in, g.cc.phim) and T.ptxtSpace == 2
        for i, v in enumerate(want):
            assert np.array_equal(T.zzX[i], intraslot.packConstant(ea, v, nbits_out)[0]), i
            assert intraslot.unpackSlots(ea, T.slots[i:i + 1]) == [v] * ea.size()
        assert T.sizes == [float(x) for x in g.enc.norm(T.zzX)]

    # both ends and a NaN: g(x) = -x below 2, NaN at 2, +x above, 3 bits in and 3 signed bits out at scale 0
    def gfun(x):
        return math.nan if x == 2 else (-x if x < 2 else x)
    want = R.table_values(gfun, 3, 0, 0, 3, 0, 1)
    assert want == [0, 7, 0, 3, 3, 3, 3, 3] and tl.tableValues(gfun, 3, 0, 0, 3, 0, 1) == want
    assert R.table_values(lambda x: -8.0 * x, 3, 0, 0, 3, 0, 1)[1] == 4                  # -8 -> the smallest value, -4
    assert tl.tableValues(lambda x: -8.0 * x, 3, 0, 0, 3, 0, 1) == R.table_values(lambda x: -8.0 * x, 3, 0, 0, 3, 0, 1)
    assert tl.tableValues(lambda x: x + 0.5, 2, 0, 0, 3, 0, 0) == [1, 2, 3, 4]           # halves round away from zero
    with pytest.raises(tl.capi.InvalidArgument):
        tl.buildLookupTable(ea, f, 17, 0, 0, 8, 0, 0)


# ---- tableLookup ----
def _lazy_probe(monkeypatch):
    """the lazy form's operands (the last _halves call) and the state its sum has when reLinearize takes it"""
    from helib_amd import table_lookup as tl
    from helib_amd.ctxt import Ctxt
    got = {}
    real_halves, real_relin = tl._halves, Ctxt.reLinearize

    def halves(*a):
        got["halves"] = real_halves(*a)
        return got["halves"]

    def relin(self):
        if set(self.parts) == {"1", "s", "s2"} and self._pendT is None:
            got["sum"] = (self.lnNoise, self.ptxtMag, self.primeSet, self.ptxtSpace, self.intFactor)
        return real_relin(self)
    monkeypatch.setattr(tl, "_halves", halves)
    monkeypatch.setattr(Ctxt, "reLinearize", relin)
    return got


@pytest.mark.parametrize("nBits,size", [(3, 8), (5, 32), (3, 6)])
def test_table_lookup_default_and_lazy_for_every_index(s, pea, monkeypatch, nBits, size):
    """both forms give the entry at the index and a correct ciphertext; the lazy sum's bookkeeping is the restatement's;
    one batched encode per prime set serves every lookup"""
    from helib_amd import table_lookup as tl
    t = _table(s, size, 7 * nBits)
    table = tl.LookupTable.fromSlots(pea, t)
    assert len(table) == size and table.sizes[0] == 0.0
    del pea.encodes[:]
    got = _lazy_probe(monkeypatch)
    for index in range(size):
        bits = s.num(index, nBits, shift=index)
        ref = tl.tableLookup(pea, table, bits, lazy=False)
        assert np.array_equal(_poly(s, ref), t[index]), index
        got.clear()
        lazy = tl.tableLookup(pea, t if index == 1 else table, bits, lazy=True)     # (a bare array is a table too)
        assert np.array_equal(_poly(s, lazy), t[index]), index
        A, Bs, k, _ = got["halves"]
        assert (k, len(A)) == (R.SPLIT[nBits][0],) * 2
        ln, mag = R.lazy_bookkeeping([c.lnNoise for c in A], [c.lnNoise for c in Bs], [c.ptxtMag for c in A],
                                     table.sizes, k, size)
        assert got["sum"][0] == pytest.approx(ln, rel=1e-12) and got["sum"][1] == pytest.approx(mag, rel=1e-12)
        assert got["sum"][2] == A[0].primeSet and all(c.primeSet == A[0].primeSet for c in A + Bs)
        assert got["sum"][3:] == (2, 1) and lazy.ptxtSpace == 2
        assert s.dec(bits) == index
    batched = [e for e in pea.encodes if e[1]]
    assert all(n == size for n, _ in batched)
    assert len(batched) == len({e[1] for e in batched}) + 1      # once per prime set (+ the bare array of index 1)
    for flag in (True, False):                           # lazy=None follows the module flag
        monkeypatch.setattr(tl, "lazyLookup", flag)
        got.clear()
        assert np.array_equal(_poly(s, tl.tableLookup(pea, table, s.num(2, nBits))), t[2]) and ("sum" in got) == flag
    with pytest.raises(RuntimeError, match="no tableTensorSum"):
        tl.tableLookup(pea, table, s.num(2, nBits), fused=True)


def test_table_lookup_short_index_and_long_table(s, pea, monkeypatch):
    """2 bits: the lazy form does not apply and the default runs; a table of 11 entries under a 3-bit index uses 8"""
    from helib_amd import table_lookup as tl
    t = _table(s, 11, 3)
    got = _lazy_probe(monkeypatch)
    for index in (0, 3):
        assert np.array_equal(_poly(s, tl.tableLookup(pea, t[:4], s.num(index, 2), lazy=True)), t[index])
    assert "sum" not in got
    for index in (0, 7):
        assert np.array_equal(_poly(s, tl.tableLookup(pea, t, s.num(index, 3), lazy=False)), t[index])
        assert np.array_equal(_poly(s, tl.tableLookup(pea, t, s.num(index, 3), lazy=True)), t[index])


def test_capacity_left_by_both_forms(s, pea, capsys):
    """printed, not asserted against each other (the figures are in the module docstring): both are correct"""
    from helib_amd import table_lookup as tl
    for nBits in (3, 5):
        table = tl.LookupTable.fromSlots(pea, _table(s, 1 << nBits, nBits))
        bits = s.num(5, nBits)
        ref, lazy = tl.tableLookup(pea, table, bits, lazy=False), tl.tableLookup(pea, table, bits, lazy=True)
        with capsys.disabled():
            print("\ntable lookup, %d bits: fresh %d, default form %d, lazy form %d bits of capacity"
                  % (nBits, bits[0].bitCapacity(), ref.bitCapacity(), lazy.bitCapacity()))
        assert ref.isCorrect() and lazy.isCorrect() and ref.bitCapacity() > 0 and lazy.bitCapacity() > 0


# ---- tableWriteIn ----
def test_table_write_in_random_increments(s):
    """the reference's test (tests/GTestTableLookup.cpp:324-361): the first bitSize entries encrypt random bits, the rest
    are empty; after random write-ins the table equals the plaintext one mod p"""
    from helib_amd import table_lookup as tl
    rng = np.random.default_rng(11)
    nBits, size = 3, 8
    like = s.pool[0][0]
    pT = [0] * size
    T = [like._emptyLike() for _ in range(size)]
    for i in range(nBits):
        pT[i] = int(rng.integers(0, 2))
        T[i] = s.pool[pT[i]][i].clone()
    held = list(T)
    for _ in range(10):
        index = int(rng.integers(0, size))
        assert tl.tableWriteIn(T, s.num(index, nBits, shift=index)) is T
        pT[index] += 1
    assert all(a is b for a, b in zip(T, held))          # in place on the list's ciphertexts
    assert [s.bit(c) for c in T] == [v % 2 for v in pT]
    assert tl.tableWriteIn([], s.num(1, 2)) == []


# ---- the level check ----
def test_not_enough_levels_raises_logic_error(s, pea):
    from helib_amd import table_lookup as tl
    from helib_amd.ckks import LogicError
    used = s.pool[1][0].clone()
    used.bringToSet(frozenset(list(s.cc.ctxtPrimes)[:1]))
    bits = [s.pool[1][1], used, s.pool[0][2]]
    need = (tl.NumBits(3) + 1) * 30
    assert 0 < used.bitCapacity() < need == 90
    for call in (lambda: tl.computeAllProducts(bits), lambda: tl.tableLookup(pea, _table(s, 8, 1), bits),
                 lambda: tl.tableLookup(pea, _table(s, 8, 1), bits, lazy=True),
                 lambda: tl.tableWriteIn([s.pool[0][0].clone() for _ in range(8)], bits)):
        with pytest.raises(LogicError, match="not enough levels for table lookup"):
            call()
    assert len(tl.computeAllProducts(bits[:1] + bits[2:])) == 4          # without the used-up bit there is room
