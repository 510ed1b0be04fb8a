"""hx_tensor_sum, Ctxt.innerProduct(fused=True) and the circuits of helib_amd.binary_arith / binary_compare on the device.
Everything here is an integer: every comparison is exact.

Chain size of the slot runs (m = 85, p = 2, c = 2, 8 slots): bits = 200, the smallest multiple of 100 at which the
reference-order runs keep every output correct (found with the oracle backend on the CPU: at 100 a fresh ciphertext has
93 bits, the 4 + 4 bit sum keeps 68 and the 3 x 3 bit product stops in addManyNumbers below 3 BPL = 90; at 200 fresh is
200 and the capacities left are 175 for the sum and the difference, 163 and 158 for the unsigned and the two's-complement
product, 165 for the comparison, 190 for the conditional and 179 for the 7-bit counter)."""
import ctypes as C

import numpy as np
import pytest

from helib_amd import hostnt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hx():
    try:
        import torch  # noqa: F401   (before this library touches the device: see test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import capi
    if capi.device_count() <= 0:
        pytest.skip("no HIP device: the GPU tests run on an MI355X (pytest -m gpu)")
    return capi


# ---- (a), (b) hx_tensor_sum against python integers and against the calls it replaces ----
TS_M, TS_N = 1031, 1030                  # phi(1031) = 1030: 515 two-word vectors, three workgroup columns
TS_WIDTHS = (60, 56, 45, 38, 60, 60)
TS_IDX = [5, 2, 0, 3, 1]                 # the output rows: five of the six primes, all four widths, in another order


@pytest.fixture(scope="module")
def ts_ring(hx):
    gens = {b: hostnt.PrimeGen(b, TS_M) for b in set(TS_WIDTHS)}
    g = hx.Context(TS_M)
    for b in TS_WIDTHS:
        g.add_prime(gens[b].next())
    assert g.phim == TS_N and [q.bit_length() for q in g.primes] == list(TS_WIDTHS)
    assert (TS_N // 2 + 255) // 256 == 3 and TS_N // 2 % 256 == 3
    return g


def _raw_tensor_sum(hx, outs, a0, a1, b0, b1, n=None):
    n = len(a0) if n is None else n

    def arr(ps):
        return (C.c_void_p * max(len(ps), 1))(*[p.h for p in ps])
    return hx.lib().hx_tensor_sum(outs[0].h, outs[1].h, outs[2].h, arr(a0), arr(a1), arr(b0), arr(b1), n)


def _sum_of_tensors(hx, a0, a1, b0, b1):
    """n x hx_tensor and the part-wise hx_add of the products"""
    acc = None
    for t in range(len(a0)):
        prod = hx.tensorProduct(a0[t], a1[t], b0[t], b1[t])
        if acc is None:
            acc = prod
        else:
            for x, y in zip(acc, prod):
                x += y
    return acc


@pytest.fixture(scope="module")
def ts_polys(hx, ts_ring):
    """per batch size: five quadruples (a0, a1, b0, b1) of polys on TS_IDX, their words as python integers, and the
    four products a0 b0, a0 b1, a1 b0, a1 b1 of each, computed once.  Quadruple 1 is a square (a is b); quadruple 2
    has quadruple 0's a0 as its b1."""
    g = ts_ring
    qs = [g.primes[i] for i in TS_IDX]
    qcol = np.array(qs, dtype=object).reshape(-1, 1, 1)
    made = {}
    for B in (1, 5, 8):
        rng = np.random.default_rng(B)

        def rnd():
            x = np.stack([rng.integers(0, q, size=(B, TS_N), dtype=np.uint64) for q in qs])
            x[:, -1, -2:] = [[q - 1, 0] for q in qs]             # the last vector of the last element of every row
            x[:, 0, :2] = [[q - 1, q - 1] for q in qs]
            return x
        words, quads = [], []
        for k in range(5):
            w = [rnd() for _ in range(4)]
            if k == 1:
                w[2], w[3] = w[0], w[1]
            if k == 2:
                w[3] = words[0][0]
            words.append(w)
        polys = {}
        for k, w in enumerate(words):
            quad = []
            for j, x in enumerate(w):
                key = id(x)
                if key not in polys:
                    polys[key] = hx.DoubleCRT(g, TS_IDX, B, x)
                quad.append(polys[key])
            quads.append(quad)
        assert quads[1][0] is quads[1][2] and quads[1][1] is quads[1][3] and quads[2][3] is quads[0][0]
        prods = []
        for w in words:
            a0, a1, b0, b1 = (x.astype(object) for x in w)
            prods.append((a0 * b0, a0 * b1 + a1 * b0, a1 * b1))
        made[B] = (quads, words, prods, qcol)
    return made


@pytest.mark.parametrize("B", [1, 5, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 129, 257])
def test_tensor_sum_against_python_integers_and_the_calls_it_replaces(hx, ts_ring, ts_polys, n, B):
    """A workgroup column takes 256 two-word vectors and a thread 1 or 4 batch elements: 1030 coefficients are three
    columns, the last with 3 live threads; B = 1, 5, 8 are BP = 1, a partial second group and two full ones.  The
    accumulators are reduced every 128 terms: n = 129 and 257 cross one and two reductions inside the loop.  Term t is
    quadruple t mod 5, so the expected sum is sum_k count_k * product_k in python integers."""
    g = ts_ring
    quads, words, prods, qcol = ts_polys[B]
    terms = [quads[t % 5] for t in range(n)]
    count = [sum(1 for t in range(n) if t % 5 == k) for k in range(5)]
    want = []
    for part in range(3):
        total = sum(count[k] * prods[k][part] for k in range(5) if count[k])
        want.append((total % qcol).astype(np.uint64))
    cols = [[q[j] for q in terms] for j in range(4)]
    rng = np.random.default_rng(n)
    bystander = np.stack([rng.integers(0, g.primes[i], size=(B, TS_N), dtype=np.uint64) for i in TS_IDX])
    before = hx.DoubleCRT(g, TS_IDX, B, bystander)
    outs = [hx.DoubleCRT(g, TS_IDX, B, bystander) for _ in range(3)]       # (overwritten, not read)
    after = hx.DoubleCRT(g, TS_IDX, B, bystander)
    assert _raw_tensor_sum(hx, outs, *cols) == 0, hx.lib().hx_last_error()
    for part in range(3):
        got = outs[part].download()
        bad = np.argwhere(got != want[part])
        assert not len(bad), "part %d: %d words differ, the first at [row, element, word] %s" % (part, len(bad), bad[0])
    assert np.array_equal(before.download(), bystander) and np.array_equal(after.download(), bystander)
    for k in range(min(n, 5)):
        for j in range(4):
            assert np.array_equal(quads[k][j].download(), words[k][j])      # the inputs are left as they were
    # the binding, and the sequence the kernel replaces: the same words
    new = hx.tensorSum(*cols)
    seq = _sum_of_tensors(hx, *cols)
    for part in range(3):
        assert new[part].getIndexSet() == TS_IDX and np.array_equal(new[part].download(), want[part])
        assert np.array_equal(seq[part].download(), want[part])


@pytest.mark.parametrize("B", [1, 5])
def test_tensor_sum_of_257_terms_of_q_minus_1(hx, ts_ring, B):
    """every operand word q - 1: (q - 1)^2 = 1 mod q, so the words are exactly n, 2 n, n mod q in every row, while the
    128-bit accumulator of the middle part takes 256 products (q - 1)^2 between two reductions, the most it ever holds"""
    g, n = ts_ring, 257
    full = np.stack([np.full((B, TS_N), g.primes[i] - 1, dtype=np.uint64) for i in TS_IDX])
    x = hx.DoubleCRT(g, TS_IDX, B, full)
    y = x.copy()                                                 # a lazy copy among the operands
    outs = [x.copy() for _ in range(3)]                          # outputs that still share the operand's rows
    ops = [x, y] * 128 + [x]
    assert _raw_tensor_sum(hx, outs, ops, ops[::-1], ops, [x] * n) == 0, hx.lib().hx_last_error()
    assert np.array_equal(x.download(), full) and np.array_equal(y.download(), full)
    for part, mult in enumerate((1, 2, 1)):
        want = np.stack([np.full((B, TS_N), mult * n % g.primes[i], dtype=np.uint64) for i in TS_IDX])
        assert np.array_equal(outs[part].download(), want), part
    seq = _sum_of_tensors(hx, ops, ops, ops, ops)
    assert all(np.array_equal(seq[k].download(), outs[k].download()) for k in range(3))


# ---- (c) refusals ----
def test_tensor_sum_refusals_touch_nothing(hx):
    import torch
    g, other = hx.Context(85), hx.Context(85)
    gen = hostnt.PrimeGen(60, 85)
    for q in [gen.next() for _ in range(4)]:
        g.add_prime(q)
        other.add_prime(q)
    rng = np.random.default_rng(2)

    def rnd(ctx=g, idx=(0, 1, 2), B=2):
        return hx.DoubleCRT(ctx, list(idx), B, np.stack([rng.integers(0, ctx.primes[i], size=(B, 64), dtype=np.uint64) for i in idx]))
    o = [rnd(), rnd(), rnd()]
    a0, a1, b0, b1 = ([rnd(), rnd()] for _ in range(4))
    polys = o + a0 + a1 + b0 + b1
    keep = [x.download() for x in polys]
    L = hx.lib()
    INV, UNS = hx.HX_ERR_INVALID, hx.HX_ERR_UNSUPPORTED

    def call(outs=o, A0=a0, A1=a1, B0=b0, B1=b1, n=None):
        return _raw_tensor_sum(hx, outs, A0, A1, B0, B1, n)
    null = type("Null", (), {"h": None})()
    # a null handle: an output, an array, an entry
    assert call(outs=[null, o[1], o[2]]) == INV and call(outs=[o[0], o[1], null]) == INV
    arr = (C.c_void_p * 2)(a0[0].h, a0[1].h)
    assert L.hx_tensor_sum(o[0].h, o[1].h, o[2].h, arr, arr, None, arr, 2) == INV and b"null" in L.hx_last_error()
    assert call(B1=[b1[0], null]) == INV and b"null poly (b1[1])" in L.hx_last_error()
    # n < 1
    assert call(n=0) == INV and b"at least one term" in L.hx_last_error() and call(n=-1) == INV
    # two outputs that are the same poly
    assert call(outs=[o[0], o[0], o[2]]) == INV and b"the same poly" in L.hx_last_error()
    assert call(outs=[o[0], o[1], o[0]]) == INV and call(outs=[o[0], o[1], o[1]]) == INV
    # an output that is also an input
    assert call(A0=[a0[0], o[2]]) == INV and b"also an input (a0[1])" in L.hx_last_error()
    assert call(B1=[o[0], b1[1]]) == INV and call(A1=[o[1], a1[1]]) == INV and call(B0=[b0[0], o[1]]) == INV
    # a poly of another context
    assert call(A1=[a1[0], rnd(other)]) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(outs=[o[0], rnd(other), o[2]]) == INV and b"incompatible objects" in L.hx_last_error()
    # a batch or a prime set that is not o0's
    assert call(B0=[rnd(B=3), b0[1]]) == INV and b"b0[0] differs from o0" in L.hx_last_error()
    assert call(A0=[a0[0], rnd(idx=(0, 2, 1))]) == INV and b"a0[1] differs from o0" in L.hx_last_error()
    assert call(A1=[rnd(idx=(0, 1)), a1[1]]) == INV and call(B1=[b1[0], rnd(idx=(0, 1, 2, 3))]) == INV
    assert call(outs=[o[0], rnd(B=1), o[2]]) == INV and b"o1 differs from o0" in L.hx_last_error()
    assert call(outs=[o[0], o[1], rnd(idx=(2, 1, 0))]) == INV and b"o2 differs from o0" in L.hx_last_error()
    # rows that are not 16-byte aligned: polys over caller-owned memory that starts 8 bytes into an allocation
    words = 3 * 2 * 64
    buf = torch.zeros(2 * (words + 2), dtype=torch.int64, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    odd_in = hx.DoubleCRT.wrap(g, [0, 1, 2], 2, buf.data_ptr() + 8)
    odd_out = hx.DoubleCRT.wrap(g, [0, 1, 2], 2, buf.data_ptr() + 8 * (words + 2) + 8)
    assert call(B0=[b0[0], odd_in]) == INV and b"b0[1]: rows are not 16-byte aligned" in L.hx_last_error()
    assert call(outs=[o[0], odd_out, o[2]]) == INV and b"output rows are not 16-byte aligned" in L.hx_last_error()
    assert not buf.cpu().numpy().any()
    # an odd number of coefficients: phi(m) is odd for m = 2 only; polys without rows reach the check
    tiny = hx.Context(2)
    t = [hx.DoubleCRT(tiny, [], 1, zero=False) for _ in range(4)]
    assert _raw_tensor_sum(hx, t[:3], [t[3]], [t[3]], [t[3]], [t[3]]) == UNS
    assert b"hx_tensor_sum needs an even number of coefficients" in L.hx_last_error()
    # a call during a graph capture
    g.graphBegin()
    try:
        assert call() == UNS and b"cannot be captured" in L.hx_last_error()
    finally:
        try:
            g.graphEnd().destroy()
        except hx.HxError:
            pass
    with pytest.raises(hx.InvalidArgument, match="term by term"):
        hx.tensorSum(a0, a1, b0, b1[:1])
    with pytest.raises(hx.InvalidArgument, match="at least one term"):
        hx.tensorSum([], [], [], [])
    for x, k in zip(polys, keep):
        assert np.array_equal(x.download(), k)
    assert call() == 0                                           # and the context still works
    seq = _sum_of_tensors(hx, a0, a1, b0, b1)
    assert all(np.array_equal(o[k].download(), seq[k].download()) for k in range(3))


# ---- (d) Ctxt.innerProduct fused against the loop ----
def _keys(hx, m, bits, seed=5):
    from helib_amd import ctxt as hc, keys as hk
    cc = hc.ChainContext(m, 2, 1, bits=bits, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    return cc, g, sk


def _state(ct):
    return ct.lnNoise, ct.primeSet, ct.ptxtSpace, ct.intFactor, ct.ptxtMag


def _same_words(x, y):
    wx = {h: (part.getIndexSet(), part.download()) for h, part in x.parts.items()}
    wy = {h: (part.getIndexSet(), part.download()) for h, part in y.parts.items()}
    assert wx.keys() == wy.keys() == {"1", "s"}
    assert all(wx[h][0] == wy[h][0] and np.array_equal(wx[h][1], wy[h][1]) for h in wx)


def _count(hx, monkeypatch):
    seen = []
    real = hx.tensorSum
    monkeypatch.setattr(hx, "tensorSum", lambda *args: (seen.append(len(args[0])), real(*args))[1])
    return seen


@pytest.mark.parametrize("m", [85, 1024])
def test_inner_product_fused_against_the_loop(hx, monkeypatch, m):
    """p = 2, batch 3.  Three pairs of fresh ciphertexts, one of them a square: one hx_tensor_sum, and the words and the
    bookkeeping of the loop.  Then pair 0 fresh x fresh and pair 1 two products: the products end on different prime
    sets, the kernel does not apply, and the results are still the loop's."""
    from helib_amd.ctxt import Ctxt, innerProduct
    cc, g, sk = _keys(hx, m, 200)
    B = 3
    rng = np.random.default_rng(m)
    idx = list(cc.ctxtPrimes)

    def fresh():
        polys = [[int(v) for v in rng.integers(0, 2, cc.phim)] for _ in range(B)]
        return sk.EncryptBatch(sk.be.fromCoeffsBatch(idx, polys))
    x = [fresh() for _ in range(5)]
    v1, v2 = [x[0], x[1], x[2]], [x[3], x[1], x[4]]
    seen = _count(hx, monkeypatch)
    loop = Ctxt.innerProduct(v1, v2, fused=False)
    assert not seen
    monkeypatch.setattr(Ctxt, "fuseTensorSum", False)
    default = Ctxt.innerProduct(v1, v2)
    assert not seen                                              # fused=None follows the class flag
    fused = Ctxt.innerProduct(v1, v2, fused=True)
    assert seen == [3]                                           # the kernel ran, once, on the three pairs
    free = innerProduct(v1, v2)
    for other in (fused, default, free):
        assert _state(other) == _state(loop)
        _same_words(other, loop)
    assert loop.isCorrect() and loop.primeSet != frozenset(idx)
    # mixed levels
    p1, p2 = x[0].clone(), x[2].clone()
    p1.multiplyBy(x[1])
    p2.multiplyBy(x[3])
    assert p1.primeSet != x[0].primeSet
    del seen[:]
    loop = Ctxt.innerProduct([x[0], p1], [x[4], p2], fused=False)
    fused = Ctxt.innerProduct([x[0], p1], [x[4], p2], fused=True)
    assert not seen
    assert _state(fused) == _state(loop)
    _same_words(fused, loop)
    # with the flag set, fused=None takes the kernel
    monkeypatch.setattr(Ctxt, "fuseTensorSum", True)
    again = Ctxt.innerProduct(v1[:2], v2[:2])
    assert seen == [2]
    ref = Ctxt.innerProduct(v1[:2], v2[:2], fused=False)
    assert _state(again) == _state(ref)
    _same_words(again, ref)


# ---- (e) the circuits on real slots ----
E_BITS = 200


@pytest.fixture(scope="module")
def slots(hx):
    """m = 85, p = 2: 8 slots, batch 2: 16 independent numbers per run"""
    from helib_amd import bgv_crt
    cc, g, sk = _keys(hx, 85, E_BITS)
    ea = bgv_crt.EncryptedArray(cc, g)
    assert ea.size() == 8
    return cc, g, sk, ea


def _values(seed, nbits):
    """[2, 8] integers below 2^nbits with the all-zero and the all-one patterns planted"""
    v = np.random.default_rng(seed).integers(0, 1 << nbits, size=(2, 8))
    v[0, 0], v[0, 1], v[1, 7] = 0, (1 << nbits) - 1, (1 << nbits) - 1
    return v


def _signed(v, nbits):
    v = v & ((1 << nbits) - 1)
    return np.where(v >> (nbits - 1), v - (1 << nbits), v)


@pytest.fixture(params=[False, True], ids=["reference", "lazy"])
def lazy(request, hx, monkeypatch):
    """lazy: the one-relinearisation carry and conditional, over hx_tensor_sum"""
    from helib_amd import binary_arith as ba
    from helib_amd.ctxt import Ctxt
    seen = _count(hx, monkeypatch)
    monkeypatch.setattr(ba, "lazyCarry", request.param)
    monkeypatch.setattr(Ctxt, "fuseTensorSum", request.param)
    return request.param, seen


def _dec(slots, number, twos=False):
    from helib_amd import binary_arith as ba
    _, _, sk, ea = slots
    live = [c for c in number if c is not None and c.parts]
    assert all(c.isCorrect() and c.bitCapacity() > 0 for c in live)
    return ba.decryptBinaryNums(number, sk, ea, twos)


def test_add_and_subtract_on_slots(slots, lazy):
    from helib_amd import binary_arith as ba
    _, _, sk, ea = slots
    a, b = _values(1, 4), _values(2, 4)
    b[0, 1] = 1                                                  # 15 + 1: the carry runs through every position
    A, Bn = ba.encryptBinaryNums(ea, sk, a, 4), ba.encryptBinaryNums(ea, sk, b, 4)
    total = ba.addTwoNumbers(A, Bn)
    assert len(total) == 5 and np.array_equal(_dec(slots, total), a + b)
    diff = ba.subtractBinary(A, Bn)
    assert len(diff) == 4 and np.array_equal(_dec(slots, diff), (a - b) % 16)
    assert np.array_equal(_dec(slots, diff, twos=True), _signed(a - b, 4))
    # three numbers: the 3-for-2 step, lazy or not, then the sum
    c = _values(3, 3)
    many = ba.addManyNumbers([list(A), list(Bn), ba.encryptBinaryNums(ea, sk, c, 3)])
    assert np.array_equal(_dec(slots, many), a + b + c)
    assert bool(lazy[1]) == lazy[0]                              # the kernel ran exactly where the lazy carry asked
    assert np.array_equal(_dec(slots, A), a)


@pytest.mark.parametrize("twos", [False, True], ids=["unsigned", "twos"])
def test_mult_on_slots(slots, lazy, twos):
    from helib_amd import binary_arith as ba
    _, _, sk, ea = slots
    a, b = _values(4, 3), _values(5, 3)
    A, Bn = ba.encryptBinaryNums(ea, sk, a, 3), ba.encryptBinaryNums(ea, sk, b, 3)
    prod = ba.multTwoNumbers(A, Bn, rhsTwosComplement=twos)
    assert len(prod) == 6
    want = a * (_signed(b, 3) if twos else b)
    assert np.array_equal(_dec(slots, prod, twos), want)
    assert bool(lazy[1]) == lazy[0] and all(n == 2 for n in lazy[1])


@pytest.mark.parametrize("twos", [False, True], ids=["unsigned", "twos"])
def test_compare_on_slots(slots, lazy, twos):
    from helib_amd import binary_compare as bc, binary_arith as ba
    _, _, sk, ea = slots
    a, b = _values(6, 4), _values(7, 4)
    b[1, 3] = a[1, 3]                                            # an equal pair
    A, Bn = ba.encryptBinaryNums(ea, sk, a, 4), ba.encryptBinaryNums(ea, sk, b, 4)
    mx, mn, mu, ni = bc.compareTwoNumbers(A, Bn, twosComplement=twos)
    va, vb = (_signed(a, 4), _signed(b, 4)) if twos else (a, b)
    assert np.array_equal(_dec(slots, mx, twos), np.maximum(va, vb))
    assert np.array_equal(_dec(slots, mn, twos), np.minimum(va, vb))
    assert np.array_equal(_dec(slots, [mu]), (va > vb).astype(np.int64))
    assert np.array_equal(_dec(slots, [ni]), (va < vb).astype(np.int64))


def test_cond_and_counter_on_slots(slots, lazy):
    from helib_amd import binary_arith as ba
    _, _, sk, ea = slots
    t, f, cond = _values(8, 4), _values(9, 4), _values(10, 1)
    T, F = ba.encryptBinaryNums(ea, sk, t, 4), ba.encryptBinaryNums(ea, sk, f, 4)
    Cn = ba.encryptBinaryNums(ea, sk, cond, 1)[0]
    got = ba.binaryCond(Cn, T, F)
    assert np.array_equal(_dec(slots, got), np.where(cond == 1, t, f))
    assert lazy[1] == ([2] * 4 if lazy[0] else [])
    bits = _values(11, 7)
    ins = ba.encryptBinaryNums(ea, sk, bits, 7)
    out, n = ba.fifteenOrLess4Four(ins)
    popcount = sum((bits >> k) & 1 for k in range(7))
    assert n == 3 and len(out) == 4 and np.array_equal(_dec(slots, out), popcount)
