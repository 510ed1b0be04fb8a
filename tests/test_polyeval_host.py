"""helib_amd.polyeval on the host side (no GPU): the digit polynomials in python integers, exhaustively; polyEval's branches,
Ctxt.linearCombination fused against unfused, extractDigits for p > 3 and extendExtractDigits over the oracle backend
with hx_lin_comb stated in python integers (tests/polyeval_ref.lin_comb); the declarations of the new C entry.

Chain sizes: every fixture below is built with bits = 100, the smallest multiple of 100 at which the unfused path leaves
every result of these tests with a positive capacity (found by running them on the CPU: at m = 31, p^r = 25 the
degree-11 polynomial keeps 33 bits, the digits of 5^2 keep 60 and 63; at m = 80, 7^2 they keep 51 and 54; the two
extended digits at m = 31, 2^4 keep 69 and 62)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import polyeval_ref as R
from tests.test_bgv_pr_host import _Setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(m, p, r, bits=100, seed=3):
    """test_bgv_pr_host's fixture (oracle backend, CPU encoder) with the two entries the oracle backend lacks stated in
    python integers: linComb (hx_lin_comb) and constantLike.  s.lc lists the linComb calls."""
    from oracle.backend import OPoly
    s = _Setup(m, p, r, seed=seed, bits=bits)
    o = s.be.o
    s.lc = []

    class Ops(type(s.be.ops)):
        def linComb(self, in0, in1, idx, w, addend=None):
            assert len(w) == len(in0) >= 1 and (in1 is None or len(in1) == len(in0))
            for t, part in enumerate(in0):
                assert isinstance(part, OPoly) and set(part.idx) <= set(idx)
                assert in1 is None or in1[t].idx == part.idx
            for row in list(w) + ([addend] if addend is not None else []):
                assert len(row) == len(idx) and all(0 <= int(x) < o.primes[i] for x, i in zip(row, idx))
            s.lc.append(([list(map(int, row)) for row in w], None if addend is None else list(map(int, addend)), list(idx)))
            outs = []
            for k, ins in enumerate((in0, in1)):
                if ins is None:
                    outs.append(None)
                    continue
                rows = R.lin_comb([part.rows[:, None, :] for part in ins], [part.idx for part in ins], idx, w,
                                  addend if k == 0 else None, o.primes)
                outs.append(OPoly(o, idx, rows[:, 0, :]))
            return tuple(outs)

        def constantLike(self, poly, idx, num):
            return OPoly(o, idx, np.array([[int(num) % o.primes[i]] * o.N for i in idx], dtype=np.uint64))
    s.be.ops = Ops(o)
    return s


@pytest.fixture(scope="module")
def s25():
    """m = 31, p^r = 5^2: 10 slots; bits = 100 (see the module docstring)"""
    s = _setup(31, 5, 2)
    assert s.ea.size() == 10
    return s


@pytest.fixture(scope="module")
def s49():
    """m = 80, p^r = 7^2: 8 slots; bits = 100"""
    s = _setup(80, 7, 2)
    assert s.ea.size() == 8
    return s


@pytest.fixture(scope="module")
def s16():
    """m = 31, p^r = 2^4: 6 slots; bits = 100"""
    return _setup(31, 2, 4)


def _state(ct):
    return ({h: part.rows.copy() for h, part in ct.parts.items()}, {h: list(part.idx) for h, part in ct.parts.items()},
            ct.lnNoise, ct.primeSet, ct.ptxtSpace, ct.intFactor, ct.ptxtMag)


def _same(a, b):
    assert a[1:] == b[1:]
    assert a[0].keys() == b[0].keys() and all(np.array_equal(a[0][h], b[0][h]) for h in a[0])


# ---- the polynomials, in python integers ----
@pytest.mark.parametrize("p,e", [(5, 2), (5, 3), (7, 2), (11, 2), (13, 2)])
def test_digit_polynomial_exhaustively(p, e):
    """poly(z0 + p^t z1) = z0 mod p^(t+1) for every balanced z0, every 1 <= t < e and every z1 below p^(e-t).  (At t = 0
    the form z0 + z1 is any integer and fixes no z0: there the statement is poly(z) = z mod p, checked for every z.)"""
    from helib_amd import polyeval
    f = polyeval.buildDigitPolynomial(p, e)
    assert len(f) == p + 1 and f[p] == 1
    for t in range(1, e):
        M = p ** (t + 1)
        for z0 in range(-(p // 2), p // 2 + 1):
            for z1 in range(p ** (e - t)):
                assert R.plain([z0 + p ** t * z1], f, M) == [z0 % M], (t, z0, z1)
    assert R.plain(range(p ** e), f, p) == [z % p for z in range(p ** e)]
    if (p, e) == (5, 2):
        assert [c % 25 for c in f] == [0, 5, 0, 20, 0, 1]
    if (p, e) == (11, 2):
        assert [c % 121 for c in f] == [0, 0, 0, 22, 0, 99, 0, 55, 0, 66, 0, 1]
    assert polyeval.buildDigitPolynomial(p, 1) == [] and polyeval.buildDigitPolynomial(1, 3) == []


@pytest.mark.parametrize("p,e", [(2, 5), (3, 3), (5, 2), (7, 2)])
def test_magic_polynomial_exhaustively(p, e):
    """G(x) = balanced (x mod p) modulo p^e for every x; the representative is in [0, 1] for p = 2"""
    from helib_amd import polyeval
    G, M = polyeval.compute_magic_poly(p, e), p ** e
    assert len(G) - 1 <= (e - 1) * (p - 1) + 1 and all(0 <= c < M for c in G)
    got = R.plain(range(M), G, M)
    assert got == [R.digits(x, p, 1)[0] % M for x in range(M)]
    if p == 2:
        assert set(got) == {0, 1}
    a = polyeval.compute_a_vals(p, e)
    assert len(a) == (e - 1) * (p - 1) + 2 and not any(a[:p])


def test_interpolate_mod():
    from helib_amd import hostnt
    xs, ys = [-2, -1, 0, 1, 2], [7, 100, 31, 62, 124]
    f = hostnt.interpolateMod(xs, ys, 5, 3)
    assert len(f) <= 5 and R.plain(xs, f, 125) == [y % 125 for y in ys]
    with pytest.raises(ValueError, match="distinct"):
        hostnt.interpolateMod([0, 5], [1, 2], 5, 2)


# ---- polyEval ----
PI = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8]
BRANCHES = {                                         # name: (polynomial, lowest coefficient first; k)
    "degree 0": ([7], 0),
    "degree 1": ([3, 24], 0),
    "degree 2": ([1, 0, 6], 0),
    "degree 8, n a power of two": (PI[:8] + [7], 0),
    "degree 6, k = 2: n = t - 1": ([2, 7, 1, 8, 2, 8, 1], 2),
    "degree 11, the general recursion": (PI, 0),
    "a leading coefficient divisible by p": ([1, 2, 3, 4, 5, 6, 5], 0),
    "a unit leading coefficient": ([1, 2, 3, 4, 5, 6, 2], 0),
    "an explicit k": (PI, 4),
    "all coefficients zero": ([0, 0, 0], 0),
    "a zero free term": ([0, 3, 0, 1], 0),
    "the digit polynomial of 5^2": ([0, 5, 0, 20, 0, 1], 0),
}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", list(BRANCHES))
def test_poly_eval_branches(s25, name, fused):
    """decrypted against the plain evaluation per slot; the products and the powers formed are the replay's"""
    from helib_amd import polyeval
    poly, k = BRANCHES[name]
    ea, sk, P = s25.ea, s25.sk, s25.P
    a = s25.slots(3)
    a[0, :3] = [0, P - 1, P // 2]
    ct = ea.encrypt(sk, a[0])
    before = _state(ct)
    st = {}
    n = len(s25.lc)
    y = polyeval.polyEval(ct, poly, k, fused=fused, stats=st)
    want, rst = R.replay(a[0], poly, P, k)
    assert want == R.plain(a[0], poly, P)
    assert [int(v) for v in ea.decrypt_batch(y, sk)[0]] == want
    assert st == rst, (st, rst)
    calls = len(s25.lc) - n                          # a leaf without a non-zero baby-step term makes no call
    assert (0 < calls <= st["leaves"]) if fused and len(R._norm(poly)) > 1 else calls == 0
    if any(poly):
        assert y.bitCapacity() > 0 and y.isCorrect() and y.ptxtSpace == P
    else:
        assert not y.parts
    _same(_state(ct), before)                        # x is left as it was
    # which branch ran
    d = len(R._norm(poly)) - 1
    if name.startswith("degree 8"):
        assert (st["mults"], ("giant", 2) in st["powers"]) == (5, True)
    if name.startswith("degree 6"):
        assert ("baby", 2) in st["powers"] and ("giant", 2) in st["powers"] and st["mults"] == 3
    if name.startswith("degree 11"):
        assert ("giant", 6) in st["powers"] and d % 2 == 1            # n k = 12 != 11: the extra term X^12
    if name.startswith("a leading") or name.startswith("a unit"):
        # k = 1, n = 6: the unit top needs 3 giant steps (t = 3), the extra term all 6
        assert (("giant", 6) in st["powers"]) == name.startswith("a leading")


def test_the_recursion_with_a_remainder_of_the_degree(s25):
    """delta = deg mod k != 0 in recursivePolyEval (:351, :382-384) cannot be reached through polyEval, whose top level
    pads the degree to n k before it recurses (and u = deg - k (t - 1) then stays a multiple of k); the step is run here
    on its own, on a monic polynomial of degree 11 with k = 2 and k + delta = 3 baby steps"""
    from helib_amd import polyeval
    ea, sk, P = s25.ea, s25.sk, s25.P
    a = s25.slots(4)
    ct = ea.encrypt(sk, a[0])
    poly = PI[:11] + [1]
    st = {}
    ev = polyeval._Eval(ct, False, st)
    baby = polyeval.DynamicCtxtPowers(ct, 3, st, "baby")
    giant = polyeval.DynamicCtxtPowers(baby.getPower(2), 4, st, "giant")
    y = ev.recursive(poly, 2, baby, giant)
    assert [int(v) for v in ea.decrypt_batch(y, sk)[0]] == R.plain(a[0], poly, P)
    assert y.bitCapacity() > 0


def test_poly_eval_of_encrypted_coefficients(s25):
    from helib_amd import polyeval
    ea, sk, P = s25.ea, s25.sk, s25.P
    a = s25.slots(5)
    x = ea.encrypt(sk, a[0])
    rng = np.random.default_rng(6)
    for n in (0, 1, 2, 6, 8):
        cf = rng.integers(0, P, size=(n, ea.size()))
        cts = [ea.encrypt(sk, row) for row in cf]
        y = polyeval.polyEvalCtxt(cts, x)
        want = [sum(int(cf[i][j]) * int(a[0][j]) ** i for i in range(n)) % P for j in range(ea.size())]
        assert [int(v) for v in ea.decrypt_batch(y, sk)[0]] == want, n
        assert n == 0 or y.bitCapacity() > 0


def test_dynamic_powers_and_power_agree(s25):
    """Ctxt.power runs on DynamicCtxtPowers: the same words and bookkeeping as the class used directly"""
    from helib_amd import polyeval
    from helib_amd import ctxt as hc
    assert polyeval.DynamicCtxtPowers is hc.DynamicCtxtPowers
    ea, sk, P = s25.ea, s25.sk, s25.P
    a = s25.slots(7)
    ct = ea.encrypt(sk, a[0])
    st = {"mults": 0, "powers": set()}
    pw = polyeval.DynamicCtxtPowers(ct, 7, st, "x")
    seven = pw.getPower(7)
    assert st == {"mults": 4, "powers": {("x", 2), ("x", 3), ("x", 4), ("x", 7)}}
    assert pw.wasComputed(3) and not pw.wasComputed(5) and pw.size() == 7
    other = ct.clone()
    assert other.power(7) is other                   # the same words and prime set (power() keeps its own way with the
    a7, b7 = _state(other), _state(seven)            # noise estimate, which this pull request leaves alone)
    _same(a7[:2] + a7[3:], b7[:2] + b7[3:])
    assert [int(v) for v in ea.decrypt_batch(seven, sk)[0]] == [pow(int(v), 7, P) for v in a[0]]
    with pytest.raises(IndexError):
        pw.getPower(8)


# ---- Ctxt.addScalar and Ctxt.linearCombination ----
def test_add_scalar(s25):
    import math
    from helib_amd import ctxt as hc
    ea, sk, P = s25.ea, s25.sk, s25.P
    a = s25.slots(8)
    ct = ea.encrypt(sk, a[0])
    ct.multiplyBy(ea.encrypt(sk, np.ones(ea.size(), dtype=np.int64)))     # an intFactor other than 1, another prime set
    assert ct.intFactor != 1
    for c, neg in ((7, False), (-3, False), (13, True), (P + 2, False)):
        before = _state(ct)
        f = ct._constFactor()
        assert ct.addScalar(c, neg) is ct
        a = (a - c) % P if neg else (a + c) % P
        assert np.array_equal(ea.decrypt_batch(ct, sk), a)
        cc = c % P - P if c % P > P // 2 else c % P
        assert ct.lnNoise == hc.logaddexp(before[2], math.log(abs(cc) * abs(f)))
        assert _state(ct)[3:] == before[3:]
    before = _state(ct)
    ct.addScalar(2 * P)                              # zero: nothing to do
    _same(_state(ct), before)
    # an empty ciphertext gains the part pointing at 1, on its prime set
    e = ct.clone()
    e.clear()
    assert not e.parts and e.primeSet == frozenset(s25.cc.ctxtPrimes)
    e.addScalar(-4)
    assert list(e.parts) == ["1"] and sorted(e.parts["1"].idx) == sorted(e.primeSet)
    assert np.array_equal(ea.decrypt_batch(e, sk), np.full((1, ea.size()), P - 4))
    e += ea.encrypt(sk, a[0])
    assert np.array_equal(ea.decrypt_batch(e, sk), (a - 4) % P)


def _terms(s, seed):
    """x, x^2 and x^4 (prime sets and intFactors that differ) and a fresh y, with coefficients that are units,
    multiples of p, zero modulo p^r and below zero"""
    ea, sk, P = s.ea, s.sk, s.P
    a, b = s.slots(seed), s.slots(seed + 1)
    x, y = ea.encrypt(sk, a[0]), ea.encrypt(sk, b[0])
    x2 = x.clone()
    x2.multiplyBy(x)
    x4 = x2.clone()
    x4.multiplyBy(x2)
    x2.multByScalar(3)                               # a unit: into the intFactor
    # the sum starts on the smaller set and is modded up by the second term; later terms are modded up to the sum
    assert x.primeSet < x4.primeSet and len({x.intFactor, x2.intFactor, x4.intFactor}) >= 2
    terms = [(x, 11), (x4, 7), (y, 2 * P), (x2, s.p), (y, -s.p * 3), (x2, P - 1), (x4, 0), (x, -2)]
    free = -8
    want = (7 * a ** 4 - 2 * a - 3 * s.p * b + (s.p + P - 1) * 3 * a ** 2 + 11 * a + free) % P
    return terms, free, want


@pytest.mark.parametrize("which", ["s25", "s49"])
def test_linear_combination_fused_equals_unfused(which, request):
    from helib_amd import ctxt as hc
    s = request.getfixturevalue(which)
    ea, sk, P = s.ea, s.sk, s.P
    terms, free, want = _terms(s, 20)
    before = [_state(ct) for ct, _ in terms]
    n = len(s.lc)
    plain = hc.Ctxt.linearCombination(terms, free, fused=False)
    also = hc.Ctxt.linearCombination(terms, free)    # the default is the call sequence
    assert len(s.lc) == n and hc.Ctxt.fuseLinComb is False
    fused = hc.Ctxt.linearCombination(terms, free, fused=True)
    assert len(s.lc) == n + 1                        # one call
    w, addend, idx = s.lc[-1]
    assert len(w) == 6 and addend is not None        # the two terms that are zero modulo p^r are dropped
    assert idx == plain.parts["1"].idx and len(idx) == len(plain.primeSet)
    _same(_state(fused), _state(plain))
    _same(_state(also), _state(plain))
    assert np.array_equal(ea.decrypt_batch(fused, sk), want) and fused.bitCapacity() > 0
    for (ct, _), st in zip(terms, before):           # the inputs are left as they were
        _same(_state(ct), st)
    # no free term: no addend; every coefficient 1: the weights are the mod-up and intFactor integers alone
    fused, plain = (hc.Ctxt.linearCombination([(ct, 1) for ct, _ in terms[:3]], 0, fused=f) for f in (True, False))
    assert s.lc[-1][1] is None
    _same(_state(fused), _state(plain))
    # one part on every side
    ones = []
    for ct, c in terms[:2]:
        o = ct.clone()
        del o.parts["s"]
        ones.append((o, c))
    n = len(s.lc)
    fused, plain = (hc.Ctxt.linearCombination(ones, 3, fused=f) for f in (True, False))
    assert len(s.lc) == n + 1 and list(fused.parts) == ["1"]
    _same(_state(fused), _state(plain))
    # what cannot be fused runs as the sequence: three parts on one side; nothing left after the zeros
    three = terms[0][0].clone()
    three.multLowLvl(terms[1][0])
    three._materializeTensor()
    assert len(three.parts) == 3
    n = len(s.lc)
    fused, plain = (hc.Ctxt.linearCombination([(three, 2), terms[0]], 1, fused=f) for f in (True, False))
    _same(_state(fused), _state(plain))
    fused, plain = (hc.Ctxt.linearCombination([(terms[0][0], P)], 6, fused=f) for f in (True, False))
    _same(_state(fused), _state(plain))
    assert list(fused.parts) == ["1"] and np.array_equal(ea.decrypt_batch(fused, sk), np.full((1, ea.size()), 6))
    assert len(s.lc) == n
    with pytest.raises(ValueError, match="no terms"):
        hc.Ctxt.linearCombination([], 1)


def test_fused_insists_on_a_backend_with_lin_comb():
    from helib_amd import ctxt as hc
    s = _Setup(31, 5, 2, bits=100)                   # the oracle backend as it is: no linComb
    ct = s.ea.encrypt(s.sk, s.slots(1)[0])
    with pytest.raises(RuntimeError, match="no linComb"):
        hc.Ctxt.linearCombination([(ct, 2)], 0, fused=True)
    hc.Ctxt.fuseLinComb = True                       # the class flag asks, it does not insist
    try:
        y = hc.Ctxt.linearCombination([(ct, 2)], 0)
    finally:
        hc.Ctxt.fuseLinComb = False
    assert np.array_equal(s.ea.decrypt_batch(y, s.sk), 2 * s.slots(1) % 25)


# ---- digit extraction ----
@pytest.mark.parametrize("which", ["s25", "s49"])
def test_extract_digits_above_three(which, request):
    from helib_amd import bgv_pr, ckks, polyeval
    s = request.getfixturevalue(which)
    ea, sk, p, r, P = s.ea, s.sk, s.p, s.r, s.P
    a = s.slots(11)
    a[0, :3] = [0, P - 1, P // 2]
    ct = ea.encrypt(sk, a[0])
    n, n_sub = len(s.lc), len(s.calls)
    plain = polyeval.extractDigits(ea, ct, fused=False)
    assert len(s.lc) == n and len(s.calls) == n_sub
    fused = polyeval.extractDigits(ea, ct, fused=True)
    assert len(s.lc) > n and len(s.calls) <= n_sub + r * (r - 1) // 2          # (hx_scaled_sub where the rows line up)
    assert len(plain) == len(fused) == r
    for j, (x, y) in enumerate(zip(fused, plain)):
        _same(_state(x), _state(y))
        assert x.ptxtSpace == p ** (r - j) and x.bitCapacity() > 0 and x.isCorrect()
        got = ea.decrypt_batch(x, sk)[0]
        assert [int(v) % p for v in got] == [R.digits(int(v), p, r)[j] % p for v in a[0]], j
    assert np.array_equal(ea.decrypt_batch(ct, sk), a)
    # the p^r module keeps its refusal, and points here
    with pytest.raises(ckks.LogicError, match="polyEval and buildDigitPolynomial"):
        bgv_pr.extractDigits(ea, ct)
    assert "helib_amd.polyeval" in bgv_pr.extractDigits.__doc__


def test_extract_digits_up_to_three_runs_the_same_steps():
    from helib_amd import bgv_pr, polyeval
    s = _setup(80, 3, 3, bits=300)
    ct = s.ea.encrypt(s.sk, s.slots(13)[0])
    for x, y in zip(polyeval.extractDigits(s.ea, ct), bgv_pr.extractDigits(s.ea, ct)):
        _same(_state(x), _state(y))
    assert not s.lc


def test_extend_extract_digits(s16):
    from helib_amd import polyeval
    ea, sk = s16.ea, s16.sk
    a = s16.slots(12)
    a[0, :3] = [0, 15, 10]
    ct = ea.encrypt(sk, a[0])
    res = {f: polyeval.extendExtractDigits(ea, ct, 2, 2, fused=f) for f in (False, True)}
    for j, (x, y) in enumerate(zip(res[True], res[False])):
        _same(_state(x), _state(y))
        assert x.ptxtSpace == 2 ** (4 - j) and x.bitCapacity() > 0
        got = ea.decrypt_batch(x, sk)[0]                                # the digit itself, modulo 2^(4-j)
        assert [int(v) for v in got] == [(int(v) >> j) & 1 for v in a[0]], j
    with pytest.raises(ValueError):
        polyeval.extendExtractDigits(ea, ct, 0, 2)


def test_ckks_is_refused():
    from helib_amd import ckks, polyeval
    from helib_amd import ctxt as hc
    cc = hc.ChainContext(64, -1, 20, bits=100, c=2, ckks=True)
    ct = hc.Ctxt(cc, None)
    with pytest.raises(ckks.LogicError, match="BGV only"):
        polyeval.polyEval(ct, [1, 2, 3])
    with pytest.raises(ckks.LogicError, match="BGV only"):
        polyeval.polyEvalCtxt([ct, ct], ct)
    with pytest.raises(TypeError):
        ct.addScalar(1)


# ---- the C entry ----
def test_lin_comb_is_declared_bound_and_exported():
    from helib_amd import capi
    from helib_amd import ctxt as hc
    hdr = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    declared = set(re.findall(r"\b(hx_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = capi.lib()                      # the cross-compiled library
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi._SO], text=True)
    assert "hx_lin_comb" in capi.SYMBOLS and "hx_lin_comb" in declared
    assert len(lib.hx_lin_comb.argtypes) == 7
    assert re.search(r"\bT hx_lin_comb$", out, re.M)
    assert len(lib.hx_mul_add_many.argtypes) == 7 and len(lib.hx_scaled_sub.argtypes) == 6      # left alone
    for cite in ("src/polyEval.cpp:240-253", "src/DoubleCRT.cpp:603-647"):
        assert cite in hdr, cite
    src = open(os.path.join(ROOT, "helib_amd", "csrc", "linalg.hip")).read()
    assert "lin_comb_kernel" in src and 'extern "C" int hx_lin_comb' in src
    # capi.linComb rejects bad arguments before it reaches the library
    with pytest.raises(capi.InvalidArgument, match="required"):
        capi.linComb(None, None, [0], [[1]])
    with pytest.raises(capi.InvalidArgument, match="at least one term"):
        capi.linComb([], None, [0], [])
    with pytest.raises(capi.InvalidArgument, match="go together"):
        capi.linComb([object()], [], [0], [[1]])
    with pytest.raises(capi.InvalidArgument, match="one weight per term"):
        capi.linComb([object()], None, [0, 1], [[1]])
    with pytest.raises(capi.InvalidArgument, match="one weight per term"):
        capi.linComb([object()], None, [0, 1], [[1, 2]], [3])
    for f in ("addScalar", "linearCombination"):
        assert f in vars(hc.Ctxt)
    assert hc.Ctxt.fuseLinComb is False and hc.Ctxt.fuseScaledSub is False
