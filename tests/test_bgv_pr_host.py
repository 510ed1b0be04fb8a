"""BGV slots modulo p^r on the host side (no GPU): the C++ table builder at r >= 1 (helib_amd/csrc/bgv_crt.h, printed by
tests/cpp/bgv_pr_dump.cpp) against the Hensel-lifting restatement tests/bgv_pr_ref.py; Ctxt.effectiveR / divideByP /
multByP / subDivideByP and helib_amd.bgv_pr (EncryptedArray, extractDigits) over the oracle backend with an injected CPU
encoder; the refusals; the declarations of the new C entries."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bgv_pr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PMAX = 46337        # the largest prime whose square is below 2^31
SHAPES = [(85, 2, 4), (127, 2, 3), (80, 3, 3), (64, 193, 2), (85, PMAX, 2)]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pr") / "bgv_pr_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "bgv_pr_dump.cpp"),
                           "-o", exe])

    def run(m, p, r, old=False, raw=False):
        out = subprocess.run([exe, str(m), str(p), str(r)] + (["old"] if old else []), capture_output=True, text=True,
                             timeout=120, check=True).stdout
        if raw:
            return out
        out = out.splitlines()
        head = out[0].split()
        if head[0] != "ok":
            return {"error": out[0][6:]}
        t = dict(zip(("m", "p", "r", "modulus", "d", "nslots", "phim", "ld", "limit"), map(int, head[1:])))
        t["gens"], t["ords"] = [int(x) for x in out[1].split()], [int(x) for x in out[2].split()]
        rows = [[int(x) for x in line.split()] for line in out[3:]]
        n = t["nslots"]
        t["F"], t["E"], t["R"] = rows[:n], rows[n:2 * n], rows[2 * n:3 * n]
        return t
    return run


def test_the_largest_prime_below_the_square_root_of_2_31():
    from helib_amd import hostnt
    assert PMAX ** 2 < 2 ** 31 and hostnt.is_prime(PMAX)
    assert not any(hostnt.is_prime(q) for q in range(PMAX + 1, 46341)) and 46341 ** 2 > 2 ** 31


@pytest.mark.parametrize("m,p,r", SHAPES)
def test_tables_against_the_hensel_restatement(dump, m, p, r):
    t, ref = dump(m, p, r), R.tables(m, p, r)
    P, n, phim, d = p ** r, ref.nslots, ref.phim, ref.d
    assert (t["p"], t["r"], t["modulus"], t["d"], t["nslots"], t["phim"]) == (p, r, P, d, n, phim)
    assert t["limit"] == min((1 << 64) // (P * P), 0xffffffff) and t["ld"] == (phim + 3) // 4 * 4
    assert (t["gens"], t["ords"]) == (ref.z.gens, ref.z.signedOrds())
    # the padding behind phi(m) is zero
    assert all(not any(row[phim:]) for row in t["E"] + t["R"])
    E, Rt = [row[:phim] for row in t["E"]], [row[:phim] for row in t["R"]]
    # word for word: the factors (the Hensel lifts, in the order found modulo p), E and R
    assert t["F"] == ref.F
    assert E == ref.E
    assert Rt == ref.Rt
    # modulo p they are the r = 1 tables: the C++ ones and the polynomial restatement's
    t1 = dump(m, p, 1)
    assert [[x % p for x in row] for row in t["F"]] == t1["F"] == [[int(x) for x in f] for f in ref.base.F]
    assert [[x % p for x in row] for row in t["E"]] == t1["E"] and [[x % p for x in row] for row in E] == ref.base.E
    assert [[x % p for x in row] for row in t["R"]] == t1["R"]
    # E_i^2 = E_i, E_i E_j = 0, sum E_i = 1 modulo (Phi_m, p^r)
    for i in range(n):
        for j in range(i, n):
            prod = R.mulmod(E[i], E[j], ref.phi, P)
            assert prod == (E[i] if i == j else [0] * phim), (i, j)
    assert [sum(col) % P for col in zip(*E)] == [1] + [0] * (phim - 1)
    # R E^T = I modulo p^r
    RE = np.array(Rt, dtype=object).dot(np.array(E, dtype=object).T) % P
    assert np.array_equal(RE, np.eye(n, dtype=object))


def test_the_mid_loop_reduction_runs_at_the_largest_modulus(dump):
    t = dump(85, PMAX, 2)
    assert t["limit"] == 4 and t["nslots"] == 4 and t["phim"] == 64     # a decode row holds 16 times the terms of one interval


@pytest.mark.parametrize("m,p", [(85, 2), (31, 3), (64, 193), (64, 2147483647)])
def test_r1_is_byte_identical_to_the_two_argument_call(dump, m, p):
    new, old = dump(m, p, 1, raw=True), dump(m, p, 1, old=True, raw=True)
    assert new == old and new.startswith("ok %d %d 1 %d " % (m, p, p))


def test_limits_are_refused_with_the_figure(dump):
    assert "less than 1" in dump(85, 2, 0)["error"]
    e = dump(85, 2, 31)["error"]
    assert "2^31" in e and "2^31 = 2147483648" in e and "2^31" in dump(85, 46349, 2)["error"]
    assert "modulus" in dump(85, 2, 30) and dump(85, 2, 30)["modulus"] == 2 ** 30
    assert "prime" in dump(85, 15, 2)["error"] and "divides" in dump(51, 3, 2)["error"]


# ---- Ctxt members and bgv_pr over the oracle backend with a CPU encoder ----
class _Setup:
    def __init__(self, m, p, r, seed=3, bits=300):
        from oracle import oracle as O
        from oracle.backend import OracleBackend, OracleOps, OPoly
        from helib_amd import bgv_pr, ctxt as hc, keys as hk
        self.m, self.p, self.r, self.P = m, p, r, p ** r
        cc = self.cc = hc.ChainContext(m, p, r, bits=bits, c=2)
        o = O.Ctx(m)
        for q in cc.primes:
            o.add_prime(q)
        calls = self.calls = []

        class Ops(OracleOps):
            """the oracle's ops with hx_scaled_sub stated in python integers"""

            def scaledSub(self, c0, c1, t0, t1, u, v):
                calls.append((list(u), list(v)))
                for c, t in ((c0, t0), (c1, t1)):
                    if c is None:
                        continue
                    assert isinstance(c, OPoly) and c.idx == t.idx and c is not t
                    for row, i in enumerate(c.idx):
                        q = o.primes[i]
                        assert 0 <= u[row] < q and 0 <= v[row] < q
                        c.rows[row] = np.array([(int(x) * u[row] - int(y) * v[row]) % q for x, y in zip(c.rows[row], t.rows[row])],
                                               dtype=np.uint64)

        class Backend(OracleBackend):
            def fromCoeffsBatch(self, idx, polys):
                assert len(polys) == 1
                d = self.fromCoeffs(idx, polys[0])
                d.batch = 1
                return d
        be = self.be = Backend(o, cc)
        be.ops = Ops(o)
        ref = self.ref = R.tables(m, p, r)
        P = self.P

        class Enc:
            def dims(self):
                return ref.z.gens, ref.z.signedOrds()

            def encode(self, v, mul, idx, coeffs=False):
                cf = ref.encode(v, mul)
                d = None
                if idx:
                    assert cf.shape[0] == 1, "the CPU backend takes one vector at a time"
                    d = be.fromCoeffs(idx, [int(x) for x in cf[0]])
                    d.batch = 1
                return (d, cf) if coeffs else d

            def embed(self, coeffs):
                return ref.decode(coeffs)

            def decode(self, acc, factor_inv):
                return ref.decode([[int(x) % P * factor_inv % P for x in be.toPoly(acc)]])

            def norm(self, coeffs):
                return np.array([be.embeddingLargestCoeff(row) for row in np.atleast_2d(coeffs)])
        self.sk = hk.SecKey(cc, be, seed=seed)
        self.sk.GenSecKey()
        self.ea = bgv_pr.EncryptedArray(cc, None, encoder=Enc())
        self.sk.zMStar = self.ea.zMStar
        hk.add1DMatrices(self.sk)

    def slots(self, seed):
        return np.random.default_rng(seed).integers(0, self.P, size=(1, self.ea.size()))


@pytest.fixture(scope="module")
def s2():
    return _Setup(85, 2, 4)


@pytest.fixture(scope="module")
def s3():
    return _Setup(80, 3, 3)


def _state(ct):
    return ({h: p.rows.copy() for h, p in ct.parts.items()}, {h: list(p.idx) for h, p in ct.parts.items()},
            ct.lnNoise, ct.primeSet, ct.ptxtSpace, ct.intFactor)


def _same(a, b):
    assert a[1:] == b[1:]
    assert a[0].keys() == b[0].keys() and all(np.array_equal(a[0][h], b[0][h]) for h in a[0])


def test_encode_encrypt_and_arithmetic_modulo_p_r(s2):
    ea, sk, P = s2.ea, s2.sk, s2.P
    assert (ea.getP(), ea.getPPowR(), ea.size(), ea.getDegree()) == (2, 16, 8, 8)
    a, b, c = s2.slots(1), s2.slots(2), s2.slots(3)
    assert np.array_equal(ea.decode(ea.encodeCoeffs(a)), a)
    big = np.array([[2 ** 63 - 1, -2 ** 63, -1, 17, 0, 5, -16, 31]])
    assert np.array_equal(ea.decode(ea.encodeCoeffs(big)), big % P)
    ct = ea.encrypt(sk, a[0])
    assert ct.ptxtSpace == P and ct.effectiveR() == 4
    assert np.array_equal(ea.decrypt_batch(ct, sk), a)
    ct.multiplyBy(ea.encrypt(sk, b[0]))
    ct += ea.encrypt(sk, c[0])
    assert np.array_equal(ea.decrypt_batch(ct, sk), (a * b + c) % P)
    ea.multByConstant(ct, ea.encodePtxt(b))
    ea.addConstant(ct, ea.encodePtxt(c))
    assert np.array_equal(ea.decrypt_batch(ct, sk), ((a * b + c) * b + c) % P)
    # the linear array with masks encoded mod p^r, over the non-native dimension of m = 85
    assert not ea.nativeDimension(0)
    ct = ea.encrypt(sk, a[0])
    ea.rotate(ct, 3)
    assert np.array_equal(ea.decrypt_batch(ct, sk), np.roll(a, 3, axis=1))
    ct = ea.encrypt(sk, a[0])
    ea.shift(ct, 2)
    assert np.array_equal(ea.decrypt_batch(ct, sk)[0], np.concatenate([[0, 0], a[0, :-2]]))
    ct = ea.encrypt(sk, a[0])
    ea.totalSums(ct)
    assert np.array_equal(ea.decrypt_batch(ct, sk)[0], np.full(8, a.sum() % P))


@pytest.mark.parametrize("which", ["s2", "s3"])
def test_effective_r_mult_by_p_and_divide_by_p(which, request):
    import math
    s = request.getfixturevalue(which)
    ea, sk, p, P, r = s.ea, s.sk, s.p, s.P, s.r
    a = s.slots(5) % (P // p)
    ct = ea.encrypt(sk, a[0])
    if p == 3:
        ct.multByScalar(2)                       # a unit: it moves into intFactor
        assert ct.intFactor != 1
        a = a * 2 % P
    ct.ptxtSpace = P // p                        # the slots are below p^(r-1): the same ciphertext in the smaller space
    ct.intFactor %= ct.ptxtSpace
    assert ct.effectiveR() == r - 1
    before = _state(ct)
    # multByP (include/helib/Ctxt.h:1216-1221): the space grows, multByConstant(p) multiplies by the balanced gcd
    ct.multByP()
    assert ct.ptxtSpace == P and ct.effectiveR() == r and ct.primeSet == before[3]
    assert ct.intFactor == before[5]             # p = p * 1: the unit part is 1
    assert ct.lnNoise == before[2] + math.log(p)
    assert np.array_equal(ea.decrypt_batch(ct, sk), a % (P // p) * p % P)
    # divideByP (src/Ctxt.cpp:2415-2435): parts times p^-1 mod Q, noise / p, space / p, intFactor reduced
    mid = _state(ct)
    Q = s.cc.productOfPrimes(ct.primeSet)
    ct.divideByP()
    assert ct.ptxtSpace == P // p and ct.intFactor == mid[5] % (P // p) and ct.primeSet == mid[3]
    assert ct.lnNoise == mid[2] - math.log(p)
    pinv = pow(p, -1, Q)
    for h, part in ct.parts.items():
        for row, i in enumerate(part.idx):
            q = s.cc.primes[i]
            assert np.array_equal(part.rows[row], np.array([int(x) * pinv % q for x in mid[0][h][row]], dtype=np.uint64))
    assert np.array_equal(ea.decrypt_batch(ct, sk), a % (P // p))
    _same((_state(ct)[0],) + _state(ct)[3:], (before[0],) + before[3:])     # p * p^-1 = 1 modulo every prime
    # the two asserts are errors; effectiveR refuses a space that is no power of p
    low = ea.encrypt(sk, a[0])
    low.ptxtSpace = p
    with pytest.raises(RuntimeError, match="strictly greater"):
        low.divideByP()
    low.ptxtSpace = 5
    with pytest.raises(RuntimeError, match="must divide"):
        low.divideByP()
    with pytest.raises(RuntimeError, match="not of the form"):
        low.effectiveR()
    low.ptxtSpace = 2 * P
    if p != 2:
        with pytest.raises(RuntimeError, match="not of the form"):
            low.effectiveR()


@pytest.mark.parametrize("which", ["s2", "s3"])
def test_sub_divide_by_p_equals_the_two_calls(which, request):
    s = request.getfixturevalue(which)
    ea, sk, p, P = s.ea, s.sk, s.p, s.P
    a = s.slots(7)
    low = a % p
    cases = []
    # (1) fresh against fresh: equal intFactors and prime sets
    cases.append((ea.encrypt(sk, a[0]), ea.encrypt(sk, low[0]), (a - low) // p))
    # (2) unequal prime sets: the subtrahend went through a product and lives on another set
    one = ea.encrypt(sk, np.ones(ea.size(), dtype=np.int64))
    t = ea.encrypt(sk, low[0])
    t.multiplyBy(one)
    cases.append((ea.encrypt(sk, a[0]), t, (a - low) // p))
    assert t.primeSet != cases[-1][0].primeSet
    # (3) unequal intFactors (p odd: units move into intFactor), on top of unequal prime sets
    if p > 2:
        t = ea.encrypt(sk, low[0] * 2 % P)
        t.multByScalar(pow(2, -1, P))
        t.multiplyBy(one)
        c = ea.encrypt(sk, a[0] * 4 % P)
        c.multByScalar(pow(4, -1, P))
        assert len({t.intFactor, c.intFactor, 1}) == 3
        cases.append((c, t, (a - low) // p))
    # (4) a one-part pair
    c, t = ea.encrypt(sk, a[0]), ea.encrypt(sk, low[0])
    del c.parts["s"], t.parts["s"]
    cases.append((c, t, None))
    for c, t, want in cases:
        two, fused, t_before = c.clone(), c.clone(), _state(t)
        two -= t
        two.divideByP()
        n = len(s.calls)
        assert fused.subDivideByP(t, fused=True) is fused
        assert len(s.calls) == n + 1
        _same(_state(fused), _state(two))
        _same(_state(t), t_before)                                  # the subtrahend is left as it was
        assert fused.ptxtSpace == P // p
        if want is not None:
            assert np.array_equal(ea.decrypt_batch(fused, sk), want % (P // p))
        # the default is the two calls, and fused=False as well
        for kw in ({}, {"fused": False}):
            again = c.clone()
            again.subDivideByP(t, **kw)
            assert len(s.calls) == n + 1
            _same(_state(again), _state(two))
    # what cannot be fused runs as the two calls: three parts on one side
    c, t = ea.encrypt(sk, a[0]), ea.encrypt(sk, low[0])
    c.multLowLvl(one)
    c._materializeTensor()
    assert len(c.parts) == 3
    two = c.clone()
    two -= t
    two.divideByP()
    n = len(s.calls)
    c.subDivideByP(t, fused=True)
    assert len(s.calls) == n
    _same(_state(c), _state(two))


_replay = R.replay       # the loop of src/extractDigits.cpp:90-124 on plain integers (shared with the device tests)


def test_the_scaled_sub_reference_is_the_stand_in_of_the_oracle_backend(s3):
    """tests/bgv_pr_ref.scaled_sub (what the device tests hold hx_scaled_sub against) and Ops.scaledSub above (what the
    host tests run subDivideByP over) are one function: two parts and one, five of the chain's primes in another order
    than the context's, u and v with 0, 1 and q - 1 among them"""
    from oracle.backend import OPoly
    o, ops = s3.be.o, s3.be.ops
    idx = list(range(len(o.primes)))[::-1][:5]
    idx[1], idx[3] = idx[3], idx[1]
    qs = [o.primes[i] for i in idx]
    rng = np.random.default_rng(21)
    n = 32

    def rnd():
        x = np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in qs])
        x[0, :3] = [0, 1, qs[0] - 1]
        x[-1, -1] = qs[-1] - 1
        return x
    c0, c1, t0, t1 = rnd(), rnd(), rnd(), rnd()
    u = [0, 1, qs[2] - 1] + [int(rng.integers(0, q)) for q in qs[3:]]
    v = [int(rng.integers(0, q)) for q in qs[:2]] + [qs[2] - 1, 0, 1]
    want = [R.scaled_sub(c, t, u, v, qs) for c, t in ((c0, t0), (c1, t1))]
    assert all(0 <= int(x) < q for w in want for row, q in zip(w, qs) for x in row)
    # one row by hand
    assert int(want[0][2][5]) == (int(c0[2][5]) * (qs[2] - 1) - int(t0[2][5]) * (qs[2] - 1)) % qs[2]
    pc = [OPoly(o, idx, c0.copy()), OPoly(o, idx, c1.copy())]
    pt = [OPoly(o, idx, t0.copy()), OPoly(o, idx, t1.copy())]
    n_calls = len(s3.calls)
    ops.scaledSub(pc[0], pc[1], pt[0], pt[1], u, v)
    assert s3.calls[n_calls:] == [(u, v)]
    del s3.calls[n_calls:]
    for got, w in zip(pc, want):
        assert np.array_equal(got.rows, w.astype(np.uint64))
    assert np.array_equal(pt[0].rows, t0) and np.array_equal(pt[1].rows, t1)
    one = OPoly(o, idx, c0.copy())
    ops.scaledSub(one, None, pt[1], None, v, u)
    del s3.calls[n_calls:]
    assert np.array_equal(one.rows, R.scaled_sub(c0, t1, v, u, qs).astype(np.uint64))


@pytest.mark.parametrize("which,fused", [("s2", False), ("s3", False), ("s2", True), ("s3", True)])
def test_extract_digits_against_the_plain_integer_replay(which, fused, request):
    """bits = 300: with the bookkeeping run on the CPU first, every digit keeps more than 250 bits of capacity at both
    shapes (the digits are squared r - 1 = 3 times, or cubed twice)"""
    from helib_amd import bgv_pr
    s = request.getfixturevalue(which)
    ea, sk, p, r = s.ea, s.sk, s.p, s.r
    a = s.slots(11)
    a[0, :3] = [0, s.P - 1, s.P // 2]
    ct = ea.encrypt(sk, a[0])
    n = len(s.calls)
    digits = bgv_pr.extractDigits(ea, ct, fused=fused)
    assert len(s.calls) == n + (r * (r - 1) // 2 if fused else 0)
    want = _replay(a[0], p, r)
    assert len(digits) == r
    assert np.array_equal(ea.decrypt_batch(ct, sk), a)              # the input is left as it was
    x = [int(v) for v in a[0]]
    for j, d in enumerate(digits):
        assert d.ptxtSpace == p ** (r - j) == want[j][1] and d.effectiveR() == r - j
        assert d.bitCapacity() > 0 and d.isCorrect()
        got = ea.decrypt_batch(d, sk)[0]
        assert [int(v) for v in got] == [int(v) for v in want[j][0]], j
        if p == 2:
            assert [int(v) for v in got] == [(v >> j) & 1 for v in x], j
        else:                                                       # the balanced expansion: digits in {-1, 0, 1}
            bal = [(v + 1) % 3 - 1 for v in x]
            assert [int(v) % 3 for v in got] == [b % 3 for b in bal], j
            x = [(v - b) // 3 for v, b in zip(x, bal)]
    # r below the effective r: the first digits alone, in the same spaces
    some = bgv_pr.extractDigits(ea, ct, 2, fused=fused)
    assert [d.ptxtSpace for d in some] == [p ** r, p ** (r - 1)]
    assert [int(v) % p for v in ea.decrypt_batch(some[1], sk)[0]] == [int(v) % p for v in want[1][0]]


def test_fused_and_unfused_extraction_agree_in_words_and_bookkeeping(s3):
    from helib_amd import bgv_pr
    ea, sk = s3.ea, s3.sk
    ct = ea.encrypt(sk, s3.slots(13)[0])
    for x, y in zip(bgv_pr.extractDigits(ea, ct, fused=True), bgv_pr.extractDigits(ea, ct, fused=False)):
        _same(_state(x), _state(y))


def test_refusals():
    from helib_amd import bgv, bgv_crt, bgv_gf, bgv_gf_matmul, bgv_hypercube, bgv_matmul, bgv_pr, capi, ckks
    from helib_amd import ctxt as hc
    # p = 5 in extractDigits
    s5 = _Setup(31, 5, 2, bits=100)
    ct = s5.ea.encrypt(s5.sk, s5.slots(1)[0])
    assert np.array_equal(s5.ea.decrypt_batch(ct, s5.sk), s5.slots(1))
    with pytest.raises(ckks.LogicError, match="polyEval and buildDigitPolynomial"):
        bgv_pr.extractDigits(s5.ea, ct)
    # a ciphertext of another context, a space that is no p^k
    other = _Setup(31, 5, 2, bits=100, seed=4)
    with pytest.raises(ckks.LogicError, match="another context"):
        bgv_pr.extractDigits(other.ea, ct)
    ct.ptxtSpace = 125
    with pytest.raises(ckks.LogicError, match="1 <= k <= r"):
        s5.ea.decrypt_batch(ct, s5.sk)
    # the matrix products over the new class
    ea = s5.ea
    D = ea.sizeOfDimension(0)
    eye = np.eye(D, dtype=np.int64)
    for build in (lambda: bgv_matmul.MatMul1D(ea, eye, 0), lambda: bgv_matmul.MatMul1DExec(ea, eye, dim=0),
                  lambda: bgv_hypercube.MatMul1DExec(ea, eye, dim=0),
                  lambda: bgv_matmul.MatMulFullExec(ea, np.eye(ea.size(), dtype=np.int64)),
                  lambda: bgv_hypercube.MatMulFullExec(ea, np.eye(ea.size(), dtype=np.int64)),
                  lambda: bgv_gf_matmul.MatMul1D(ea, eye, 0), lambda: bgv_gf_matmul.BlockMatMul1D(ea, eye, 0)):
        with pytest.raises(ckks.LogicError, match="r > 1"):
            build()
    # the old classes at r = 2 still raise, GF(p^d) slots included
    cc = hc.ChainContext(85, 2, 2, bits=100, c=2)
    for cls in (bgv.EncryptedArray, bgv_crt.EncryptedArray, bgv_hypercube.EncryptedArray, bgv_gf.EncryptedArray):
        with pytest.raises(capi.HxError, match="r > 1") as e:
            cls(cc, None, encoder=object())
        assert e.value.code == capi.HX_ERR_UNSUPPORTED
    # a CKKS context, and a context whose space is not p^r
    with pytest.raises(ckks.LogicError, match="CKKS"):
        bgv_pr.EncryptedArray(hc.ChainContext(64, -1, 20, bits=100, c=2, ckks=True), None, encoder=object())
    cc.ptxtSpace = 8
    with pytest.raises(ckks.LogicError, match="not p\\^r"):
        bgv_pr.EncryptedArray(cc, None, encoder=object())


def test_at_r1_the_restatement_is_the_r1_restatement():
    from tests import bgv_crt_ref
    ref1, refr = bgv_crt_ref.tables(85, 2), R.tables(85, 2, 1)
    a = np.random.default_rng(2).integers(-9, 9, size=(3, 8))
    assert np.array_equal(refr.encode(a), ref1.encode(a))
    assert np.array_equal(refr.decode(refr.encode(a)), a % 2)
    assert refr.E == ref1.E and refr.F == [[int(x) for x in f] for f in ref1.F]


def test_scaled_sub_and_create_pr_are_declared_bound_and_exported():
    from helib_amd import bgv_pr, capi
    from helib_amd import ctxt as hc
    hdr = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    declared = set(re.findall(r"\b(hx_[a-zA-Z0-9_]+)\s*\(", hdr))
    lib = capi.lib()                      # the cross-compiled library
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi._SO], text=True)
    for name, nargs in (("hx_scaled_sub", 6), ("hx_bgv_crt_create_pr", 4), ("hx_bgv_crt_space", 3)):
        assert name in capi.SYMBOLS and name in declared, name
        assert len(getattr(lib, name).argtypes) == nargs
        assert re.search(r"\bT %s$" % name, out, re.M), name
    assert len(lib.hx_bgv_crt_create.argtypes) == 3 and len(lib.hx_bgv_crt_info.argtypes) == 8     # left alone
    for cite in ("src/extractDigits.cpp:106-107", "src/PAlgebra.cpp:757-763", ":2415-2435", "src/zzX.cpp:122-137"):
        assert cite in hdr, cite
    assert hasattr(capi, "scaledSub")
    with pytest.raises(capi.InvalidArgument, match="go together"):
        capi.scaledSub(None, None, None, object(), [], [])
    assert capi.BgvCrt.__init__.__defaults__ == (1,)
    for f in ("effectiveR", "divideByP", "multByP", "subDivideByP"):
        assert f in vars(hc.Ctxt)
    assert hc.Ctxt.fuseScaledSub is False
    for f in ("encrypt_batch", "decrypt_batch", "encodePtxt", "addConstant"):
        assert f in vars(bgv_pr.EncryptedArray)
    assert callable(bgv_pr.extractDigits)
