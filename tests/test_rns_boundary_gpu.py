"""The exact RNS kernels at planted boundary integers (tests/rns_boundary_ref.py), on the device.

Between two transforms the engine's arithmetic is exact except for decisions taken per coefficient on the integer the
residues stand for: the centring compare (garner_front, rns_extend_kernel, break_digits_kernel: mixed-radix digits
against P.half[k]; the single-prime prep store: x > P.half), the HPS quotient with its redo list (hps_front,
rns_extend_wide_kernel, rns_extend_mfma_kernel: floor and fraction of a double-precision sum, untrusted within
hps_eps of 0, 1/2 and 1) and the tie dm == ptxtSpace/2 && neg at an even plaintext space.  Uniform residues land
within 2^-30 of a boundary once in 2^28 coefficients, so every other device test leaves the redo list empty at the
default threshold and never meets a tie.  Here the boundary values are the coefficients: 0, +-1, +-2, the two
neighbours of P/2, values inside and just outside hps_eps of 0 and P/2, single-term sums, thirds as a control --
first in the polynomial, uniform filler behind, batch element 1 rotated by 37 coefficients.  Expected words come
from python integers (the C oracle is checked against the same expectation in test_rns_boundary_host.py, and is the
reference where the key switch follows); every output word is compared exactly, fdelta and norms within
atol = 1e-9 max(1, ptxt) / rtol = 1e-9, and the kernels that ran are asserted by name.  HX_HPS_EPS stays at its
default throughout: the point is the default threshold."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import rns_boundary_ref as R

pytestmark = pytest.mark.gpu

B = 2
TOL = 1e-9
MODULI = (7, 1000003)
MFMA, WIDE = "rns_extend_mfma_kernel", "rns_extend_wide_kernel<"


@pytest.fixture(scope="module")
def hx():
    try:
        import torch  # noqa: F401   (before this library touches the device: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import capi
    if capi.device_count() <= 0:
        pytest.skip("no HIP device: the GPU boundary tests run on an MI355X (pytest -m gpu)")
    return capi


class Pair:
    """A device context and an oracle context with the same primes/roots (created under the current environment)."""

    def __init__(self, hx, m, primes):
        self.g = hx.Context(m)
        self.o = O.Ctx(m)
        for q in primes:
            i = self.o.add_prime(q)
            assert self.g.add_prime(q, self.o.roots[i]) == i
        self.m, self.N, self.primes = m, self.o.N, list(primes)

    def ps(self, idx):
        return [self.primes[i] for i in idx]

    def rand(self, idx, seed, batch=B):
        return np.stack([np.stack([O.fill_uniform(self.N, self.primes[i], seed * 100003 + i * 131 + b)
                                   for b in range(batch)]) for i in idx])


def kernels_of(hx, fn):
    hx.profileBegin()
    out = fn()
    return out, " | ".join(sorted(k["kernel"] for k in hx.profileEnd()["kernels"]))


def check_names(names, must, must_not=()):
    for piece in must:
        assert piece in names, (piece, names)
    for piece in must_not:
        assert piece not in names, (piece, names)


def blame(P, idx, got_eval, want_coef, values, ps, ptxt):
    """which planted classes the differing coefficients belong to (for the assertion message)"""
    diff = (P.o.ifft(idx, got_eval) != want_coef).any(axis=0)
    where = np.nonzero(diff)[0]
    return {"coefficients": where[:8].tolist(), "count": int(diff.sum()),
            "classes": sorted({R.class_of(values[i], ps, ptxt) or "filler" for i in where})}


# ---------------------------------------------------------------- the operations
def run_add_primes(hx, P, src, tgt, seed):
    """addPrimes onto tgt and toPolyMod(7 / 1000003) of the planted values; returns the kernel names of each"""
    ps, ts = P.ps(src), P.ps(tgt)
    k_rem = k_add = ""
    for batch in R.extension_inputs(ps, 4, P.N, seed):
        rows = R.eval_rows(P.o, src, batch)
        d = hx.DoubleCRT(P.g, src, B, rows)
        rems, k_rem = kernels_of(hx, lambda: [d.toPolyMod(t) for t in MODULI])
        _, k_add = kernels_of(hx, lambda: d.addPrimes(tgt))
        got = d.download()
        assert d.getIndexSet() == src + tgt
        for b, coef in enumerate(batch):
            want = R.want_add_primes(coef, ps, ts)
            assert np.array_equal(got[:len(src), b], rows[:, b])
            assert np.array_equal(got[len(src):, b], P.o.fft(tgt, want)), blame(P, tgt, got[len(src):, b], want, coef, ps, 4)
            centred = R.want_to_poly(coef, ps)
            for t, rem in zip(MODULI, rems):
                bad = [i for i, v in enumerate(centred) if int(rem[b, i]) != v % t]
                assert not bad, (t, b, bad[:8], sorted({R.class_of(coef[i], ps, 4) or "filler" for i in bad}))
    return k_add, k_rem


def run_scale_down(hx, P, own, drop, seed, ptxts=((65537, 1), (4, 1), (2, 1), (1, 1), (2, 2))):
    """scaleDownToSetMulti(fdelta, norms) dropping `drop`, delta running over the planted values; (ptxt, parts) pairs"""
    own_ps, drop_ps = P.ps(own), P.ps(drop)
    keep = [i for i in own if i not in drop]
    pos = [own.index(i) for i in drop]
    Pd = R.prod(drop_ps)
    names = ""
    for ptxt, nparts in ptxts:
        per_part = [R.scale_down_inputs(drop_ps, P.ps(keep), ptxt, P.N, seed + 7 * k) for k in range(nparts)]
        for parts in zip(*per_part):
            polys = [hx.DoubleCRT(P.g, own, B, R.eval_rows(P.o, own, x)) for x in parts]
            (nrm, fd), names = kernels_of(hx, lambda: hx.scaleDownToSetMulti(polys, keep, ptxt, norms=True, fdelta=True))
            for k, (x, d) in enumerate(zip(parts, polys)):
                gi, got = d.getIndexSet(), d.download()
                assert sorted(gi) == sorted(keep)
                for b, coef in enumerate(x):
                    want, wfd = R.want_scale_down(coef, own_ps, pos, ptxt)
                    order = [keep.index(i) for i in gi]
                    assert np.array_equal(got[:, b], P.o.fft(gi, want[order])), \
                        (ptxt, k, b, blame(P, gi, got[:, b], want[order], [c % Pd for c in coef], drop_ps, ptxt))
                    err = np.abs(fd[k, b] - wfd)
                    worst = int(np.argmax(err - TOL * np.abs(wfd)))
                    assert np.allclose(fd[k, b], wfd, rtol=TOL, atol=TOL * max(1.0, float(ptxt))), \
                        (ptxt, k, b, worst, fd[k, b, worst], wfd[worst], R.class_of(coef[worst] % Pd, drop_ps, ptxt))
                    assert np.isclose(nrm[k, b], O.embedding_largest_coeff(P.m, wfd), rtol=TOL), (ptxt, k, b)
    return names


def run_break(hx, P, own, digits, sp, seed):
    """breakIntoDigits with norms, the planted class on each digit in turn (the later ones are what the in-place fix-up
    digits[j] -= digits[i]; digits[j] /= P_i leaves)"""
    own_ps, allp = P.ps(own), own + sp
    dps = [P.ps(d) for d in digits]
    dpos = [[own.index(i) for i in d] for d in digits]
    names = []
    for which in range(len(digits)):
        for batch in R.digit_inputs(dps, which, P.N, seed + which):
            d = hx.DoubleCRT(P.g, own, B, R.eval_rows(P.o, own, batch))
            (dg, nr), k = kernels_of(hx, lambda: d.breakIntoDigits(digits, sp, norms=True))
            names.append(k)
            got = dg.download()
            for b, coef in enumerate(batch):
                want, frac, digs = R.want_digits(coef, own_ps, dpos, P.ps(allp))
                gb = got[:, b].reshape(len(digits), len(allp), P.N)
                for j in range(len(digits)):
                    assert np.array_equal(gb[j], P.o.fft(allp, want[j])), \
                        (digits, which, j, b, blame(P, allp, gb[j], want[j], digs[j], dps[j], 4))
                    assert np.isclose(nr[j, b], O.embedding_largest_coeff(P.m, frac[j]), rtol=TOL), (digits, which, j, b)
    return " | ".join(names)


def oracle_relin(P, own, sp, digits, t0, t1, t2, kb, ka):
    allp = own + sp
    pad = np.zeros((len(sp), P.N), dtype=np.uint64)
    o0 = np.vstack([P.o.scale_by_primes(own, t0, sp), pad])
    o1 = np.vstack([P.o.scale_by_primes(own, t1, sp), pad])
    return P.o.key_switch_digits(allp, P.o.break_into_digits(own, t2, digits, allp), kb, ka, o0, o1)


def run_relin(hx, P, own, digits, sp, seed, mul):
    """reLinearize (norms) with the planted polynomial as the s^2 part, each digit in turn; mul: also hx_mul_relin
    with c1 = the planted polynomial and d1 = the constant 1, so that t2 = c1 d1 is the planted polynomial.  Words
    against the oracle (its digits are checked against python integers on the CPU), norms against python integers."""
    own_ps, allp, D = P.ps(own), own + sp, len(digits)
    dps = [P.ps(d) for d in digits]
    dpos = [[own.index(i) for i in d] for d in digits]
    kb = np.stack([P.rand(allp, seed + 20 + i, 1)[:, 0] for i in range(D)])
    ka = np.stack([P.rand(allp, seed + 30 + i, 1)[:, 0] for i in range(D)])
    W = hx.KeySwitch(P.g, allp, kb, ka)
    x0, x1 = P.rand(own, seed + 1), P.rand(own, seed + 2)
    ones = np.ones_like(x0)
    names = []
    for which in range(D):
        for batch in R.digit_inputs(dps, which, P.N, seed + which):
            x2 = R.eval_rows(P.o, own, batch)
            t0, t1, t2 = (hx.DoubleCRT(P.g, own, B, x) for x in (x0, x1, x2))
            (o0, o1, nr), k = kernels_of(hx, lambda: hx.reLinearize(t0, t1, t2, W, digits, sp, norms=True))
            names.append(k)
            assert o0.getIndexSet() == allp == o1.getIndexSet()
            g0, g1 = o0.download(), o1.download()
            if mul:
                one = hx.DoubleCRT(P.g, own, B, ones)
                (p0, p1), k = kernels_of(hx, lambda: hx.multiplyBy(t0, t2, t1, one, W, digits))
                names.append(k)
                m0, m1 = p0.download(), p1.download()
            for b, coef in enumerate(batch):
                w0, w1 = oracle_relin(P, own, sp, digits, x0[:, b], x1[:, b], x2[:, b], kb, ka)
                assert np.array_equal(g0[:, b], w0) and np.array_equal(g1[:, b], w1), (digits, which, b)
                _, frac, _ = R.want_digits(coef, own_ps, dpos, [])
                for j in range(D):
                    assert np.isclose(nr[j, b], O.embedding_largest_coeff(P.m, frac[j]), rtol=TOL), (digits, which, j, b)
                if mul:
                    v0, v1 = P.o.mul_relin(own, sp, digits, x0[:, b], x2[:, b], x1[:, b], ones[:, b], kb, ka)
                    assert np.array_equal(m0[:, b], v0) and np.array_equal(m1[:, b], v1), ("mul_relin", digits, which, b)
    return " | ".join(names)


# ---------------------------------------------------------------- which kernels launch_extend chooses
def extension_kernels(n, env, in_place=False):
    """(must, must_not) name pieces for an extension from n 60-bit sources onto targets above 2^32 (engine.hip:
    launch_extend).  in_place: a launch that also updates rows in place (breakIntoDigits) has no HPS form below 17 sources."""
    hps_min = 2 if "HX_HPS_MIN_N" in env else 9
    fast_g, fast_h = "rns_extend_fast_kernel<%d, false>" % n, "rns_extend_fast_kernel<%d, true>" % n
    if n > 40:
        return ["rns_extend_kernel<64>"], [MFMA, WIDE]
    if n > 16:
        if "HX_NO_MFMA_EXT" in env:
            return [WIDE, "rns_extend_kernel<40>"], [MFMA]
        return [MFMA, "rns_extend_kernel<40>"], [WIDE]
    if n < 2 or in_place:
        return [fast_g], [fast_h, MFMA]
    if n >= 9 and "HX_NO_MFMA_EXT" not in env:
        return [MFMA, fast_g], [fast_h]
    if n >= hps_min:
        return [fast_h, fast_g], [MFMA]
    return [fast_g], [fast_h, MFMA]


def generic_kernel(n):
    return "rns_extend_kernel<%d>" % (8 if n <= 8 else 16 if n <= 16 else 40 if n <= 40 else 64)


def digit_kernels(sizes, env, lazy):
    """break_digits_fused's choice for digits of these sizes (all primes 60-bit, ascending)"""
    z = "true" if lazy else "false"
    brk_min = 2 if "HX_HPS_MIN_N" in env else 5
    if max(sizes) > 8:
        return ["break_digits_kernel<16>"], ["break_digits_fast_kernel<"]
    if min(sizes) >= max(2, brk_min):
        return ["break_digits_fast_kernel<true, %s>" % z, "break_digits_fast_kernel<false, %s>" % z], []
    return ["break_digits_fast_kernel<false, %s>" % z], ["break_digits_fast_kernel<true"]


def setenv(monkeypatch, env):
    for k in ("HX_HPS_MIN_N", "HX_NO_MFMA_EXT", "HX_NO_PROTH_RNS", "HX_NO_PREP_FUSE", "HX_HPS_EPS", "HX_MFMA_MIN_N"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


HPS2, VALU, SHOUP = {"HX_HPS_MIN_N": "2"}, {"HX_NO_MFMA_EXT": "1"}, {"HX_NO_PROTH_RNS": "1"}
CASES = ([(1, {})] + [(n, e) for n in (2, 3, 5, 8) for e in ({}, HPS2)]
         + [(n, e) for n in (9, 11, 16) for e in ({}, VALU, SHOUP)] + [(n, e) for n in (17, 24, 40) for e in ({}, VALU)]
         + [(44, {})])
IDS = ["%d%s" % (n, "".join("-" + k[3:].lower() for k in e)) for n, e in CASES]


# ---------------------------------------------------------------- m = 256: n 60-bit sources onto 60- / 56- / 45-bit targets
@pytest.mark.parametrize("n,env", CASES, ids=IDS)
def test_add_primes_and_to_poly_at_planted_values(hx, monkeypatch, n, env):
    """addPrimes from the n sources onto eleven targets of three sizes, and toPolyMod(7), toPolyMod(1000003) (a target
    below 2^32: the generic rns_extend_kernel<8/16/40/64>, whose plan fast16_ok refuses whatever the sources are)."""
    setenv(monkeypatch, env)
    P = Pair(hx, 256, R.many_source_chain(O, n, 256))
    k_add, k_rem = run_add_primes(hx, P, list(range(n)), list(range(n, n + 11)), 100 + n)
    check_names(k_add, *extension_kernels(n, env))
    check_names(k_rem, [generic_kernel(n)], [MFMA, WIDE, "rns_extend_fast_kernel"])


@pytest.mark.parametrize("n,env", CASES[:-1], ids=IDS[:-1])
def test_scale_down_at_planted_values(hx, monkeypatch, n, env):
    """scaleDownToSetMulti dropping the n sources at ptxtSpace 65537, 4, 2 and 1 with fdelta and norms, and two parts in
    one call: delta runs over the planted values, so x = +-1 is the tie dm == ptxt/2 on both signs at ptxtSpace 2
    (+-2 and +-6 at 4), and fdelta = -+1/2 there."""
    setenv(monkeypatch, env)
    P = Pair(hx, 256, R.many_source_chain(O, n, 256))
    names = run_scale_down(hx, P, list(range(n + 11)), list(range(n)), 200 + n)
    check_names(names, *extension_kernels(n, env))


@pytest.mark.parametrize("n,env", CASES[:-1], ids=IDS[:-1])
def test_break_into_digits_at_planted_values(hx, monkeypatch, n, env):
    """breakIntoDigits (norms) with an n-prime digit next to a 4-prime digit, in both orders, the planted class on each
    digit in turn: the launches update the later digit's rows in place."""
    setenv(monkeypatch, env)
    P = Pair(hx, 256, R.many_source_chain(O, n, 256))
    src, four, sp = list(range(n)), list(range(n, n + 4)), list(range(n + 4, n + 11))
    for k, digits in enumerate(([src, four], [four, src])):
        names = run_break(hx, P, src + four, digits, sp, 300 + n + 10 * k)
        check_names(names, *extension_kernels(n, env, in_place=True))
        check_names(names, ["rns_extend_fast_kernel<4, false>"])


@pytest.mark.parametrize("n,env", [c for c in CASES if 2 <= c[0] <= 40], ids=[i for c, i in zip(CASES, IDS) if 2 <= c[0] <= 40])
def test_relinearize_digit_kernels_at_planted_values(hx, monkeypatch, n, env):
    """reLinearize on the small ring with the planted polynomial as the s^2 part: the one-pass digit kernels
    (break_digits_fast_kernel in its Garner and HPS + redo forms up to 8 primes per digit, break_digits_kernel<16> from
    9 to 16, the per-digit extension launches beyond).  Digits: n primes next to 5 (both at or above the digit
    kernel's HPS threshold from n = 5 on), both orders."""
    setenv(monkeypatch, env)
    P = Pair(hx, 256, R.many_source_chain(O, n, 256))
    src, five, sp = list(range(n)), list(range(n, n + 5)), list(range(n + 5, n + 11))
    for k, digits in enumerate(([src, five], [five, src])):   # (the one-pass kernels want the digits to tile the rows in order)
        names = run_relin(hx, P, digits[0] + digits[1], digits, sp, 400 + n + 10 * k, mul=False)
        if n <= 16:
            check_names(names, *digit_kernels([n, 5], env, lazy=False))
        else:
            check_names(names, *extension_kernels(n, env, in_place=True))


# ---------------------------------------------------------------- the digit shapes of the existing tests
SHAPES = [[[0, 1], [2, 3], [4]], [[0, 1, 2, 3, 4]], [[0], [1, 2, 3], [4, 5]], [[0, 1], [2, 3], [4, 5]]]


@pytest.mark.parametrize("hps2", [False, True], ids=["default", "hps_min_n=2"])
@pytest.mark.parametrize("digits", SHAPES, ids=["2_2_1", "5", "1_3_2", "2_2_2"])
def test_digit_shapes_at_planted_values(hx, monkeypatch, digits, hps2):
    """breakIntoDigits with norms on the shapes of test_break_into_digits / test_proth_form_of_the_fast_rns_kernels,
    the planted class on every digit in turn."""
    setenv(monkeypatch, HPS2 if hps2 else {})
    L = sum(len(d) for d in digits)
    g60, g56 = O.PrimeGen(60, 256), O.PrimeGen(56, 256)
    P = Pair(hx, 256, [g60.next() for _ in range(L)] + [g56.next() for _ in range(2)])
    names = run_break(hx, P, list(range(L)), digits, [L, L + 1], 500 + L)
    check_names(names, ["rns_extend_fast_kernel<%d, false>" % len(d) for d in digits], [MFMA, WIDE])


@pytest.mark.parametrize("hps2", [False, True], ids=["default", "hps_min_n=2"])
@pytest.mark.parametrize("digits", SHAPES, ids=["2_2_1", "5", "1_3_2", "2_2_2"])
def test_relinearize_and_mul_relin_lazy_digit_kernels(hx, monkeypatch, digits, hps2):
    """hx_relinearize and hx_mul_relin at m = 16384, where the digit kernels leave their extension words unreduced for
    the forward transform (break_digits_fast_kernel<., true>): t2 = the planted polynomial (c1 = planted, d1 = 1 for
    the fused multiply), against O.Ctx.mul_relin / the oracle's digits and key switch."""
    env = HPS2 if hps2 else {}
    setenv(monkeypatch, env)
    m = 16384
    L = sum(len(d) for d in digits)
    g60, g56 = O.PrimeGen(60, m), O.PrimeGen(56, m)
    P = Pair(hx, m, [g60.next() for _ in range(L)] + [g56.next() for _ in range(2)])
    names = run_relin(hx, P, list(range(L)), digits, [L, L + 1], 600 + L, mul=True)
    check_names(names, *digit_kernels([len(d) for d in digits], env, lazy=True))


# ---------------------------------------------------------------- one dropped prime: the prep store's x > P.half
@pytest.mark.parametrize("no_fuse", [False, True], ids=["fused", "HX_NO_PREP_FUSE"])
def test_single_prime_mod_switch_at_planted_values(hx, monkeypatch, no_fuse):
    """One dropped prime at m = 16384: S = [x > (qd - 1)/2] + the balanced correction formed in the prep kernel's store
    (moddown_S_of), or by moddown_S_kernel under HX_NO_PREP_FUSE=1.  ptxtSpace 65537, 4, 2, 1 and 2^40 (the wide
    correction; its tie is delta = +-2^39), the dropped row last, in the middle and first."""
    setenv(monkeypatch, {"HX_NO_PREP_FUSE": "1"} if no_fuse else {})
    m = 16384
    g60 = O.PrimeGen(60, m)
    P = Pair(hx, m, [g60.next() for _ in range(4)])
    own = [0, 1, 2, 3]
    for k, drop in enumerate(([3], [1], [0])):
        ptxts = ((65537, 1), (4, 1), (2, 2), (1, 1), (1 << 40, 1)) if k == 0 else ((2, 1),)
        names = run_scale_down(hx, P, own, drop, 700 + k, ptxts)
        check_names(names, ["ntt_moddown_prep_kernel<"], ["rns_extend"])
        assert ("moddown_S_kernel" in names) == no_fuse, names


# ---------------------------------------------------------------- tensor product folded into the mod-switch
DROPS = {"add1_drop1": ([5], [2]), "drop1": ([], [1]), "drop_last": ([], [4]), "add1_drop2": ([5], [1, 3]),
         "drop2": ([], [0, 4]), "drop3": ([], [1, 2, 4])}


@pytest.mark.parametrize("with_s2", [False, True], ids=["d1=0", "d1=1"])
@pytest.mark.parametrize("shape", list(DROPS))
def test_tensor_bring_to_set_at_planted_values(hx, shape, with_s2):
    """hx_tensor_bring_to_set with d0 = 1, d1 = 0, c0 = X, c1 = Y (t0 = X, t1 = Y, t2 = 0; d1 = 1: t1 = X + Y, t2 = Y)
    at the drop shapes of test_tensor_folded_into_the_mod_switch: X and Y stand for the planted values on the dropped
    primes AFTER the mod-up (the operands carry F^-1, F the added prime), ptxtSpace 2, 4 and 65537; against the oracle's
    tensor product, addPrimesAndScale and scaleDownToSet, which test_rns_boundary_host.py holds to python integers."""
    m = 16384
    g60 = O.PrimeGen(60, m)
    P = Pair(hx, m, [g60.next() for _ in range(7)])
    own = [0, 1, 2, 3, 4]
    add, drop = DROPS[shape]
    keep = [i for i in own + add if i not in drop]
    Q, F = R.prod(P.ps(own)), R.prod(P.ps(add))
    Finv = pow(F, -1, Q)
    one, zero = np.ones((5, B, P.N), dtype=np.uint64), np.zeros((5, B, P.N), dtype=np.uint64)
    for ptxt in (2, 4, 65537):
        xs = [R.scale_down_inputs(P.ps(drop), P.ps([i for i in own if i not in drop]), ptxt, P.N, 800 + s)[0] for s in (0, 1)]
        ops = [R.eval_rows(P.o, own, [[c * Finv % Q for c in coef] for coef in x]) for x in xs]
        c0, c1 = (hx.DoubleCRT(P.g, own, B, x) for x in ops)
        d0, d1 = hx.DoubleCRT(P.g, own, B, one), hx.DoubleCRT(P.g, own, B, one if with_s2 else zero)
        (fused, nf), names = kernels_of(hx, lambda: hx.tensorBringToSet(c0, c1, d0, d1, add, keep, ptxt, norms=True))
        if len(drop) == 1:
            check_names(names, ["ntt_moddown_prep_tensor_kernel<"], ["rns_extend"])
        else:
            check_names(names, ["rns_extend_fast_kernel<%d, false>" % len(drop)])
        for b in range(B):
            w = P.o.tensor(own, ops[0][:, b], ops[1][:, b], one[:, b], (one if with_s2 else zero)[:, b])
            for part in range(3):
                up = w[part]
                if add:
                    up = np.vstack([P.o.scale_by_primes(own, up, add), np.zeros((len(add), P.N), dtype=np.uint64)])
                want, wfd = P.o.scale_down(own + add, up, drop, ptxt, want_fdelta=True)
                gi, gd = fused[part].getIndexSet(), fused[part].download()
                assert sorted(gi) == sorted(keep)
                for r, i in enumerate(gi):
                    assert np.array_equal(gd[r, b], want[keep.index(i)]), (ptxt, part, i, b)
                assert np.isclose(nf[part, b], O.embedding_largest_coeff(m, wfd), rtol=TOL), (ptxt, part, b)


# ---------------------------------------------------------------- mixed prime sizes, plans the fast kernels refuse, general m
@pytest.mark.parametrize("env", [{}, HPS2, SHOUP], ids=["default", "hps_min_n=2", "no_proth_rns"])
def test_mixed_prime_sizes_at_planted_values(hx, monkeypatch, env):
    """The chain of test_proth_form_of_the_fast_rns_kernels: a 38-bit prime that is not of Proth form as a source next
    to 60-bit ones (Shoup Garner steps, targets of both kinds) and as a target of all-Proth sources (both reductions
    in one launch)."""
    setenv(monkeypatch, env)
    P = Pair(hx, 256, R.mixed_chain(O, 256))
    for src, tgt in (([0, 1, 2], [3, 4, 6]), ([1, 2, 3], [0, 4, 6])):
        k_add, _ = run_add_primes(hx, P, src, tgt, 900 + src[0])
        check_names(k_add, *extension_kernels(3, env))
    for drop in ([0, 5], [1, 2, 3]):
        run_scale_down(hx, P, list(range(6)), drop, 910 + drop[0], ((65537, 1), (2, 1), (4, 1)))
    for digits in ([[0, 1], [2, 3], [4, 5]], [[0], [1, 2, 3], [4, 5]]):
        run_break(hx, P, list(range(6)), digits, [6, 7], 920 + len(digits[0]))
        names = run_relin(hx, P, list(range(6)), digits, [6, 7], 930 + len(digits[0]), mul=False)
        check_names(names, *digit_kernels([len(d) for d in digits], env, lazy=False))


def test_plans_the_fast_kernels_refuse(hx):
    """Sources the fast kernels' Garner form does not take -- a 38-bit prime BEHIND two 60-bit ones in one digit: neither
    ascending nor within a factor of two, so garner_cs, fast_ok and fast16_ok are all off -- reach rns_extend_kernel<8>
    and break_digits_kernel<8> with primes a chain may hold.  (<16> of either kernel needs no such chain: a target
    below 2^32 and a digit of 9 to 16 primes do it, in the cases above.)"""
    m = 256
    g60, g56 = O.PrimeGen(60, m), O.PrimeGen(56, m)
    q38 = O.PrimeGen(38, m).next()
    a, b = g60.next(), g60.next()
    P = Pair(hx, m, [a, b, q38] + [g60.next() for _ in range(2)] + [g56.next() for _ in range(2)])
    k_add, k_rem = run_add_primes(hx, P, [0, 1, 2], [3, 4, 5], 1001)
    check_names(k_add, ["rns_extend_kernel<8>"], ["rns_extend_fast_kernel", MFMA])
    names = run_scale_down(hx, P, [0, 1, 2, 3, 4], [0, 1, 2], 1002, ((2, 1), (4, 1), (65537, 1)))
    check_names(names, ["rns_extend_kernel<8>"], ["rns_extend_fast_kernel", MFMA])   # (the generic kernel's own tie rule)
    names = run_relin(hx, P, [0, 1, 2, 3, 4], [[0, 1, 2], [3, 4]], [5, 6], 1003, mul=False)
    check_names(names, ["break_digits_kernel<8>"], ["break_digits_fast_kernel<"])
    names = run_break(hx, P, [0, 1, 2, 3, 4], [[0, 1, 2], [3, 4]], [5, 6], 1004)
    check_names(names, ["rns_extend_kernel<8>", "rns_extend_fast_kernel<2, false>"])


def test_general_m_ring_at_planted_values(hx):
    """m = 105 (N = 48): the general-m entry into the same kernels; the planted list takes two polynomials there."""
    P = Pair(hx, 105, R.many_source_chain(O, 3, 105))
    src, rest = [0, 1, 2], list(range(3, 14))
    k_add, k_rem = run_add_primes(hx, P, src, rest, 1101)
    check_names(k_add, *extension_kernels(3, {}))
    check_names(k_rem, [generic_kernel(3)])
    check_names(run_scale_down(hx, P, src + rest, src, 1102), *extension_kernels(3, {}))
    run_break(hx, P, src + rest[:4], [src, rest[:4]], rest[4:], 1103)
    run_relin(hx, P, src + rest[:4], [src, rest[:4]], rest[4:], 1104, mul=False)
