"""The planted boundary integers of tests/rns_boundary_ref.py on the CPU: the C oracle's exact-RNS routines against the
python-integer expectation on every planted polynomial (the oracle has only ever seen uniform residues either), and
the conditions on the inputs themselves -- against the restatement of the device's trust rule alone -- that make
tests/test_rns_boundary_gpu.py worth running: every class in every polynomial, the threshold classes on their side of
the default hps_eps, and at every source count a value a trusted HPS lane would get wrong."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import rns_boundary_ref as R

M = 256
NS = [1, 2, 3, 5, 8, 9, 11, 16, 17, 24, 40, 44]
PTXTS = (65537, 4, 2, 1)


def ctx_of(m, primes):
    ctx = O.Ctx(m)
    for q in primes:
        ctx.add_prime(q)
    return ctx


def check_extension(ctx, src, tgt, seed):
    """add_primes and to_poly of the planted values themselves"""
    ps, ts = [ctx.primes[i] for i in src], [ctx.primes[i] for i in tgt]
    for batch in R.extension_inputs(ps, 4, ctx.N, seed):
        rows = R.eval_rows(ctx, src, batch)
        for b, coef in enumerate(batch):
            assert R.classes_present(coef, ps, 4) == set(R.CLASSES)
            want = R.want_to_poly(coef, ps)
            assert ctx.to_poly(src, rows[:, b]) == want
            ext, pf = ctx.add_primes(src, rows[:, b], tgt, want_poly=True)
            assert np.array_equal(ext, ctx.fft(tgt, R.want_add_primes(coef, ps, ts))), (src, b)
            if R.prod(ps).bit_length() < 1000:   # (the coefficients as doubles, while a double holds them)
                assert np.allclose(pf, np.array([float(v) for v in want]), rtol=1e-15)


def check_scale_down(ctx, own, drop, seed):
    """scale_down with fdelta; delta runs over the planted values, the tie dm == ptxt/2 on both signs at ptxt 2 and 4"""
    own_ps = [ctx.primes[i] for i in own]
    pos = [own.index(i) for i in drop]
    drop_ps = [ctx.primes[i] for i in drop]
    keep = [i for i in own if i not in drop]
    P = R.prod(drop_ps)
    for ptxt in PTXTS:
        for batch in R.scale_down_inputs(drop_ps, [ctx.primes[i] for i in keep], ptxt, ctx.N, seed):
            rows = R.eval_rows(ctx, own, batch)
            for b, coef in enumerate(batch):
                assert R.classes_present([c % P for c in coef], drop_ps, ptxt) == set(R.CLASSES)
                got, fd = ctx.scale_down(own, rows[:, b], drop, ptxt, want_fdelta=True)
                want, wfd = R.want_scale_down(coef, own_ps, pos, ptxt)
                assert np.array_equal(got, ctx.fft(keep, want)), (ptxt, b)
                assert np.allclose(fd, wfd, rtol=1e-9, atol=1e-9 * max(1, ptxt)), (ptxt, b)
                if ptxt > 1 and ptxt % 2 == 0:   # (the planted tie is there: fdelta = -+ptxt/2 at delta = +-ptxt/2 ...)
                    assert np.any(np.isclose(np.abs(wfd), ptxt / 2, rtol=1e-12))


def check_digits(ctx, own, digits, sp, seed):
    """break_into_digits with norms, the planted class on each digit in turn"""
    own_ps = [ctx.primes[i] for i in own]
    allp = own + sp
    dps = [[ctx.primes[i] for i in d] for d in digits]
    dpos = [[own.index(i) for i in d] for d in digits]
    for which in range(len(digits)):
        for batch in R.digit_inputs(dps, which, ctx.N, seed + which):
            rows = R.eval_rows(ctx, own, batch)
            for b, coef in enumerate(batch):
                want, frac, digs = R.want_digits(coef, own_ps, dpos, [ctx.primes[i] for i in allp])
                assert R.classes_present(digs[which], dps[which], 4) == set(R.CLASSES), (digits, which, b)
                got, nrm = ctx.break_into_digits(own, rows[:, b], digits, allp, want_norms=True)
                for d in range(len(digits)):
                    assert np.array_equal(got[d], ctx.fft(allp, want[d])), (digits, which, d, b)
                    assert np.isclose(nrm[d], O.embedding_largest_coeff(ctx.m, frac[d]), rtol=1e-9), (digits, which, d, b)


@pytest.mark.parametrize("n", NS)
def test_planted_lists_sit_where_they_are_meant_to(n):
    """Against the restatement of hps_front alone, at the default hps_eps parsed from switches.h: inside-eps, zero and
    half values are untrusted (a retuned threshold that trusted one of them fails here, not silently on the device),
    outside-eps and thirds values are trusted, at least one planted value would come out WRONG from a trusted lane and
    at least one would come out right with the wrong sign (the sign decides the tie at an even ptxtSpace)."""
    eps = R.default_hps_eps()
    assert 0 < eps < 2.0 ** -20
    ps = R.many_source_chain(O, n, M)[:n]
    P = R.prod(ps)
    value_wrong = sign_wrong = 0
    seen = set()
    for ptxt in PTXTS:
        for cls, x in R.planted(ps, ptxt):
            assert 0 <= x < P
            seen.add(cls)
            trusted, value_ok, neg_ok = R.hps_front(ps, x, eps)
            if cls in ("inside_eps", "zero", "half"):
                assert not trusted, (cls, x)
            if cls in ("outside_eps", "thirds"):
                assert trusted and value_ok and neg_ok, (cls, x)
            value_wrong += not value_ok
            sign_wrong += value_ok and not neg_ok
    assert seen == set(R.CLASSES)
    assert value_wrong >= 1 and sign_wrong >= 1, (value_wrong, sign_wrong)
    # the two half neighbours and x = +-1 are on the list by value, whatever the classes are called
    vals = {x for _, x in R.planted(ps, 2)}
    assert {(P - 1) // 2, (P + 1) // 2, 1, P - 1, 2, P - 2} <= vals


@pytest.mark.parametrize("n", NS)
def test_oracle_on_planted_polynomials(n):
    """add_primes, to_poly, scale_down (fdelta) and break_into_digits (norms) of the C oracle from n 60-bit sources onto
    60-, 56- and 45-bit targets, ring m = 256, equal the python-integer expectation on every planted polynomial."""
    ctx = ctx_of(M, R.many_source_chain(O, n, M))
    src, rest = list(range(n)), list(range(n, n + 11))
    check_extension(ctx, src, rest, 1000 + n)
    check_scale_down(ctx, src + rest, src, 2000 + n)
    for digits in ([src, rest[:4]], [rest[:4], src]):
        check_digits(ctx, src + rest[:4], digits, rest[4:], 3000 + n)


@pytest.mark.parametrize("digits", [[[0, 1], [2, 3], [4]], [[0, 1, 2, 3, 4]], [[0], [1, 2, 3], [4, 5]]])
def test_oracle_on_planted_digit_shapes(digits):
    """the digit shapes of the device tests: the planted class on every digit in turn, later digits included"""
    L = sum(len(d) for d in digits)
    g60, g56 = O.PrimeGen(60, M), O.PrimeGen(56, M)
    ctx = ctx_of(M, [g60.next() for _ in range(L)] + [g56.next() for _ in range(2)])
    check_digits(ctx, list(range(L)), digits, [L, L + 1], 4000 + L)


def test_oracle_on_planted_polynomials_mixed_prime_sizes():
    """a 38-bit prime that is not of Proth form as a source next to 60-bit ones, and as a target of 60-bit sources"""
    ctx = ctx_of(M, R.mixed_chain(O, M))
    check_extension(ctx, [0, 1, 2], [3, 4, 6], 5001)
    check_extension(ctx, [1, 2, 3], [0, 4, 6], 5002)
    check_scale_down(ctx, list(range(6)), [0, 5], 5003)
    check_scale_down(ctx, list(range(6)), [1, 2, 3], 5004)
    for digits in ([[0, 1], [2, 3], [4, 5]], [[0], [1, 2, 3], [4, 5]]):
        check_digits(ctx, list(range(6)), digits, [6, 7], 5005)


def test_oracle_on_planted_polynomials_unsorted_sources():
    """a 38-bit source BEHIND two 60-bit ones (the chain of test_plans_the_fast_kernels_refuse on the device)"""
    g60, g56 = O.PrimeGen(60, M), O.PrimeGen(56, M)
    q38 = O.PrimeGen(38, M).next()
    a, b = g60.next(), g60.next()
    ctx = ctx_of(M, [a, b, q38] + [g60.next() for _ in range(2)] + [g56.next() for _ in range(2)])
    check_extension(ctx, [0, 1, 2], [3, 4, 5], 7001)
    check_scale_down(ctx, [0, 1, 2, 3, 4], [0, 1, 2], 7002)
    check_digits(ctx, [0, 1, 2, 3, 4], [[0, 1, 2], [3, 4]], [5, 6], 7003)


def test_general_m_ring():
    """the same at m = 105 (N = 48): the planted list is split over two polynomials there"""
    ctx = ctx_of(105, R.many_source_chain(O, 3, 105))
    src, rest = [0, 1, 2], list(range(3, 14))
    assert len(R.extension_inputs([ctx.primes[i] for i in src], 4, ctx.N, 1)) >= 2
    check_extension(ctx, src, rest, 6001)
    check_scale_down(ctx, src + rest, src, 6002)
    check_digits(ctx, src + rest[:4], [src, rest[:4]], rest[4:], 6003)
