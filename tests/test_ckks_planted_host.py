"""The references and the planted inputs of tests/test_ckks_planted_gpu.py held to their conditions on the CPU, so that
the device file cannot pass by leaving cases out or by planting inputs that miss the branches they are named for.
No device here: tests/ckks_planted_ref.py against exact integers, `decimal`, and tests/ckks_ref.py."""
import math

import numpy as np
import pytest

from tests import ckks_planted_ref as P
from tests import ckks_ref as R

# (m, the n of the decode cases at that ring): tests/test_ckks_planted_gpu.py runs exactly these
DECODE_RINGS = ((64, P.NS), (16, (1, 9, 33, 64)), (1024, (1, 9, 33, 64)))


def _decode_params():
    return [(m, n, kind) for m, ns in DECODE_RINGS for n in ns for kind in P.KINDS]


@pytest.mark.parametrize("m,n,kind", _decode_params())
def test_model_meets_the_bound_and_the_skipped_share_is_pinned(m, n, kind):
    """For every case the device file asserts on: the restated kernel arithmetic is within crt_rel_bound of the exact
    quotient and has its sign, the asserted |exact| lie in [2^-1000, 2^1020], and the number of planted values the
    device file may skip is exactly expected_skips -- at most one quarter wherever one quarter can be had.

    It cannot be had everywhere: with 32 primes or more Q exceeds 2^1900, and at ratFactor 1 or e^37.12 the 29 planted
    values of the size of Q (the products, the thirds, the halves, the uniform ones) are beyond the double range --
    the 11 small ones are what those cases assert (their weights 2^we_k reach 2^3800: digits that must be skipped);
    at 64 primes and ratFactor sqrt(Q) only 0 is left.  Every such count is pinned here, so a device file that skipped
    one more case would disagree with this one.

    Known difference from the reference's exact centring, recorded here: at the two neighbours of Q/2 the kernel
    decides the sign from frac = value/Q in doubles, and (Q+1)/2 / Q rounds to exactly 0.5 at every n, so the model
    calls (Q+1)/2 POSITIVE (the host's Decrypt: negative, -(Q-1)/2), and (Q-1)/2 positive as Decrypt does.  The
    magnitudes agree to 2/Q.  The device file asserts the magnitude only at those two values."""
    qs = P.prime_sets(m)[(n, kind)]
    assert len(qs) == n and len(set(qs)) == n
    bits = (60,) * 4 if kind == "60" else (60, 60, 48, 36)
    assert all(int(q).bit_length() == bits[k % 4] for k, q in enumerate(qs))
    lnQ = P.lnQ_of(qs)
    for li, lr in enumerate(P.ln_rats(qs)):
        names, vals, exact, keep = P.decode_cases(qs, lr)
        assert len(names) == 40
        res, frac, _ = P.crt_model(vals, qs, lr)
        skipped = int((~keep).sum())
        assert skipped == P.expected_skips(n, li), (li, [names[i] for i in np.nonzero(~keep)[0]])
        if P.expected_skips(n, li) <= 10:
            assert skipped * 4 <= len(names)
        bound = P.crt_rel_bound(n, lnQ, lr)
        for i, name in enumerate(names):
            if not keep[i]:
                continue
            if vals[i] == 0:
                assert exact[i] == 0.0 and res[i] == 0.0
                continue
            assert P.RANGE_LO <= abs(exact[i]) <= P.RANGE_HI
            if name in P.NEIGHBOURS:
                assert res[i] > 0 and frac[i] <= 0.5, name                 # the known difference (docstring)
                assert exact[i] * (1 if name == "half_lo" else -1) > 0
                assert abs(abs(res[i]) - abs(exact[i])) <= bound * abs(exact[i]), name
                continue
            assert np.sign(res[i]) == np.sign(exact[i]), name
            assert abs(res[i] - exact[i]) <= bound * abs(exact[i]), (name, res[i], exact[i])


@pytest.mark.parametrize("m,n,kind", _decode_params())
def test_planted_values_reach_the_branches_they_are_named_for(m, n, kind):
    qs = [int(q) for q in P.prime_sets(m)[(n, kind)]]
    Q = P._prod(qs)
    pv = P.planted_values(qs)
    lr = P.ln_rats(qs)[2]                     # Q / e^30: every value below of the size of Q is asserted at every n
    names, vals, exact, keep = P.decode_cases(qs, lr)
    _, frac, digs = P.crt_model(vals, qs, lr)
    f = dict(zip(names, frac))
    d = dict(zip(names, digs))
    # the delta margin: the model's sign is the exact one on both sides, at every n
    assert f["half-d"] <= 0.5 < f["half+1+d"]
    assert 2 * pv["half-d"] < Q < 2 * pv["half+1+d"]
    # a negative value whose complement Q - 1 - value has all-zero high digits: -5 (and -1: every digit zero, the
    # `+ 1` term alone)
    for name, low in (("-5", 4), ("-1", 0)):
        comp = [q - 1 - a for q, a in zip(qs, d[name])]
        assert f[name] > 0.5 and comp == [low] + [0] * (n - 1)
    assert keep[names.index("-5")] or n >= 32           # (asserted at ratFactor 1 instead: next test)
    # no zero digit, positive and negative
    full = [k for k in names if k.startswith("u") and all(d[k])]
    assert any(f[k] <= 0.5 for k in full) and any(f[k] > 0.5 for k in full)
    assert all(keep[names.index(k)] for k in full)
    # only the top digit non-zero
    assert d["+top"] == [0] * (n - 1) + [1 % qs[-1]] and keep[names.index("+top")]
    if n > 1:
        assert d["Q-top"] == [0] * (n - 1) + [qs[-1] - 1] and f["Q-top"] > 0.5
    # every dispatch edge has its n
    assert {8, 9, 16, 17, 32, 33, 64, 1} <= set(P.NS)


@pytest.mark.parametrize("n", P.NS)
def test_small_values_are_asserted_where_their_weights_leave_the_double_range(n):
    """at ratFactor 1 the small planted values (high digits zero, or all q_k - 1 when negative) are asserted at every
    n, and from 18 primes on the weights of the digits they must skip are beyond 2^1024"""
    qs = P.prime_sets(64)[(n, "60")]
    names, vals, exact, keep = P.decode_cases(qs, 0.0)
    for k in ("+1", "-1", "+5", "-5", "+big", "-big"):
        assert keep[names.index(k)]
    _, we = P.crt_weights(qs, 0.0)
    assert (max(we) > 1024) == (n >= 18)
    if n == 64:
        assert max(we) > 3700


def test_residue_scalings_cover_the_quotient_classes():
    """the planted coefficients of the residues test: for every prime size |x| in [q, 2q) and |x| >= 4q; x = -k q
    exactly for every size whose multiples a double holds (48, 36 and 30 bits -- no multiple of a 60-bit prime of
    this form is a double); INT64_MIN; quotients of 7 and more at 60 bits and above 2^26 at 36 bits; and every one
    an integer a double holds exactly"""
    qs = P.residue_primes(1024)
    assert [int(q).bit_length() for q in qs] == list(P.RESIDUE_BITS)
    xs = P.residue_scalings(qs)
    assert -(1 << 63) in xs and (1 << 63) not in xs
    for x in xs:
        assert int(float(x)) == x and -(1 << 63) <= x < (1 << 63)
    for q in qs:
        assert any(q <= abs(x) < 2 * q for x in xs), q
        assert any(abs(x) >= 4 * q for x in xs), q
        assert any(x < 0 and x % q == 0 for x in xs) == (q < 1 << 53), q
        assert any(x < 0 and x % q for x in xs)
    assert max(abs(x) // qs[0] for x in xs) >= 7
    assert max(abs(x) // qs[3] for x in xs) >= 1 << 26
    want = P.residues_exact(np.array(xs, dtype=object), qs)
    assert want.dtype == np.uint64 and want.shape == (5, len(xs))
    assert int(want[3, xs.index(-qs[3])]) == 0 and int(want[0, xs.index(-(1 << 63))]) == (-(1 << 63)) % qs[0]


@pytest.mark.parametrize("m,B", P.LARGE_CASES)
def test_large_encode_case_has_its_share_of_coefficients_beyond_the_primes(m, B):
    v, scaling = P.large_encode_case(m, B)
    x = R.embed_unrounded(v, m, scaling, P._reps(m))
    qmax = max(P.residue_primes(m))
    assert abs(np.max(np.abs(x)) - 0.9 * 2.0 ** 62) <= 2.0 ** 62 * 1e-9
    assert np.max(np.abs(x)) >= 2.0 ** 61
    share = float(np.mean(np.abs(x) > qmax))
    print(f"m={m} B={B}: scaling 2^{math.log2(scaling):.2f}, {share:.3f} of the coefficients beyond the largest prime")
    assert share >= 0.1
    # the longdouble reference at its sample agrees with the double one to the double one's own error
    idx = P.sample_coeffs(m)
    ld = P.encode_unrounded_ld(v, m, scaling, coeffs=idx)
    l1 = 2 * np.sum(np.abs(v), axis=1, keepdims=True)
    assert np.all(np.abs(ld - x[:, idx].astype(P.LD)) <= P.fft_abs_bound(m // 2, l1) * scaling / (m // 2))


@pytest.mark.parametrize("m", [16, 64])
def test_embed_ld_agrees_with_the_double_restatements(m):
    """longdouble against double: the difference is the double reference's own error"""
    rng = np.random.default_rng(m)
    f = rng.uniform(-1e6, 1e6, size=(3, m // 2))
    assert np.array_equal(P._reps(m), R.reps(m))
    re, im = P.embed_ld(f, m)
    got = re.astype(np.float64) + 1j * im.astype(np.float64)
    for want in (R.direct_embedding(f, m), R.canonical_embedding(f, m)):
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    # and the encode reference inverts it: slots -> coefficients -> slots
    v = rng.uniform(-1, 1, size=(2, m // 4)) + 1j * rng.uniform(-1, 1, size=(2, m // 4))
    cf = P.encode_unrounded_ld(v, m, 1.0)
    assert np.max(np.abs(cf.astype(np.float64) - R.embed_unrounded(v, m, 1.0))) <= 1e-14
    re, im = P.embed_ld(cf, m)
    assert np.max(np.abs(re.astype(np.float64) + 1j * im.astype(np.float64) - v)) <= 1e-15 * m


@pytest.mark.parametrize("m", [32768, 131072])
def test_samples_hold_the_edges_of_every_sub_transform(m):
    N = m // 2
    S = N // 8192
    assert S > 1
    ks = set(int(k) for k in P.sample_coeffs(m))
    assert len(ks) >= 64 and all(s in ks and N - S + s in ks for s in range(S))
    sl = P.sample_slots(m)
    j = P.slot_root(m)[sl]
    roots = set(int(x) for x in j) | set(N - 1 - int(x) for x in j)
    assert len(sl) >= 64 and all(s in roots and N - S + s in roots for s in range(S))
    # the sampled O(N) evaluation is the full transform at those slots
    f = np.random.default_rng(m).uniform(-1e6, 1e6, size=(1, N))
    re, im = P.embed_ld(f, m, sl[:8])
    want = R.canonical_embedding(f, m, P._reps(m))[:, sl[:8]]
    assert np.max(np.abs(re.astype(np.float64) + 1j * im.astype(np.float64) - want)) <= 1e-11 * np.max(np.abs(want))


def test_bounds_are_the_stated_formulas():
    assert P.crt_rel_bound(64, 2661.0, 2631.0) == 68 * 2.0 ** -52 + 65 * 5293.0 * 2.0 ** -62
    assert P.fft_abs_bound(65536, 3.0) == (8 * 16 + 16) * 2.0 ** -53 * 3.0
