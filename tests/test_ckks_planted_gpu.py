"""The integer kernels of the CKKS slot unit (helib_amd/csrc/ckks_slots.h) at planted inputs: ckks_crt_double_kernel<8 /
16 / 32 / 64> from 1 to 64 primes at the integers where its branches part, ckks_residues_kernel at coefficients beyond
the primes, the encode's slot skip where the first levels are folded into the load, and both transforms against
longdouble evaluations of their definitions.  Expected values come from tests/ckks_planted_ref.py (python integers,
`decimal`, numpy longdouble); tests/test_ckks_planted_host.py holds those references and these inputs to their
conditions on the CPU."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import ckks_planted_ref as P
from tests import ckks_ref as R

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


@pytest.fixture(scope="module")
def rings(hx):
    """(m, kind) -> (device context, oracle context, primes), built once: kind "60" / "mixed" = the 64 primes of
    prime_sets (a case of n primes takes the rows 0 .. n-1) and, behind the 60-bit ones, a 65th; "res" = the five
    rows of the residues tests; "one" = a single 60-bit prime"""
    made = {}

    def get(m, kind):
        if (m, kind) not in made:
            if kind == "res":
                primes = list(P.residue_primes(m))
            elif kind == "one":
                primes = list(P.prime_sets(m)[(1, "60")])
            else:
                primes = list(P.prime_sets(m)[(64, kind)])
                if kind == "60":
                    primes.append(P.residue_primes(m)[2])
            o, c = O.Ctx(m), hx.Context(m)
            for q in primes:
                i = o.add_prime(q)
                c.add_prime(q, o.roots[i])
            made[(m, kind)] = (c, o, primes)
        return made[(m, kind)]
    return get


def _crt_kernels(hx, fn):
    """run fn, return (its result, the set of ckks_crt_double_kernel instantiations it launched)"""
    hx.profileBegin()
    try:
        out = fn()
    finally:
        ks = hx.profileEnd()["kernels"]
    names = {k["kernel"].replace("hx::", "") for k in ks if "ckks_crt_double_kernel" in k["kernel"]}
    return out, names


def _instantiation(n):
    return "ckks_crt_double_kernel<%d>" % (8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64)


def _residue_table(vals, qs):
    return np.array([[int(v) % int(q) for v in vals] for q in qs], dtype=np.uint64)      # [n, count]


def _decode_isolated(hx, rings, m, n, kind, B):
    """every planted value alone in coefficient 0 of a batch element: all slots are the kernel's value, exactly"""
    c, _, primes = rings(m, kind)
    qs = primes[:n]
    N, lnQ = m // 2, P.lnQ_of(qs)
    worst = 0.0
    for li, lr in enumerate(P.ln_rats(qs)):
        names, vals, exact, keep = P.decode_cases(qs, lr)
        assert int((~keep).sum()) == P.expected_skips(n, li)
        bound = P.crt_rel_bound(n, lnQ, lr)
        tab = _residue_table(vals, qs)
        for b0 in range(0, len(vals), B):
            sel = [min(b0 + b, len(vals) - 1) for b in range(B)]      # (the last chunk repeats the last value)
            rows = np.zeros((n, B, N), dtype=np.uint64)
            rows[:, :, 0] = tab[:, sel]
            d = hx.DoubleCRT(c, range(n), B, rows)
            d.FFT()
            before = d.download()
            got, ran = _crt_kernels(hx, lambda: hx.ckksDecode(d, lr))
            assert ran == {_instantiation(n)}, ran
            assert np.array_equal(d.download(), before)                # the source poly is unchanged
            d.close()
            for b, i in enumerate(sel):
                if not keep[i]:
                    continue
                x = got[b].real[0]
                assert np.all(got[b].imag == 0) and np.all(got[b].real == x), (names[i], got[b][:4])
                if vals[i] == 0:
                    assert x == 0.0, names[i]
                    continue
                rel = abs(abs(x) - abs(exact[i])) / abs(exact[i])
                worst = max(worst, rel)
                assert rel <= bound, (names[i], li, x, exact[i], rel, bound)
                if names[i] not in P.NEIGHBOURS:                       # (magnitude only there: see the host file)
                    assert np.sign(x) == np.sign(exact[i]), (names[i], li, x, exact[i])
    print(f"m={m} n={n} {kind}: largest relative error {worst:.2e} (bound at ratFactor 1: "
          f"{P.crt_rel_bound(n, lnQ, 0.0):.2e})")


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("n", P.NS)
def test_decode_of_planted_constants(hx, rings, n, kind):
    """m = 64, one batch element per planted value: 40 * 32 = 1280 words, five 256-thread blocks"""
    _decode_isolated(hx, rings, 64, n, kind, 40)


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("n", [1, 9, 33, 64])
@pytest.mark.parametrize("m,B", [(16, 40), (1024, 3)])
def test_decode_of_planted_constants_partial_and_full_blocks(hx, rings, m, B, n, kind):
    """m = 16: 320 words, one full block and a partial one; m = 1024, three values at a time: 1536 words, six full
    blocks"""
    _decode_isolated(hx, rings, m, n, kind, B)


@pytest.mark.parametrize("n,li", [(2, 1), (17, 1), (64, 1), (64, 2)])
@pytest.mark.parametrize("m", [64, 1024])
def test_decode_with_every_coefficient_planted(hx, rings, m, n, li):
    """coefficient i of element b takes planted value (i + 7b) mod count: every block, row and element meets every
    branch.  ratFactor sqrt(Q); at 64 primes that leaves no planted value but 0 inside the double range (the host
    file pins it), so the 64-row kernel also runs at Q / e^30, where 30 of the 40 are."""
    c, _, primes = rings(m, "mixed")
    qs = primes[:n]
    N, B, lnQ = m // 2, 3, P.lnQ_of(qs)
    lr = P.ln_rats(qs)[li]
    names, vals, exact, keep = P.decode_cases(qs, lr)
    use = [i for i in range(len(vals)) if keep[i] and names[i] not in P.NEIGHBOURS]
    assert len(use) == (1 if (n, li) == (64, 1) else 38 - P.expected_skips(n, li))
    pick = (np.arange(N)[None, :] + 7 * np.arange(B)[:, None]) % len(use)          # [B, N]
    tab = _residue_table([vals[i] for i in use], qs)
    d = hx.DoubleCRT(c, range(n), B, tab[:, pick])
    d.FFT()
    got, ran = _crt_kernels(hx, lambda: hx.ckksDecode(d, lr))
    assert ran == {_instantiation(n)}, ran
    f = P.crt_exact_ld([vals[i] for i in use], qs, lr)[pick]
    re, im = P.embed_ld(f, m)
    l1 = np.sum(np.abs(f), axis=1, keepdims=True).astype(np.float64)
    tol = P.crt_rel_bound(n, lnQ, lr) * l1 + P.fft_abs_bound(N, l1)
    err = np.maximum(np.abs(got.real.astype(P.LD) - re), np.abs(got.imag.astype(P.LD) - im)).astype(np.float64)
    print(f"m={m} n={n} ln_rat[{li}]: {len(use)} values, max error / tolerance {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert np.all(err <= tol)
    if len(use) == 1:
        assert not got.any()


def test_decode_edges(hx, rings):
    c, _, primes = rings(1024, "60")
    N = 512
    empty = hx.DoubleCRT(c, [], 2)
    got, ran = _crt_kernels(hx, lambda: hx.ckksDecode(empty, 3.0))
    assert got.shape == (2, N // 2) and not got.any() and not ran
    d = hx.DoubleCRT(c, [0, 1], 1, np.ones((2, 1, N), dtype=np.uint64))
    for bad in (float("inf"), float("-inf"), float("nan")):
        with pytest.raises(hx.InvalidArgument, match="must be finite"):
            hx.ckksDecode(d, bad)
    assert len(primes) == 65
    with pytest.raises(hx.HxError) as e:
        hx.ckksDecode(hx.DoubleCRT(c, range(65), 1), 0.0)
    assert e.value.code == hx.HX_ERR_UNSUPPORTED


def _ones(sign, m):
    return np.full((1, m // 4), float(sign))


def test_encode_residues_at_planted_coefficients(hx, rings):
    """every slot +-1 encodes the constant polynomial +-scaling exactly (test_encode_rounds_halves_away_from_zero
    rests on the same): coefficient 0 is the planted integer, and the five rows (60, 60, 48, 36, 30 bits) are its
    residues -- quotients up to 9 at 60 bits and 2^33 at 30 bits, exact negative multiples, INT64_MIN"""
    m = 1024
    c, o, primes = rings(m, "res")
    idx = list(range(len(primes)))
    for x in P.residue_scalings(primes):
        d, cf = hx.ckksEncode(c, _ones(1 if x > 0 else -1, m), float(abs(x)), idx, coeffs=True)
        assert int(cf[0, 0]) == x and not cf[0, 1:].any(), x
        want = P.residues_exact(cf[0], primes)
        assert [int(w) for w in want[:, 0]] == [x % q for q in primes]
        assert np.array_equal(d.download()[:, 0], o.fft(idx, want)), x
        d.close()


@pytest.mark.parametrize("m", [16384, 32768, 65536, 131072])
def test_encode_residues_of_exact_multiples_through_every_row_kernel(hx, rings, m):
    """the exact multiples -k q and INT64_MIN again, at the rings served by the other forward transforms (N = 2^13,
    2^14, 2^15 row kernels and the split N = 2^16): the rows leave hx_ckks_encode only through that transform, so
    this is where a residue left at q instead of 0 would have to show"""
    c, o, primes = rings(m, "res")
    idx = list(range(len(primes)))
    xs = [x for x in P.residue_scalings(primes) if x < 0 and any(x % q == 0 for q in primes)] + [-(1 << 63)]
    assert len(xs) >= 9
    for x in xs:
        d, cf = hx.ckksEncode(c, _ones(-1, m), float(-x), idx, coeffs=True)
        # (coefficient 0 is the exact sum of the slots; the others are the transform's rounding noise times the
        # scaling, where the load is folded no longer exactly 0 at 2^63)
        noise = 0.5 + P.fft_abs_bound(m // 2, m // 2) * float(-x) / (m // 2)
        assert int(cf[0, 0]) == x and np.max(np.abs(cf[0, 1:])) <= noise, x
        nz = np.nonzero(cf[0])[0]
        want = np.zeros((len(primes), m // 2), dtype=np.uint64)
        want[:, nz] = P.residues_exact(cf[0, nz], primes)
        assert [int(w) for w in want[:, 0]] == [x % q for q in primes]
        assert np.array_equal(d.download()[:, 0], o.fft(idx, want)), x
        d.close()


def test_encode_overflow_guard_and_row_limit(hx, rings):
    m = 1024
    c, o, primes = rings(m, "60")
    for sign, scaling in ((1, 2.0 ** 63), (-1, 2.0 ** 63 + 2048.0)):
        with pytest.raises(hx.HxError, match="overflow in encoding"):
            hx.ckksEncode(c, _ones(sign, m), scaling, [0])
    for sign, scaling, want in ((-1, 2.0 ** 63, -(1 << 63)), (1, 2.0 ** 63 - 1024.0, (1 << 63) - 1024)):
        _, cf = hx.ckksEncode(c, _ones(sign, m), scaling, [0], coeffs=True)
        assert int(cf[0, 0]) == want and not cf[0, 1:].any()
    # 64 rows are served, 65 are not
    idx = list(range(64))
    d, cf = hx.ckksEncode(c, _ones(-1, m), 2.0 ** 62, idx, coeffs=True)
    assert int(cf[0, 0]) == -(1 << 62)
    assert np.array_equal(d.download()[:, 0], o.fft(idx, P.residues_exact(cf[0], primes[:64])))
    with pytest.raises(hx.HxError) as e:
        hx.ckksEncode(c, _ones(1, m), 2.0 ** 20, list(range(65)))
    assert e.value.code == hx.HX_ERR_UNSUPPORTED


def _check_against_ld(cf, v, m, scaling):
    """|cf - the longdouble evaluation| <= 0.5 + the transform's forward error, at the sampled coefficients"""
    N = m // 2
    ks = P.sample_coeffs(m)
    ld = P.encode_unrounded_ld(v, m, scaling, coeffs=ks)
    l1 = 2 * np.sum(np.abs(v), axis=1, keepdims=True)
    tol = 0.5 + P.fft_abs_bound(N, l1) * scaling / N
    err = np.abs(cf[:, ks].astype(P.LD) - ld).astype(np.float64)
    assert np.all(err <= tol), (float(np.max(err - tol)), float(np.max(tol)))
    return float(np.max((err - 0.5) / (tol - 0.5))) if np.all(tol > 0.5) else 0.0


@pytest.mark.parametrize("m,B", P.LARGE_CASES)
def test_encode_with_large_coefficients_everywhere(hx, rings, m, B):
    """random slots scaled so that the largest coefficient is 0.9 * 2^62: a third of the coefficients exceed every
    prime, so the reduction and the negative branch work on every word of every block (S = 4 at m = 65536)"""
    c, o, primes = rings(m, "res")
    primes, idx = primes[:4], [0, 1, 2, 3]
    v, scaling = P.large_encode_case(m, B)
    d, cf = hx.ckksEncode(c, v, scaling, idx, coeffs=True)
    big = np.abs(cf.astype(np.float64))
    assert np.max(big) >= 2.0 ** 61
    assert np.mean(big > max(primes)) >= 0.1
    want = P.residues_exact(cf, primes)                               # [4, B, N]
    rows = d.download()
    for b in range(B):
        assert np.array_equal(rows[:, b], o.fft(idx, want[:, b])), b
    used = _check_against_ld(cf, v, m, scaling)
    print(f"m={m} B={B}: {np.mean(big > max(primes)):.3f} of the coefficients beyond the largest prime, "
          f"largest error {used:.3f} of the transform's bound")


@pytest.mark.parametrize("frac", ["0", "1", "37", "N/2-1"])
@pytest.mark.parametrize("m", [32768, 65536, 131072])
def test_encode_with_fewer_values_where_the_load_is_folded(hx, rings, m, frac):
    """S = 2, 4, 8 sub-transforms per row: the slots that are not given are skipped inside the folded S-term load"""
    N = m // 2
    ns = {"0": 0, "1": 1, "37": 37, "N/2-1": N // 2 - 1}[frac]
    c, _, _ = rings(m, "one")
    rng = np.random.default_rng(m + ns)
    v = rng.uniform(-1, 1, size=(2, ns)) + 1j * rng.uniform(-1, 1, size=(2, ns))
    scaling = 2.0 ** 30
    _, cf = hx.ckksEncode(c, v, scaling, [0], coeffs=True)
    if ns == 0:
        assert not cf.any()
        return
    x = R.embed_unrounded(v, m, scaling, P._reps(m))
    want = R.round_away(x).astype(np.int64)
    near_half = np.abs(np.abs(x - np.trunc(x)) - 0.5) < 1e-6
    assert np.mean(near_half) <= 1e-4
    diff = cf != want
    assert not (diff & ~near_half).any()
    assert np.max(np.abs(cf - want)) <= 1
    _check_against_ld(cf, v, m, scaling)


@pytest.mark.parametrize("m", [16, 1024, 32768, 131072])
def test_embed_against_the_longdouble_evaluation(hx, rings, m):
    N = m // 2
    c, _, _ = rings(m, "one")
    rng = np.random.default_rng(m)
    mono = np.zeros(N)
    mono[N - 1] = 1.0
    near = (2.0 ** 52 - rng.integers(0, 1000, size=N)) * rng.choice([-1.0, 1.0], size=N)
    f = np.stack([rng.uniform(-1e6, 1e6, size=N), np.full(N, 1e6), mono, near])
    got = hx.ckksEmbed(c, f)
    sl = P.sample_slots(m)
    re, im = P.embed_ld(f, m, sl)
    tol = P.fft_abs_bound(N, np.sum(np.abs(f), axis=1, keepdims=True))
    err = np.maximum(np.abs(got.real[:, sl].astype(P.LD) - re), np.abs(got.imag[:, sl].astype(P.LD) - im))
    err = err.astype(np.float64)
    print(f"m={m}: largest error / bound per row {np.max(err / tol, axis=1)}")
    assert np.all(err <= tol)
