"""hx_mul_add_many against the hx_mul / hx_add sequence it replaces (every word), and MatMul1DExec / the slot
rotations and sums of helib_amd.ckks on the device: fused against forced term by term (equality), against the
oracle-backend run of the same mirror (equality) and against the numpy restatement (the scheme's own errorBound)."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import ckks_linalg_ref as L

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


def _ctx(hx, m, nprimes):
    g = O.PrimeGen(60, m)
    primes = [g.next() for _ in range(nprimes)]
    o, c = O.Ctx(m), hx.Context(m)
    for q in primes:
        i = o.add_prime(q)
        c.add_prime(q, o.roots[i])
    return c, primes


KEY = bytes(range(32))


def _rand(hx, c, idx, batch, stream):
    return hx.DoubleCRT(c, idx, batch, zero=False).randomize(KEY, stream)


def _sequence(out, consts, ins, accumulate):
    """n x { tmp = b; tmp *= a; x += tmp }"""
    if not accumulate:
        out = out.__class__(out.context, out.getIndexSet(), out.batch)
    for a, b in zip(consts, ins):
        tmp = b.copy()
        tmp *= a
        out += tmp
    return out


# (m, n, batch, constants per batch element, constants on a superset, parts, accumulate)
CASES = [(1024, 1, 1, False, False, 2, 0), (1024, 2, 3, False, True, 2, 1), (1024, 7, 3, True, False, 1, 1),
         (1024, 128, 1, False, False, 1, 0), (1024, 182, 3, True, True, 2, 0), (1024, 300, 3, False, False, 2, 1),
         (1024, 300, 64, False, True, 2, 0), (32768, 7, 3, False, True, 2, 1), (32768, 300, 1, False, False, 2, 1),
         (65536, 128, 64, False, False, 2, 1), (65536, 182, 64, False, True, 1, 0), (65536, 2, 3, True, False, 2, 0),
         (16, 7, 3, False, False, 2, 1)]


@pytest.mark.parametrize("m,n,batch,cper,superset,parts,accumulate", CASES)
def test_mul_add_many_equals_the_sequence(hx, m, n, batch, cper, superset, parts, accumulate):
    big = m >= 32768 and n * batch > 1000
    c, primes = _ctx(hx, m, 2 if big else 4)
    own = [0] if big else [0, 2, 1]
    cidx = list(range(len(primes))) if superset else own
    consts = [_rand(hx, c, cidx, batch if cper else 1, 1000 + t) for t in range(n)]
    ins = [[_rand(hx, c, own, batch, 5000 * (p + 1) + t) for t in range(n)] for p in range(parts)]
    outs = [_rand(hx, c, own, batch, 90 + p) for p in range(parts)]
    want = [_sequence(outs[p].copy(), consts, ins[p], accumulate).download() for p in range(parts)]
    hx.mulAddMany(outs[0], outs[1] if parts == 2 else None, consts, ins[0], ins[1] if parts == 2 else None,
                  accumulate=bool(accumulate))
    for p in range(parts):
        assert np.array_equal(outs[p].download(), want[p])


@pytest.mark.parametrize("n", [1, 256, 300, 513])
def test_worst_case_accumulator(hx, n):
    """every operand word q - 1, primes just below 2^60: the largest value the 128-bit accumulator can reach"""
    m, batch = 1024, 3
    c, primes = _ctx(hx, m, 3)
    assert all((1 << 59) < q < (1 << 60) for q in primes)
    idx = [0, 1, 2]
    full = np.stack([np.full((batch, m // 2), q - 1, dtype=np.uint64) for q in primes])
    one = hx.DoubleCRT(c, idx, batch, full)
    k = hx.DoubleCRT(c, idx, 1, full[:, :1])
    o0, o1 = one.copy(), one.copy()
    hx.mulAddMany(o0, o1, [k] * n, [one] * n, [one] * n, accumulate=True)
    want = np.stack([np.full((batch, m // 2), (q - 1 + n * (q - 1) * (q - 1)) % q, dtype=np.uint64) for q in primes])
    assert np.array_equal(o0.download(), want) and np.array_equal(o1.download(), want)


def test_error_returns(hx):
    m = 1024
    c, primes = _ctx(hx, m, 3)
    a, b, k = (_rand(hx, c, [0, 1], 3, s) for s in (1, 2, 3))
    out = hx.DoubleCRT(c, [0, 1], 3)
    out1 = hx.DoubleCRT(c, [0, 1], 3)
    polys = (a, b, k, out, out1)
    keep = [x.download() for x in polys]
    with pytest.raises(hx.InvalidArgument):
        hx.mulAddMany(out, None, [], [], None)
    with pytest.raises(hx.InvalidArgument, match="the same poly"):
        hx.mulAddMany(out, out, [k], [a], [b])
    with pytest.raises(hx.InvalidArgument, match=r"also an input \(term 1\)"):
        hx.mulAddMany(out, None, [k, out], [a, b], None)                     # an output that is also a constant
    with pytest.raises(hx.InvalidArgument, match=r"also an input \(term 0\)"):
        hx.mulAddMany(out, out1, [k], [a], [out1])
    with pytest.raises(hx.InvalidArgument, match=r"in1\[1\] differs from the output"):
        hx.mulAddMany(out, out1, [k, k], [a, a], [b, _rand(hx, c, [0, 1], 2, 7)])
    with pytest.raises(hx.InvalidArgument, match="out0 and out1 differ"):
        hx.mulAddMany(out, hx.DoubleCRT(c, [0, 2], 3), [k], [a], [b])
    c2, _ = _ctx(hx, m, 3)
    foreign = _rand(hx, c2, [0, 1], 3, 8)
    with pytest.raises(hx.InvalidArgument, match=r"incompatible objects \(term 1\)"):
        hx.mulAddMany(out, None, [k, k], [a, foreign], None)
    with pytest.raises(hx.InvalidArgument, match=r"incompatible objects \(term 0\)"):
        hx.mulAddMany(out, None, [_rand(hx, c2, [0, 1], 1, 9)], [a], None)
    with pytest.raises(hx.InvalidArgument, match="incompatible objects"):
        hx.mulAddMany(out, foreign, [k], [a], [b])
    # more rows than one launch descriptor holds (refused before the terms' shapes are looked at)
    from helib_amd import hostnt
    big, gen = hx.Context(85), hostnt.PrimeGen(50, 85)
    for _ in range(161):
        big.add_prime(gen.next())
    wide, thin = hx.DoubleCRT(big, range(161), 1), hx.DoubleCRT(big, [5], 1)
    with pytest.raises(hx.HxError, match="too many rows") as e:
        hx.mulAddMany(wide, None, [thin], [thin], None)
    assert e.value.code == hx.HX_ERR_UNSUPPORTED
    # an odd number of coefficients: phi(m) is odd for m = 2 only (phi = 1); polys without rows reach the check
    tiny = hx.Context(2)
    assert tiny.phim == 1
    ta, tb, tk = (hx.DoubleCRT(tiny, [], 1, zero=False) for _ in range(3))
    with pytest.raises(hx.HxError, match="hx_mul_add_many needs an even number of coefficients") as e:
        hx.mulAddMany(ta, None, [tk], [tb], None)
    assert e.value.code == hx.HX_ERR_UNSUPPORTED
    with pytest.raises(hx.InvalidArgument, match="no row for prime"):
        hx.mulAddMany(out, None, [_rand(hx, c, [0], 1, 4)], [a], None)
    with pytest.raises(hx.InvalidArgument, match="batch"):
        hx.mulAddMany(out, None, [_rand(hx, c, [0, 1], 2, 5)], [a], None)
    with pytest.raises(hx.InvalidArgument, match="differs"):
        hx.mulAddMany(out, None, [k], [_rand(hx, c, [0, 2], 3, 6)], None)
    with pytest.raises(hx.InvalidArgument, match="also an input"):
        hx.mulAddMany(out, None, [k], [out], None)
    with pytest.raises(hx.InvalidArgument, match="go together"):
        hx.mulAddMany(out, b, [k], [a], None)
    one = hx.DoubleCRT(c, [0, 1], 1)
    with pytest.raises(hx.InvalidArgument, match="batch element"):
        hx._chk(hx.lib().hx_poly_extract(one.h, a.h, 3))
    with pytest.raises(hx.InvalidArgument, match="batch element"):
        hx._chk(hx.lib().hx_poly_extract(one.h, a.h, -1))
    narrow = hx.DoubleCRT(c, [0], 1)
    with pytest.raises(hx.InvalidArgument, match="prime set"):
        hx._chk(hx.lib().hx_poly_extract(narrow.h, a.h, 0))
    with pytest.raises(hx.InvalidArgument, match="batch 1"):
        hx._chk(hx.lib().hx_poly_extract(out.h, a.h, 0))
    with pytest.raises(hx.InvalidArgument, match="null argument"):
        hx._chk(hx.lib().hx_poly_extract(one.h, None, 0))
    with pytest.raises(hx.InvalidArgument, match="null argument"):
        hx._chk(hx.lib().hx_poly_extract(None, a.h, 0))
    with pytest.raises(hx.InvalidArgument, match="null argument"):
        hx._chk(hx.lib().hx_poly_extract(one.h, one.h, 0))                   # dst is src
    with pytest.raises(hx.InvalidArgument, match="incompatible objects"):
        hx._chk(hx.lib().hx_poly_extract(one.h, foreign.h, 0))
    assert not one.download().any() and not narrow.download().any()
    rows = a.download()
    for b, d in enumerate(hx.splitBatch(a)):
        assert np.array_equal(d.download()[:, 0], rows[:, b])
    c.graphBegin()
    try:
        with pytest.raises(hx.HxError) as e:
            hx.mulAddMany(out, None, [k], [a], None)
        assert e.value.code == hx.HX_ERR_UNSUPPORTED and "hx_mul_add_many uploads a pointer table" in str(e.value)
    finally:
        try:
            c.graphEnd().destroy()
        except hx.HxError:
            pass               # (nothing was recorded)
    for x, w in zip(polys, keep):
        assert np.array_equal(x.download(), w)


def _chain(hx, m, bits, fam, seed=5, extra=()):
    from helib_amd import ckks, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, -1, 20, bits=bits, c=3, ckks=True)
    g = hx.Context(m)
    o = O.Ctx(m)
    for q in cc.primes:
        i = o.add_prime(q)
        g.add_prime(q, o.roots[i])
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey(maxDegKswitch=2)
    {"full": hk.add1DMatrices, "min": hk.addMinimal1DMatrices, "bsgs": hk.addBSGS1DMatrices}[fam](sk)
    for k in extra:
        if not sk.haveKeySWmatrix(1, k):
            sk.GenKeySWmatrix(1, k)
    sk.setKeySwitchMap()
    return cc, g, o, sk, ckks.EncryptedArrayCx(cc, g)


def _slots(B, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (B, n)) + 1j * rng.uniform(-1, 1, (B, n))) / math.sqrt(2)


def _banded(D, ndiag, seed, contiguous=False):
    """ndiag non-zero diagonals: scattered, or the band 0 .. ndiag - 1"""
    rng = np.random.default_rng(seed)
    A = np.zeros((D, D), dtype=np.complex128)
    j = np.arange(D)
    for i in (range(ndiag) if contiguous else rng.choice(D, size=ndiag, replace=False)):
        A[(j - i) % D, j] = (rng.uniform(-1, 1, D) + 1j * rng.uniform(-1, 1, D)) / ndiag
    return A


def _same(a, b):
    assert set(a.parts) == set(b.parts)
    for h in a.parts:
        assert np.array_equal(a.parts[h].download(), b.parts[h].download()), h
    assert (a.lnNoise, a.lnRatFactor, a.ptxtMag, a.primeSet) == (b.lnNoise, b.lnRatFactor, b.ptxtMag, b.primeSet)


@pytest.mark.parametrize("m,bits,B,ndiag", [(1024, 300, 1, 256), (1024, 300, 8, 256), (65536, 1400, 4, 64)])
def test_matmul_fused_equals_term_by_term(hx, m, bits, B, ndiag):
    from helib_amd import ckks, linalg
    cc, g, o, sk, ea = _chain(hx, m, bits, "bsgs")
    D = m // 4
    # m = 65536: the band of diagonals 0..63 is one giant step of 64 terms, baby step 0 (not hoisted) among them
    A = _banded(D, ndiag, m + B, contiguous=ndiag < D)
    ex = ckks.MatMul1DExec(ea, A)
    assert ex.g == math.isqrt(D - 1) + 1
    v = _slots(B, D, 11)
    ct = ea.encrypt_batch(sk, v)
    fused, plain = ct.clone(), ct.clone()
    before = linalg.MatMul1DExec.fallbacks
    ex.mul(fused, sk)
    assert linalg.MatMul1DExec.fallbacks == before
    ex.mul(plain, sk, fused=False)
    _same(fused, plain)
    got = ea.rawDecrypt_batch(fused, sk)
    err, bound = float(np.max(np.abs(got - v @ A))), ckks.errorBound(fused)
    print(f"m={m} B={B}: max slot error {err:.3e}, errorBound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("fam,minimal", [("bsgs", False), ("min", False), ("full", False)])
def test_matmul_equals_the_oracle_backend_run(hx, fam, minimal):
    """m = 256 (m = 128 for the g = 0 form): the same keys, samples and encoded coefficients through the CPU
    backend, term by term there"""
    from helib_amd import ckks, keys as hk
    from oracle.backend import OracleBackend
    m = 128 if fam == "full" else 256
    cc, g, o, sk, ea = _chain(hx, m, 300, fam)
    be = OracleBackend(o, cc)
    osk = hk.SecKey(cc, be, seed=5)
    osk.GenSecKey(maxDegKswitch=2)
    {"full": hk.add1DMatrices, "min": hk.addMinimal1DMatrices, "bsgs": hk.addBSGS1DMatrices}[fam](osk)
    osk.setKeySwitchMap()
    oea = ckks.EncryptedArrayCx(cc, None, encoder=L.HostEncoder(be, m, coeffs=lambda v, s: ea.encodeCoeffs(v, s)))
    D = m // 4
    A = _banded(D, D, 3)
    v = _slots(1, D, 4)
    d, f = ea.encode(v)
    od, of = oea.encode(v)
    assert np.array_equal(d.download()[:, 0], od.rows)
    ct, oct = sk.CKKSencrypt(d, -1.0, f), osk.CKKSencrypt(od, -1.0, of)
    for h in ct.parts:
        assert np.array_equal(ct.parts[h].download()[:, 0], oct.parts[h].rows), h
    from helib_amd import linalg
    before = linalg.MatMul1DExec.fallbacks
    ckks.MatMul1DExec(ea, A, minimal=minimal).mul(ct, sk)
    if fam != "min":
        # g = 0 too: diagonal 0 alone, then the hoisted terms.  (The iterative form's baby steps are a chain of
        # smartAutomorph + cleanUp: each has its own factor, equalizeRationalFactors asks for multipliers other than
        # 1 and those groups go term by term, as the counter then shows.)
        assert linalg.MatMul1DExec.fallbacks == before
    ckks.MatMul1DExec(oea, A, minimal=minimal).mul(oct, osk)
    assert set(ct.parts) == set(oct.parts) and ct.primeSet == oct.primeSet
    for h in ct.parts:
        assert np.array_equal(ct.parts[h].download()[:, 0], oct.parts[h].rows), h
    # the same python arithmetic in the same order; the measured norms that enter lnNoise come from the device on one
    # side and from the oracle's floating-point embedding on the other, which agree to rounding only
    assert ct.lnRatFactor == oct.lnRatFactor and ct.ptxtMag == oct.ptxtMag
    assert abs(ct.lnNoise - oct.lnNoise) < 1e-9
    got = ea.rawDecrypt(ct, sk)
    assert np.max(np.abs(got - (v @ A)[0])) <= ckks.errorBound(ct)


def test_rotations_sums_and_parts_on_the_device(hx):
    from helib_amd import ckks
    m, B = 1024, 3
    cc, g, o, sk, ea = _chain(hx, m, 300, "full", extra=(m - 1,))
    n, v = m // 4, _slots(B, m // 4, 8)

    def run(op, want):
        ct = ea.encrypt_batch(sk, v)
        op(ct)
        got = ea.rawDecrypt_batch(ct, sk)
        exp = np.stack([want(x) for x in v])
        assert np.max(np.abs(got - exp)) <= ckks.errorBound(ct)
    for amt in (1, -3, n + 5):
        run(lambda ct: ea.rotate(ct, amt), lambda x: L.rotate(x, amt))
    for amt in (2, -7):
        run(lambda ct: ea.shift(ct, amt), lambda x: L.shift(x, amt))
    ct = ea.encrypt_batch(sk, v)
    ea.shift(ct, n)
    assert not ct.parts
    run(ea.totalSums, L.totalSums)
    run(ea.runningSums, L.runningSums)
    run(ea.extractRealPart, lambda x: x.real)
    run(ea.extractImPart, lambda x: x.imag)
    # the switch, as an argument (D = 256 > 50: BSGS, g = 16)
    A = _banded(n, 5, 1)
    ex = ckks.MatMul1DExec(ea, A)
    a, b = ea.encrypt_batch(sk, v), None
    b = a.clone()
    ex.mul(a, sk)
    ex.mul(b, sk, fused=False)
    _same(a, b)
    assert np.max(np.abs(ea.rawDecrypt_batch(a, sk) - v @ A)) <= ckks.errorBound(a)


@pytest.mark.parametrize("m,fam", [(128, "full"), (1024, "bsgs")])
def test_environment_switch_forces_term_by_term(hx, monkeypatch, m, fam):
    """HX_MATMUL_TERMWISE=1, read when the MatMul1DExec is built: no fused call is made (the device entry is made to
    fail if it is reached), the result equals the fused one; m = 128 is the g = 0 hoisted form with diagonal 0"""
    from helib_amd import ckks, linalg
    cc, g, o, sk, ea = _chain(hx, m, 300, fam)
    D = m // 4
    A = _banded(D, min(D, 40), 9, contiguous=True)
    v = _slots(2, D, 12)
    ct = ea.encrypt_batch(sk, v)
    fused, plain = ct.clone(), ct.clone()
    before = linalg.MatMul1DExec.fallbacks
    ex = ckks.MatMul1DExec(ea, A)
    assert ex.fused and ex.g == (0 if m == 128 else 16)
    ex.mul(fused, sk)
    assert linalg.MatMul1DExec.fallbacks == before
    monkeypatch.setenv("HX_MATMUL_TERMWISE", "1")
    ex2 = ckks.MatMul1DExec(ea, A)
    assert not ex2.fused

    def refuse(*a, **k):
        raise AssertionError("hx_mul_add_many reached although term by term was forced")
    monkeypatch.setattr(hx, "mulAddMany", refuse)
    ex2.mul(plain, sk)
    monkeypatch.undo()
    _same(fused, plain)
    assert np.max(np.abs(ea.rawDecrypt_batch(fused, sk) - v @ A)) <= ckks.errorBound(fused)
