"""hx_mask_split against the hx_poly_copy / hx_mul / hx_sub sequence it replaces (every word), and the BGV linear-array
rotate / shift / totalSums / runningSums (helib_amd.bgv.EncryptedArray) with real keys against numpy on the plaintext
slots.  Everything here is an integer: every comparison is exact."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import bgv_linalg_ref as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _ctx(hx, m, nprimes=3, bits=60):
    g = O.PrimeGen(bits, m)
    primes = [g.next() for _ in range(nprimes)]
    o, c = O.Ctx(m), hx.Context(m)
    for q in primes:
        i = o.add_prime(q)
        c.add_prime(q, o.roots[i])
    return c, primes


def _rand(rng, primes, idx, batch, n):
    """canonical residues [rows, batch, n] with 0, 1, q - 1 and q - 2 among them"""
    x = np.stack([rng.integers(0, primes[i], size=(batch, n), dtype=np.uint64) for i in idx])
    for r, i in enumerate(idx):
        x[r, :, :4] = [0, primes[i] - 1, 1, primes[i] - 2]
        x[r, -1, -2:] = [primes[i] - 1, 0]
    return x


def _three_calls(hx, keep, mask):
    """tmp = keep; tmp *= mask; keep -= tmp  -> tmp"""
    out = []
    for k in keep:
        t = k.copy()
        t *= mask
        k -= t
        out.append(t)
    return out


def _split_case(hx, c, primes, rng, parts, batch, mask_batch, superset):
    n = c.phim
    idx = [0, 2] if superset else [0, 1, 2]
    midx = [2, 1, 0] if superset else idx            # more primes than keep, in another order
    data = [_rand(rng, primes, idx, batch, n) for _ in range(parts)]
    md = _rand(rng, primes, midx, mask_batch, n)
    mask = hx.DoubleCRT(c, midx, mask_batch, md)
    keep = [hx.DoubleCRT(c, idx, batch, x) for x in data]
    take = [hx.likeUninit(k) for k in keep]
    hx.maskSplit(keep[0], keep[1] if parts == 2 else None, take[0], take[1] if parts == 2 else None, mask)
    ref_keep = [hx.DoubleCRT(c, idx, batch, x) for x in data]
    ref_take = _three_calls(hx, ref_keep, mask)
    for a in range(parts):
        gk, gt = keep[a].download(), take[a].download()
        assert np.array_equal(gt, ref_take[a].download()), (parts, batch, mask_batch, superset, a)
        assert np.array_equal(gk, ref_keep[a].download()), (parts, batch, mask_batch, superset, a)
        if n <= 64:                                   # and python integers, independent of any kernel
            for r, i in enumerate(idx):
                q = primes[i]
                mrow = md[midx.index(i)]
                for b in range(batch):
                    mb = mrow[b if mask_batch > 1 else 0]
                    t = [int(x) * int(y) % q for x, y in zip(data[a][r, b], mb)]
                    assert [int(x) for x in gt[r, b]] == t
                    assert [int(x) for x in gk[r, b]] == [(int(x) - y) % q for x, y in zip(data[a][r, b], t)]
    assert np.array_equal(mask.download(), md)        # the mask is read only
    return keep, take


# ---- 1. the kernel against the three-call sequence ----
@pytest.mark.parametrize("m", [105, 1024, 32768])
def test_mask_split_equals_copy_mul_sub(hx, m):
    c, primes = _ctx(hx, m)
    assert c.phim == {105: 48, 1024: 512, 32768: 16384}[m]
    rng = np.random.default_rng(m)
    for parts in (1, 2):
        for batch in (1, 3, 5, 64):
            for mask_batch in sorted({1, batch}):
                for superset in (False, True):
                    _split_case(hx, c, primes, rng, parts, batch, mask_batch, superset)


def test_mask_split_when_take_is_a_lazy_copy_of_keep(hx):
    """hx_poly_copy shares rows until one side is written: take sharing keep's rows, and keep sharing a bystander's"""
    c, primes = _ctx(hx, 1024)
    rng = np.random.default_rng(2)
    x, md = _rand(rng, primes, [0, 1, 2], 3, c.phim), _rand(rng, primes, [0, 1, 2], 1, c.phim)
    mask = hx.DoubleCRT(c, [0, 1, 2], 1, md)
    keep = hx.DoubleCRT(c, [0, 1, 2], 3, x)
    take, bystander = keep.copy(), keep.copy()
    hx.maskSplit(keep, None, take, None, mask)
    ref = hx.DoubleCRT(c, [0, 1, 2], 3, x)
    rt = _three_calls(hx, [ref], mask)[0]
    assert np.array_equal(keep.download(), ref.download()) and np.array_equal(take.download(), rt.download())
    assert np.array_equal(bystander.download(), x)


_CHILD = r"""
import hashlib, sys
import numpy as np
try:
    import torch  # noqa: F401
except ImportError:
    pass
from helib_amd import capi as hx
from tests import test_bgv_linalg_gpu as T
c, primes = T._ctx(hx, 1024)
rng = np.random.default_rng(77)
h = hashlib.sha256()
for parts, batch, mask_batch, superset in T.SWITCH_CASES:
    keep, take = T._split_case(hx, c, primes, rng, parts, batch, mask_batch, superset)
    for d in keep + take:
        h.update(d.download().tobytes())
print("WORDS", h.hexdigest())
"""
SWITCH_CASES = [(2, 5, 1, True), (1, 3, 3, False), (2, 64, 64, True), (2, 1, 1, False)]


def test_no_mask_split_switch_gives_the_same_words(hx):
    """HX_NO_MASK_SPLIT=1 is read when a context is created: a fresh child process runs the cases under it (there
    hx_mask_split issues the three calls itself), the parent runs them on the kernel; same random data, same words"""
    env = dict(os.environ, HX_NO_MASK_SPLIT="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    theirs = [ln.split()[1] for ln in out.stdout.splitlines() if ln.startswith("WORDS")]
    assert "HX_NO_MASK_SPLIT" not in os.environ
    c, primes = _ctx(hx, 1024)
    rng = np.random.default_rng(77)
    h = hashlib.sha256()
    for parts, batch, mask_batch, superset in SWITCH_CASES:
        keep, take = _split_case(hx, c, primes, rng, parts, batch, mask_batch, superset)
        for d in keep + take:
            h.update(d.download().tobytes())
    assert theirs == [h.hexdigest()]


# ---- 2. end to end with real keys ----
def _chain(hx, m, p, bits, seed=5, autos=None):
    from helib_amd import bgv, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, 1, bits=bits, c=3)
    g = hx.Context(m)
    o = O.Ctx(m)
    for q in cc.primes:
        i = o.add_prime(q)
        g.add_prime(q, o.roots[i])
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    ea = bgv.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    if autos is None:
        hk.add1DMatrices(sk)
    else:
        for k in autos:
            sk.GenKeySWmatrix(1, k)
        sk.setKeySwitchMap()
    return cc, g, sk, ea


def _same(x, y):
    assert (x.lnNoise, x.primeSet, x.intFactor, x.ptxtSpace) == (y.lnNoise, y.primeSet, y.intFactor, y.ptxtSpace)
    assert sorted(x.parts, key=str) == sorted(y.parts, key=str)
    for h in x.parts:
        assert np.array_equal(x.parts[h].download(), y.parts[h].download()), h


@pytest.mark.parametrize("m,p,bits,ngens", [(1024, 12289, 900, 2), (105, 211, 900, 3), (17, 103, 300, 1)])
def test_rotate_shift_and_sums_with_keys(hx, m, p, bits, ngens):
    """decrypt_batch after rotate / shift / totalSums / runningSums against numpy, fused (the kernel) and term by
    term: the same plaintext, and the same words and bookkeeping"""
    cc, g, sk, ea = _chain(hx, m, p, bits)
    assert ea.dimension() == ngens and all(ea.nativeDimension(i) for i in range(ngens))
    B, n = 3, ea.size()
    a = np.random.default_rng(m).integers(0, p, size=(B, n))
    amts = L.amounts(ea.zMStar.ords)
    fresh = ea.encrypt_batch(sk, a)                    # both paths start from the same words: encryption is randomised
    for op, args, truth in (("rotate", amts, L.rotate),
                            ("shift", amts + [-(n - 1), -(n + 3), 2 * n, -2 * n - 1], L.shift)):
        for amt in args:
            res = {}
            for fused in ((True, False) if ngens > 1 else (None, False)):
                ct = fresh.clone()
                assert getattr(ea, op)(ct, amt, fused=fused) is ct
                got = ea.decrypt_batch(ct, sk)
                want = truth(a, amt)
                if not ct.parts:                       # an empty ciphertext decrypts to one vector of zeros
                    assert op == "shift" and abs(amt) >= n and not got.any() and not want.any()
                else:
                    assert np.array_equal(got, want), (op, amt, fused)
                    assert ct.isCorrect(), (op, amt, fused)
                res[fused] = ct
            _same(*res.values())
    for op, truth in (("totalSums", L.total_sums), ("runningSums", L.running_sums)):
        res = {}
        for fused in ((True, False) if ngens > 1 else (None, False)):
            ct = fresh.clone()
            assert getattr(ea, op)(ct, fused=fused) is ct
            assert np.array_equal(ea.decrypt_batch(ct, sk), truth(a, p)), (op, fused)
            print(f"m = {m} {op} fused = {fused}: capacity {ct.capacity():.1f}")
            assert ct.isCorrect(), (op, fused)
            res[fused] = ct
        _same(*res.values())
    assert len(ea._masks) <= ea.MASK_CACHE


# ---- 3. fused against term by term: which path ran ----
def test_fused_keyword_selects_the_path(hx, monkeypatch):
    m, p = 1024, 12289
    z_amt = 5 * 2 + 1                                  # both coordinates non-zero (ords [256, 2])
    cc, g, sk, ea = _chain(hx, m, p, 300, autos=())
    for k in L.needed_automorphisms(ea.zMStar, [z_amt]):
        sk.GenKeySWmatrix(1, k)
    sk.setKeySwitchMap()
    a = np.random.default_rng(9).integers(0, p, size=(2, ea.size()))
    calls = []
    real = hx.maskSplit
    monkeypatch.setattr(hx, "maskSplit", lambda *args: (calls.append(1), real(*args))[1])
    out = {}
    fresh = ea.encrypt_batch(sk, a)
    for fused, expect in ((True, 1), (False, 0), (None, 1 if ea.fuseMaskSplit else 0)):
        del calls[:]
        ct = fresh.clone()
        ea.rotate(ct, z_amt, fused=fused)
        assert len(calls) == expect, fused
        assert np.array_equal(ea.decrypt_batch(ct, sk), L.rotate(a, z_amt))
        out[fused] = ct
    _same(out[True], out[False])
    _same(out[None], out[False])


# ---- 4. the benchmark shape ----
def test_rotate_by_one_at_the_benchmark_shape(hx):
    m, p = 32768, 65537
    from helib_amd import hostnt
    z = hostnt.ZmStar(m, p)
    cc, g, sk, ea = _chain(hx, m, p, 950, autos=L.needed_automorphisms(z, [1]))
    assert ea.zMStar.gens == z.gens and ea.dimension() == 2
    a = np.random.default_rng(1).integers(0, p, size=(8, ea.size()))
    for fused in (True, False):
        ct = ea.encrypt_batch(sk, a)
        ea.rotate(ct, 1, fused=fused)
        assert np.array_equal(ea.decrypt_batch(ct, sk), np.roll(a, 1, axis=1)), fused
        assert ct.isCorrect()


# ---- 5. inside a graph capture ----
def test_mask_split_in_a_graph_capture(hx):
    c, primes = _ctx(hx, 1024)
    rng = np.random.default_rng(4)
    n, idx, B = c.phim, [0, 1, 2], 5
    x0, x1 = _rand(rng, primes, idx, B, n), _rand(rng, primes, idx, B, n)
    md = _rand(rng, primes, idx, 1, n)
    mask = hx.DoubleCRT(c, idx, 1, md)
    direct = [hx.DoubleCRT(c, idx, B, x0), hx.DoubleCRT(c, idx, B, x1)]
    dt = [hx.likeUninit(d) for d in direct]
    hx.maskSplit(direct[0], direct[1], dt[0], dt[1], mask)          # eagerly once
    keep = [hx.DoubleCRT(c, idx, B, x0), hx.DoubleCRT(c, idx, B, x1)]
    take = [hx.likeUninit(k) for k in keep]
    c.graphBegin()
    hx.maskSplit(keep[0], keep[1], take[0], take[1], mask)
    graph = c.graphEnd()
    keep[0].upload(x0)                                               # (nothing ran yet)
    keep[1].upload(x1)
    graph.launch()
    for a in range(2):
        assert np.array_equal(keep[a].download(), direct[a].download())
        assert np.array_equal(take[a].download(), dt[a].download())
    # new operands in the same polys
    y0, y1 = _rand(rng, primes, idx, B, n), _rand(rng, primes, idx, B, n)
    keep[0].upload(y0)
    keep[1].upload(y1)
    graph.launch()
    ref = [hx.DoubleCRT(c, idx, B, y0), hx.DoubleCRT(c, idx, B, y1)]
    rt = _three_calls(hx, ref, mask)
    for a in range(2):
        assert np.array_equal(keep[a].download(), ref[a].download())
        assert np.array_equal(take[a].download(), rt[a].download())
    graph.destroy()


# ---- 6. refusals ----
def test_mask_split_refusals_touch_nothing(hx):
    c, primes = _ctx(hx, 1024)
    other, _ = _ctx(hx, 1024)
    rng = np.random.default_rng(6)
    n, idx, B = c.phim, [0, 1], 3
    xs = [_rand(rng, primes, idx, B, n) for _ in range(4)]
    k0, k1, t0, t1 = (hx.DoubleCRT(c, idx, B, x) for x in xs)
    mask = hx.DoubleCRT(c, [0, 1, 2], 1, _rand(rng, primes, [0, 1, 2], 1, n))

    def refused(code, match, *args):
        with pytest.raises(hx.HxError, match=match) as e:
            hx._chk(hx.lib().hx_mask_split(*[a.h if a is not None else None for a in args]))
        assert e.value.code == code, (match, e.value.code)
        for d, x in zip((k0, k1, t0, t1), xs):
            assert np.array_equal(d.download(), x), match

    INV, PS = hx.HX_ERR_INVALID, hx.HX_ERR_PRIMESET
    refused(INV, "null argument", None, None, t0, None, mask)
    refused(INV, "null argument", k0, None, None, None, mask)
    refused(INV, "null argument", k0, None, t0, None, None)
    refused(INV, "go together", k0, k1, t0, None, mask)
    refused(INV, "go together", k0, None, t0, t1, mask)
    # aliasing
    refused(INV, "also the mask", k0, None, k0, None, k0)
    one = hx.DoubleCRT(c, idx, B, xs[0])
    refused(INV, "also the mask", one, None, t0, None, one)
    refused(INV, "also the mask", k0, None, one, None, one)
    refused(INV, "also the mask", k0, one, t0, t1, one)
    refused(INV, "also the mask", k0, k1, t0, one, one)
    refused(INV, "different polys", k0, None, k0, None, mask)
    refused(INV, "different polys", k0, k1, t0, k0, mask)
    refused(INV, "different polys", k0, k1, k1, t1, mask)
    refused(INV, "different polys", k0, k0, t0, t1, mask)
    refused(INV, "different polys", k0, k1, t0, t0, mask)
    # a foreign context
    fk = hx.DoubleCRT(other, idx, B, xs[0])
    fm = hx.DoubleCRT(other, [0, 1, 2], 1)
    refused(INV, "incompatible objects", k0, None, fk, None, mask)
    refused(INV, "incompatible objects", k0, fk, t0, t1, mask)
    refused(INV, "incompatible objects", k0, None, t0, None, fm)
    # shapes
    for bad in (hx.DoubleCRT(c, idx, B + 1), hx.DoubleCRT(c, [0], B), hx.DoubleCRT(c, [1, 0], B), hx.DoubleCRT(c, [0, 1, 2], B)):
        refused(INV, "take0 differs", k0, None, bad, None, mask)
        refused(INV, "keep1 differs", k0, bad, t0, t1, mask)
        refused(INV, "take1 differs", k0, k1, t0, bad, mask)
    refused(INV, "neither 1 nor 3", k0, None, t0, None, hx.DoubleCRT(c, [0, 1, 2], 2))
    # a mask missing a prime
    refused(PS, "no row for prime 1", k0, None, t0, None, hx.DoubleCRT(c, [0, 2], 1))
    # more rows than one launch descriptor holds
    from helib_amd import hostnt
    big, gen = hx.Context(85), hostnt.PrimeGen(50, 85)
    for _ in range(161):
        big.add_prime(gen.next())
    wide = [hx.DoubleCRT(big, range(161), 1) for _ in range(3)]
    refused(hx.HX_ERR_UNSUPPORTED, "too many rows", wide[0], None, wide[1], None, wide[2])
    assert not any(w.download().any() for w in wide)
    # an odd number of coefficients: phi(m) is odd for m = 2 only (phi = 1); polys without rows reach the check
    tiny = hx.Context(2)
    assert tiny.phim == 1
    a, b, mk = (hx.DoubleCRT(tiny, [], 1, zero=False) for _ in range(3))
    with pytest.raises(hx.HxError, match="even number of coefficients") as e:
        hx.maskSplit(a, None, b, None, mk)
    assert e.value.code == hx.HX_ERR_UNSUPPORTED
    # and after all that the call still works
    hx.maskSplit(k0, k1, t0, t1, mask)
    ref = [hx.DoubleCRT(c, idx, B, xs[0]), hx.DoubleCRT(c, idx, B, xs[1])]
    rt = _three_calls(hx, ref, mask)
    assert np.array_equal(k0.download(), ref[0].download()) and np.array_equal(t1.download(), rt[1].download())
