"""hx_mask_fan against the hx_poly_copy / hx_mul sequence it replaces (every word), and helib_amd.permutations with real
keys -- PermNetwork.applyToCtxt fused and unfused over native and non-native dimensions, Galois-ring slots and CKKS --
against applyPermToVec on the plaintext slots.  Except for CKKS everything here is an integer: every comparison is
exact."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import bgv_hypercube_ref as H

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


def _sequence(c, cs, masks):
    """per output and part: copy(); *= mask"""
    outs = []
    for k in masks:
        row = []
        for part in cs:
            t = part.copy()
            t *= k
            row.append(t)
        outs.append(row)
    return outs


def _fan_case(hx, c, primes, rng, parts, batch, nout, mask_batch, superset):
    n = c.phim
    idx = [0, 2] if superset else [0, 1, 2]
    midx = [2, 1, 0] if superset else idx            # more primes than c, in another order
    cd = [_rand(rng, primes, idx, batch, n) for _ in range(parts)]
    # masks of batch 1 and of the frame's batch alternate when both are asked for
    mbs = [mask_batch if (t % 2 == 0) else 1 for t in range(nout)]
    md = [_rand(rng, primes, midx, mb, n) for mb in mbs]
    masks = [hx.DoubleCRT(c, midx, mb, x) for mb, x in zip(mbs, md)]
    cs = [hx.DoubleCRT(c, idx, batch, x) for x in cd]
    outs = [[hx.likeUninit(cs[0]) for _ in range(nout)] for _ in range(parts)]
    hx.maskFan(outs[0], outs[1] if parts == 2 else None, cs[0], cs[1] if parts == 2 else None, masks)
    want = _sequence(c, cs, masks)
    for t in range(nout):
        for a in range(parts):
            got = outs[a][t].download()
            assert np.array_equal(got, want[t][a].download()), (n, parts, batch, nout, mask_batch, superset, t, a)
            if n <= 64:                               # and python integers, independent of any kernel
                for r, i in enumerate(idx):
                    q = primes[i]
                    mrow = md[t][midx.index(i)]
                    mb = mrow if mbs[t] > 1 else mrow[:1]                   # (python integers in object arrays)
                    exact = cd[a][r].astype(object) * mb.astype(object) % q
                    assert np.array_equal(got[r].astype(object), exact)
    for a in range(parts):
        assert np.array_equal(cs[a].download(), cd[a]), "c is read only"
    for k, x in zip(masks, md):
        assert np.array_equal(k.download(), x), "the masks are read only"
    return outs


# ---- 1. the kernel against the sequence it replaces ----
@pytest.mark.parametrize("m", [85, 119, 1785])
def test_mask_fan_equals_copy_and_multiply(hx, m):
    """N = 64; 96 (48 vectors: fewer than one workgroup's threads); 768 (384 vectors: two workgroups, the second
    partial).  Batch 5 leaves the BP = 4 kernel a tail of one element."""
    c, primes = _ctx(hx, m)
    assert c.phim == {85: 64, 119: 96, 1785: 768}[m]
    rng = np.random.default_rng(m)
    for parts in (1, 2):
        for batch in (1, 3, 5):
            for nout in (1, 2, 3, 5, 9):
                for mask_batch in sorted({1, batch}):
                    for superset in (False, True):
                        _fan_case(hx, c, primes, rng, parts, batch, nout, mask_batch, superset)


def test_mask_fan_into_lazy_copies_of_c(hx):
    """hx_poly_copy shares rows until one side is written: outputs that share c's rows let go of them, c and a
    bystander copy keep theirs"""
    c, primes = _ctx(hx, 1785)
    rng = np.random.default_rng(2)
    idx, B, n = [0, 1, 2], 3, c.phim
    x0, x1 = _rand(rng, primes, idx, B, n), _rand(rng, primes, idx, B, n)
    md = [_rand(rng, primes, idx, 1, n) for _ in range(4)]
    masks = [hx.DoubleCRT(c, idx, 1, v) for v in md]
    c0, c1 = hx.DoubleCRT(c, idx, B, x0), hx.DoubleCRT(c, idx, B, x1)
    out0, out1 = [c0.copy() for _ in masks], [c1.copy() for _ in masks]
    bystander = c0.copy()
    hx.maskFan(out0, out1, c0, c1, masks)
    assert np.array_equal(c0.download(), x0) and np.array_equal(c1.download(), x1)
    assert np.array_equal(bystander.download(), x0)
    want = _sequence(c, [c0, c1], masks)
    for t in range(len(masks)):
        assert np.array_equal(out0[t].download(), want[t][0].download())
        assert np.array_equal(out1[t].download(), want[t][1].download())


def test_mask_fan_in_a_graph_capture(hx):
    c, primes = _ctx(hx, 1785)
    rng = np.random.default_rng(4)
    n, idx, B, K = c.phim, [0, 1, 2], 5, 5
    x = [_rand(rng, primes, idx, B, n) for _ in range(2)]
    md = [_rand(rng, primes, idx, 1 if t % 2 else B, n) for t in range(K)]
    masks = [hx.DoubleCRT(c, idx, v.shape[1], v) for v in md]
    direct = [hx.DoubleCRT(c, idx, B, v) for v in x]
    want = [[w.download() for w in row] for row in _sequence(c, direct, masks)]
    d0, d1 = [hx.likeUninit(direct[0]) for _ in range(K)], [hx.likeUninit(direct[0]) for _ in range(K)]
    hx.maskFan(d0, d1, direct[0], direct[1], masks)                 # eagerly once
    ops = [hx.DoubleCRT(c, idx, B, v) for v in x]
    o0 = [hx.DoubleCRT(c, idx, B) for _ in range(K)]
    o1 = [hx.DoubleCRT(c, idx, B) for _ in range(K)]
    c.graphBegin()
    hx.maskFan(o0, o1, ops[0], ops[1], masks)
    graph = c.graphEnd()
    for d, v in zip(ops, x):                                        # (nothing ran yet)
        d.upload(v)
    # eager calls between the recording and its replays rewrite the shared table and its staging ring
    for _ in range(5):
        hx.maskFan(d0[:2], None, direct[0], None, masks[:2])
    graph.launch()
    for t in range(K):
        assert np.array_equal(o0[t].download(), want[t][0]) and np.array_equal(o1[t].download(), want[t][1])
        assert np.array_equal(d0[t].download(), want[t][0])
    # fresh operands in the same polys
    y = [_rand(rng, primes, idx, B, n) for _ in range(2)]
    for d, v in zip(ops, y):
        d.upload(v)
    graph.launch()
    ref = _sequence(c, [hx.DoubleCRT(c, idx, B, v) for v in y], masks)
    for t in range(K):
        assert np.array_equal(o0[t].download(), ref[t][0].download())
        assert np.array_equal(o1[t].download(), ref[t][1].download())
    for d, v in zip(ops, y):
        assert np.array_equal(d.download(), v)
    graph.destroy()


def test_mask_fan_refusals_touch_nothing(hx):
    c, primes = _ctx(hx, 119)
    other, _ = _ctx(hx, 119)
    rng = np.random.default_rng(6)
    n, idx, B = c.phim, [0, 1], 3
    xs = [_rand(rng, primes, idx, B, n) for _ in range(6)]
    c0, c1, a0, a1, b0, b1 = (hx.DoubleCRT(c, idx, B, x) for x in xs)
    md = [_rand(rng, primes, [0, 1, 2], 1, n), _rand(rng, primes, [1, 0], B, n)]
    k0, k1 = hx.DoubleCRT(c, [0, 1, 2], 1, md[0]), hx.DoubleCRT(c, [1, 0], B, md[1])
    L = hx.lib()

    def arr(ps):
        return None if ps is None else (C.c_void_p * max(len(ps), 1))(*[p.h if p is not None else None for p in ps])

    def refused(code, match, out0, out1, cc0, cc1, masks, nout=None):
        rc = L.hx_mask_fan(arr(out0), arr(out1), len(out0) if nout is None else nout, cc0.h if cc0 is not None else None,
                           cc1.h if cc1 is not None else None, arr(masks))
        assert rc == code, (match, rc, L.hx_last_error())
        assert match.encode() in L.hx_last_error(), (match, L.hx_last_error())
        for d, x in zip((c0, c1, a0, a1, b0, b1), xs):
            assert np.array_equal(d.download(), x), match
        assert np.array_equal(k0.download(), md[0]) and np.array_equal(k1.download(), md[1]), match

    INV, PS, UNS = hx.HX_ERR_INVALID, hx.HX_ERR_PRIMESET, hx.HX_ERR_UNSUPPORTED
    ks = [k0, k1]
    refused(INV, "null argument", None, None, c0, None, ks, nout=2)
    refused(INV, "null argument", [a0, b0], None, None, None, ks)
    refused(INV, "null argument", [a0, b0], None, c0, None, None)
    refused(INV, "null poly (output 1)", [a0, None], None, c0, None, ks)
    refused(INV, "null poly (output 0)", [a0, b0], None, c0, None, [None, k1])
    refused(INV, "null poly (output 1)", [a0, b0], [a1, None], c0, c1, ks)
    refused(INV, "go together", [a0, b0], [a1, b1], c0, None, ks)
    refused(INV, "go together", [a0, b0], None, c0, c1, ks)
    # aliasing: distinct outputs, none of them c0, c1 or a mask
    refused(INV, "also c0, c1 or a mask", [a0, c0], None, c0, None, ks)
    refused(INV, "also c0, c1 or a mask", [a0, b0], [a1, c1], c0, c1, ks)
    refused(INV, "also c0, c1 or a mask", [a0, b0], [a1, c0], c0, c1, ks)
    one = hx.DoubleCRT(c, idx, B, xs[2])
    refused(INV, "also c0, c1 or a mask", [a0, one], None, c0, None, [k0, one])
    refused(INV, "appears twice", [a0, a0], None, c0, None, ks)
    refused(INV, "appears twice", [a0, b0], [a1, a0], c0, c1, ks)
    refused(INV, "the same poly", [a0, b0], [a1, b1], c0, c0, ks)
    # a foreign context
    fk = hx.DoubleCRT(other, idx, B, xs[0])
    fm = hx.DoubleCRT(other, [0, 1, 2], 1)
    refused(INV, "incompatible objects", [a0, fk], None, c0, None, ks)
    refused(INV, "incompatible objects", [a0, b0], [a1, fk], c0, c1, ks)
    refused(INV, "incompatible objects", [a0, b0], None, c0, None, [k0, fm])
    refused(INV, "incompatible objects", [a0, b0], [a1, b1], c0, fk, ks)
    # shapes: batch, rows, row order
    for bad in (hx.DoubleCRT(c, idx, B + 1), hx.DoubleCRT(c, [0], B), hx.DoubleCRT(c, [1, 0], B), hx.DoubleCRT(c, [0, 1, 2], B)):
        refused(INV, "output 1 differs", [a0, bad], None, c0, None, ks)
        refused(INV, "output 0 differs", [a0, b0], [bad, b1], c0, c1, ks)
        refused(INV, "c0 and c1 differ", [a0, b0], [a1, b1], c0, bad, ks)
    refused(INV, "neither 1 nor 3", [a0, b0], None, c0, None, [k0, hx.DoubleCRT(c, [0, 1, 2], 2)])
    # a mask missing a prime
    refused(PS, "no row for prime 1", [a0, b0], None, c0, None, [k0, hx.DoubleCRT(c, [0, 2], 1)])
    # nout
    refused(INV, "at least one output", [a0], None, c0, None, [k0], nout=0)
    refused(INV, "at least one output", [a0], None, c0, None, [k0], nout=-1)
    refused(UNS, "too many outputs", [a0], None, c0, None, [k0], nout=257)
    # more rows than one launch descriptor holds
    from helib_amd import hostnt
    big, gen = hx.Context(85), hostnt.PrimeGen(50, 85)
    for _ in range(161):
        big.add_prime(gen.next())
    wide = [hx.DoubleCRT(big, range(161), 1) for _ in range(3)]
    refused(UNS, "too many rows", [wide[0]], None, wide[1], None, [wide[2]])
    assert not any(w.download().any() for w in wide)
    # an odd number of coefficients: phi(m) is odd for m = 2 only (phi = 1); polys without rows reach the check
    tiny = hx.Context(2)
    assert tiny.phim == 1
    a, b, mk = (hx.DoubleCRT(tiny, [], 1, zero=False) for _ in range(3))
    with pytest.raises(hx.HxError, match="even number of coefficients") as e:
        hx.maskFan([a], None, b, None, [mk])
    assert e.value.code == UNS
    with pytest.raises(hx.InvalidArgument, match="maskFan"):
        hx.maskFan([a0], None, c0, None, ks)
    # 256 outputs are taken, and after all that the call still works
    many = [hx.likeUninit(c0) for _ in range(256)]
    hx.maskFan(many, None, c0, None, [k0, k1] * 128)
    hx.maskFan([a0, b0], [a1, b1], c0, c1, ks)
    want = _sequence(c, [c0, c1], ks)
    for t, (p, q) in enumerate(((a0, a1), (b0, b1))):
        assert np.array_equal(p.download(), want[t][0].download()) and np.array_equal(q.download(), want[t][1].download())
        assert np.array_equal(many[254 + t].download(), want[t][0].download())


_CHILD = r"""
import hashlib
import numpy as np
import torch  # noqa: F401
from helib_amd import capi as hx
from tests.test_permutations_gpu import _ctx, _fan_case, SWITCH_CASES
c, primes = _ctx(hx, 1785)
rng = np.random.default_rng(77)
h = hashlib.sha256()
for case in SWITCH_CASES:
    for part in _fan_case(hx, c, primes, rng, *case):
        for d in part:
            h.update(d.download().tobytes())
print("WORDS", h.hexdigest())
"""
SWITCH_CASES = [(2, 5, 3, 5, True), (1, 3, 9, 1, False), (2, 1, 2, 1, False)]


def test_no_mask_fan_switch_gives_the_same_words(hx):
    """HX_NO_MASK_FAN=1 is read when a context is created: a fresh child process runs the cases under it (there
    hx_mask_fan issues the copies and products itself), the parent runs them on the kernel; same random data, same
    words"""
    env = dict(os.environ, HX_NO_MASK_FAN="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    theirs = [ln.split()[1] for ln in out.stdout.splitlines() if ln.startswith("WORDS")]
    assert "HX_NO_MASK_FAN" not in os.environ
    c, primes = _ctx(hx, 1785)
    rng = np.random.default_rng(77)
    h = hashlib.sha256()
    for case in SWITCH_CASES:
        for part in _fan_case(hx, c, primes, rng, *case):
            for d in part:
                h.update(d.download().tobytes())
    assert theirs == [h.hexdigest()]


# ---- 2. end to end with real keys ----
def _chain(hx, m, p, bits, seed=5):
    from helib_amd import bgv_hypercube, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, 1, bits=bits, c=3)
    g = hx.Context(m)
    o = O.Ctx(m)
    for q in cc.primes:
        i = o.add_prime(q)
        g.add_prime(q, o.roots[i])
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    ea = bgv_hypercube.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    return cc, g, sk, ea


def _same(x, y):
    assert (x.lnNoise, x.ptxtMag, x.primeSet, x.intFactor, x.ptxtSpace) == (y.lnNoise, y.ptxtMag, y.primeSet, y.intFactor,
                                                                            y.ptxtSpace)
    assert sorted(x.parts, key=str) == sorted(y.parts, key=str)
    for h in x.parts:
        assert np.array_equal(x.parts[h].download(), y.parts[h].download()), h


# (m, p, bits, a depth bound with room for every Benes level the optimiser wants, one that makes it collapse them)
CHAINS = [(255, 2, 600, 12, 3), (527, 2, 600, 12, 3), (1785, 2, 700, 12, 5)]


@pytest.mark.parametrize("m,p,bits,deep,shallow", CHAINS)
def test_permutations_with_keys(hx, monkeypatch, m, p, bits, deep, shallow):
    """identity, reversal and two random permutations through PermPrecomp, fused (the kernel) and unfused from clones
    of one ciphertext: the same words and bookkeeping, and the permuted plaintext"""
    from helib_amd import keys as hk, permutations as P
    cc, g, sk, ea = _chain(hx, m, p, bits)
    assert ea.zMStar.signedOrds() == H.RINGS[m, p]
    B, n = 3, ea.size()
    rng = np.random.default_rng(m)
    a = rng.integers(0, p, size=(B, n))
    a[0] = 0
    a[0, 0] = 1
    # every network and its matrices first: a ciphertext sees the matrices its key had when it was made
    nets = {}
    for depth in (deep, shallow):
        pip = P.PermIndepPrecomp(ea, depth)
        assert pip.getDepth() <= depth
        nets[depth] = [P.PermPrecomp(pip, pi)
                       for pi in (np.arange(n), np.arange(n)[::-1].copy(), P.randomPerm(n, rng), P.randomPerm(n, rng))]
        for pp in nets[depth]:
            hk.addMatrices4Network(sk, pp.net)
    fresh = ea.encrypt_batch(sk, a)
    fans = []
    real = hx.maskFan
    monkeypatch.setattr(hx, "maskFan", lambda o0, o1, c0, c1, masks: (fans.append(len(masks)), real(o0, o1, c0, c1, masks))[1])
    assert P.PermNetwork.fuseMaskFan in (True, False)
    for depth in (deep, shallow):
        widest = 0
        for pp in nets[depth]:
            pi = pp.pi
            ks = [len(pp.net.getLayer(i).amounts()) for i in range(pp.net.depth()) if not pp.net.getLayer(i).isID]
            widest = max([widest] + ks)
            res = {}
            for fused in (True, False):
                del fans[:]
                ct = fresh.clone()
                assert pp.apply(ct, fused=fused) is ct
                assert np.array_equal(ea.decrypt_batch(ct, sk), P.applyPermToVec(a.T, pi).T), (depth, pi, fused)
                assert np.array_equal(pp.apply(a), P.applyPermToVec(a.T, pi).T)
                assert ct.isCorrect(), (depth, pi, fused)
                assert fans == (ks if fused else []), (fans, ks)   # one call per layer on a two-part ciphertext
                res[fused] = ct
            _same(res[True], res[False])
        if depth == shallow:
            assert widest > 3                                   # the nout > 3 path ran under real use


def test_permutation_of_galois_ring_slots(hx):
    """bgv_gr at m = 85, p^r = 16: slots [B, nslots, d], whole slot values move"""
    from helib_amd import bgv_gr, ctxt as hc, keys as hk, permutations as P
    m, p, r = 85, 2, 4
    cc = hc.ChainContext(m, p, r, bits=300, c=3)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=5)
    sk.GenSecKey()
    ea = bgv_gr.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    B, n, d = 3, ea.size(), ea.getDegree()
    rng = np.random.default_rng(m)
    a = rng.integers(0, p ** r, size=(B, n, d))
    pi = P.randomPerm(n, rng)
    pp = P.PermPrecomp(P.PermIndepPrecomp(ea, 3), pi)
    hk.addMatrices4Network(sk, pp.net)
    fresh = ea.encrypt_batch(sk, a)
    res = {}
    for fused in (True, False):
        ct = fresh.clone()
        pp.apply(ct, fused=fused)
        assert np.array_equal(ea.decrypt_batch(ct, sk), a[:, pi]) and ct.isCorrect()
        res[fused] = ct
    assert np.array_equal(pp.apply(a), a[:, pi])
    _same(res[True], res[False])


def test_permutation_of_ckks_slots(hx):
    """m = 128: 32 slots, one native dimension; the tolerance is the scheme's own errorBound of the result"""
    from helib_amd import ckks, ctxt as hc, keys as hk, permutations as P
    m = 128
    cc = hc.ChainContext(m, -1, 20, bits=300, c=3, ckks=True)
    g = hx.Context(m)
    o = O.Ctx(m)
    for q in cc.primes:
        i = o.add_prime(q)
        g.add_prime(q, o.roots[i])
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=5)
    sk.GenSecKey(maxDegKswitch=2)
    ea = ckks.EncryptedArrayCx(cc, g)
    n = ea.size()
    assert n == 32
    rng = np.random.default_rng(9)
    v = (rng.uniform(-1, 1, (1, n)) + 1j * rng.uniform(-1, 1, (1, n))) / np.sqrt(2)
    pi = P.randomPerm(n, rng)
    pp = P.PermPrecomp(P.PermIndepPrecomp(ea, 3), pi)
    assert pp.net.depth() == 3
    hk.addMatrices4Network(sk, pp.net)
    ct = ea.encrypt_batch(sk, v)
    pp.apply(ct)
    got = ea.rawDecrypt_batch(ct, sk)
    err, bound = float(np.max(np.abs(got - v[:, pi]))), ckks.errorBound(ct)
    print(f"max slot error {err:.3e}, errorBound {bound:.3e}")
    assert err <= bound
    assert np.array_equal(pp.apply(v), v[:, pi])
    with pytest.raises(ckks.LogicError, match="no fused mask stage"):
        pp.apply(ct, fused=True)
