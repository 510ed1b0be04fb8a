"""hx_mul_add_circulant against the hx_mul / hx_add sequence it replaces (every word), and helib_amd.intraslot with real
keys on the device: unpack against unpackPlain, repack(unpack) against the input, the fused path against the reference's
sequence word for word and field for field.  Everything here is an integer: every comparison is exact.

Chain sizes of the end-to-end cases: bits = 300, c = 2 for every ring -- the chain the existing Frobenius tests use at
m = 85, and the one at which tests/test_intraslot_host.py shows the unfused unpack and the repack of these rings correct
with isCorrect() true (asserted again here)."""
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


@pytest.fixture(scope="module")
def rings(hx):
    """one context of five primes just below 2^60 per ring: N = phi(m) = 30, 64, 640"""
    out = {}
    for m in (31, 85, 641):
        g = hostnt.PrimeGen(60, m)
        c = hx.Context(m)
        for _ in range(5):
            c.add_prime(g.next())
        assert all((1 << 59) < q < (1 << 60) for q in c.primes)
        out[m] = c
    assert [out[m].phim for m in (31, 85, 641)] == [30, 64, 640]
    return out


KEY = bytes(range(32))


def _rand(hx, c, idx, batch, stream):
    return hx.DoubleCRT(c, idx, batch, zero=False).randomize(KEY, stream)


def _sequence(hx, consts, ins, nout):
    """out[i] = in[0] * c[i]; then per j >= 1: tmp = in[j]; tmp *= c[(i + j) mod d]; out[i] += tmp"""
    d, outs = len(consts), []
    for i in range(nout):
        out = ins[0].copy()
        out *= consts[i]
        for j in range(1, d):
            tmp = ins[j].copy()
            tmp *= consts[(i + j) % d]
            out += tmp
        outs.append(out)
    return outs


# (m, d, nout, batch, prime rows, constants per batch element, constants on a superset, parts).  N = 30 is one partly
# filled block of threads, 640 two blocks; d = 3, 5 are no powers of two; nout = 2, 5, 7, 15, 63 are no multiples of the
# output block (4 for nout <= 4, else 8) and nout < d; nout = 16, 64 fill two and eight blocks; batch 3 and 17 are odd
CASES = [(31, 1, 1, 1, 1, False, False, 2), (31, 2, 1, 3, 4, False, True, 2), (85, 2, 2, 1, 1, True, False, 1),
         (85, 3, 2, 17, 1, True, False, 2), (641, 3, 3, 3, 4, False, False, 2), (85, 5, 5, 3, 4, False, False, 1),
         (31, 5, 4, 17, 4, True, True, 2), (641, 8, 7, 3, 1, False, True, 2), (85, 8, 8, 17, 4, False, False, 2),
         (641, 16, 16, 1, 4, True, True, 2), (85, 16, 15, 17, 1, False, False, 2), (31, 64, 64, 3, 4, False, False, 2),
         (641, 64, 63, 1, 1, False, False, 1), (85, 64, 1, 3, 1, True, False, 2)]


@pytest.mark.parametrize("m,d,nout,batch,rows,cper,superset,parts", CASES)
def test_mul_add_circulant_equals_the_sequence(hx, rings, m, d, nout, batch, rows, cper, superset, parts):
    c = rings[m]
    own = [0] if rows == 1 else [0, 3, 1, 2]
    cidx = [4, 3, 2, 1, 0] if superset else own
    consts = [_rand(hx, c, cidx, batch if cper else 1, 1000 + t) for t in range(d)]
    ins = [[_rand(hx, c, own, batch, 5000 * (p + 1) + t) for t in range(d)] for p in range(parts)]
    want = [[o.download() for o in _sequence(hx, consts, ins[p], nout)] for p in range(parts)]
    outs = [[_rand(hx, c, own, batch, 90 + 100 * p + i) for i in range(nout)] for p in range(parts)]      # overwritten
    hx.mulAddCirculant(outs[0], outs[1] if parts == 2 else None, consts, ins[0], ins[1] if parts == 2 else None)
    for p in range(parts):
        for i in range(nout):
            assert np.array_equal(outs[p][i].download(), want[p][i]), (p, i)


def test_worst_case_accumulator(hx, rings):
    """d = 64, every operand word q - 1, primes just below 2^60: the largest value the 128-bit accumulator reaches,
    64 (q - 1)^2 < 2^126, reduced once"""
    c, d, batch = rings[85], 64, 3
    idx = [0, 1, 2]
    N = c.phim
    full = np.stack([np.full((batch, N), c.primes[i] - 1, dtype=np.uint64) for i in idx])
    ins = [hx.DoubleCRT(c, idx, batch, full) for _ in range(d)]
    ins1 = [hx.DoubleCRT(c, idx, batch, full) for _ in range(d)]
    ks = [hx.DoubleCRT(c, idx, 1, full[:, :1]) for _ in range(d)]
    o0 = [hx.DoubleCRT(c, idx, batch) for _ in range(d)]
    o1 = [hx.DoubleCRT(c, idx, batch) for _ in range(d)]
    hx.mulAddCirculant(o0, o1, ks, ins, ins1)
    want = np.stack([np.full((batch, N), d * (c.primes[i] - 1) ** 2 % c.primes[i], dtype=np.uint64) for i in idx])
    for o in o0 + o1:
        assert np.array_equal(o.download(), want)


def test_error_returns_leave_the_outputs_untouched(hx, rings):
    c = rings[85]
    d = 3
    ins = [_rand(hx, c, [0, 1], 3, 10 + t) for t in range(d)]
    ks = [_rand(hx, c, [0, 1], 1, 20 + t) for t in range(d)]
    outs = [_rand(hx, c, [0, 1], 3, 30 + t) for t in range(d)]
    before = [o.download() for o in outs + ins + ks]
    with pytest.raises(hx.InvalidArgument, match="also an input"):
        hx.mulAddCirculant([outs[0], ins[1], outs[2]], None, ks, ins, None)
    with pytest.raises(hx.InvalidArgument, match="also an input"):
        hx.mulAddCirculant([outs[0], ks[2]], None, ks, ins, None)
    with pytest.raises(hx.InvalidArgument, match="appears twice"):
        hx.mulAddCirculant([outs[0], outs[0]], None, ks, ins, None)
    with pytest.raises(hx.InvalidArgument, match="appears twice"):
        hx.mulAddCirculant(outs[:2], [outs[2], outs[1]], ks, ins, ins)
    with pytest.raises(hx.InvalidArgument, match="no row for prime"):
        hx.mulAddCirculant(outs, None, [_rand(hx, c, [0], 1, 4)] + ks[1:], ins, None)
    with pytest.raises(hx.InvalidArgument, match="batch"):
        hx.mulAddCirculant(outs, None, [_rand(hx, c, [0, 1], 2, 5)] + ks[1:], ins, None)
    with pytest.raises(hx.InvalidArgument, match="differs"):
        hx.mulAddCirculant(outs, None, ks, [_rand(hx, c, [0, 2], 3, 6)] + ins[1:], None)
    with pytest.raises(hx.InvalidArgument):
        hx.mulAddCirculant(outs, None, ks, ins, ins)                         # out1 and in1 go together
    with pytest.raises(hx.InvalidArgument):
        hx.mulAddCirculant([], None, ks, ins, None)                          # nout < 1
    arr = (C.c_void_p * 65)(*[ins[0].h] * 65)
    L = hx.lib()
    assert L.hx_mul_add_circulant(arr, None, 1, arr, arr, None, 65) == hx.HX_ERR_UNSUPPORTED and b"64" in L.hx_last_error()
    assert L.hx_mul_add_circulant(arr, None, 4, arr, arr, None, 3) == hx.HX_ERR_INVALID
    assert L.hx_mul_add_circulant(None, None, 1, arr, arr, None, 1) == hx.HX_ERR_INVALID

    def raw(out0, out1, consts, in0, in1, nout=None):
        def pa(ps):
            return (C.c_void_p * len(ps))(*[p.h if p is not None else None for p in ps]) if ps is not None else None
        return L.hx_mul_add_circulant(pa(out0), pa(out1), len(out0) if nout is None else nout, pa(consts), pa(in0), pa(in1),
                                      len(consts))
    INV, UNS = hx.HX_ERR_INVALID, hx.HX_ERR_UNSUPPORTED
    assert raw(outs, None, ks, ins, ins) == INV and b"go together" in L.hx_last_error()
    assert raw(outs[:2], outs[2:], ks, ins, None, nout=1) == INV and b"go together" in L.hx_last_error()
    assert raw([outs[0], None], None, ks, ins, None) == INV and b"null poly (output 1)" in L.hx_last_error()
    assert raw(outs, None, ks, [ins[0], None, ins[2]], None) == INV and b"null poly (term 1)" in L.hx_last_error()
    foreign = _rand(hx, rings[31], [0, 1], 3, 40)
    assert raw([outs[0], foreign], None, ks, ins, None) == INV and b"incompatible objects" in L.hx_last_error()
    assert raw(outs, None, ks, [ins[0], foreign, ins[2]], None) == INV and b"incompatible objects" in L.hx_last_error()
    assert raw(outs, None, [foreign] + ks[1:], ins, None) == INV and b"incompatible objects" in L.hx_last_error()
    assert raw([outs[0], _rand(hx, c, [0, 1], 2, 41)], None, ks, ins, None) == INV and b"the outputs differ" in L.hx_last_error()
    assert raw([outs[0], _rand(hx, c, [1, 0], 3, 42)], None, ks, ins, None) == INV and b"the outputs differ" in L.hx_last_error()
    assert raw(outs[:1], outs[1:2], ks, ins, [ins[0], _rand(hx, c, [0, 2], 3, 43), ins[2]]) == INV
    assert b"in1[1] differs from the outputs" in L.hx_last_error()
    # more rows than one launch descriptor holds (refused before the terms' shapes are looked at)
    big, gen = hx.Context(85), hostnt.PrimeGen(50, 85)
    for _ in range(161):
        big.add_prime(gen.next())
    wide, thin = hx.DoubleCRT(big, range(161), 1), hx.DoubleCRT(big, [5], 1)
    assert raw([wide], None, [thin], [thin], None) == UNS and b"too many rows" in L.hx_last_error()
    # an odd number of coefficients: phi(m) is odd for m = 2 only (phi = 1); polys without rows reach the check
    tiny = hx.Context(2)
    assert tiny.phim == 1
    ta, tb, tk = (hx.DoubleCRT(tiny, [], 1, zero=False) for _ in range(3))
    assert raw([ta], None, [tk], [tb], None) == UNS
    assert b"hx_mul_add_circulant needs an even number of coefficients" in L.hx_last_error()
    # batch 8192 in eight blocks of outputs: one more than the grid's third axis holds
    c31 = rings[31]
    many = [hx.DoubleCRT(c31, [0], 8192) for _ in range(57)]
    x, k1 = hx.DoubleCRT(c31, [0], 8192), hx.DoubleCRT(c31, [0], 1)
    assert raw(many, None, [k1] * 57, [x] * 57, None) == UNS and b"exceeds the grid" in L.hx_last_error()
    assert not many[0].download().any() and not many[56].download().any()
    del many, x
    c.graphBegin()
    try:
        with pytest.raises(hx.HxError) as e:
            hx.mulAddCirculant(outs, None, ks, ins, None)
        assert e.value.code == hx.HX_ERR_UNSUPPORTED and "hx_mul_add_circulant uploads a pointer table" in str(e.value)
    finally:
        try:
            c.graphEnd().destroy()
        except hx.HxError:
            pass               # (nothing was recorded)
    for o, b in zip(outs + ins + ks, before):
        assert np.array_equal(o.download(), b)
    hx.mulAddCirculant(outs, None, ks, ins, None)                            # and the call still works
    want = _sequence(hx, ks, ins, d)
    assert all(np.array_equal(o.download(), w.download()) for o, w in zip(outs, want))


# ---- end to end with real keys ----
BITS = 300


def _chain(hx, m, p, r, seed=5):
    from helib_amd import bgv_gf, bgv_gr, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, r, bits=BITS, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    ea = (bgv_gf if r == 1 and m == 31 else bgv_gr).EncryptedArray(cc, g)     # (31, 2, 1) runs over helib_amd.bgv_gf
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    hk.addFrbMatrices(sk)
    return cc, g, sk, ea


class _Counted:
    """counts the hx_mul_add_circulant calls made through helib_amd.capi while it is open"""

    def __init__(self, hx):
        self.hx, self.calls = hx, []

    def __enter__(self):
        self.orig = self.hx.mulAddCirculant

        def counted(out0, out1, consts, in0, in1):
            self.calls.append((len(consts), len(out0)))
            return self.orig(out0, out1, consts, in0, in1)
        self.hx.mulAddCirculant = counted
        return self

    def __exit__(self, *exc):
        self.hx.mulAddCirculant = self.orig


def _fields(ct):
    return (sorted(ct.parts, key=str), ct.lnNoise, ct.primeSet, ct.ptxtSpace, ct.intFactor, ct.ptxtMag)


def _same(a, b):
    assert _fields(a) == _fields(b)
    for h in a.parts:
        assert a.parts[h].getIndexSet() == b.parts[h].getIndexSet()
        assert np.array_equal(a.parts[h].download(), b.parts[h].download()), h


@pytest.mark.parametrize("m,p,r", [(85, 2, 1), (31, 2, 1), (13, 3, 2), (85, 2, 4)])
def test_unpack_and_repack_with_real_keys(hx, m, p, r):
    from helib_amd import intraslot
    cc, g, sk, ea = _chain(hx, m, p, r)
    B, n, d, P = 3, ea.size(), ea.getDegree(), p ** r
    assert d == {85: 8, 31: 5, 13: 3}[m]
    a = np.random.default_rng(m + r).integers(0, P, size=(B, n, d))
    a[0, 0] = P - 1
    ct = ea.encrypt_batch(sk, a)
    if P > 2:
        ct.multByScalar(P - 1)                           # a unit: an intFactor other than 1 goes through both paths
        a = a * (P - 1) % P
    enc = intraslot.buildUnpackSlotEncoding(ea)
    want = intraslot.unpackPlain(ea, a)
    with _Counted(hx) as n_calls:
        plain = intraslot.unpack(ea, ct, enc, fused=False)
        assert n_calls.calls == []
        fused = intraslot.unpack(ea, ct, enc, fused=True)
    assert n_calls.calls == [(d, d)] and len(plain) == len(fused) == d
    for i, (u, v) in enumerate(zip(plain, fused)):
        assert u.isCorrect(), i
        got = ea.decrypt_batch(u, sk)
        assert np.array_equal(got[:, :, 0], want[:, :, i]) and not np.any(got[:, :, 1:]), i
        _same(u, v)
    k = max(1, d - 1)
    for u, v in zip(plain, intraslot.unpack(ea, ct, enc, n=k, fused=True)):
        _same(u, v)
    back = intraslot.repack(ea, fused)
    assert back.isCorrect() and np.array_equal(ea.decrypt_batch(back, sk), a)
    assert np.array_equal(ea.decrypt_batch(ct, sk), a)   # the input is left as it was


def test_circulant_combination_with_other_int_factors_and_prime_sets(hx):
    """terms whose intFactors differ (each multiplied by another unit of Z_9) and one of which sits on fewer primes:
    addCtxt harmonises with (e1, e2) and mods up; the fused form folds that into one mod-up and one product by an
    integer per term, and the words and fields are those of the sequence"""
    from helib_amd import ctxt as hc
    cc, g, sk, ea = _chain(hx, 13, 3, 2)
    B, n, d, P = 3, ea.size(), ea.getDegree(), 9
    rng = np.random.default_rng(8)
    vals, cts = [], []
    for j, u in enumerate((2, 4, 7)):
        a = rng.integers(0, P, size=(B, n, d))
        ct = ea.encrypt_batch(sk, a)
        ct.multByScalar(u)
        vals.append(a * u % P)
        cts.append(ct)
    cts[1].modDownToSet(sorted(cts[1].primeSet)[:-1])
    assert len({c.intFactor for c in cts}) > 1 and cts[1].primeSet != cts[0].primeSet
    ks = [rng.integers(0, P, size=(1, n, d)) for _ in range(d)]
    primes = sorted(frozenset().union(*[c.primeSet for c in cts]))
    consts = [ea.enc.encode(k, 1, primes) for k in ks]
    plain = hc.Ctxt.circulantCombination(cts, consts, fused=False)
    with _Counted(hx) as n_calls:
        fused = hc.Ctxt.circulantCombination(cts, consts, fused=True)
    assert n_calls.calls == [(d, d)]
    for i, (u, v) in enumerate(zip(plain, fused)):
        _same(u, v)
        want = sum(ea.mulPlain(np.broadcast_to(ks[(i + j) % d], vals[j].shape), vals[j]) for j in range(d)) % P
        assert v.isCorrect() and np.array_equal(ea.decrypt_batch(v, sk), want), i
    for c, a in zip(cts, vals):
        assert np.array_equal(ea.decrypt_batch(c, sk), a)                   # the terms are left as they were


def test_unpack_then_divide_by_p(hx):
    """slots 3 a' at p^r = 9: every coordinate is a multiple of 3, Ctxt.divideByP leaves c_i(a') mod 3, a ciphertext at
    p^(r-1) decoded through the p^r tables"""
    from helib_amd import intraslot
    m, p, r = 13, 3, 2
    cc, g, sk, ea = _chain(hx, m, p, r)
    n, d = ea.size(), ea.getDegree()
    a1 = np.random.default_rng(1).integers(0, 3, size=(3, n, d))
    ct = ea.encrypt_batch(sk, 3 * a1)
    enc = intraslot.buildUnpackSlotEncoding(ea)
    want = intraslot.unpackPlain(ea, a1) % 3
    for fused in (False, True):
        for i, u in enumerate(intraslot.unpack(ea, ct, enc, fused=fused)):
            u.divideByP()
            assert u.ptxtSpace == 3 and u.isCorrect()
            got = ea.decrypt_batch(u, sk)
            assert np.array_equal(got[:, :, 0], want[:, :, i]) and not np.any(got[:, :, 1:]), (fused, i)
