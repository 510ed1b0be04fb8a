"""hx_bgv_encode_diagonals against hx_bgv_encode of numpy-built diagonals (every word of the constants and of the zzX),
its refusals, and the BGV matrix products (helib_amd.bgv_matmul) with real keys against numpy on the plaintext slots,
the device and the host construction path giving the same ciphertext words.  Everything here is an integer: every
comparison is exact."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import bgv_slots_ref as R

pytestmark = pytest.mark.gpu

RINGS = [(16, 17), (105, 211), (1024, 12289)]


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


class _Geom:
    """what bgv_matmul.diagonalSlots asks of an EncryptedArray (the formula itself is held to the reference's loops
    in tests/test_bgv_matmul_host.py)"""

    def __init__(self, table, n):
        from helib_amd import hostnt
        self.p, self.n = table.p, n
        self.zMStar = hostnt.ZmStar(table.context.m, table.p, table.gens, table.ords)

    def size(self):
        return self.n


def _matrix(rng, D, p):
    """entries below 0 and above p, with 0 and p - 1 among them"""
    a = rng.integers(-2 * p, 3 * p, size=(D, D))
    a.flat[:4] = [0, p - 1, -1, p]
    return a


def _descs(geom, dim, rng, count):
    """`count` descriptors: the offsets run through every dimension, the rotations through 0, 1, ord - 1 and a
    negative amount, along every dimension and none (-1)"""
    ords = geom.zMStar.ords
    out = []
    for t in range(count):
        off = [int(rng.integers(-o, 2 * o)) for o in ords]
        if dim >= 0:
            off[dim] = t
        rd = t % (len(ords) + 1) - 1
        amt = 0 if rd < 0 else [0, 1, ords[rd] - 1, -3][(t // (len(ords) + 1)) % 4]
        out.append((off, rd, amt))
    return out


def _compare(hx, table, geom, a, dim, descs, idx):
    from helib_amd import bgv_matmul as M
    mat = hx.BgvMatrix(table, a, dim)
    slots = np.stack([M.diagonalSlots(geom, a, dim, *d) for d in descs])
    got, cf, nz = hx.bgvEncodeDiagonals(table, mat, descs, idx, coeffs=True)
    want, wcf = hx.bgvEncode(table, slots, idx, coeffs=True)
    assert np.array_equal(cf, wcf), (dim, len(descs))
    assert np.array_equal(got.download(), want.download()), (dim, len(descs))
    assert nz.tolist() == [bool(np.any(s % table.p)) for s in slots]
    assert np.array_equal(hx.bgvEncodeDiagonals(table, mat, descs)[2], nz)          # the flags alone
    return slots, cf, nz


# ---- 1. the kernel against the existing encode ----
@pytest.mark.parametrize("m,p", RINGS)
def test_encode_diagonals_equals_encode_of_numpy_diagonals(hx, m, p):
    c, primes = _ctx(hx, m)
    table = hx.BgvSlots(c, p)
    n = c.phim
    geom = _Geom(table, n)
    ords = table.ords
    rng = np.random.default_rng(m)
    st = [int(np.prod(ords[i + 1:])) for i in range(len(ords))]
    for dim in [-1] + list(range(len(ords))):
        D = n if dim < 0 else ords[dim]
        a = _matrix(rng, D, p)
        if dim >= 0 and D > 3:
            j = np.arange(D)
            a[(j - 2) % D, j] = p * rng.integers(-2, 3, size=D)          # diagonal 2: zero mod p
            a[(j - 3) % D, j] = 0
            a[(1 - 3) % D, 1] = -1                                       # diagonal 3: a single non-zero entry
        if dim < 0:
            s = np.arange(n)
            a[(s + st[0]) % n, s] = p * rng.integers(-2, 3, size=n)      # off = (-1, 0, ...) zero mod p
            a[(s + 2 * st[0]) % n, s] = 0
            a[(5 + 2 * st[0]) % n, 5] = p + 1                            # off = (-2, 0, ...) a single non-zero entry
        for count in sorted({1, 3, D}):
            descs = _descs(geom, dim, rng, count)
            if count == D and dim < 0:
                descs[1] = ([-1] + [0] * (len(ords) - 1), 0, 1)
                descs[2] = ([-2] + [0] * (len(ords) - 1), -1, 0)
            idx = [0, 2] if count == 3 else [0, 1, 2]
            slots, cf, nz = _compare(hx, table, geom, a, dim, descs, idx)
            if count == D and D > 3:
                if dim >= 0:
                    assert not nz[2] and nz[3] and np.count_nonzero(slots[3]) == n // D
                else:
                    assert not nz[1] and nz[2] and np.count_nonzero(slots[2]) == 1
            if m == 16:                                                  # python integers, independent of any kernel
                for t in range(len(descs)):
                    assert np.array_equal(cf[t], R.encode_crt(slots[t], m, p)), (dim, t)
                    assert R.decode(cf[t][None], m, p)[0].tolist() == [int(x) for x in slots[t]]


def test_wide_entries_and_a_poly_on_no_primes(hx):
    """any int64 is an entry; idx = [] gives the zzX alone"""
    m, p = 1024, 12289
    c, primes = _ctx(hx, m)
    table = hx.BgvSlots(c, p)
    geom = _Geom(table, c.phim)
    rng = np.random.default_rng(3)
    a = rng.integers(-2 ** 63, 2 ** 63 - 1, size=(256, 256), dtype=np.int64)
    a[0, :2] = [-2 ** 63, 2 ** 63 - 1]
    descs = _descs(geom, 0, rng, 5)
    _compare(hx, table, geom, a, 0, descs, [1])
    _compare(hx, table, geom, a, 0, descs, [])


# ---- 2. refusals ----
def test_refusals_touch_nothing(hx):
    m, p = 1024, 12289
    c, primes = _ctx(hx, m)
    table = hx.BgvSlots(c, p)
    n = c.phim
    good = np.ones((256, 256), dtype=np.int64)
    for a, dim in ((np.ones((256, 255), dtype=np.int64), 0), (np.ones((2, 2), dtype=np.int64), 0), (good, 1), (good, -1),
                   (good, 2), (good, -2), (np.ones((n, n + 1), dtype=np.int64), -1)):
        with pytest.raises(hx.InvalidArgument):
            hx.BgvMatrix(table, a, dim)
    with pytest.raises(hx.InvalidArgument, match="two axes"):
        hx.BgvMatrix(table, np.ones(4, dtype=np.int64), 0)
    mat = hx.BgvMatrix(table, good, 0)
    rng = np.random.default_rng(0)
    seed = rng.integers(0, primes[0], size=(1, 2, n), dtype=np.uint64)
    out = hx.DoubleCRT(c, [0], 2, seed)
    descs = [([1, 0], 0, 0), ([2, 0], 0, 0)]

    def untouched():
        assert np.array_equal(out.download(), seed)
    other = hx.BgvSlots(c, p)                                            # a matrix from another table
    with pytest.raises(hx.InvalidArgument, match="another slot table"):
        hx.bgvEncodeDiagonals(other, mat, descs, out=out)
    untouched()
    with pytest.raises(hx.InvalidArgument, match="rot_dim"):
        hx.bgvEncodeDiagonals(table, mat, [([1, 0], 2, 0), ([2, 0], 0, 0)], out=out)
    untouched()
    with pytest.raises(hx.InvalidArgument, match="output batch"):
        hx.bgvEncodeDiagonals(table, mat, descs[:1], out=out)
    untouched()
    c2, _ = _ctx(hx, m)
    with pytest.raises(hx.InvalidArgument, match="another context"):
        hx.bgvEncodeDiagonals(table, mat, descs, out=hx.DoubleCRT(c2, [0], 2))
    with pytest.raises(hx.InvalidArgument, match="null argument"):
        hx._chk(hx.lib().hx_bgv_encode_diagonals(table.h, mat.h, None, 1, out.h, None, None))
    untouched()
    c.graphBegin()                                                       # an open graph capture
    try:
        with pytest.raises(hx.InvalidArgument, match="cannot be captured"):
            hx.bgvEncodeDiagonals(table, mat, descs, out=out)
        with pytest.raises(hx.InvalidArgument, match="cannot be captured"):
            hx.BgvMatrix(table, good, 0)
    finally:
        try:
            c.graphEnd().destroy()
        except hx.HxError:
            pass               # (nothing was recorded)
    untouched()
    got, _, nz = hx.bgvEncodeDiagonals(table, mat, descs, out=out)       # and the device is as it was
    assert got is out and nz.all()
    want = hx.bgvEncode(table, np.ones((2, n), dtype=np.int64), [0])
    assert np.array_equal(out.download(), want.download())


# ---- 3. end to end with real keys ----
def _chain(hx, m, p, bits, family, seed=5):
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
    getattr(hk, family)(sk)
    return cc, g, sk, ea


def _same(x, y):
    assert (x.lnNoise, x.primeSet, x.intFactor, x.ptxtSpace) == (y.lnNoise, y.primeSet, y.intFactor, y.ptxtSpace)
    assert sorted(x.parts, key=str) == sorted(y.parts, key=str)
    for h in x.parts:
        assert np.array_equal(x.parts[h].download(), y.parts[h].download()), h


def _same_constants(x, y):
    assert [mm is None for mm in x.multiplier] == [mm is None for mm in y.multiplier]
    for a, b in zip(x.multiplier, y.multiplier):
        if a is not None:
            assert a[1] == b[1] and a[0].batch == 1 and np.array_equal(a[0].download(), b[0].download())


# bits: 900 leaves the reference's bookkeeping (isCorrect, asserted below) room for the product and its key switches
@pytest.mark.parametrize("m,p,family", [(105, 211, "add1DMatrices"), (1024, 12289, "addBSGS1DMatrices")])
def test_matmul_full_with_keys(hx, m, p, family):
    from helib_amd import bgv_matmul as M
    cc, g, sk, ea = _chain(hx, m, p, 900, family)
    n, B = ea.size(), 3
    rng = np.random.default_rng(m)
    a = rng.integers(0, p, size=(n, n))
    v = rng.integers(0, p, size=(B, n))
    full = M.MatMulFull(ea, a)
    dev = M.MatMulFullExec(ea, full, device_diagonals=True)
    host = M.MatMulFullExec(ea, full, device_diagonals=False)
    assert all(t.onDevice for t in dev.transforms) and not any(t.onDevice for t in host.transforms)
    for x, y in zip(dev.transforms, host.transforms):
        _same_constants(x, y)
    fresh = ea.encrypt_batch(sk, v)
    res = []
    for ex in (dev, host):
        ct = fresh.clone()
        assert ex.mul(ct, pk=sk) is ct
        assert np.array_equal(ea.decrypt_batch(ct, sk), np.array(v.astype(object) @ a.astype(object) % p, dtype=np.int64))
        assert ct.isCorrect()
        res.append(ct)
    _same(*res)
    assert np.array_equal(M.mulPlain(ea, v, full), ea.decrypt_batch(res[0], sk))


@pytest.mark.parametrize("family", ["addBSGS1DMatrices", "addMinimal1DMatrices"])
def test_matmul1d_with_keys(hx, family):
    from helib_amd import bgv_matmul as M, linalg
    m, p = 1024, 12289
    cc, g, sk, ea = _chain(hx, m, p, 900, family)
    n, B = ea.size(), 3
    assert ea.zMStar.ords == [256, 2]
    rng = np.random.default_rng(17)
    v = rng.integers(0, p, size=(B, n))
    fresh = ea.encrypt_batch(sk, v)
    minimal = family == "addMinimal1DMatrices"
    for dim, D in ((0, 256), (1, 2)):
        a = rng.integers(-p, 2 * p, size=(D, D))
        if D > 2:                                        # banded: 100 live diagonals, past one chunk of 64
            j = np.arange(D)
            for i in range(100, D):
                a[(j - i) % D, j] = 0
        mat = M.MatMul1D(ea, a, dim)
        dev = M.MatMul1DExec(ea, mat, minimal=minimal, device_diagonals=True)
        host = M.MatMul1DExec(ea, mat, minimal=minimal, device_diagonals=False)
        assert dev.onDevice and not host.onDevice and dev.g == (16 if D > 2 else 0)
        if D > 2:
            assert [i for i, mm in enumerate(dev.multiplier) if mm is not None] == list(range(100))
        _same_constants(dev, host)
        want = M.mulPlain(ea, v, mat)
        x = np.moveaxis(v.reshape(B, 256, 2), 1 + dim, -1).astype(object)
        assert np.array_equal(want, np.array(np.moveaxis(x @ (a.astype(object) % p) % p, -1, 1 + dim).reshape(B, n),
                                             dtype=np.int64))
        res = []
        for ex, fused in ((dev, True), (host, False)):
            ct = fresh.clone()
            before = linalg.MatMul1DExec.fallbacks
            assert ex.mul(ct, pk=sk, fused=fused) is ct
            if fused and ex.g and not minimal:
                assert linalg.MatMul1DExec.fallbacks == before       # hoisted baby steps: every group fuses
            assert np.array_equal(ea.decrypt_batch(ct, sk), want), (family, dim, fused)
            assert ct.isCorrect(), (family, dim)
            res.append(ct)
        _same(*res)
