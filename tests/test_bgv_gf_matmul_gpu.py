"""Linear maps on GF(p^d) slots on the device (hx_bgv_gf_matrix_*, hx_bgv_gf_gather, helib_amd.bgv_gf_matmul) against
the restatement tests/bgv_gf_matmul_ref.py, the host path, and numpy on slot arrays after homomorphic products with real
keys.  Everything here is an integer: every comparison is exact."""
import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_gf_matmul_ref as MR
from tests import bgv_hypercube_ref as H

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


def _ctx(hx, m, nprimes=1, bits=60):
    g = hostnt.PrimeGen(bits, m)
    c = hx.Context(m)
    for _ in range(nprimes):
        c.add_prime(g.next())
    return c


def _ea(hx, m, p, bits=100):
    from helib_amd import bgv_gf, ctxt as hc
    cc = hc.ChainContext(m, p, 1, bits=bits, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    return bgv_gf.EncryptedArray(cc, g)


# ---- (a) bgv_gf_linpoly_kernel on every entry ----
# (803, 3): d = 60, d^2 = 3600 -- 57 column tiles, the last one partial, 225 staged steps
@pytest.mark.parametrize("m,p,D", [(31, 2, 6), (85, 2, 8), (13, 3, 4), (803, 3, 2)])
def test_linpoly_kernel_against_the_restatement(hx, m, p, D):
    from helib_amd import bgv_gf_matmul as GM
    ea = _ea(hx, m, p)
    ref = MR.tables(m, p) if m != 803 else None
    n, d = ea.size(), ea.getDegree()
    rng = np.random.default_rng(m)
    A = rng.integers(0, p, size=(1, D, D, d, d))
    A[0, 0, 0] = p - 1
    mat = hx.BgvGfMatrix(ea.enc.table, A, np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32) % D)
    C = mat.coeffs().astype(np.int64)
    assert C.shape == A.shape
    if ref is not None:
        for i in range(D):
            for j in range(D):
                assert MR.linpoly_holds(ref, C[0, i, j], A[0, i, j]), (i, j)
    else:
        # d = 60: the defining property on random elements, in the class's own field arithmetic (checked against the
        # restatement at the other rings): sum_k C[k] alpha^(p^k) = alpha A
        a = rng.integers(0, p, size=(1, n, d))
        for i in range(D):
            for j in range(D):
                want = np.array(a.astype(object) @ A[0, i, j].astype(object) % p, dtype=np.int64)
                assert np.array_equal(GM.evalLinPoly(ea, C[0, i, j], a), want), (i, j)
    assert np.array_equal(C, GM.buildLinPolyCoeffs(ea, A))


# ---- (b) lazy reduction, every word p - 1, at the largest prime below 2^31 ----
@pytest.mark.parametrize("m,d,n", [(64, 2, 16), (13, 6, 2)])
def test_linpoly_lazy_reduction_at_the_largest_prime(hx, m, d, n):
    from helib_amd import bgv_gf_matmul as GM
    p = 2147483647
    ref = MR.tables(m, p)
    assert (ref.d, ref.nslots, (1 << 64) // (p * p)) == (d, n, 4)
    ea = _ea(hx, m, p)
    A = np.full((n, 1, 1, d, d), p - 1, dtype=np.int64)
    A[1:] = np.random.default_rng(7).integers(0, p, size=(n - 1, 1, 1, d, d))
    mat = hx.BgvGfMatrix(ea.enc.table, A, np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
    C = mat.coeffs().astype(np.int64)
    for s in range(n):
        assert MR.linpoly_holds(ref, C[s, 0, 0], A[s, 0, 0]), s
    # the gather's Frobenius map at this prime: d = 6 > limit = 4 terms
    perm, frob = GM.slotAutomorph(ea, ea.zMStar.genToPow(-1, d - 1))
    maps = np.stack([np.arange(n), frob], axis=1).astype(np.int32)[None]
    got, nz = hx.bgvGfGather(mat, [(0, k, 0) for k in range(d)], maps)
    for k in range(d):
        assert np.array_equal(got[k], ea.frobeniusPlain(C[None, :, 0, 0, k], d - 1)[0]), k
    assert nz.all()


# ---- (c) bgv_gf_gather_kernel: identity, rotated, masked and Frobenius-twisted descriptors ----
@pytest.mark.parametrize("block", [True, False])
def test_gather_kernel_descriptors(hx, block):
    from helib_amd import bgv_gf_matmul as GM
    m, p = 85, 2
    ea = _ea(hx, m, p)
    ref = MR.tables(m, p)
    n, d, D, z = ea.size(), ea.getDegree(), ea.sizeOfDimension(0), ea.zMStar
    rng = np.random.default_rng(3 + block)
    mat = (GM.BlockMatMul1D(ea, rng.integers(0, p, size=(D, D, d, d)), 0) if block
           else GM.MatMul1D(ea, rng.integers(0, p, size=(D, D, d)), 0))
    maps = GM._Maps(ea)
    mask = ea.maskSlots(0, 3)
    rows = [maps.add(1), maps.add(z.genToPow(0, -2)), maps.add(1, mask), maps.add(z.genToPow(-1, -3)),
            maps.add(z.genToPow(0, D - 3) * z.genToPow(-1, -1) % m, 1 - mask), maps.add(1, np.zeros(n, dtype=np.int64))]
    ks = (0, 1, d - 1) if block else (0,)
    descs = [(i, k, mp) for i in (0, 3, D - 1) for k in ks for mp in rows]
    got, nz = hx.bgvGfGather(mat.handle(ea.enc), descs, np.stack(maps.rows))
    for t, (i, k, mp) in enumerate(descs):
        want = GM.hostConstant(ea, mat, i, k, maps.rows[mp])
        assert np.array_equal(got[t], want), (i, k, mp)
        assert bool(nz[t]) == bool(np.any(want))
    assert not nz[len(rows) - 1]
    # one of them against the literal substitution: the masked second half moved by rho^(D - 3) sigma^-1
    i, k = 3, ks[-1]
    v = (mat.slotValues(i, k) * (1 - mask)[:, None])[None]
    for a in (z.genToPow(-1, -1), z.genToPow(0, D - 3)):
        v = MR.automorph(ref, v, a)
    assert np.array_equal(got[descs.index((i, k, rows[4]))], v[0])


# ---- (d) real keys ----
def _chain(hx, m, p, bits, minimal=False, seed=5):
    from helib_amd import bgv_gf, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, 1, bits=bits, c=3)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    ea = bgv_gf.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    if minimal:
        hk.addMinimal1DMatrices(sk)
        hk.addMinimalFrbMatrices(sk)
    else:
        hk.addSome1DMatrices(sk)
        hk.addFrbMatrices(sk)
    return cc, g, sk, ea


def _same_constants(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(x[0].download(), y[0].download()) and x[1] == y[1]


BITS = 300


# (ring, dim, native, strategy, minimal keys)
@pytest.mark.parametrize("m,native,strategy,minimal", [(31, True, +1, False), (73, True, -1, False), (85, False, +1, False),
                                                       (51, False, -1, False), (51, False, -1, True)])
def test_block_matmul_with_real_keys(hx, m, native, strategy, minimal):
    from helib_amd import bgv_gf_matmul as GM, linalg
    p = 2
    cc, g, sk, ea = _chain(hx, m, p, BITS, minimal)
    n, d, D = ea.size(), ea.getDegree(), ea.sizeOfDimension(0)
    rng = np.random.default_rng(m)
    A = rng.integers(0, p, size=(D, D, d, d))
    A[(np.arange(D) - 1) % D, np.arange(D)] = 0                       # a zero diagonal
    mat = GM.BlockMatMul1D(ea, A, 0)
    ex = GM.BlockMatMul1DExec(ea, mat)
    assert (ex.native, ex.strategy, ex.onDevice) == (native, strategy, True)
    host = GM.BlockMatMul1DExec(ea, mat, device_diagonals=False)
    assert not host.onDevice
    _same_constants(ex.vec, host.vec)
    if not native:
        _same_constants(ex.vec1, host.vec1)
    v = rng.integers(0, p, size=(2, n, d))
    want = GM.mulPlain(ea, v, mat)
    res, before = {}, linalg.MatMul1DExec.fallbacks
    fresh = ea.encrypt_batch(sk, v)                                    # one encryption: the noise bounds follow the data
    for fused in (True, False):
        ct = fresh.clone()
        ex.mul(ct, pk=sk, fused=fused)
        assert ct.isCorrect()
        assert np.array_equal(ea.decrypt_batch(ct, sk), want), fused
        res[fused] = ct
    H.same(res[True], res[False], lambda part: part.download())
    assert linalg.MatMul1DExec.fallbacks == before


def test_block_matmul_special_dimension_with_real_keys(hx):
    from helib_amd import bgv_gf_matmul as GM
    cc, g, sk, ea = _chain(hx, 85, 2, BITS)
    n, d = ea.size(), ea.getDegree()
    rng = np.random.default_rng(11)
    A = rng.integers(0, 2, size=(n, 1, 1, d, d))                       # another block in every slot
    mat = GM.BlockMatMul1D(ea, A, ea.dimension())
    ex = GM.BlockMatMul1DExec(ea, mat)
    assert (ex.D, ex.strategy, ex.onDevice) == (1, -1, True)
    _same_constants(ex.vec, GM.BlockMatMul1DExec(ea, mat, device_diagonals=False).vec)
    v = rng.integers(0, 2, size=(2, n, d))
    ct = ea.encrypt_batch(sk, v)
    ex.mul(ct, pk=sk)
    assert ct.isCorrect()
    want = np.array([[x.astype(object) @ A[s, 0, 0].astype(object) % 2 for s, x in enumerate(row)] for row in v], dtype=np.int64)
    assert np.array_equal(GM.mulPlain(ea, v, mat), want)
    assert np.array_equal(ea.decrypt_batch(ct, sk), want)


@pytest.mark.parametrize("m", [31, 85])
def test_gf_matmul1d_and_linpoly_with_real_keys(hx, m):
    from helib_amd import bgv_gf_matmul as GM, bgv_hypercube
    p = 2
    cc, g, sk, ea = _chain(hx, m, p, BITS)
    n, d, D = ea.size(), ea.getDegree(), ea.sizeOfDimension(0)
    rng = np.random.default_rng(m + 5)
    A = rng.integers(0, p, size=(D, D, d))
    mat = GM.MatMul1D(ea, A, 0)
    ex, host = GM.MatMul1DExec(ea, mat), GM.MatMul1DExec(ea, mat, device_diagonals=False)
    assert ex.onDevice and not host.onDevice and ex.native == (m == 31)
    names = ("multiplier",) + (() if ex.native else ("multiplier1",))
    for name in names:
        _same_constants(getattr(ex, name), getattr(host, name))
    v = rng.integers(0, p, size=(2, n, d))
    ct = ea.encrypt_batch(sk, v)
    ex.mul(ct, pk=sk)
    assert ct.isCorrect()
    assert np.array_equal(ea.decrypt_batch(ct, sk), GM.mulPlain(ea, v, mat))
    Ai = rng.integers(0, p, size=(D, D))                               # integers: the words of the integer class
    exi, exh = GM.MatMul1DExec(ea, Ai, dim=0), bgv_hypercube.MatMul1DExec(ea, Ai, dim=0)
    for name in names:
        _same_constants(getattr(exi, name), getattr(exh, name))
    if m == 85:
        F = ea._frobenius()
        for L in (F, rng.integers(0, p, size=(d, d))):
            ct = ea.encrypt_batch(sk, v)
            GM.applyLinPoly1(ea, ct, GM.buildLinPolyCoeffs(ea, L))
            assert ct.isCorrect()
            assert np.array_equal(ea.decrypt_batch(ct, sk), np.array(v.astype(object) @ L.astype(object) % p, dtype=np.int64))
        Ls = np.concatenate([F[None], rng.integers(0, p, size=(n - 1, d, d))])
        ct = ea.encrypt_batch(sk, v)
        GM.applyLinPolyMany(ea, ct, GM.buildLinPolyCoeffs(ea, Ls))
        want = np.array([[x.astype(object) @ Ls[s].astype(object) % p for s, x in enumerate(row)] for row in v], dtype=np.int64)
        assert np.array_equal(ea.decrypt_batch(ct, sk), want)


# ---- (e) the measured ring: one full-size construct along the size-1 dimension, no keys ----
def test_full_size_special_dimension_constants(hx):
    from helib_amd import bgv_gf_matmul as GM
    m, p = 21845, 2
    ea = _ea(hx, m, p, bits=60)
    n, d = ea.size(), ea.getDegree()
    assert (n, d, ea.dimension()) == (1024, 16, 2)
    rng = np.random.default_rng(21845)
    mat = GM.BlockMatMul1D(ea, rng.integers(0, p, size=(n, 1, 1, d, d)), 2)
    maps, z = GM._Maps(ea), ea.zMStar
    rows = [maps.add(1), maps.add(z.genToPow(-1, -5)), maps.add(z.genToPow(0, -3), ea.maskSlots(0, 3)),
            maps.add(z.genToPow(1, 8 - 2) * z.genToPow(-1, -1) % m, 1 - ea.maskSlots(1, 2))]
    descs = [(0, k, mp) for k, mp in ((0, 0), (15, 0), (3, 1), (7, 1), (1, 2), (9, 2), (4, 3), (12, 3))]
    got, nz = hx.bgvGfGather(mat.handle(ea.enc), descs, np.stack(maps.rows))
    for t, (i, k, mp) in enumerate(descs):
        assert np.array_equal(got[t], GM.hostConstant(ea, mat, i, k, maps.rows[mp])), (k, mp)
    assert nz.all()
    idx = list(ea.cc.ctxtPrimes)
    dev = GM._constants(ea, mat, descs, maps, idx, True)
    host = GM._constants(ea, mat, descs, maps, idx, False)
    _same_constants(dev, host)
