"""Linear maps on Galois-ring slots modulo p^r on the device (hx_bgv_gr_matrix_create, hx_bgv_gf_encode_gathered,
helib_amd.bgv_gr_matmul): the linearized-polynomial and gather kernels with the modulus p^r, the fused kernel
bgv_gf_gather_map_kernel against hx_bgv_gf_encode of the host's constants, the three constant paths against each other,
and homomorphic products with real keys against numpy on slot arrays.  Everything here is an integer: every comparison is
exact."""
import numpy as np
import pytest

from tests import bgv_hypercube_ref as H
from tests import intraslot_ref as IR

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


def _ea(hx, m, p, r, bits=100):
    from helib_amd import bgv_gr, ctxt as hc
    cc = hc.ChainContext(m, p, r, bits=bits, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    return bgv_gr.EncryptedArray(cc, g)


# ---- (a) bgv_gf_linpoly_kernel modulo P on every entry ----
# (803, 3, 2): d = 60, d^2 = 3600 -- 57 column tiles, the last one partial
@pytest.mark.parametrize("m,p,r,D", [(31, 2, 3, 6), (85, 2, 4, 8), (13, 3, 2, 4), (803, 3, 2, 2)])
def test_linpoly_kernel_modulo_p_to_the_r(hx, m, p, r, D):
    from helib_amd import bgv_gr_matmul as RM
    ea = _ea(hx, m, p, r)
    n, d, P = ea.size(), ea.getDegree(), p ** r
    rng = np.random.default_rng(m)
    A = rng.integers(0, P, size=(1, D, D, d, d))
    A[0, 0, 0] = P - 1
    with pytest.raises(hx.HxError, match="r > 1"):                    # the r = 1 entry keeps refusing the table
        hx.BgvGfMatrix(ea.enc.table, A, np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32) % D)
    mat = hx.BgvGfMatrix(ea.enc.table, A, np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32) % D, ring=True)
    C = mat.coeffs().astype(np.int64)
    assert C.shape == A.shape
    assert np.array_equal(C, RM.buildLinPolyCoeffs(ea, A))
    # the defining property on random elements: sum_k C[k] sigma^k(alpha) = alpha A, through frobeniusPlain and _mul
    a = rng.integers(0, P, size=(1, n, d))
    for i, j in ((0, 0), (D - 1, 1), (1, D - 1)):
        want = np.array(a.astype(object) @ A[0, i, j].astype(object) % P, dtype=np.int64)
        got = np.zeros_like(a)
        for k in range(d):
            got = (got + ea._mul(ea.frobeniusPlain(a, k), C[0, i, j, k][None, None, :])) % P
        assert np.array_equal(got, want), (i, j)
    with pytest.raises(hx.HxError, match="not below"):
        bad = A.copy()
        bad[0, 1, 1, 0, 0] = P
        hx.BgvGfMatrix(ea.enc.table, bad, np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32) % D, ring=True)


# ---- (b) lazy reduction at the edge: P = 46337^2 = 2147117569 < 2^31, limit = 4 < d = 10, 3 slots ----
def test_lazy_reduction_at_the_largest_modulus(hx):
    from helib_amd import bgv_gr_matmul as RM
    m, p, r = 31, 46337, 2
    P = p ** r
    ref = IR.tables(m, p, r)
    ea = _ea(hx, m, p, r)
    n, d = ea.size(), ea.getDegree()
    assert (P, d, n, (1 << 64) // (P * P)) == (2147117569, 10, 3, 4)
    A = np.full((n, 1, 1, d, d), P - 1, dtype=np.int64)
    A[1:] = np.random.default_rng(7).integers(0, P, size=(n - 1, 1, 1, d, d))
    mat = hx.BgvGfMatrix(ea.enc.table, A, np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int32), ring=True)
    C = mat.coeffs().astype(np.int64)
    eye = np.eye(d, dtype=np.int64)
    for s in range(n):                                                # in python integers: sum_k C[k] sigma^k(X^j) = L[j]
        for j in range(d):
            acc = [0] * d
            for k in range(d):
                acc = [(x + y) % P for x, y in zip(acc, ref.mul1(C[s, 0, 0, k], ref.sigma1(eye[j], k)))]
            assert acc == [int(x) for x in A[s, 0, 0, j]], (s, j)
    # the gather's Frobenius map: d = 10 > limit = 4 terms
    perm, frob = RM.slotAutomorph(ea, ea.zMStar.genToPow(-1, d - 1))
    assert np.array_equal(perm, np.arange(n)) and np.all(frob == d - 1)
    maps = np.stack([np.arange(n), frob], axis=1).astype(np.int32)[None]
    descs = [(0, k, 0) for k in range(d)]
    got, nz = hx.bgvGfGather(mat, descs, maps)
    want = np.array([[ref.sigma1(C[s, 0, 0, k], d - 1) for s in range(n)] for k in range(d)], dtype=np.int64)
    assert np.array_equal(got, want) and nz.all()
    # both products of the fused kernel: sigma^(d-1) and the per-slot map, against the encode of the expected slots
    idx = list(ea.cc.ctxtPrimes)
    poly, cf, flags = ea.enc.encodeGathered(mat, descs, maps, 1, idx, coeffs=True)
    wpoly, wcf = ea.enc.encode(want, 1, idx, coeffs=True)
    assert np.array_equal(cf, wcf) and np.array_equal(poly.download(), wpoly.download()) and flags.all()
    assert np.array_equal(ea.enc.embed(cf), want)


# ---- (c) bgv_gf_gather_map_kernel against hx_bgv_gf_encode of the host's constants ----
# (m, p, r): d / dp = 3 / 4, 5 / 8 (6 slots), 9 / 16, 8 / 8, 60 / 64, and p = 1 mod m: 1 / 1
FUSED_RINGS = [(13, 3, 2), (31, 2, 3), (73, 2, 2), (85, 2, 4), (803, 3, 2), (13, 53, 2)]


@pytest.mark.parametrize("block", [True, False])
@pytest.mark.parametrize("m,p,r", FUSED_RINGS)
def test_fused_kernel_against_the_encode_of_host_constants(hx, m, p, r, block):
    from helib_amd import bgv_gr_matmul as RM
    ea = _ea(hx, m, p, r)
    n, d, D, z, P = ea.size(), ea.getDegree(), ea.sizeOfDimension(0), ea.zMStar, p ** r
    assert d == {13: 3 if p == 3 else 1, 31: 5, 73: 9, 85: 8, 803: 60}[m]
    rng = np.random.default_rng(m + block)
    mat = (RM.BlockMatMul1D(ea, rng.integers(0, P, size=(D, D, d, d)), 0) if block
           else RM.MatMul1D(ea, rng.integers(0, P, size=(D, D, d)), 0))
    maps = RM._Maps(ea)
    i1 = min(3, D - 1)
    mask = ea.maskSlots(0, i1)
    rows = [maps.add(1), maps.add(z.genToPow(0, -2)), maps.add(1, mask), maps.add(z.genToPow(-1, -3)),
            maps.add(z.genToPow(0, D - i1) * z.genToPow(-1, -1) % m, 1 - mask), maps.add(1, np.zeros(n, dtype=np.int64))]
    dead = rows[-1]
    ks = sorted({0, min(1, d - 1), d - 1}) if block else [0]
    descs = [(i, k, mp) for i in sorted({0, i1, D - 1}) for k in ks for mp in rows]
    table, handle, idx = np.stack(maps.rows), mat.handle(ea.enc), list(ea.cc.ctxtPrimes)
    want = np.stack([RM.hostConstant(ea, mat, i, k, maps.rows[mp]) for i, k, mp in descs])
    wflags = want.reshape(len(descs), -1).any(axis=1)
    assert wflags.any() and not wflags[[t for t, x in enumerate(descs) if x[2] == dead]].any()
    slots, gflags = hx.bgvGfGather(handle, descs, table)              # the gather kernel modulo P
    assert np.array_equal(slots, want) and np.array_equal(gflags, wflags)
    only = ea.enc.encodeGathered(handle, descs, table, 1, idx, flags_only=True)
    assert np.array_equal(only, wflags)
    for lo in range(0, len(descs), 7):                                # 7 descriptors: at 6 slots 42 units, a ragged last wave
        part = descs[lo:lo + 7]
        poly, cf, flags = ea.enc.encodeGathered(handle, part, table, 1, idx, coeffs=True)
        wpoly, wcf = ea.enc.encode(want[lo:lo + 7], 1, idx, coeffs=True)
        assert np.array_equal(flags, wflags[lo:lo + 7]), lo
        assert np.array_equal(cf, wcf), lo
        assert np.array_equal(poly.download(), wpoly.download()), lo
        assert np.array_equal(ea.enc.norm(cf), ea.enc.norm(wcf))
        for t, x in enumerate(part):
            if x[2] == dead:
                assert not np.any(cf[t])                              # flag 0 and a zero polynomial
    # a multiplier other than 1, and no coefficients asked for
    poly, flags = ea.enc.encodeGathered(handle, descs[:3], table, P - 2, idx)
    assert np.array_equal(poly.download(), ea.enc.encode(want[:3], P - 2, idx).download())


def test_fused_entry_refusals(hx):
    ea, other = _ea(hx, 85, 2, 2), _ea(hx, 85, 2, 2)
    from helib_amd import bgv_gr_matmul as RM
    n, d, D = ea.size(), ea.getDegree(), ea.sizeOfDimension(0)
    mat = RM.BlockMatMul1D(ea, np.ones((D, D, d, d), dtype=np.int64), 0)
    handle, idx = mat.handle(ea.enc), list(ea.cc.ctxtPrimes)
    ident = np.stack([np.arange(n), np.zeros(n)], axis=1).astype(np.int32)[None]
    for descs, maps in (([(D, 0, 0)], ident), ([(0, d, 0)], ident), ([(0, 0, 1)], ident), ([(0, 0, 0)], ident + np.int32(n)),
                        ([(0, 0, 0)], np.stack([np.arange(n), np.full(n, d)], axis=1).astype(np.int32)[None])):
        with pytest.raises(hx.HxError, match="out of range"):
            ea.enc.encodeGathered(handle, descs, maps, 1, idx)
        with pytest.raises(hx.HxError, match="out of range"):
            ea.enc.encodeGathered(handle, descs, maps, 1, idx, flags_only=True)
    with pytest.raises(hx.HxError, match="another context"):
        other.enc.encodeGathered(handle, [(0, 0, 0)], ident, 1, list(other.cc.ctxtPrimes))
    with pytest.raises(hx.HxError, match="null argument"):
        hx._chk(hx.lib().hx_bgv_gf_encode_gathered(ea.enc.table.h, None, None, 1, None, 1, 1, None, None, None))


# ---- (d) real keys ----
def _chain(hx, m, p, r, bits, minimal=False, seed=5):
    from helib_amd import bgv_gr, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, r, bits=bits, c=3)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    ea = bgv_gr.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    hk.addSome1DMatrices(sk)
    hk.addFrbMatrices(sk)
    if minimal:
        hk.addMinimal1DMatrices(sk)
        hk.addMinimalFrbMatrices(sk)
    return cc, g, sk, ea


def _same_constants(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(x[0].download(), y[0].download()) and x[1] == y[1]


BITS = 300


def _three_paths(make, names):
    """the exec built through the device path, the host path and the fused path: identical constants; -> the default"""
    from helib_amd import bgv_gr_matmul as RM
    ex, host, fused, default = make(fused=False), make(device_diagonals=False), make(fused=True), make()
    assert (ex.onDevice, ex.fusedConstants) == (True, False)
    assert (host.onDevice, host.fusedConstants) == (False, False)
    assert (fused.onDevice, fused.fusedConstants) == (True, True)
    assert (default.onDevice, default.fusedConstants) == (True, RM.BlockMatMul1DExec.fuseConstants)
    for name in names:
        assert any(c is not None for c in getattr(ex, name))
        for other in (host, fused, default):
            _same_constants(getattr(ex, name), getattr(other, name))
    return default


# (ring, native, strategy, minimal keys as well)
@pytest.mark.parametrize("m,p,r,native,strategy,minimal", [(31, 2, 3, True, +1, False), (73, 2, 2, True, -1, False),
                                                           (85, 2, 2, False, +1, False), (51, 2, 2, False, -1, False),
                                                           (13, 3, 2, True, +1, True)])
def test_block_matmul_with_real_keys(hx, m, p, r, native, strategy, minimal):
    from helib_amd import bgv_gr_matmul as RM, linalg
    cc, g, sk, ea = _chain(hx, m, p, r, BITS, minimal)
    n, d, D, P = ea.size(), ea.getDegree(), ea.sizeOfDimension(0), p ** r
    rng = np.random.default_rng(m)
    A = rng.integers(0, P, size=(D, D, d, d))
    A[(np.arange(D) - 1) % D, np.arange(D)] = 0                       # a zero diagonal
    mat = RM.BlockMatMul1D(ea, A, 0)
    ex = _three_paths(lambda **kw: RM.BlockMatMul1DExec(ea, mat, **kw), ("vec",) + (() if native else ("vec1",)))
    assert (ex.native, ex.strategy) == (native, strategy)
    v = rng.integers(0, P, size=(2, n, d))
    want = RM.mulPlain(ea, v, mat)
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
    from helib_amd import bgv_gr_matmul as RM
    cc, g, sk, ea = _chain(hx, 85, 2, 2, BITS)
    n, d, P = ea.size(), ea.getDegree(), 4
    rng = np.random.default_rng(11)
    A = rng.integers(0, P, size=(n, 1, 1, d, d))                       # another block in every slot
    mat = RM.BlockMatMul1D(ea, A, ea.dimension())
    ex = _three_paths(lambda **kw: RM.BlockMatMul1DExec(ea, mat, **kw), ("vec",))
    assert (ex.D, ex.strategy) == (1, -1)
    v = rng.integers(0, P, size=(2, n, d))
    ct = ea.encrypt_batch(sk, v)
    ex.mul(ct, pk=sk)
    assert ct.isCorrect()
    want = np.array([[x.astype(object) @ A[s, 0, 0].astype(object) % P for s, x in enumerate(row)] for row in v], dtype=np.int64)
    assert np.array_equal(RM.mulPlain(ea, v, mat), want)
    assert np.array_equal(ea.decrypt_batch(ct, sk), want)


@pytest.mark.parametrize("m,p,r", [(31, 2, 3), (85, 2, 2)])
def test_ring_matmul1d_and_linpoly_with_real_keys(hx, m, p, r):
    from helib_amd import bgv_gr_matmul as RM
    cc, g, sk, ea = _chain(hx, m, p, r, BITS)
    n, d, D, P = ea.size(), ea.getDegree(), ea.sizeOfDimension(0), p ** r
    rng = np.random.default_rng(m + 5)
    A = rng.integers(0, P, size=(D, D, d))
    mat = RM.MatMul1D(ea, A, 0)
    native = m == 31
    names = ("multiplier",) + (() if native else ("multiplier1",))
    ex = _three_paths(lambda **kw: RM.MatMul1DExec(ea, mat, **kw), names)
    assert ex.native == native
    v = rng.integers(0, P, size=(2, n, d))
    ct = ea.encrypt_batch(sk, v)
    ex.mul(ct, pk=sk)
    assert ct.isCorrect()
    assert np.array_equal(ea.decrypt_batch(ct, sk), RM.mulPlain(ea, v, mat))
    Ai = rng.integers(0, P, size=(D, D))                               # integers: constants in the slots
    exi = _three_paths(lambda **kw: RM.MatMul1DExec(ea, Ai, dim=0, **kw), names)
    ct = ea.encrypt_batch(sk, v)
    exi.mul(ct, pk=sk)
    assert ct.isCorrect()
    assert np.array_equal(ea.decrypt_batch(ct, sk), RM.mulPlain(ea, v, RM.MatMul1D(ea, Ai, 0)))
    if m == 85:
        F = ea._frobenius()
        for L in (F, rng.integers(0, P, size=(d, d))):
            ct = ea.encrypt_batch(sk, v)
            RM.applyLinPoly1(ea, ct, RM.buildLinPolyCoeffs(ea, L))
            assert ct.isCorrect()
            assert np.array_equal(ea.decrypt_batch(ct, sk), np.array(v.astype(object) @ L.astype(object) % P, dtype=np.int64))
        Ls = np.concatenate([F[None], rng.integers(0, P, size=(n - 1, d, d))])
        ct = ea.encrypt_batch(sk, v)
        RM.applyLinPolyMany(ea, ct, RM.buildLinPolyCoeffs(ea, Ls))
        want = np.array([[x.astype(object) @ Ls[s].astype(object) % P for s, x in enumerate(row)] for row in v], dtype=np.int64)
        assert np.array_equal(ea.decrypt_batch(ct, sk), want)


# ---- (e) the measured ring: one full-size construct along the size-1 dimension, no keys ----
def test_full_size_special_dimension_constants(hx):
    from helib_amd import bgv_gr_matmul as RM
    m, p, r = 21845, 2, 2
    ea = _ea(hx, m, p, r, bits=60)
    n, d = ea.size(), ea.getDegree()
    assert (n, d, ea.dimension()) == (1024, 16, 2)
    rng = np.random.default_rng(21845)
    mat = RM.BlockMatMul1D(ea, rng.integers(0, 4, size=(n, 1, 1, d, d)), 2)
    maps, z = RM._Maps(ea), ea.zMStar
    maps.add(1), maps.add(z.genToPow(-1, -5)), maps.add(z.genToPow(0, -3), ea.maskSlots(0, 3))
    maps.add(z.genToPow(1, 8 - 2) * z.genToPow(-1, -1) % m, 1 - ea.maskSlots(1, 2))
    descs = [(0, k, mp) for k, mp in ((0, 0), (15, 0), (3, 1), (7, 1), (1, 2), (9, 2), (4, 3), (12, 3))]
    idx = list(ea.cc.ctxtPrimes)
    dev = RM._constants(ea, mat, descs, maps, idx, True)
    host = RM._constants(ea, mat, descs, maps, idx, False)
    fused = RM._constants(ea, mat, descs, maps, idx, True, fused=True)
    assert all(c is not None for c in dev)
    _same_constants(dev, host)
    _same_constants(dev, fused)
