"""Linear maps on GF(p^d) slots on the host side (no GPU): helib_amd.bgv_gf_matmul's plain-side mathematics and the C++
table builder (helib_amd/csrc/bgv_gf_linalg.h, printed by tests/cpp/bgv_gf_linalg_dump.cpp) against the restatement
tests/bgv_gf_matmul_ref.py, the classes over the oracle backend with an injected CPU encoder, the declared and exported
symbols, and the refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bgv_gf_matmul_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "bgv_gf_linalg_dump.cpp")
LINPOLY_RINGS = [(31, 2), (13, 3), (85, 2), (73, 2)]      # d = 5, 3, 8, 9


def _plain_ea(m, p):
    """bgv_gf.EncryptedArray over an encoder that only knows the geometry: the plain side needs no more"""
    from helib_amd import bgv_gf, ctxt as hc
    ref = MR.tables(m, p)

    class Enc:
        G = [int(x) for x in ref.G]

        def dims(self):
            return ref.z.gens, ref.z.signedOrds()
    return bgv_gf.EncryptedArray(hc.ChainContext(m, p, 1, bits=100, c=2), None, encoder=Enc()), ref


@pytest.mark.parametrize("m,p", LINPOLY_RINGS)
def test_linpoly_matrix_and_defining_property(m, p):
    from helib_amd import bgv_gf_matmul as GM
    ea, ref = _plain_ea(m, p)
    d = ea.getDegree()
    M, K = GM.linPolyMatrix(ea)
    X = np.array([0, 1], dtype=np.int64)
    for i in range(d):                                            # M[i][j] = (X^j)^(p^i) mod G, literally
        for j in range(d):
            w = MR.R.ppowmod(X, j * p ** i, ref.G, p) if j else np.array([1])
            assert np.array_equal(M[i, j], MR._pad(w, d)), (i, j)
    # K M = I over the field
    for j in range(d):
        for jj in range(d):
            s = np.zeros(d, dtype=np.int64)
            for k in range(d):
                s = (s + MR._fmul(K[j, k], M[k, jj], ref)) % p
            assert np.array_equal(s, np.eye(d, dtype=np.int64)[0] * (j == jj)), (j, jj)
    rng = np.random.default_rng(m)
    L = rng.integers(0, p, size=(3, d, d))
    L[2] = p - 1
    C = GM.buildLinPolyCoeffs(ea, L)
    assert np.array_equal(C[0], MR.linpoly_solve(ref, L[0]))
    for t in range(3):
        assert MR.linpoly_holds(ref, C[t], L[t])
    # the defining property on slots: sum_k C[k] alpha^(p^k) = sum_j alpha_j L[j]
    a = rng.integers(0, p, size=(2, ea.size(), d))
    want = np.array([[sum(int(x[j]) * L[0][j].astype(object) for j in range(d)) % p for x in row] for row in a], dtype=np.int64)
    assert np.array_equal(GM.evalLinPoly(ea, C[0], a), want)
    # the flat table: what the device multiplies by
    E = rng.integers(0, p, size=(5, d, d))
    assert np.array_equal(GM.linPolyFlat(ea, E), GM.buildLinPolyCoeffs(ea, E))


def _powers(ea):
    z = ea.zMStar
    ks = {z.genToPow(-1, j) for j in range(-1, ea.getDegree())}
    for i in range(ea.dimension()):
        D = ea.sizeOfDimension(i)
        ks |= {z.genToPow(i, a) for a in list(range(-D, D + 1))}
    return sorted(ks)


@pytest.mark.parametrize("m,p", [(85, 2), (51, 2), (255, 2)])
def test_slot_automorph_against_the_literal_substitution(m, p):
    from helib_amd import bgv_gf_matmul as GM
    ea, ref = _plain_ea(m, p)
    n, d = ea.size(), ea.getDegree()
    rng = np.random.default_rng(m)
    a = rng.integers(0, p, size=(1, n, d))
    consts = rng.integers(0, p, size=(1, n))
    for k in _powers(ea):
        perm, frob = GM.slotAutomorph(ea, k)
        assert np.array_equal(perm, ea.slotPermutation(k)), k
        assert np.array_equal(GM.automorphPlain(ea, a, k), MR.automorph(ref, a, k)), k
        assert np.array_equal(GM.automorphPlain(ea, consts, k)[:, :, 0], consts[:, perm]), k     # Frobenius fixes constants
    for j in range(d):
        perm, frob = GM.slotAutomorph(ea, pow(p, j, m))
        assert np.array_equal(perm, np.arange(n)) and np.all(frob == j)
        assert np.array_equal(GM.automorphPlain(ea, a, pow(p, j, m)), ea.frobeniusPlain(a, j))


@pytest.mark.parametrize("m,p,dim", [(85, 2, 0), (51, 2, 0), (13, 3, 0)])
def test_mul_plain_against_the_loops(m, p, dim):
    from helib_amd import bgv_gf_matmul as GM
    ea, ref = _plain_ea(m, p)
    n, d, D = ea.size(), ea.getDegree(), ea.sizeOfDimension(dim)
    rng = np.random.default_rng(m + 1)
    v = rng.integers(0, p, size=(2, n, d))
    A = rng.integers(0, p, size=(D, D, d, d))
    assert np.array_equal(GM.mulPlain(ea, v, GM.BlockMatMul1D(ea, A, dim)), MR.mul_block(ref, v, A, dim))
    Am = rng.integers(0, p, size=(n // D, D, D, d, d))
    assert np.array_equal(GM.mulPlain(ea, v, GM.BlockMatMul1D(ea, Am, dim)), MR.mul_block(ref, v, Am, dim))
    Ag = rng.integers(0, p, size=(D, D, d))
    assert np.array_equal(GM.mulPlain(ea, v, GM.MatMul1D(ea, Ag, dim)), MR.mul_gf(ref, v, Ag, dim))
    As = rng.integers(0, p, size=(n, 1, 1, d, d))
    assert np.array_equal(GM.mulPlain(ea, v, GM.BlockMatMul1D(ea, As, ea.dimension())), MR.mul_block(ref, v, As, ea.dimension()))


# ---- the C++ table builder ----
def _run(exe, m, p):
    out = subprocess.run([exe, str(m), str(p)], capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    assert out[0].split()[0] == "ok", out[0]
    d = int(out[0].split()[3])
    rows = [np.array(line.split(), dtype=np.int64) for line in out[1:]]
    return d, rows[0], rows[1].reshape(d, d, d), rows[2].reshape(d, d, d), rows[3].reshape(d * d, d * d)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gfl") / "bgv_gf_linalg_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", SRC, "-o", exe])
    return lambda m, p: _run(exe, m, p)


@pytest.mark.parametrize("m,p", LINPOLY_RINGS + [(13, 2147483647), (64, 193)])
def test_cpp_tables_against_the_python(dump, m, p):
    from helib_amd import bgv_gf_matmul as GM
    ea, ref = _plain_ea(m, p)
    d, G, frob, K, T = dump(m, p)
    assert d == ea.getDegree() and [int(x) for x in G] == ea.getG()
    M, Kp = GM.linPolyMatrix(ea)
    assert np.array_equal(frob, M) and np.array_equal(K, Kp) and np.array_equal(T, GM.linPolyTable(ea))


def test_dump_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "bgv_gf_linalg_dump_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("the sanitizer runtimes do not link here: " + build.stderr.strip().splitlines()[-1][:200])
    for m, p in ((85, 2), (13, 2147483647), (64, 193)):
        run = subprocess.run([exe, str(m), str(p)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
        assert run.stdout.startswith("ok %d %d " % (m, p))


# ---- the classes over the oracle backend with a CPU encoder ----
def _setup(m, p, seed=3, bits=300, minimal=False):
    from oracle import oracle as O
    from oracle.backend import OracleBackend
    from helib_amd import bgv_gf, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, 1, bits=bits, c=2)
    o = O.Ctx(m)
    for q in cc.primes:
        o.add_prime(q)

    class Backend(OracleBackend):
        def fromCoeffsBatch(self, idx, polys):
            assert len(polys) == 1
            d = self.fromCoeffs(idx, polys[0])
            d.batch = 1
            return d
    be = Backend(o, cc)
    ref = MR.tables(m, p)

    class Enc:
        G = [int(x) for x in ref.G]

        def dims(self):
            return ref.z.gens, ref.z.signedOrds()

        def encode(self, v, mul, idx, coeffs=False):
            cf = ref.encode(v, mul)
            d = None
            if idx:
                assert cf.shape[0] == 1, "the CPU backend takes one vector at a time"
                d = be.fromCoeffs(idx, [int(x) for x in cf[0]])
                d.batch = 1
                d.slots = np.array(v[0], dtype=np.int64)          # what the constant holds, for the tests below
            return (d, cf) if coeffs else d

        def embed(self, coeffs):
            return ref.decode(coeffs)

        def decode(self, acc, factor_inv):
            return ref.decode([[int(x) % p * factor_inv % p for x in be.toPoly(acc)]])

        def norm(self, coeffs):
            return np.array([be.embeddingLargestCoeff(row) for row in np.atleast_2d(coeffs)])
    sk = hk.SecKey(cc, be, seed=seed)
    sk.GenSecKey()
    ea = bgv_gf.EncryptedArray(cc, None, encoder=Enc())
    sk.zMStar = ea.zMStar
    if minimal:
        hk.addMinimal1DMatrices(sk)
        hk.addMinimalFrbMatrices(sk)
    else:
        hk.add1DMatrices(sk)
        hk.addFrbMatrices(sk)
    return cc, sk, ea, ref


def _literal_constant(ea, ref, C, i, k, mask, autos):
    """the reference's poly-space construction on slots: coefficient k of the diagonal, the mask, then the plaintext
    automorphisms one after the other, each the literal substitution"""
    D, blk, col = C.shape[1], *_break(ea, C)
    v = np.array([C[blk[s] if C.shape[0] > 1 else 0, (col[s] - i) % D, col[s], k] for s in range(ea.size())], dtype=np.int64)
    if mask is not None:
        v = v * np.asarray(mask)[:, None]
    v = v[None]
    for a in autos:
        v = MR.automorph(ref, v, a)
    return v[0]


def _break(ea, C):
    dim = C.dim
    pairs = [MR.break_index(ea.zMStar.ords, s, dim) for s in range(ea.size())]
    return [b for b, _ in pairs], [c for _, c in pairs]


class _Coeffs(np.ndarray):
    dim = 0


# (m, p, native, strategy): the four construct branches
@pytest.mark.parametrize("m,p,native,strategy", [(31, 2, True, +1), (73, 2, True, -1), (85, 2, False, +1), (51, 2, False, -1)])
def test_block_exec_over_the_oracle_backend(m, p, native, strategy):
    from helib_amd import bgv_gf_matmul as GM
    cc, sk, ea, ref = _setup(m, p)
    n, d, D, dim = ea.size(), ea.getDegree(), ea.sizeOfDimension(0), 0
    z = ea.zMStar
    rng = np.random.default_rng(m)
    A = rng.integers(0, p, size=(D, D, d, d))
    A[(np.arange(D) - 1) % D, np.arange(D)] = 0                       # diagonal 1 is zero: no multipliers
    mat = GM.BlockMatMul1D(ea, A, dim)
    ex = GM.BlockMatMul1DExec(ea, mat)
    assert (ex.native, ex.strategy, ex.onDevice) == (native, strategy, False)
    C = np.array([[MR.linpoly_solve(ref, A[i, j]) for j in range(D)] for i in range(D)])[None].view(_Coeffs)
    C.dim = dim
    assert np.array_equal(np.asarray(C), GM.buildLinPolyCoeffs(ea, A)[None])
    for i in (0, 1, 2, D - 1):
        for j in (0, 1, d - 1):
            at = i * d + j if strategy == +1 else i + j * D
            mask = None if native else ea.maskSlots(dim, i)
            if strategy == +1:
                a0, a1 = [z.genToPow(-1, -j)], [z.genToPow(-1, -j), z.genToPow(dim, D)]
            else:
                a0, a1 = [z.genToPow(dim, -i)], [z.genToPow(dim, D - i)]
            for lst, msk, autos in ((ex.vec, mask, a0),) + (() if native else ((ex.vec1, 1 - mask, a1),)):
                want = _literal_constant(ea, ref, C, i, j, msk, autos)
                if not np.any(want):
                    assert lst[at] is None, (i, j)
                else:
                    assert np.array_equal(lst[at][0].slots, want), (i, j)
    assert all(ex.vec[(1 * d + j) if strategy == +1 else (1 + j * D)] is None for j in range(d))
    v = rng.integers(0, p, size=(1, n, d))
    want = MR.mul_block(ref, v, A, dim)
    assert np.array_equal(GM.mulPlain(ea, v, mat), want)
    ct = ea.encrypt(sk, v)
    ex.mul(ct, pk=sk)
    assert np.array_equal(ea.decrypt_batch(ct, sk), want)


def test_block_exec_special_dimension_and_minimal_keys():
    from helib_amd import bgv_gf_matmul as GM
    cc, sk, ea, ref = _setup(51, 2, minimal=True)
    n, d = ea.size(), ea.getDegree()
    rng = np.random.default_rng(9)
    v = rng.integers(0, 2, size=(1, n, d))
    A = rng.integers(0, 2, size=(n, 1, 1, d, d))
    mat = GM.BlockMatMul1D(ea, A, ea.dimension())
    ex = GM.BlockMatMul1DExec(ea, mat)
    assert (ex.D, ex.native, ex.strategy) == (1, True, -1)
    ct = ea.encrypt(sk, v)
    ex.mul(ct, pk=sk)                                                  # iterative0 along the Frobenius
    assert np.array_equal(ea.decrypt_batch(ct, sk), MR.mul_block(ref, v, A, ea.dimension()))
    B = rng.integers(0, 2, size=(n // 4, 4, 4, d, d))                  # multipleTransforms, non-native, minimal keys
    matB = GM.BlockMatMul1D(ea, B, 0)
    ct = ea.encrypt(sk, v)
    GM.BlockMatMul1DExec(ea, matB).mul(ct, pk=sk)
    assert np.array_equal(ea.decrypt_batch(ct, sk), MR.mul_block(ref, v, B, 0))


@pytest.mark.parametrize("m,p", [(31, 2), (85, 2)])
def test_gf_matmul1d_and_linpoly_over_the_oracle_backend(m, p):
    from helib_amd import bgv_gf_matmul as GM, bgv_hypercube
    cc, sk, ea, ref = _setup(m, p)
    n, d, D = ea.size(), ea.getDegree(), ea.sizeOfDimension(0)
    rng = np.random.default_rng(m + 2)
    v = rng.integers(0, p, size=(1, n, d))
    A = rng.integers(0, p, size=(D, D, d))
    mat = GM.MatMul1D(ea, A, 0)
    ex = GM.MatMul1DExec(ea, mat)
    assert ex.native == ea.nativeDimension(0)
    ct = ea.encrypt(sk, v)
    ex.mul(ct, pk=sk)
    assert np.array_equal(ea.decrypt_batch(ct, sk), MR.mul_gf(ref, v, A, 0))
    # a callable gives the same constants
    ex2 = GM.MatMul1DExec(ea, lambda i, j: A[i, j], dim=0)
    for a, b in zip(ex.multiplier, ex2.multiplier):
        assert (a is None) == (b is None) and (a is None or (np.array_equal(a[0].slots, b[0].slots) and a[1] == b[1]))
    # an integer matrix gives the constants of the integer class
    Ai = rng.integers(0, p, size=(D, D))
    exi, exh = GM.MatMul1DExec(ea, Ai, dim=0), bgv_hypercube.MatMul1DExec(ea, Ai, dim=0)
    for name in ("multiplier",) + (() if exi.native else ("multiplier1",)):
        for a, b in zip(getattr(exi, name), getattr(exh, name)):
            assert (a is None) == (b is None)
            if a is not None:
                assert np.array_equal(a[0].slots[:, 0], np.asarray(b[0].slots).reshape(n, -1)[:, 0]) and a[1] == b[1]
                assert not np.any(a[0].slots[:, 1:])
    # linearized polynomials: the Frobenius itself and a random map
    F = ea._frobenius()                                                # row l = X^(l p): the image of X^l
    for L in (F, rng.integers(0, p, size=(d, d))):
        C = GM.buildLinPolyCoeffs(ea, L)
        ct = ea.encrypt(sk, v)
        GM.applyLinPoly1(ea, ct, C)
        want = np.array([[sum(int(x[j]) * L[j].astype(object) for j in range(d)) % p for x in row] for row in v], dtype=np.int64)
        assert np.array_equal(ea.decrypt_batch(ct, sk), want)
    one = np.zeros((d, d), dtype=np.int64)
    one[1, 0] = 1                                                      # the Frobenius is the linearized polynomial alpha^p
    assert np.array_equal(GM.buildLinPolyCoeffs(ea, F), one)
    Ls = rng.integers(0, p, size=(n, d, d))
    ct = ea.encrypt(sk, v)
    GM.applyLinPolyMany(ea, ct, GM.buildLinPolyCoeffs(ea, Ls))
    want = np.array([[(x.astype(object) @ Ls[s].astype(object)) % p for s, x in enumerate(row)] for row in v], dtype=np.int64)
    assert np.array_equal(ea.decrypt_batch(ct, sk), want)


# ---- the C ABI: declared, listed, exported ----
NAMES = ["hx_bgv_gf_linalg_tables", "hx_bgv_gf_matrix_create", "hx_bgv_gf_matrix_destroy", "hx_bgv_gf_matrix_coeffs",
         "hx_bgv_gf_gather"]


def test_symbols_are_declared_listed_and_exported():
    from helib_amd import build, capi
    header = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SYMBOLS, name
    so = build.build()
    dyn = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r" T %s$" % name, dyn, re.M), name
    text = subprocess.run(["nm", "-C", so], capture_output=True, text=True, check=True).stdout
    for kernel in ("bgv_gf_linpoly_kernel", "bgv_gf_gather_kernel"):
        assert kernel in text, kernel
    # the host tables through the C ABI (no device is touched) equal the Python's
    from helib_amd import bgv_gf_matmul as GM
    ea, ref = _plain_ea(85, 2)
    frob, K, T = capi.bgvGfLinalgTables(2, 8, ea.getG())
    M, Kp = GM.linPolyMatrix(ea)
    assert np.array_equal(frob, M) and np.array_equal(K, Kp) and np.array_equal(T, GM.linPolyTable(ea))


# ---- refusals ----
def test_refusals():
    from helib_amd import bgv_gf_matmul as GM, bgv_matmul, capi, ckks, ctxt as hc, bgv_gf
    ea, ref = _plain_ea(85, 2)
    n, d, D = ea.size(), ea.getDegree(), ea.sizeOfDimension(0)
    z = np.zeros((D, D, d, d), dtype=np.int64)
    with pytest.raises(ckks.LogicError, match="BlockMatMulFull"):
        GM.BlockMatMulFull(ea, z)
    with pytest.raises(ckks.LogicError, match="BlockMatMulFull"):
        GM.BlockMatMulFullExec(ea, z)
    with pytest.raises(ckks.LogicError, match="MatMulFull with GF entries"):
        GM.MatMulFull(ea, np.zeros((n, n, d), dtype=np.int64))
    with pytest.raises(ckks.LogicError, match="multipleTransforms"):
        GM.MatMul1D(ea, np.zeros((n // D, D, D, d), dtype=np.int64), 0)
    with pytest.raises(ckks.LogicError, match="dimension"):
        GM.BlockMatMul1D(ea, z, ea.dimension() + 1)
    with pytest.raises(ckks.LogicError, match="one block per slot"):
        GM.BlockMatMul1D(ea, np.zeros((1, 1, d, d), dtype=np.int64), ea.dimension())
    with pytest.raises(ckks.LogicError, match="shape"):
        GM.BlockMatMul1D(ea, np.zeros((D, D, d, d + 1), dtype=np.int64), 0)
    with pytest.raises(ckks.LogicError, match="shape"):
        GM.MatMul1D(ea, np.zeros((D, D + 1, d), dtype=np.int64), 0)
    with pytest.raises(capi.HxError, match="r > 1"):                   # r > 1 stays refused where the slots are made
        bgv_gf.EncryptedArray(hc.ChainContext(85, 2, 2, bits=100, c=2), None, encoder=ea.enc)
    with pytest.raises(ckks.LogicError):                               # the integer classes keep refusing GF shapes
        bgv_matmul.MatMul1D(ea, np.zeros((D, D, d), dtype=np.int64), 0)
    with pytest.raises(ckks.LogicError, match="bgv_gf.EncryptedArray"):
        GM.buildLinPolyCoeffs(object(), z)
