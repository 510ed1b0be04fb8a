"""Linear maps on Galois-ring slots modulo p^r on the host side (no GPU): the C++ table builder modulo P
(helib_amd/csrc/bgv_gf_linalg.h, printed by tests/cpp/bgv_gr_linalg_dump.cpp) against helib_amd.intraslot's tables and the
restatement tests/intraslot_ref.py; helib_amd.bgv_gr_matmul's classes over the oracle backend with the table encoder of
tests/bgv_gr_tables.py against the literal substitution; the thread map of the fused kernel
(helib_amd/csrc/gather_map.h) on the CPU; the refusals and the symbols.  Every comparison is an exact integer."""
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import bgv_gf_matmul_ref as MR
from tests import bgv_gr_tables as T
from tests import bgv_pr_ref as PR
from tests import intraslot_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [(13, 3, 2), (31, 2, 3), (85, 2, 2)]


def _compile(name):
    exe = os.path.join(tempfile.mkdtemp(prefix=name + "_"), name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe])
    return exe


@functools.lru_cache(maxsize=None)
def _dump_exe():
    return _compile("bgv_gr_linalg_dump")


@functools.lru_cache(maxsize=None)
def _dump(m, p, r):
    out = subprocess.run([_dump_exe(), str(m), str(p), str(r)], capture_output=True, text=True, timeout=120, check=True).stdout
    lines = out.splitlines()
    assert lines[0].split()[0] == "ok", lines[0]
    head = dict(zip(("m", "p", "r", "P", "d", "limit"), map(int, lines[0].split()[1:])))
    d = head["d"]
    rows = [np.array(line.split(), dtype=np.int64) for line in lines[1:]]
    return head, rows[0], rows[1].reshape(d, d, d), rows[2].reshape(d, d, d), rows[3].reshape(d * d, d * d), out


def _plain_ea(m, p, r):
    """bgv_gr.EncryptedArray over an encoder that only knows the geometry: the plain side needs no more"""
    from helib_amd import bgv_gr, ctxt as hc
    ref = IR.tables(m, p, r)

    class Enc:
        G = [int(x) for x in ref.G]

        def dims(self):
            return ref.z.gens, ref.z.signedOrds()
    return bgv_gr.EncryptedArray(hc.ChainContext(m, p, r, bits=100, c=2), None, encoder=Enc()), ref


# ---- the tables modulo P ----
@pytest.mark.parametrize("m,p,r", RINGS)
def test_cpp_tables_modulo_p_to_the_r(m, p, r):
    from helib_amd import bgv_gr_matmul as RM, capi, intraslot
    ea, ref = _plain_ea(m, p, r)
    head, G, frob, K, Tf, _ = _dump(m, p, r)
    P, d = p ** r, ea.getDegree()
    assert (head["P"], head["d"], head["limit"]) == (P, d, min((1 << 64) // (P * P), 0xffffffff))
    assert [int(x) for x in G] == ea.getG() == [int(x) for x in ref.G]
    t = intraslot._tables(ea)
    assert np.array_equal(frob, t.frob) and np.array_equal(K, t.K) and np.array_equal(Tf, RM.linPolyTable(ea))
    M, Kp = RM.linPolyMatrix(ea)
    assert np.array_equal(M, frob) and np.array_equal(Kp, K)
    # against the restatement: frob[e][l] = sigma^e(X^l) by composition, and M K = the identity over the ring
    eye = np.eye(d, dtype=np.int64)
    for e in range(d):
        for l in range(d):
            assert [int(x) for x in frob[e, l]] == ref.sigma1(eye[l], e), (e, l)
    for i in range(d):
        for k in range(d):
            s = [0] * d
            for j in range(d):                                        # M[i][j] = frob[i][j]
                s = [(a + b) % P for a, b in zip(s, ref.mul1(frob[i, j], K[j, k]))]
            assert s == [int(i == k)] + [0] * (d - 1), (i, k)
    # the flat table is X^b K[j][k], literally
    for j in range(d):
        for b in range(d):
            for k in range(d):
                assert [int(x) for x in Tf[j * d + b, k * d:(k + 1) * d]] == ref.mul1(eye[b], K[j, k])
    # reduced mod p they are the r = 1 tables, which are hx_bgv_gf_linalg_tables' byte for byte
    h1, G1, frob1, K1, T1, text1 = _dump(m, p, 1)
    assert np.array_equal(frob % p, frob1) and np.array_equal(K % p, K1) and np.array_equal(Tf % p, T1)
    assert np.array_equal(G % p, G1)
    old = _dump(m, p, 0)
    assert old[5].splitlines()[1:] == text1.splitlines()[1:]           # build_gf_linalg and build_gr_linalg at r = 1
    f0, k0, t0 = capi.bgvGfLinalgTables(p, d, G1)
    f1, k1, t1 = capi.bgvGrLinalgTables(p, 1, d, G1)
    assert f0.tobytes() == f1.tobytes() == frob1.astype(np.uint32).tobytes()
    assert k0.tobytes() == k1.tobytes() == K1.astype(np.uint32).tobytes()
    assert t0.tobytes() == t1.tobytes() == T1.astype(np.uint32).tobytes()
    fr, kr, tr = capi.bgvGrLinalgTables(p, r, d, G)
    assert np.array_equal(fr, frob) and np.array_equal(kr, K) and np.array_equal(tr, Tf)


def test_cpp_tables_at_the_lazy_reduction_edge():
    """P = 46337^2 < 2^31: limit = 4 < d = 10; the tables still invert the Moore matrix"""
    m, p, r = 31, 46337, 2
    head, G, frob, K, Tf, _ = _dump(m, p, r)
    P, d = head["P"], head["d"]
    assert (P, d, head["limit"], (1 << 64) // (P * P)) == (2147117569, 10, 4, 4)
    ea, ref = _plain_ea(m, p, r)
    from helib_amd import intraslot
    t = intraslot._tables(ea)
    assert np.array_equal(frob, t.frob) and np.array_equal(K, t.K)
    for i in (0, 1, d - 1):
        for k in (0, d - 1):
            s = [0] * d
            for j in range(d):
                s = [(a + b) % P for a, b in zip(s, ref.mul1(frob[i, j], K[j, k]))]
            assert s == [int(i == k)] + [0] * (d - 1), (i, k)


def test_dump_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "bgv_gr_linalg_dump_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "bgv_gr_linalg_dump.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("the sanitizer runtimes do not link here: " + build.stderr.strip().splitlines()[-1][:200])
    for m, p, r in ((85, 2, 2), (31, 46337, 2), (13, 3, 2)):
        run = subprocess.run([exe, str(m), str(p), str(r)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
        assert run.stdout.startswith("ok %d %d %d " % (m, p, r))


# ---- the thread map of bgv_gf_gather_map_kernel ----
def test_gather_map_owns_every_word_once():
    out = subprocess.run([_compile("gather_map_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-500:]
    assert int(out.stdout.split()[1]) >= 64 * 4


# ---- the plain side ----
def _automorph(ref, a, k):
    """slots [B, n, d] -> the slots of H(X^k) mod (Phi_m, P): encode literally, substitute on the polynomial, decode"""
    m, P = ref.m, ref.P
    out = []
    for h in ref.encode(a):
        g = [0] * m
        for i, c in enumerate(h):
            g[i * k % m] = (g[i * k % m] + int(c)) % P
        rem = PR._divmod(g, ref.base.phi, P)[1]
        out.append((list(rem) + [0] * ref.phim)[:ref.phim])
    return ref.decode(out)


@pytest.mark.parametrize("m,p,r", [(85, 2, 2), (13, 3, 2)])
def test_slot_automorph_and_linpoly_over_the_ring(m, p, r):
    from helib_amd import bgv_gr_matmul as RM, intraslot
    ea, ref = _plain_ea(m, p, r)
    n, d, P, z = ea.size(), ea.getDegree(), p ** r, ea.zMStar
    rng = np.random.default_rng(m + r)
    a = rng.integers(0, P, size=(1, n, d))
    ks = {z.genToPow(-1, 1), z.genToPow(-1, d - 1), z.genToPow(0, 1), z.genToPow(0, -2) * z.genToPow(-1, 2) % m}
    for k in sorted(ks):
        assert np.array_equal(RM.automorphPlain(ea, a, k), _automorph(ref, a, k)), k
    L = rng.integers(0, P, size=(2, d, d))
    L[1] = P - 1
    C = RM.buildLinPolyCoeffs(ea, L)
    assert np.array_equal(C, intraslot.buildLinPolyCoeffs(ea, L)) and np.array_equal(C, RM.linPolyFlat(ea, L))
    for t in range(2):
        want = np.array(a.astype(object) @ L[t].astype(object) % P, dtype=np.int64)
        assert np.array_equal(RM.evalLinPoly(ea, C[t], a), want)
        got = np.zeros((n, d), dtype=object)                          # the same sum in the restatement's arithmetic
        for s in range(n):
            for k in range(d):
                got[s] = (got[s] + np.array(ref.mul1(C[t, k], ref.sigma1(a[0, s], k)), dtype=object)) % P
        assert np.array_equal(np.array(got, dtype=np.int64), want[0])


# ---- the classes over the oracle backend with the table encoder ----
def _held(S, const):
    """the slots a constant (DoubleCRT, size) holds"""
    return S.enc.slots([[int(x) for x in S.be.toPoly(const[0])]])[0]


def _literal(S, C, blk, col, i, k, mask, autos):
    D = C.shape[1]
    v = np.array([C[blk[s] if C.shape[0] > 1 else 0, (col[s] - i) % D, col[s], k] for s in range(S.ea.size())], dtype=np.int64)
    if mask is not None:
        v = v * np.asarray(mask)[:, None]
    v = v[None]
    for a in autos:
        v = _automorph(S.ref, v, a)
    return v[0]


def _break(ea, dim):
    pairs = [MR.break_index(ea.zMStar.ords, s, dim) for s in range(ea.size())]
    return [b for b, _ in pairs], [c for _, c in pairs]


def _mul_block(ea, v, A, dim, P):
    """mul(PlaintextArray, BlockMatMul1D) as plain loops over breakIndexByDim, modulo P"""
    n, d = ea.size(), ea.getDegree()
    D = 1 if dim == ea.dimension() else ea.sizeOfDimension(dim)
    A = np.asarray(A)
    where = {MR.break_index(ea.zMStar.ords, s, dim): s for s in range(n)}
    out = np.zeros(v.shape, dtype=np.int64)
    for b in range(v.shape[0]):
        for k in range(n // D):
            for j in range(D):
                acc = np.zeros(d, dtype=object)
                for i in range(D):
                    blkm = A[k][i][j] if A.ndim == 5 else A[i][j]
                    acc = (acc + v[b, where[k, i]].astype(object) @ blkm.astype(object)) % P
                out[b, where[k, j]] = [int(x) for x in acc]
    return out


# (m, p, r, native, strategy)
@pytest.mark.parametrize("m,p,r,native,strategy", [(31, 2, 3, True, +1), (51, 2, 2, False, -1), (13, 3, 2, True, +1)])
def test_block_exec_over_the_oracle_backend(m, p, r, native, strategy):
    from helib_amd import bgv_gr_matmul as RM
    S = T.Setup(m, p, r)
    ea, P, z = S.ea, p ** r, S.ea.zMStar
    n, d, D, dim = ea.size(), ea.getDegree(), ea.sizeOfDimension(0), 0
    rng = np.random.default_rng(m)
    A = rng.integers(0, P, size=(D, D, d, d))
    A[(np.arange(D) - 1) % D, np.arange(D)] = 0                       # diagonal 1 is zero: no multipliers
    mat = RM.BlockMatMul1D(ea, A, dim)
    ex = RM.BlockMatMul1DExec(ea, mat)
    assert (ex.native, ex.strategy, ex.onDevice, ex.fusedConstants) == (native, strategy, False, False)
    C = RM.buildLinPolyCoeffs(ea, A)[None]
    blk, col = _break(ea, dim)
    for i in (0, 2, D - 1):
        for j in (0, d - 1):
            at = i * d + j if strategy == +1 else i + j * D
            mask = None if native else ea.maskSlots(dim, i)
            if strategy == +1:
                a0, a1 = [z.genToPow(-1, -j)], [z.genToPow(-1, -j), z.genToPow(dim, D)]
            else:
                a0, a1 = [z.genToPow(dim, -i)], [z.genToPow(dim, D - i)]
            for lst, msk, autos in ((ex.vec, mask, a0),) + (() if native else ((ex.vec1, 1 - mask, a1),)):
                want = _literal(S, C, blk, col, i, j, msk, autos)
                if not np.any(want):
                    assert lst[at] is None, (i, j)
                else:
                    assert np.array_equal(_held(S, lst[at]), want), (i, j)
    assert all(ex.vec[(1 * d + j) if strategy == +1 else (1 + j * D)] is None for j in range(d))
    v = rng.integers(0, P, size=(1, n, d))
    want = _mul_block(ea, v, A, dim, P)
    assert np.array_equal(RM.mulPlain(ea, v, mat), want)
    ct = ea.encrypt(S.sk, v)
    ex.mul(ct, pk=S.sk)
    assert np.array_equal(ea.decrypt_batch(ct, S.sk), want)


def test_ring_entry_matmul1d_integers_and_the_size_one_dimension():
    from helib_amd import bgv_gr_matmul as RM
    m, p, r = 85, 2, 2
    S = T.Setup(m, p, r)
    ea, P, z = S.ea, p ** r, S.ea.zMStar
    n, d, D = ea.size(), ea.getDegree(), ea.sizeOfDimension(0)
    rng = np.random.default_rng(5)
    v = rng.integers(0, P, size=(1, n, d))
    A = rng.integers(0, P, size=(D, D, d))
    mat = RM.MatMul1D(ea, A, 0)
    ex = RM.MatMul1DExec(ea, mat)
    assert not ex.native and not ex.onDevice
    # the plain truth from the restatement's ring product
    blk, col = _break(ea, 0)
    where = {(b, c): s for s, (b, c) in enumerate(zip(blk, col))}
    want = np.zeros((1, n, d), dtype=np.int64)
    for k in range(n // D):
        for j in range(D):
            acc = [0] * d
            for i in range(D):
                acc = [(x + y) % P for x, y in zip(acc, S.ref.mul1(v[0, where[k, i]], A[i, j]))]
            want[0, where[k, j]] = acc
    assert np.array_equal(RM.mulPlain(ea, v, mat), want)
    # the constants against the literal substitution: (diag * mask_i) and the other half moved by rho^D
    g = ex.g
    assert g == 0
    vals = A[None, :, :, None, :]
    for i in (0, 1, D - 1):
        mask = ea.maskSlots(0, i)
        for lst, msk, autos in ((ex.multiplier, mask, []), (ex.multiplier1, 1 - mask, [z.genToPow(0, D)])):
            lit = _literal(S, vals, blk, col, i, 0, msk, autos)
            assert (lst[i] is None) == (not np.any(lit))
            if lst[i] is not None:
                assert np.array_equal(_held(S, lst[i]), lit), i
    ct = ea.encrypt(S.sk, v)
    ex.mul(ct, pk=S.sk)
    assert np.array_equal(ea.decrypt_batch(ct, S.sk), want)
    # a [D, D] integer matrix: the constants of the same diagonals encoded as [B, nslots] constant slots
    Ai = rng.integers(0, P, size=(D, D))
    exi = RM.MatMul1DExec(ea, Ai, dim=0)
    for i in range(D):
        diag = np.array([Ai[(col[s] - i) % D, col[s]] for s in range(n)], dtype=np.int64)
        mask = ea.maskSlots(0, i)
        for lst, msk, k in ((exi.multiplier, mask, 1), (exi.multiplier1, 1 - mask, z.genToPow(0, D))):
            perm = ea.slotPermutation(k)
            consts = (diag * msk)[perm][None]                          # sigma fixes constants: the move is the permutation
            if not np.any(consts):
                assert lst[i] is None
            else:
                poly, cf = ea.enc.encode(consts, 1, list(lst[i][0].idx), coeffs=True)
                assert np.array_equal(lst[i][0].rows, poly.rows) and lst[i][1] == float(ea.enc.norm(cf)[0])
    # the size-1 dimension: another block in every slot
    As = rng.integers(0, P, size=(n, 1, 1, d, d))
    mats = RM.BlockMatMul1D(ea, As, ea.dimension())
    exs = RM.BlockMatMul1DExec(ea, mats)
    assert (exs.D, exs.native, exs.strategy) == (1, True, -1)
    wants = np.array([[x.astype(object) @ As[s, 0, 0].astype(object) % P for s, x in enumerate(row)] for row in v], dtype=np.int64)
    assert np.array_equal(RM.mulPlain(ea, v, mats), wants)
    ct = ea.encrypt(S.sk, v)
    exs.mul(ct, pk=S.sk)
    assert np.array_equal(ea.decrypt_batch(ct, S.sk), wants)
    # linearized polynomials on a ciphertext: sigma itself and a random map
    F = ea._frobenius()
    for L in (F, rng.integers(0, P, size=(d, d))):
        ct = ea.encrypt(S.sk, v)
        RM.applyLinPoly1(ea, ct, RM.buildLinPolyCoeffs(ea, L))
        assert np.array_equal(ea.decrypt_batch(ct, S.sk), np.array(v.astype(object) @ L.astype(object) % P, dtype=np.int64))


def test_at_r_equal_one_every_constant_is_bgv_gf_matmuls():
    from helib_amd import bgv_gf_matmul as GM, bgv_gr_matmul as RM
    m, p = 31, 2
    Sr, Sf = T.Setup(m, p, 1), T.Setup(m, p, 1, gf=True)
    n, d, D = Sr.ea.size(), Sr.ea.getDegree(), Sr.ea.sizeOfDimension(0)
    rng = np.random.default_rng(31)
    A = rng.integers(0, p, size=(D, D, d, d))
    Ag = rng.integers(0, p, size=(D, D, d))

    def same(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert (x is None) == (y is None)
            if x is not None:
                assert np.array_equal(x[0].rows, y[0].rows) and x[0].idx == y[0].idx and x[1] == y[1]
    same(RM.BlockMatMul1DExec(Sr.ea, A, dim=0).vec, GM.BlockMatMul1DExec(Sf.ea, A, dim=0).vec)
    same(RM.MatMul1DExec(Sr.ea, Ag, dim=0).multiplier, GM.MatMul1DExec(Sf.ea, Ag, dim=0).multiplier)
    assert np.array_equal(RM.buildLinPolyCoeffs(Sr.ea, A), GM.buildLinPolyCoeffs(Sf.ea, A))
    v = rng.integers(0, p, size=(1, n, d))
    assert np.array_equal(RM.mulPlain(Sr.ea, v, RM.BlockMatMul1D(Sr.ea, A, 0)), GM.mulPlain(Sf.ea, v, GM.BlockMatMul1D(Sf.ea, A, 0)))


# ---- refusals ----
def test_refusals():
    from helib_amd import bgv_gf_matmul as GM, bgv_gr_matmul as RM, ckks
    ea, ref = _plain_ea(85, 2, 2)
    n, d, D = ea.size(), ea.getDegree(), ea.sizeOfDimension(0)
    z = np.zeros((D, D, d, d), dtype=np.int64)
    for fn in (RM.BlockMatMulFull, RM.BlockMatMulFullExec):
        with pytest.raises(ckks.LogicError, match="BlockMatMulFull"):
            fn(ea, z)
    for fn in (RM.MatMulFull, RM.MatMulFullExec):
        with pytest.raises(ckks.LogicError, match="MatMulFull with ring entries"):
            fn(ea, np.zeros((n, n, d), dtype=np.int64))
    with pytest.raises(ckks.LogicError, match="EvalMap"):
        RM.EvalMap(ea)
    with pytest.raises(ckks.LogicError, match="multipleTransforms"):
        RM.MatMul1D(ea, np.zeros((n // D, D, D, d), dtype=np.int64), 0)
    with pytest.raises(ckks.LogicError, match="one block per slot"):
        RM.BlockMatMul1D(ea, np.zeros((1, 1, d, d), dtype=np.int64), ea.dimension())
    with pytest.raises(ckks.LogicError, match="shape"):
        RM.BlockMatMul1D(ea, np.zeros((D, D, d, d + 1), dtype=np.int64), 0)
    gf, _ = __import__("tests.test_bgv_gf_matmul_host", fromlist=["_plain_ea"])._plain_ea(85, 2)
    for call in (lambda: RM.buildLinPolyCoeffs(gf, z), lambda: RM.BlockMatMul1D(gf, z, 0), lambda: RM.MatMul1D(gf, z[..., 0], 0),
                 lambda: RM.slotAutomorph(gf, 2), lambda: RM.mulPlain(gf, z, None), lambda: RM.linPolyMatrix(object()),
                 lambda: RM.BlockMatMul1DExec(gf, z, dim=0), lambda: RM.MatMul1DExec(gf, z[..., 0], dim=0),
                 lambda: RM.applyLinPoly1(gf, None, z[0, 0])):
        with pytest.raises(ckks.LogicError, match="bgv_gr.EncryptedArray"):
            call()
    # bgv_gf_matmul keeps refusing the ring at r > 1
    with pytest.raises(ckks.LogicError, match="r > 1"):
        GM.BlockMatMul1D(ea, z, 0)
    # fused=True needs an encoder with the call; fused=None follows the class attribute, which is on exactly when the
    # recorded measurement has the fused path winning every alternated pair against the device path
    import json
    with open(os.path.join(ROOT, "profiles", "bgv_gr_matmul.json")) as fh:
        rec = json.load(fh)
    assert rec["same_words_and_sizes"] and rec["mul_correct"]
    assert RM.BlockMatMul1DExec.fuseConstants is RM.MatMul1DExec.fuseConstants is bool(rec["fused_faster_in_every_pair"])
    assert RM.BlockMatMul1DExec(ea, z, dim=0).fusedConstants is False     # no device here: the default falls back to the host
    with pytest.raises(ckks.LogicError, match="encodeGathered"):
        RM.BlockMatMul1DExec(ea, z, dim=0, fused=True)
    with pytest.raises(ckks.LogicError, match="encodeGathered"):
        RM.MatMul1DExec(ea, z[..., 0], dim=0, fused=True)


# ---- the C ABI: declared, listed, exported ----
NAMES = ["hx_bgv_gr_linalg_tables", "hx_bgv_gr_matrix_create", "hx_bgv_gf_encode_gathered"]


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
    assert "bgv_gf_gather_map_kernel" in text
    for fn in ("bgvGrLinalgTables", "bgvGfEncodeGathered"):
        assert callable(getattr(capi, fn))
