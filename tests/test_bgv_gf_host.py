"""BGV slots in GF(p^d) on the host side (no GPU): the C++ table builder (helib_amd/csrc/bgv_gf.h, printed by
tests/cpp/bgv_gf_dump.cpp) against the restatement tests/bgv_gf_ref.py, helib_amd.bgv_gf.EncryptedArray's control flow
over the oracle backend with an injected CPU encoder, the declared and exported symbols, and the refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bgv_crt_ref as R
from tests import bgv_gf_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [(15, 2), (85, 2), (32, 7), (13, 3), (341, 2), (13, 2147483647)]
SRC = os.path.join(ROOT, "tests", "cpp", "bgv_gf_dump.cpp")


def _run(exe, m, p):
    out = subprocess.run([exe, str(m), str(p)], capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    head = out[0].split()
    if head[0] != "ok":
        return {"error": out[0][6:]}
    t = dict(zip(("m", "p", "d", "nslots", "phim", "ld", "ldr", "limit"), map(int, head[1:])))
    rows = [[int(x) for x in line.split()] for line in out[1:]]
    t["gens"], t["ords"], t["G"] = rows[0], rows[1], rows[2]
    n, d = t["nslots"], t["d"]
    at = 3
    for name, count in (("F", n), ("A", n), ("M", n), ("T", d - 1), ("Rx", n)):
        t[name] = rows[at:at + count]
        at += count
    assert at == len(rows)
    return t


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gf") / "bgv_gf_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", SRC, "-o", exe])
    return lambda m, p: _run(exe, m, p)


def _check_tables(t, m, p):
    """every table of bgv_gf.h against the definitions, then the sliding window, the fold and the decode built from
    the printed tables against the literal CRT"""
    ref = GR.tables(m, p)
    n, phim, d = ref.nslots, ref.phim, ref.d
    assert (t["d"], t["nslots"], t["phim"]) == (d, n, phim) and t["ldr"] == (phim + d - 1 + 3) // 4 * 4
    assert (t["gens"], t["ords"]) == (ref.z.gens, ref.z.signedOrds())
    assert t["G"] == [int(x) for x in ref.G] and t["F"] == [[int(x) for x in f] for f in ref.F]
    rng = np.random.default_rng(m)
    X = np.array([0, 1], dtype=np.int64)
    A = [np.array(a, dtype=object).reshape(d, d) for a in t["A"]]
    M = [np.array(a, dtype=object).reshape(d, d) for a in t["M"]]
    for i in range(n):
        f = ref.F[i]
        # the R extension: Rx_i[k] = [X^0](X^k mod F_i) for every k < phim + d - 1
        x, want = np.array([1], dtype=np.int64), []
        for _ in range(phim + d - 1):
            want.append(int(x[0]) if len(x) else 0)
            x = R.prem(np.concatenate([[0], x]), f, p)
        assert t["Rx"][i] == want, i
        # A_i alpha = alpha(X^(t_i)) mod F_i; M_i inverts it through u_j = [X^0](X^j c mod F_i)
        for alpha in (rng.integers(0, p, size=d), np.full(d, p - 1), np.eye(d, dtype=np.int64)[d - 1]):
            c = [int(v) % p for v in np.array([int(v) for v in alpha], dtype=object) @ A[i]]
            w = GR.compose(alpha, ref.xt[i], f, p)
            assert c == [int(v) for v in np.pad(w, (0, d - len(w)))], i
            u = []
            for j in range(d):
                r = R.prem(R.pmul(R.ppowmod(X, j, f, p), np.array(c, dtype=np.int64), p), f, p)
                u.append(int(r[0]) if len(r) else 0)
            assert u == [sum(c[k] * t["Rx"][i][k + j] for k in range(d)) % p for j in range(d)], i
            assert [int(v) % p for v in M[i] @ np.array(u, dtype=object)] == [int(v) for v in alpha], i
    # T_u = X^(phim + u) mod Phi_m
    for u in range(d - 1):
        x = R.prem(np.concatenate([np.zeros(phim + u, dtype=np.int64), [1]]), ref.base.phi, p)
        assert t["T"][u] == [int(v) for v in np.pad(x, (0, phim - len(x)))], u
    # the decomposition end to end on the printed tables
    E = ref.base.E
    a = rng.integers(0, p, size=(2, n, d))
    a[1] = p - 1
    want = ref.encode(a)
    for b in range(2):
        W = [0] * (phim + d - 1)
        for i in range(n):
            c = [int(v) % p for v in np.array([int(v) for v in a[b, i]], dtype=object) @ A[i]]
            for j in range(d):
                if c[j]:
                    for k in range(phim):
                        W[k + j] += c[j] * E[i][k]
        H = [(W[k] + sum(W[phim + u] * t["T"][u][k] for u in range(d - 1))) % p for k in range(phim)]
        assert np.array_equal(ref.base.balanced([H])[0], want[b])
        got = [[int(v) % p for v in M[i] @ np.array([sum(H[k] * t["Rx"][i][k + j] for k in range(phim)) % p for j in range(d)],
                                                    dtype=object)] for i in range(n)]
        assert np.array_equal(np.array(got, dtype=np.int64), a[b] % p)
    assert np.array_equal(ref.decode(want), a % p)


@pytest.mark.parametrize("m,p", RINGS)
def test_tables_against_the_restatement(dump, m, p):
    _check_tables(dump(m, p), m, p)


def test_d1_tables_are_the_integer_path(dump):
    t = dump(64, 193)   # 193 = 1 mod 64: d = 1
    assert t["d"] == 1 and t["T"] == [] and all(a == [1] for a in t["A"]) and all(a == [1] for a in t["M"])
    assert t["G"] == t["F"][0] and len(t["G"]) == 2


def test_limits_are_refused_with_the_figures(dump):
    assert "2^31" in dump(64, 2147483659)["error"]
    why = dump(131, 2)["error"]                     # ord_131(2) = 130
    assert "130" in why and "64" in why


def test_dump_program_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "bgv_gf_dump_san")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", SRC, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0:
        pytest.skip("the sanitizer runtimes do not link here: " + build.stderr.strip().splitlines()[-1][:200])
    run = subprocess.run([exe, "85", "2"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    assert run.stdout.startswith("ok 85 2 8 8 64 ")


# ---- EncryptedArray over the oracle backend with a CPU encoder ----
def _setup(m, p, seed=3, bits=200):
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
    ref = GR.tables(m, p)

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
    hk.add1DMatrices(sk)
    hk.addFrbMatrices(sk)
    return cc, sk, ea, ref


def test_encrypted_array_over_the_oracle_backend():
    m, p = 85, 2
    cc, sk, ea, ref = _setup(m, p)
    n, d = ea.size(), ea.getDegree()
    assert (n, d, ea.getG()) == (8, 8, [int(x) for x in ref.G])
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, p, size=(2, 1, n, d))
    # the plain-side truths against the restatement
    assert np.array_equal(ea.mulPlain(a, b), ref.mul(a, b))
    for j in (1, 3, d):
        assert np.array_equal(ea.frobeniusPlain(a, j), ref.frobenius(a, j)), j
    assert np.array_equal(ea.frobeniusPlain(a, d), a)
    assert np.array_equal(ea.decode(ea.encodeCoeffs(a)), a)
    ca, cb = ea.encrypt(sk, a), ea.encrypt(sk, b)
    assert np.array_equal(ea.decrypt_batch(ca, sk), a)
    prod = ca.clone()
    prod.multiplyBy(cb)
    assert np.array_equal(ea.decrypt_batch(prod, sk), ea.mulPlain(a, b))
    rot = ca.clone()
    ea.rotate(rot, 3)
    assert np.array_equal(ea.decrypt_batch(rot, sk), np.roll(a, 3, axis=1))
    tot = ca.clone()
    ea.totalSums(tot)
    assert np.array_equal(ea.decrypt_batch(tot, sk), np.broadcast_to(a.sum(axis=1, keepdims=True) % p, a.shape))
    for j in (1, d):
        fr = ca.clone()
        ea.frobeniusAutomorph(fr, j)
        assert np.array_equal(ea.decrypt_batch(fr, sk), ea.frobeniusPlain(a, j)), j
    one = ca.clone()
    ea.multByConstant(one, ea.encodePtxt(b))
    ea.addConstant(one, ea.encodePtxt(a))
    assert np.array_equal(ea.decrypt(one, sk), (ea.mulPlain(a, b) + a)[0] % p)
    # constants in the slots: a 2-D array
    k = rng.integers(0, p, size=(1, n))
    assert np.array_equal(ea.decrypt_batch(ea.encrypt(sk, k), sk)[:, :, 0], k)
    assert not np.any(ea.decrypt_batch(ea.encrypt(sk, k), sk)[:, :, 1:])


# ---- the C ABI: declared, listed, exported ----
NAMES = ["hx_bgv_gf_create", "hx_bgv_gf_destroy", "hx_bgv_gf_info", "hx_bgv_gf_encode", "hx_bgv_gf_decode", "hx_bgv_gf_embed"]


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
    # the device code: the kernels by name in the gfx950 code object's symbols
    text = subprocess.run(["nm", "-C", so], capture_output=True, text=True, check=True).stdout
    for kernel in ("bgv_gf_encode_kernel", "bgv_gf_decode_kernel"):
        assert kernel in text, kernel


# ---- refusals ----
def test_refusals():
    from helib_amd import bgv_gf, capi, ckks, ctxt as hc
    ref = GR.tables(85, 2)

    class Enc:
        G = [int(x) for x in ref.G]

        def dims(self):
            return ref.z.gens, ref.z.signedOrds()

        def encode(self, v, mul, idx, coeffs=False):
            raise AssertionError("a refused shape reached the encoder")
    cc = hc.ChainContext(85, 2, 1, bits=100, c=2)
    ea = bgv_gf.EncryptedArray(cc, None, G=list(Enc.G), encoder=Enc())         # F_0 given explicitly (also mod p)
    assert ea.getG() == Enc.G
    bgv_gf.EncryptedArray(cc, None, G=[x + 2 for x in Enc.G], encoder=Enc())
    other = [int(x) for x in ref.F[1]]
    assert other != Enc.G
    with pytest.raises(ckks.LogicError, match="FindRoots"):
        bgv_gf.EncryptedArray(cc, None, G=other, encoder=Enc())
    with pytest.raises(ckks.LogicError, match="deg G"):
        bgv_gf.EncryptedArray(cc, None, G=[1, 1], encoder=Enc())
    with pytest.raises(ckks.LogicError, match="CKKS"):
        bgv_gf.EncryptedArray(hc.ChainContext(64, -1, 20, bits=100, c=2, ckks=True), None, encoder=Enc())
    with pytest.raises(capi.HxError, match="r > 1") as e:
        bgv_gf.EncryptedArray(hc.ChainContext(85, 2, 2, bits=100, c=2), None, encoder=Enc())
    assert e.value.code == capi.HX_ERR_UNSUPPORTED
    with pytest.raises(capi.InvalidArgument):
        ea.encodeCoeffs(np.zeros((1, 9, 8), dtype=np.int64))                   # more values than slots
    with pytest.raises(capi.InvalidArgument):
        ea.encodeCoeffs(np.zeros((1, 8, 9), dtype=np.int64))                   # more coefficients than d
