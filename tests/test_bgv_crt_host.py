"""BGV slots for d > 1 on the host side (no GPU): the C++ table builder (helib_amd/csrc/bgv_crt.h, printed by
tests/cpp/bgv_crt_dump.cpp) against the polynomial restatement tests/bgv_crt_ref.py, the hypercube geometry, and
helib_amd.bgv_crt.EncryptedArray's control flow over the oracle backend with an injected CPU encoder."""
import os
import subprocess

import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_crt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [(17, 2), (51, 2), (85, 2), (105, 2), (119, 2), (31, 3), (64, 2147483647)]
# (p, phi(m), m, d) of the reference's bootstrapping table (tests/GTestBootstrapping.cpp) up to m = 4369
BOOT = [(2, 48, 105, 12), (2, 600, 1023, 10), (2, 1200, 1705, 20), (2, 1728, 4095, 12), (2, 4096, 4369, 16)]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("crt") / "bgv_crt_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "bgv_crt_dump.cpp"),
                           "-o", exe])

    def run(m, p, geom=False):
        out = subprocess.run([exe, str(m), str(p)] + (["geom"] if geom else []), capture_output=True, text=True, timeout=120,
                             check=True).stdout.splitlines()
        head = out[0].split()
        if head[0] != "ok":
            return {"error": out[0][6:]}
        t = dict(zip(("m", "p", "d", "nslots", "phim", "ld", "limit"), map(int, head[1:])))
        t["gens"], t["ords"] = [int(x) for x in out[1].split()], [int(x) for x in out[2].split()]
        if not geom:
            rows = [[int(x) for x in line.split()] for line in out[3:]]
            n = t["nslots"]
            t["F"], t["E"], t["R"] = rows[:n], rows[n:2 * n], rows[2 * n:3 * n]
        return t
    return run


@pytest.mark.parametrize("m,p", RINGS)
def test_tables_against_the_polynomial_restatement(dump, m, p):
    t, ref = dump(m, p), R.tables(m, p)
    n, phim, d = ref.nslots, ref.phim, ref.d
    assert (t["d"], t["nslots"], t["phim"]) == (d, n, phim) and t["limit"] == min((1 << 64) // (p * p), 0xffffffff)
    assert (t["gens"], t["ords"]) == (ref.z.gens, ref.z.signedOrds())
    # F_0 and every F_i
    assert [list(map(int, f)) for f in ref.F] == t["F"]
    assert R.poly_key(t["F"][0]) == min(R.poly_key(f) for f in t["F"])
    # prod F_i = Phi_m mod p
    prod = np.array([1], dtype=np.int64)
    for f in t["F"]:
        prod = R.pmul(prod, np.array(f, dtype=np.int64), p)
    assert np.array_equal(prod, ref.phi)
    # E_i mod F_j = delta_ij, and E against the literal CRT
    for i in range(n):
        for j in range(n):
            r = R.prem(np.array(t["E"][i], dtype=np.int64), np.array(t["F"][j], dtype=np.int64), p)
            assert [int(x) for x in r] == ([1] if i == j else []), (i, j)
    assert t["E"] == ref.E
    # R . H is the constant term of H mod F_i
    rng = np.random.default_rng(m)
    H = rng.integers(0, p, size=(3, phim))
    got = [[sum(int(a) * b for a, b in zip(h, t["R"][i])) % p for i in range(n)] for h in H]
    assert np.array_equal(np.array(got), ref.decode(H))
    # and decode(encode) is the identity
    a = rng.integers(0, p, size=(2, n))
    assert np.array_equal(ref.decode(ref.encode(a)), a)


def test_geometry_of_the_measured_ring_and_the_bootstrapping_rows(dump):
    t = dump(21845, 2, geom=True)
    assert (t["d"], t["nslots"], t["ords"]) == (16, 1024, [-128, -8])
    z = hostnt.ZmStar(21845, 2)
    assert (t["gens"], t["ords"]) == (z.gens, z.signedOrds())
    for p, phim, m, d in BOOT:
        t = dump(m, p, geom=True)
        assert (t["phim"], t["d"], t["nslots"]) == (phim, d, phim // d), m


def test_limits_are_refused_with_the_figure(dump):
    assert "2^31" in dump(64, 2147483659)["error"]            # the first prime above 2^31
    assert "prime" in dump(64, 15)["error"]
    assert "divides" in dump(51, 3)["error"]


# ---- EncryptedArray over the oracle backend with a CPU encoder ----
def _setup(m, p, seed=3, bits=200):
    from oracle import oracle as O
    from oracle.backend import OracleBackend
    from helib_amd import bgv_crt, ctxt as hc, keys as hk
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
    ref = R.tables(m, p)

    class Enc:
        calls = []

        def dims(self):
            return ref.z.gens, ref.z.signedOrds()

        def encode(self, v, mul, idx, coeffs=False):
            self.calls.append(("encode", int(mul), list(idx)))
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
    enc = Enc()
    ea = bgv_crt.EncryptedArray(cc, None, encoder=enc)
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    return cc, sk, ea, enc


def _roll(a, ea, i, k):
    shape = [ea.sizeOfDimension(j) for j in range(ea.dimension())]
    return np.roll(np.asarray(a).reshape(-1, *shape), k, axis=1 + i).reshape(np.asarray(a).shape)


@pytest.mark.parametrize("m,p", [(51, 2), (119, 2)])
def test_rotate1d_over_a_non_native_dimension_is_a_roll(m, p):
    from helib_amd import ckks
    cc, sk, ea, enc = _setup(m, p)
    ref = R.tables(m, p)
    assert (ea.size(), ea.getDegree(), ea.dimension()) == (ref.nslots, ref.d, len(ref.z.gens))
    assert [ea.nativeDimension(i) for i in range(ea.dimension())] == [o > 0 for o in ref.z.signedOrds()]
    assert not all(ea.nativeDimension(i) for i in range(ea.dimension()))
    a = np.random.default_rng(m).integers(0, p, size=(1, ea.size()))
    a[0, 0] = 1
    for i in range(ea.dimension()):
        for k in (1, -1, ea.sizeOfDimension(i) + 1):
            ct = ea.encrypt(sk, a[0])
            ea.rotate1D(ct, i, k)
            assert np.array_equal(ea.decrypt_batch(ct, sk), _roll(a, ea, i, k)), (i, k)
        # shift1D: zero fill
        ct = ea.encrypt(sk, a[0])
        ea.shift1D(ct, i, 1)
        want = _roll(a, ea, i, 1) * (ea._coords(i) >= 1)
        assert np.array_equal(ea.decrypt_batch(ct, sk), want), i
    for f in (lambda c: ea.rotate(c, 1), lambda c: ea.shift(c, 1), ea.totalSums, ea.runningSums):
        if ea.dimension() > 1 or f in (ea.totalSums, ea.runningSums):
            with pytest.raises(ckks.LogicError, match="non-native"):
                f(ea.encrypt(sk, a[0]))


def test_rotate1d_dont_care_issues_one_automorphism():
    cc, sk, ea, enc = _setup(51, 2)
    seen = []

    class Spy:
        parts = True

        def smartAutomorph(self, k):
            seen.append(k)
            return self
    z = ea.zMStar
    assert not ea.nativeDimension(0)
    ea.rotate1D(Spy(), 0, 3, dc=True)
    assert seen == [pow(z.gens[0], 3, 51)]
    # without dc: g^amt on the ciphertext, g^-ord on the copy
    ct = ea.encrypt(sk, [1, 0, 1, 1])
    autos = []
    real = type(ct).smartAutomorph

    def spy(self, k):
        autos.append(k)
        return real(self, k)
    type(ct).smartAutomorph = spy
    try:
        ea.rotate1D(ct, 0, 1)
    finally:
        type(ct).smartAutomorph = real
    assert autos == [z.gens[0] % 51, pow(z.gens[0], -z.ords[0], 51)]
