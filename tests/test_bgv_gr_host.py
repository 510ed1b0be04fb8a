"""Galois-ring slots (Z_(p^r)[X] / G) on the host side (no GPU): the tables helib_amd/csrc/bgv_gf.h builds at r >= 1
(tests/cpp/bgv_gr_dump.cpp), run as the device kernels run them (tests/bgv_gr_tables.TableEncoder), against the literal
CRT of tests/intraslot_ref.py; helib_amd.bgv_gr.EncryptedArray's plain side and its control flow over the oracle backend;
the declared and exported symbols; the refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bgv_gf_ref as GF
from tests import bgv_gr_tables as T
from tests import bgv_pr_ref as PR
from tests import intraslot_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = [(85, 2, 4), (31, 2, 3), (13, 3, 2), (341, 2, 2)]


def _ea(m, p, r):
    from helib_amd import bgv_gr, ctxt as hc
    cc = hc.ChainContext(m, p, r, bits=100, c=2)
    return bgv_gr.EncryptedArray(cc, None, encoder=T.TableEncoder(m, p, r))


def _rand(rng, P, n, d, B=2):
    a = rng.integers(0, P, size=(B, n, d))
    a[B - 1] = P - 1                                     # every word at its largest
    return a


@pytest.mark.parametrize("m,p,r", RINGS)
def test_tables_encode_and_decode_as_the_literal_crt(m, p, r):
    """the words of encode and decode, the round trip, and the product: every slot is the same ring Z_(p^r)[X] / G"""
    enc, ref = T.TableEncoder(m, p, r), IR.tables(m, p, r)
    P, n, d, N = ref.P, ref.nslots, ref.d, ref.phim
    t = enc.t
    assert (t["P"], t["d"], t["nslots"], t["phim"]) == (P, d, n, N)
    assert t["limit"] == min((1 << 64) // (P * P), 0xffffffff) >= 1            # computed from p^r
    assert t["G"] == ref.G and t["F"] == ref.F                                 # the Hensel lifts, by another method
    rng = np.random.default_rng(m + r)
    a, b = _rand(rng, P, n, d), _rand(rng, P, n, d)
    ha, hb = enc.coeffs(a), enc.coeffs(b)
    assert np.array_equal(ha, ref.encode(a)) and np.array_equal(enc.coeffs(b, 5), ref.encode(b, 5))
    assert np.array_equal(enc.slots(ha), a) and np.array_equal(ref.decode(ha), a)
    ea = _ea(m, p, r)
    assert np.array_equal(ea.decode(ea.encodeCoeffs(a)), a)
    phi = ref.base.phi
    prod = [PR.mulmod([int(x) for x in ha[k]], [int(x) for x in hb[k]], phi, P) for k in range(2)]
    prod = [row + [0] * (N - len(row)) for row in prod]
    want = ref.mul(a, b)
    assert np.array_equal(enc.slots(prod), want)
    assert np.array_equal(ea.mulPlain(a, b), want)


def test_tables_at_the_largest_degree_against_the_literal_crt():
    """(641, 2, 2): d = 64 = ord_641(2), 10 slots, phi = 640.  tests/test_bgv_gr_gpu.py compares the device with
    TableEncoder at this ring; here TableEncoder's tables (A, M, T, Rx at d = 64) meet a reference that shares nothing
    with them: factors lifted by Hensel's lemma, idempotents by Newton's iteration, Horner in Z_4[X] / F_i."""
    m, p, r = 641, 2, 2
    enc = T.TableEncoder(m, p, r)
    ref = IR.from_golden(os.path.join(ROOT, "tests", "golden", "gr_641_2_2.json"))       # lifted once: seconds at d = 64
    assert (enc.d, enc.n, enc.phim) == (64, 10, 640) and enc.t["G"] == ref.G and enc.t["F"] == ref.F
    rng = np.random.default_rng(641)
    a = rng.integers(0, 4, size=(1, 10, 64))
    a[0, 9] = 3
    h = enc.coeffs(a, 3)
    assert np.array_equal(h, ref.encode(a, 3))
    f = rng.integers(-2 ** 40, 2 ** 40, size=(1, 640))
    assert np.array_equal(enc.slots(f), ref.decode(f))


@pytest.mark.parametrize("m,p,r", RINGS)
def test_tables_mod_p_are_bgv_gfs_and_constants_are_bgv_prs(m, p, r):
    t, t1 = T.dump(m, p, r), T.dump(m, p, 1)
    for name in ("G", "F", "A", "M", "E", "T", "Rx"):
        assert [[x % p for x in row] for row in (t[name] if name != "G" else [t[name]])] == \
            (t1[name] if name != "G" else [t1[name]]), name
    assert (t["gens"], t["ords"], t["d"], t["nslots"]) == (t1["gens"], t1["ords"], t1["d"], t1["nslots"])
    # r = 1 through the new argument is hx_bgv_gf_create's table, byte for byte
    assert T.raw(m, p, 1) == T.raw(m, p, 0)
    ref1 = GF.tables(m, p)
    assert t1["G"] == [int(x) for x in ref1.G] and t1["F"] == [[int(x) for x in f] for f in ref1.F]
    # [B, nslots] constants: the words bgv_pr gives
    pr = PR.tables(m, p, r)
    k = np.random.default_rng(m).integers(0, p ** r, size=(2, t["nslots"]))
    enc = T.TableEncoder(m, p, r)
    assert np.array_equal(enc.coeffs(k, 3), pr.encode(k, 3))
    got = enc.slots(pr.encode(k))
    assert np.array_equal(got[:, :, 0], k) and not np.any(got[:, :, 1:])
    assert np.array_equal(_ea(m, p, r).encodeCoeffs(k), pr.encode(k))


@pytest.mark.parametrize("m,p,r", RINGS)
def test_sigma_is_a_ring_automorphism_of_order_d(m, p, r):
    ea, ref = _ea(m, p, r), IR.tables(m, p, r)
    P, n, d = ref.P, ref.nslots, ref.d
    rng = np.random.default_rng(7 * m + r)
    a, b = _rand(rng, P, n, d), _rand(rng, P, n, d)
    assert np.array_equal(ea.frobeniusPlain(a, d), a) and np.array_equal(ea.frobeniusPlain(a, 0), a)
    assert np.array_equal(ea.frobeniusPlain(a[:1, :2], 1)[:, :2], ref.sigma(a[:1, :2], 1)[:, :2])
    assert np.array_equal(ea.frobeniusPlain(a[:1, :2], d - 1)[:, :2], ref.sigma(a[:1, :2], d - 1)[:, :2])
    for j in (1, d - 1):
        assert np.array_equal(ea.frobeniusPlain(ea.mulPlain(a, b), j), ea.mulPlain(ea.frobeniusPlain(a, j), ea.frobeniusPlain(b, j)))
        assert np.array_equal(ea.frobeniusPlain((a + b) % P, j), (ea.frobeniusPlain(a, j) + ea.frobeniusPlain(b, j)) % P)
    # on the encoded side sigma is X -> X^p: the plaintext automorphism moves every slot by sigma
    enc = T.TableEncoder(m, p, r)
    h = [int(x) for x in enc.coeffs(a[:1])[0]]
    hp = [0] * m
    for k, x in enumerate(h):
        hp[k * p % m] += x
    hp = PR._divmod(hp, ref.base.phi, P)[1]
    assert np.array_equal(enc.slots([hp + [0] * (ref.phim - len(hp))]), ea.frobeniusPlain(a[:1], 1))


def test_r1_is_bgv_gf_word_for_word():
    from helib_amd import bgv_gf, bgv_gr, ctxt as hc
    m, p = 85, 2
    cc = hc.ChainContext(m, p, 1, bits=100, c=2)
    enc = T.TableEncoder(m, p, 1)
    gr, gf = bgv_gr.EncryptedArray(cc, None, encoder=enc), bgv_gf.EncryptedArray(cc, None, encoder=enc)
    ref = GF.tables(m, p)
    a, b = np.random.default_rng(1).integers(0, p, size=(2, 1, 8, 8))
    assert gr.getG() == gf.getG() and gr.getDegree() == gf.getDegree() == 8 and gr.getPPowR() == 2
    assert np.array_equal(gr.encodeCoeffs(a), ref.encode(a)) and np.array_equal(gr.encodeCoeffs(a), gf.encodeCoeffs(a))
    assert np.array_equal(gr.mulPlain(a, b), gf.mulPlain(a, b))
    assert np.array_equal(gr.frobeniusPlain(a, 3), gf.frobeniusPlain(a, 3))
    assert np.array_equal(gr._frobenius(), gf._frobenius())
    # both classes run one body (helib_amd.slot_ring), so the arithmetic is pinned to the independent restatement
    assert np.array_equal(gf.mulPlain(a, b), ref.mul(a, b))
    assert np.array_equal(gf.frobeniusPlain(a, 3), ref.frobenius(a, 3))


def test_encrypted_array_over_the_oracle_backend():
    """bits = 300 (the chain the existing Frobenius tests use at m = 85); m = 13, p^r = 9: d = 3, 4 slots"""
    s = T.Setup(13, 3, 2, bits=300)
    ea, sk, P = s.ea, s.sk, s.P
    n, d = ea.size(), ea.getDegree()
    assert (n, d, ea.getG(), ea.getPPowR()) == (4, 3, s.ref.G, 9)
    a, b = s.slots(5), s.slots(6)
    ca, cb = ea.encrypt(sk, a), ea.encrypt(sk, b)
    assert np.array_equal(ea.decrypt_batch(ca, sk), a)
    prod = ca.clone()
    prod.multiplyBy(cb)
    assert np.array_equal(ea.decrypt_batch(prod, sk), ea.mulPlain(a, b))
    rot = ca.clone()
    ea.rotate(rot, 1)
    assert np.array_equal(ea.decrypt_batch(rot, sk), np.roll(a, 1, axis=1))
    tot = ca.clone()
    ea.totalSums(tot)
    assert np.array_equal(ea.decrypt_batch(tot, sk), np.broadcast_to(a.sum(axis=1, keepdims=True) % P, a.shape))
    for j in (1, d):
        fr = ca.clone()
        ea.frobeniusAutomorph(fr, j)
        assert np.array_equal(ea.decrypt_batch(fr, sk), ea.frobeniusPlain(a, j)), j
    one = ca.clone()
    ea.multByConstant(one, ea.encodePtxt(b))
    ea.addConstant(one, ea.encodePtxt(a))
    assert np.array_equal(ea.decrypt(one, sk), (ea.mulPlain(a, b) + a)[0] % P)
    # a ciphertext at p^(r-1): 3 * a, divided by p, is a mod 3, decoded through the p^2 tables
    low = ea.encrypt(sk, a * 3 % P)
    low.divideByP()
    assert low.ptxtSpace == 3 and np.array_equal(ea.decrypt_batch(low, sk), a % 3)
    k = np.random.default_rng(2).integers(0, P, size=(1, n))
    got = ea.decrypt_batch(ea.encrypt(sk, k), sk)
    assert np.array_equal(got[:, :, 0], k) and not np.any(got[:, :, 1:])


# ---- the C ABI: declared, listed, exported ----
def test_symbols_are_declared_listed_and_exported():
    from helib_amd import build, capi
    header = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    names = {"hx_bgv_gf_create_pr": 4, "hx_bgv_gf_space": 3, "hx_mul_add_circulant": 7}
    so = build.build()
    dyn = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    lib = capi.lib()
    for name, nargs in names.items():
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SYMBOLS, name
        assert re.search(r" T %s$" % name, dyn, re.M), name
        assert len(getattr(lib, name).argtypes) == nargs
    text = subprocess.run(["nm", "-C", so], capture_output=True, text=True, check=True).stdout
    assert "mul_add_circulant_kernel" in text
    assert len(lib.hx_bgv_gf_create.argtypes) == 3 and len(lib.hx_mul_add_many.argtypes) == 7           # left alone


# ---- refusals ----
def test_refusals():
    from helib_amd import bgv, bgv_gf_matmul, bgv_gr, bgv_hypercube, bgv_matmul, ckks, ctxt as hc
    m, p, r = 13, 3, 2
    enc = T.TableEncoder(m, p, r)
    cc = hc.ChainContext(m, p, r, bits=100, c=2)
    ea = bgv_gr.EncryptedArray(cc, None, G=list(enc.G), encoder=enc)                 # the lifted F_0 given explicitly
    bgv_gr.EncryptedArray(cc, None, G=[x + 9 for x in enc.G], encoder=enc)           # any representatives mod p^r
    with pytest.raises(ckks.LogicError, match="FindRoots"):
        bgv_gr.EncryptedArray(cc, None, G=enc.t["F"][1], encoder=enc)
    with pytest.raises(ckks.LogicError, match="FindRoots"):                          # F_0 mod p is not its lift
        bgv_gr.EncryptedArray(cc, None, G=[x % p for x in enc.G], encoder=enc)
    with pytest.raises(ckks.LogicError, match="deg G"):
        bgv_gr.EncryptedArray(cc, None, G=[1, 1], encoder=enc)
    with pytest.raises(ckks.LogicError, match="CKKS"):
        bgv_gr.EncryptedArray(hc.ChainContext(64, -1, 20, bits=100, c=2, ckks=True), None, encoder=enc)

    class Ctx:
        """the fields the constructor reads before it builds anything"""
        ckks = False

        def __init__(self, m, p, r):
            self.m, self.p, self.r, self.ptxtSpace = m, p, r, p ** r
    with pytest.raises(ckks.LogicError, match="2\\^31"):
        bgv_gr.EncryptedArray(Ctx(13, 3, 20), None, encoder=enc)                     # 3^20 > 2^31
    with pytest.raises(ckks.LogicError, match="d <= 64"):
        bgv_gr.EncryptedArray(Ctx(131, 2, 2), None, encoder=enc)                     # ord_131(2) = 130
    assert "2^31" in T.dump(13, 3, 20)["error"]
    why = T.dump(131, 2, 2)["error"]
    assert "130" in why and "64" in why
    # matrix products over this class at r > 1
    mat = np.zeros((4, 4), dtype=np.int64)
    with pytest.raises(ckks.LogicError, match="r > 1"):
        bgv_matmul.MatMul1DExec(ea, mat, dim=0)
    with pytest.raises(ckks.LogicError, match="r > 1"):
        bgv_hypercube.MatMul1DExec(ea, mat, dim=0)
    with pytest.raises(ckks.LogicError, match="r > 1"):
        bgv_gf_matmul.buildLinPolyCoeffs(ea, np.zeros((3, 3), dtype=np.int64))
    with pytest.raises(ckks.LogicError, match="r > 1"):
        bgv_gf_matmul.linPolyMatrix(ea)
    with pytest.raises(ckks.LogicError, match="r > 1"):
        bgv_gf_matmul.applyLinPoly1(ea, None, np.zeros((3, 3), dtype=np.int64))
    assert isinstance(ea, bgv.EncryptedArray)
