"""helib_amd.intraslot on the host side (no GPU): the normal basis, linearized polynomials over the Galois ring, the plain
pack / unpack maps, and unpack / repack over the oracle backend with hx_mul_add_circulant stated in python integers
(tests/intraslot_ref.circulant) -- fused against unfused, word for word and field for field.

Chain sizes: every fixture is built with bits = 300, the chain the existing Frobenius tests use at m = 85; the unfused
unpack decrypts correctly with isCorrect() true in every case below (asserted)."""
import numpy as np
import pytest

from tests import bgv_gr_tables as T
from tests import intraslot_ref as IR

RINGS = [(85, 2, 4), (31, 2, 3), (13, 3, 2), (85, 2, 1), (13, 3, 1), (16, 17, 1)]


def _ea(m, p, r, gf=False):
    from helib_amd import bgv_gf, bgv_gr, ctxt as hc
    cc = hc.ChainContext(m, p, r, bits=100, c=2)
    return (bgv_gf if gf else bgv_gr).EncryptedArray(cc, None, encoder=T.TableEncoder(m, p, r))


# ---- the normal basis ----
@pytest.mark.parametrize("m,p,r", RINGS)
def test_normal_basis_matrices(m, p, r):
    from helib_amd import intraslot
    ea, ref = _ea(m, p, r), IR.tables(m, p, r)
    P, d = ref.P, ref.d
    CB, CBi = intraslot.normalBasisMatrices(ea)
    eye = np.eye(d, dtype=object)
    assert np.array_equal(CB.astype(object).dot(CBi.astype(object)) % P, eye)
    assert np.array_equal(CBi.astype(object).dot(CB.astype(object)) % P, eye)
    for i in range(d):                                   # row i + 1 is sigma of row i, and sigma^d closes the cycle
        assert ref.sigma1(CB[i]) == [int(x) for x in CB[(i + 1) % d]], i
    theta, want = ref.first_normal()                     # the rule, by brute force
    assert [int(x) for x in CB[0]] == theta and [[int(x) for x in row] for row in CB] == want


def test_the_rules_choice_is_pinned():
    """(85, 2): d = 8; (13, 3): d = 3.  The values come from tests/intraslot_ref.first_normal: every candidate in the
    rule's order, its conjugates by Horner, the determinant mod p by elimination."""
    from helib_amd import intraslot
    for m, p, r in ((85, 2, 1), (85, 2, 4), (13, 3, 1), (13, 3, 2)):
        ref = IR.tables(m, p, r)
        d = ref.d
        theta, _ = ref.first_normal()
        rejected = []
        for cand in [[1 if i == k else 0 for i in range(d)] for k in range(d)]:
            if cand == theta:
                break
            assert IR.det_mod(ref.conjugates(cand), p) == 0
            rejected.append(cand)
        assert [1] + [0] * (d - 1) in rejected or d == 1          # X^0 = 1 is never normal for d > 1
        assert IR.det_mod(ref.conjugates(theta), p) != 0
        assert [int(x) for x in intraslot.normalBasisMatrices(_ea(m, p, r))[0][0]] == theta
    # the choice depends on the residues mod p alone: r does not move it
    assert IR.tables(85, 2, 1).first_normal()[0] == IR.tables(85, 2, 4).first_normal()[0]
    assert IR.tables(13, 3, 1).first_normal()[0] == IR.tables(13, 3, 2).first_normal()[0]


def test_injected_normal_element():
    from helib_amd import ckks, intraslot
    m, p, r = 13, 3, 2
    ea, ref = _ea(m, p, r), IR.tables(m, p, r)
    with pytest.raises(ckks.LogicError, match="not normal"):
        intraslot.normalBasisMatrices(ea, normal_element=[1, 0, 0])          # 1 is fixed by sigma
    with pytest.raises(ckks.LogicError, match="not normal"):
        intraslot.normalBasisMatrices(ea, normal_element=[3, 3, 6])          # zero mod p
    with pytest.raises(ckks.LogicError, match="more than d"):
        intraslot.normalBasisMatrices(ea, normal_element=[1, 1, 1, 1])
    # another normal element than the rule's: found by brute force over all of Z_3[X] / G
    rule = ref.first_normal()[0]
    other = next(t for t in ([a, b, c] for a in range(3) for b in range(3) for c in range(3))
                 if t != rule and IR.det_mod(ref.conjugates(t), p))
    lifted = [x + 3 for x in other]                                          # any lift of a normal element is normal
    CB, CBi = intraslot.normalBasisMatrices(ea, normal_element=lifted)
    assert [int(x) for x in CB[0]] == lifted
    assert np.array_equal(CB.astype(object).dot(CBi.astype(object)) % 9, np.eye(3, dtype=object))
    a = np.random.default_rng(0).integers(0, 9, size=(1, 4, 3))
    c = intraslot.unpackPlain(ea, a, normal_element=lifted)
    assert np.array_equal(intraslot.repackPlain(ea, c, normal_element=lifted), a)
    assert not np.array_equal(c, intraslot.unpackPlain(ea, a))


# ---- linearized polynomials ----
@pytest.mark.parametrize("m,p,r", RINGS)
def test_build_lin_poly_coeffs(m, p, r):
    from helib_amd import intraslot
    ea, ref = _ea(m, p, r), IR.tables(m, p, r)
    P, d, n = ref.P, ref.d, ref.nslots
    rng = np.random.default_rng(m + 3 * r)
    L = rng.integers(0, P, size=(d, d))
    C = intraslot.buildLinPolyCoeffs(ea, L)
    alpha = rng.integers(0, P, size=(1, n, d))
    alpha[0, 0] = P - 1
    want = np.array(alpha.astype(object).dot(L.astype(object)) % P, dtype=np.int64)         # L(alpha) = sum_j alpha_j L[j]
    assert np.array_equal(intraslot.applyLinPolyPlain(ea, C, alpha), want)
    # the same sum through the restatement's product and sigma, on two slots
    for s in range(min(n, 2)):
        acc = [0] * d
        for k in range(d):
            acc = [(x + y) % P for x, y in zip(acc, ref.mul1(C[k], ref.sigma1(alpha[0, s], k)))]
        assert acc == [int(x) for x in want[0, s]]
    if r == 1:
        from helib_amd import bgv_gf_matmul
        gf = _ea(m, p, 1, gf=True)
        assert np.array_equal(C, bgv_gf_matmul.buildLinPolyCoeffs(gf, L))
        assert np.array_equal(intraslot.buildLinPolyCoeffs(gf, L), C)
    stack = rng.integers(0, P, size=(2, d, d))
    assert np.array_equal(intraslot.buildLinPolyCoeffs(ea, stack)[1], intraslot.buildLinPolyCoeffs(ea, stack[1]))


# ---- the plain side ----
@pytest.mark.parametrize("m,p,r", RINGS)
def test_unpack_plain_and_repack_plain(m, p, r):
    from helib_amd import intraslot
    ea, ref = _ea(m, p, r), IR.tables(m, p, r)
    P, d, n = ref.P, ref.d, ref.nslots
    a = np.random.default_rng(m + r).integers(0, P, size=(2, n, d))
    a[1] = P - 1
    c = intraslot.unpackPlain(ea, a)
    assert np.array_equal(intraslot.repackPlain(ea, c), a)
    assert np.array_equal(intraslot.unpackPlain(ea, intraslot.repackPlain(ea, a)), a)
    CB = [[int(x) for x in row] for row in intraslot.normalBasisMatrices(ea)[0]]
    for s in range(min(n, 2)):                            # the coordinates by solving the system, another way
        assert ref.coords(CB, a[0, s]) == [int(x) for x in c[0, s]]
    # unpack's constants: sum_j C[(i + j) mod d] sigma^j(alpha) is coordinate i, as a constant
    enc = intraslot.buildUnpackSlotEncoding(ea)
    assert len(enc) == d and all(e.ptxtSpace == P for e in enc)
    C = [e.v[0, 0] for e in enc]
    assert all(np.array_equal(e.v[0], np.broadcast_to(e.v[0, 0], (n, d))) for e in enc)
    fr = [ea.frobeniusPlain(a, j) for j in range(d)]
    for i in range(d):
        got = sum(ea.mulPlain(np.broadcast_to(C[(i + j) % d], a.shape), fr[j]) for j in range(d)) % P
        assert np.array_equal(got[:, :, 0], c[:, :, i]) and not np.any(got[:, :, 1:]), i


@pytest.mark.parametrize("m,r", [(85, 1), (31, 3)])
def test_pack_constants_and_unpack_slots_round_trip_bit_patterns(m, r):
    from helib_amd import ckks, intraslot
    ea = _ea(m, 2, r)
    n, d = ea.size(), ea.getDegree()
    data = [int(x) for x in np.random.default_rng(m).integers(0, 1 << d, size=n)]
    data[0], data[-1] = (1 << d) - 1, 0
    poly = intraslot.packConstants(ea, data, d)
    assert poly.shape == (1, ea.cc.phim)
    assert intraslot.unpackSlots(ea, ea.decode(poly)) == data
    low = intraslot.packConstants(ea, data, 3)
    assert intraslot.unpackSlots(ea, ea.decode(low)) == [x & 7 for x in data]
    one = intraslot.packConstant(ea, 0b1011, d)
    assert intraslot.unpackSlots(ea, ea.decode(one)) == [0b1011] * n
    assert np.array_equal(intraslot.unpackPlain(ea, ea.decode(one))[0, :, :4], np.broadcast_to([1, 1, 0, 1], (n, 4)))
    with pytest.raises(ckks.LogicError, match="data size"):
        intraslot.packConstants(ea, data[:-1], d)
    with pytest.raises(ckks.LogicError, match="capacity"):
        intraslot.packConstant(ea, 1, d + 1)


# ---- unpack / repack over the oracle backend ----
@pytest.fixture(scope="module", params=[(16, 17, 1), (13, 3, 2), (31, 2, 3), (85, 2, 4)], ids=lambda c: "m%d-p%d-r%d" % c)
def setup(request):
    """d = 1, 3, 5, 8; bits = 300"""
    m, p, r = request.param
    s = T.Setup(m, p, r, bits=300)
    assert s.ea.getDegree() == {16: 1, 13: 3, 31: 5, 85: 8}[m]
    return s


def test_unpack_fused_against_unfused_and_repack(setup):
    from helib_amd import intraslot
    from helib_amd import ctxt as hc
    s = setup
    ea, sk, P = s.ea, s.sk, s.P
    d, n = ea.getDegree(), ea.size()
    a = s.slots(11)
    a[0, 0] = P - 1
    ct = ea.encrypt(sk, a)
    enc = intraslot.buildUnpackSlotEncoding(ea)
    want = intraslot.unpackPlain(ea, a)
    assert hc.Ctxt.fuseCirculant is False
    before = T.state(ct)
    s.circ.clear()
    plain = intraslot.unpack(ea, ct, enc)                                    # fused=None follows the class switch
    assert s.circ == [] and len(plain) == d
    T.same(before, T.state(ct))                                              # the input is left as it was
    for i, u in enumerate(plain):
        assert u.isCorrect(), i
        got = ea.decrypt_batch(u, sk)
        assert np.array_equal(got[:, :, 0], want[:, :, i]) and not np.any(got[:, :, 1:]), i
    fused = intraslot.unpack(ea, ct, enc, fused=True)
    assert s.circ == [(d, d)]
    T.same(before, T.state(ct))
    for u, v in zip(plain, fused):
        T.same(T.state(u), T.state(v))
    # n < d: the first n of them, one call
    for k in sorted({1, max(1, d - 1)}):
        s.circ.clear()
        part = intraslot.unpack(ea, ct, enc, n=k, fused=True)
        assert s.circ == [(d, k)] and len(part) == k
        for u, v in zip(intraslot.unpack(ea, ct, enc, n=k, fused=False), part):
            T.same(T.state(u), T.state(v))
        for u, v in zip(plain, part):
            T.same(T.state(u), T.state(v))
    # repack brings the slots back; the partial sum is the plain partial sum
    back = intraslot.repack(ea, fused)
    assert back.isCorrect() and np.array_equal(ea.decrypt_batch(back, sk), a)
    if d > 1:
        some = intraslot.repack(ea, plain[:d - 1])
        keep = want.copy()
        keep[:, :, d - 1:] = 0
        assert np.array_equal(ea.decrypt_batch(some, sk), intraslot.repackPlain(ea, keep))
    # the list overloads slice as the reference does
    many = intraslot.unpackMany(ea, [ct, ct], enc, d + 1, fused=True)
    assert len(many) == d + 1
    T.same(T.state(many[d]), T.state(plain[0]))
    packed = intraslot.repackMany(ea, many)
    assert len(packed) == 2 and np.array_equal(ea.decrypt_batch(packed[0], sk), a)


def test_circulant_combination_with_other_int_factors_and_prime_sets(setup):
    """Ctxt.circulantCombination on terms whose intFactors differ (each multiplied by another unit) and one of which sits
    on fewer primes: addCtxt harmonises with (e1, e2) and mods up, which the fused form folds into one mod-up and one
    product by an integer per term.  (The Frobenius images of one ciphertext leave their key switches with equal
    intFactors on one prime set, so unpack itself never gets here.)"""
    from oracle.backend import OPoly
    from helib_amd import ctxt as hc
    s = setup
    ea, sk, P, p = s.ea, s.sk, s.P, s.p
    d, n = ea.getDegree(), ea.size()
    rng = np.random.default_rng(21)
    units = [u for u in range(2, P) if u % p]
    vals, cts = [], []
    for j in range(d):
        a = rng.integers(0, P, size=(1, n, d))
        ct = ea.encrypt(sk, a)
        u = units[j % len(units)]
        ct.multByScalar(u)
        vals.append(a * u % P)
        cts.append(ct)
    if d > 1:
        cts[1].modDownToSet(sorted(cts[1].primeSet)[:-1])
    ks = [rng.integers(0, P, size=(1, n, d)) for _ in range(d)]
    primes = sorted(frozenset().union(*[c.primeSet for c in cts]))
    consts = [ea.enc.encode(k, 1, primes) for k in ks]
    before = [T.state(c) for c in cts]
    plain = hc.Ctxt.circulantCombination(cts, consts, fused=False)
    calls, orig = [], OPoly.mulConstant

    def counted(self, num):
        calls.append(int(num))
        return orig(self, num)
    OPoly.mulConstant = counted
    s.circ.clear()
    try:
        fused = hc.Ctxt.circulantCombination(cts, consts, fused=True)
    finally:
        OPoly.mulConstant = orig
    assert s.circ == [(d, d)]
    if d > 1:
        assert any(c not in (0, 1) for c in calls)                          # integers were folded in
    for c, b in zip(cts, before):
        T.same(T.state(c), b)                                               # the terms are left as they were
    for i, (u, v) in enumerate(zip(plain, fused)):
        T.same(T.state(u), T.state(v))
        want = sum(ea.mulPlain(ks[(i + j) % d], vals[j]) for j in range(d)) % P
        assert np.array_equal(ea.decrypt_batch(v, sk), want), i


def test_unpack_refusals():
    from helib_amd import bgv_pr, ckks, intraslot
    from helib_amd import ctxt as hc
    s = T.Setup(13, 3, 2, bits=300, circulant=False)                         # a backend without the call
    ea, sk = s.ea, s.sk
    ct = ea.encrypt(sk, s.slots(1))
    enc = intraslot.buildUnpackSlotEncoding(ea)
    with pytest.raises(ckks.LogicError, match="no mulAddCirculant"):
        intraslot.unpack(ea, ct, enc, fused=True)
    with pytest.raises(RuntimeError, match="no mulAddCirculant"):
        hc.Ctxt.circulantCombination([ct], [None], fused=True)
    assert len(intraslot.unpack(ea, ct, enc, n=2)) == 2                      # fused=None: the sequence
    with pytest.raises(ckks.LogicError, match="1 <= n <= d"):
        intraslot.unpack(ea, ct, enc, n=4)
    with pytest.raises(ckks.LogicError, match="constants"):
        intraslot.unpack(ea, ct, enc[:2])
    with pytest.raises(ckks.LogicError, match="Not enough ciphertexts"):
        intraslot.unpackMany(ea, [ct], enc, 4)
    with pytest.raises(ckks.LogicError, match="between 1 and d"):
        intraslot.repack(ea, [ct] * 4)
    pr = bgv_pr.EncryptedArray(s.cc, None, encoder=s.enc)
    with pytest.raises(ckks.LogicError, match="bgv_gf.EncryptedArray or"):
        intraslot.buildUnpackSlotEncoding(pr)


def test_unpack_over_bgv_gf():
    """the r = 1 class of helib_amd.bgv_gf: the same module, the same words as bgv_gr at r = 1"""
    from helib_amd import intraslot
    m, p = 31, 2
    g, f = T.Setup(m, p, 1, bits=300), T.Setup(m, p, 1, bits=300, gf=True)
    a = g.slots(4)
    eg, ef = intraslot.buildUnpackSlotEncoding(g.ea), intraslot.buildUnpackSlotEncoding(f.ea)
    assert all(np.array_equal(x.v, y.v) and np.array_equal(x.poly, y.poly) for x, y in zip(eg, ef))
    ug = intraslot.unpack(g.ea, g.ea.encrypt(g.sk, a), eg, fused=True)
    uf = intraslot.unpack(f.ea, f.ea.encrypt(f.sk, a), ef, fused=True)
    for x, y in zip(ug, uf):
        T.same(T.state(x), T.state(y))
    assert np.array_equal(f.ea.decrypt_batch(intraslot.repack(f.ea, uf), f.sk), a)
