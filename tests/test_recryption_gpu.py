"""The pre-processing of recryption on the device: recrypt_prep_kernel (hx_recrypt_prep) against tests/recryption_ref.py on
synthetic rows and on the inputs built for every branch, its refusals, and helib_amd.recryption.rawModSwitch of a real
ciphertext against the same restatement applied to the downloaded parts.  Everything here is an integer: every
comparison is exact.

The shapes of the kernel tests: phi(m) = 8, 36, 48 and 64 (one workgroup, partly idle) at k = 1, 3, 5 and batch 1 and 3;
phi(m) = 256, 300, 512 and 576 at batch 2 (one full workgroup, a second one of 44 words, two and three workgroups, the
ties of batch element 1 decided at j >= 256); every k from 1 to 16, and 17 refused; seven parameter sets at the edges of
what the plan admits (q and p^r just below 2^30, p^e' = 1 and q - 1, odd p, q = 3) at k = 1, 4 and 16.  The tables of the
last three are tests/recryption_ref.py's, which tests/test_recryption_host.py replays on the CPU."""
import ctypes as C

import numpy as np
import pytest

from tests import recryption_ref as RR

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


def _context(hx, cc):
    g = hx.Context(cc.m)
    for q in cc.primes:
        g.add_prime(q)
    return g


# ---- (a) the kernel against the restatement ----
# phi(m) = 8 (less than a wave), 36 and 48; p = 2 (the delta and divisibility ties) and p = 7 (q even: the x tie);
# k = 1, 3 and 3 + the special primes; one target and all; batch 1 and 3 (3 * 36 and 3 * 48 words: no multiple of a
# wave, the last block partly idle); p2ePrime = p^e' and 1
@pytest.mark.parametrize("key", [(15, 2, 1), (57, 7, 1), (105, 2, 1)])
@pytest.mark.parametrize("k", [1, 3, 5])
def test_kernel_is_the_restatement(hx, key, k):
    cc = RR.chain(*key)
    g = _context(hx, cc)
    src_idx = (list(cc.ctxtPrimes)[:3] + list(cc.specialPrimes))[:k]
    assert len(src_idx) == k and (k < 5 or len(cc.specialPrimes) == 2)
    everything = list(range(len(cc.primes)))
    for nt, B, e_one in ((1, 1, False), (None, 3, False), (1, 3, True)):
        src, tgt, q, p, p2r, p2e = RR.params(key, k, nt)
        tgt_idx = everything if nt is None else everything[-nt:]
        assert [cc.primes[i] for i in src_idx] == src and [cc.primes[i] for i in tgt_idx] == tgt
        if e_one:
            p2e = 1
        rows = RR.synthetic_rows(src, q, p, p2r, p2e, B, g.phim, key[0] + k)
        seed, part = 0xC0FFEE + k + (1 << 63), k % 2
        want = RR.prep(rows, src, tgt, q, p, p2r, p2e, seed, part)
        a = hx.DoubleCRT(g, src_idx, B, data=rows)
        out, x, v = hx.recryptPrep(a, tgt_idx, q, p, p2r, p2e, seed, part, debug=True)
        assert np.array_equal(x, want[0]) and np.array_equal(v, want[1])
        assert np.array_equal(out.download(), want[2])
        assert out.getIndexSet() == tgt_idx and np.array_equal(a.download(), rows)       # the input is left alone
        plain = hx.recryptPrep(a, tgt_idx, q, p, p2r, p2e, seed, part)                    # without the debug arrays
        assert np.array_equal(plain.download(), want[2])
        if not e_one and B == 3:                                                          # the ties do follow the seed
            other = RR.prep(rows, src, tgt[:1], q, p, p2r, p2e, seed + 1, part)
            assert not np.array_equal(other[1], want[1])
            got = hx.recryptPrep(a, tgt_idx[:1], q, p, p2r, p2e, seed + 1, part, debug=True)
            assert np.array_equal(got[2], other[1]) and np.array_equal(got[0].download(), other[2])


def test_kernel_takes_sixteen_rows(hx):
    cc = RR.chain(85, 2, 1, True, 1000)
    g = _context(hx, cc)
    idx = (list(cc.ctxtPrimes) + list(cc.specialPrimes))[:16]
    src = [cc.primes[i] for i in idx]
    q, p, p2r, p2e = 2 ** cc.e + 1, 2, 2, 2 ** cc.ePrime
    rows = RR.synthetic_rows(src, q, p, p2r, p2e, 1, g.phim, 16)
    want = RR.prep(rows, src, src[:2], q, p, p2r, p2e, 5, 1)
    out, x, v = hx.recryptPrep(hx.DoubleCRT(g, idx, 1, data=rows), idx[:2], q, p, p2r, p2e, 5, 1, debug=True)
    assert np.array_equal(x, want[0]) and np.array_equal(v, want[1]) and np.array_equal(out.download(), want[2])
    idx17 = (list(cc.ctxtPrimes) + list(cc.specialPrimes))[:17]
    with pytest.raises(hx.HxError, match="17 rows"):
        hx.recryptPrep(hx.DoubleCRT(g, idx17, 1), idx[:2], q, p, p2r, p2e, 5, 1)


def _run_case(hx, g, case):
    """one call with the debug arrays: x, v and every output row are the restatement's, and the input is left alone"""
    a = hx.DoubleCRT(g, case.src_idx, case.B, data=case.rows)
    out, x, v = hx.recryptPrep(a, case.tgt_idx, *case.args, debug=True)
    assert np.array_equal(x, case.want[0]) and np.array_equal(v, case.want[1])
    assert np.array_equal(out.download(), case.want[2])
    assert out.getIndexSet() == case.tgt_idx and np.array_equal(a.download(), case.rows)
    return a


# more than one workgroup of 256 threads: blockIdx.x > 0, the guard of a partly idle last workgroup, the tie words of
# j >= 256, and batch element 1 in a workgroup that is not the first
@pytest.mark.parametrize("key", RR.PAST_ONE_BLOCK)
def test_kernel_past_one_block(hx, key):
    case = RR.past_one_block_case(key)
    n = case.n
    assert n == {257: 256, 341: 300, 771: 512, 1365: 576}[key[0]] and case.B == 2 and len(case.src) == 3
    assert len(case.tgt) == len(case.cc.primes)
    # a tie decides an output of batch element 1 past the first workgroup (at phi(m) = 256: in its last wave), and the
    # reference there does follow the seed
    ties = [at for at in RR.tie_positions(case) if at[0] == 1 and at[1] >= (RR.BLOCK if n > RR.BLOCK else n - 64)]
    assert ties and ties[-1][1] >= n - 2
    other = RR.past_one_block_case(key, 1)
    assert np.array_equal(other.rows, case.rows) and other.seed == case.seed + 1
    assert any(other.want[1][at] != case.want[1][at] or other.want[0][at] != case.want[0][at] for at in ties)
    g = _context(hx, case.cc)
    assert g.phim == n
    a = _run_case(hx, g, case)
    got = hx.recryptPrep(a, case.tgt_idx, *other.args, debug=True)
    assert np.array_equal(got[1], other.want[0]) and np.array_equal(got[2], other.want[1])
    assert np.array_equal(got[0].download(), other.want[2])


# every instantiation of the kernel and every case of the dispatch in hx_recrypt_prep
def test_kernel_at_every_k(hx):
    g = _context(hx, RR.sixteen_rows()[0])
    for k in RR.EVERY_K:
        case = RR.every_k_case(k)
        assert len(case.src) == k and case.B == 2 and len(case.tgt) == 2 and case.n == g.phim == 64
        try:
            _run_case(hx, g, case)
        except AssertionError as e:
            raise AssertionError("k = %d" % k) from e
    assert len({RR.every_k_case(k).seed for k in RR.EVERY_K}) == 16 and {RR.every_k_case(k).part for k in RR.EVERY_K} == {0, 1, 2}


# the edges of the range that build_plan admits, where the bounds of recrypt_core.h are stated
@pytest.mark.parametrize("which", range(len(RR.EDGES)))
def test_kernel_at_the_edges_of_the_plan(hx, which):
    g = _context(hx, RR.sixteen_rows()[0])
    for k in RR.EDGE_KS:
        case = RR.edge_case(which, k)
        if case is None:                                                 # Q shares a factor with this q: refused, and
            continue                                                     # tests/test_recryption_host.py counts these
        assert (case.p, case.q, case.p2r, case.p2e) == RR.EDGES[which] and len(case.src) == k and case.B == 2
        try:
            _run_case(hx, g, case)
        except AssertionError as e:
            raise AssertionError("k = %d" % k) from e


# ---- (b) the refusals of the C entry ----
def test_refusals(hx):
    L = hx.lib()
    cc = RR.chain(15, 2, 1)
    g = _context(hx, cc)
    small = g.add_prime(31)                                              # 31 = 1 mod 15: a prime that a q can share a factor with
    idx = list(cc.ctxtPrimes)[:3]
    q, p, p2r, p2e = 2 ** cc.e + 1, 2, 2, 2 ** cc.ePrime
    a = hx.DoubleCRT(g, idx, 2)
    mark = np.full((2, 2, g.phim), 7, dtype=np.uint64)
    out = hx.DoubleCRT(g, idx[:2], 2, data=mark)

    def call(src=a, dst=out, q=q, p=p, p2r=p2r, p2e=p2e, part=0):
        rc = L.hx_recrypt_prep(src.h if src is not None else None, dst.h if dst is not None else None, q, p, p2r, p2e, 1,
                               part, None, None)
        return rc, L.hx_last_error()
    for kw, what in ((dict(q=2 ** 12), b"gcd(q, p2r) = gcd(4096, 2) = 2"),
                     (dict(p2e=2 ** (cc.e + 1)), b"is not 1 modulo p2ePrime"),
                     (dict(q=2 ** 30 + 1), b"q = 1073741825 is not in [2, 2^30)"),
                     (dict(p2r=6), b"not powers of p = 2"),
                     (dict(dst=a), b"the output is the input"),
                     (dict(src=None), b"null argument"),
                     (dict(part=-1), b"part -1"),
                     (dict(dst=hx.DoubleCRT(g, idx[:2], 1)), b"2 batch elements, the output 1"),
                     (dict(dst=hx.DoubleCRT(g, [small], 2)), b"the output modulus 31 is not in [2^31, 2^63)"),
                     (dict(src=hx.DoubleCRT(g, [small], 2), q=93, p2e=4), b"gcd(Q mod q, q) = gcd(31, 93) = 31")):
        rc, msg = call(**kw)
        assert rc == hx.HX_ERR_INVALID and what in msg, (kw, msg)
    other = hx.Context(15)
    other.add_prime(cc.primes[0])
    rc, msg = call(dst=hx.DoubleCRT(other, [0], 2))
    assert rc == hx.HX_ERR_INVALID and b"another context" in msg
    g.graphBegin()                                                       # an open graph capture
    try:
        rc, msg = call()
        assert rc == hx.HX_ERR_INVALID and b"captured" in msg
    finally:
        try:
            g.graphEnd().destroy()
        except hx.HxError:
            pass
    assert np.array_equal(out.download(), mark)                          # a refused call touches no output
    assert call()[0] == 0 and not np.array_equal(out.download(), mark)   # and the same call with nothing wrong runs


# ---- (c) rawModSwitch of a real ciphertext ----
@pytest.mark.parametrize("key,mvec", [((57, 7, 1), (3, 19)), ((85, 2, 1), (5, 17)), ((85, 2, 2), (5, 17))])
def test_raw_mod_switch_of_a_ciphertext(hx, key, mvec):
    from helib_amd import keys as hk, powerful as PW, recryption as RC
    m, p, r = key
    cc = RR.chain(*key)
    g = _context(hx, cc)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=11)
    sk.GenSecKey()
    rc = RC.RecryptData(cc, g, mvec)
    assert (rc.e, rc.ePrime, rc.q, rc.p2ePrime) == (cc.e, cc.ePrime, p ** cc.e + 1, p ** cc.ePrime)
    ptxt = np.random.default_rng(m).integers(0, p ** r, size=g.phim)
    ct = sk.Encrypt(ptxt)
    first3 = sorted(cc.ctxtPrimes)[:3]
    ct.modDownToSet(frozenset(first3))
    assert sorted(ct.primeSet) == first3
    before = {h: part.download() for h, part in ct.parts.items()}
    (z0, z1), noise_est = RC.rawModSwitch(ct, rc, seed=99)
    src = [cc.primes[i] for i in ct.parts["1"].getIndexSet()]
    tgt_idx = sorted(cc.ctxtPrimes)
    tgt = [cc.primes[i] for i in tgt_idx]
    assert noise_est == pytest.approx(np.exp(ct.lnNoise) * rc.q / RR.product(src), rel=1e-9) and 0 < noise_est < rc.q
    conv = PW.PowerfulConversion(mvec)                                   # the numpy form: no device
    for i, (h, z) in enumerate(zip(ct.parts, (z0, z1))):
        assert np.array_equal(ct.parts[h].download(), before[h])         # the ciphertext is not affected
        coeff = ct.parts[h].copy().iFFT().download()                     # [k, 1, phi(m)]
        cube = np.stack([conv.polyToPowerful(coeff[j].astype(np.int64), s) for j, s in enumerate(src)]).astype(np.uint64)
        x, v, want = RR.prep(cube, src, tgt, rc.q, p, p ** r, rc.p2ePrime, 99, i)
        assert np.abs(x).max() <= rc.q // 2 and np.abs(x).max() > rc.q // 8           # spread over the range of q
        back = np.stack([conv.powerfulToPoly(want[j].astype(np.int64), t) for j, t in enumerate(tgt)]).astype(np.uint64)
        assert z.getIndexSet() == tgt_idx
        assert np.array_equal(z.copy().iFFT().download(), back)
    # the same behind reCrypt's check of the estimate: it passes as the ciphertext stands, and refuses, before any
    # device work, once the noise bound is raised by hand to a third of Q
    stats = {}
    zz = RC.preProcess(ct, rc, 99, stats=stats)
    assert all(np.array_equal(a.download(), b.download()) for a, b in zip(zz, (z0, z1)))
    assert stats["raw-mod-switch-noise"][0] == pytest.approx(noise_est * RC.normBnd(m) / (RC.HELIB_MIN_CAP_FRAC * p ** r *
                                                                                          cc.boundForRecryption()))
    loud = ct.clone()
    loud.lnNoise = cc.logOfProduct(ct.primeSet) - np.log(3.0)
    with pytest.raises(RC.LogicError, match="rawModSwitch scaled noise exceeds bound"):
        RC.preProcess(loud, rc, 99, stats=stats)
    assert len(stats["raw-mod-switch-noise"]) == 2 and stats["raw-mod-switch-noise"][1] > 1


# ---- (d) the whole reCrypt on the device ----
BITS = 400       # tests/test_recryption_host.py: the smallest multiple of 100 at which reCrypt holds, plus 100


@pytest.mark.parametrize("m,r", [(57, 1), (85, 1), (85, 2)])
def test_recrypt_on_the_device(hx, m, r):
    from helib_amd import ctxt as hc, keys as hk, recryption as RC
    from tests import evalmap_tables as E
    p, _, mvec, gens, ords = E.ring(m)
    cc = hc.ChainContext(m, p, r, bits=BITS, c=2, bootstrappable=True)
    g = _context(hx, cc)
    rc = RC.RecryptData(cc, g, mvec, gens=gens, ords=ords, maps=True)
    ea = rc.ea
    assert rc.ea_boot.P == p ** (cc.e - cc.ePrime + r) and ea.P == p ** r and rc.ea_boot.cc is cc
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=5)
    sk.GenSecKey()
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    hk.addFrbMatrices(sk)
    assert sk.genRecryptData(rc) == 1 and sk.recryptEkey.ptxtSpace == rc.ea_boot.P
    v = np.random.default_rng(m + r).integers(0, p ** r, size=(2, ea.size(), ea.getDegree()))
    want = v
    ct = ea.encrypt_batch(sk, v)
    while ct.bitCapacity() > 60:                                         # use the capacity up
        ct.multiplyBy(ea.encrypt_batch(sk, v))
        want = ea.mulPlain(want, v)
    if p > 2:
        ct.mulIntFactor(3)                                               # intFactor != 1: reCrypt loses and restores it
    before = ct.bitCapacity()
    assert np.array_equal(ea.decrypt_batch(ct, sk), want)
    stats = {}
    RC.reCrypt(ct, sk, rc, seed=5, stats=stats)
    assert 0 < stats["raw-mod-switch-noise"][0] <= 1
    assert ct.isCorrect() and ct.bitCapacity() > before and ct.ptxtSpace == p ** r
    assert np.array_equal(ea.decrypt_batch(ct, sk), want)                # exact, both batch elements
    ct.multiplyBy(ea.encrypt_batch(sk, v))                               # one more multiplication, and again
    want = ea.mulPlain(want, v)
    RC.reCrypt(ct, sk, rc, seed=6)
    assert ct.isCorrect() and np.array_equal(ea.decrypt_batch(ct, sk), want)
