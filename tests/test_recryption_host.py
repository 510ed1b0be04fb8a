"""Recryption on the CPU: the bootstrappable chain and setAE, the pre-processing of reCrypt (tests/recryption_ref.py in
Python integers against the definition in exact fractions, helib_amd/csrc/recrypt_core.h replayed by
tests/cpp/recrypt_core_replay.cpp under AddressSanitizer and UBSan as a stand-alone program) and the declarations.
Then helib_amd.recryption over the CPU oracle backend: extractDigitsThin (both branches) and extractDigitsPacked against
a restatement on slot values, and the whole reCrypt with the per-part pre-processing stated in Python integers.
Everything here is an integer: every comparison is exact.  No GPU.

The chain: on this code reCrypt holds (the decryption is the plaintext, isCorrect(), the capacity grows, a second
reCrypt after one more multiplication decrypts) from bits = 300 on, the smallest multiple of 100, at (57, 7, 1),
(85, 2, 1) and (85, 2, 2); at 200 the check of rawModSwitch's noise estimate refuses.  The tests here run at 300,
tests/test_recryption_gpu.py at 400."""
import functools
import math
import os
import random
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

from tests import recryption_ref as RR
from tests.recryption_ref import chain, params, synthetic_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "recrypt_core_replay.cpp")

# (m, p, r) -> (e, e') with skHwt = 120, scale = 10: RecryptData::setAE (src/recryption.cpp:200-256) transcribed
AE = {(57, 7, 1): (4, 1), (85, 2, 1): (13, 6), (85, 2, 2): (14, 7), (105, 2, 1): (14, 7), (21845, 2, 1): (12, 4)}


# ---- (a) the chain ----
@pytest.mark.parametrize("key", sorted(AE))
def test_setAE_gives_the_table(key):
    cc = chain(*key)
    assert (cc.e, cc.ePrime) == AE[key]
    assert cc.hwt == 120 and cc.bootstrappable
    assert cc.p ** cc.e + 1 < 1 << 30 and cc.e > cc.ePrime >= 1 and cc.e > cc.r


def test_bound_for_recryption_is_the_reference_formula():
    cc = chain(105, 2, 1)                                               # 105 = 3 * 5 * 7: three prime factors
    sd = math.sqrt(48 / 105 * 120 * 8 / 3.0) * 0.5
    assert cc.stdDevForRecryption() == sd and cc.boundForRecryption() == 0.5 + 10.0 * sd
    assert chain(21845, 2, 1).stdDevForRecryption() == math.sqrt(16384 / 21845 * 120 * 8 / 3.0) * 0.5    # 5 * 17 * 257


@pytest.mark.parametrize("key", [(57, 7, 1), (85, 2, 2)])
def test_special_primes_follow_p2e(key):
    """Context::addSpecialPrimes (src/Context.cpp:874-1035) with p2e = p^r p^(e - e'): the number and the size of the
    special primes from the formula, restated here"""
    from helib_amd import ctxt as hc, hostnt
    cc = chain(*key)
    m, p, r = key
    p2e = p ** r * p ** (cc.e - cc.ePrime)
    maxDigitLog = max(cc.logOfProduct(d) for d in cc.digits)
    log_phim = max(math.log(cc.phim), 1.0)
    nBits = (maxDigitLog + math.log(m) + math.log(p2e) + math.log(cc.stdev) + 0.5 * math.log(12.0) + math.log(len(cc.digits))
             - 0.5 * log_phim - 0.5 * math.log(log_phim) - 2 * math.log(p) - math.log(120)) / math.log(2.0)
    bit_loss = cc._bit_loss()
    nPrimes = int(math.ceil(nBits / (hc.HELIB_SP_NBITS - bit_loss)))
    t = hc.HELIB_SP_NBITS
    while (t - 1) >= 0.55 * hc.HELIB_SP_NBITS and (t - 1) >= 30 and ((t - 1) - bit_loss) * nPrimes >= nBits:
        t -= 1
    assert len(cc.specialPrimes) == nPrimes
    for i in cc.specialPrimes:
        q = cc.primes[i]
        assert hostnt.is_prime(q) and (q - 1) % m == 0 and t - 1 < math.log2(q) < t
    # the same chain without the flag has smaller (or fewer) special primes: the flag does change p2e
    plain = chain(m, p, r, False)
    assert cc.logOfProduct(cc.specialPrimes) > plain.logOfProduct(plain.specialPrimes)


# the chains of the commit before this feature, recorded from its ChainContext: (primes, specialPrimes, digits)
BEFORE = [
    (dict(m=85, p=2, r=1, bits=200, c=2),
     ([65598914561, 60251176961, 3856075325441, 31761283153921, 262851998515201, 1985992877670401, 17383278835138561,
       15841213777182721, 17243091102597121, 16285141596897281, 34018889763389441, 33738514298306561], [10, 11], [[6, 7], [8, 9]])),
    (dict(m=57, p=7, r=2, bits=150, c=3, skHwt=64),
     ([60246982657, 67419242497, 3886408531969, 32804960206849, 251667903676417, 1989841168367617, 16482778811990017,
       17234844765388801, 16075409753899009, 67685935805890561], [9], [[6], [7], [8]])),
]


@pytest.mark.parametrize("args,before", BEFORE)
def test_a_chain_without_the_flag_is_what_it_was(args, before):
    from helib_amd import ctxt as hc
    a, b = hc.ChainContext(**args), hc.ChainContext(bootstrappable=False, **args)
    assert (a.primes, a.specialPrimes, a.digits) == before
    assert a.primes == b.primes and a.specialPrimes == b.specialPrimes and a.digits == b.digits
    assert (a.e, a.ePrime, a.bootstrappable, a.hwt) == (0, 0, False, args.get("skHwt", 0))
    ck = hc.ChainContext(m=64, p=-1, r=8, bits=100, c=2, ckks=True)
    cb = hc.ChainContext(m=64, p=-1, r=8, bits=100, c=2, ckks=True, bootstrappable=True)      # ignored for CKKS
    assert ck.primes == cb.primes and not cb.bootstrappable and cb.hwt == 0


# ---- (b) the pre-processing in Python integers against the definition ----
RINGS = [(57, 7, 1), (85, 2, 1), (85, 2, 2)]


def check_definition(c, Q, q, p, p2r, p2e, R):
    x0, x, v, w = R["x0"], R["x"], R["v"], R["w"]
    assert abs(Fraction(c * q, Q) - x0) <= Fraction(p2r, 2)            # the rounding error is at most p^r / 2
    assert (x0 * Q - c * q) % p2r == 0                                  # x0 = c q Q^-1 mod p^r
    assert (x - x0) % q == 0 and 2 * abs(x) <= q                        # the symmetric reduction modulo q
    assert 2 * abs(v) <= p2e and (x + q * v) % p2e == 0 and w * p2e == x + q * v
    if p2e == 1:
        assert v == 0


@pytest.mark.parametrize("key", RINGS)
@pytest.mark.parametrize("k", [1, 3, 5])
def test_ref_prep_is_the_definition(key, k):
    src, _, q, p, p2r, p2e = params(key, k)
    Q = RR.product(src)
    rng = random.Random(k * 1000 + key[0])
    for e in (p2e, 1):
        for i in range(300):
            c = rng.randrange(-(Q - 1) // 2, (Q - 1) // 2 + 1)
            assert RR.centred_lift([c % s for s in src], src) == c
            check_definition(c, Q, q, p, p2r, e, RR.prep_value(c, Q, q, p, p2r, e, rng.getrandbits(64)))


@pytest.mark.parametrize("key", RINGS)
@pytest.mark.parametrize("k", [1, 3, 5])
def test_ref_prep_on_inputs_built_for_every_branch(key, k):
    src, _, q, p, p2r, p2e = params(key, k)
    Q = RR.product(src)
    ins = RR.branch_inputs(Q, q, p, p2r, p2e)
    want = {"c_zero", "c_top", "c_bottom", "Y_just_below_half_X+3", "Y_just_below_half_X-3", "Y_just_above_half_X+3",
            "Y_just_above_half_X-3"}
    want |= {"delta_half_Y_pos", "delta_half_Y_neg", "z_half", "z_half_neg"} if p == 2 else {"x_plus_half", "x_minus_half"}
    assert set(ins) == want
    got = {}
    for name, c in ins.items():
        assert abs(c) <= (Q - 1) // 2
        for ties in (lambda which: 0, lambda which: 1):
            R = RR.prep_value(c, Q, q, p, p2r, p2e, ties)
            check_definition(c, Q, q, p, p2r, p2e, R)
            got[name, ties(0)] = R
    half = (Q - 1) // 2
    for t in (0, 1):
        assert got["c_zero", t]["x"] == 0 and got["c_zero", t]["w"] == 0
        assert 2 * abs(got["c_top", t]["x0"]) >= q - 2 * p2r and 2 * abs(got["c_bottom", t]["x0"]) >= q - 2 * p2r
        for X in (3, -3):
            lo, hi = got["Y_just_below_half_X%+d" % X, t], got["Y_just_above_half_X%+d" % X, t]
            assert "Y_wrapped" not in lo["hit"] and lo["X"] == X and half - lo["Y"] < q * p2r
            assert "Y_wrapped" in hi["hit"] and hi["X"] == X and hi["Y"] + half < q * p2r
        if p == 2:
            assert "delta_at_half_Y_pos" in got["delta_half_Y_pos", t]["hit"] and got["delta_half_Y_pos", t]["delta"] == p2r // 2
            assert "delta_at_half_Y_neg" in got["delta_half_Y_neg", t]["hit"] and got["delta_half_Y_neg", t]["delta"] == -(p2r // 2)
            for name in ("z_half", "z_half_neg"):
                assert "z_at_half" in got[name, t]["hit"]
                assert got[name, t]["v"] == (p2e // 2 if t else -(p2e // 2))           # the tie bit decides
        else:
            assert q % 2 == 0
            for name, sign in (("x_plus_half", 1), ("x_minus_half", -1)):
                assert "x_at_half" in got[name, t]["hit"] and got[name, t]["x0"] == sign * (q // 2)
                assert got[name, t]["x"] == (-sign if t else sign) * (q // 2)         # the tie bit decides


def test_tie_bits_are_reproducible_and_balanced():
    words = [RR.tie_word(7, part, b, j) for part in range(2) for b in range(3) for j in range(500)]
    assert words == [RR.tie_word(7, part, b, j) for part in range(2) for b in range(3) for j in range(500)]
    assert len(set(words)) == len(words) and RR.tie_word(8, 0, 0, 0) != RR.tie_word(7, 0, 0, 0)
    for which in range(3):
        ones = sum(RR.tie_bit(w, which) for w in words)
        assert abs(ones - 1500) < 5 * math.sqrt(3000) / 2               # five standard deviations of a fair coin
    assert RR.mix(0) == 0xE220A8397B1DCDAF                              # splitmix64's first output from state 0


# ---- (c) recrypt_core.h replayed, under the sanitizers, as a stand-alone program ----
@functools.lru_cache(maxsize=None)
def _exe():
    exe = os.path.join(tempfile.mkdtemp(prefix="recrypt_replay_"), "recrypt_core_replay")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    return exe


def replay(src, tgt, q, p, p2r, p2e, seed, part, rows):
    r = subprocess.run([_exe()], input=RR.replay_input(src, tgt, q, p, p2r, p2e, seed, part, rows), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr               # it ends clean: no sanitizer report
    lines = r.stdout.splitlines()
    if lines[0] != "ok":
        return lines[0]
    B = np.asarray(rows).shape[1]
    body = [[int(x) for x in line.split()] for line in lines[1:]]
    return (np.array(body[:B], dtype=np.int64), np.array(body[B:2 * B], dtype=np.int64),
            np.array(body[2 * B:], dtype=np.uint64).reshape(len(tgt), B, -1))


@pytest.mark.parametrize("key", RINGS)
@pytest.mark.parametrize("k", [1, 3, 5])
def test_the_core_header_replays_the_reference_word_for_word(key, k):
    for nt, B, e_one in ((1, 1, False), (None, 3, False), (1, 3, True)):
        src, tgt, q, p, p2r, p2e = params(key, k, nt)
        if e_one:
            p2e = 1
        rows = synthetic_rows(src, q, p, p2r, p2e, B, 24, key[0] + k)
        want = RR.prep(rows, src, tgt, q, p, p2r, p2e, 0xC0FFEE + k, k % 2)
        got = replay(src, tgt, q, p, p2r, p2e, 0xC0FFEE + k, k % 2, rows)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w)


def test_the_core_header_takes_sixteen_rows():
    """the largest k: sixteen 50-odd-bit primes"""
    cc = chain(85, 2, 1, True, 1000)
    src = [cc.primes[i] for i in list(cc.ctxtPrimes) + list(cc.specialPrimes)][:16]
    assert len(src) == 16
    q, p, p2r, p2e = 2 ** cc.e + 1, 2, 2, 2 ** cc.ePrime
    rows = synthetic_rows(src, q, p, p2r, p2e, 1, 24, 16)
    want = RR.prep(rows, src, src[:2], q, p, p2r, p2e, 5, 1)
    for g, w in zip(replay(src, src[:2], q, p, p2r, p2e, 5, 1, rows), want):
        assert np.array_equal(g, w)


def _replay_case(case):
    got = replay(case.src, case.tgt, *case.args, case.rows)
    assert not isinstance(got, str), got
    for g, w in zip(got, case.want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


# the tables of tests/test_recryption_gpu.py, word for word through the same header
@pytest.mark.parametrize("key", RR.PAST_ONE_BLOCK)
def test_the_core_header_replays_the_rows_past_one_block(key):
    case = RR.past_one_block_case(key)
    assert case.n >= RR.BLOCK and case.B == 2
    _replay_case(case)
    _replay_case(RR.past_one_block_case(key, 1))                        # the other seed


def test_the_core_header_replays_every_k():
    for k in RR.EVERY_K:
        case = RR.every_k_case(k)
        assert len(case.src) == k
        _replay_case(case)


@pytest.mark.parametrize("which", range(len(RR.EDGES)))
def test_the_core_header_replays_the_edges_of_the_plan(which):
    p, q, p2r, p2e = RR.EDGES[which]
    assert q < 1 << 30 and p2r < 1 << 30 and (q - 1) % p2e == 0 and math.gcd(q, p2r) == 1
    for k in RR.EDGE_KS:
        case = RR.edge_case(which, k)
        if case is not None:
            _replay_case(case)
        else:                                                            # the plan refuses it, with the figures
            cc, idx = RR.sixteen_rows(k)
            src = [cc.primes[i] for i in idx]
            out = replay(src, src[:1], q, p, p2r, p2e, 1, 0, np.zeros((k, 1, 2), dtype=np.uint64))
            assert isinstance(out, str) and "gcd(Q mod q, q)" in out


def test_the_tables_take_every_branch():
    """which branches of the per-coefficient arithmetic the inputs of the three tables reach, stated, not hoped for"""
    cases = [RR.past_one_block_case(key) for key in RR.PAST_ONE_BLOCK] + [RR.every_k_case(k) for k in RR.EVERY_K]
    edges = [RR.edge_case(which, k) for which in range(len(RR.EDGES)) for k in RR.EDGE_KS]
    assert len(edges) == 21 and sum(c is None for c in edges) <= 1      # at most one (parameter set, k) is refused
    taken = set().union(*(c.branches() for c in cases + edges if c is not None))
    assert RR.BRANCHES <= taken, sorted(RR.BRANCHES - taken)
    assert "delta_at_half_Y_zero" not in taken                          # Y = 0 makes delta = 0
    # at the edges: q = 2^29 + 1 with p2r = 2^29 and p2e = 2^29 spread x and v over 30 bits, so |q v| nears 2^58
    big = RR.edge_case(2, 16)
    assert int(np.abs(big.want[0]).max()) > 2 ** 27 and int(np.abs(big.want[1]).max()) * big.q > 2 ** 56
    # past one block, a tie decides an output of batch element 1 at j >= 256 wherever the row is that long
    for key in RR.PAST_ONE_BLOCK:
        case = RR.past_one_block_case(key)
        ties = [at for at in RR.tie_positions(case) if at[0] == 1 and at[1] >= RR.BLOCK]
        assert bool(ties) == (case.n > RR.BLOCK), key
        if ties:
            other = RR.past_one_block_case(key, 1)
            assert any(other.want[1][at] != case.want[1][at] or other.want[0][at] != case.want[0][at] for at in ties), key


def test_the_plan_refuses_with_the_figures():
    src, tgt, q, p, p2r, p2e = params((85, 2, 1), 3, 1)
    rows = np.zeros((3, 1, 2), dtype=np.uint64)

    def why(**kw):
        a = dict(src=src, tgt=tgt, q=q, p=p, p2r=p2r, p2e=p2e)
        a.update(kw)
        out = replay(a["src"], a["tgt"], a["q"], a["p"], a["p2r"], a["p2e"], 1, 0, rows[:len(a["src"])])
        assert isinstance(out, str) and out.startswith("refused: "), out
        return out
    assert "gcd(q, p2r) = gcd(8192, 2) = 2" in why(q=8192)
    assert "q = 8193 is not 1 modulo p2ePrime = 16384" in why(p2e=16384)
    assert "gcd(Q mod q, q) = gcd(3, 9) = 3" in why(q=9, p2e=2, src=[3 * 1000003])    # (any odd moduli replay)
    assert "q = 1073741825 is not in [2, 2^30)" in why(q=2 ** 30 + 1)
    assert "not powers of p = 2" in why(p2r=6)
    assert "the output modulus 31 is not in [2^31, 2^63)" in why(tgt=[31])
    big = chain(85, 2, 1, True, 1000)
    seventeen = [big.primes[i] for i in list(big.ctxtPrimes) + list(big.specialPrimes)][:17]
    assert len(seventeen) == 17
    assert "17 rows" in replay(seventeen, tgt, q, p, p2r, p2e, 1, 0, np.zeros((17, 1, 2), dtype=np.uint64))


# ---- (d) helib_amd.recryption on the host ----
def test_noise_check_raises_as_the_reference():
    from helib_amd import recryption as RC
    cc = RR.chain(85, 2, 1)
    bound = RC.HELIB_MIN_CAP_FRAC * 2 * cc.boundForRecryption()
    stats = {}
    assert RC.checkNoise(cc, 0.5 * bound, 2, 1.0, stats) == pytest.approx(0.5)
    with pytest.raises(RC.LogicError, match="rawModSwitch scaled noise exceeds bound: 2.0"):
        RC.checkNoise(cc, bound, 2, 2.0, stats)
    assert [round(x, 9) for x in stats["raw-mod-switch-noise"]] == [0.5, 2.0]


def test_reduce_ptxt_space():
    from helib_amd import ctxt as hc
    ct = hc.Ctxt(chain(57, 7, 2, False), None)
    ct.ptxtSpace, ct.intFactor = 49, 40
    assert ct.reducePtxtSpace(7 ** 3) is ct and (ct.ptxtSpace, ct.intFactor) == (49, 40)
    ct.reducePtxtSpace(7)
    assert (ct.ptxtSpace, ct.intFactor) == (7, 5)
    with pytest.raises(RuntimeError, match="coprime"):
        ct.reducePtxtSpace(2)


def test_the_noise_check_on_a_ciphertext_whose_bound_was_raised_by_hand():
    """reCrypt's check (src/recryption.cpp:443-463) sits in front of the device work in preProcess, so a ciphertext
    that is refused needs no parts"""
    from helib_amd import ctxt as hc, recryption as RC
    cc = chain(85, 2, 1)
    rc = RC.RecryptData(cc, None, (5, 17))
    ct = hc.Ctxt(cc, None)
    ct.primeSet = frozenset(sorted(cc.ctxtPrimes)[:3])
    bound = RC.HELIB_MIN_CAP_FRAC * 2 * cc.boundForRecryption() / RC.normBnd(85)     # on noise q / Q
    ct.lnNoise = math.log(2.0 * bound) + cc.logOfProduct(ct.primeSet) - math.log(rc.q)
    stats = {}
    with pytest.raises(RC.LogicError, match="rawModSwitch scaled noise exceeds bound: 2.0"):
        RC.preProcess(ct, rc, 1, stats=stats)
    assert stats["raw-mod-switch-noise"] == [pytest.approx(2.0)]
    ct.lnNoise -= math.log(4.0)                                                       # half the bound: the check passes
    with pytest.raises(RC.LogicError, match="without a device context"):             # and the device work is next
        RC.preProcess(ct, rc, 1, stats=stats)
    assert stats["raw-mod-switch-noise"][1] == pytest.approx(0.5)


def test_recrypt_data_holds_the_parameters():
    from helib_amd import recryption as RC
    with pytest.raises(RC.LogicError, match="bootstrappable=True"):
        RC.RecryptData(chain(85, 2, 1, False), None, (5, 17))
    with pytest.raises(RC.LogicError, match="Cyclotomic polynomial mismatch"):
        RC.RecryptData(chain(85, 2, 1), None, (5, 19))
    rc = RC.RecryptData(chain(85, 2, 2), None, (5, 17))
    assert (rc.e, rc.ePrime, rc.q, rc.p2ePrime, rc.p2r, rc.skHwt) == (14, 7, 2 ** 14 + 1, 2 ** 7, 4, 120)
    with pytest.raises(RC.LogicError, match="without a device context"):
        RC.rawModSwitch(None, rc, 1)
    assert RC.normBnd(85) == pytest.approx(2 / math.tan(math.pi / 10) / 5 * 2 / math.tan(math.pi / 34) / 17, rel=1e-15)
    assert RC.normBnd(64) == pytest.approx(1.0, rel=1e-15)              # 2 cot(pi / 4) / 2
    from helib_amd import evalmap                                       # the old module keeps refusing as it did
    with pytest.raises(evalmap.LogicError, match="are the pieces in the tree"):
        evalmap.reCrypt()


# ---- (e) the digit extractions over the oracle backend, m = 85 ----
@pytest.mark.parametrize("botHigh,r,ePrime,force,chen_han", [(3, 1, 2, 0, False), (2, 2, 1, 0, True), (2, 2, 1, -1, False),
                                                             (2, 2, 1, 1, True), (2, 3, 1, 0, False)])
def test_extract_digits_thin(botHigh, r, ePrime, force, chen_han):
    """both branches; the cost rule picks the basic one at r = 1, Chen and Han's at r = 2 and the basic one with its
    free bit at r = 3 (src/recryption.cpp:806-832, 875-876)"""
    from helib_amd import recryption as RC
    from tests.test_polyeval_host import _setup
    s = _setup(85, 2, botHigh + r, bits=300)
    assert RC.useChenHan(2, botHigh, r) is (chen_han if force == 0 else r == 2)
    z = s.slots(5)[0]
    ct = s.ea.encrypt(s.sk, z)
    assert RC.extractDigitsThin(s.ea, ct, botHigh, r, ePrime, force_chen_han=force) is ct
    assert ct.ptxtSpace == 2 ** r and ct.isCorrect() and ct.bitCapacity() > 0
    want = [RR.thin_digits_plain(int(x), 2, botHigh, r, ePrime) for x in np.asarray(z).reshape(-1)]
    assert [int(x) for x in np.asarray(s.ea.decrypt(ct, s.sk)).reshape(-1)] == want


BITS_MIN = 300       # see the module docstring


@functools.lru_cache(maxsize=None)
def recrypt_ring(m, r):
    from tests import evalmap_tables as E
    p, _, mvec, gens, ords = E.ring(m)
    return RR.recrypt_setup(m, p, r, mvec, gens, ords, BITS_MIN)


def test_extract_digits_packed():
    from helib_amd import intraslot, recryption as RC
    S, rc = recrypt_ring(85, 1)
    eb, ea = rc.ea_boot, rc.ea
    n, d, Pb = eb.size(), eb.getDegree(), eb.P
    assert (d, Pb, ea.P) == (8, 2 ** 8, 2) and len(rc.unpackSlotEncoding) == d
    a = np.random.default_rng(8).integers(0, Pb, size=(1, n, d))
    ct = S.sk.skEncrypt([int(x) % Pb for x in eb.enc.coeffs(a)[0]], Pb)
    assert np.array_equal(eb.decrypt_batch(ct, S.sk), a)
    RC.extractDigitsPacked(rc, ct, rc.e - rc.ePrime, rc.r, rc.ePrime)
    coords = intraslot.unpackPlain(eb, a)[0]                            # [n, d]: the normal-basis coordinates of every slot
    want = np.array([[RR.thin_digits_plain(int(c), 2, rc.e - rc.ePrime, rc.r, rc.ePrime) for c in row] for row in coords])
    assert ct.ptxtSpace == 2 and ct.isCorrect()
    assert np.array_equal(ea.decrypt_batch(ct, S.sk)[0], want)          # coordinate i became the coefficient of X^i


# ---- (f) the whole reCrypt over the oracle backend ----
@pytest.mark.parametrize("m,r", [(57, 1), (85, 1), (85, 2)])
def test_recrypt_over_the_oracle_backend(m, r):
    from helib_amd import recryption as RC, timing
    S, rc = recrypt_ring(m, r)
    ea, sk = S.ea, S.sk
    assert sk.recryptKeyID == 1 and (1, 1, 0, 1) in sk.keySwitchingTo and (1, 1) not in sk.keySwitching
    assert sk.recryptEkey.ptxtSpace == rc.p ** (rc.e - rc.ePrime + rc.r)
    v = S.slots(1)
    want = v
    ct = ea.encrypt(sk, v)
    while ct.bitCapacity() > 60:                                         # use the capacity up
        ct.multiplyBy(ea.encrypt(sk, v))
        want = ea.mulPlain(want, v)
    if m == 57:
        ct.mulIntFactor(3)                                               # intFactor != 1: reCrypt loses and restores it
        assert ct.intFactor != 1
    before = ct.bitCapacity()
    assert np.array_equal(ea.decrypt_batch(ct, sk), want)
    timing.resetAllTimers()
    stats = {}
    assert RC.reCrypt(ct, sk, rc, seed=5, stats=stats) is ct
    assert [c[0] for c in S.prep_calls[-2:]] == [0, 1] and all(c[1] <= 3 + len(S.cc.specialPrimes) for c in S.prep_calls)
    assert 0 < stats["raw-mod-switch-noise"][0] <= 1
    for name in ("AAA_preProcess", "AAA_LinearTransform1", "AAA_extractDigitsPacked", "AAA_LinearTransform2", "unpack", "repack"):
        assert timing.getTimerByName(name).numCalls == 1, name
    assert ct.isCorrect() and ct.bitCapacity() > before and ct.ptxtSpace == rc.p2r
    assert np.array_equal(ea.decrypt_batch(ct, sk), want)
    ct.multiplyBy(ea.encrypt(sk, v))                                     # one more multiplication, and again
    want = ea.mulPlain(want, v)
    RC.reCrypt(ct, sk, rc, seed=6)
    assert ct.isCorrect() and np.array_equal(ea.decrypt_batch(ct, sk), want)


def test_recrypt_refusals():
    from helib_amd import recryption as RC
    S, rc = recrypt_ring(85, 1)
    ct = S.ea.encrypt(S.sk, S.slots(2))
    with pytest.raises(RC.LogicError, match="holds no maps"):
        RC.reCrypt(ct, S.sk, RC.RecryptData(S.cc, None, rc.mvec))
    loud = ct.clone()
    loud.lnNoise = S.cc.logOfProduct(ct.primeSet) - math.log(3.0)       # the noise bound raised by hand, to Q / 3
    with pytest.raises(RC.LogicError, match="rawModSwitch scaled noise exceeds bound"):
        RC.reCrypt(loud, S.sk, rc, seed=1)
    sk2 = type(S.sk)(S.cc, S.be, seed=9)
    sk2.GenSecKey()
    with pytest.raises(RC.LogicError, match="No bootstrapping data"):
        RC.reCrypt(ct, sk2, rc)
    with pytest.raises(RuntimeError, match="non-bootstrappable"):
        type(S.sk)(chain(85, 2, 1, False), S.be, seed=9).genRecryptData(rc)


# ---- (z) declarations ----
def test_symbol_is_declared_bound_listed_and_exported():
    from helib_amd import build, capi
    header = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    so = build.build()
    dyn = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    lib = capi.lib()
    assert re.search(r"\bint hx_recrypt_prep\(", header)
    assert "hx_recrypt_prep" in capi.SYMBOLS
    assert re.search(r" T hx_recrypt_prep$", dyn, re.M)
    assert len(lib.hx_recrypt_prep.argtypes) == 10
    for cite in ("src/Ctxt.cpp:2949-3049", "src/recryption.cpp:73-136", "src/recryption.cpp:367-545"):
        assert cite in header, cite
    text = subprocess.run(["nm", "-C", so], capture_output=True, text=True, check=True).stdout
    assert "recrypt_prep_kernel" in text
