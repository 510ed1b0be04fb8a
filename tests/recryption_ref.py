"""TEST INFRASTRUCTURE shared by tests/test_recryption_host.py and tests/test_recryption_gpu.py: the bootstrappable
chains and the rows of the tests, and the pre-processing of recryption in Python integers -- Ctxt::rawModSwitch
(src/Ctxt.cpp:2949-3049), newMakeDivisible (src/recryption.cpp:73-136) and the division by p^e', per coefficient, as
include/helib_amd.h states them for hx_recrypt_prep: divmod on big integers, nothing shared with
helib_amd/csrc/recrypt_core.h but the definition of the tie bits."""
import functools
from functools import reduce

import numpy as np

M64 = (1 << 64) - 1
TIE_DELTA, TIE_Q, TIE_DIV = 0, 1, 2


def mix(z):
    """the splitmix64 finaliser over z + 0x9E3779B97F4A7C15"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def tie_word(seed, part, b, j):
    return mix((mix((mix((mix(seed & M64) + part) & M64) + b) & M64) + j) & M64)


def tie_bit(word, which):
    return (word >> (61 + which)) & 1


def product(primes):
    return reduce(lambda a, b: a * b, primes, 1)


def centred_lift(residues, primes):
    """the integer in [-Q/2, Q/2) with these residues, as DoubleCRT::toPoly gives it"""
    Q = product(primes)
    c = 0
    for x, q in zip(residues, primes):
        Qi = Q // q
        c += int(x) * Qi * pow(Qi, -1, q)
    c %= Q
    return c - Q if c > Q // 2 else c


def prep_value(c, Q, q, p, p2r, p2e, ties):
    """one coefficient -> a dict: X, Y (after centring), delta, x0 = X + delta, x, v, w, and `hit`: which branches it
    took.  ties: a 64-bit tie word (tie_word) or a callable which -> bit."""
    bit = ties if callable(ties) else (lambda which: tie_bit(ties, which))
    hit = set()
    X, Y = divmod(c * q, Q)
    if Y > Q // 2:
        Y -= Q
        X += 1
        hit.add("Y_wrapped")
    delta = (Y % p2r) * pow(Q, -1, p2r) % p2r
    if delta > p2r // 2:
        delta -= p2r
        hit.add("delta_above_half")
    elif p2r % 2 == 0 and delta == p2r // 2:
        hit.add("delta_at_half_Y_neg" if Y < 0 else ("delta_at_half_Y_zero" if Y == 0 else "delta_at_half_Y_pos"))
        if Y < 0 or (Y == 0 and bit(TIE_DELTA)):
            delta -= p2r
    x0 = x = X + delta
    if x > q // 2:
        x -= q
        hit.add("x_above")
    elif q % 2 == 0 and x == q // 2 and bit(TIE_Q):
        x -= q
        hit.add("x_at_plus_half_taken")
    elif x < -(q // 2):
        x += q
        hit.add("x_below")
    elif q % 2 == 0 and x == -(q // 2) and bit(TIE_Q):
        x += q
        hit.add("x_at_minus_half_taken")
    if q % 2 == 0 and abs(x0) == q // 2:
        hit.add("x_at_half")
    if p2e == 1:
        v = 0
    else:
        z = x % p2e
        if z > p2e // 2:
            v = p2e - z
            hit.add("z_above_half")
        elif p == 2 and z == p2e // 2:
            hit.add("z_at_half")
            v = p2e - z if bit(TIE_DIV) else -z
        else:
            v = -z
    w, rest = divmod(x + q * v, p2e)
    assert rest == 0
    return dict(X=X, Y=Y, delta=delta, x0=x0, x=x, v=v, w=w, hit=hit)


def prep(rows, primes, targets, q, p, p2r, p2e, seed, part, hits=None):
    """rows: [k, batch, n] residues -> x, v (int64 [batch, n]) and out ([|T|, batch, n] uint64), coefficient j of batch
    element b taking tie_word(seed, part, b, j).  hits: a dict that receives {(b, j): the branches that coefficient took}"""
    rows = np.asarray(rows)
    k, B, n = rows.shape
    Q = product(primes)
    x = np.zeros((B, n), dtype=np.int64)
    v = np.zeros((B, n), dtype=np.int64)
    out = np.zeros((len(targets), B, n), dtype=np.uint64)
    for b in range(B):
        for j in range(n):
            c = centred_lift([int(rows[i, b, j]) for i in range(k)], primes)
            R = prep_value(c, Q, q, p, p2r, p2e, tie_word(seed, part, b, j))
            x[b, j], v[b, j] = R["x"], R["v"]
            if hits is not None:
                hits[b, j] = R["hit"]
            for t, qt in enumerate(targets):
                out[t, b, j] = R["w"] % qt
    return x, v, out


# ---- inputs built to take every branch ----
def _crt2(r1, m1, r2, m2):
    """the residue modulo m1 m2 (coprime) that is r1 mod m1 and r2 mod m2"""
    return (r1 + m1 * ((r2 - r1) * pow(m1, -1, m2) % m2)) % (m1 * m2)


def coefficient_for(Q, q, X, near, mod=1, res=0):
    """c with c q = Q X + Y exactly, Y = -Q X mod q, Y = res mod `mod` (coprime to q), and Y the value nearest to
    `near` on the side of zero; None when c would leave [-(Q - 1) / 2, (Q - 1) / 2]"""
    step = q * mod
    r = _crt2((-Q * X) % q, q, res % mod, mod)
    Y = near - ((near - r) % step) if near >= 0 else near + ((r - near) % step)
    if abs(Y) > (Q - 1) // 2:
        return None
    c, rest = divmod(Q * X + Y, q)
    assert rest == 0
    return c if abs(c) <= (Q - 1) // 2 else None


def branch_inputs(Q, q, p, p2r, p2e):
    """{name: c}: the coefficients the tests want, for the moduli at hand (a case that the parameters cannot reach is
    left out: the delta tie needs an even p2r, the x tie an even q, the z tie p = 2 and p2e > 1)"""
    half = (Q - 1) // 2
    out = {"c_zero": 0, "c_top": half, "c_bottom": -half}
    Qi = pow(Q, -1, p2r)
    for X in (3, -3):
        out["Y_just_below_half_X%+d" % X] = coefficient_for(Q, q, X, half)          # Y <= floor(Q/2): no wrap
        out["Y_just_above_half_X%+d" % X] = coefficient_for(Q, q, X, -half)         # Y was above Q/2 before the wrap
    if p2r % 2 == 0:
        want = (p2r // 2) * Q % p2r                                                 # delta = Y Q^-1 = p2r / 2
        assert want * Qi % p2r == p2r // 2
        out["delta_half_Y_pos"] = coefficient_for(Q, q, 5, 10 * q * p2r, p2r, want)
        out["delta_half_Y_neg"] = coefficient_for(Q, q, 5, -10 * q * p2r, p2r, want)
    if q % 2 == 0:                                                                  # delta = 0, X = +-q/2
        out["x_plus_half"] = coefficient_for(Q, q, q // 2, -half // 2, p2r, 0)
        out["x_minus_half"] = coefficient_for(Q, q, -(q // 2), half // 2, p2r, 0)
    if p == 2 and p2e > 1:                                                          # delta = 0, X = p2e/2 (+ p2e)
        out["z_half"] = coefficient_for(Q, q, p2e // 2, 10 * q * p2r, p2r, 0)
        out["z_half_neg"] = coefficient_for(Q, q, -(p2e // 2) - p2e, -10 * q * p2r, p2r, 0)
    return {k: c for k, c in out.items() if c is not None}


def replay_input(primes, targets, q, p, p2r, p2e, seed, part, rows):
    """the text tests/cpp/recrypt_core_replay.cpp reads"""
    rows = np.asarray(rows)
    k, B, n = rows.shape
    lines = ["%d %d %d %d %d %d %d %d %d %d" % (k, len(targets), B, n, q, p, p2r, p2e, seed, part),
             " ".join(map(str, primes)), " ".join(map(str, targets))]
    lines += [" ".join(str(int(x)) for x in rows[i].reshape(-1)) for i in range(k)]
    return "\n".join(lines) + "\n"


# ---- the chains and the rows of the tests ----
@functools.lru_cache(maxsize=None)
def chain(m, p, r, bootstrappable=True, bits=200):
    from helib_amd import ctxt as hc
    return hc.ChainContext(m, p, r, bits=bits, c=2, bootstrappable=bootstrappable)


def params(key, k, nt=None):
    """the moduli of one ring: the first k of (three ciphertext primes, then the special primes), the targets, q,
    p, p2r, p2e"""
    cc = chain(*key)
    m, p, r = key
    src = [cc.primes[i] for i in (list(cc.ctxtPrimes)[:3] + list(cc.specialPrimes))][:k]
    assert len(src) == k
    tgt = list(cc.primes) if nt is None else list(cc.primes)[-nt:]
    return src, tgt, p ** cc.e + 1, p, p ** r, p ** cc.ePrime


def synthetic_rows(src, q, p, p2r, p2e, B, n, seed, tail=False):
    """[k, B, n] residues: the branch-hitting coefficients first, then random words over each row's whole range.
    tail: the same coefficients once more in the last positions of the last batch element"""
    Q = product(src)
    cs = list(branch_inputs(Q, q, p, p2r, p2e).values())
    rng = np.random.default_rng(seed)
    rows = np.stack([rng.integers(0, s, size=(B, n), dtype=np.uint64) for s in src])
    flat = rows.reshape(len(src), -1)
    for pos, c in enumerate(cs[:B * n]):
        for i, s in enumerate(src):
            flat[i, pos] = c % s
    if B * n > len(cs) + 1:
        for i, s in enumerate(src):
            flat[i, len(cs)] = s - 1                                    # c = -1: the top of every row's range
    if tail:
        assert n >= 2 * len(cs) + 2                                     # (the two copies do not meet)
        for pos, c in enumerate(cs):
            for i, s in enumerate(src):
                rows[i, B - 1, n - len(cs) + pos] = c % s
    return rows


# ---- the tables of the kernel's tests, shared by the host replay and the device ----
# past one workgroup of 256 threads: phi(m) = 256 (one full block), 300 (a last block of 44 words: less than one live
# wave), 512 (two full blocks) and 576
PAST_ONE_BLOCK = [(257, 2, 1), (341, 2, 1), (771, 2, 1), (1365, 2, 1)]
BLOCK = 256                                                             # recrypt.hip's RC_T
EVERY_K = tuple(range(1, 17))
# (p, q, p2r, p2e) at the edges of what the plan admits: q and p2r just below 2^30, p2e = 1, p2e = q - 1, odd p with an
# even q, p2r = p2e = p for a 15-bit p, and the smallest q there is
EDGES = [(2, 2 ** 29 + 1, 2 ** 8, 2 ** 20), (2, 2 ** 29 + 1, 2 ** 29, 1), (2, 2 ** 29 + 1, 2, 2 ** 29),
         (3, 3 ** 18 + 1, 3 ** 5, 3 ** 10), (7, 7 ** 10 + 1, 7 ** 3, 7 ** 6), (32749, 32749 ** 2 + 1, 32749, 32749), (2, 3, 2, 2)]
EDGE_KS = (1, 4, 16)
# the branches of prep_value that the three tables take between them.  (delta_at_half_Y_zero is not in the list: Y = 0
# makes delta = Y Q^-1 = 0, so it cannot occur.)
BRANCHES = {"Y_wrapped", "delta_above_half", "delta_at_half_Y_pos", "delta_at_half_Y_neg", "x_above", "x_below",
            "x_at_plus_half_taken", "x_at_minus_half_taken", "z_above_half", "z_at_half"}


class Case:
    """one call of the kernel: the rows, the parameters and what tests/recryption_ref.py makes of them (computed once:
    nobody writes to the arrays)"""

    def __init__(self, cc, src_idx, tgt_idx, q, p, p2r, p2e, B, n, seed, part, rows_seed, tail=False):
        self.cc, self.src_idx, self.tgt_idx = cc, list(src_idx), list(tgt_idx)
        self.src, self.tgt = [cc.primes[i] for i in src_idx], [cc.primes[i] for i in tgt_idx]
        self.q, self.p, self.p2r, self.p2e, self.B, self.n, self.seed, self.part = q, p, p2r, p2e, B, n, seed, part
        self.rows = synthetic_rows(self.src, q, p, p2r, p2e, B, n, rows_seed, tail=tail)
        self.hits = {}
        self.want = prep(self.rows, self.src, self.tgt, q, p, p2r, p2e, seed, part, hits=self.hits)
        for a in (self.rows,) + self.want:
            a.setflags(write=False)

    @property
    def args(self):
        return self.q, self.p, self.p2r, self.p2e, self.seed, self.part

    def branches(self):
        return set().union(*self.hits.values())


def sixteen_rows(k=16):
    """the chain with the most rows and the indices of its first k (ciphertext primes, then special primes)"""
    cc = chain(85, 2, 1, True, 1000)
    idx = (list(cc.ctxtPrimes) + list(cc.specialPrimes))[:k]
    assert len(idx) == k
    return cc, idx


@functools.lru_cache(maxsize=None)
def past_one_block_case(key, seed_offset=0):
    """batch 2, k = 3, every prime of the chain a target; the branch inputs at the front of batch element 0 and at the end
    of batch element 1"""
    cc = chain(*key)
    m, p, r = key
    return Case(cc, list(cc.ctxtPrimes)[:3], range(len(cc.primes)), p ** cc.e + 1, p, p ** r, p ** cc.ePrime, 2, cc.phim,
                0xB10C + m + seed_offset, m % 2, m, tail=True)


def tie_positions(case):
    """the (b, j) whose output a tie bit decides"""
    return sorted(at for at, hit in case.hits.items() if hit & {"z_at_half", "x_at_half"})


@functools.lru_cache(maxsize=None)
def every_k_case(k):
    """batch 2, two targets, the seed and the part varying with k"""
    cc, idx = sixteen_rows(k)
    return Case(cc, idx, sixteen_rows(2)[1], 2 ** cc.e + 1, 2, 2, 2 ** cc.ePrime, 2, cc.phim, 0xE7E2 + 977 * k + (k << 59), k % 3,
                100 + k)


@functools.lru_cache(maxsize=None)
def edge_case(which, k):
    """EDGES[which] on the first k rows of the same chain, or None where Q shares a factor with q (the kernel refuses
    that)"""
    from math import gcd
    cc, idx = sixteen_rows(k)
    p, q, p2r, p2e = EDGES[which]
    if gcd(product(cc.primes[i] for i in idx) % q, q) != 1:
        return None
    return Case(cc, idx, sixteen_rows(2)[1], q, p, p2r, p2e, 2, cc.phim, 0xED6E + 31 * which + k, (which + k) % 2, 1000 * which + k)


# ---- the whole reCrypt over the CPU oracle backend ----
def thin_digits_plain(z, p, botHigh, r, ePrime):
    """what extractDigitsThin leaves of the integer z (mod p^(botHigh + r)) for p = 2, modulo 2^r: minus (z >> botHigh
    plus the bit below, which rounds), plus 2^e' times the r - e' lowest bits when r > e'"""
    assert p == 2
    out = -((z >> botHigh) + ((z >> (botHigh - 1)) & 1 if botHigh > 0 else 0))
    if r > ePrime:
        out += (1 << ePrime) * (z % (1 << (r - ePrime)))
    return out % (1 << r)


def recrypt_setup(m, p, r, mvec, gens, ords, bits):
    """tests/evalmap_tables.setup over a bootstrappable chain, with what the oracle backend lacks stated in python
    integers -- linComb, constantLike (as tests/test_polyeval_host.py), recryptPrep (prep above on coefficient rows) and
    the two conversions of PowerfulDCRT through toPoly and tests/powerful_ref.py -- the array over
    p^(e - e' + r) on the exact-integer encoder, RecryptData with its maps and genRecryptData.  -> (S, rc)"""
    from unittest import mock
    from oracle.backend import OPoly
    from helib_amd import ctxt as hc, recryption as RC
    from tests import evalmap_tables as E, polyeval_ref as R, powerful_ref as PR
    real = hc.ChainContext
    with mock.patch.object(hc, "ChainContext", lambda *a, **k: real(*a, bootstrappable=True, **k)):
        S = E.setup(m, p, r, gens, ords, bits)
    cc, be = S.cc, S.be
    assert cc.bootstrappable and cc.hwt == 120
    o = be.o
    S.prep_calls = []

    def recryptPrep(self, cube, out_set, q_, p_, p2r, p2e, seed, i):
        """hx_recrypt_prep on an OPoly of coefficient rows, in python integers"""
        src = [o.primes[k] for k in cube.idx]
        x, v, out = prep(cube.rows[:, None, :], src, [o.primes[k] for k in out_set], q_, p_, p2r, p2e, seed, i)
        S.prep_calls.append((i, len(cube.idx), list(out_set)))
        return OPoly(o, list(out_set), out[:, 0, :])

    def linComb(self, in0, in1, idx, w, addend=None):
        outs = []
        for k, ins in enumerate((in0, in1)):
            if ins is None:
                outs.append(None)
                continue
            rows = R.lin_comb([part.rows[:, None, :] for part in ins], [part.idx for part in ins], idx, w,
                              addend if k == 0 else None, o.primes)
            outs.append(OPoly(o, idx, rows[:, 0, :]))
        return tuple(outs)

    def constantLike(self, poly, idx, num):
        return OPoly(o, idx, np.array([[int(num) % o.primes[i]] * o.N for i in idx], dtype=np.uint64))
    ops = type(be.ops)
    ops.recryptPrep, ops.linComb, ops.constantLike = recryptPrep, linComb, constantLike
    rb = cc.e - cc.ePrime + r
    ea_boot = RC.arrayAt(cc, None, rb, encoder=E.GensEncoder(m, p, rb, gens, ords, be))

    class Cubes:
        """powerful.PowerfulDCRT's coefficientCube / fromCube on OPolys: through toPoly and the powerful basis over Z
        (tests/powerful_ref.py); an OPoly of coefficient rows holds the cube's words modulo each prime"""

        def coefficientCube(self, part):
            cube = PR.poly_to_powerful([int(x) for x in be.toPoly(part)], mvec, None)
            return OPoly(o, list(part.idx), np.array([[int(x) % o.primes[k] for x in cube] for k in part.idx], dtype=np.uint64))

        def fromCube(self, z):
            w = [centred_lift([int(z.rows[t, j]) for t in range(len(z.idx))], [o.primes[k] for k in z.idx]) for j in range(o.N)]
            d = be.fromCoeffs(list(z.idx), PR.powerful_to_poly(w, mvec, None))
            z.rows, z.batch = d.rows, 1
            return z
    rc = RC.RecryptData(cc, None, mvec, ea=S.ea, ea_boot=ea_boot, p2dConv=Cubes())
    S.sk.genRecryptData(rc)
    return S, rc
