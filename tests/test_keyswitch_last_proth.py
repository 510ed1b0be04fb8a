"""The Montgomery store loop of the fused key switch on rows of Proth-form primes (helib_amd/csrc/ks_proth.h,
ntt_kernels.hip KsLastIO::store_rows, engine.hip ksk_build_mont).

CPU: the loop's per-coefficient functions replayed under HX_CHECK_BOUNDS (tests/cpp/ks_proth_store_replay.cpp: the
kernel's slot order, masks and constants) against python integers, for D = 2, 3, 4, every owner and the special rows,
on every prime of the bits = 950 chain at m = 32768 and of the CKKS m = 65536 chain; and the key conversion k 2^64 mod q.
GPU: the fused route against its twin (a context created under HX_NO_KS_LAST_FUSE=1, which neither builds nor reads the
Montgomery-form key rows) word for word, and both against the oracle's Ctxt::reLinearize; the in-situ profiler's kernel
names prove which route ran (the pattern of tests/test_keyswitch_last_fused.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_KERNEL = "ntt_keyswitch_last_kernel"


# ---------------------------------------------------------------- CPU: the replay
@pytest.fixture(scope="module")
def replay():
    src = os.path.join(ROOT, "tests", "cpp", "ks_proth_store_replay.cpp")
    so = os.path.join(ROOT, "tests", "cpp", "libks_proth_store_replay.so")
    hdrs = [os.path.join(ROOT, "helib_amd", "csrc", h) for h in ("ks_proth.h", "ntt_core.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DHX_CHECK_BOUNDS", "-shared", "-fPIC", "-o", so, src])
    L = C.CDLL(so)
    L.ks_proth_store_replay.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int] + [C.c_void_p] * 8 + [
        C.c_uint64, C.c_void_p, C.c_void_p]
    L.ks_proth_fused_bound.argtypes = [C.c_int]
    L.ks_proth_key_to_mont.argtypes = [C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    return L


def bgv950_chain():
    """bits = 950 at m = 32768: 16 ctxt primes of 60 bits, 6 special primes of 56 bits (bench.py bgv32768)."""
    g60, g56 = O.PrimeGen(60, 32768), O.PrimeGen(56, 32768)
    return 14, [g60.next() for _ in range(16)] + [g56.next() for _ in range(6)]


def ckks65536_chain():
    """bits = 1400 at m = 65536: 24 + 8 primes of 59 bits (bench.py ckks65536)."""
    g = O.PrimeGen(59, 65536)
    return 15, [g.next() for _ in range(32)]


NRAND = 24


def words(rng, q, extremes, n):
    """n canonical words: the extremes first, then random ones."""
    x = rng.integers(0, q, n, dtype=np.uint64)
    x[:len(extremes)] = extremes
    return x


def replay_row(L, logn, nd, owner, q, rng, has_s, scaled):
    """One row of the store loop on n coefficients; returns nothing, asserts every output word."""
    B = L.ks_proth_fused_bound(logn)
    assert 8 <= B <= 16
    fd = nd - 2 if owner == nd - 1 else nd - 1
    # coefficient 0: everything at its largest (the fused word at B q - 1); 1: everything zero; 2, 3: mixed; then random
    hi, lo = q - 1, 0
    n = NRAND + 4
    dig = np.stack([words(rng, q, [hi, lo, hi, lo], n) for _ in range(nd)])
    lazy = rng.integers(0, B, n, dtype=np.uint64)
    lazy[:4] = [B - 1, 0, 0, B - 1]
    vf = dig[fd] + lazy * np.uint64(q)
    assert int(vf[0]) == B * q - 1
    own_src = words(rng, q, [hi, lo, lo, hi], n)
    acc0, acc1 = words(rng, q, [hi, lo, hi, lo], n), words(rng, q, [hi, lo, lo, hi], n)
    kb = np.stack([words(rng, q, [hi, lo, hi, 1], n) for _ in range(nd)])
    ka = np.stack([words(rng, q, [hi, lo, 1, hi], n) for _ in range(nd)])
    pe = [int(rng.integers(1, q)) for _ in range(nd - 1)]
    pinv = np.array([pow(p, -1, q) for p in pe], dtype=np.uint64)
    ps = 0 if scaled else int(rng.integers(1, q))
    o0, o1 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    rc = L.ks_proth_store_replay(logn, nd, owner, q, n, dig.ctypes.data, vf.ctypes.data, own_src.ctypes.data,
                                 acc0.ctypes.data, acc1.ctypes.data if has_s else None, kb.ctypes.data, ka.ctypes.data,
                                 pinv.ctypes.data, ps, o0.ctypes.data, o1.ctypes.data)
    assert rc == 0
    for i in range(n):
        d = [int(dig[e, i]) for e in range(nd)]
        w0 = w1 = 0
        if owner >= 0:
            own = int(own_src[i])
            for e in range(owner):
                own = (own - d[e]) * int(pinv[e]) % q
            d[owner] = own
            f = ps if ps else 1
            w0 = int(acc0[i]) * f
            w1 = int(acc1[i]) * f if has_s else 0
        w0 = (w0 + sum(d[e] * int(kb[e, i]) for e in range(nd))) % q
        w1 = (w1 + sum(d[e] * int(ka[e, i]) for e in range(nd))) % q
        assert (int(o0[i]), int(o1[i])) == (w0, w1), (logn, nd, owner, q, i)


@pytest.mark.parametrize("chain", [bgv950_chain, ckks65536_chain], ids=["bgv32768_bits950", "ckks65536"])
def test_proth_store_loop_replayed_against_python_integers(replay, chain):
    """Every prime of the chain; D = 2, 3, 4; owned rows with every owner and special rows; with and without the (s)
    part; the parts unscaled and already scaled.  The replay aborts the process if a bound assertion fires."""
    logn, primes = chain()
    rng = np.random.default_rng(logn)
    for q in primes:
        assert q % (1 << 32) == 1 and q < (1 << 60)
        for nd in (2, 3, 4):
            for owner in range(-1, nd):
                replay_row(replay, logn, nd, owner, q, rng, True, False)
            replay_row(replay, logn, nd, nd - 1, q, rng, False, False)     # no (s) part
            replay_row(replay, logn, nd, 0, q, rng, True, True)            # the parts stand scaled
    # N = 2^13 (the GPU cases' ring) has a bound of its own
    q13 = O.PrimeGen(60, 16384).next()
    for nd in (2, 3, 4):
        for owner in range(-1, nd):
            replay_row(replay, 13, nd, owner, q13, rng, True, False)


def test_key_rows_converted_to_montgomery_form(replay):
    """k 2^64 mod q, canonical, for the same primes (what ksk_mont_kernel stores beside the plain key rows)."""
    rng = np.random.default_rng(64)
    for q in bgv950_chain()[1] + ckks65536_chain()[1]:
        k = words(rng, q, [0, 1, q - 1, q // 2], 40)
        out = np.zeros_like(k)
        assert replay.ks_proth_key_to_mont(q, len(k), k.ctypes.data, out.ctypes.data) == 0
        assert [int(x) for x in out] == [(int(x) << 64) % q for x in k]
    q36 = O.PrimeGen(36, 16384).next()
    assert q36 % (1 << 32) != 1
    assert replay.ks_proth_key_to_mont(q36, 0, None, None) == -2


# ---------------------------------------------------------------- GPU: parity
@pytest.fixture(scope="module")
def hx():
    try:
        import torch  # noqa: F401  (before the library touches the device: tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import capi
    if capi.device_count() <= 0:
        pytest.skip("no HIP device: the GPU parity tests run on an MI355X (pytest -m gpu)")
    return capi


class Pair:
    """A device context and an oracle context with the same primes / roots (as tests/test_gpu_parity.py)."""

    def __init__(self, hx, m, primes, oracle=None):
        self.g = hx.Context(m)
        self.o = oracle or O.Ctx(m)
        for n, q in enumerate(primes):
            i = n if oracle else self.o.add_prime(q)
            assert self.g.add_prime(q, self.o.roots[i]) == i
        self.N = self.o.N
        self.primes = list(primes)

    def rand(self, idx, seed, batch):
        out = np.zeros((len(idx), batch, self.N), dtype=np.uint64)
        for r, i in enumerate(idx):
            for b in range(batch):
                out[r, b] = O.fill_uniform(self.N, self.primes[i], seed * 100003 + i * 131 + b)
        return out


def chain(m, L, K):
    g60, g56 = O.PrimeGen(60, m), O.PrimeGen(56, m)
    return [g60.next() for _ in range(L)] + [g56.next() for _ in range(K)]


def kernels_of(hx, fn):
    hx.profileBegin()
    out = fn()
    return out, {k["kernel"] for k in hx.profileEnd()["kernels"]}


def both_routes(hx, monkeypatch, m, primes, run):
    """run(P) on a context with the fused route and on its HX_NO_KS_LAST_FUSE=1 twin (the switch is read when a context
    is created); the kernel names say which route each took.  Returns the fused context's Pair and the two results."""
    monkeypatch.delenv("HX_NO_KS_LAST_FUSE", raising=False)
    Pf = Pair(hx, m, primes)
    monkeypatch.setenv("HX_NO_KS_LAST_FUSE", "1")
    Pc = Pair(hx, m, primes, oracle=Pf.o)
    monkeypatch.delenv("HX_NO_KS_LAST_FUSE", raising=False)
    got, kf = kernels_of(hx, lambda: run(Pf))
    ctl, kc = kernels_of(hx, lambda: run(Pc))
    assert any(FUSED_KERNEL in k for k in kf), sorted(kf)
    assert not any("::keyswitch_kernel" in k for k in kf), sorted(kf)
    assert not any(FUSED_KERNEL in k for k in kc), sorted(kc)
    assert any("keyswitch_kernel" in k for k in kc), sorted(kc)
    return Pf, got, ctl


def oracle_relin(P, own, sp, digits, t0, t1, t2, kb, ka, wrows):
    """Ctxt::reLinearize on one batch element: t0, t1 (or None), t2 = [L, N] evaluation rows; kb / ka = [D', nW, N]
    on the key's rows `wrows`, of which the first len(digits) digits and the rows of own + sp are used."""
    allp = own + sp
    pad = np.zeros((len(sp), P.N), dtype=np.uint64)
    o0 = np.vstack([P.o.scale_by_primes(own, t0, sp), pad])
    o1 = np.vstack([P.o.scale_by_primes(own, t1, sp), pad]) if t1 is not None else np.zeros_like(o0)
    dg = P.o.break_into_digits(own, t2, digits, allp)
    sel = [wrows.index(i) for i in allp]
    D = len(digits)
    return P.o.key_switch_digits(allp, dg, np.ascontiguousarray(kb[:D][:, sel]), np.ascontiguousarray(ka[:D][:, sel]), o0, o1)


def mixed_chain(m, L, K):
    """The chain of `chain`, its ctxt prime 1 replaced by one in (2^32, 2^60) that is not 1 mod 2^32: its row runs the
    Shoup transform and the Barrett store loop on the PLAIN key rows, beside the Proth-form rows of the same launch."""
    primes = chain(m, L, K)
    q = O.PrimeGen(36, m).next()
    assert (1 << 32) < q < (1 << 60) and q % (1 << 32) != 1 and q not in primes
    primes[1] = q
    return primes


CASES = {
    # name: (m, chain, L, K, digits of the key, [(ciphertext rows, digits used), ...] on ONE matrix, batch, has (s) part)
    "2_2_1_batch5": (16384, chain, 5, 2, [[0, 1], [2, 3], [4]], [(5, 3)], 5, True),
    "nd2_batch3": (16384, chain, 4, 2, [[0, 1], [2, 3]], [(4, 2)], 3, True),
    "nd4_batch5": (16384, chain, 6, 2, [[0, 1], [2, 3], [4], [5]], [(6, 4)], 5, True),
    # a ciphertext two primes below the key's level: rows 0..2 of a key made for 0..4 (the special rows' map.brow is
    # two past their row)
    "two_levels_below": (16384, chain, 5, 2, [[0, 1], [2], [3, 4]], [(3, 2)], 3, True),
    "no_s_part": (16384, chain, 5, 2, [[0, 1], [2, 3], [4]], [(5, 3)], 3, False),
    # one matrix, two consecutive calls at different levels: the converted copy is built once, with the matrix, and
    # indexed by the key's rows
    "one_matrix_two_levels": (16384, chain, 5, 2, [[0, 1], [2, 3], [4]], [(5, 3), (4, 2)], 3, True),
    "proth_and_shoup_rows": (16384, mixed_chain, 5, 2, [[0, 1], [2, 3], [4]], [(5, 3)], 3, True),
    "n14_6_5_5_batch2": (32768, chain, 16, 6, [list(range(0, 6)), list(range(6, 11)), list(range(11, 16))], [(16, 3)], 2, True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_proth_store_loop_equals_the_two_launch_route_and_the_oracle(hx, monkeypatch, name):
    m, mk, L, K, kdigits, calls, B, has_s = CASES[name]
    primes = mk(m, L, K)
    wrows = list(range(L + K))
    sp = list(range(L, L + K))
    D = len(kdigits)

    def run(P):
        kb = np.stack([P.rand(wrows, 20 + i, 1)[:, 0] for i in range(D)])
        ka = np.stack([P.rand(wrows, 30 + i, 1)[:, 0] for i in range(D)])
        W = hx.KeySwitch(P.g, wrows, kb, ka)
        outs = []
        for n, (Lc, nd) in enumerate(calls):
            own = list(range(Lc))
            assert sum(len(d) for d in kdigits[:nd]) == Lc
            t = [P.rand(own, 81 + 10 * n + i, B) for i in range(3)]
            t0, t1, t2 = (hx.DoubleCRT(P.g, own, B, x) for x in t)
            o0, o1 = hx.reLinearize(t0, t1 if has_s else None, t2, W, kdigits[:nd], sp)
            assert o0.getIndexSet() == own + sp == o1.getIndexSet()
            outs.append((o0.download(), o1.download(), t))
        return outs, kb, ka

    P, (got, kb, ka), (ctl, _, _) = both_routes(hx, monkeypatch, m, primes, run)
    for (Lc, nd), (g0, g1, t), (c0, c1, _) in zip(calls, got, ctl):
        own = list(range(Lc))
        assert np.array_equal(g0, c0) and np.array_equal(g1, c1), (Lc, nd)
        for b in range(B):
            w0, w1 = oracle_relin(P, own, sp, kdigits[:nd], t[0][:, b], t[1][:, b] if has_s else None, t[2][:, b], kb, ka, wrows)
            assert np.array_equal(g0[:, b], w0), (Lc, nd, b)
            assert np.array_equal(g1[:, b], w1), (Lc, nd, b)


@pytest.mark.gpu
def test_proth_store_loop_accumulating_into_scaled_parts(hx, monkeypatch):
    """hx_mul_relin with the tensor pass kept apart (HX_NO_MULRELIN_FUSE=1): the parts (1), (s) stand scaled in the
    outputs (scale_parts = 0) and enter the Montgomery sums times 2^64 mod q -- against the twin and the oracle."""
    m, L, K, digits, B = 16384, 5, 2, [[0, 1], [2, 3], [4]], 3
    primes = chain(m, L, K)
    own, sp = list(range(L)), list(range(L, L + K))
    allp = own + sp
    monkeypatch.setenv("HX_NO_MULRELIN_FUSE", "1")

    def run(P):
        kb = np.stack([P.rand(allp, 20 + i, 1)[:, 0] for i in range(3)])
        ka = np.stack([P.rand(allp, 30 + i, 1)[:, 0] for i in range(3)])
        W = hx.KeySwitch(P.g, allp, kb, ka)
        ops = [P.rand(own, s, B) for s in (1, 2, 3, 4)]
        G = [hx.DoubleCRT(P.g, own, B, x) for x in ops]
        o0, o1 = hx.multiplyBy(*G, W, digits)
        return o0.download(), o1.download(), ops, kb, ka

    P, (g0, g1, ops, kb, ka), (c0, c1, _, _, _) = both_routes(hx, monkeypatch, m, primes, run)
    assert np.array_equal(g0, c0) and np.array_equal(g1, c1)
    for b in range(B):
        w0, w1 = P.o.mul_relin(own, sp, digits, *(x[:, b] for x in ops), kb, ka)
        assert np.array_equal(g0[:, b], w0) and np.array_equal(g1[:, b], w1)
