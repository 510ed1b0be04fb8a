"""The key switch with each output row's last digit transform fused in (helib_amd/csrc/ntt_kernels.hip
ntt_keyswitch_last_kernel, engine.hip relin_core).

GPU: the fused route against its twin in the same binary (a context created under HX_NO_KS_LAST_FUSE=1: every
extension row through the row kernel, then keyswitch_kernel<D>) word for word on both output parts, and both against
the oracle's replay of Ctxt::reLinearize (addPrimesAndScale of the parts (1), (s); breakIntoDigits of the s^2 part;
keySwitchDigits).  The in-situ profiler says which kernels ran, so a case that silently took the other route fails.
CPU: the kernel's work map is a bijection with each row's workgroups adjacent in an XCD's dispatch order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_KERNEL = "ntt_keyswitch_last_kernel"


# ---------------------------------------------------------------- CPU: the work map
def test_ks_last_work_map_is_a_bijection_with_rows_adjacent_per_xcd():
    """ks_last_work (work_map.h) at the timed shape -- 22 rows x 128 elements: every XCD touches at most four rows'
    key words and twiddle tables -- at the shapes of the parity cases below, and over a sweep of odd sizes."""
    src = os.path.join(ROOT, "tests", "cpp", "ks_last_work_test.cpp")
    so = os.path.join(ROOT, "tests", "cpp", "libks_last_work_test.so")
    hdr = os.path.join(ROOT, "helib_amd", "csrc", "work_map.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    L = C.CDLL(so)
    L.check_ks_last_work.argtypes = [C.c_uint, C.c_uint, C.c_void_p]
    most = C.c_uint(0)
    assert L.check_ks_last_work(22, 128, C.byref(most)) == 0
    assert most.value <= 4                       # 2.75 rows per XCD, cut at most twice
    named = [(22, 3), (22, 5), (7, 3), (7, 5), (6, 3), (8, 3), (6, 2), (7, 2), (22, 1), (1, 1), (1, 7)]
    sweep = [(r, b) for r in range(1, 41) for b in (1, 2, 3, 4, 5, 7, 8, 9, 16, 31, 64, 128)]
    for r, b in named + sweep:
        assert L.check_ks_last_work(r, b, C.byref(most)) == 0, (r, b)
        assert most.value <= (r + 7) // 8 + 2, (r, b, most.value)


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
    assert not any(k.startswith("hx::keyswitch_kernel") or "::keyswitch_kernel" in k for k in kf), sorted(kf)
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


CASES = {
    # name: (m, L, K, digits of the key, ciphertext rows, digits used, batch, has (s) part)
    "6_5_5_batch3": (16384, 16, 6, [list(range(0, 6)), list(range(6, 11)), list(range(11, 16))], 16, 3, 3, True),
    "2_2_1_batch5": (16384, 5, 2, [[0, 1], [2, 3], [4]], 5, 3, 5, True),
    "nd2_batch3": (16384, 4, 2, [[0, 1], [2, 3]], 4, 2, 3, True),
    "nd4_batch5": (16384, 6, 2, [[0, 1], [2, 3], [4], [5]], 6, 4, 5, True),
    # a ciphertext one level below the key: rows 0..3 of a key made for 0..4, the first two digits (map.brow skips a row)
    "one_level_below": (16384, 5, 2, [[0, 1], [2, 3], [4]], 4, 2, 3, True),
    # (1, s(X^k)) after an automorphism: no part pointing at s
    "no_s_part": (16384, 5, 2, [[0, 1], [2, 3], [4]], 5, 3, 3, False),
    "n14_2_2_1": (32768, 5, 2, [[0, 1], [2, 3], [4]], 5, 3, 2, True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_fused_route_equals_the_two_launch_route_and_the_oracle(hx, monkeypatch, name):
    """Digit layouts 6/5/5 and 2/2/1 (rows owned by digit 0, 1, 2 and special rows), D = 2 and D = 4, batches 3 and 5
    (work-map remainders), a ciphertext below the key's level, a ciphertext without an (s) part, N = 2^13 and 2^14."""
    m, L, K, kdigits, Lc, nd, B, has_s = CASES[name]
    primes = chain(m, L, K)
    wrows = list(range(L + K))
    own, sp = list(range(Lc)), list(range(L, L + K))
    digits = kdigits[:nd]
    assert sum(len(d) for d in digits) == Lc
    D = len(kdigits)

    def run(P):
        kb = np.stack([P.rand(wrows, 20 + i, 1)[:, 0] for i in range(D)])
        ka = np.stack([P.rand(wrows, 30 + i, 1)[:, 0] for i in range(D)])
        W = hx.KeySwitch(P.g, wrows, kb, ka)
        t = [P.rand(own, 81 + i, B) for i in range(3)]
        t0, t1, t2 = (hx.DoubleCRT(P.g, own, B, x) for x in t)
        o0, o1 = hx.reLinearize(t0, t1 if has_s else None, t2, W, digits, sp)
        assert o0.getIndexSet() == own + sp == o1.getIndexSet()
        for d, x in zip((t0, t1, t2), t):
            assert np.array_equal(d.download(), x)            # operands untouched
        return o0.download(), o1.download(), t, kb, ka

    P, (g0, g1, t, kb, ka), (c0, c1, _, _, _) = both_routes(hx, monkeypatch, m, primes, run)
    assert np.array_equal(g0, c0) and np.array_equal(g1, c1)
    for b in range(B):
        w0, w1 = oracle_relin(P, own, sp, digits, t[0][:, b], t[1][:, b] if has_s else None, t[2][:, b], kb, ka, wrows)
        assert np.array_equal(g0[:, b], w0), b
        assert np.array_equal(g1[:, b], w1), b


@pytest.mark.gpu
def test_fused_route_with_shared_operands_and_in_place_outputs(hx, monkeypatch):
    """Copy-on-write: the parts (1) and (s) are lazy copies of one object, the s^2 part a lazy copy of another -- and
    then the outputs ARE the parts (1), (s) (lazy copies that the call has to take private first): the fused kernel
    reads a word of its accumulator row and writes the same word of the same row."""
    m, L, K, digits, B = 16384, 5, 2, [[0, 1], [2, 3], [4]], 3
    primes = chain(m, L, K)
    own, sp = list(range(L)), list(range(L, L + K))
    allp = own + sp

    def run(P):
        kb = np.stack([P.rand(allp, 20 + i, 1)[:, 0] for i in range(3)])
        ka = np.stack([P.rand(allp, 30 + i, 1)[:, 0] for i in range(3)])
        W = hx.KeySwitch(P.g, allp, kb, ka)
        x, y = P.rand(own, 91, B), P.rand(own, 92, B)
        t0 = hx.DoubleCRT(P.g, own, B, x)
        t1 = t0.copy()                                        # lazily shared with t0
        src2 = hx.DoubleCRT(P.g, own, B, y)
        t2 = src2.copy()
        o0, o1 = hx.reLinearize(t0, t1, t2, W, digits, sp)
        a0, a1 = o0.download(), o1.download()
        assert np.array_equal(t0.download(), x) and np.array_equal(t1.download(), x) and np.array_equal(src2.download(), y)
        p0, p1 = t0.copy(), t0.copy()
        hx.reLinearize(p0, p1, t2, W, digits, sp, out0=p0, out1=p1)
        assert np.array_equal(t0.download(), x)               # the shared source kept its words
        return a0, a1, p0.download(), p1.download(), x, y, kb, ka

    P, got, ctl = both_routes(hx, monkeypatch, m, primes, run)
    for g, c in zip(got[:4], ctl[:4]):
        assert np.array_equal(g, c)
    a0, a1, i0, i1, x, y, kb, ka = got
    assert np.array_equal(a0, i0) and np.array_equal(a1, i1)
    w0, w1 = oracle_relin(P, own, sp, digits, x[:, 0], x[:, 0], y[:, 0], kb, ka, allp)
    assert np.array_equal(a0[:, 0], w0) and np.array_equal(a1[:, 0], w1)


@pytest.mark.gpu
def test_fused_route_accumulating_into_scaled_parts(hx, monkeypatch):
    """hx_mul_relin with the tensor pass kept apart (HX_NO_MULRELIN_FUSE=1): the parts (1), (s) stand scaled in the
    outputs and the key switch accumulates onto them -- the fused kernel's identity-scale form -- against its twin and
    the oracle's mul_relin."""
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
