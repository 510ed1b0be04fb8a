"""CPU-side checks of the product's host logic (no GPU needed):
  * the HIP NTT kernel's phase functions (helib_amd/csrc/ntt_core.h), replayed
    thread-by-thread on the CPU, equal the oracle for every supported size;
  * the C-ABI library loads and exports every symbol include/helib_amd.h declares;
  * product-side parameter helpers agree with the oracle's restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def replay():
    src = os.path.join(ROOT, "tests", "cpp", "ntt_replay.cpp")
    so = os.path.join(ROOT, "tests", "cpp", "libntt_replay.so")
    hdr = os.path.join(ROOT, "helib_amd", "csrc", "ntt_core.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        # HX_CHECK_BOUNDS: every compile-time lazy bound of the kernel (values < B*q before each
        # butterfly / normalisation) is also asserted at run time in the replay
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DHX_CHECK_BOUNDS", "-shared", "-fPIC", "-o", so, src])
    L = C.CDLL(so)
    L.ntt_replay.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    L.ntt_replay_proth.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    L.mont_acc_replay.argtypes = [C.c_uint64, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ntt_replay_proth_mul.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.mark.parametrize("logn", [13, 14, 15])
@pytest.mark.parametrize("bits", [60, 49, 36, 31])
def test_ntt_kernel_phases_replayed_on_cpu(replay, logn, bits):
    # 60: the largest primes the lazy scheme admits (16q <= 2^64); 31: q < 2^32, the normaliser's
    # conditional-subtraction chain instead of the reciprocal estimate
    N = 1 << logn
    m = 2 * N
    q = O.PrimeGen(bits, m).next()
    cm = O.Cmod(m, q)
    for seed, x in ((1, O.fill_uniform(N, q, 5)), (2, np.full(N, q - 1, dtype=np.uint64)),
                    (3, np.zeros(N, dtype=np.uint64))):
        y = cm.fft(x)
        out = np.zeros(N, dtype=np.uint64)
        assert replay.ntt_replay(logn, 0, q, cm.root, x.ctypes.data, out.ctypes.data) == 0
        assert np.array_equal(out, y)
        back = np.zeros(N, dtype=np.uint64)
        assert replay.ntt_replay(logn, 1, q, cm.root, y.ctypes.data, back.ctypes.data) == 0
        assert np.array_equal(back, x)


# ---------------------------------------------------------------- round 5: the Proth-form butterflies
def _proth_parts(q):
    """q = t 2^s + 1, t odd (src/PrimeGenerator.h:66-118 makes every chain prime in this form)."""
    s = ((q - 1) & -(q - 1)).bit_length() - 1
    return (q - 1) >> s, s


def _chain_primes():
    """The primes of the benchmark chains the row kernels see: ctxt, special and small primes of the m = 32768 and
    m = 65536 rings (helib_amd.ctxt.ChainContext restates Context::buildModChain)."""
    from helib_amd import ctxt as CT
    out = {}
    for m, bits, ckks in ((32768, 950, False), (65536, 1400, True), (65536, 440, True), (32768, 6400, False)):
        cc = CT.ChainContext(m, -1 if ckks else 65537, 1, bits=bits, c=3, ckks=ckks)
        out[(m, bits)] = [int(q) for q in cc.primes]
    return out


def test_proth_form_of_the_chain_primes():
    """every prime PrimeGenerator makes is t 2^s + 1; the Proth-form rows need s >= 32 (the
    low word of q is 1).  That holds for every prime of the bits = 950 / 1400 / 6400 chains; rows of any other
    prime (the two 38-bit small primes of the CKKS bits = 440 chain, s = 29; user primes; the m = 12 fixture) keep the Shoup
    butterflies -- the choice is per row (PrimeDev::proth), not per context."""
    for m, bits in ((32768, 60), (32768, 56), (65536, 60), (65536, 55), (32768, 50), (65536, 45)):
        g = O.PrimeGen(bits, m)
        for _ in range(8):
            q = g.next()
            t, s = _proth_parts(q)
            assert s >= 32 and q & 0xffffffff == 1 and q >> 32 == t << (s - 32)
    chains = _chain_primes()
    for key, qs in chains.items():
        bad = [q for q in qs if _proth_parts(q)[1] < 32]
        assert (len(bad) == 2 and all(q.bit_length() <= 40 for q in bad)) if key == (65536, 440) else not bad, (key, bad)
        assert all(q < 2 ** 60 for q in qs)


@pytest.mark.parametrize("bits,m", [(60, 32768), (56, 32768), (57, 32768), (40, 32768), (60, 65536), (55, 65536), (45, 65536)])
def test_proth_montgomery_product_restated_in_python_integers(replay, bits, m):
    """mont_acc (helib_amd/csrc/ntt_core.h) against python integers: for q = qh 2^32 + 1, W = w 2^64 mod q and any
    y below 207/16 q, the word-wise reduction with the complemented quotient digits n0, n1 returns x + R with
    R 2^64 = y W + M q, M = (n0+1) + (n1+1) 2^32 -- so R = y w (mod q) -- and 0 < R < q (1 + y/2^64 + 2^-32) < 2q;
    none of the 64-bit accumulators wraps.  Both the identity (in python) and the device's word arithmetic
    (mont_acc_replay, the same source compiled for the host) are checked, incl. the extreme operands."""
    q = O.PrimeGen(bits, m).next()
    assert q & 0xffffffff == 1
    qh = q >> 32
    c1 = (1 + qh) * (2 ** 32 + 1)
    lim = 207 * q // 16
    rng = np.random.default_rng(bits * m)
    n = 4000
    ys = [0, 1, q - 1, q, lim - 1, 2 ** 32 - 1, 2 ** 32, (lim - 1) | 0xffffffff if ((lim - 1) | 0xffffffff) < lim else lim - 1]
    ys += [int(v) % lim for v in rng.integers(0, 2 ** 63, n - len(ys), dtype=np.uint64) * 2]
    Ws = [0, 1, q - 1, 0xffffffff, q - 2 ** 32] + [int(v) for v in rng.integers(0, q, n - 5, dtype=np.uint64)]
    xs = [0, 2 ** 64 - 2 * q - 1] + [int(v) for v in rng.integers(0, 14 * q - 1, n - 2, dtype=np.uint64)]
    got = np.zeros(n, dtype=np.uint64)
    ya, Wa, xa = (np.array(v, dtype=np.uint64) for v in (ys, Ws, xs))
    replay.mont_acc_replay(q, n, ya.ctypes.data, Wa.ctypes.data, xa.ctypes.data, got.ctypes.data)
    Rinv = pow(2 ** 64, -1, q)
    M32 = 2 ** 32 - 1
    for y, W, x, g in zip(ys, Ws, xs, got):
        yl, yh, wl, wh = y & M32, y >> 32, W & M32, W >> 32
        a = yl * wl
        n0 = ~a & M32
        G = yl * wh + c1 + n0 * qh + (a >> 32) + yh * wl
        assert G < 2 ** 64                                   # (the operand limit is what keeps this sum in a word)
        n1 = ~G & M32
        D = yh * wh + n1 * qh + (G >> 32)
        Mq = (n0 + 1) + (n1 + 1) * 2 ** 32
        assert D * 2 ** 64 == y * W + Mq * q                 # the reduction is exact: nothing was dropped
        assert D % q == y * W * Rinv % q and 0 < D < 2 * q
        assert D * 2 ** 64 < q * (2 ** 64 + y + 2 ** 32) + 2 ** 64   # R < q (1 + y W / (q 2^64) + 2^-32), W < q
        assert x + D < 2 ** 64 and int(g) == x + D           # the device's words


@pytest.mark.parametrize("logn", [13, 14, 15])
@pytest.mark.parametrize("bits", [60, 56, 45])
def test_proth_row_transform_replayed_on_cpu(replay, logn, bits):
    """The row kernels' phases with the Proth-form butterflies (RowNTT<LOGN, ArProth>), thread by thread, every
    compile-time bound (sixteenths of q forward, whole q inverse) asserted at run time (HX_CHECK_BOUNDS): canonical,
    all-(q-1) and zero rows, and rows of lazy words in [0,8q) (the load bound of the exact-RNS kernels' output)."""
    N = 1 << logn
    m = 2 * N
    q = O.PrimeGen(bits, m).next()
    cm = O.Cmod(m, q)
    rng = np.random.default_rng(logn * bits)
    for x in (O.fill_uniform(N, q, 5), np.full(N, q - 1, dtype=np.uint64), np.zeros(N, dtype=np.uint64)):
        y = cm.fft(x)
        out = np.zeros(N, dtype=np.uint64)
        assert replay.ntt_replay_proth(logn, 0, 0, q, cm.root, x.ctypes.data, out.ctypes.data) == 0
        assert np.array_equal(out, y)
        back = np.zeros(N, dtype=np.uint64)
        assert replay.ntt_replay_proth(logn, 1, 0, q, cm.root, y.ctypes.data, back.ctypes.data) == 0
        assert np.array_equal(back, x)
        lazy = x + np.uint64(q) * rng.integers(0, 8, N, dtype=np.uint64)
        lazy[0] = x[0] + np.uint64(7 * q)
        assert replay.ntt_replay_proth(logn, 0, 1, q, cm.root, lazy.ctypes.data, out.ctypes.data) == 0
        assert np.array_equal(out, y)
        # the digit rows as the device reads them (BufIOT<8>::load_bound<ArProth>() = 2): words in [0,2q)
        lazy2 = x + np.uint64(q) * rng.integers(0, 2, N, dtype=np.uint64)
        lazy2[0] = x[0] + np.uint64(q)
        assert replay.ntt_replay_proth(logn, 0, 2, q, cm.root, lazy2.ctypes.data, out.ctypes.data) == 0
        assert np.array_equal(out, y)
    # a prime that is not of the form is refused by the Proth replay (the engine gives such rows the Shoup kernels)
    q31 = O.PrimeGen(31, m).next()
    assert replay.ntt_replay_proth(logn, 0, 0, q31, O.Cmod(m, q31).root, out.ctypes.data, out.ctypes.data) == -2


def test_proth_form_of_the_digit_kernel_restated():
    """break_digit_pass / rns_extend_fast_one on Proth-form primes (helib_amd/csrc/rns_kernels.h: ExtPlanDev::src_mont,
    TgtRec::mont; engine.hip: rec_to_mont), restated word for word with python integers on the digits of the bits = 950
    chain (6 / 5 / 5 ctxt primes, 60 bits; 6 special primes, 56 bits) and checked against the definition
    (src/DoubleCRT.cpp:479-561: digit = centred CRT of its own rows, extended to every other row; later digits'
    rows -= digit, /= P):
      * Garner steps as Montgomery products by p_l^-1 2^64: operand v + 2 p_k - a_l in (0, 6 p_k), result below 2 p_k;
      * a target's limb sum (30-bit limbs, three accumulators, none wraps) + cnt (-P 2^64), reduced by mont_redc128:
        the stray 2^-64 cancels the 2^64 of the record's words, the result is below 2q and congruent to the digit;
      * the later rows' fix-up u + 2q - v (u < 4q) times P^-1 2^64: below 2q, so the next digit's loads stay lazy
        words below 4 p_k."""
    import random
    rnd = random.Random(17)
    M32, M64 = 2 ** 32 - 1, 2 ** 64 - 1
    qs = _chain_primes()[(32768, 950)]
    ctxt = sorted(q for q in qs if q.bit_length() == 60)[:16]
    special = [q for q in qs if q.bit_length() == 56][:6]
    assert len(ctxt) == 16 and len(special) == 6
    rows = ctxt + special                    # all rows, ctxt first (the digit kernel's order is ascending row index)
    L = 16
    offs = [0, 6, 11, 16]

    def mont_acc(y, W, q, x=0):              # ntt_core.h mont_acc, word for word
        qh = q >> 32
        c1 = (1 + qh) * (2 ** 32 + 1)
        assert q & M32 == 1 and y < 207 * q // 16
        yl, yh, wl, wh = y & M32, y >> 32, W & M32, W >> 32
        a = yl * wl
        n0 = ~a & M32
        G = yl * wh + c1 + n0 * qh + (a >> 32) + yh * wl
        assert G <= M64
        n1 = ~G & M32
        D = yh * wh + x + n1 * qh + (G >> 32)
        assert D <= M64
        return D

    def mont_redc128(lo, hi, q):             # ntt_core.h mont_redc128, word for word
        qh = q >> 32
        c1 = (1 + qh) * (2 ** 32 + 1)
        assert hi < 2 ** 62
        n0 = ~lo & M32
        G = n0 * qh + c1 + (lo >> 32)
        assert G <= M64
        n1 = ~G & M32
        D = n1 * qh + hi + (G >> 32)
        assert D <= M64
        return D

    def m64(x, q):
        return (x << 64) % q

    for trial in range(60):
        x = [rnd.randrange(q) for q in ctxt]                     # the operand's coefficient, canonical rows
        if trial == 0:
            x = [q - 1 for q in ctxt]
        if trial == 1:
            x = [0] * 16
        xs = list(x)                                             # the LDS column: later rows updated in place
        want_rows = list(x)
        for d in range(3):
            off, N = offs[d], offs[d + 1] - offs[d]
            p = ctxt[off:off + N]
            P = 1
            for v in p:
                P *= v
            # ---- Garner front (garner_front, src_mont) on lazy words
            a = []
            for k in range(N):
                v = xs[off + k]
                assert v < 4 * p[k]
                for l in range(k):
                    ginv_m = m64(pow(p[l], -1, p[k]), p[k])
                    y = v + 2 * p[k] - a[l]
                    assert 0 < y < 6 * p[k]
                    v = mont_acc(y, ginv_m, p[k])
                    assert 0 < v < 2 * p[k]
                if v >= 2 * p[k]:
                    v -= 2 * p[k]
                if v >= p[k]:
                    v -= p[k]
                a.append(v)
            val, run = 0, 1
            for k in range(N):
                val += a[k] * run
                run *= p[k]
            assert 0 <= val < P and all(val % p[k] == want_rows[off + k] % p[k] for k in range(N))
            neg = val > (P - 1) // 2
            cnt = 1 if neg else 0
            digit = val - P if neg else val
            a0 = [v & 0x3fffffff for v in a]
            a1 = [v >> 30 for v in a]
            assert all(v < 2 ** 30 for v in a1)
            # ---- every other row
            for r, q in enumerate(rows):
                if off <= r < off + N:
                    continue
                negP_m = m64(q - P % q, q)
                c00 = c01 = c11 = 0
                run = 1
                for k in range(N):
                    W = m64(run % q, q)                          # the record's multiplier: (p_0..p_{k-1}) 2^64 mod q
                    run *= p[k]
                    w0, w1 = W & 0x3fffffff, W >> 30
                    assert w1 < 2 ** 30
                    c00 += a0[k] * w0
                    c01 += a0[k] * w1 + a1[k] * w0
                    c11 += a1[k] * w1
                assert max(c00, c01, c11) <= M64
                S = cnt * negP_m + c00 + (c01 << 30) + (c11 << 60)
                v = mont_redc128(S & M64, S >> 64, q)
                assert 0 < v < 2 * q and v % q == digit % q
                if off + N <= r < L:
                    u = xs[r]
                    assert u < 4 * q
                    y = u + 2 * q - v
                    assert 0 < y < 6 * q
                    xs[r] = mont_acc(y, m64(pow(P, -1, q), q), q)
                    assert 0 < xs[r] < 2 * q
                    want_rows[r] = (want_rows[r] - digit) * pow(P, -1, q) % q
                    assert xs[r] % q == want_rows[r]
    # a target with sixteen 60-bit sources (rns_extend_fast_one, four accumulators): S 2^-64 + q (1 + 2^-32) < 3q
    q = special[0]
    S = 16 * (2 ** 60 - 1) * (q - 1) + 17 * (q - 1)
    v = mont_redc128(S & M64, S >> 64, q)
    assert v < 3 * q and v % q == S * pow(2 ** 64, -1, q) % q


@pytest.mark.parametrize("logn", [13, 14, 15])
@pytest.mark.parametrize("bits", [60, 56, 45])
def test_proth_product_on_load_replayed_on_cpu(replay, logn, bits):
    """ntt_inv_mul_kernel on a Proth-form row (MulLoadIO<true>, helib_amd/csrc/ntt_kernels.hip): the inverse transform
    of a pointwise product whose 128-bit words are reduced by mont_redc128 alone on load -- values in (0, 2q) carrying
    2^-64, taken by the inverse passes at bound 2, the factor given back by the last stage's constants times 2^128.
    The same arithmetic replayed thread by thread with every lazy bound asserted: random rows, all-(q-1) rows (the
    largest products) and rows with zeros, against the oracle's iFFT of the canonical product."""
    N = 1 << logn
    m = 2 * N
    q = O.PrimeGen(bits, m).next()
    cm = O.Cmod(m, q)
    rng = np.random.default_rng(logn + bits)
    cases = [(O.fill_uniform(N, q, 3), O.fill_uniform(N, q, 4)),
             (np.full(N, q - 1, dtype=np.uint64), np.full(N, q - 1, dtype=np.uint64)),
             (O.fill_uniform(N, q, 6) * rng.integers(0, 2, N, dtype=np.uint64), O.fill_uniform(N, q, 7))]
    for a, b in cases:
        prod = np.array([int(x) * int(y) % q for x, y in zip(a, b)], dtype=np.uint64)
        want = cm.ifft(prod)
        out = np.zeros(N, dtype=np.uint64)
        assert replay.ntt_replay_proth_mul(logn, q, cm.root, a.ctypes.data, b.ctypes.data, out.ctypes.data) == 0
        assert np.array_equal(out, want)


def test_c_abi_exports_every_declared_symbol():
    from helib_amd import capi
    hdr = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    declared = sorted(set(re.findall(r"\b(hx_[a-zA-Z0-9_]+)\s*\(", hdr)))
    assert declared, "no declarations parsed"
    lib = capi.lib()
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, f"declared in include/helib_amd.h but not exported: {missing}"
    assert sorted(capi.SYMBOLS) == declared
    assert b"gfx950" in lib.hx_version()


def test_no_cpu_fallback_without_device():
    from helib_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(capi.HxError) as ei:
        capi.Context(32768)
    assert ei.value.code == capi.HX_ERR_DEVICE


def test_product_does_not_import_oracle():
    """oracle/ is test infrastructure: only tests/, __graft_entry__.smoke() and bench.py's
    cpu_baseline leg may touch it -- not the package, not the C/C++ headers, not the tools."""
    for sub in ("helib_amd", "include", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                if f.endswith((".py", ".h", ".hpp", ".hip", ".cpp", ".sh")):
                    txt = open(os.path.join(dirpath, f)).read()
                    assert "import oracle" not in txt and "from oracle" not in txt, f
                    assert "hx_oracle" not in txt and "liboracle" not in txt, f
    # bench.py: the oracle appears only inside the cpu_baseline functions
    import ast
    src = open(os.path.join(ROOT, "bench.py")).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef):
            body = ast.get_source_segment(src, node)
            uses = any(k in body for k in ("from oracle", "import oracle", "build_native_oracle()", "hx_oracle",
                                            "cpu_baseline_fresh(", "cpu_baseline_fixed("))
            if uses and node.name != "main":       # main() only calls the cpu_baseline functions
                assert node.name in ("build_native_oracle", "cpu_baseline_fixed", "cpu_baseline_fresh",
                                     "cpu_baseline_all_cores"), node.name


def test_every_environment_switch_is_set_by_a_test_or_a_tool():
    """A switch selects a second path through the engine; one that no test, tool or bench.py sets is a path nothing
    runs.  Every HX_* name the library hands to getenv (helib_amd/csrc/switches.h: directly or through its on()
    helper, so every "HX_..." literal of a file that calls getenv counts) must be named under tests/, tools/ or in
    bench.py -- except the diagnostic and the wait policy, which select no compute path."""
    exempt = {"HX_ARENA_TRACE", "HX_WAIT_POLL_US"}
    read = set()
    for sub in (os.path.join("helib_amd", "csrc"), "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                if "getenv" in txt:
                    read |= set(re.findall(r'"(HX_[A-Z0-9_]+)"', txt))
    assert exempt <= read and len(read) > len(exempt), sorted(read)
    users = open(os.path.join(ROOT, "bench.py")).read()
    for sub in ("tests", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, sub)):
            for f in files:
                if f.endswith((".py", ".sh", ".cpp", ".h", ".hpp", ".hip")):
                    users += open(os.path.join(dirpath, f), errors="ignore").read()
    unused = sorted(n for n in read - exempt if not re.search(r"\b%s\b" % n, users))
    assert not unused, f"environment switches that no test, tool or bench.py sets: {unused}"


def test_hostnt_matches_oracle():
    from helib_amd import hostnt
    for length, m in [(60, 32768), (56, 32768), (49, 16384), (60, 21845), (59, 65536)]:
        a, b = hostnt.PrimeGen(length, m), O.PrimeGen(length, m)
        assert [a.next() for _ in range(6)] == [b.next() for _ in range(6)]
    q = O.PrimeGen(60, 21845).next()
    assert hostnt.find_primitive_root(q, 21845) == O.lib().ho_find_prim_root(q, 21845)


def test_cpp_facade_header_compiles_and_links():
    """include/helib_amd.hpp + tests/cpp/facade_test.cpp build against the C ABI and the oracle
    (no GPU needed to compile/link; the program itself runs in the -m gpu suite)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    out = os.path.join(ROOT, "tests", "cpp", "facade_test.bin")
    libdir = os.path.join(ROOT, "helib_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "cpp", "facade_test.cpp"),
                           "-L" + libdir, "-lhelib_amd", os.path.join(ROOT, "oracle", "liboracle.so"),
                           "-Wl,-rpath," + libdir, "-o", out])
    os.remove(out)
    out2 = os.path.join(ROOT, "tests", "cpp", "ctxt_test.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ctxt_test.cpp"), "-L" + libdir, "-lhelib_amd",
                           "-Wl,-rpath," + libdir, "-o", out2])
    os.remove(out2)
    out3 = os.path.join(ROOT, "tests", "cpp", "keys_test.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "keys_test.cpp"), "-L" + libdir, "-lhelib_amd",
                           "-Wl,-rpath," + libdir, "-o", out3])
    # the product path fails loudly without a device: no CPU fallback behind the C++ keys either
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([out3, "128", "257", "150", "0"], capture_output=True, text=True)
        assert r.returncode != 0 and "no HIP device" in r.stderr
    os.remove(out3)
    # the wider Ctxt operations and Ctxt::writeTo / read link against the product library as well
    for name in ("ctxt_ops_test", "io_test"):
        out4 = os.path.join(ROOT, "tests", "cpp", name + ".bin")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-L" + libdir, "-lhelib_amd",
                               "-Wl,-rpath," + libdir, "-o", out4])
        os.remove(out4)


@pytest.mark.parametrize("m,p,bits", [(32768, 65537, 950), (16384, 65537, 250), (128, 257, 150), (1705, 7, 200),
                                      (32768, 2, 300), (65536, -1, 1400), (128, -1, 250), (65536, -1, 440),
                                      (16384, -1, 300)])
def test_cpp_host_chain_and_prime_set_decision_match_the_python_mirror(m, p, bits, tmp_path):
    """include/helib_amd_ctxt.hpp (C++ host side: PrimeGenerator, buildModChain, ModuliSizes,
    computeIntervalForMul) against helib_amd/ctxt.py: same primes, digits, table size and the same
    prime set chosen for the product of two fresh ciphertexts."""
    import json
    import math
    from helib_amd import ctxt as hc
    exe = str(tmp_path / "chain_test")
    libdir = os.path.join(ROOT, "helib_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "chain_test.cpp"), "-L" + libdir, "-lhelib_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    got = json.loads(subprocess.check_output([exe, str(m), str(p), str(bits)]))
    ckks = p == -1                  # the CKKS chain (precision 20): other special-prime sizing, other window end
    c = hc.ChainContext(m, p, 20 if ckks else 1, bits=bits, c=3, ckks=ckks)
    assert got["primes"] == c.primes
    assert got["small"] == c.smallPrimes and got["ctxt"] == c.ctxtPrimes and got["special"] == c.specialPrimes
    assert got["digits"] == c.digits and got["nsizes"] == len(c.modSizes.sizes)
    assert abs(got["fresh_ln"] - math.log(c.freshNoiseBound())) < 1e-12
    assert got["bitSizeOfQ"] == c.bitSizeOfQ() and abs(got["securityLevel"] - c.securityLevel()) < 1e-9
    a = hc.Ctxt(c, None)
    a.parts = {"1": None, "s": None}
    a.primeSet = frozenset(c.ctxtPrimes)
    a.lnNoise = math.log(c.freshNoiseBound())
    lo, hi = hc.Ctxt.computeIntervalForMul(a, a)
    assert abs(got["lo"] - lo) < 1e-9 and abs(got["hi"] - hi) < 1e-9
    assert got["common"] == sorted(c.modSizes.getSet4Size(lo, hi, a.primeSet, a.primeSet, ckks))


@pytest.mark.parametrize("radix,logq", [(4, 13), (8, 13)])
def test_split_convolution_replayed_on_cpu(replay, radix, logq):
    """The long convolutions of the Bluestein path (conv_core.h): radix-4 split (2^16 / 2^17) and
    radix-8 split (2^18) = first stages on elements Q apart, then independent Q-point sub-transforms
    with their own twiddle tables.  Replayed on the CPU with the kernel's phase functions and
    compared with a direct negacyclic product of two sparse polynomials."""
    Q = 1 << logq
    n = radix * Q
    q = O.PrimeGen(50, 4 * n).next()                     # 2n | q-1 with room
    psi = O.lib().ho_find_prim_root(q, 2 * n)
    rng = np.random.default_rng(radix)
    a, b = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    ia, ib = rng.choice(n, 6, replace=False), rng.choice(n, 5, replace=False)
    a[ia] = rng.integers(1, q, 6, dtype=np.uint64)
    b[ib] = rng.integers(1, q, 5, dtype=np.uint64)
    want = [0] * n
    for i in ia:
        for j in ib:
            k, v = int(i + j), int(a[i]) * int(b[j]) % q
            if k >= n:                                    # X^n = -1
                k, v = k - n, (q - v) % q
            want[k] = (want[k] + v) % q
    c = np.zeros(n, dtype=np.uint64)
    fn = replay.split_conv_replay if radix == 4 else replay.split_conv8_replay
    fn.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn(logq, q, psi, a.ctypes.data, b.ctypes.data, c.ctypes.data) == 0
    assert [int(v) for v in c] == want


@pytest.mark.parametrize("radix,logq", [(4, 14), (4, 13), (8, 13), (16, 13)])
def test_big_power_of_two_transform_replayed_on_cpu(replay, radix, logq):
    """Power-of-two rings beyond one row kernel (engine.hip pow2_big_rows: N = 2^16 .. 2^19 as 4 / 8 / 16
    sub-transforms, natural order in and out): the kernel phase functions, the sub-transform twiddle
    tables and the interleave replayed on the CPU against the oracle's Cmodulus::FFT / iFFT
    (src/CModulus.cpp:389-426, 493-553).  (4, 14) is m = 131072 as the engine runs it."""
    n = radix << logq
    m = 2 * n
    q = O.PrimeGen(55, m).next()
    o = O.Ctx(m)
    i = o.add_prime(q)
    psi = o.roots[i]
    rng = np.random.default_rng(radix * 100 + logq)
    x = rng.integers(0, q, n, dtype=np.uint64)
    x[:3] = [q - 1, 0, 1]
    want = o.fft([i], x[None, :])[0]
    fn = replay.big_ntt_replay
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    y = np.zeros(n, dtype=np.uint64)
    assert fn(logq, radix, 0, q, psi, x.ctypes.data, y.ctypes.data) == 0
    assert np.array_equal(y, want)
    back = np.zeros(n, dtype=np.uint64)
    assert fn(logq, radix, 1, q, psi, want.ctypes.data, back.ctypes.data) == 0
    assert np.array_equal(back, x)


def test_cpp_key_material_generator_is_chacha20_keyed_from_os_entropy(tmp_path):
    """include/helib_amd_keys.hpp draws key material from a ChaCha20 generator keyed with
    std::random_device by default (the reference seeds NTL's PRG from OS entropy, src/keys.cpp
    GenKeySWmatrix: RandomBits(prgSeed, 256)); an explicit seed is deterministic, for tests.  The block
    function reproduces RFC 8439 section 2.3.2."""
    exe = str(tmp_path / "prg_test")
    libdir = os.path.join(ROOT, "helib_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "prg_test.cpp"), "-L" + libdir, "-lhelib_amd",
                           "-Wl,-rpath," + libdir, "-o", exe])
    out = subprocess.check_output([exe], text=True).splitlines()
    assert out[0] == ("block e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
                      "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2")
    assert out[1:] == ["seeded 1 1", "entropy 1", "urbg 1"]


def test_slab_arena_on_the_cpu(tmp_path):
    """helib_amd/csrc/arena.h (the device-memory arena behind every DoubleCRT slab) with malloc standing in
    for hipMalloc: no overlapping extents over 20 000 random operations, full coalescing, no system
    allocation per step once a keep-the-results loop is warm, the HIP-graph pin / defer rules, and the
    out-of-memory path."""
    exe = str(tmp_path / "arena_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "arena_test.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "arena_test OK" in r.stdout, r.stdout + r.stderr


def test_register_tiled_norm_kernel_replayed_on_cpu(tmp_path):
    """helib_amd/csrc/norm_r16.h (the N = 2^14 canonical-embedding norm as three radix-16 register passes + the
    last stage inside the pairing pass): its phase functions run thread by thread on the CPU, with the kernel's
    index maps, twiddle strides and padded LDS layout, against the long-double definition max_j |f(W^(2j+1))|
    over ALL evaluation points, for a sparse and a dense polynomial (1e-9 relative)."""
    exe = str(tmp_path / "norm_replay")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas",
                           os.path.join(ROOT, "tests", "cpp", "norm_replay.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "norm_replay OK" in r.stdout, r.stdout + r.stderr


def test_bench_ckks_basic_op_list_over_the_cpu_checker():
    """bench.py's ckks_basic_ops leg (the reference's benchmarks/ckks_basic.cpp list: add / subtract / negate /
    square / rotate / multiply without and with relinearisation / multiply-and-add / encrypt / decrypt) run at
    m = 1024 with the CPU checker standing in for the device polynomials: every operation decodes to the plaintext
    operation within the error bound its ciphertext reports (the leg aborts the benchmark otherwise)."""
    import bench
    from helib_amd import ctxt as hc
    from oracle.backend import OracleBackend, OPoly

    def backend(cc):
        o = O.Ctx(cc.m)
        for q in cc.primes:
            o.add_prime(q)
        return OracleBackend(o, cc), (lambda idx, rows: OPoly(o, idx, rows[:, 0]))
    for precision in (1, 20):      # the reference's benchmark setting, and one where the relative check applies too
        out = bench.ckks_basic_ops(None, hc, 0, 0, lambda: None, 300, B=1, reps=1, m=1024, backend=backend, precision=precision)
        _check_ckks_list(out)


def _check_ckks_list(out):
    names = ["adding_two_ciphertexts", "subtracting_two_ciphertexts", "negating_a_ciphertext", "square_a_ciphertext",
             "rotate_a_ciphertext_by1", "multiplying_two_ciphertexts_no_relin", "multiplying_two_ciphertexts",
             "multiply_and_add_two_ciphertexts", "encrypting_ciphertexts", "decrypting_ciphertexts"]
    for nme in names:
        assert isinstance(out[nme], dict), (nme, out[nme])
    for nme in names[:8]:
        assert out[nme]["decode_max_abs_err"] <= out[nme]["reported_error_bound"]


def test_approximate_barrett_of_the_fused_kernels_restated():
    """red128_q8 / tensor_red128 (helib_amd/csrc/rns_kernels.h, ntt_kernels.hip): S mod q for S < 8 q^2 with ONE
    approximate high product -- xt = S >> (k-1) (k = bitlen q), qh = xh*mh + hi32(xh*ml) + hi32(xl*mh) with
    mu63 = floor(2^(63+k)/q) split into 32-bit halves, r = S - qh*q mod 2^64, then conditional subtractions of
    4q, 2q, q.  Restated with python integers: the estimate is at most 5 short of floor(S/q) and never above it, so
    r < 8q and three conditional subtractions finish the job -- for 31..60-bit primes, random and extreme S
    (0, q-1, q, 8q^2-1, products of (q-1)s as the tensor product and the key switch form them)."""
    import random
    rnd = random.Random(5)

    def red(S, q):
        k = q.bit_length()
        mu63 = (1 << (63 + k)) // q
        assert mu63 < (1 << 64)
        xt = S >> (k - 1)
        assert xt < (1 << 64)
        xl, xh = xt & 0xffffffff, xt >> 32
        ml, mh = mu63 & 0xffffffff, mu63 >> 32
        qh = (xh * mh + ((xh * ml) >> 32) + ((xl * mh) >> 32)) & ((1 << 64) - 1)
        true_q = S // q
        assert true_q - 5 <= qh <= true_q, (S, q, true_q - qh)
        r = (S - qh * q) & ((1 << 64) - 1)
        assert r == S - qh * q and r < 8 * q
        for m in (4 * q, 2 * q, q):
            if r >= m:
                r -= m
        return r
    for bits, m in ((60, 32768), (59, 65536), (56, 32768), (49, 16384), (36, 16384), (31, 4096)):
        g = O.PrimeGen(bits, m)
        for _ in range(3):
            q = g.next()
            edge = [0, 1, q - 1, q, q + 1, 8 * q * q - 1, (q - 1) * (q - 1), 2 * (q - 1) * (q - 1), 7 * (q - 1) * (q - 1) + q - 1]
            for S in edge + [rnd.randrange(8 * q * q) for _ in range(4000)]:
                assert red(S, q) == S % q


def test_unreduced_words_of_the_rns_kernels_restated():
    """The round-4 "lazy" hand-overs between kernels (helib_amd/csrc/rns_kernels.h), restated with python integers --
    every value the device code leaves unreduced stays inside the 64-bit word and inside the bound its reader is
    declared with, and is congruent to what the reduced form would have been:
      * red128_q8_lazy: S - qh q in [0,6q) for S < 8 q^2 (break_digits_fast_kernel<., true>, the tensor fold of
        keyswitch_kernel, ExtArgs::lazy_out);
      * red128_any_lazy: shoup4(H, 2^64 mod q) + norm_any(Lo) in [0,5q) for any S < 2^127;
      * mul_shoup with an unreduced operand (any 64-bit x): x c - floor(x c' / 2^64) q in [0,2q), so ONE conditional
        subtraction gives x c mod q -- the key switch scales [0,6q) products with it and rebuilds its own digit from
        own + q - x (own in [0,6q), x in [0,q));
      * the plaintext-space correction on a lazy word: r + corr and r + q - corr stay below 7q (LOAD_BOUND 8);
      * the in-place fix-up of the later digits' rows: u + 8q - v for u in [0,q), v in [0,6q) is positive and below
        2^64, and shoup4 of it lands in [0,4q)."""
    import random
    rnd = random.Random(11)
    M64 = (1 << 64) - 1

    def red_q8_lazy(S, q):
        k = q.bit_length()
        mu63 = (1 << (63 + k)) // q
        xt = S >> (k - 1)
        xl, xh = xt & 0xffffffff, xt >> 32
        ml, mh = mu63 & 0xffffffff, mu63 >> 32
        qh = (xh * mh + ((xh * ml) >> 32) + ((xl * mh) >> 32)) & M64
        return (S - qh * q) & M64

    def shoup4(y, w, q):                       # ntt_core.h: approximate high product, result in [0,4q)
        wp = (w << 64) // q
        yl, yh = y & 0xffffffff, y >> 32
        pl, ph = wp & 0xffffffff, wp >> 32
        h = yh * ph + ((yh * pl) >> 32) + ((yl * ph) >> 32)
        return (y * w - h * q) & M64

    def norm_any(x, q):                        # any 64-bit x -> [0,q), q > 2^32
        mu32 = (1 << 64) // q
        assert mu32 < (1 << 32)
        e = (x * mu32) >> 64
        r = x - e * q
        assert 0 <= r < 2 * q
        return r - q if r >= q else r

    def mul_shoup_raw(x, c, q):
        cp = (c << 64) // q
        return x * c - ((x * cp) >> 64) * q

    for bits, m in ((60, 32768), (59, 65536), (56, 32768), (45, 16384), (36, 16384)):
        g = O.PrimeGen(bits, m)
        for _ in range(3):
            q = g.next()
            r64 = (1 << 64) % q
            for _ in range(1500):
                S = rnd.choice([rnd.randrange(8 * q * q), 8 * q * q - 1, 7 * (q - 1) ** 2 + q - 1, 0, q])
                r = red_q8_lazy(S, q)
                assert r < 6 * q and r % q == S % q
                # the same word scaled by a Shoup constant without reducing it first
                c = rnd.randrange(1, q)
                for x in (r, 6 * q - 1, M64, rnd.randrange(1 << 64)):
                    t = mul_shoup_raw(x, c, q)
                    assert 0 <= t < 2 * q and t % q == x * c % q
                # own + q - x inside mul_shoup; the plaintext-space correction on a lazy word
                xx, corr = rnd.randrange(q), rnd.randrange(q)
                assert 0 < r + q - xx < 7 * q <= M64
                assert (r + corr) < 7 * q and (r + q - corr) < 7 * q + 1
                assert (r + q - corr) % q == (S - corr) % q
                # later digits' rows: u + 8q - v, then shoup4 with P^-1
                u = rnd.randrange(q)
                y = u + (q << 3) - r
                assert 0 < y <= M64
                t4 = shoup4(y, c, q)
                assert t4 < 4 * q and t4 % q == (u - S) * c % q
            for _ in range(1500):
                S = rnd.choice([rnd.randrange(1 << 127), (1 << 127) - 1, rnd.randrange(1 << 70), 0])
                H, Lo = S >> 64, S & M64
                h4 = shoup4(H, r64, q)
                assert h4 < 4 * q
                r = h4 + norm_any(Lo, q)
                assert r < 5 * q and r % q == S % q


def test_one_word_form_of_the_mod_down_correction_restated():
    """moddown_S_of (helib_amd/csrc/ntt_kernels.hip) for a plaintext space below 2^32: S = [x > (qd-1)/2] +
    balanced((delta mod p) qd^-1 mod p) with red64 (one high product and one conditional subtraction) on x, and on the
    ONE-WORD product r * (qd^-1 mod p) < 2^64 instead of the 128-bit Barrett -- restated with python integers against
    the definition (src/DoubleCRT.cpp:1098-1099, :1485-1508) for odd, even and prime-power p, x over the whole range of
    a 60-bit dropped prime."""
    import random
    rnd = random.Random(3)
    M64 = (1 << 64) - 1

    def red64(x, q):
        mu64 = (1 << 64) // q
        r = x - ((x * mu64) >> 64) * q
        assert 0 <= r < 2 * q
        return r - q if r >= q else r
    g = O.PrimeGen(60, 32768)
    for p in (2, 4, 257, 65537, 1 << 16, 3 ** 20, (1 << 32) - 5, 1 << 31):
        qd = g.next()
        half, qd_mod_p, qdinv = (qd - 1) // 2, qd % p, pow(qd % p, -1, p) if p > 1 and (qd % p) and __import__("math").gcd(qd % p, p) == 1 else None
        if qdinv is None:
            continue
        for x in [0, 1, half, half + 1, qd - 1] + [rnd.randrange(qd) for _ in range(3000)]:
            neg = x > half
            S = 1 if neg else 0
            r = red64(x, p)
            assert r == x % p
            if neg:
                r = (r - qd_mod_p) % p
            prod = r * qdinv
            assert prod <= M64
            dm = red64(prod, p)
            assert dm == prod % p
            sub_p = dm > p // 2 or (p % 2 == 0 and dm == p // 2 and neg)
            S += dm - p if sub_p else dm
            # the definition: delta = x - [neg] qd, then the multiple of qd that makes it divisible by p, balanced
            delta = x - qd if neg else x
            dmod = delta % p * qdinv % p
            if dmod > p // 2 or (p % 2 == 0 and dmod == p // 2 and delta < 0):
                dmod -= p
            assert S == (1 if neg else 0) + dmod and (x - qd * S) % p == 0


def test_ckks_verification_is_signal_relative_at_low_precision():
    """at precision(1) the bound a CKKS product reports (O(1)) exceeds its coefficients (~1e-4), so
    "within the bound" accepts an all-zero or a foreign product.  helib_amd.host.ckks_correlation is the second
    criterion of Session.verify / bench.py for r < 10: the decoded product must correlate with the expected one beyond
    8 standard deviations of what an unrelated vector shows (1/sqrt(N))."""
    from helib_amd.host import ckks_correlation
    rng = np.random.default_rng(3)
    n = 32768
    want = rng.normal(0, 1e-4, n)
    thr = 8.0 / np.sqrt(n)
    for snr in (4.0, 1.0, 0.25):                                   # rms signal / rms noise
        got = want + rng.normal(0, 1e-4 / snr, n)
        c = ckks_correlation(got, want)
        assert abs(c - 1 / np.sqrt(1 + 1 / snr ** 2)) < 0.02 and c > thr
    assert ckks_correlation(np.zeros(n), want) == 0.0 < thr                       # an all-zero product
    assert abs(ckks_correlation(rng.normal(0, 1e-4, n), want)) < thr              # a product of other operands
    assert abs(ckks_correlation(rng.normal(0, 3e-4, n), want)) < thr              # noise alone


# ---------------------------------------------------------------- round 6: config 5 without Bluestein
@pytest.fixture(scope="module")
def pfa_replay():
    src = os.path.join(ROOT, "tests", "cpp", "pfa_replay.cpp")
    so = os.path.join(ROOT, "tests", "cpp", "libpfa_replay.so")
    hdrs = [os.path.join(ROOT, "helib_amd", "csrc", h) for h in ("pfa_core.h", "ntt_core.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DHX_CHECK_BOUNDS", "-shared", "-fPIC", "-o", so, src])
    L = C.CDLL(so)
    for f in (L.pfa_replay_forward, L.pfa_replay_inverse, L.pfa_replay_inverse_rem):
        f.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    L.pfa_supported.argtypes = [C.c_uint64, C.c_uint64]
    return L


@pytest.mark.parametrize("m", [85, 255, 1285, 4369])
def test_good_thomas_rader_restated_in_python_integers(m):
    """Cmodulus::FFT / iFFT (src/CModulus.cpp:431-443, 555-577) of an m that is a product of distinct Fermat primes as
    Good-Thomas x Rader (tests/pfa_ref.py): DFT_p1 (x) ... (x) DFT_pr with each DFT_p at its non-zero outputs ONE cyclic
    convolution of length p - 1 (a power of two), and rem Phi_m as binomial passes -- against the oracle's Bluestein
    restatement, every word, forward and inverse, including the extreme rows."""
    import pfa_ref as R
    assert R.is_fermat_product(m) and not R.is_fermat_product(32003) and not R.is_fermat_product(2 * 85)
    g = O.PrimeGen(60, m)
    for n in range(2):
        q = g.next()
        cm = O.Cmod(m, q)
        P = R.Pfa(m, q, cm.root)
        assert P.phim == cm.phim
        for x in (O.fill_uniform(cm.phim, q, 3 + n), np.full(cm.phim, q - 1, dtype=np.uint64)):
            y = cm.fft(x)
            assert P.forward([int(v) for v in x]) == [int(v) for v in y]
            X = P.inverse_full([int(v) for v in y])
            # X is the length-m inverse transform of y scattered onto Z_m^*: it vanishes at the non-units ...
            zeta = cm.root * cm.root % q
            j = next(j for j in range(1, m) if j not in P.rank)
            acc = 0
            for c in reversed(X):
                acc = (acc * pow(zeta, j, q) + c) % q
            assert acc == 0
            # ... and both forms of rem Phi_m give the coefficients back (long division; binomial passes)
            phi = [int(v) % q for v in O.phimx(m)]
            assert R.rem_phi_times_minv(X, phi, m, q) == [int(v) for v in x]
            assert R.rem_by_binomials(X, m, q) == [int(v) for v in x]


def test_good_thomas_rader_restatement_at_config5():
    """the same at BASELINE config 5's own m = 21845 = 5 * 17 * 257 (one prime, python integers: ~2 s)"""
    import pfa_ref as R
    m = 21845
    q = O.PrimeGen(60, m).next()
    cm = O.Cmod(m, q)
    P = R.Pfa(m, q, cm.root)
    x = O.fill_uniform(cm.phim, q, 11)
    y = cm.fft(x)
    assert P.forward([int(v) for v in x]) == [int(v) for v in y]
    assert R.rem_by_binomials(P.inverse_full([int(v) for v in y]), m, q) == [int(v) for v in x]
    assert R.phi_binomials(m) == ([5, 17, 257, 21845], [1, 85, 1285, 4369])


def test_good_thomas_rader_kernel_phases_replayed_on_cpu(pfa_replay):
    """The phase functions of pfa_row_kernel<0 / 1 / 2> (helib_amd/csrc/pfa_core.h: forward; inverse up to X; inverse
    with rem Phi_m and 1/m fused), run thread by thread with a vector for the LDS and every compile-time bound asserted
    (HX_CHECK_BOUNDS aborts the process on a violation), on the tables the engine uploads (pfa::host::build_*): equal to
    the oracle on chain primes of PrimeGenerator(60, 21845) -- random, all-(q-1), zero and single-one rows."""
    import pfa_ref as R
    m = 21845
    g = O.PrimeGen(60, m)
    for n in range(3):
        q = g.next()
        assert pfa_replay.pfa_supported(m, q) == 1
        cm = O.Cmod(m, q)
        one = np.zeros(cm.phim, dtype=np.uint64)
        one[(977 * (n + 1)) % cm.phim] = 1
        for x in (O.fill_uniform(cm.phim, q, 7 + n), np.full(cm.phim, q - 1, dtype=np.uint64),
                  np.zeros(cm.phim, dtype=np.uint64), one):
            y = cm.fft(x)
            out = np.zeros(cm.phim, dtype=np.uint64)
            assert pfa_replay.pfa_replay_forward(q, cm.root, x.ctypes.data, out.ctypes.data) == 0
            assert np.array_equal(out, y)
            back = np.zeros(cm.phim, dtype=np.uint64)
            assert pfa_replay.pfa_replay_inverse_rem(q, cm.root, y.ctypes.data, back.ctypes.data) == 0
            assert np.array_equal(back, x)
            # evaluations that are not the image of a small polynomial: x itself as the evaluation row
            assert pfa_replay.pfa_replay_inverse_rem(q, cm.root, x.ctypes.data, back.ctypes.data) == 0
            assert np.array_equal(back, cm.ifft(x))
        # the unfused inverse: X (all m words) as the python restatement has it
        y = cm.fft(O.fill_uniform(cm.phim, q, 31 + n))
        X = np.zeros(m, dtype=np.uint64)
        assert pfa_replay.pfa_replay_inverse(q, cm.root, y.ctypes.data, X.ctypes.data) == 0
        if n == 0:
            assert [int(v) for v in X] == R.Pfa(m, q, cm.root).inverse_full([int(v) for v in y])
    # primes that are not of the Proth form (the 36- / 40- / 48-bit small primes of a chain: t m 2^k + 1 with k < 32) take
    # the generic Montgomery product (pfa_core.h QCG) under the same bound schedules; the same forced onto a 60-bit prime
    pfa_replay.pfa_force_generic.argtypes = [C.c_int]
    for bits, force in ((40, 0), (48, 0), (36, 0), (60, 1)):
        pfa_replay.pfa_force_generic(force)
        q = O.PrimeGen(bits, m).next()
        assert pfa_replay.pfa_supported(m, q) == 1 and (bits == 60 or (q & 0xffffffff) != 1)
        cm = O.Cmod(m, q)
        for x in (O.fill_uniform(cm.phim, q, 3), np.full(cm.phim, q - 1, dtype=np.uint64)):
            y, out, back = cm.fft(x), np.zeros(cm.phim, dtype=np.uint64), np.zeros(cm.phim, dtype=np.uint64)
            assert pfa_replay.pfa_replay_forward(q, cm.root, x.ctypes.data, out.ctypes.data) == 0 and np.array_equal(out, y)
            assert pfa_replay.pfa_replay_inverse_rem(q, cm.root, y.ctypes.data, back.ctypes.data) == 0 and np.array_equal(back, x)
    pfa_replay.pfa_force_generic(0)
    # a prime without the 256-th roots of unity is refused: Bluestein serves it
    assert pfa_replay.pfa_supported(m, 21845 * 2 * 17 + 1) == 0


# ---------------------------------------------------------------- round 6: the work maps at the timed launch shapes
def test_work_maps_are_bijections_at_every_launch_shape():
    """md_tile / md_work (the 2-D XCD tiling of ntt_moddown_apply_kernel and ntt_moddown_apply_tensor_kernel) and
    xcd_remap (every other row kernel) are functions of the LAUNCH SIZE: the batch-128 / batch-64 launches bench.py
    times run different index arithmetic from the batch-4 / batch-2 launches most parity tests pin.  Compiled for the
    host (helib_amd/csrc/work_map.h has no HIP types): every (row, element) of a launch is handed to exactly one
    workgroup, for the shapes of the benchmark legs -- bits = 950 at batch 128 (16 / 22 rows x 256 / 384 elements),
    CKKS 1400 at batch 64 (24 / 21 / 14 rows x 128 / 192), bits = 6400 at batch 16, CKKS 440 -- and for a sweep around
    them; the 1-D remap is one-to-one and keeps each XCD on one contiguous range for every grid size up to 4096 and
    for the line's own 8192 / 6144 / 6400 / 2048 / 16384 / 7168 / 5376 / 4608 (src/Ctxt.cpp:1681-1774 is what these
    launches compute)."""
    src = os.path.join(ROOT, "tests", "cpp", "work_map_test.cpp")
    so = os.path.join(ROOT, "tests", "cpp", "libwork_map_test.so")
    hdr = os.path.join(ROOT, "helib_amd", "csrc", "work_map.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    L = C.CDLL(so)
    L.check_md_work.restype = C.c_long
    L.check_md_work.argtypes = [C.c_uint, C.c_uint, C.c_void_p]
    for nwg in list(range(1, 4097)) + [8192, 6144, 6400, 2048, 16384, 7168, 5376, 4608, 12288, 24576, 65536 + 3]:
        assert L.check_xcd_remap(nwg) == 0, nwg
        assert L.check_xcd_remap_contiguous(nwg) == 0, nwg
    pad = C.c_uint(0)
    named = [(16, 384), (16, 256), (22, 256), (15, 384), (15, 256), (24, 192), (24, 128), (21, 192), (21, 128), (14, 192),
             (14, 128), (32, 128), (107, 48), (143, 32), (72, 48), (8, 192), (8, 128), (11, 128), (5, 192)]
    sweep = [(nk, npb) for nk in range(1, 65) for npb in (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512)]
    for nk, npb in named + sweep:
        grid = L.check_md_work(nk, npb, C.byref(pad))
        assert grid > 0, (nk, npb, grid)
        assert grid - pad.value == nk * npb
        assert pad.value < 8 * (nk + npb) + 64, (nk, npb, grid, pad.value)   # uneven tiles idle a fringe, not a share
    # the dominant launch of the headline: 16 kept rows x 3 parts x 128 elements = 6144 workgroups, none idle
    assert L.check_md_work(16, 384, C.byref(pad)) == 6144 and pad.value == 0


# ---------------------------------------------------------------- round 6: the basis extension as an int8 matrix product
def test_mfma_basis_extension_limb_split_tables_and_recombination():
    """helib_amd/csrc/mfma_ext.h (what rns_mfma_kernels.hip computes with V_MFMA_I32_32X32X32_I8): the exact basis
    extension from 4..40 source primes -- addPrimes / scaleDownToSet / breakIntoDigits at the reference's own
    benchmark chain, src/DoubleCRT.cpp:565-599, benchmarks/bgv_basic.cpp:247 -- with y_k and the pre-reduced
    multipliers W_kt 2^(8a) mod t in balanced 8-bit limbs.  Compiled for the host, the MFMA restated as a triple
    loop over its operand layout: the host-built operand table and accumulator start values, the packing of y, the
    register -> (target, limb) map, the 80-bit recombination and its bounds, and
    sum_k y_k W_kt + cnt (-P) mod t for every (coefficient, target) -- random instances and the extreme ones (all
    y = p_k - 1, cnt = n + 1, multipliers t - 1 - k), 60-bit sources onto 60- / 56- / 45- / 33-bit targets."""
    src = os.path.join(ROOT, "tests", "cpp", "mfma_ext_test.cpp")
    so = os.path.join(ROOT, "tests", "cpp", "libmfma_ext_test.so")
    hdr = os.path.join(ROOT, "helib_amd", "csrc", "mfma_ext.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src])
    L = C.CDLL(so)
    L.mfma_ext_check.argtypes = [C.c_int] * 6 + [C.c_uint64, C.c_int, C.c_void_p]
    mx = C.c_uint32(0)
    for n in (4, 6, 7, 8, 9, 11, 12, 16, 17, 19, 20, 24, 25, 33, 36, 39, 40):
        steps = (n + 1 + 3) // 4
        for nt, tb in ((11, (60, 56, 45)), (107, (60, 60, 60)), (5, (33, 40, 59)), (143, (60, 59, 58))):
            for worst in (0, 1, 2):
                assert L.mfma_ext_check(n, nt, 60, *tb, 7 + n, worst, C.byref(mx)) == 0, (n, nt, tb, worst)
                # every start-offset limb sum is a non-negative number below 2^23.5: a01 = S0 + (S1 << 8) fits 32 bits
                assert mx.value < 2 * steps * 32 * 16384 + 256 < 2 ** 23.5
    assert L.mfma_ext_check(3, 4, 60, 60, 60, 60, 1, 0, None) == 100     # one step: below the kernels' range
