"""hx_lin_comb and helib_amd.polyeval on the device, against python integers (tests/polyeval_ref.py), the call sequence the
kernel replaces and the plain evaluation of the polynomials per slot.  Everything here is an integer: every comparison is
exact.

Chain sizes of the homomorphic runs (c = 2, as the host fixtures): bits = 100 for 11^2 and for 2^4, 200 for 19^2 and 31^2,
the smallest multiples of 100 at which the unfused path keeps a positive capacity on the CPU (the digits of 11^2 keep 27
and 31 bits; 19^2 and 31^2 end below zero at 100 and keep 116 / 120 and 107 / 112 bits at 200)."""
import ctypes as C

import numpy as np
import pytest

from helib_amd import hostnt

from tests import polyeval_ref as R

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


# ---- (a) hx_lin_comb against python integers where its indices move ----
LC_M, LC_N, LC_PRIMES = 1031, 1030, 104      # phi(1031) = 1030: 515 two-word vectors, three workgroup columns


@pytest.fixture(scope="module")
def lc_ring(hx):
    """m = 1031 with 104 primes of mixed widths: 60 bits, and 56, 45, 38 bits at every eighth index (7, 15, ...)"""
    gens = {b: hostnt.PrimeGen(b, LC_M) for b in (60, 56, 45, 38)}
    narrow = {i: (56, 45, 38)[i // 8 % 3] for i in range(7, LC_PRIMES, 8)}
    g = hx.Context(LC_M)
    for i in range(LC_PRIMES):
        g.add_prime(gens[narrow.get(i, 60)].next())
    assert g.phim == LC_N and len(set(g.primes)) == LC_PRIMES
    assert {g.primes[i].bit_length() for i in narrow} == {56, 45, 38}
    assert all(g.primes[i].bit_length() == 60 for i in range(LC_PRIMES) if i not in narrow)
    return g, set(narrow)


def _out_idx(kind, rows):
    """a subset of the context's primes in an order that is not the context's: idx[r] != r for every r"""
    if kind == "rev":                                # the last `rows` primes backwards: 103, 102, ...
        return [LC_PRIMES - 1 - r for r in range(rows)]
    return [(37 * r + 7) % LC_PRIMES for r in range(rows)]      # a fixed permutation: 7, 44, 81, 14, ...


def _term_rows(t, n, rows):
    """the output rows term t lives on, in the term's own order.  No term holds row `rows // 2`; term 0 lacks the last
    row; with more than two terms every term leaves out about two rows in five."""
    keep = [r for r in range(rows) if r != rows // 2 and (n <= 2 or (3 * r + 7 * t) % 5 < 3)]
    if t == 0:
        keep = [r for r in keep if r != rows - 1]
    rot = (5 * t + 3) % len(keep)
    keep = keep[rot:] + keep[:rot]
    return keep[::-1] if t & 1 else keep


def _raw_lin_comb(hx, out0, out1, in0, in1, w, addend):
    n = len(in0)

    def arr(ps):
        return (C.c_void_p * n)(*[p.h for p in ps])
    wa = np.array(w, dtype=np.uint64)
    aa = np.array(addend, dtype=np.uint64) if addend is not None else None
    return hx.lib().hx_lin_comb(out0.h, out1.h if out1 is not None else None, arr(in0), arr(in1) if in1 is not None else None,
                                n, wa.ctypes.data_as(C.c_void_p), aa.ctypes.data_as(C.c_void_p) if aa is not None else None)


#           rows, kind, n, B, parts, addend
LC_CASES = [(49, "rev", 1, 1, 1, None), (49, "perm", 2, 5, 2, "max"), (49, "rev", 5, 8, 1, "zero"),
            (49, "perm", 16, 5, 2, "max"), (97, "rev", 2, 1, 2, "zero"), (97, "perm", 5, 5, 2, "max"),
            (97, "perm", 16, 8, 1, None), (97, "rev", 16, 1, 2, "max"), (97, "perm", 1, 8, 2, None),
            (97, "rev", 5, 5, 1, "max")]


@pytest.mark.parametrize("rows,kind,n,B,parts,addend", LC_CASES)
def test_lin_comb_against_python_integers_where_its_indices_move(hx, lc_ring, rows, kind, n, B, parts, addend):
    """A workgroup column takes 256 two-word vectors and a thread 1 or 4 batch elements: 1030 coefficients are three
    columns, the last with 3 live threads; B = 1, 5, 8 are BP = 1, a partial second group and two full ones.  The output
    rows are 49 or 97 of the context's 104 primes, of four widths, in another order; every term has its own subset of
    them in its own order, so the table's row addresses differ term by term."""
    g, narrow = lc_ring
    idx = _out_idx(kind, rows)
    assert len(idx) == rows == len(set(idx)) and all(idx[r] != r for r in range(rows)) and set(idx) & narrow
    assert (LC_N // 2 + 255) // 256 == 3 and LC_N // 2 % 256 == 3
    qs = [g.primes[i] for i in idx]
    rng = np.random.default_rng(10000 * rows + 100 * n + 10 * B + parts)
    tr = [_term_rows(t, n, rows) for t in range(n)]
    covered = set().union(*map(set, tr))
    assert rows // 2 not in covered and rows - 1 not in tr[0] and (n == 1 or rows - 1 in covered)
    assert all(rws != sorted(rws) for rws in tr)
    tidx = [[idx[r] for r in rws] for rws in tr]
    hot = tr[0][0]                                   # a row where everything is q - 1: the accumulator's largest value
    data = []
    for t in range(n):
        per_part = []
        for _ in range(parts):
            x = np.stack([rng.integers(0, qs[r], size=(B, LC_N), dtype=np.uint64) for r in tr[t]])
            x[:, -1, -2:] = [[qs[r] - 1, 0] for r in tr[t]]              # the last vector of the last element of every row
            x[(t + 1) % len(tr[t])] = 0                                  # a row of zeros ...
            if hot in tr[t]:
                x[tr[t].index(hot)] = qs[hot] - 1                        # ... and a row of q - 1
            per_part.append(x)
        data.append(per_part)
    w = [[int(rng.integers(0, q)) for q in qs] for _ in range(n)]
    for t in range(n):
        w[t][hot] = qs[hot] - 1
    w[0][tr[0][1]], w[0][tr[0][2]] = 0, 1                                # 0, 1 and q - 1 in different rows
    r1, r0 = [r for r in tr[-1] if r != hot][3:5]
    w[-1][r1], w[-1][r0] = 1, 0
    add = None if addend is None else [0] * rows if addend == "zero" else [q - 1 for q in qs]
    want = [R.lin_comb_packed([d[k] for d in data], tidx, idx, w, add if k == 0 else None, g.primes) for k in range(parts)]
    # one word by hand: the hot row holds n' (q - 1)^2 + addend, n' the terms that cover it
    cover = sum(hot in rws for rws in tr)
    q = qs[hot]
    assert int(want[0][hot, 0, 0]) == (cover * (q - 1) ** 2 + (add[hot] if add else 0)) % q
    assert not want[0][rows // 2].any() if addend != "max" else (want[0][rows // 2] == qs[rows // 2] - 1).all()
    ins = [[hx.DoubleCRT(g, tidx[t], B, data[t][k]) for t in range(n)] for k in range(parts)]
    bystander = np.stack([rng.integers(0, q, size=(B, LC_N), dtype=np.uint64) for q in qs])
    before = hx.DoubleCRT(g, idx, B, bystander)
    outs = [hx.DoubleCRT(g, idx, B, bystander) for _ in range(parts)]   # (overwritten, not read)
    after = hx.DoubleCRT(g, idx, B, bystander)
    assert _raw_lin_comb(hx, outs[0], outs[1] if parts == 2 else None, ins[0], ins[1] if parts == 2 else None, w, add) == 0, \
        hx.lib().hx_last_error()
    for k in range(parts):
        got = outs[k].download()
        bad = np.argwhere(got != want[k])
        assert not len(bad), "part %d: %d words differ, the first at [row, element, word] %s" % (k, len(bad), bad[0])
        for t in range(n):
            assert np.array_equal(ins[k][t].download(), data[t][k])     # the inputs are left as they were
    assert np.array_equal(before.download(), bystander) and np.array_equal(after.download(), bystander)
    # the binding: new outputs on idx
    o0, o1 = hx.linComb(ins[0], ins[1] if parts == 2 else None, idx, w, add)
    assert o0.getIndexSet() == idx and np.array_equal(o0.download(), want[0])
    assert (o1 is None) if parts == 1 else np.array_equal(o1.download(), want[1])
    if (rows, n, B, parts) == (97, 5, 5, 2):         # the second witness: the calls the kernel replaces
        # weights of the form (product of the primes the term lacks) * c_t, as a mod-up and a multByConstant leave them
        cs = [int(rng.integers(2, 1 << 40)) for _ in range(n)]
        w2 = []
        for t in range(n):
            lack = [i for i in idx if i not in tidx[t]]
            prod = 1
            for i in lack:
                prod *= g.primes[i]
            w2.append([prod * cs[t] % q for q in qs])
        acc = hx.DoubleCRT(g, idx, B)                # zero
        acc.addConstant(add)
        for t in range(n):
            tmp = ins[1][t].copy()
            tmp.addPrimesAndScale([i for i in idx if i not in tidx[t]])
            tmp.mulConstant(cs[t])
            acc += tmp
        o0, _ = hx.linComb(ins[1], None, idx, w2, add)
        assert np.array_equal(o0.download(), acc.download())
        assert np.array_equal(o0.download(), R.lin_comb_packed([d[1] for d in data], tidx, idx, w2, add, g.primes))


def test_lin_comb_takes_lazy_copies_and_256_terms(hx):
    """outputs that still share an input's rows (a lazy hx_poly_copy) let go of them; n = 256 is the most one call takes,
    and with every word and weight q - 1 the 128-bit accumulator holds its largest value"""
    g = hx.Context(85)
    gen = hostnt.PrimeGen(60, 85)
    for _ in range(3):
        g.add_prime(gen.next())
    qs, idx, B = g.primes, [2, 0, 1], 2
    full = np.stack([np.full((B, 64), qs[i] - 1, dtype=np.uint64) for i in idx])
    x = hx.DoubleCRT(g, idx, B, full)
    out = x.copy()
    w = [[qs[i] - 1 for i in idx]] * 256
    add = [qs[i] - 1 for i in idx]
    assert _raw_lin_comb(hx, out, None, [x] * 256, None, w, add) == 0
    assert np.array_equal(x.download(), full)
    want = np.stack([np.full((B, 64), (256 * (qs[i] - 1) ** 2 + qs[i] - 1) % qs[i], dtype=np.uint64) for i in idx])
    assert np.array_equal(out.download(), want)
    assert _raw_lin_comb(hx, out, None, [x] * 257, None, w + w[:1], add) == hx.HX_ERR_UNSUPPORTED
    assert b"256" in hx.lib().hx_last_error()
    assert np.array_equal(out.download(), want)


def test_lin_comb_refusals_touch_nothing(hx):
    g = hx.Context(85)
    other = hx.Context(85)
    gen = hostnt.PrimeGen(60, 85)
    for q in [gen.next() for _ in range(4)]:
        g.add_prime(q)
        other.add_prime(q)
    qs = g.primes
    rng = np.random.default_rng(2)

    def rnd(ctx=g, idx=(0, 1, 2), B=2):
        return hx.DoubleCRT(ctx, list(idx), B, np.stack([rng.integers(0, ctx.primes[i], size=(B, 64), dtype=np.uint64) for i in idx]))
    o0, o1, a0, a1, b0, b1 = rnd(), rnd(), rnd(), rnd(), rnd(idx=(2, 0)), rnd(idx=(2, 0))
    polys = (o0, o1, a0, a1, b0, b1)
    keep = [x.download() for x in polys]
    w = [[1, 2, 3], [4, 5, 6]]
    L = hx.lib()
    INV, UNS = hx.HX_ERR_INVALID, hx.HX_ERR_UNSUPPORTED

    def call(out0, out1, in0, in1, w=w, addend=None):
        return _raw_lin_comb(hx, out0, out1, in0, in1, w, addend)
    null = type("Null", (), {"h": None})()
    assert call(null, None, [a0, b0], None) == INV and call(o0, None, [a0, null], None) == INV
    assert L.hx_lin_comb(o0.h, None, None, None, 2, None, None) == INV
    arr = (C.c_void_p * 2)(a0.h, b0.h)
    assert L.hx_lin_comb(o0.h, None, arr, None, 2, None, None) == INV and b"null" in L.hx_last_error()
    assert call(o0, o1, [a0, b0], None) == INV and b"go together" in L.hx_last_error()
    assert call(o0, None, [a0, b0], [a1, b1]) == INV and b"go together" in L.hx_last_error()
    assert L.hx_lin_comb(o0.h, None, arr, None, 0, None, None) == INV
    assert call(o0, o0, [a0, b0], [a1, b1]) == INV and b"the same poly" in L.hx_last_error()
    assert call(o0, None, [a0, o0], None) == INV and b"also an input" in L.hx_last_error()
    assert call(o0, o1, [a0, b0], [a1, o1]) == INV and call(o0, o1, [a0, b0], [o0, b1]) == INV
    assert call(o0, None, [a0, rnd(other)], None) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(o0, rnd(other), [a0, b0], [a1, b1]) == INV
    assert call(o0, None, [a0, rnd(B=3)], None) == INV and b"batch" in L.hx_last_error()
    assert call(o0, rnd(B=1), [a0, b0], [a1, b1]) == INV and call(o0, rnd(idx=(0, 2, 1)), [a0, b0], [a1, b1]) == INV
    assert b"out0 and out1 differ" in L.hx_last_error()
    assert call(o0, o1, [a0, b0], [a1, rnd(idx=(0, 2))]) == INV and b"differs from in0" in L.hx_last_error()
    assert call(o0, None, [a0, rnd(idx=(0, 3))], None) == hx.HX_ERR_PRIMESET and b"prime 3" in L.hx_last_error()
    assert call(o0, None, [a0, b0], None, w=[[1, qs[1], 3], [4, 5, 6]]) == INV and b"not reduced" in L.hx_last_error()
    assert call(o0, None, [a0, b0], None, addend=[0, 0, qs[2]]) == INV and b"not reduced" in L.hx_last_error()
    # more rows than one launch descriptor holds
    big = hx.Context(85)
    gen = hostnt.PrimeGen(50, 85)
    for _ in range(161):
        big.add_prime(gen.next())
    wide, narrow = hx.DoubleCRT(big, range(161), 1), hx.DoubleCRT(big, [5], 1)
    assert _raw_lin_comb(hx, wide, None, [narrow], None, [[0] * 161], None) == UNS and b"too many rows" in L.hx_last_error()
    # an odd number of coefficients: phi(m) is odd for m = 2 only (phi = 1); polys without rows reach the check
    tiny = hx.Context(2)
    assert tiny.phim == 1
    ta, tb = (hx.DoubleCRT(tiny, [], 1, zero=False) for _ in range(2))
    assert _raw_lin_comb(hx, ta, None, [tb], None, [[0]], None) == UNS
    assert b"hx_lin_comb needs an even number of coefficients" in L.hx_last_error()
    # a call during a graph capture
    g.graphBegin()
    try:
        assert call(o0, None, [a0, b0], None) == UNS and b"cannot be captured" in L.hx_last_error()
    finally:
        try:
            g.graphEnd().destroy()
        except hx.HxError:
            pass
    with pytest.raises(hx.InvalidArgument, match="one weight per term"):
        hx.linComb([a0, b0], None, [0, 1, 2], [[1, 2, 3]])
    for x, k in zip(polys, keep):
        assert np.array_equal(x.download(), k)
    assert call(o0, o1, [a0, b0], [a1, b1], addend=[7, 8, 9]) == 0          # and the context still works
    want = R.lin_comb([keep[2], keep[4]], [[0, 1, 2], [2, 0]], [0, 1, 2], w, [7, 8, 9], qs)
    assert np.array_equal(o0.download(), want)
    assert np.array_equal(o1.download(), R.lin_comb([keep[3], keep[5]], [[0, 1, 2], [2, 0]], [0, 1, 2], w, None, qs))


# ---- (b) homomorphic runs ----
def _chain(hx, m, p, r, bits, seed=5):
    from helib_amd import bgv_pr, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, r, bits=bits, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    ea = bgv_pr.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    return cc, g, sk, ea


def _state(ct):
    return ct.lnNoise, ct.primeSet, ct.ptxtSpace, ct.intFactor, ct.ptxtMag


def _same_words(x, y):
    wx = {h: (part.getIndexSet(), part.download()) for h, part in x.parts.items()}
    wy = {h: (part.getIndexSet(), part.download()) for h, part in y.parts.items()}
    assert wx.keys() == wy.keys()
    assert all(wx[h][0] == wy[h][0] and np.array_equal(wx[h][1], wy[h][1]) for h in wx)


def _count(hx, monkeypatch):
    seen = []
    real = hx.linComb
    monkeypatch.setattr(hx, "linComb", lambda *args: (seen.append(args), real(*args))[1])
    return seen


@pytest.mark.parametrize("p,bits,k,pow2", [(11, 100, 2, False), (19, 200, 4, False), (31, 200, 4, True)])
def test_extract_digits_above_three_fused_and_unfused(hx, monkeypatch, p, bits, k, pow2):
    """m = 80, r = 2, B = 3: digits[0] goes through polyEval of the digit polynomial of degree p -- k baby steps; at
    p = 31 n = 8 is a power of two (degPowerOfTwo), at 11 and 19 the general recursion with the extra term"""
    import math
    from helib_amd import polyeval
    cc, g, sk, ea = _chain(hx, 80, p, 2, bits)
    B, n, P = 3, ea.size(), p * p
    kk = int(math.sqrt(p / 2.0))
    nn = -(-p // k)
    assert 1 << max(kk - 1, 0).bit_length() == k and (nn & (nn - 1) == 0) == pow2
    a = np.random.default_rng(p).integers(0, P, size=(B, n))
    a[0, :3] = [0, P - 1, P // 2]
    ct = ea.encrypt_batch(sk, a)
    seen = _count(hx, monkeypatch)
    plain = polyeval.extractDigits(ea, ct, fused=False)
    assert not seen                                  # the unfused path never calls the kernel
    fused = polyeval.extractDigits(ea, ct, fused=True)
    assert seen and all(len(args[0]) >= 1 and args[1] is not None for args in seen)
    assert len(fused) == len(plain) == 2
    for j, (x, y) in enumerate(zip(fused, plain)):
        assert _state(x) == _state(y)
        _same_words(x, y)
        assert x.ptxtSpace == p ** (2 - j) and x.bitCapacity() > 0
        got = ea.decrypt_batch(x, sk)
        want = [[R.digits(int(v), p, 2)[j] % p for v in row] for row in a]
        assert [[int(v) % p for v in row] for row in got] == want, j
    assert np.array_equal(ea.decrypt_batch(ct, sk), a)


@pytest.fixture(scope="module")
def k16(hx):
    """m = 85, p^r = 2^4: 8 slots"""
    return _chain(hx, 85, 2, 4, 100)


def test_poly_eval_plain_and_encrypted_coefficients(hx, k16, monkeypatch):
    from helib_amd import polyeval
    cc, g, sk, ea = k16
    B, n, P = 3, ea.size(), 16
    rng = np.random.default_rng(85)
    a = rng.integers(0, P, size=(B, n))
    ct = ea.encrypt_batch(sk, a)
    poly = [5, -3, 0, 8, 1, 16, 7, 2, -6, 3]         # degree 9: units, multiples of 2, zero modulo 16, below zero
    seen = _count(hx, monkeypatch)
    st, st2 = {}, {}
    plain = polyeval.polyEval(ct, poly, fused=False, stats=st)
    assert not seen
    fused = polyeval.polyEval(ct, poly, fused=True, stats=st2)
    assert 0 < len(seen) <= st["leaves"]
    want = [R.plain(row, poly, P) for row in a]
    _, rst = R.replay(a[0], poly, P)
    assert st == st2 == rst
    assert _state(fused) == _state(plain)
    _same_words(fused, plain)
    assert [[int(v) for v in row] for row in ea.decrypt_batch(fused, sk)] == want and fused.bitCapacity() > 0
    # encrypted coefficients, degree 5
    cf = rng.integers(0, P, size=(6, B, n))
    y = polyeval.polyEvalCtxt([ea.encrypt_batch(sk, c) for c in cf], ct)
    want = sum(cf[i].astype(object) * a.astype(object) ** i for i in range(6)) % P
    assert np.array_equal(ea.decrypt_batch(y, sk), want.astype(np.int64)) and y.bitCapacity() > 0


def test_extend_extract_digits(hx, k16):
    from helib_amd import polyeval
    cc, g, sk, ea = k16
    B, n = 3, ea.size()
    a = np.random.default_rng(86).integers(0, 16, size=(B, n))
    a[0, :3] = [0, 15, 10]
    ct = ea.encrypt_batch(sk, a)
    res = {f: polyeval.extendExtractDigits(ea, ct, 2, 2, fused=f) for f in (False, True)}
    for j, (x, y) in enumerate(zip(res[True], res[False])):
        assert _state(x) == _state(y)
        _same_words(x, y)
        assert x.ptxtSpace == 2 ** (4 - j) and x.bitCapacity() > 0
        assert np.array_equal(ea.decrypt_batch(x, sk), (a >> j) & 1), j


def test_add_scalar_and_an_empty_ciphertext(hx, k16):
    cc, g, sk, ea = k16
    B, n, P = 3, ea.size(), 16
    a = np.random.default_rng(87).integers(0, P, size=(B, n))
    ct = ea.encrypt_batch(sk, a)
    ct.addScalar(-5)
    assert np.array_equal(ea.decrypt_batch(ct, sk), (a - 5) % P)
    ct.clear()
    ct.addScalar(3)
    assert list(ct.parts) == ["1"] and ct.parts["1"].batch == B
    assert sorted(ct.parts["1"].getIndexSet()) == sorted(ct.primeSet)
    assert np.array_equal(ea.decrypt_batch(ct, sk), np.full((B, n), 3))
