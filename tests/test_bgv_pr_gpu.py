"""BGV slots modulo p^r on the device (hx_bgv_crt_create_pr, hx_scaled_sub, helib_amd.bgv_pr) against the Hensel-lifting
restatement tests/bgv_pr_ref.py, numpy and the unfused call sequences.  Everything here is an integer: every comparison
is exact."""
import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_pr_ref as R

pytestmark = pytest.mark.gpu
PMAX = 46337        # the largest prime whose square is below 2^31


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


def _ctx(hx, m, nprimes=2, bits=60):
    g = hostnt.PrimeGen(bits, m)
    c = hx.Context(m)
    for _ in range(nprimes):
        c.add_prime(g.next())
    return c


# ---- (a) encode / embed / decode ----
@pytest.mark.parametrize("m,p,r,B", [(85, 2, 4, 17), (127, 2, 3, 17), (85, PMAX, 2, 3)])
def test_encode_embed_decode_against_the_restatement(hx, m, p, r, B):
    ref = R.tables(m, p, r)
    P = p ** r
    c = _ctx(hx, m, 3)
    t = hx.BgvCrt(c, p, r)
    assert (t.prime, t.r, t.p) == (p, r, P)
    assert (t.d, t.nslots, t.gens, t.ords) == (ref.d, ref.nslots, ref.z.gens, ref.z.signedOrds())
    rng = np.random.default_rng(m + r)
    a = rng.integers(-2 ** 63, 2 ** 63 - 1, size=(B, ref.nslots), endpoint=True)     # the whole int64 range
    a[0, :4] = [-1, P // 2, -(P // 2), P - 1][:min(4, ref.nslots)]
    for idx, mul in (([0, 2], 1), ([], 1), ([1], P - 3)):
        want = ref.encode(a, mul)
        d, cf = hx.bgvCrtEncode(t, a, idx, mul, coeffs=True)
        assert np.array_equal(cf, want)
        if idx:
            res = np.stack([np.mod(want, np.int64(c.primes[i])).astype(np.uint64) for i in idx])
            assert np.array_equal(d.download(), hx.DoubleCRT(c, list(idx), B, res).FFT().download())
    want = ref.encode(a)
    assert want.max() <= P // 2 and want.min() > -(P // 2) - (P & 1)          # balanced, +P/2 kept at an even modulus
    slots = np.array([[int(x) % P for x in row] for row in a], dtype=np.int64)
    assert np.array_equal(hx.bgvCrtEmbed(t, want), slots)
    f = rng.integers(-2 ** 63, 2 ** 63 - 1, size=(B, ref.phim), endpoint=True)
    assert np.array_equal(hx.bgvCrtEmbed(t, f), ref.decode(f))
    # hx_bgv_crt_decode: a polynomial on two primes holding small coefficients, times factor_inv
    small = rng.integers(-10 ** 6, 10 ** 6, size=(B, ref.phim))
    res = np.stack([np.mod(small, np.int64(c.primes[i])).astype(np.uint64) for i in (0, 1)])
    acc = hx.DoubleCRT(c, [0, 1], B, res).FFT()
    finv = P - 2
    assert np.array_equal(hx.bgvCrtDecode(t, acc, finv), ref.decode([[int(x) * finv for x in row] for row in small]))


# rings at which the tiles end inside every loop and `limit` = floor(2^64 / p^2r) is small: (m, p, r) -> limit
EDGE = {(341, 2, 30): 16,       # the largest even modulus (+P/2 is kept): 30 slots, 300 coefficients
        (80, 3, 19): 13,        # odd, 3^19 = 1162261467: 8 slots, 32 coefficients, limit no multiple of 4
        (105, 1289, 3): 4}      # odd, 1289^3 = 2141700569 = 2^31 / 1.003: 24 slots, 48 coefficients, 2^64 / P^2 = 4.02


@pytest.fixture(scope="module")
def edge_refs():
    """the restatement's tables, built once (m = 341 at r = 30 takes its 300 idempotent products in python integers)"""
    return {k: R.tables(*k) for k in EDGE}


def _miscounts(ref, kind, x):
    """words of this test's own input x that a reduction left out, and one that comes four terms late, would change"""
    good = ref.kernel_replay(kind, x)
    return (int(np.count_nonzero(ref.kernel_replay(kind, x, drop=True) != good)),
            int(np.count_nonzero(ref.kernel_replay(kind, x, late=4) != good)))


@pytest.mark.parametrize("m,p,r", list(EDGE))
def test_crt_kernels_where_a_tile_ends_and_a_reduction_fires(hx, edge_refs, m, p, r):
    """bgv_crt_encode_kernel / bgv_crt_decode_kernel count `limit` down by four terms at a time and reduce their 64-bit
    accumulators when fewer than four are left.  At all three rings the tiles are partial in every direction (17
    elements: a full tile and a lone element) and whole elements are p^r - 1.  What a miscount of the reductions would
    do to these inputs is replayed on the reference tables first (Tables.kernel_replay):
      (105, 1289, 3)  a reduction left out and one four terms late both change words, in encode and in decode
      (80, 3, 19)     a reduction left out changes decode words (limit = 13: the counter 13, 9, 5, 1 runs out twice in 32
                      terms); four terms late changes nothing, and the 8 terms of an encode sum stay below 2^64
      (341, 2, 30)    nothing shows: 2^30 divides 2^64, so a sum that wraps keeps its residue.  This ring is here for
                      the even modulus (+P/2 kept by the balancing) and for its tile edges, not for the counter"""
    ref, P, B = edge_refs[m, p, r], p ** r, 17
    enc_worst, dec_worst = ref.worst_sums()
    assert min((1 << 64) // (P * P), 0xffffffff) == EDGE[m, p, r] <= 16
    assert ref.nslots % 16 != 0 and ref.nslots % 64 != 0 and ref.phim % 256 != 0 and B % 16 == 1
    assert dec_worst > 2 ** 64
    rng = np.random.default_rng(m + r)
    a = rng.integers(-2 ** 63, 2 ** 63 - 1, size=(B, ref.nslots), endpoint=True)     # the whole int64 range
    a[0] = a[16] = P - 1
    a[1, :4] = [-1, P // 2, -(P // 2), P - 1]
    a[2], a[3] = P // 2, P - P // 2                  # the constants P/2 and -(P/2) (P/2 again at an even modulus)
    f = rng.integers(-2 ** 63, 2 ** 63 - 1, size=(B, ref.phim), endpoint=True)
    f[0] = f[16] = P - 1
    # before the device is touched: what this case can catch, on its own inputs
    enc_miss, dec_miss = _miscounts(ref, "encode", a), _miscounts(ref, "decode", f)
    assert np.array_equal(ref.balanced(ref.kernel_replay("encode", a)), ref.encode(a))
    assert np.array_equal(ref.kernel_replay("decode", f), ref.decode(f))
    if (m, p, r) == (105, 1289, 3):
        assert min(enc_miss) > 0 and min(dec_miss) > 0 and enc_worst > 2 ** 64 and ref.phim % 32 != 0
    elif (m, p, r) == (80, 3, 19):
        assert EDGE[m, p, r] % 4 != 0
        assert ref.phim > 2 * (EDGE[m, p, r] // 4 * 4)                              # the counter runs out twice
        assert dec_miss[0] > 0 and dec_miss[1] == 0
        assert enc_worst < 2 ** 64 and enc_miss == (0, 0)                           # encode cannot wrap here
    else:
        assert enc_worst > 2 ** 64 and ref.phim > 256 and ref.phim % 32 != 0        # the sums do wrap ...
        assert (1 << 64) % P == 0 and enc_miss == dec_miss == (0, 0)                # ... and the residue survives it
    c = _ctx(hx, m, 3)
    t = hx.BgvCrt(c, p, r)
    assert (t.prime, t.r, t.p) == (p, r, P)
    assert (t.d, t.nslots, t.gens, t.ords) == (ref.d, ref.nslots, ref.z.gens, ref.z.signedOrds())
    for idx, mul in (([0, 2], 1), ([], 1), ([1], P - 3)):
        want = ref.encode(a, mul)
        d, cf = hx.bgvCrtEncode(t, a, idx, mul, coeffs=True)
        assert np.array_equal(cf, want), (idx, mul)
        if idx:
            res = np.stack([np.mod(want, np.int64(c.primes[i])).astype(np.uint64) for i in idx])
            assert np.array_equal(d.download(), hx.DoubleCRT(c, list(idx), B, res).FFT().download())
    want = ref.encode(a)
    if P % 2 == 0:                                   # balanced, +P/2 kept at an even modulus
        assert want.max() == P // 2 == want[2, 0] and want.min() > -(P // 2)
    else:                                            # symmetric at an odd one
        assert want.max() == P // 2 == want[2, 0] and want.min() == -(P // 2) == want[3, 0]
    slots = np.array([[int(x) % P for x in row] for row in a], dtype=np.int64)
    assert np.array_equal(hx.bgvCrtEmbed(t, want), slots)
    got = hx.bgvCrtEmbed(t, f)
    assert np.array_equal(got[[0, 16]], ref.decode(f[[0, 16]]))                      # the rows of P - 1 alone, first
    assert np.array_equal(got, ref.decode(f))
    # hx_bgv_crt_decode: a polynomial on two primes holding small coefficients, times factor_inv
    small = rng.integers(-10 ** 6, 10 ** 6, size=(B, ref.phim))
    res = np.stack([np.mod(small, np.int64(c.primes[i])).astype(np.uint64) for i in (0, 1)])
    acc = hx.DoubleCRT(c, [0, 1], B, res).FFT()
    finv = P - 2
    assert np.array_equal(hx.bgvCrtDecode(t, acc, finv), ref.decode([[int(x) * finv for x in row] for row in small]))


def test_create_pr_refusals_and_r1(hx):
    c = _ctx(hx, 85, 2)
    for p, r, code in ((2, 0, hx.HX_ERR_INVALID), (2, -1, hx.HX_ERR_INVALID), (2, 31, hx.HX_ERR_UNSUPPORTED),
                       (46349, 2, hx.HX_ERR_UNSUPPORTED), (15, 2, hx.HX_ERR_INVALID), (5, 2, hx.HX_ERR_INVALID)):
        with pytest.raises(hx.HxError) as e:
            hx.BgvCrt(c, p, r)
        assert e.value.code == code, (p, r)
        if code == hx.HX_ERR_UNSUPPORTED:
            assert "2^31 = 2147483648" in str(e.value)
    with pytest.raises(hx.HxError) as e:
        hx.BgvCrt(c, 15)
    assert e.value.code == hx.HX_ERR_INVALID
    # r = 1 through the new entry is the old table: the same words out of both
    import ctypes as C
    h = C.c_void_p()
    assert hx.lib().hx_bgv_crt_create_pr(c.h, 2, 1, C.byref(h)) == 0
    old = hx.BgvCrt(c, 2)
    new = hx.BgvCrt.__new__(hx.BgvCrt)
    new.context, new.p, new.h, new.nslots = c, 2, h, old.nslots
    a = np.random.default_rng(0).integers(-5, 5, size=(3, old.nslots))
    d0, c0 = hx.bgvCrtEncode(old, a, [0, 1], 1, coeffs=True)
    d1, c1 = hx.bgvCrtEncode(new, a, [0, 1], 1, coeffs=True)
    assert np.array_equal(c0, c1) and np.array_equal(d0.download(), d1.download())
    new.close()


# ---- (b) hx_scaled_sub against the four calls ----
@pytest.mark.parametrize("m,phim", [(85, 64), (127, 126)])
def test_scaled_sub_is_bit_exact_against_the_four_calls(hx, m, phim):
    from helib_amd import ctxt as hc
    cc = hc.ChainContext(m, 2, 1, bits=200, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    assert g.phim == phim
    idx = list(range(len(cc.primes)))            # all chain primes as rows
    qs = [cc.primes[i] for i in idx]
    rng = np.random.default_rng(m)
    special = [0, 1, None]                       # None: q - 1
    for B in (1, 5):
        for parts in (1, 2):
            def rnd():
                return hx.DoubleCRT(g, idx, B, np.stack([rng.integers(0, q, size=(B, phim), dtype=np.uint64) for q in qs]))
            c, t = [rnd() for _ in range(parts)], [rnd() for _ in range(parts)]
            u = [int(rng.integers(0, q)) for q in qs]
            v = [int(rng.integers(0, q)) for q in qs]
            for k in range(min(3, len(qs))):     # 0, 1 and q - 1 in both lists, at different rows
                u[k] = qs[k] - 1 if special[k] is None else special[k]
                v[-1 - k] = qs[-1 - k] - 1 if special[k] is None else special[k]
            want = []
            for x, y in zip(c, t):
                w, y2 = x.copy(), y.copy()
                w.mulConstant(u)
                y2.mulConstant(v)
                w -= y2
                want.append(w.download())
            t_before = [y.download() for y in t]
            c_before = c[0].download()
            hx.scaledSub(c[0], c[1] if parts == 2 else None, t[0], t[1] if parts == 2 else None, u, v)
            for x, w in zip(c, want):
                assert np.array_equal(x.download(), w), (B, parts)
            for y, w in zip(t, t_before):
                assert np.array_equal(y.download(), w)
            # and against python integers: the last row of the first part
            q = qs[-1]
            py = (c_before[-1].astype(object) * u[-1] - t_before[0][-1].astype(object) * v[-1]) % q
            assert np.array_equal(c[0].download()[-1], py.astype(np.uint64))
    # a c that still shares its rows with t (a lazy copy): c takes its own copy, t stays
    t0 = hx.DoubleCRT(g, idx, 2, np.stack([rng.integers(0, q, size=(2, phim), dtype=np.uint64) for q in qs]))
    c0 = t0.copy()
    before = t0.download()
    hx.scaledSub(c0, None, t0, None, [3] * len(qs), [1] * len(qs))
    assert np.array_equal(t0.download(), before)
    assert np.array_equal(c0.download(), np.stack([(before[i].astype(object) * 2 % q).astype(np.uint64) for i, q in enumerate(qs)]))


# ---- (b2) hx_scaled_sub against python integers where its indices move ----
SS_M, SS_N, SS_ROWS, SS_PRIMES = 1031, 1030, 48, 104     # phi(1031) = 1030: 515 two-word vectors, three workgroups


@pytest.fixture(scope="module")
def ss_ring(hx):
    """m = 1031 with 104 primes of mixed widths: 60 bits, and 56, 45, 38 bits at every eighth index (7, 15, ...)"""
    gens = {b: hostnt.PrimeGen(b, SS_M) for b in (60, 56, 45, 38)}
    narrow = {i: (56, 45, 38)[i // 8 % 3] for i in range(7, SS_PRIMES, 8)}
    g = hx.Context(SS_M)
    for i in range(SS_PRIMES):
        g.add_prime(gens[narrow.get(i, 60)].next())
    assert g.phim == SS_N and len(set(g.primes)) == SS_PRIMES
    assert all((g.primes[i].bit_length() < 60) == (i in narrow) for i in range(SS_PRIMES))
    assert {g.primes[i].bit_length() for i in narrow} == {56, 45, 38}
    return g, set(narrow)


def _ss_idx(kind, rows):
    """a subset of the context's primes in an order that is not the context's: idx[r] != r for every r, and rows 48 and
    96 (a launch of their own) fall on narrow primes"""
    if kind == "rev":                                # the last `rows` primes backwards: 103, 102, ...
        return [SS_PRIMES - 1 - r for r in range(rows)]
    return [(37 * r + 7) % SS_PRIMES for r in range(rows)]      # a fixed permutation: 7, 44, 81, 14, ...


def _ss_operands(hx, g, idx, B, parts, rng):
    rows, qs = len(idx), [g.primes[i] for i in idx]
    last, mid = rows - 1, rows // 2

    def rnd():
        return np.stack([rng.integers(0, q, size=(B, SS_N), dtype=np.uint64) for q in qs])
    cd, td = [rnd() for _ in range(parts)], [rnd() for _ in range(parts)]
    for x in cd:
        x[:, -1, -2:] = [[q - 1, 0] for q in qs]     # the last vector of the last element of every row
        x[last], x[2] = qs[last] - 1, 0              # a row of q - 1 (under u = q - 1) and a row of zeros
    for x in td:
        x[:, -1, -2:] = [[1, q - 1] for q in qs]
        x[mid + 1], x[3] = qs[mid + 1] - 1, 0        # a row of q - 1 (under v = q - 1) and a row of zeros
    u = [int(rng.integers(0, q)) for q in qs]
    v = [int(rng.integers(0, q)) for q in qs]
    u[0], v[1] = 0, 0
    u[mid], v[mid + 1] = 1, qs[mid + 1] - 1
    u[last], v[last] = qs[last] - 1, 1
    return qs, cd, td, u, v


SS_CASES = [(48, "rev", 5, 2), (48, "perm", 1, 1), (49, "rev", 5, 2), (49, "perm", 8, 1), (97, "rev", 5, 2),
            (97, "perm", 1, 1), (97, "perm", 5, 2), (97, "perm", 8, 2), (97, "perm", 5, 1)]


@pytest.mark.parametrize("rows,kind,B,parts", SS_CASES)
def test_scaled_sub_against_python_integers_where_its_indices_move(hx, ss_ring, rows, kind, B, parts):
    """One launch takes 48 rows, which it numbers from 0 for its scalars and for the prime of a row, and from row_base
    for the words; a workgroup column takes 256 two-word vectors.  48, 49 and 97 rows: one full launch, a second of
    one row, a third with row_base = 96; 1030 coefficients: three columns, the last with 3 live threads; the rows are
    a subset of the context's primes in another order, of four widths."""
    g, narrow = ss_ring
    idx = _ss_idx(kind, rows)
    chunks = [range(b, min(b + SS_ROWS, rows)) for b in range(0, rows, SS_ROWS)]
    assert len(idx) == rows == len(set(idx)) < SS_PRIMES and idx != sorted(idx)
    assert all(idx[r] != r for r in range(rows))                                 # no row is its own prime index
    assert all(any(idx[r] in narrow for r in ch) for ch in chunks)               # a narrow prime in every launch
    assert len(chunks) == (rows + 47) // 48 and (SS_N // 2 + 255) // 256 == 3 and SS_N // 2 % 256 == 3
    rng = np.random.default_rng(1000 * rows + 10 * B + parts)
    qs, cd, td, u, v = _ss_operands(hx, g, idx, B, parts, rng)
    if len(chunks) == 3:                             # 0, 1 and q - 1 lie in different launches, q - 1 in row 96
        assert rows - 1 == 96 and u[96] == qs[96] - 1 and u[0] == 0 and 48 <= rows // 2 < 96 and u[rows // 2] == 1
    bystander = np.stack([rng.integers(0, q, size=(B, SS_N), dtype=np.uint64) for q in qs])
    before = hx.DoubleCRT(g, idx, B, bystander)
    c = [hx.DoubleCRT(g, idx, B, x) for x in cd]
    t = [hx.DoubleCRT(g, idx, B, x) for x in td]
    after = hx.DoubleCRT(g, idx, B, bystander)
    want = [R.scaled_sub(x, y, u, v, qs).astype(np.uint64) for x, y in zip(cd, td)]
    hx.scaledSub(c[0], c[1] if parts == 2 else None, t[0], t[1] if parts == 2 else None, u, v)
    for k in range(parts):
        got = c[k].download()
        bad = np.argwhere(got != want[k])
        assert not len(bad), "part %d: %d words differ, the first at [row, element, word] %s" % (k, len(bad), bad[0])
        assert np.array_equal(t[k].download(), td[k])
    assert np.array_equal(before.download(), bystander) and np.array_equal(after.download(), bystander)
    if parts == 2 and B == 5:                        # the second witness: the four calls the kernel replaces
        x, y = hx.DoubleCRT(g, idx, B, cd[1]), hx.DoubleCRT(g, idx, B, td[1])
        x.mulConstant(u)
        y.mulConstant(v)
        x -= y
        assert np.array_equal(x.download(), want[1])


def test_scaled_sub_in_a_graph_capture(hx, ss_ring):
    """49 rows: the graph holds two launches, each with its own argument block of scalars; one replay"""
    g, _ = ss_ring
    idx, B = _ss_idx("perm", 49), 5
    rng = np.random.default_rng(49)
    qs, cd, td, u, v = _ss_operands(hx, g, idx, B, 2, rng)
    direct = [hx.DoubleCRT(g, idx, B, x) for x in cd + td]
    hx.scaledSub(direct[0], direct[1], direct[2], direct[3], u, v)      # eagerly once
    want = [R.scaled_sub(x, y, u, v, qs).astype(np.uint64) for x, y in zip(cd, td)]
    assert all(np.array_equal(direct[k].download(), want[k]) for k in range(2))
    ops = [hx.DoubleCRT(g, idx, B, x) for x in cd + td]
    g.graphBegin()
    hx.scaledSub(ops[0], ops[1], ops[2], ops[3], u, v)
    graph = g.graphEnd()
    for d, x in zip(ops, cd + td):                                      # (nothing ran yet)
        d.upload(x)
    graph.launch()
    for k in range(2):
        assert np.array_equal(ops[k].download(), want[k])
        assert np.array_equal(ops[2 + k].download(), td[k])
    graph.destroy()


def test_scaled_sub_refusals_touch_nothing(hx):
    import ctypes as C
    m = 85
    g = _ctx(hx, m, 3)
    other = _ctx(hx, m, 3)
    qs = g.primes
    rng = np.random.default_rng(1)

    def rnd(ctx=g, idx=(0, 1, 2), B=2):
        return hx.DoubleCRT(ctx, list(idx), B, np.stack([rng.integers(0, ctx.primes[i], size=(B, 64), dtype=np.uint64) for i in idx]))
    c0, c1, t0, t1 = rnd(), rnd(), rnd(), rnd()
    keep = [x.download() for x in (c0, c1, t0, t1)]
    ok = np.array([1, 2, 3], dtype=np.uint64)
    L = hx.lib()

    def call(a, b, c, d, u=ok, v=ok):
        def h(x):
            return x.h if x is not None else None
        return L.hx_scaled_sub(h(a), h(b), h(c), h(d), u.ctypes.data_as(C.c_void_p) if u is not None else None,
                               v.ctypes.data_as(C.c_void_p) if v is not None else None)
    INV = hx.HX_ERR_INVALID
    assert call(None, None, t0, None) == INV and call(c0, None, None, None) == INV
    assert call(c0, None, t0, None, u=None) == INV and call(c0, None, t0, None, v=None) == INV
    assert call(c0, c1, t0, None) == INV and b"go together" in L.hx_last_error()
    assert call(c0, None, t0, t1) == INV and b"go together" in L.hx_last_error()
    assert call(c0, None, c0, None) == INV and b"different polys" in L.hx_last_error()
    assert call(c0, c0, t0, t1) == INV and call(c0, c1, t0, t0) == INV and call(c0, c1, t0, c1) == INV
    assert call(c0, None, rnd(other), None) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(c0, None, rnd(B=3), None) == INV and b"batch or prime set" in L.hx_last_error()
    assert call(c0, None, rnd(idx=(0, 1)), None) == INV and call(c0, None, rnd(idx=(0, 2, 1)), None) == INV
    assert call(c0, c1, t0, rnd(B=1)) == INV
    big = np.array([1, qs[1], 3], dtype=np.uint64)
    assert call(c0, None, t0, None, u=big) == INV and b"not reduced" in L.hx_last_error()
    assert call(c0, None, t0, None, v=big) == INV
    # more rows than one launch descriptor holds
    many, gen = hx.Context(85), hostnt.PrimeGen(50, 85)
    for _ in range(161):
        many.add_prime(gen.next())
    wide = [hx.DoubleCRT(many, range(161), 1) for _ in range(2)]
    zeros = np.zeros(161, dtype=np.uint64)
    assert call(wide[0], None, wide[1], None, u=zeros, v=zeros) == hx.HX_ERR_UNSUPPORTED and b"too many rows" in L.hx_last_error()
    # an odd number of coefficients: phi(m) is odd for m = 2 only (phi = 1); polys without rows reach the check
    tiny = hx.Context(2)
    assert tiny.phim == 1
    ta, tb = (hx.DoubleCRT(tiny, [], 1, zero=False) for _ in range(2))
    assert call(ta, None, tb, None) == hx.HX_ERR_UNSUPPORTED
    assert b"hx_scaled_sub needs an even number of coefficients" in L.hx_last_error()
    with pytest.raises(hx.InvalidArgument, match="one u and one v per prime row"):
        hx.scaledSub(c0, None, t0, None, [1, 2], [1, 2, 3])
    for x, w in zip((c0, c1, t0, t1), keep):
        assert np.array_equal(x.download(), w)
    assert call(c0, c1, t0, t1) == 0             # and the state still works
    assert not np.array_equal(c0.download(), keep[0])


# ---- (c) homomorphic operations ----
def _chain(hx, m, p, r, bits, seed=5):
    from helib_amd import bgv_pr, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, r, bits=bits, c=3)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    ea = bgv_pr.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    return cc, g, sk, ea


def test_encrypt_multiply_add_decrypt_and_divide_by_p(hx):
    cc, g, sk, ea = _chain(hx, 85, 2, 4, 300)
    B, n, P = 3, ea.size(), 16
    rng = np.random.default_rng(85)
    a, b, c = rng.integers(0, P, size=(3, B, n))
    ca, cb, cx = ea.encrypt_batch(sk, a), ea.encrypt_batch(sk, b), ea.encrypt_batch(sk, c)
    assert ca.ptxtSpace == P and np.array_equal(ea.decrypt_batch(ca, sk), a)
    prod = ca.clone()
    prod.multiplyBy(cb)
    prod += cx
    assert np.array_equal(ea.decrypt_batch(prod, sk), (a * b + c) % P)
    one = ea.encrypt(sk, a[0])
    ea.multByConstant(one, ea.encodePtxt(b[:1]))
    ea.addConstant(one, ea.encodePtxt(c[:1]))
    assert np.array_equal(ea.decrypt(one, sk), (a[0] * b[0] + c[0]) % P)
    # divideByP on an encryption of 2 a: a mod 8
    dbl = ea.encrypt_batch(sk, 2 * a)
    dbl.divideByP()
    assert dbl.ptxtSpace == 8 and dbl.effectiveR() == 3
    assert np.array_equal(ea.decrypt_batch(dbl, sk), a % 8)
    dbl.multByP()
    assert dbl.ptxtSpace == 16 and np.array_equal(ea.decrypt_batch(dbl, sk), 2 * (a % 8))


def test_rotate_shift_total_sums(hx):
    cc, g, sk, ea = _chain(hx, 85, 2, 2, 300)
    B, n, P = 2, ea.size(), 4
    a = np.random.default_rng(4).integers(0, P, size=(B, n))
    ca = ea.encrypt_batch(sk, a)
    for k in (1, 3, -2):
        ct = ca.clone()
        ea.rotate(ct, k)
        assert np.array_equal(ea.decrypt_batch(ct, sk), np.roll(a, k, axis=1)), k
    ct = ca.clone()
    ea.shift(ct, 3)
    want = np.zeros_like(a)
    want[:, 3:] = a[:, :-3]
    assert np.array_equal(ea.decrypt_batch(ct, sk), want)
    ct = ca.clone()
    ea.totalSums(ct)
    assert np.array_equal(ea.decrypt_batch(ct, sk), np.repeat(a.sum(axis=1, keepdims=True) % P, n, axis=1))


def _words(ct):
    return {h: p.download() for h, p in ct.parts.items()}


def test_extract_digits_fused_and_unfused(hx):
    from helib_amd import bgv_pr
    cc, g, sk, ea = _chain(hx, 85, 2, 3, 300)
    B, n, P = 4, ea.size(), 8
    a = np.random.default_rng(9).integers(0, P, size=(B, n))
    a[0, :3] = [0, 7, 4]
    ct = ea.encrypt_batch(sk, a)
    fused = bgv_pr.extractDigits(ea, ct, fused=True)
    plain = bgv_pr.extractDigits(ea, ct, fused=False)
    assert len(fused) == len(plain) == 3
    for j, (x, y) in enumerate(zip(fused, plain)):
        assert (x.lnNoise, x.primeSet, x.ptxtSpace, x.intFactor) == (y.lnNoise, y.primeSet, y.ptxtSpace, y.intFactor)
        wx, wy = _words(x), _words(y)
        assert wx.keys() == wy.keys() and all(np.array_equal(wx[h], wy[h]) for h in wx)
        assert x.ptxtSpace == 2 ** (3 - j) and x.bitCapacity() > 0
        assert np.array_equal(ea.decrypt_batch(x, sk), (a >> j) & 1), j
    assert np.array_equal(ea.decrypt_batch(ct, sk), a)
    # one fused step against the two calls, words and bookkeeping
    c1, c2, t = ct.clone(), ct.clone(), ea.encrypt_batch(sk, a % 2)
    c1 -= t
    c1.divideByP()
    c2.subDivideByP(t, fused=True)
    assert (c1.lnNoise, c1.primeSet, c1.ptxtSpace, c1.intFactor) == (c2.lnNoise, c2.primeSet, c2.ptxtSpace, c2.intFactor)
    w1, w2 = _words(c1), _words(c2)
    assert all(np.array_equal(w1[h], w2[h]) for h in w1)
    assert np.array_equal(ea.decrypt_batch(c2, sk), a >> 1)


# ---- (d) p = 3, r = 3: intFactors other than 1, balanced residues below zero, cube() ----
@pytest.fixture(scope="module")
def k27(hx):
    """m = 80, p^r = 27: 8 slots, 14 chain primes"""
    cc, g, sk, ea = _chain(hx, 80, 3, 3, 300)
    assert (ea.size(), ea.getPPowR(), len(cc.primes)) == (8, 27, 14)
    return cc, g, sk, ea


def _state(ct):
    return ct.lnNoise, ct.primeSet, ct.ptxtSpace, ct.intFactor


def _same_words(x, y):
    wx, wy = _words(x), _words(y)
    assert wx.keys() == wy.keys() and all(np.array_equal(wx[h], wy[h]) for h in wx)


def test_p3_encrypt_multiply_add_with_int_factors(hx, k27):
    cc, g, sk, ea = k27
    B, n, P = 3, ea.size(), 27
    rng = np.random.default_rng(80)
    a, b, c = rng.integers(0, P, size=(3, B, n))
    a[0, :3], b[0, :3] = [26, 13, 14], [26, 2, 14]
    ca, cb, cx = ea.encrypt_batch(sk, a), ea.encrypt_batch(sk, b), ea.encrypt_batch(sk, c)
    assert ca.ptxtSpace == P and ca.intFactor == 1 and np.array_equal(ea.decrypt_batch(ca, sk), a)
    prod = ca.clone()
    prod.multiplyBy(cb)
    seen = [prod.intFactor]                          # the product takes Q mod 27 into its factor
    prod += cx                                       # unequal factors: the sum harmonises them
    seen.append(prod.intFactor)
    assert np.array_equal(ea.decrypt_batch(prod, sk), (a * b + c) % P)
    prod.multiplyBy(ca)
    seen.append(prod.intFactor)
    assert np.array_equal(ea.decrypt_batch(prod, sk), ((a * b + c) * a) % P)
    one = ea.encrypt(sk, a[0])
    one.multiplyBy(ea.encrypt(sk, b[0]))
    k = 4 if one.intFactor == 2 else 2               # a unit: its inverse moves into the factor, which is not 1 afterwards
    one.multByScalar(k)
    seen.append(one.intFactor)
    assert one.intFactor != 1
    ea.multByConstant(one, ea.encodePtxt(b[:1]))
    ea.addConstant(one, ea.encodePtxt(c[:1]))        # the constant is scaled by intFactor * Q mod 27
    assert np.array_equal(ea.decrypt(one, sk), (k * a[0] * b[0] * b[0] + c[0]) % P)
    assert any(f != 1 for f in seen), seen
    assert prod.isCorrect() and one.isCorrect()


def test_p3_divide_by_p_and_mult_by_p(hx, k27):
    cc, g, sk, ea = k27
    B, n, P = 3, ea.size(), 27
    a = np.random.default_rng(81).integers(0, P, size=(B, n))
    a[0, :3] = [26, 9, 13]
    ct = ea.encrypt_batch(sk, 3 * a % P)
    ct.divideByP()
    assert ct.ptxtSpace == 9 and ct.effectiveR() == 2
    assert np.array_equal(ea.decrypt_batch(ct, sk), a % 9)
    ct.multByP()
    assert ct.ptxtSpace == 27 and ct.effectiveR() == 3
    assert np.array_equal(ea.decrypt_batch(ct, sk), 3 * (a % 9))


def test_p3_extract_digits_fused_and_unfused(hx, k27):
    from helib_amd import bgv_pr
    cc, g, sk, ea = k27
    B, n, p, r, P = 3, ea.size(), 3, 3, 27
    a = np.random.default_rng(82).integers(0, P, size=(B, n))
    a[0, :4] = [26, 5, 13, 14]                       # balanced digits (-1, 0, 0), (-1, -1, 1), (1, 1, 1), (-1, -1, -1)
    a[1, 0] = 5
    assert all((v + 1) % 3 - 1 == -1 for v in (26, 5))
    ct = ea.encrypt_batch(sk, a)
    before, state = _words(ct), _state(ct)
    fused = bgv_pr.extractDigits(ea, ct, fused=True)
    plain = bgv_pr.extractDigits(ea, ct, fused=False)
    assert len(fused) == len(plain) == r
    want = [R.replay(row, p, r) for row in a]
    for j, (x, y) in enumerate(zip(fused, plain)):
        assert _state(x) == _state(y)
        _same_words(x, y)
        M = p ** (r - j)
        assert x.ptxtSpace == M == want[0][j][1] and x.effectiveR() == r - j and x.bitCapacity() > 0
        got = ea.decrypt_batch(x, sk)
        assert [[int(v) for v in row] for row in got] == [[int(v) for v in w[j][0]] for w in want], j
    # the digits are those of the balanced expansion, modulo 3
    x = [[int(v) for v in row] for row in a]
    for j in range(r):
        bal = [[(v + 1) % 3 - 1 for v in row] for row in x]
        assert [[int(v) % 3 for v in w[j][0]] for w in want] == [[d % 3 for d in row] for row in bal], j
        x = [[(v - d) // 3 for v, d in zip(rv, rd)] for rv, rd in zip(x, bal)]
    assert _state(ct) == state and np.array_equal(ea.decrypt_batch(ct, sk), a)      # the input is left as it was
    after = _words(ct)
    assert after.keys() == before.keys() and all(np.array_equal(after[h], before[h]) for h in before)


def test_p3_sub_divide_by_p_with_unequal_int_factors(hx, k27, monkeypatch):
    """c with intFactor 2 and t with intFactor 23 = -4 mod 27: the pair that harmonises them, 2 e1 = 23 e2, is not
    (1, 1), e1 != e2 and one balanced residue is below zero (the search gives e1 = 25 = -2, e2 = 1), so the kernel
    gets u = bal(e1) / 3 != v = bal(e2) / 3"""
    cc, g, sk, ea = k27
    B, n, p, P = 3, ea.size(), 3, 27
    a = np.random.default_rng(83).integers(0, P, size=(B, n))
    a[0, :3] = [26, 5, 14]
    low = a % p
    c = ea.encrypt_batch(sk, a * 2 % P)
    c.multByScalar(pow(2, -1, P))
    t = ea.encrypt_batch(sk, low * 23 % P)
    t.multByScalar(pow(23, -1, P))
    assert (c.intFactor, t.intFactor) == (2, 23)
    assert np.array_equal(ea.decrypt_batch(c, sk), a) and np.array_equal(ea.decrypt_batch(t, sk), low)
    _, _, e1, e2 = c.clone()._alignForAdd(t)
    bal = lambda e: e - P if e > P // 2 else e       # noqa: E731
    assert (e1, e2) != (1, 1) and e1 != e2 and min(bal(e1), bal(e2)) < 0
    assert e1 * c.intFactor % P == e2 * t.intFactor % P
    seen = []
    real = hx.scaledSub
    monkeypatch.setattr(hx, "scaledSub", lambda *args: (seen.append(args), real(*args))[1])
    t_words, t_state = _words(t), _state(t)
    two, one = c.clone(), c.clone()
    two -= t
    two.divideByP()
    assert not seen
    assert one.subDivideByP(t, fused=True) is one
    assert len(seen) == 1
    c0, c1, t0, t1, u, v = seen[0]
    assert c1 is not None and t1 is not None                                        # both parts in the one call
    qs = [cc.primes[i] for i in c0.getIndexSet()]
    assert len(u) == len(v) == len(qs) > 1
    assert any(x != y for x, y in zip(u, v))
    # what reached the kernel is bal(e) / p modulo every row's prime
    assert all(0 <= x < q and x * p % q == bal(e1) % q for x, q in zip(u, qs))
    assert all(0 <= y < q and y * p % q == bal(e2) % q for y, q in zip(v, qs))
    assert _state(one) == _state(two) and one.ptxtSpace == 9
    _same_words(one, two)
    assert np.array_equal(ea.decrypt_batch(one, sk), (a - low) // p % 9)
    assert _state(t) == t_state
    now = _words(t)
    assert all(np.array_equal(now[h], t_words[h]) for h in t_words)
