"""The powerful basis, the slot tables over supplied generators and EvalMap on the device (powerful_kernel,
hx_bgv_gf_create_gens, helib_amd.powerful, helib_amd.evalmap) against tests/powerful_ref.py, the CPU tables of
tests/evalmap_tables.py and numpy on slot arrays.  Everything here is an integer: every comparison is exact.

The shapes of the conversion tests: eleven factorisations (tests/powerful_ref.py: DEVICE_MVECS -- squarefree and odd ones
from 8 words to m = 4641, then (9, 5), (4, 5), (25, 3), (8, 15) and (7, 5, 9, 13)) at 9 rows x batch 3, one item per
workgroup; (3, 5) and (7, 3, 221) at 3 rows x batch 100 and as 300, 1 and 301 rows of host words, where the 256
workgroups walk to a second item with another row's modulus and the buffers of the table grow twice.
tests/test_evalmap_host.py::test_census_of_the_division_passes_the_device_tests_run says which forms of the passes these
reach."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import bgv_hypercube_ref as H
from tests import evalmap_tables as E
from tests import powerful_ref as PR

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


# ---- (f) the device conversion against the definition ----
# (3, 5): 8 words, less than a wave; (3, 35): Phi_105 has a coefficient -2 and m - 1 - phi(m) > phi(m); (7, 3, 65): three
# dimensions; (17, 257): the e = 1 scan over 4369 words, m - 1 - phi(m) < phi(m); (7, 3, 221): fifteen binomials, a composite
# factor; (31): the single-factor identity
# (9, 5), (25, 3): e > 1 in a per-factor dimension; (4, 5), (8, 15): m even, and a factor whose reduction has no binomial
# pass at all; (7, 5, 9, 13): m = 4095, four factors.  The chain of a row test is over p = 2 where m is odd, p = 3 at
# m = 20 and p = 7 at m = 120.
MVECS = [mvec for mvec, _ in PR.DEVICE_MVECS]
WORD_MODULI = (2, 49, (1 << 62) - 57)


@functools.lru_cache(maxsize=None)
def _truth(mvec):
    """three inputs as integers and their two conversions over Z (tests/powerful_ref.py divides once; reduced modulo q
    they are the conversions modulo q): random words below 2^62 (modulo a row's prime: words over its whole range), all
    -1 (q - 1 modulo every q), a single 1 at the exponent phi(m) - 1"""
    n = PR.indexes(mvec).phim
    rng = np.random.default_rng(n)
    ins = [[int(x) for x in rng.integers(0, 1 << 62, size=n)], [-1] * n, [0] * (n - 1) + [1]]
    return ins, [PR.poly_to_powerful(f, mvec, None) for f in ins], [PR.powerful_to_poly(f, mvec, None) for f in ins]


def _mod(rows, q):
    return np.array([[int(x) % q for x in r] for r in rows], dtype=np.uint64)


@pytest.mark.parametrize("mvec,p", PR.DEVICE_MVECS, ids=["mvec%d" % i for i in range(len(PR.DEVICE_MVECS))])
def test_rows_of_a_poly_convert_as_the_definition_does(hx, mvec, p):
    from helib_amd import ctxt as hc, powerful as PW
    m = int(np.prod(mvec))
    cc = hc.ChainContext(m, p, 1, bits=100, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    idx = list(range(len(cc.primes)))
    assert len(idx) >= 2
    ins, cubes, polys = _truth(mvec)
    pd = PW.PowerfulDCRT(g, mvec)
    rows = np.stack([_mod(ins, q) for q in cc.primes])                   # [nrows, 3, phi(m)]
    a = hx.DoubleCRT(g, idx, 3, data=rows)
    pd.dcrtToPowerful(a)
    assert np.array_equal(a.download(), np.stack([_mod(cubes, q) for q in cc.primes]))
    pd.powerfulToDCRT(a)
    assert np.array_equal(a.download(), rows)                            # the round trip
    pd.powerfulToDCRT(a)
    assert np.array_equal(a.download(), np.stack([_mod(polys, q) for q in cc.primes]))
    # words over the whole range of every row: the round trip, both ways round
    rng = np.random.default_rng(m)
    full = np.stack([rng.integers(0, q, size=(3, g.phim), dtype=np.uint64) for q in cc.primes])
    b = hx.DoubleCRT(g, idx, 3, data=full)
    pd.dcrtToPowerful(b)
    assert mvec == (31,) or not np.array_equal(b.download(), full)
    pd.powerfulToDCRT(b)
    assert np.array_equal(b.download(), full)
    pd.powerfulToDCRT(b)
    pd.dcrtToPowerful(b)
    assert np.array_equal(b.download(), full)


@pytest.mark.parametrize("mvec", MVECS)
def test_words_modulo_any_q(hx, mvec):
    from helib_amd import powerful as PW
    m = int(np.prod(mvec))
    g = hx.Context(m)
    dev, host = PW.PowerfulConversion(mvec, g), PW.PowerfulConversion(mvec)
    ins, cubes, polys = _truth(mvec)
    for q in WORD_MODULI:
        w = _mod(ins, q).astype(np.int64)
        got = dev.polyToPowerful(w, q)
        assert np.array_equal(got, _mod(cubes, q).astype(np.int64)), q
        assert np.array_equal(got, host.polyToPowerful(w, q)), q         # the numpy form gives the same words
        assert np.array_equal(dev.powerfulToPoly(got, q), w), q
        back = dev.powerfulToPoly(w, q)
        assert np.array_equal(back, _mod(polys, q).astype(np.int64)) and np.array_equal(back, host.powerfulToPoly(w, q)), q
    # any int64 is reduced first
    q = 49
    assert np.array_equal(dev.polyToPowerful(np.array(ins[1:2], dtype=np.int64), q), _mod(cubes[1:2], q).astype(np.int64))


# ---- (f') more items than workgroups ----
# 300 items on a grid of 256: workgroups 0..43 take a second item, of another row (another modulus) and other data, into
# buffers that hold the first one's cube and ping-pong pair
Q62 = (1 << 62) - 57


def _bulk(mvec, primes, batch):
    """[rows, batch, phi(m)] words over each row's whole range with the three inputs of _truth at items 0, 1, 2 and
    256, 257, 258; -> (rows, {(row, b): which input})"""
    n = PR.indexes(mvec).phim
    rng = np.random.default_rng(n + batch)
    rows = np.stack([rng.integers(0, q, size=(batch, n), dtype=np.uint64) for q in primes])
    ins = _truth(mvec)[0]
    where = {}
    for item in (0, 1, 2, 256, 257, 258):
        r, b = divmod(item, batch)
        rows[r, b] = _mod(ins, primes[r])[item % 256]
        where[r, b] = item % 256
    return rows, where


@pytest.mark.parametrize("mvec", PR.MANY_ITEMS)
def test_more_items_than_workgroups(hx, mvec):
    from helib_amd import ctxt as hc, powerful as PW
    m = int(np.prod(mvec))
    cc = hc.ChainContext(m, 2, 1, bits=100, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    host = PW.PowerfulConversion(mvec)                                   # the numpy form: no device
    ins, cubes, polys = _truth(mvec)
    pd = PW.PowerfulDCRT(g, mvec)
    # one row first, then three, then all on the same tables: the moduli's buffer grows twice
    one = hx.DoubleCRT(g, [1], 3, data=_mod(ins, cc.primes[1])[None])
    pd.dcrtToPowerful(one)
    assert np.array_equal(one.download()[0], _mod(cubes, cc.primes[1]))
    idx, B = [0, 4, 8], 100
    primes = [cc.primes[i] for i in idx]
    assert len(set(primes)) == 3 and len(idx) * B == 300 > 256 and all(q < 1 << 62 for q in primes)
    rows, where = _bulk(mvec, primes, B)
    assert sorted(where) == [(0, 0), (0, 1), (0, 2), (2, 56), (2, 57), (2, 58)]     # items i and i + 256: rows 0 and 2
    want_cube = np.stack([host.polyToPowerful(rows[r].astype(np.int64), q) for r, q in enumerate(primes)]).astype(np.uint64)
    want_poly = np.stack([host.powerfulToPoly(rows[r].astype(np.int64), q) for r, q in enumerate(primes)]).astype(np.uint64)
    assert not np.array_equal(want_cube[0, :3], want_cube[2, 56:59])
    a = hx.DoubleCRT(g, idx, B, data=rows)
    pd.dcrtToPowerful(a)
    got = a.download()
    for (r, b), i in where.items():                                      # the definition itself, on both trips
        assert np.array_equal(got[r, b], _mod(cubes[i:i + 1], primes[r])[0]), (r, b)
    assert np.array_equal(got, want_cube)
    pd.powerfulToDCRT(a)
    assert np.array_equal(a.download(), rows)                            # the round trip
    pd.powerfulToDCRT(a)
    got = a.download()
    for (r, b), i in where.items():
        assert np.array_equal(got[r, b], _mod(polys[i:i + 1], primes[r])[0]), (r, b)
    assert np.array_equal(got, want_poly)
    pd.dcrtToPowerful(a)
    assert np.array_equal(a.download(), rows)
    everything = list(range(len(cc.primes)))
    full = hx.DoubleCRT(g, everything, 3, data=np.stack([_mod(ins, q) for q in cc.primes]))
    pd.dcrtToPowerful(full)
    assert np.array_equal(full.download(), np.stack([_mod(cubes, q) for q in cc.primes]))
    # host words: batch 300, then 1, then 301 through one handle -- its buffer grows, is reused for less, grows again
    t = hx.Powerful(g, mvec)
    w, where = _bulk(mvec, [Q62], 301)
    w = w[0].astype(np.int64)
    want = host.polyToPowerful(w, Q62)
    back = host.powerfulToPoly(w, Q62)
    for n_items in (300, 1, 301):
        got = hx.powerfulWords(t, w[:n_items], Q62, True)
        assert np.array_equal(got, want[:n_items]), n_items
        assert np.array_equal(hx.powerfulWords(t, got, Q62, False), w[:n_items]), n_items
        assert np.array_equal(hx.powerfulWords(t, w[:n_items], Q62, False), back[:n_items]), n_items
    for (_, b), i in where.items():
        assert np.array_equal(want[b], _mod(cubes[i:i + 1], Q62)[0].astype(np.int64))
        assert np.array_equal(back[b], _mod(polys[i:i + 1], Q62)[0].astype(np.int64))


def test_powerful_refusals(hx):
    L = hx.lib()
    g = hx.Context(15)
    h = C.c_void_p()

    def create(mv):
        a = np.array(mv, dtype=np.uint64)
        return L.hx_powerful_create(g.h, a.ctypes.data_as(C.c_void_p), len(mv), C.byref(h))
    assert create([3, 15]) == hx.HX_ERR_INVALID and b"not coprime" in L.hx_last_error()
    assert create([3, 7]) == hx.HX_ERR_INVALID and b"21" in L.hx_last_error() and b"15" in L.hx_last_error()
    assert create([1, 15]) == hx.HX_ERR_INVALID
    assert L.hx_powerful_create(g.h, None, 2, C.byref(h)) == hx.HX_ERR_INVALID and b"null argument" in L.hx_last_error()
    assert not h.value
    t = hx.Powerful(g, (3, 5))
    w = np.zeros((1, 8), dtype=np.int64)
    for q in (1, 1 << 62):
        assert L.hx_powerful_words(t.h, 1, q, w.ctypes.data_as(C.c_void_p), 1, w.ctypes.data_as(C.c_void_p)) == hx.HX_ERR_INVALID
    assert L.hx_powerful_words(t.h, 1, 7, None, 1, None) == hx.HX_ERR_INVALID
    assert L.hx_poly_to_powerful(t.h, None) == hx.HX_ERR_INVALID and L.hx_powerful_to_poly(None, None) == hx.HX_ERR_INVALID
    from helib_amd import ctxt as hc
    other = hx.Context(15)
    other.add_prime(hc.ChainContext(15, 2, 1, bits=100, c=2).primes[0])
    with pytest.raises(hx.HxError, match="another context"):
        hx.polyToPowerful(t, hx.DoubleCRT(other, [0], 1))
    g.graphBegin()                                                       # an open graph capture
    try:
        assert L.hx_powerful_words(t.h, 1, 7, w.ctypes.data_as(C.c_void_p), 1, w.ctypes.data_as(C.c_void_p)) == hx.HX_ERR_INVALID
        assert b"captured" in L.hx_last_error()
        assert create([3, 5]) == hx.HX_ERR_INVALID and b"captured" in L.hx_last_error()
    finally:
        try:
            g.graphEnd().destroy()
        except hx.HxError:
            pass


# ---- (g) the slot tables over supplied generators ----
BITS = 200       # tests/test_evalmap_host.py: the smallest multiple of 100 at which the map stays correct, plus 100


def _chain(hx, m, p, r, gens, ords, bits=BITS, keys=True, seed=5):
    from helib_amd import bgv_gr, ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, r, bits=bits, c=3)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    ea = bgv_gr.EncryptedArray(cc, g, gens=gens, ords=ords)
    if not keys:
        return cc, g, None, ea
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    sk.zMStar = ea.zMStar
    hk.addSome1DMatrices(sk)
    hk.addFrbMatrices(sk)
    return cc, g, sk, ea


@pytest.mark.parametrize("ring", E.RINGS, ids=lambda x: "m%d" % int(np.prod(x[2])))
def test_tables_over_generators_agree_with_the_plain_side(hx, ring):
    from helib_amd import hostnt
    p, rs, mvec, gens, ords = ring
    m, r = int(np.prod(mvec)), rs[-1]
    cc, g, _, ea = _chain(hx, m, p, r, gens, ords, bits=100, keys=False)
    z = hostnt.ZmStar(m, p, gens, ords)
    assert ea.enc.table.gens == list(gens) and ea.enc.table.ords == z.signedOrds()
    assert ea.zMStar.reps() == z.reps() and ea.size() == z.getNSlots()
    cpu = E.GensEncoder(m, p, r, gens, ords)
    assert ea.G == cpu.G
    n, d, P = ea.size(), ea.getDegree(), p ** r
    v = np.random.default_rng(m).integers(0, P, size=(2, n, d))
    v[1] = P - 1
    poly, cf = ea.enc.encode(v, 1, list(cc.ctxtPrimes), coeffs=True)
    assert np.array_equal(cf, cpu.coeffs(v))                             # the words the CPU tables give
    assert np.array_equal(ea.enc.embed(cf), v) and np.array_equal(cpu.slots(cf), v)
    assert np.array_equal(ea.enc.decode(poly, 1), v)


def test_no_generators_is_the_table_of_today(hx):
    from helib_amd import ctxt as hc
    m, p, r = 85, 2, 4
    g = hx.Context(m)
    h = C.c_void_p()
    assert hx.lib().hx_bgv_gf_create_gens(g.h, p, r, None, None, 0, C.byref(h)) == 0
    t = hx.BgvGf(g, p, r)
    raw = hx.BgvGf.__new__(hx.BgvGf)                                   # the same wrapper over the handle of the new entry
    raw.__dict__.update(t.__dict__)
    raw.h = h
    v = np.random.default_rng(1).integers(0, p ** r, size=(2, t.nslots, t.d))
    idx = [g.add_prime(q) for q in hc.ChainContext(m, p, r, bits=100, c=2).primes[:2]]
    a, acf = hx.bgvGfEncode(raw, v, idx, coeffs=True)
    b, bcf = hx.bgvGfEncode(t, v, idx, coeffs=True)
    assert np.array_equal(acf, bcf) and acf.any() and np.array_equal(a.download(), b.download())
    assert np.array_equal(hx.bgvGfEmbed(raw, acf), v)
    gg, oo, nd = (C.c_uint64 * 8)(), (C.c_int64 * 8)(), C.c_int()
    assert hx.lib().hx_bgv_gf_info(h, None, None, None, C.byref(nd), gg, oo, None, None) == 0
    assert (list(gg[:nd.value]), list(oo[:nd.value])) == (t.gens, t.ords)
    raw.close()
    assert hx.BgvGf(g, p, r, gens=(), ords=()).gens == t.gens


def test_generator_refusals(hx):
    g = hx.Context(85)
    for gens, ords, what in (((52, 52), (4, 2), "enumerate"), ((5,), (8,), "not coprime"), ((52, 71), (4, 4), "multiply to 16"),
                             ((3,) * 9, (1,) * 9, "9 generators")):
        with pytest.raises(hx.InvalidArgument, match=what):
            hx.BgvGf(g, 2, 4, gens=gens, ords=ords)
    with pytest.raises(hx.InvalidArgument, match="come together"):
        hx.BgvGf(g, 2, 4, gens=(52, 71))
    h = C.c_void_p()
    one = np.array([52], dtype=np.uint64)
    assert hx.lib().hx_bgv_gf_create_gens(g.h, 2, 4, one.ctypes.data_as(C.c_void_p), None, 1, C.byref(h)) == hx.HX_ERR_INVALID
    assert b"null argument" in hx.lib().hx_last_error() and not h.value


@pytest.mark.parametrize("m", [57, 1365])
def test_rotate1d_along_the_chosen_dimensions(hx, m):
    p, rs, mvec, gens, ords = E.ring(m)
    r = rs[-1]
    cc, g, sk, ea = _chain(hx, m, p, r, gens, ords)
    n, d, P = ea.size(), ea.getDegree(), p ** r
    sizes = [abs(o) for o in ords]
    assert [ea.sizeOfDimension(i) for i in range(ea.dimension())] == sizes
    assert [ea.nativeDimension(i) for i in range(ea.dimension())] == [o > 0 for o in ords]
    v = np.random.default_rng(m).integers(0, P, size=(2, n, d))
    for dim, D in enumerate(sizes):
        for amt in sorted({1, D - 1}):
            ct = ea.encrypt_batch(sk, v)
            ea.rotate1D(ct, dim, amt)
            assert ct.isCorrect()
            want = np.roll(v.reshape([2] + sizes + [d]), amt, axis=1 + dim).reshape(2, n, d)
            assert np.array_equal(ea.decrypt_batch(ct, sk), want), (dim, amt)


# ---- (h) EvalMap with real keys ----
@pytest.mark.parametrize("m,r", [(105, 3), (57, 2), (85, 4), (1365, 1)])
def test_evalmap_with_real_keys(hx, m, r):
    from helib_amd import evalmap
    p, _, mvec, gens, ords = E.ring(m)
    cc, g, sk, ea = _chain(hx, m, p, r, gens, ords)
    n, d, P = ea.size(), ea.getDegree(), p ** r
    rng = np.random.default_rng(m)
    F = rng.integers(0, P, size=(2, n * d))
    cube = np.stack([np.array(PR.poly_to_powerful(f, mvec, P), dtype=np.int64).reshape(n, d) for f in F])
    slots = np.array([E.slots_of(f, ea.zMStar, ea.G, P) for f in F], dtype=np.int64)
    for invert, v, want in ((False, cube, slots), (True, slots, cube)):
        res = {}
        fresh = ea.encrypt_batch(sk, v)                                   # one encryption: the noise bounds follow the data
        for fused in (True, False):
            em = evalmap.EvalMap(ea, mvec, invert=invert, fused=fused)
            assert np.array_equal(em.applyPlain(v), want), invert
            ct = fresh.clone()
            em.apply(ct, pk=sk)
            assert em.mat1.onDevice and em.mat1.fusedConstants is fused
            assert all(ex is None or ex.fusedConstants is fused for ex in em.matvec)
            assert ct.isCorrect()
            assert np.array_equal(ea.decrypt_batch(ct, sk), want), (invert, fused)
            res[fused] = ct
        H.same(res[True], res[False], lambda part: part.download())
