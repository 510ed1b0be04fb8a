"""hx_table_tensor_sum and helib_amd.table_lookup on the device.  Everything here is an integer: every comparison is exact.

Chain size of the slot runs (m = 85, p = 2, c = 2, 8 slots of degree 8, batch 3): bits = 200, the smallest multiple of
100 at which the default form keeps every output correct for 3-bit and 5-bit indices (found with the oracle backend on
the CPU; the reference's test takes 30 (5 + nBits) = 240 and 300: at 100 a fresh ciphertext has 93 bits, the 3-bit lookup
keeps 69 and the 5-bit one is refused by the level check, 93 < (NumBits(5) + 1) 30 = 120; at 200 fresh is 200 and the
lookups keep 176 and 165 bits, in the default and in the lazy form alike).  The write-in test runs at p^r = 16, where a
fresh ciphertext starts four bits of noise higher per factor of p: it takes 300."""
import ctypes as C

import numpy as np
import pytest

from helib_amd import hostnt
from tests import table_lookup_ref as R

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


# ---- (a) the kernel against python integers and against the calls it replaces ----
TS_M, TS_N = 1031, 1030                  # phi(1031) = 1030: 515 two-word vectors, three workgroup columns
TS_WIDTHS = (60, 56, 45, 38, 60, 60)
TS_IDX = [5, 2, 0, 3, 1]                 # the output rows: five of the six primes, all four widths, in another order
TS_ALL = [0, 1, 2, 3, 4, 5]              # the table's rows
KMAX = LMAX = 16
BATCHES = (1, 2, 3, 4)                   # BP = 1; then, two elements to a thread: one group, a partial last one, two


@pytest.fixture(scope="module")
def ts_ring(hx):
    gens = {b: hostnt.PrimeGen(b, TS_M) for b in set(TS_WIDTHS)}
    g = hx.Context(TS_M)
    for b in TS_WIDTHS:
        g.add_prime(gens[b].next())
    assert g.phim == TS_N and [q.bit_length() for q in g.primes] == list(TS_WIDTHS)
    assert (TS_N // 2 + 255) // 256 == 3 and TS_N // 2 % 256 == 3
    return g


def _arr(ps):
    return (C.c_void_p * max(len(ps), 1))(*[p.h for p in ps])


def _raw(hx, outs, a0, a1, b0, b1, table, size, k=None, l=None):
    k = len(a0) if k is None else k
    l = len(b0) if l is None else l
    return hx.lib().hx_table_tensor_sum(outs[0].h, outs[1].h, outs[2].h, _arr(a0), _arr(a1), k, _arr(b0), _arr(b1), l,
                                        table.h, size)


def _sequence(hx, a0, a1, b0, b1, entries, size):
    """one hx_mul_add_many per row of the grid that holds an entry, and one hx_tensor_sum"""
    k = len(a0)
    l = min(len(b0), (size + k - 1) // k)
    b0, b1 = b0[:l], b1[:l]
    w0, w1 = [], []
    for j in range(l):
        kj = min(k, size - j * k)
        u0, u1 = hx.likeUninit(a0[0]), hx.likeUninit(a0[0])
        hx.mulAddMany(u0, u1, entries[j * k:j * k + kj], a0[:kj], a1[:kj], accumulate=False)
        w0.append(u0)
        w1.append(u1)
    return hx.tensorSum(w0, w1, b0, b1)


@pytest.fixture(scope="module")
def ts_polys(hx, ts_ring):
    """per batch size: 16 pairs a, 16 pairs b (pair 1 of b IS pair 1 of a: an operand used twice) on TS_IDX with q - 1
    planted in the first vector of the first element and the last vector of the last; shared by them, one table poly of
    256 entries on all six primes (planted likewise), its entries as batch-1 polys, and everything as integers"""
    g = ts_ring
    qs = [g.primes[i] for i in TS_IDX]
    rng = np.random.default_rng(17)

    def rnd(idx, B):
        x = np.stack([rng.integers(0, g.primes[i], size=(B, TS_N), dtype=np.uint64) for i in idx])
        x[:, -1, -2:] = [[g.primes[i] - 1, 0] for i in idx]
        x[:, 0, :2] = [[g.primes[i] - 1, g.primes[i] - 1] for i in idx]
        return x
    tw = rnd(TS_ALL, KMAX * LMAX)
    table = hx.DoubleCRT(g, TS_ALL, KMAX * LMAX, tw)
    entries = hx.splitBatch(table)
    tsel = tw[[TS_ALL.index(i) for i in TS_IDX]]
    made = {}
    for B in BATCHES:
        words = {n: [rnd(TS_IDX, B) for _ in range(KMAX)] for n in ("a0", "a1", "b0", "b1")}
        polys = {n: [hx.DoubleCRT(g, TS_IDX, B, x) for x in w] for n, w in words.items()}
        for n, m in (("b0", "a0"), ("b1", "a1")):
            words[n][1], polys[n][1] = words[m][1], polys[m][1]
        made[B] = (polys, words)
    return table, entries, tw, tsel, qs, made


def _table_of(hx, g, tw, size):
    return hx.DoubleCRT(g, TS_ALL, size, np.ascontiguousarray(tw[:, :size]))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("k,l,size", [(4, 2, 8), (4, 2, 5), (16, 2, 32), (16, 16, 256), (16, 8, 100)])
def test_table_tensor_sum_against_the_sequence_and_python_integers(hx, ts_ring, ts_polys, k, l, size, B):
    """A workgroup column takes 256 two-word vectors and a thread 1 or 2 batch elements and 4 values of j: 1030
    coefficients are three columns, the last with 3 live threads; l = 2 is half a block of j, l = 8 and 16 two and four;
    sizes 5 and 100 end in a ragged row (1 and 4 entries of it), and at (16, 8, 100) the eighth row holds nothing.  Every word against l x hx_mul_add_many and one
    hx_tensor_sum; against python integers every word at (4, 2), elsewhere the first and last two vectors of every row
    and element and 32 random coefficients."""
    g = ts_ring
    table_all, entries, tw, tsel, qs, made = ts_polys
    polys, words = made[B]
    a0, a1, b0, b1 = polys["a0"][:k], polys["a1"][:k], polys["b0"][:l], polys["b1"][:l]
    table = table_all if size == KMAX * LMAX else _table_of(hx, g, tw, size)
    rng = np.random.default_rng(size + B)
    bystander = np.stack([rng.integers(0, g.primes[i], size=(B, TS_N), dtype=np.uint64) for i in TS_IDX])
    before = hx.DoubleCRT(g, TS_IDX, B, bystander)
    outs = [hx.DoubleCRT(g, TS_IDX, B, bystander) for _ in range(3)]       # (overwritten, not read)
    after = hx.DoubleCRT(g, TS_IDX, B, bystander)
    assert _raw(hx, outs, a0, a1, b0, b1, table, size) == 0, hx.lib().hx_last_error()
    got = [o.download() for o in outs]
    seq = _sequence(hx, a0, a1, b0, b1, entries, size)
    for part in range(3):
        bad = np.argwhere(got[part] != seq[part].download())
        assert not len(bad), "part %d: %d words differ, the first at [row, element, word] %s" % (part, len(bad), bad[0])
    cols = np.arange(TS_N) if k == 4 else \
        np.unique(np.concatenate([[0, 1, 2, 3, TS_N - 4, TS_N - 3, TS_N - 2, TS_N - 1], rng.integers(0, TS_N, 32)]))
    sel = lambda ws: [w[:, :, cols].astype(object) for w in ws]      # noqa: E731
    want = R.table_tensor_sum(sel(words["a0"][:k]), sel(words["a1"][:k]), sel(words["b0"][:l]), sel(words["b1"][:l]),
                              tsel[:, :size][:, :, cols].astype(object), size, qs)
    for part in range(3):
        assert np.array_equal(got[part][:, :, cols], want[part].astype(np.uint64)), part
    assert np.array_equal(before.download(), bystander) and np.array_equal(after.download(), bystander)
    for n, ps in polys.items():
        assert all(np.array_equal(p.download(), w) for p, w in zip(ps[:2], words[n][:2]))     # the inputs are as they were
    assert np.array_equal(table.download(), tw[:, :size])
    new = hx.tableTensorSum(a0, a1, b0, b1, table)                                            # the binding
    assert all(new[p].getIndexSet() == TS_IDX and np.array_equal(new[p].download(), got[p]) for p in range(3))


def test_table_tensor_sum_of_512_entries_of_q_minus_1(hx, ts_ring):
    """k = 256, l = 2 on the 60-bit prime, every word q - 1: an inner sum takes 256 products (q - 1)^2, the most its
    128-bit accumulator ever holds; (q - 1)^3 = -1, so o0 = o2 = -512 and o1 = -1024 mod q"""
    g, k, l, B = ts_ring, 256, 2, 2
    q = g.primes[0]
    assert q.bit_length() == 60
    x = hx.DoubleCRT(g, [0], B, np.full((1, B, TS_N), q - 1, dtype=np.uint64))
    table = hx.DoubleCRT(g, [0], k * l, np.full((1, k * l, TS_N), q - 1, dtype=np.uint64))
    outs = [x.copy() for _ in range(3)]                          # outputs that still share the operand's rows
    assert _raw(hx, outs, [x] * k, [x] * k, [x] * l, [x] * l, table, k * l) == 0, hx.lib().hx_last_error()
    for part, mult in enumerate((1, 2, 1)):
        assert np.array_equal(outs[part].download(), np.full((1, B, TS_N), (-512 * mult) % q, dtype=np.uint64)), part
    assert np.array_equal(x.download(), np.full((1, B, TS_N), q - 1, dtype=np.uint64))


def test_table_tensor_sum_of_65536_entries_of_q_minus_1(hx):
    """k = l = 256 on N = 16 (m = 17), two primes, every word q - 1: the outer sums cross their reduction after 128
    values of j inside the loop; -65536 and -131072 mod q"""
    g, k, l = hx.Context(17), 256, 256
    for bits in (60, 45):
        g.add_prime(hostnt.PrimeGen(bits, 17).next())
    assert g.phim == 16
    for B in (1, 3):
        full = np.stack([np.full((B, 16), q - 1, dtype=np.uint64) for q in g.primes])
        x = hx.DoubleCRT(g, [0, 1], B, full)
        table = hx.DoubleCRT(g, [1, 0], k * l, np.stack([np.full((k * l, 16), g.primes[i] - 1, dtype=np.uint64) for i in (1, 0)]))
        o = hx.tableTensorSum([x] * k, [x] * k, [x] * l, [x] * l, table)
        for part, mult in enumerate((1, 2, 1)):
            want = np.stack([np.full((B, 16), (-65536 * mult) % q, dtype=np.uint64) for q in g.primes])
            assert np.array_equal(o[part].download(), want), (B, part)


# ---- (b) refusals ----
def test_table_tensor_sum_refusals_touch_nothing(hx):
    import torch
    g, other = hx.Context(85), hx.Context(85)
    gen = hostnt.PrimeGen(60, 85)
    for q in [gen.next() for _ in range(4)]:
        g.add_prime(q)
        other.add_prime(q)
    rng = np.random.default_rng(2)

    def rnd(ctx=g, idx=(0, 1, 2), B=2):
        return hx.DoubleCRT(ctx, list(idx), B, np.stack([rng.integers(0, ctx.primes[i], size=(B, 64), dtype=np.uint64) for i in idx]))
    o = [rnd(), rnd(), rnd()]
    a0, a1, b0, b1 = ([rnd(), rnd()] for _ in range(4))
    tab = rnd(idx=(2, 0, 3, 1), B=4)
    polys = o + a0 + a1 + b0 + b1 + [tab]
    keep = [x.download() for x in polys]
    L = hx.lib()
    INV, UNS, PRS = hx.HX_ERR_INVALID, hx.HX_ERR_UNSUPPORTED, hx.HX_ERR_PRIMESET

    def call(outs=o, A0=a0, A1=a1, B0=b0, B1=b1, T=tab, size=4, k=None, l=None):
        return _raw(hx, outs, A0, A1, B0, B1, T, size, k, l)
    null = type("Null", (), {"h": None})()
    # a null handle: an output, an array, an entry, the table
    assert call(outs=[null, o[1], o[2]]) == INV and call(outs=[o[0], o[1], null]) == INV
    arr = _arr(a0)
    assert L.hx_table_tensor_sum(o[0].h, o[1].h, o[2].h, arr, arr, 2, None, arr, 2, tab.h, 4) == INV and b"null" in L.hx_last_error()
    assert call(B1=[b1[0], null]) == INV and b"null poly (b1[1])" in L.hx_last_error()
    assert call(T=null) == INV and b"null" in L.hx_last_error()
    # k, l, size out of range
    assert call(k=0) == INV and b"at least one" in L.hx_last_error() and call(l=0) == INV and call(k=-1) == INV
    big = [a0[0]] * 257
    assert call(A0=big, A1=big, size=257) == UNS and b"at most 256" in L.hx_last_error()
    assert call(B0=big, B1=big, size=513) == UNS
    assert call(size=5) == INV and b"is not in" in L.hx_last_error() and call(size=0) == INV and call(size=-1) == INV
    # two outputs that are the same poly
    assert call(outs=[o[0], o[0], o[2]]) == INV and b"the same poly" in L.hx_last_error()
    assert call(outs=[o[0], o[1], o[0]]) == INV and call(outs=[o[0], o[1], o[1]]) == INV
    # an output that is also an input, or the table
    assert call(A0=[a0[0], o[2]]) == INV and b"also an input (a0[1])" in L.hx_last_error()
    assert call(B1=[o[0], b1[1]]) == INV and call(A1=[o[1], a1[1]]) == INV and call(B0=[b0[0], o[1]]) == INV
    assert call(T=o[1]) == INV and b"also the table" in L.hx_last_error()
    # a poly of another context
    assert call(A1=[a1[0], rnd(other)]) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(outs=[o[0], rnd(other), o[2]]) == INV and b"incompatible objects" in L.hx_last_error()
    assert call(T=rnd(other, idx=(0, 1, 2, 3), B=4)) == INV and b"incompatible objects" in L.hx_last_error()
    # a batch or a prime set that is not o0's
    assert call(B0=[rnd(B=3), b0[1]]) == INV and b"b0[0] differs from o0" in L.hx_last_error()
    assert call(A0=[a0[0], rnd(idx=(0, 2, 1))]) == INV and b"a0[1] differs from o0" in L.hx_last_error()
    assert call(A1=[rnd(idx=(0, 1)), a1[1]]) == INV and call(B1=[b1[0], rnd(idx=(0, 1, 2, 3))]) == INV
    assert call(outs=[o[0], rnd(B=1), o[2]]) == INV and b"o1 differs from o0" in L.hx_last_error()
    assert call(outs=[o[0], o[1], rnd(idx=(2, 1, 0))]) == INV and b"o2 differs from o0" in L.hx_last_error()
    # a table whose batch is not size, or without a row for a prime
    assert call(T=rnd(idx=(0, 1, 2), B=3)) == INV and b"the table has batch 3" in L.hx_last_error()
    assert call(T=rnd(idx=(0, 1, 3), B=4)) == PRS and b"the table has no row for prime 2" in L.hx_last_error()
    # rows that are not 16-byte aligned: polys over caller-owned memory that starts 8 bytes into an allocation
    words = 4 * 4 * 64
    buf = torch.zeros(3 * (words + 2), dtype=torch.int64, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    odd_in = hx.DoubleCRT.wrap(g, [0, 1, 2], 2, buf.data_ptr() + 8)
    odd_out = hx.DoubleCRT.wrap(g, [0, 1, 2], 2, buf.data_ptr() + 8 * (words + 2) + 8)
    odd_tab = hx.DoubleCRT.wrap(g, [0, 1, 2, 3], 4, buf.data_ptr() + 16 * (words + 2) + 8)
    assert call(B0=[b0[0], odd_in]) == INV and b"b0[1]: rows are not 16-byte aligned" in L.hx_last_error()
    assert call(outs=[o[0], odd_out, o[2]]) == INV and b"output rows are not 16-byte aligned" in L.hx_last_error()
    assert call(T=odd_tab) == INV and b"table: rows are not 16-byte aligned" in L.hx_last_error()
    assert not buf.cpu().numpy().any()
    # an odd number of coefficients: phi(m) is odd for m = 2 only; polys without rows reach the check
    tiny = hx.Context(2)
    t = [hx.DoubleCRT(tiny, [], 1, zero=False) for _ in range(5)]
    assert _raw(hx, t[:3], [t[3]], [t[3]], [t[3]], [t[3]], t[4], 1) == UNS
    assert b"hx_table_tensor_sum needs an even number of coefficients" in L.hx_last_error()
    # a call during a graph capture
    g.graphBegin()
    try:
        assert call() == UNS and b"cannot be captured" in L.hx_last_error()
    finally:
        try:
            g.graphEnd().destroy()
        except hx.HxError:
            pass
    with pytest.raises(hx.InvalidArgument, match="entry by entry"):
        hx.tableTensorSum(a0, a1, b0, b1[:1], tab)
    with pytest.raises(hx.InvalidArgument, match="at least one"):
        hx.tableTensorSum([], [], b0, b1, tab)
    for x, k in zip(polys, keep):
        assert np.array_equal(x.download(), k)
    assert call() == 0                                           # and the context still works
    seq = _sequence(hx, a0, a1, b0, b1, hx.splitBatch(tab), 4)
    assert all(np.array_equal(o[k].download(), seq[k].download()) for k in range(3))


# ---- (c) end to end on real slots ----
E_BITS = 200
W_BITS = 300
E_BATCH = 3


def _chain(hx, module, m, p, r, bits, seed=5):
    from helib_amd import ctxt as hc, keys as hk
    cc = hc.ChainContext(m, p, r, bits=bits, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=seed)
    sk.GenSecKey()
    return cc, g, sk, module.EncryptedArray(cc, g)


@pytest.fixture(scope="module")
def slots(hx):
    from helib_amd import bgv_gf
    cc, g, sk, ea = _chain(hx, bgv_gf, 85, 2, 1, E_BITS)
    assert ea.size() == 8 and ea.getDegree() == 8
    return cc, g, sk, ea


def _state(ct):
    return ct.lnNoise, ct.primeSet, ct.ptxtSpace, ct.intFactor, ct.ptxtMag


def _words(ct):
    assert set(ct.parts) == {"1", "s"}
    return {h: (part.getIndexSet(), part.download()) for h, part in ct.parts.items()}


def _same_words(x, y):
    wx, wy = _words(x), _words(y)
    return all(wx[h][0] == wy[h][0] and np.array_equal(wx[h][1], wy[h][1]) for h in wx)


def _encrypt_index(ea, sk, index, nBits):
    return [ea.encrypt_batch(sk, (index >> i) & 1) for i in range(nBits)]


@pytest.mark.parametrize("kind", ["built", "slots"])
@pytest.mark.parametrize("nBits", [3, 5])
def test_table_lookup_on_slots(hx, slots, monkeypatch, nBits, kind):
    """another random index in every slot of every element.  built: buildLookupTable of 1 / (x + 1) with 8 bits out,
    read back by unpackSlots; slots: a fromSlots table with another value of GF(2^8) in every slot of every entry.  The
    default form, the lazy form through hx_mul_add_many / hx_tensor_sum and the lazy form through hx_table_tensor_sum all
    give the entry at each slot's index; the two lazy paths agree word for word; the default form's words are those of
    plain multByConstant and += on the same products."""
    from helib_amd import intraslot, table_lookup as tl
    from helib_amd.ctxt import Ctxt
    cc, g, sk, ea = slots
    n, d, size = ea.size(), ea.getDegree(), 1 << nBits
    rng = np.random.default_rng(10 * nBits + len(kind))
    index = rng.integers(0, size, size=(E_BATCH, n))
    index[0, 0], index[0, 1] = 0, size - 1
    if kind == "built":
        f = lambda x: 1.0 / (x + 1.0)                           # noqa: E731
        table = tl.buildLookupTable(ea, f, nBits, 0, 0, 8, -7, 0)
        values = np.array(tl.tableValues(f, nBits, 0, 0, 8, -7, 0))
        assert list(values[:2]) == [128, 64]
    else:
        tslots = rng.integers(0, 2, size=(size, n, d))
        table = tl.LookupTable.fromSlots(ea, tslots)
    assert len(table) == size and table.zzX.shape == (size, cc.phim) and len(table.sizes) == size
    idx = _encrypt_index(ea, sk, index, nBits)
    keep = [_state(c) for c in idx]
    calls = {"tableTensorSum": 0, "tensorSum": 0, "mulAddMany": 0}
    for name in calls:
        real = getattr(hx, name)
        monkeypatch.setattr(hx, name, lambda *a, _r=real, _n=name, **kw: (calls.__setitem__(_n, calls[_n] + 1), _r(*a, **kw))[1])
    default = tl.tableLookup(ea, table, idx, lazy=False)
    assert calls == {"tableTensorSum": 0, "tensorSum": 0, "mulAddMany": 0}
    lazy = tl.tableLookup(ea, table, idx, lazy=True, fused=False)
    k, l = R.SPLIT[nBits]
    assert calls == {"tableTensorSum": 0, "tensorSum": 1, "mulAddMany": l}
    fused = tl.tableLookup(ea, table, idx, lazy=True, fused=True)
    assert calls == {"tableTensorSum": 1, "tensorSum": 1, "mulAddMany": l}
    # lazy=None and fused=None follow table_lookup.lazyLookup and Ctxt.fuseTableSum
    monkeypatch.setattr(tl, "lazyLookup", True)
    monkeypatch.setattr(Ctxt, "fuseTableSum", False)
    assert _same_words(tl.tableLookup(ea, table, idx), lazy) and calls == {"tableTensorSum": 1, "tensorSum": 2, "mulAddMany": 2 * l}
    monkeypatch.setattr(Ctxt, "fuseTableSum", True)
    assert _same_words(tl.tableLookup(ea, table, idx), lazy) and calls["tableTensorSum"] == 2 and calls["tensorSum"] == 2
    monkeypatch.setattr(tl, "lazyLookup", False)
    assert _same_words(tl.tableLookup(ea, table, idx), default) and calls["tableTensorSum"] == 2 and calls["tensorSum"] == 2
    for name, ct in (("default", default), ("lazy", lazy), ("fused", fused)):
        assert ct.isCorrect() and ct.bitCapacity() > 0, name
        got = ea.decrypt_batch(ct, sk)
        if kind == "built":
            for b in range(E_BATCH):
                assert intraslot.unpackSlots(ea, got[b:b + 1]) == list(values[index[b]]), (name, b)
        else:
            want = tslots[index, np.arange(n)[None, :]]                      # [B, n, d]: slot s of entry index[b, s]
            assert np.array_equal(got, want), name
    assert _state(lazy) == _state(fused) and _same_words(lazy, fused)
    assert [_state(c) for c in idx] == keep
    # the default form's words: plain multByConstant / += on the same products
    products = tl.computeAllProducts(idx, size)
    primes = sorted(frozenset().union(*[c.primeSet for c in products]))
    consts = hx.splitBatch(ea.enc.encode(table.slots, 1, primes))
    replay = products[0]._emptyLike()
    for i, c in enumerate(products):
        c.multByConstant(consts[i], table.sizes[i])
    for c in products:
        replay += c
    assert _state(replay) == _state(default) and _same_words(replay, default)


def test_table_write_in_histogram_mod_16(hx):
    """p^r = 16 over helib_amd.bgv_pr (m = 85): ten write-ins at random per-slot indices leave the per-slot histogram"""
    from helib_amd import bgv_pr, table_lookup as tl
    cc, g, sk, ea = _chain(hx, bgv_pr, 85, 2, 4, W_BITS)
    n, P, nBits, size = ea.size(), 16, 2, 4
    rng = np.random.default_rng(16)
    start = rng.integers(0, P, size=(size, E_BATCH, n))
    T = [ea.encrypt_batch(sk, start[i]) for i in range(size)]
    hist = start.copy()
    for _ in range(10):
        index = rng.integers(0, size, size=(E_BATCH, n))
        tl.tableWriteIn(T, _encrypt_index(ea, sk, index, nBits))
        for i in range(size):
            hist[i] += index == i
    for i in range(size):
        assert T[i].isCorrect() and T[i].ptxtSpace == P
        assert np.array_equal(ea.decrypt_batch(T[i], sk), hist[i] % P), i
