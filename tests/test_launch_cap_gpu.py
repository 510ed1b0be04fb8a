"""The slot kernels past the BGV_MAX_BLOCKS cap of their launches: every grid-stride loop of bgv_gf.hip, bgv_crt.hip,
bgv_gf_linalg.hip and the diagonal scatter of bgv_slots.h takes a second (ragged) trip here, at the sizes that
tests/test_launch_cap_host.py derives from the constants in the sources.  The references are the restatements in tests/,
computed on 13 distinct elements (descriptors, entries) plus a few that occur once, around the trip boundaries; the big
input repeats the 13 (big[i] = base[i % 13]) and the expectation is the reference tiled the same way.  13 divides no
stride of the launch arithmetic (asserted on the host), so a word taken from the wrong trip or tile differs.  Everything
here is an integer: every comparison is exact."""
import itertools

import numpy as np
import pytest

from helib_amd import hostnt

from tests import bgv_crt_ref as CR
from tests import intraslot_ref as IR
from tests import test_launch_cap_host as LC

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


@pytest.fixture(scope="module")
def K():
    return LC.constants()


def _ctx(hx, m, nprimes=1, bits=60):
    g = hostnt.PrimeGen(bits, m)
    c = hx.Context(m)
    for _ in range(nprimes):
        c.add_prime(g.next())
    return c


def _ea(hx, m, p, r, bits=100):
    from helib_amd import bgv_gr, ctxt as hc
    cc = hc.ChainContext(m, p, r, bits=bits, c=2)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    return bgv_gr.EncryptedArray(cc, g)


@pytest.fixture(scope="module")
def full_ea(hx):
    """the measured ring, built once for the gather and the linearized-polynomial cases"""
    m, p, r = LC.FULL_RING
    ea = _ea(hx, m, p, r, bits=60)
    assert (ea.size(), ea.getDegree(), ea.dimension()) == (1024, 16, 2)
    return ea


# ---- 1. GF / Galois-ring encode, embed, decode ----
@pytest.mark.parametrize("m,p,r", LC.GF_RINGS)
def test_gf_encode_embed_decode_past_the_cap(hx, K, m, p, r):
    case = LC.gf_case(m, p, K)
    ref = IR.tables(m, p, r)
    n, d, N, P, B = ref.nslots, ref.d, ref.phim, p ** r, case.size
    c = _ctx(hx, m)
    t = hx.BgvGf(c, p, r)
    assert (t.d, t.nslots, c.phim) == (d, n, N) == LC.ring(m, p)
    sel, pos = LC.selection(B, case.boundaries)
    rng = np.random.default_rng(m)
    uniq = LC.distinct_elements(rng, LC.PERIOD + len(pos), (n, d), P)
    want = ref.encode(uniq)
    a = uniq[sel]
    L = case.launches
    tb, ek = K["GF_TB"], K["GF_EK"]
    ktiles = -(-(N + d - 1) // ek)
    cf = hx.bgvGfEncode(t, a, [], coeffs=True)[1]
    LC.check(cf, want[sel], "encode", lambda b, k: b // tb * ktiles + k // ek, L["bgv_gf_encode_kernel"])
    # embed of polynomials that are no encodings
    f = LC.distinct_elements(rng, len(uniq), (N,), P, -2 ** 40, 2 ** 40)
    jc, di = LC._jc(d), K["GF_DI"]
    itiles, jchunks = -(-n // di), -(-d // jc)
    dunit = lambda b, w: (b // tb * itiles + w // d // di) * jchunks + w % d // jc      # noqa: E731
    LC.check(hx.bgvGfEmbed(t, f[sel]), ref.decode(f)[sel], "embed", dunit, L["bgv_gf_decode_kernel"])
    LC.check(hx.bgvGfEmbed(t, cf), a % P, "round trip", dunit, L["bgv_gf_decode_kernel"])
    if (m, p, r) == LC.GF_RINGS[0]:                              # onto one 60-bit prime, with a multiplier
        wmul = ref.encode(uniq, P - 1)[sel]
        poly, cm = hx.bgvGfEncode(t, a, [0], P - 1, coeffs=True)
        LC.check(cm, wmul, "encode with mul = P - 1")
        res = np.mod(wmul, np.int64(c.primes[0])).astype(np.uint64)[None]
        LC.check(poly.download(), hx.DoubleCRT(c, [0], B, res).FFT().download(), "the words of the encode")


# ---- 2. integer slots through the CRT tables ----
@pytest.mark.parametrize("m,p", LC.CRT_RINGS)
def test_crt_encode_embed_past_the_cap(hx, K, m, p):
    case = LC.crt_case(m, p, K)
    ref = CR.tables(m, p)
    n, N, B = ref.nslots, ref.phim, case.size
    c = _ctx(hx, m)
    t = hx.BgvCrt(c, p)
    assert (t.d, t.nslots, c.phim) == LC.ring(m, p)
    sel, pos = LC.selection(B, case.boundaries)
    rng = np.random.default_rng(m + 1)
    uniq = LC.distinct_elements(rng, LC.PERIOD + len(pos), (n,), p)
    tb = K["CRT_TB"]
    ktiles = -(-(-(-N // 4) * 4) // K["CRT_EK"])
    cf = hx.bgvCrtEncode(t, uniq[sel], [], coeffs=True)[1]
    LC.check(cf, ref.encode(uniq)[sel], "encode", lambda b, k: b // tb * ktiles + k // K["CRT_EK"], case.launches["bgv_crt_encode_kernel"])
    f = LC.distinct_elements(rng, len(uniq), (N,), p, -2 ** 40, 2 ** 40)
    itiles = -(-n // K["CRT_DI"])
    LC.check(hx.bgvCrtEmbed(t, f[sel]), ref.decode(f)[sel], "embed", lambda b, i: b // tb * itiles + i // K["CRT_DI"],
             case.launches["bgv_crt_decode_kernel"])
    LC.check(hx.bgvCrtEmbed(t, cf), uniq[sel] % p, "round trip")


# ---- 3. the gather and the fused gather-map kernel ----
def _descriptors(ea, count, period):
    """(maps, uniq [(diagonal, k, map)], dead): `period` base descriptors over identity, rotated, masked and twisted maps
    and several coefficient indices, with three consecutive dead ones (the all-zero map) at 3, 4, 5, then `count - period`
    live ones that differ from all of them"""
    from helib_amd import bgv_gr_matmul as RM
    n, d, D, z, m = ea.size(), ea.getDegree(), ea.sizeOfDimension(0), ea.zMStar, ea.zMStar.m
    maps = RM._Maps(ea)
    i1 = min(3, D - 1)
    mask = ea.maskSlots(0, i1)
    rows = [maps.add(1), maps.add(z.genToPow(0, -2)), maps.add(1, mask), maps.add(z.genToPow(-1, -3)),
            maps.add(z.genToPow(0, D - i1) * z.genToPow(-1, -1) % m, 1 - mask), maps.add(1, np.zeros(n, dtype=np.int64))]
    dead = rows[-1]
    assert len(set(rows)) == 6
    diags, ks = sorted({0, i1, D - 1}), sorted({0, min(1, d - 1), d - 1})
    live = list(itertools.product(diags, ks, rows[:-1]))
    assert len(live) % 7 != 0 and len(live) >= count - 3
    live = [live[7 * t % len(live)] for t in range(len(live))]    # a walk through all of them that changes map and k
    gone = [(dg, k, dead) for dg, k in zip(itertools.cycle(diags), ks * 3)][:3]
    uniq = live[:3] + gone + live[3:count - 3]
    assert len(set(uniq)) == count
    assert len({x[1] for x in uniq[:period]}) == len(ks) and len({x[2] for x in uniq[:period]}) == len(rows)
    return maps, uniq, dead


@pytest.mark.parametrize("m,p,r", LC.GATHER_RINGS)
def test_gather_and_fused_kernel_past_the_cap(hx, K, m, p, r):
    from helib_amd import bgv_gr_matmul as RM
    case = LC.gather_case(m, p, K)
    ea = _ea(hx, m, p, r)
    n, d, D, P, ndesc = ea.size(), ea.getDegree(), ea.sizeOfDimension(0), p ** r, case.size
    assert (d, n) == LC.ring(m, p)[:2]
    sel, pos = LC.selection(ndesc, case.boundaries)
    rng = np.random.default_rng(m)
    A = rng.integers(0, P, size=(D, D, d, d))
    A[0, 0] = P - 1
    mat = RM.BlockMatMul1D(ea, A, 0)
    maps, uniq, dead = _descriptors(ea, LC.PERIOD + len(pos), LC.PERIOD)
    table, handle = np.stack(maps.rows), mat.handle(ea.enc)
    want = np.stack([RM.hostConstant(ea, mat, i, k, maps.rows[mp]) for i, k, mp in uniq])
    wflags = want.reshape(len(uniq), -1).any(axis=1)
    isdead = np.array([x[2] == dead for x in uniq])
    assert wflags[~isdead].all() and not wflags[isdead].any() and isdead[3:6].all() and (want == P - 1).any()
    descs = np.array(uniq, dtype=np.int32)[sel]
    G, F = case.launches["bgv_gf_gather_kernel"], case.launches["bgv_gf_gather_map_kernel"]
    per = K["GM_THREADS"] // LC.gm_group(d)
    slots, gflags = hx.bgvGfGather(handle, descs, table)
    LC.check(slots, want[sel], "gather", lambda q, w: (q * n * d + w) // LC.THREADS, G)
    LC.check(gflags, wflags[sel], "gather flags")
    LC.check(ea.enc.encodeGathered(handle, descs, table, 1, [], flags_only=True), wflags[sel], "fused flags",
             lambda q, _: q * n // per, F)
    wcf = ea.enc.encode(want, 1, [], coeffs=True)[1]             # hx_bgv_gf_encode of the distinct constants
    # one call of the same size with every descriptor live: the grow-only scratch holds non-zero words behind it
    alive = np.array([x for x in uniq if x[2] != dead], dtype=np.int32)
    _, lcf, lflags = ea.enc.encodeGathered(handle, alive[np.arange(ndesc) % len(alive)], table, 1, [], coeffs=True)
    assert lflags.all() and lcf.reshape(ndesc, -1).any(axis=1).all()
    _, cf, flags = ea.enc.encodeGathered(handle, descs, table, 1, [], coeffs=True)
    LC.check(flags, wflags[sel], "fused flags beside the coefficients", lambda q, _: q * n // per, F)
    # a wrong component c[q][s] spreads over the whole polynomial q: the unit is that of the descriptor's first slot
    LC.check(cf, wcf[sel], "fused coefficients", lambda q, _: q * n // per, F)
    assert not cf[isdead[sel]].any()                             # flag 0 and a zero polynomial


def test_gather_chunks_of_the_measured_ring(hx, K, full_ea):
    """70 descriptors of period 7 at m = 21845: a trip is 32 descriptors there, and 64 is what the library sends"""
    from helib_amd import bgv_gr_matmul as RM
    case = LC.full_gather_case(K)
    ea = full_ea
    n, d, m = ea.size(), ea.getDegree(), LC.FULL_RING[0]
    mat = RM.BlockMatMul1D(ea, np.random.default_rng(m).integers(0, 4, size=(n, 1, 1, d, d)), 2)
    maps, z = RM._Maps(ea), ea.zMStar
    maps.add(1), maps.add(z.genToPow(-1, -5)), maps.add(z.genToPow(0, -3), ea.maskSlots(0, 3))
    maps.add(z.genToPow(1, 8 - 2) * z.genToPow(-1, -1) % m, 1 - ea.maskSlots(1, 2))
    seven = [(0, k, mp) for k, mp in ((0, 0), (15, 0), (3, 1), (7, 1), (1, 2), (9, 2), (4, 3))]
    table, handle = np.stack(maps.rows), mat.handle(ea.enc)
    want = np.stack([RM.hostConstant(ea, mat, i, k, maps.rows[mp]) for i, k, mp in seven])
    wflags = want.reshape(7, -1).any(axis=1)
    assert len({x.tobytes() for x in want}) == 7 and wflags.all()
    for ndesc in (64, case.size):
        sel = np.arange(ndesc) % LC.FULL_PERIOD
        descs = np.array(seven, dtype=np.int32)[sel]
        slots, gflags = hx.bgvGfGather(handle, descs, table)
        LC.check(slots, want[sel], "gather of %d" % ndesc, lambda q, w: (q * n * d + w) // LC.THREADS, case.launches["bgv_gf_gather_kernel"])
        LC.check(gflags, wflags[sel], "gather flags of %d" % ndesc)
        LC.check(ea.enc.encodeGathered(handle, descs, table, 1, [], flags_only=True), wflags[sel], "fused flags of %d" % ndesc)
    # flags that are not all up: the masked map alone on a matrix whose blocks outside the mask are the only live ones
    A = np.zeros((n, 1, 1, d, d), dtype=np.int64)
    A[ea.maskSlots(0, 3) == 0] = 1
    zero = RM.BlockMatMul1D(ea, A, 2)
    pair = [(0, 0, 0), (0, 0, 2)]                                 # the identity sees the live blocks, the masked map none
    wz = np.stack([RM.hostConstant(ea, zero, i, k, maps.rows[mp]) for i, k, mp in pair]).reshape(2, -1).any(axis=1)
    assert wz.tolist() == [True, False]
    sel = (np.arange(case.size) % LC.FULL_PERIOD) % 2
    descs = np.array(pair, dtype=np.int32)[sel]
    LC.check(ea.enc.encodeGathered(zero.handle(ea.enc), descs, table, 1, [], flags_only=True), wz[sel], "fused flags, half of them down")
    LC.check(hx.bgvGfGather(zero.handle(ea.enc), descs, table)[1], wz[sel], "gather flags, half of them down")


# ---- 4. the linearized polynomials of a block matrix ----
def test_linpoly_kernel_past_the_cap(hx, K, full_ea):
    from helib_amd import bgv_gr_matmul as RM
    case = LC.linpoly_case(K)
    ea = full_ea
    n, d, D, P = ea.size(), ea.getDegree(), case.size, 4
    sel, pos = LC.selection(case.count, case.boundaries)
    uniq = LC.distinct_elements(np.random.default_rng(D), LC.PERIOD + len(pos), (d, d), P, 0, P)
    uniq[0].reshape(-1)[0] = 0                                    # (entries are words below P)
    want = RM.buildLinPolyCoeffs(ea, uniq)
    assert len({x.tobytes() for x in want}) == len(uniq)
    A = uniq.astype(np.uint32)[sel].reshape(1, D, D, d, d)
    mat = hx.BgvGfMatrix(ea.enc.table, A, np.zeros(n, dtype=np.int32), np.arange(n, dtype=np.int32) % D, ring=True)
    ctiles = -(-d * d // K["LP_TN"])
    LC.check(mat.coeffs().reshape(case.count, d, d), want.astype(np.uint32)[sel], "linearized polynomials",
             lambda e, w: e // K["LP_TM"] * ctiles + w // K["LP_TN"], case.launches["bgv_gf_linpoly_kernel"])


# ---- 5. the diagonal scatter of the d = 1 path ----
class _Geom:
    """what bgv_matmul.diagonalSlots asks of an EncryptedArray"""

    def __init__(self, table, n):
        self.p, self.n = table.p, n
        self.zMStar = hostnt.ZmStar(table.context.m, table.p, table.gens, table.ords)

    def size(self):
        return self.n


@pytest.mark.parametrize("dim", [-1, 0])
def test_diag_scatter_past_the_cap(hx, K, dim):
    """dim = -1: the full-matrix form, dim = 0: the one-dimension form; with and without a rotation, one diagonal zero"""
    from helib_amd import bgv_matmul as M
    case = LC.diag_case(K)
    m, p = LC.DIAG_RING
    c = _ctx(hx, m)
    table = hx.BgvSlots(c, p)
    n, ords, ndiag = c.phim, table.ords, case.size
    assert (n, ords) == (512, [256, 2])
    geom = _Geom(table, n)
    sel, pos = LC.selection(ndiag, case.boundaries)
    rng = np.random.default_rng(5 + dim)
    D = n if dim < 0 else ords[dim]
    a = rng.integers(-2 * p, 3 * p, size=(D, D))
    a.flat[:4] = [0, p - 1, -1, p]
    j = np.arange(D)
    if dim < 0:
        a[(j + 2 * ords[1]) % n, j] = p * rng.integers(-2, 3, size=n)      # off = (-2, 0): zero mod p
        zero = ([-2, 0], -1, 0)
    else:
        a[(j - 3) % D, j] = 0
        zero = ([3, 1], -1, 0)
    a[(-4) % D if dim >= 0 else (-4) % ords[0] * ords[1] + 1, 0] = p - 1      # on the diagonal of offset (4, 1), a base one
    uniq = [zero]
    for t in range(1, LC.PERIOD + len(pos)):                     # offsets 4 .. : distinct diagonals, none of them the zero one
        rd = t % 3 - 1                                           # no rotation, along dimension 0, along dimension 1
        amt = 0 if rd < 0 else [1, ords[rd] - 1, -3][t // 3 % 3]
        uniq.append(([3 + t, t % 2], rd, amt))
    slots = np.stack([M.diagonalSlots(geom, a, dim, *x) for x in uniq])
    assert len({x.tobytes() for x in slots % p}) == len(uniq) and not (slots[0] % p).any() and (slots % p == p - 1).any()
    wflags = (slots % p).any(axis=1)
    mat = hx.BgvMatrix(table, a, dim)
    wpoly, wcf = hx.bgvEncode(table, slots, [0], coeffs=True)
    descs = hx.bgvDiags(uniq)[sel]
    got, cf, nz = hx.bgvEncodeDiagonals(table, mat, descs, [0], coeffs=True)
    # (the transform behind the scatter mixes a diagonal's words: the unit is that of the diagonal's first word)
    L = case.launches["bgv_diag_scatter_kernel"]
    LC.check(cf, wcf[sel], "coefficients", lambda q, _: q * n // LC.THREADS, L)
    LC.check(got.download(), wpoly.download()[:, sel], "words")
    LC.check(nz, wflags[sel], "flags")
    LC.check(hx.bgvEncodeDiagonals(table, mat, descs)[2], wflags[sel], "the flags alone")
