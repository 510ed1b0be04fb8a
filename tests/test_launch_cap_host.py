"""The shapes of tests/test_launch_cap_gpu.py, derived on the host (no GPU).  Every kernel of the slot paths for d > 1,
and the diagonal scatter of the d = 1 path, is launched with at most BGV_MAX_BLOCKS workgroups and walks the rest of its
work in a grid-stride loop.  This file reads the cap and the tile constants out of the sources by regular expression,
restates each launch's trip count, and derives every batch, descriptor count and matrix size of the GPU file as the
smallest size whose work is at least 1.5 x cap plus a ragged remainder -- so a raised cap grows the shapes instead of
dropping them below it, and a constant that can no longer be parsed fails here.  It also holds the periodic construction
of the big inputs (big[i] = base[i % 13], a few positions overwritten with elements that occur nowhere else) and proves
it against the restatement alone at one small ring."""
import collections
import os
import re

import numpy as np
import pytest

from helib_amd import hostnt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "helib_amd", "csrc")
THREADS = 256              # __launch_bounds__(256) and blocks_for's 256 words per workgroup: the one-thread-per-word kernels
PERIOD = 13                # prime, while every stride of the launch arithmetic is a power of two times a small number
FULL_PERIOD = 7            # the 64-descriptor chunks at the measured ring: a trip there is 32 descriptors
RAGGED_DESCS = 37          # descriptors past 1.5 trips: prime to 13, to 7 and to every power of two
SOURCES = {"bgv_slots.h": ("BGV_MAX_BLOCKS",), "bgv_gf.hip": ("GF_TB", "GF_EK", "GF_DI"),
           "bgv_crt.hip": ("CRT_TB", "CRT_EK", "CRT_DI"), "bgv_gf_linalg.hip": ("LP_TM", "LP_TN"), "gather_map.h": ("GM_THREADS",)}
TODAY = {"BGV_MAX_BLOCKS": 2048, "GF_TB": 16, "GF_EK": 256, "GF_DI": 64, "CRT_TB": 16, "CRT_EK": 256, "CRT_DI": 64,
         "LP_TM": 64, "LP_TN": 64, "GM_THREADS": 256}

GF_RINGS = [(85, 2, 4), (13, 3, 2), (341, 2, 2)]
CRT_RINGS = [(85, 2), (341, 2)]
GATHER_RINGS = [(31, 2, 3), (85, 2, 4), (803, 3, 2)]
FULL_RING = (21845, 2, 2)
DIAG_RING = (1024, 12289)


def constants(csrc=CSRC):
    """{name: value} of the launch constants, read from the text of the sources; a name that is not found exactly once as
    `constexpr <integer type> NAME = <digits>;` raises AssertionError"""
    out = {}
    for name, wanted in SOURCES.items():
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        for c in wanted:
            found = re.findall(r"^\s*constexpr\s+(?:unsigned|int|uint32_t|size_t)\s+%s\s*=\s*(\d+)\s*;" % c, text, re.M)
            assert len(found) == 1, "%s: %d definitions of %s" % (name, len(found), c)
            out[c] = int(found[0])
    return out


def _ceil(a, b):
    return -(-a // b)


class Launch(collections.namedtuple("Launch", "work grid trips last")):
    """`work` workgroups' worth of units on a grid of min(work, cap): trips of the grid-stride loop, and the workgroups
    that still have a unit in the last one"""

    @property
    def ragged(self):
        return 0 < self.last < self.grid

    def locate(self, unit):
        """(trip, workgroup) of a work unit (a tile, or a word's block of 256)"""
        return unit // self.grid, unit % self.grid


def launch(work, cap):
    grid = min(max(work, 1), cap)
    trips = _ceil(work, grid)
    return Launch(work, grid, trips, work - (trips - 1) * grid)


def word_launch(words, cap):
    """one thread per word: ceil(words / 256) workgroups"""
    return launch(_ceil(words, THREADS), cap)


def gm_group(d):
    dp = 1
    while dp < d:
        dp *= 2
    return dp


def gather_map_launch(units, d, K):
    """bgv_gf_gather_map_kernel (gather_map.h): GM_THREADS / dp units per workgroup, the same passes for every thread"""
    return launch(_ceil(units, K["GM_THREADS"] // gm_group(d)), K["BGV_MAX_BLOCKS"])


def ring(m, p):
    """(d, nslots, phi(m))"""
    z = hostnt.ZmStar(m, p)
    return z.ordP, z.getNSlots(), z.ordP * z.getNSlots()


def _jc(d):
    return 1 if d == 1 else 4 if d <= 4 else 8         # decode_out's choice of bgv_gf_decode_kernel<JC>


def _batch(inner, tb, cap):
    """the smallest batch of 1.5 x cap tiles at `inner` tiles per 16 elements, one more batch tile, and a remainder that
    leaves the last tile ragged: 5 elements (a full quad of a thread and a single one), 3 (a partial quad) where the
    batch tiles come in pairs"""
    return tb * (_ceil(3 * cap, 2 * inner) + 1) + (5 if inner == 1 else 3)


Case = collections.namedtuple("Case", "size count launches strides boundaries")
# size: the batch / descriptors / matrix dimension; count: the periodic elements (size, or the D^2 entries of a matrix);
# launches {kernel: Launch}; strides [(stride, unit)]: an output taken `stride` units too early equals the right one
# under the period only if stride is a multiple of period x unit; boundaries: the element (descriptor, entry) indices at
# which a first trip ends


def gf_case(m, p, K):
    cap, tb = K["BGV_MAX_BLOCKS"], K["GF_TB"]
    d, n, N = ring(m, p)
    ktiles = _ceil(N + d - 1, K["GF_EK"])
    dinner = _ceil(n, K["GF_DI"]) * _ceil(d, _jc(d))
    B = _batch(min(ktiles, dinner), tb, cap)
    btiles = _ceil(B, tb)
    launches = {"bgv_gf_map_kernel": word_launch(B * n * d, cap), "bgv_gf_encode_kernel": launch(ktiles * btiles, cap),
                "bgv_gf_fold_kernel": word_launch(B * N, cap), "bgv_gf_decode_kernel": launch(dinner * btiles, cap)}
    strides = [(tb, 1), (cap, ktiles), (cap, dinner), (cap * THREADS, n * d), (cap * THREADS, N)]
    bounds = sorted({cap // ktiles * tb, cap // dinner * tb, cap * THREADS // (n * d), cap * THREADS // N})
    return Case(B, B, launches, strides, bounds)


def crt_case(m, p, K):
    """the decode has ceil(nslots / 64) tiles per 16 elements: at a ring whose encode has two it stays inside one trip"""
    cap, tb = K["BGV_MAX_BLOCKS"], K["CRT_TB"]
    d, n, N = ring(m, p)
    ld = _ceil(N, 4) * 4
    ktiles, itiles = _ceil(ld, K["CRT_EK"]), _ceil(n, K["CRT_DI"])
    B = _batch(ktiles, tb, cap)
    btiles = _ceil(B, tb)
    launches = {"bgv_crt_encode_kernel": launch(ktiles * btiles, cap), "bgv_crt_decode_kernel": launch(itiles * btiles, cap)}
    bounds = sorted(b for b in {cap // ktiles * tb, cap // itiles * tb} if b < B - 1)
    return Case(B, B, launches, [(tb, 1), (cap, ktiles), (cap, itiles)], bounds)


def gather_case(m, p, K):
    """ndesc: 1.5 x the larger of the descriptors in the gather's first trip and in the fused kernel's first pass"""
    cap = K["BGV_MAX_BLOCKS"]
    d, n, N = ring(m, p)
    per = K["GM_THREADS"] // gm_group(d)
    ndesc = max(3 * cap * THREADS // (2 * n * d), 3 * cap * per // (2 * n)) + RAGGED_DESCS
    launches = {"bgv_gf_gather_kernel": word_launch(ndesc * n * d, cap), "bgv_gf_gather_map_kernel": gather_map_launch(ndesc * n, d, K)}
    return Case(ndesc, ndesc, launches, [(cap * THREADS, n * d), (cap * per, n)], sorted({cap * THREADS // (n * d), cap * per // n}))


def full_gather_case(K, chunk=64):
    """the chunk the library sends at the measured ring (bgv_gf_matmul.GATHER_CHUNK), and 70 descriptors of period 7"""
    cap = K["BGV_MAX_BLOCKS"]
    d, n, N = ring(*FULL_RING[:2])
    per = K["GM_THREADS"] // gm_group(d)
    launches = {"chunk: bgv_gf_gather_kernel": word_launch(chunk * n * d, cap),
                "chunk: bgv_gf_gather_map_kernel": gather_map_launch(chunk * n, d, K)}
    ndesc = chunk + chunk // 10                                # a third, ragged trip: 70 = 10 periods
    launches.update({"bgv_gf_gather_kernel": word_launch(ndesc * n * d, cap), "bgv_gf_gather_map_kernel": gather_map_launch(ndesc * n, d, K)})
    return Case(ndesc, ndesc, launches, [(cap * THREADS, n * d), (cap * per, n)], [])


def linpoly_case(K):
    """nb = 1 and the smallest D with 1.5 x cap tiles; nb D <= nslots bounds D"""
    cap, tm = K["BGV_MAX_BLOCKS"], K["LP_TM"]
    d, n, N = ring(*FULL_RING[:2])
    ctiles = _ceil(d * d, K["LP_TN"])
    D = 1
    while _ceil(D * D, tm) * ctiles < 3 * cap // 2:
        D += 1
    assert D <= n, "no matrix over %d slots reaches 1.5 x cap" % n
    return Case(D, D * D, {"bgv_gf_linpoly_kernel": launch(_ceil(D * D, tm) * ctiles, cap)}, [(tm, 1), (cap, ctiles)], [cap // ctiles * tm])


def diag_case(K):
    """1.5 x cap descriptors, one more, and two for the ragged end"""
    cap = K["BGV_MAX_BLOCKS"]
    N = ring(*DIAG_RING)[2]
    ndiag = 3 * cap // 2 + 1 + 2
    return Case(ndiag, ndiag, {"bgv_diag_scatter_kernel": word_launch(ndiag * N, cap)}, [(cap * THREADS, N)], [cap * THREADS // N])


# ---- the periodic construction ----
def selection(count, boundaries, period=PERIOD):
    """-> (sel [count], positions): big = uniq[sel] with uniq = base (period elements) followed by one element per
    position that occurs nowhere else.  The positions: index 0, around every boundary the last index of trip one and the
    first two of trip two, and the very last index."""
    pos = {0, count - 1}
    for b in boundaries:
        pos |= {x for x in (b - 1, b, b + 1) if 0 < x < count - 1}
    pos = sorted(pos)
    sel = np.arange(count) % period
    sel[pos] = period + np.arange(len(pos))
    return sel, pos


def check(got, want, what, unit=None, launched=None):
    """np.array_equal with the place of the first wrong word: its flat index, the leading index (element, descriptor,
    entry) and, given unit(leading, rest) -> the launch's work unit, the trip and workgroup it belongs to"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    flat = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
    inner = int(np.prod(got.shape[1:], dtype=np.int64))
    lead, rest = flat // inner, flat % inner
    where = ""
    if unit is not None:
        u = unit(lead, rest)
        where = ", work unit %d = trip %d, workgroup %d of %d" % ((u,) + launched.locate(u) + (launched.grid,))
    raise AssertionError("%s: first wrong word at flat index %d = [%d] + %d%s: got %s, want %s (%d words differ)"
                         % (what, flat, lead, rest, where, got.reshape(-1)[flat], want.reshape(-1)[flat],
                            int(np.count_nonzero(got != want))))


# ---- the tests ----
@pytest.fixture(scope="module")
def K():
    return constants()


def _all_cases(K):
    out = {("gf",) + r: gf_case(r[0], r[1], K) for r in GF_RINGS}
    out.update({("crt",) + r: crt_case(r[0], r[1], K) for r in CRT_RINGS})
    out.update({("gather",) + r: gather_case(r[0], r[1], K) for r in GATHER_RINGS})
    out["gather", "full"] = full_gather_case(K)
    out["linpoly",] = linpoly_case(K)
    out["diag",] = diag_case(K)
    return out


def test_constants_parse_and_a_lost_one_fails(K, tmp_path):
    assert set(K) == set(TODAY) and all(v > 0 for v in K.values())
    for name in SOURCES:                                       # a renamed constant is an error, not a silent default
        with open(os.path.join(CSRC, name)) as f:
            (tmp_path / name).write_text(f.read().replace("BGV_MAX_BLOCKS =", "BGV_MOST_BLOCKS ="))
    with pytest.raises(AssertionError, match="BGV_MAX_BLOCKS"):
        constants(str(tmp_path))


def test_every_case_takes_a_second_trip_with_a_ragged_end(K):
    single = {(("crt", 341, 2), "bgv_crt_decode_kernel")}      # one slot tile: past the cap at (85, 2) only
    for key, case in _all_cases(K).items():
        for kernel, ln in case.launches.items():
            if (key, kernel) in single:
                continue
            assert ln.grid == K["BGV_MAX_BLOCKS"] and ln.trips >= 2, (key, kernel, ln)
            assert ln.ragged or kernel.startswith("chunk:"), (key, kernel, ln)     # (the library's chunk ends on a trip)
        assert all(0 < b < case.count - 1 for b in case.boundaries), (key, case.boundaries)


def test_no_stride_is_a_multiple_of_the_period(K):
    for key, case in _all_cases(K).items():
        period = FULL_PERIOD if key == ("gather", "full") else PERIOD
        for stride, unit in case.strides:
            assert stride % (period * unit) != 0, (key, stride, unit)
    # the strides in elements where they are whole: 16 per tile, 2048 tiles, 8192 and 32768 per trip, 32 descriptors
    cap = K["BGV_MAX_BLOCKS"]
    d, n, N = ring(85, 2)
    for s in (K["GF_TB"], cap, cap * THREADS // (n * d), cap * K["GF_TB"]):
        assert s % PERIOD != 0
    d, n, N = ring(*FULL_RING[:2])
    assert cap * THREADS % (n * d) == 0 and cap * THREADS // (n * d) % FULL_PERIOD != 0


def test_todays_numbers(K):
    """what the formulas give at today's constants; another cap moves them and this test with it"""
    if K != TODAY:
        pytest.fail("the launch constants changed: %s -- restate the figures of this test for them" % sorted(set(K.items()) ^ set(TODAY.items())))
    C = _all_cases(K)
    g = C["gf", 85, 2, 4]
    assert ring(85, 2) == (8, 8, 64) and g.size == 16 * 3073 + 5 == 49173
    assert (g.launches["bgv_gf_encode_kernel"].work, g.launches["bgv_gf_decode_kernel"].work) == (3074, 3074)
    assert g.launches["bgv_gf_map_kernel"].work == g.launches["bgv_gf_fold_kernel"].work == 12294
    g = C["gf", 13, 3, 2]
    assert ring(13, 3) == (3, 4, 12) and g.size == 49173 and g.launches["bgv_gf_decode_kernel"].work == 3074
    g = C["gf", 341, 2, 2]
    assert ring(341, 2) == (10, 30, 300) and g.size == 16 * 1537 + 3 == 24595
    assert (g.launches["bgv_gf_encode_kernel"].work, g.launches["bgv_gf_decode_kernel"].work) == (3076, 3076)
    assert (C["crt", 85, 2].size, C["crt", 341, 2].size) == (49173, 24595)
    assert C["crt", 341, 2].launches["bgv_crt_encode_kernel"].work == 3076
    g = C["gather", 31, 2, 3]
    assert ring(31, 2) == (5, 6, 30) and g.size == 26251
    assert g.launches["bgv_gf_gather_kernel"].work == _ceil(787530, 256)
    assert g.launches["bgv_gf_gather_map_kernel"][1:] == (2048, 3, _ceil(157506 - 2 * 65536, 32))
    assert (C["gather", 85, 2, 4].size, C["gather", 803, 3, 2].size) == (12325, 1129)
    f = C["gather", "full"]
    assert ring(21845, 2) == (16, 1024, 16384) and f.size == 70
    assert f.launches["chunk: bgv_gf_gather_map_kernel"].trips == 2 and f.launches["chunk: bgv_gf_gather_kernel"].trips == 2
    assert f.launches["bgv_gf_gather_map_kernel"].trips == 3
    lp = C["linpoly",]
    assert lp.size == 222 and lp.launches["bgv_gf_linpoly_kernel"].work == 771 * 4 == 3084
    dg = C["diag",]
    assert dg.size == 3073 + 2 and dg.launches["bgv_diag_scatter_kernel"].work == 2 * 3075


def test_the_library_chunk_is_the_one_assumed():
    from helib_amd import bgv_gf_matmul as GM
    assert GM.GATHER_CHUNK == 64


def test_selection():
    sel, pos = selection(100, [32, 50])
    assert pos == [0, 31, 32, 33, 49, 50, 51, 99]
    assert sel[pos].tolist() == list(range(13, 21))
    rest = np.setdiff1d(np.arange(100), pos)
    assert np.array_equal(sel[rest], rest % 13)
    with pytest.raises(AssertionError, match=r"flat index 7 = \[2\] \+ 1, work unit 2 = trip 1, workgroup 0 of 2"):
        check(np.arange(12).reshape(4, 3), np.where(np.arange(12) >= 7, 0, np.arange(12)).reshape(4, 3), "x",
              unit=lambda lead, rest: lead, launched=launch(4, 2))


def test_periodic_construction_against_the_restatement_alone():
    """40 elements of (13, 3, 2) encoded one by one equal the tiled expectation built from the 13 + 5 distinct ones"""
    from tests import intraslot_ref as IR
    ref = IR.tables(13, 3, 2)
    P, n, d = 9, ref.nslots, ref.d
    sel, pos = selection(40, [16])
    assert pos == [0, 15, 16, 17, 39]
    rng = np.random.default_rng(40)
    uniq = distinct_elements(rng, PERIOD + len(pos), (n, d), P)
    big = uniq[sel]
    want = ref.encode(uniq)[sel]
    for i in range(40):
        assert np.array_equal(ref.encode(big[i:i + 1])[0], want[i]), i
    assert np.array_equal(ref.decode(want), big % P)
    assert len({x.tobytes() for x in want}) == PERIOD + len(pos)       # distinct inputs, distinct outputs: a wrong trip shows


def distinct_elements(rng, count, shape, P, lo=None, hi=None):
    """count pairwise distinct (also modulo P) random elements of `shape` in [-3 P, 5 P): signed and out of range;
    element 1 is all P - 1, element 0 starts with -1"""
    lo, hi = (-3 * P, 5 * P) if lo is None else (lo, hi)
    while True:
        a = rng.integers(lo, hi, size=(count,) + tuple(shape))
        a[1] = P - 1
        a[0].reshape(-1)[0] = -1
        if len({(x % P).tobytes() for x in a}) == count:
            return a
