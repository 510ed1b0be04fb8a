"""helib_amd.permutations without a device: Benes networks, the generator trees and the cube mapping, networks applied to
plain cubes (the reference's TestPermutationsGeneral list), and PermNetwork.applyToCtxt / PermPrecomp over the oracle
backend with keys from addMatrices4Network.  Everything is an integer: every comparison is exact."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from helib_amd import permutations as P
from helib_amd.capi import InvalidArgument
from helib_amd.ckks import LogicError
from tests import bgv_hypercube_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = {(119, 2): 400, (255, 2): 500}

# (orders, good, depth): TestPermutationsGeneral of the reference
CUBES = [([3], [1], 1), ([31], [0], 5), ([2, 3], [0, 0], 3), ([2, 3], [1, 0], 3), ([6], [1], 3), ([6, 2], [1, 0], 5),
         ([682, 2], [1, 0], 11)]


def _gens(orders, good):
    return [P.GenDescriptor(o, g, i) for i, (o, g) in enumerate(zip(orders, good))]


# ---- Benes networks ----
@pytest.mark.parametrize("n", range(1, 10))
def test_benes_network_routes_every_permutation(n):
    if n == 1:
        with pytest.raises(InvalidArgument, match="greater than one"):
            P.GeneralBenesNetwork([0])
        return
    rng = np.random.default_rng(n)
    perms = itertools.permutations(range(n)) if n <= 6 else (P.randomPerm(n, rng) for _ in range(50))
    k = P.GeneralBenesNetwork.depth(n)
    assert (1 << k) >= n > (1 << (k - 1)) or n == 2
    for pi in perms:
        net = P.GeneralBenesNetwork(pi)
        assert net.getNumLevels() == 2 * k - 1 and net.getSize() == n and net.getDepth() == k
        assert net.testNetwork(pi), pi
        assert all(v in (-1, 0, 1) for i in range(net.getNumLevels()) for v in net.getLevel(i))
    assert [net.shamt(i) for i in range(2 * k - 1)] == [((n >> d) + 1) >> 1 for d in
                                                        [(k - 1) - abs((k - 1) - i) for i in range(2 * k - 1)]]
    with pytest.raises(InvalidArgument):
        P.GeneralBenesNetwork.levelToDepthMap(n, k, 2 * k - 1)
    with pytest.raises(LogicError):
        P.GeneralBenesNetwork([0] * n)


def test_perm_helpers():
    v, pi = np.array([10, 11, 12, 13]), [2, 0, 3, 1]
    assert P.applyPermToVec(v, pi).tolist() == [12, 10, 13, 11]
    assert P.applyPermsToVec(v, pi, [1, 1, 0, 3]).tolist() == [10, 10, 12, 11]     # v[p2[p1[i]]]
    for n in (1, 2, 17):
        assert sorted(P.randomPerm(n, np.random.default_rng(n)).tolist()) == list(range(n))
    sig = P.CubeSignature([2, 3, 4])
    assert sig.getSize() == 24 and sig.getProd(1) == 12 and sig.getCoord(17, 1) == 1 and sig.getCoord(17, 2) == 1
    assert sig.addCoord(17, 1, 2) == 13 and sig.addCoord(17, 1, -1) == 13 and sig.addCoord(17, 0, 1) == 5
    assert sig.numSlices(1) == 2 and sig.numSlices(2) == 6


def test_break_perm_by_dim_is_a_product_of_column_permutations():
    rng = np.random.default_rng(8)
    for dims in ([5], [2, 3], [3, 2, 2], [2, 2, 3, 2]):
        sig = P.CubeSignature(dims)
        for _ in range(5):
            pi = P.randomPerm(sig.getSize(), rng)
            cols = P.breakPermByDim(pi, sig)
            m = len(dims)
            assert len(cols) == 2 * m - 1
            assert [c.getPermDim() for c in cols] == list(range(m)) + list(range(m - 2, -1, -1))
            v = np.arange(sig.getSize())
            for c in cols:
                e = c.makeExplicit()
                assert sorted(e.tolist()) == v.tolist()
                # a column permutation changes the coordinate of its dimension alone
                step = sig.getProd(c.getPermDim() + 1)
                assert all((int(e[k]) - k) % step == 0 and
                           all(sig.getCoord(int(e[k]), d) == sig.getCoord(k, d) for d in range(m) if d != c.getPermDim())
                           for k in range(sig.getSize()))
            out = np.arange(sig.getSize())
            for c in cols:
                out = P.applyPermToVec(out, c.makeExplicit())
            # applied in order, first to last, the column permutations give pi
            assert np.array_equal(out, pi)


# ---- the cube tests ----
@pytest.mark.parametrize("orders,good,depth", CUBES)
def test_networks_on_plain_cubes(orders, good, depth):
    trees = P.GeneratorTrees()
    cost = trees.buildOptimalTrees(_gens(orders, good), depth)
    n = int(np.prod(orders))
    assert cost is not None and cost > 0
    assert trees.getSize() == n and trees.numLayers() <= depth
    assert np.array_equal(trees.mapToCube()[trees.mapToArray()], np.arange(n))
    assert np.array_equal(trees.mapToArray()[trees.mapToCube()], np.arange(n))
    assert trees.getCubeDims() == list(orders)
    assert int(np.prod(trees.getCubeSubDims())) == n
    sig = P.CubeSignature(trees.getCubeDims())
    rng = np.random.default_rng(depth)
    every = (orders, good) in (([6], [1]), ([2, 3], [1, 0]))
    perms = list(itertools.permutations(range(n))) if every else [P.randomPerm(n, rng) for _ in range(3)]
    assert len(perms) == (720 if every else 3)
    leaves = {T.getAuxKey(): list(T.leaves()) for T in trees.trees}
    for pi in perms:
        net = P.PermNetwork(pi, trees)
        assert net.depth() == trees.numLayers()
        cube = P.HyperCube(sig, np.arange(n))
        net.applyToCube(cube)
        assert np.array_equal(cube.getData(), P.applyPermToVec(np.arange(n), pi)), pi
        for i in range(net.depth()):
            lyr = net.getLayer(i)
            if lyr.isID:
                assert not lyr.getShifts().any()
                continue
            leaf = [d for d in leaves[lyr.getGenIdx()] if d.e == lyr.getE()]
            assert leaf
            s = lyr.getShifts()
            if good[lyr.getGenIdx()] and leaf[0].good:
                assert s.min() >= 0 and s.max() < max(d.size for d in leaf)
            if not good[lyr.getGenIdx()]:                # a bad dimension: nothing leaves it
                dim = lyr.getGenIdx()
                c = np.array([sig.getCoord(j, dim) for j in range(n)])
                moved = c + lyr.getE() * s
                assert moved.min() >= 0 and moved.max() < orders[dim]


def test_depth_bound():
    # two generators: the one that is not the middle needs two layers, the middle one
    assert P.GeneratorTrees().buildOptimalTrees(_gens([2, 3], [0, 0]), 2) is None
    assert P.GeneratorTrees().buildOptimalTrees(_gens([6, 2], [1, 0]), 2) is None
    assert P.GeneratorTrees().buildOptimalTrees(_gens([6, 2], [1, 0]), 3) == 9
    # a single generator is the middle: one collapsed layer fits depth 1 (as in the reference, which finds 60 here)
    t = P.GeneratorTrees()
    assert t.buildOptimalTrees(_gens([31], [0]), 1) == 60 and t.numLayers() == 1
    for bad in (0, -1):
        with pytest.raises(InvalidArgument, match="depthBound"):
            P.GeneratorTrees().buildOptimalTrees(_gens([31], [0]), bad)
    t = P.GeneratorTrees()
    assert t.buildOptimalTrees([], 3) == 0 and t.numTrees() == 0 and t.getSize() == 1
    net = P.PermNetwork([0], t)
    assert net.depth() == 0

    class Ea:
        def dimension(self):
            return 2

        def sizeOfDimension(self, i):
            return (2, 3)[i]

        def nativeDimension(self, i):
            return False

        def size(self):
            return 6
    pip = P.PermIndepPrecomp(Ea(), 2)
    with pytest.raises(LogicError, match="buildOptimalTrees failed"):
        pip.getCost()
    with pytest.raises(LogicError, match="buildOptimalTrees failed"):
        P.PermPrecomp(pip, np.arange(6))
    ok = P.PermIndepPrecomp(Ea(), 3)
    assert ok.getCost() == 8 and ok.getDepth() == 3
    with pytest.raises(LogicError, match="pi wrong size"):
        P.PermPrecomp(ok, np.arange(5))


def test_single_good_generator_of_order_three_is_one_layer_of_shift_amounts():
    trees = P.GeneratorTrees()
    assert trees.buildOptimalTrees(_gens([3], [1]), 1) == 2
    leaf, = trees[0].leaves()
    assert (leaf.size, leaf.good, leaf.e, leaf.frstBenes, leaf.scndBenes) == (3, True, 1, [3], [])
    for pi in itertools.permutations(range(3)):
        net = P.PermNetwork(pi, trees)
        assert net.depth() == 1
        col = P.ColPerm(P.CubeSignature([3]), pi, 0)
        shifts, nonZero = col.getShiftAmounts()
        lyr = net.getLayer(0)
        assert lyr.isID == (not nonZero) == (list(pi) == [0, 1, 2])
        if not lyr.isID:
            assert np.array_equal(lyr.getShifts(), np.where(shifts < 0, shifts + 3, shifts))
            # the element at j moves shifts[j] places: out[j + shifts[j]] = in[j]
            assert all(pi[(j + int(shifts[j])) % 3] == j for j in range(3))


def test_amounts_follow_make_mask():
    lyr = P.PermNetLayer()
    lyr.shifts = np.array([3, 0, -1, 3, 2, -1, 0, 5])
    got = lyr.amounts()
    assert [a for a, _ in got] == [0, 3, -1, 2, 5]           # zero first, then the first amount not served yet
    assert [m.tolist() for _, m in got][1] == [1, 0, 0, 1, 0, 0, 0, 0]
    assert np.array_equal(sum(m for _, m in got), np.ones(8, dtype=np.int64))
    lyr.shifts = np.array([2, 2, 1])
    assert [a for a, _ in lyr.amounts()] == [2, 1]           # nobody stays: no mask for zero


# ---- end to end over the oracle backend ----
def _run(ea, sk, cc, pi, depth, a):
    from helib_amd import keys as hk
    pip = P.PermIndepPrecomp(ea, depth)
    pp = P.PermPrecomp(pip, pi)
    hk.addMatrices4Network(sk, pp.net)
    ct = ea.encrypt(sk, a)
    assert pp.apply(ct) is ct
    got = ea.decrypt_batch(ct, sk)
    assert np.array_equal(got, P.applyPermToVec(a[0], pi)[None]), pi
    assert np.array_equal(pp.apply(a), got)
    assert ct.isCorrect()
    return pp, ct


def test_all_permutations_of_four_slots_over_the_oracle():
    m, p = 119, 2
    cc, sk, ea = H.setup(m, p, BITS[m, p], keys=False)
    assert ea.zMStar.signedOrds() == [2, -2]
    a = np.array([[1, 0, 1, 1]])
    for pi in itertools.permutations(range(4)):
        _run(ea, sk, cc, np.array(pi), 3, a if sum(pi[:2]) % 2 else np.array([[0, 1, 0, 0]]))


def test_permutations_of_sixteen_slots_over_the_oracle():
    m, p = 255, 2
    cc, sk, ea = H.setup(m, p, BITS[m, p], keys=False)
    assert ea.zMStar.signedOrds() == [-8, 2]
    n = ea.size()
    rng = np.random.default_rng(3)
    swap = np.arange(n)
    swap[[2, 11]] = [11, 2]
    perms = [np.arange(n), np.roll(np.arange(n), 1), np.arange(n)[::-1].copy(), swap] + [P.randomPerm(n, rng) for _ in range(3)]
    a = rng.integers(0, p, size=(1, n))
    a[0, :2] = [1, 0]
    for pi in perms:
        pp, ct = _run(ea, sk, cc, pi, 5, a)
    # the identity: every layer is the identity and the ciphertext's words stay as they are
    pp = P.PermPrecomp(P.PermIndepPrecomp(ea, 5), np.arange(n))
    assert pp.net.depth() == 5 and all(pp.net.getLayer(i).isID for i in range(5))
    ct = ea.encrypt(sk, a)
    before = {h: part.download().copy() for h, part in ct.parts.items()}
    noise = ct.lnNoise
    pp.apply(ct)
    assert ct.lnNoise == noise and list(ct.parts) == list(before)
    assert all(np.array_equal(before[h], part.download()) for h, part in ct.parts.items())


# ---- refusals and symbols ----
def test_refusals():
    m, p = 119, 2
    cc, sk, ea = H.setup(m, p, BITS[m, p], keys=False)
    from helib_amd import keys as hk
    pp = P.PermPrecomp(P.PermIndepPrecomp(ea, 3), np.array([1, 0, 3, 2]))
    hk.addMatrices4Network(sk, pp.net)
    ct = ea.encrypt(sk, np.array([[1, 0, 0, 1]]))
    assert not hasattr(ct.ops, "maskFan")
    with pytest.raises(LogicError, match="no maskFan"):
        pp.apply(ct, fused=True)
    with pytest.raises(LogicError, match="no maskFan"):
        pp.net.applyToCtxt(ct, ea, fused=True)
    assert P.PermNetwork.fuseMaskFan in (True, False)
    with pytest.raises(LogicError, match="applyToPtxt is not implemented"):
        pp.net.applyToPtxt([0, 1], ea)
    with pytest.raises(InvalidArgument):
        pp.apply(np.zeros(4))


def test_symbols_are_declared_listed_and_exported():
    from helib_amd import build, capi
    header = open(os.path.join(ROOT, "include", "helib_amd.h")).read()
    so = build.build()
    dyn = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    lib = capi.lib()
    assert re.search(r"\bint hx_mask_fan\(", header)
    assert "hx_mask_fan" in capi.SYMBOLS
    assert re.search(r" T hx_mask_fan$", dyn, re.M)
    assert len(lib.hx_mask_fan.argtypes) == 6
    assert "src/PermNetwork.cpp:239-242" in header and "HX_NO_MASK_FAN" in header
    text = subprocess.run(["nm", "-C", so], capture_output=True, text=True, check=True).stdout
    assert "mask_fan_kernel" in text
    sw = open(os.path.join(ROOT, "helib_amd", "csrc", "switches.h")).read()
    assert 'on("HX_NO_MASK_FAN")' in sw
    assert hasattr(capi, "maskFan")
    from helib_amd import keys
    assert hasattr(keys, "addMatrices4Network")
