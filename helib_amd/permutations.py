"""Arbitrary slot permutations: the reference's permutations.h family, restated in its names.

  Permut, applyPermToVec, applyPermsToVec, randomPerm       src/permutations.cpp:20-108 (out[i] = v[pi[i]])
  CubeSignature, HyperCube                                  as far as ColPerm and applyToCube need them (getCoord, addCoord, slices)
  ColPerm, breakPermByDim                                   src/permutations.cpp:110-369; the n1 perfect matchings of the bipartite
                                                            graph of breakPermTo3 are found here by augmenting paths
  GeneralBenesNetwork                                       src/BenesNetwork.cpp
  GenDescriptor, SubDimension, OneGeneratorTree,
  GeneratorTrees                                            src/OptimizePermutations.cpp (the memoised upper / lower optimisation and the
                                                            collapsing of Benes levels), src/permutations.cpp:371-499 (the cube mapping)
  PermNetLayer, PermNetwork                                 src/PermNetwork.cpp: buildNetwork, applyToCube, applyToCtxt
  PermIndepPrecomp, PermPrecomp                             src/permutations.cpp:531-584

PermNetwork.applyToCtxt runs a layer as the reference does (src/PermNetwork.cpp:217-259): per distinct shift amount, in
makeMask's order (zero first, then the first amount still unused), tmp = c; tmp.multByConstant(mask); tmp.smartAutomorph;
sum += tmp.  The fused form gets the K masked copies of a layer from one capi.maskFan (hx_mask_fan) per pair
of parts and gives each copy multByConstant's bookkeeping; automorphisms and the sum run as before, so the words and the
bookkeeping are those of the unfused form.  It works over every BGV array class with _encodedMask and smartAutomorph
(bgv, bgv_crt, bgv_hypercube, bgv_pr, bgv_gf, bgv_gr: a permutation moves whole slot values) and, unfused, over
ckks.EncryptedArrayCx (one native dimension of m/4 slots, the mask encoded as that class's shift encodes its masks).
Non-native dimensions need nothing special: the layer's masks zero what would wrap and the rotation is a plain
smartAutomorph by g^(e shamt).

Refused: applyToPtxt on a polynomial (the reference does not implement it either).  There is no C++ twin of this module.
keys.addMatrices4Network generates the key-switching matrices a network needs.
"""
import functools

import numpy as np

from . import capi
from . import ctxt as hc
from .ckks import LogicError

NTL_MAX_LONG = (1 << 63) - 1


def _invalid(msg):
    return capi.InvalidArgument(capi.HX_ERR_INVALID, msg)


# ---------------------------------------------------------------------------------------------
# permutations as vectors
# ---------------------------------------------------------------------------------------------
def Permut(v):
    """a permutation of [0, n): a numpy int64 vector"""
    return np.asarray(v, dtype=np.int64).reshape(-1)


def applyPermToVec(v, pi):
    """out[i] = v[pi[i]]"""
    return np.asarray(v)[Permut(pi)]


def applyPermsToVec(v, p2, p1):
    """out[i] = v[p2[p1[i]]]"""
    p1, p2 = Permut(p1), Permut(p2)
    if len(p1) != len(p2):
        raise LogicError("Permutation p1 and p2 sizes differ")
    return np.asarray(v)[p2[p1]]


def randomPerm(n, rng):
    """src/permutations.cpp:94-108 with rng.integers(m) for RandomBnd(m)"""
    perm = np.arange(n, dtype=np.int64)
    for m in range(n, 0, -1):
        p = int(rng.integers(m))
        perm[p], perm[m - 1] = perm[m - 1], perm[p]
    return perm


# ---------------------------------------------------------------------------------------------
# the cube
# ---------------------------------------------------------------------------------------------
class CubeSignature:
    """dims and the products of their tails; index = sum coord[d] * getProd(d + 1) (the last dimension runs fastest)"""

    def __init__(self, dims):
        self.dims = [int(d) for d in dims]
        if any(d <= 0 for d in self.dims):
            raise _invalid("CubeSignature: dimensions must be positive")
        self.prods = [1] * (len(self.dims) + 1)
        for i in range(len(self.dims) - 1, -1, -1):
            self.prods[i] = self.prods[i + 1] * self.dims[i]

    def getSize(self):
        return self.prods[0]

    def getNumDims(self):
        return len(self.dims)

    def getDim(self, d):
        return self.dims[d]

    def getProd(self, d):
        return self.prods[d]

    def getCoord(self, i, d):
        return i % self.prods[d] // self.prods[d + 1]

    def addCoord(self, i, d, offset):
        """the index of i with `offset` added to its coordinate d, modulo that dimension"""
        c = self.getCoord(i, d)
        return i + ((c + offset) % self.dims[d] - c) * self.prods[d + 1]

    def numSlices(self, d=1):
        return self.getSize() // self.prods[d]

    def sliceSize(self, d=1):
        return self.prods[d]


class HyperCube:
    """data over a CubeSignature; slice(i, d): the view of the i-th subcube of the dimensions d.."""

    def __init__(self, sig, data=None):
        self.sig = sig
        self.data = np.zeros(sig.getSize(), dtype=np.int64) if data is None else np.array(data)
        if len(self.data) != sig.getSize():
            raise _invalid("HyperCube: data and signature differ in size")

    def getSig(self):
        return self.sig

    def getData(self):
        return self.data

    def getSize(self):
        return self.sig.getSize()

    def getDim(self, d):
        return self.sig.getDim(d)

    def getCoord(self, i, d):
        return self.sig.getCoord(i, d)

    def addCoord(self, i, d, offset):
        return self.sig.addCoord(i, d, offset)

    def numSlices(self, d=1):
        return self.sig.numSlices(d)

    def slice(self, i, d):
        n = self.sig.sliceSize(d)
        return self.data[i * n:(i + 1) * n]

    def slices(self, d):
        return (self.slice(i, d) for i in range(self.numSlices(d)))

    def __getitem__(self, i):
        return self.data[i]

    def __setitem__(self, i, v):
        self.data[i] = v

    def __eq__(self, other):
        return self.sig.dims == other.sig.dims and np.array_equal(self.data, other.data)


# ---------------------------------------------------------------------------------------------
# Benes networks
# ---------------------------------------------------------------------------------------------
class GeneralBenesNetwork:
    """level[i][j] in {0, 1, -1}: an edge from node j of level i to node j + level[i][j] * shamt(i) of level i + 1;
    2 k - 1 levels of n nodes, k = depth(n).  Following the edges from input j ends at the j1 with perm[j1] = j."""

    @staticmethod
    def depth(n):
        k = 1
        while (1 << k) < n:
            k += 1
        return k

    @staticmethod
    def levelToDepthMap(n, k, i):
        if not 0 <= i < 2 * k - 1:
            raise _invalid("Level number i not in [0, 2 * k - 1)")
        return (k - 1) - abs((k - 1) - i)

    @staticmethod
    def _shamt(n, k, i):
        d = GeneralBenesNetwork.levelToDepthMap(n, k, i)
        return ((n >> d) + 1) >> 1

    def shamt(self, i):
        return self._shamt(self.n, self.k, i)

    def getDepth(self):
        return self.k

    def getSize(self):
        return self.n

    def getNumLevels(self):
        return 2 * self.k - 1

    def getLevel(self, i):
        if not 0 <= i < 2 * self.k - 1:
            raise _invalid("Level number i not in [0, 2 * k - 1)")
        return self.level[i]

    def __init__(self, perm):
        perm = [int(x) for x in perm]
        n = self.n = len(perm)
        if n <= 1:
            raise _invalid("permutation length must be greater than one")
        k = self.k = self.depth(n)
        iperm = [-1] * n
        for j, j1 in enumerate(perm):
            if not 0 <= j1 < n:
                raise LogicError("permutation element out of range")
            iperm[j1] = j
        if -1 in iperm:
            raise LogicError("permutation element not processed")
        self.level = [[0] * n for _ in range(2 * k - 1)]
        ilevel = [[0] * n for _ in range(2 * k - 1)]
        self._init(0, 0, perm, iperm, ilevel)

    def _init(self, d, delta_j, perm, iperm, ilevel):
        """the recursion of src/BenesNetwork.cpp:26-257: the outer two levels of this sub-network by walking the
        cycles of the two-colouring, then the upper and the lower inner network"""
        n, k, level = self.n, self.k, self.level
        sz = len(perm)
        if d == k - 1:
            if sz == 2 and perm[0] != 0:                     # the swap
                level[d][delta_j], level[d][delta_j + 1] = 1, -1
                ilevel[d][delta_j], ilevel[d][delta_j + 1] = 1, -1
            else:
                for j in range(sz):
                    level[d][delta_j + j] = ilevel[d][delta_j + j] = 0
            return
        nlev = 2 * k - 1
        sz0 = self._shamt(n, k, d)                           # size of the upper inner network
        sz1 = sz - sz0
        if abs(sz0 - sz1) > 1:
            raise LogicError("sz1 must be within 1 of sz0")
        ident = list(range(sz))
        xperm, xiperm = (ident, perm), (ident, iperm)
        first_level = (level[d], ilevel[nlev - 1 - d])
        ifirst_level = (ilevel[d], level[nlev - 1 - d])
        last_level = (level[nlev - 1 - d], ilevel[d])
        ilast_level = (ilevel[nlev - 1 - d], level[d])
        inner = [[[0] * sz0, [0] * sz0], [[0] * sz1, [0] * sz1]]   # [net][perm, inverse]
        marked = [[False] * sz, [False] * sz]
        counter = [0, 0]
        dir_, e = 0, 0
        if sz0 == sz1:
            node, stop_node, stop_side = 0, sz0, 0
        elif sz0 > sz1:
            node, stop_node, stop_side = sz0 - 1, sz0 - 1, 1
        else:
            node, stop_node, stop_side = sz - 1, sz - 1, 1
        while True:
            marked[dir_][node] = True
            v = xperm[dir_][node]
            net = int(node >= sz0) ^ abs(e)                  # 0: upper inner network, 1: lower
            node1 = node - sz0 * int(node >= sz0)
            node3 = xiperm[1 - dir_][v]                      # the node of the other side
            node2 = node3 - sz0 * int(node3 >= sz0)
            t = node3 - (node2 + net * sz0)
            e2 = int(t / sz0)                                # (C division: t is 0 or +-sz0)
            first_level[dir_][delta_j + node] = e
            ifirst_level[dir_][delta_j + net * sz0 + node1] = -e
            last_level[dir_][delta_j + net * sz0 + node2] = e2
            ilast_level[dir_][delta_j + node3] = -e2
            inner[net][dir_][node2] = node1
            inner[net][1 - dir_][node1] = node2
            dir_ = 1 - dir_
            marked[dir_][node3] = True
            if node3 == stop_node and dir_ == stop_side:
                while counter[dir_] < sz and marked[dir_][counter[dir_]]:
                    counter[dir_] += 1
                if counter[dir_] >= sz:
                    break
                node, e = counter[dir_], 0
                stop_node = node + sz0 if node < sz0 else node - sz0
                stop_side = dir_
            else:
                node = node3 + sz0 if node3 < sz0 else node3 - sz0
                e = e2
        self._init(d + 1, delta_j, inner[0][0], inner[0][1], ilevel)
        self._init(d + 1, delta_j + sz0, inner[1][0], inner[1][1], ilevel)

    def testNetwork(self, perm):
        for j in range(self.n):
            j1 = j
            for i in range(self.getNumLevels()):
                j1 += self.shamt(i) * self.level[i][j1]
            if perm[j1] != j:
                return False
        return True


def _collapseBenesLevels(net, startLvl, numLvls):
    """-> (shift amounts of the levels startLvl .. startLvl + numLvls - 1 taken together, whether they are all zero)"""
    n = net.getSize()
    out = np.zeros(n, dtype=np.int64)
    for i in range(n):
        i2 = i
        for lvl in range(startLvl, startLvl + numLvls):
            i2 += net.shamt(lvl) * net.level[lvl][i2]
        out[i] = i2 - i
    return out, not out.any()


# ---------------------------------------------------------------------------------------------
# column permutations
# ---------------------------------------------------------------------------------------------
class ColPerm(HyperCube):
    """a permutation of the columns along one dimension: data[k] is the coordinate along `dim` that the element at k
    comes from (out[k] = in[addCoord(k, dim, data[k] - coordinate(k))])"""

    def __init__(self, sig, data=None, dim=-1):
        super().__init__(sig, data)
        self.dim = dim

    def getPermDim(self):
        return self.dim

    def setPermDim(self, d):
        if not 0 <= d < self.sig.getNumDims():
            raise _invalid("ColPerm: bad dimension")
        self.dim = d

    def makeExplicit(self):
        sig, dim = self.sig, self.dim
        return np.array([sig.addCoord(k, dim, int(self.data[k]) - sig.getCoord(k, dim)) for k in range(sig.getSize())],
                        dtype=np.int64)

    def getShiftAmounts(self):
        """-> (out, nonZero): out[j] is how far the element at j moves along the dimension (src/permutations.cpp:126-141)"""
        sig, dim = self.sig, self.dim
        out = np.zeros(sig.getSize(), dtype=np.int64)
        nonZero = 0
        for k in range(sig.getSize()):
            i, pi_i = sig.getCoord(k, dim), int(self.data[k])
            if i != pi_i:
                nonZero = 1
            out[sig.addCoord(k, dim, pi_i - i)] = i - pi_i
        return out, nonZero

    def getBenesShiftAmounts(self, benesLvls):
        """-> (out, isID): out[i][j] the shift of item j in the i-th collapsed layer, isID[i] whether that layer moves
        nothing (src/permutations.cpp:170-226): a Benes network per column, its levels collapsed as benesLvls says"""
        sig, dim = self.sig, self.dim
        n, m = sig.getDim(dim), sig.getProd(dim + 1)
        nl = len(benesLvls)
        out = [np.zeros(sig.getSize(), dtype=np.int64) for _ in range(nl)]
        isID = [True] * nl
        step = sig.sliceSize(dim)
        for s in range(sig.numSlices(dim)):
            base = s * step
            for col in range(m):
                at = base + col + m * np.arange(n)
                net = GeneralBenesNetwork(self.data[at])
                if net.getNumLevels() != sum(benesLvls):
                    raise LogicError("Sum of benesLvls entries is different to number of levels")
                lvl = 0
                for k in range(nl):
                    shifts, ident = _collapseBenesLevels(net, lvl, benesLvls[k])
                    isID[k] = isID[k] and ident
                    out[k][at] = shifts
                    lvl += benesLvls[k]
        return out, isID


def _perfectMatching(adj, n):
    """a perfect matching of the bipartite multigraph adj[u] = {v: [labels]} on n + n nodes, every node of the same
    positive degree: matchL[u] = v.  Augmenting paths by breadth-first search."""
    matchL, matchR = [-1] * n, [-1] * n
    for s in range(n):
        via, queue, found, qi = {}, [s], -1, 0
        while qi < len(queue) and found < 0:
            u = queue[qi]
            qi += 1
            for v in adj[u]:
                if v in via:
                    continue
                via[v] = u
                if matchR[v] < 0:
                    found = v
                    break
                queue.append(matchR[v])
        if found < 0:
            raise LogicError("breakPermTo3: the bipartite graph is not regular")
        v = found
        while v >= 0:
            u = via[v]
            matchL[u], matchR[v], v = v, u, matchL[u]
    return matchL


def breakPermTo3(pi, dim, rho1, rho2, rho3):
    """src/permutations.cpp:233-327: pi permutes each subcube of the dimensions dim..; rho1 and rho3 permute along dim
    alone, rho2 each subcube of the dimensions dim + 1...  Per subcube, the n edges i2 -> j2 (i = (i1, i2) goes to
    pi(i) = (j1, j2)) of an n1-regular bipartite graph are split into n1 perfect matchings; the matching c of the edge
    labelled i is the row it travels through."""
    sig = pi.getSig()
    n1, n2 = sig.getDim(dim), sig.getProd(dim + 1)
    n = n1 * n2
    for s in range(pi.numSlices(dim)):
        ps, r1, r2, r3 = pi.slice(s, dim), rho1.slice(s, dim), rho2.slice(s, dim), rho3.slice(s, dim)
        adj = [{} for _ in range(n2)]
        for i in range(n):
            adj[i % n2].setdefault(int(ps[i]) % n2, []).append(i)
        for c in range(n1):
            matchL = _perfectMatching(adj, n2)
            for i2, j2 in enumerate(matchL):
                labels = adj[i2][j2]
                i = labels.pop(0)                            # parallel edges in the order of their labels
                if not labels:
                    del adj[i2][j2]
                j1 = int(ps[i]) // n2
                r3[i] = c
                r2[c * n2 + i2] = j2
                r1[c * n2 + j2] = j1
    rho1.setPermDim(dim)
    rho3.setPermDim(dim)


def breakPermByDim(pi, sig):
    """pi over the cube sig as 2 m - 1 column permutations, out[i] and out[2 (m - 1) - i] along dimension i
    (src/permutations.cpp:334-369): applying them in order to a vector gives applyPermToVec(v, pi)"""
    pi = Permut(pi)
    if sig.getSize() != len(pi):
        raise LogicError("Signature sig size is different to pi.length")
    m = sig.getNumDims()
    out = [ColPerm(sig) for _ in range(2 * m - 1)]
    tp1, tp2 = HyperCube(sig, pi), HyperCube(sig)
    if m == 1:
        out[0].data[:] = pi
        out[0].setPermDim(0)
        return out
    for i in range(m - 2):
        breakPermTo3(tp1, i, out[i], tp2, out[2 * m - i - 2])
        tp1, tp2 = tp2, tp1
    breakPermTo3(tp1, m - 2, out[m - 2], out[m - 1], out[m])
    out[m - 1].setPermDim(m - 1)
    return out


# ---------------------------------------------------------------------------------------------
# generator trees
# ---------------------------------------------------------------------------------------------
class GenDescriptor:
    def __init__(self, order, good, genIdx=0):
        self.order, self.good, self.genIdx = int(order), bool(good), int(genIdx)


class SubDimension:
    def __init__(self, size=0, good=False, e=1, frstBenes=(), scndBenes=()):
        self.size, self.good, self.e = int(size), bool(good), int(e)
        self.frstBenes, self.scndBenes = list(frstBenes), list(scndBenes)

    def __repr__(self):
        return "(%s %d %d)%s%s" % ("g" if self.good else "b", self.size, self.e, self.frstBenes, self.scndBenes)


class _TreeNode:
    def __init__(self, data):
        self.data = data
        self.parent = self.leftChild = self.rightChild = self.prev = self.next = -1

    def getData(self):
        return self.data


class OneGeneratorTree:
    """a full binary tree of SubDimension nodes held in a list, the leaves chained from left to right; getAuxKey():
    the generator it belongs to"""

    def __init__(self, auxKey=0):
        self.nodes = [_TreeNode(SubDimension())]
        self.nLeaves, self.frstLeaf, self.lstLeaf, self.aux = 1, 0, 0, auxKey

    def __getitem__(self, i):
        return self.nodes[i]

    def DataOfNode(self, i):
        return self.nodes[i].data

    def putDataInRoot(self, data):
        self.nodes[0].data = data

    def getNleaves(self):
        return self.nLeaves

    def firstLeaf(self):
        return self.frstLeaf

    def nextLeaf(self, i):
        return self.nodes[i].next

    def prevLeaf(self, i):
        return self.nodes[i].prev

    def lastLeaf(self):
        return self.lstLeaf

    def leaves(self):
        i = self.frstLeaf
        while i >= 0:
            yield self.nodes[i].data
            i = self.nodes[i].next

    def rootIdx(self):
        return 0

    def leftChildIdx(self, i):
        return self.nodes[i].leftChild

    def rightChildIdx(self, i):
        return self.nodes[i].rightChild

    def getAuxKey(self):
        return self.aux

    def setAuxKey(self, k):
        self.aux = k

    def addChildren(self, prntIdx, leftData, rightData):
        """the leaf prntIdx becomes the parent of two leaves, which take its place in the chain"""
        parent = self.nodes[prntIdx]
        if parent.leftChild != -1 or parent.rightChild != -1:
            raise LogicError("OneGeneratorTree.addChildren: not a leaf")
        c = len(self.nodes)
        left, right = _TreeNode(leftData), _TreeNode(rightData)
        self.nodes += [left, right]
        parent.leftChild, parent.rightChild = c, c + 1
        left.parent = right.parent = prntIdx
        left.prev, left.next, right.prev, right.next = parent.prev, c + 1, c, parent.next
        if parent.prev >= 0:
            self.nodes[parent.prev].next = c
            parent.prev = -1
        else:
            self.frstLeaf = c
        if parent.next >= 0:
            self.nodes[parent.next].prev = c + 1
            parent.next = -1
        else:
            self.lstLeaf = c + 1
        self.nLeaves += 1
        return c


@functools.lru_cache(maxsize=None)
def _benesCostTable(n, good):
    """tab[i][j]: the number of distinct nonzero shift amounts of the layer made of levels i .. i + j of the width-n
    network (src/OptimizePermutations.cpp:127-163); for a good dimension amounts are counted modulo n"""
    k = GeneralBenesNetwork.depth(n)
    nlev = 2 * k - 1
    tab = []
    for i in range(nlev):
        x, row = {0}, []
        for j in range(nlev - i):
            s = GeneralBenesNetwork._shamt(n, k, i + j)
            x |= {v + d for v in x for d in (s, -s) if -n < v + d < n}
            row.append((len({v % n for v in x}) if good else len(x)) - 1)
        tab.append(row)
    return tab


@functools.lru_cache(maxsize=None)
def optimalBenes(n, budget, good):
    """-> (cost, [s_1 .. s_k]), k <= budget: collapse the first s_1 levels, the next s_2, ... so that the total number
    of shifts is least (src/OptimizePermutations.cpp:286-379; ties go to the first choice found, as there)"""
    k = GeneralBenesNetwork.depth(n)
    nlev = 2 * k - 1
    tab = _benesCostTable(n, good)
    memo = {}

    def aux(i, b):
        if not 0 <= i <= nlev:
            raise _invalid("Level to collapse index out of bound")
        if b <= 0:
            raise _invalid("No budget left")
        hit = memo.get((i, b))
        if hit is not None:
            return hit
        if i == nlev:
            r = (0, ())
        elif b == 1:
            r = (tab[i][nlev - i - 1], (nlev - i,))
        else:
            best, bestJ, bestT = NTL_MAX_LONG, 0, (0, ())
            for j in range(nlev - i):
                t = aux(i + j + 1, b - 1)
                if t[0] + tab[i][j] < best:
                    best, bestJ, bestT = t[0] + tab[i][j], j, t
            r = (best, (bestJ + 1,) + bestT[1])
        memo[(i, b)] = r
        return r
    cost, sol = aux(0, budget)
    return cost, list(sol)


class _SplitNode:
    def __init__(self, order, mid, good, solution1=None, solution2=None, left=None, right=None):
        self.order, self.mid, self.good = order, mid, good
        self.solution1, self.solution2, self.left, self.right = solution1, solution2, left, right

    def isLeaf(self):
        return self.left is None and self.right is None


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def _optimalLower(order, good, budget, mid, memo):
    """one generator's tree (src/OptimizePermutations.cpp:625-736): a leaf with one Benes network (the middle) or two,
    or any split order = order1 * order2 with the budget, the middle token and the good flag shared out"""
    if order <= 1:
        raise _invalid("Order must be greater than 1")
    if budget <= 0:
        raise _invalid("No budget left")
    key = (order, good, budget, mid)
    hit = memo.get(key)
    if hit is not None:
        return hit
    if mid == 0 and budget == 1:
        r = (NTL_MAX_LONG, None)
    else:
        if mid == 1:
            cost, s1 = optimalBenes(order, budget, good)
            s2 = []
        else:
            cost1, s1 = optimalBenes(order, budget // 2, good)
            if budget % 2 == 0:
                cost2, s2 = cost1, s1
            else:
                cost2, s2 = optimalBenes(order, budget - budget // 2, good)
            cost = cost1 + cost2
        solution = _SplitNode(order, mid, good, s1, s2)
        for order1 in range(2, order):
            if order % order1:
                continue
            good1 = good2 = good
            if good and _gcd(order1, order // order1) != 1:
                good2 = False
            for budget1 in range(1, budget):
                for mid1 in range(mid + 1):
                    a = _optimalLower(order1, good1, budget1, mid1, memo)
                    b = _optimalLower(order // order1, good2, budget - budget1, mid - mid1, memo)
                    if a[0] != NTL_MAX_LONG and b[0] != NTL_MAX_LONG and a[0] + b[0] < cost:
                        cost = a[0] + b[0]
                        solution = _SplitNode(order, mid, good, left=a[1], right=b[1])
        r = (cost, solution)
    memo[key] = r
    return r


def _optimalUpperAux(vec, i, budget, mid, upper, lower):
    """the budget and the middle token shared out between the generators i.. (src/OptimizePermutations.cpp:741-821)
    -> (cost, [one _SplitNode per generator]) or (NTL_MAX_LONG, None)"""
    key = (i, budget, mid)
    hit = upper.get(key)
    if hit is not None:
        return hit
    if i == len(vec):
        r = (0, [])
    elif budget == 0:
        r = (NTL_MAX_LONG, None)
    else:
        best, bestS, bestT = NTL_MAX_LONG, None, None
        for budget1 in range(1, budget + 1):
            for mid1 in range(mid + 1):
                s = _optimalLower(vec[i].order, vec[i].good, budget1, mid1, lower)
                t = _optimalUpperAux(vec, i + 1, budget - budget1, mid - mid1, upper, lower)
                if s[0] != NTL_MAX_LONG and t[0] != NTL_MAX_LONG and s[0] + t[0] < best:
                    best, bestS, bestT = s[0] + t[0], s, t
        r = (best, None if best == NTL_MAX_LONG else [bestS[1]] + bestT[1])
    upper[key] = r
    return r


def _CRTcoeff(p, q):
    """0 mod p, 1 mod q"""
    return p * pow(p, -1, q)


def _copy2Tree(tree, idx, sol):
    """-> the number of layers of the (sub)network (src/OptimizePermutations.cpp:865-890)"""
    if sol.isLeaf():
        data = tree[idx].data
        data.frstBenes, data.scndBenes = list(sol.solution1), list(sol.solution2)
        return len(data.frstBenes) + len(data.scndBenes)
    # the child with the middle token goes last (to the right)
    left, right = (sol.right, sol.left) if sol.left.mid else (sol.left, sol.right)
    tree.addChildren(idx, SubDimension(left.order, left.good), SubDimension(right.order, right.good))
    return _copy2Tree(tree, tree.leftChildIdx(idx), left) + _copy2Tree(tree, tree.rightChildIdx(idx), right)


def _computeEvalues(tree, idx, genOrd):
    """the exponent e of every node: its sub-dimension is generated by g^e (src/OptimizePermutations.cpp:893-929)"""
    left, right = tree[idx].leftChild, tree[idx].rightChild
    if left < 0 or right < 0:
        return
    lData, rData = tree[left].data, tree[right].data
    sz1, sz2, ee = lData.size, rData.size, tree[idx].data.e
    if not rData.good:
        rData.e, lData.e = ee, ee * sz2
    elif not lData.good:
        lData.e, rData.e = ee, ee * sz1
    else:
        f1 = _CRTcoeff(sz1, sz2)
        f2 = sz1 * sz2 + 1 - f1
        lData.e, rData.e = ee * f2 % genOrd, ee * f1 % genOrd
    _computeEvalues(tree, left, genOrd)
    _computeEvalues(tree, right, genOrd)


def _copyToGenTree(sol, genIdx):
    tree = OneGeneratorTree(genIdx)
    tree.putDataInRoot(SubDimension(sol.order, sol.good, 1))
    n = _copy2Tree(tree, 0, sol)
    _computeEvalues(tree, 0, sol.order)
    return tree, n


def _oneGenMapping(T):
    """linear array <-> the leaves' cube of one generator (src/permutations.cpp:424-453)"""
    leaves = list(T.leaves())
    dims, coefs = [d.size for d in leaves], [d.e for d in leaves]
    sz = T[0].data.size
    rep = [0] * len(dims)
    genMap = [0] * sz
    for i in range(1, sz):
        for j in range(len(rep) - 1, -1, -1):                # rep += 1 in base dims, the last digit first
            rep[j] += 1
            if rep[j] >= dims[j]:
                rep[j] -= dims[j]
            else:
                break
        genMap[i] = sum(r * c % sz for r, c in zip(rep, coefs)) % sz
    return genMap


class GeneratorTrees:
    def __init__(self):
        self.trees, self.depth = [], 0
        self.map2cube = self.map2array = np.zeros(0, dtype=np.int64)

    def __getitem__(self, i):
        return self.trees[i]

    def numTrees(self):
        return len(self.trees)

    def numLayers(self):
        return self.depth

    def getSize(self):
        return len(self.map2cube)

    def mapToCube(self, i=None):
        return self.map2cube if i is None else int(self.map2cube[i])

    def mapToArray(self, i=None):
        return self.map2array if i is None else int(self.map2array[i])

    def getCubeDims(self):
        """one dimension per tree, at the position of its generator"""
        dims = [0] * len(self.trees)
        for T in self.trees:
            dims[T.getAuxKey()] = T.DataOfNode(T.rootIdx()).size
        return dims

    def getCubeSubDims(self):
        """one dimension per leaf, tree after tree"""
        return [d.size for T in self.trees for d in T.leaves()]

    def ComputeCubeMapping(self):
        trees = self.trees
        if not trees:
            raise LogicError("Trees length is less than 1")
        if len(trees) == 1:
            m2a = _oneGenMapping(trees[0])
        else:
            maps = [_oneGenMapping(T) for T in trees]
            sig1 = CubeSignature([T[0].data.size for T in trees])
            sig2 = CubeSignature(self.getCubeDims())
            m2a = []
            for i in range(sig1.getSize()):
                t = 0
                for j1, T in enumerate(trees):
                    t += maps[j1][sig1.getCoord(i, j1)] * sig2.getProd(T.getAuxKey() + 1)
                m2a.append(t)
        self.map2array = np.array(m2a, dtype=np.int64)
        self.map2cube = np.empty_like(self.map2array)
        self.map2cube[self.map2array] = np.arange(len(m2a))

    def buildOptimalTrees(self, gens, depthBound):
        """-> the cost (the number of rotations at most), or None when no network fits depthBound
        (src/OptimizePermutations.cpp:943-1015, where that is NTL_MAX_LONG)"""
        gens = list(gens)
        self.trees, self.depth = [], 0
        if not gens:
            self.map2cube = self.map2array = np.zeros(1, dtype=np.int64)
            return 0
        if depthBound <= 0:
            raise _invalid("Zero or negative depthBound")
        cost, sol = _optimalUpperAux(gens, 0, int(depthBound), 1, {}, {})
        mid = None
        if sol is not None:
            for i, s in enumerate(sol):
                if s.mid:                                    # the middle tree goes last
                    mid = i
                    continue
                tree, n = _copyToGenTree(s, gens[i].genIdx)
                self.trees.append(tree)
                self.depth += n
        if mid is None:
            self.trees, self.depth = [], 0
            self.map2cube = self.map2array = np.zeros(0, dtype=np.int64)
            return None
        tree, n = _copyToGenTree(sol[mid], gens[mid].genIdx)
        self.trees.append(tree)
        self.depth += n
        self.ComputeCubeMapping()
        return cost


# ---------------------------------------------------------------------------------------------
# permutation networks
# ---------------------------------------------------------------------------------------------
class PermNetLayer:
    """slot j moves e * shifts[j] positions along the dimension of generator genIdx"""

    def __init__(self):
        self.genIdx, self.e, self.isID, self.shifts = 0, 1, True, np.zeros(0, dtype=np.int64)

    def getGenIdx(self):
        return self.genIdx

    def getE(self):
        return self.e

    def getShifts(self):
        return self.shifts

    def amounts(self):
        """[(shift amount, 0/1 mask of the slots that take it)] in makeMask's order (src/PermNetwork.cpp:196-256): zero
        first, then each time the amount of the first slot not served yet; an amount nobody takes is left out"""
        unused = self.shifts.copy()
        out, shamt = [], 0
        while True:
            mask = unused == shamt
            unused[mask] = 0
            if mask.any():
                out.append((int(shamt), mask.astype(np.int64)))
            nz = np.flatnonzero(unused)
            if not nz.size:
                return out
            shamt = unused[nz[0]]


class PermNetwork:
    fuseMaskFan = True     # fused=None: hx_mask_fan, the faster form in all ten alternated pairs measured

    def __init__(self, pi=None, trees=None):
        self.layers = []
        if pi is not None:
            self.buildNetwork(pi, trees)

    def depth(self):
        return len(self.layers)

    def getLayer(self, i):
        return self.layers[i]

    def setLayers4Leaf(self, lyrIdx, p, benesLvls, gIdx, leafData, map2cube):
        """the layers of one Benes network of one leaf (src/PermNetwork.cpp:32-74)"""
        if len(benesLvls) == 1:                              # a one-layer network: the shifts themselves
            s, nonZero = p.getShiftAmounts()
            shifts, isID = [s], [not nonZero]
        else:
            shifts, isID = p.getBenesShiftAmounts(benesLvls)
        for i in range(len(benesLvls)):
            lyr = self.layers[lyrIdx + i]
            lyr.genIdx, lyr.isID, lyr.e = gIdx, isID[i], leafData.e
            if not lyr.isID:
                s = shifts[i]
                if leafData.good:                            # a shift by -x is one by size - x
                    s = np.where(s < 0, s + leafData.size, s)
                lyr.shifts = applyPermToVec(s, map2cube)     # from the leaves' cube to the slots
            else:
                lyr.shifts = np.zeros(len(map2cube), dtype=np.int64)

    def buildNetwork(self, pi, trees):
        """src/PermNetwork.cpp:77-146"""
        pi = Permut(pi)
        if trees.numTrees() == 0:
            self.layers = []
            return
        if len(pi) != trees.getSize():
            raise LogicError("pi wrong size")
        rho = applyPermsToVec(trees.mapToCube(), pi, trees.mapToArray())
        perms = breakPermByDim(rho, CubeSignature(trees.getCubeSubDims()))
        self.layers = [PermNetLayer() for _ in range(trees.numLayers())]
        dimIdx, frntLyr, backLyr = 0, 0, len(self.layers)
        for T in trees.trees:
            for leafData in T.leaves():
                self.setLayers4Leaf(frntLyr, perms[dimIdx], leafData.frstBenes, T.getAuxKey(), leafData, trees.mapToCube())
                frntLyr += len(leafData.frstBenes)
                dimIdx += 1
                if leafData.scndBenes:
                    backLyr -= len(leafData.scndBenes)
                    self.setLayers4Leaf(backLyr, perms[len(perms) - dimIdx], leafData.scndBenes, T.getAuxKey(), leafData,
                                        trees.mapToCube())

    def applyToCube(self, cube):
        """src/PermNetwork.cpp:149-183, on a HyperCube over trees.getCubeDims()"""
        n = cube.getSize()
        for lyr in self.layers:
            if lyr.isID:
                continue
            if len(lyr.shifts) != n:
                raise LogicError("layer has incorrect size")
            tmp = cube.data.copy()
            for j in range(n):
                tmp[cube.addCoord(j, lyr.genIdx, lyr.e * int(lyr.shifts[j]))] = cube.data[j]
            cube.data[:] = tmp
        return cube

    def applyToPtxt(self, p, ea):
        raise LogicError("PermNetwork::applyToPtxt is not implemented")

    def applyToCtxt(self, ct, ea, fused=None):
        """src/PermNetwork.cpp:217-259.  fused (None: PermNetwork.fuseMaskFan): the K masked copies of a layer from one
        ops.maskFan per pair of parts, each copy then given multByConstant(mask, size)'s lnNoise + ln(size); words and
        bookkeeping are the unfused form's.  fused=True on a backend without maskFan, or on an array class whose masks
        are not _encodedMask's (CKKS), raises LogicError."""
        bgv = hasattr(ea, "_encodedMask")
        has = hasattr(ct.ops, "maskFan")
        if fused and not has:
            raise LogicError("PermNetwork: fused=True, but this backend has no maskFan")
        if fused and not bgv:
            raise LogicError("PermNetwork: fused=True, but this array class has no fused mask stage")
        fuse = bool(self.fuseMaskFan if fused is None else fused) and has and bgv
        z, m = ea.zMStar, ea.zMStar.m
        for lyr in self.layers:
            if lyr.isID or not ct.parts:
                continue
            g2e = pow(z.gens[lyr.genIdx], lyr.e, m)
            amounts = lyr.amounts()
            ct._materializeTensor()
            if fuse:
                enc = [ea._encodedMask(mask, ct.primeSet) for _, mask in amounts]
                tmps = [ct.clone() for _ in amounts]         # lazy copies: maskFan's outputs let go of ct's rows
                hs = list(ct.parts)
                for a in range(0, len(hs), 2):
                    h0, h1 = hs[a], hs[a + 1] if a + 1 < len(hs) else None
                    ct.ops.maskFan([t.parts[h0] for t in tmps], [t.parts[h1] for t in tmps] if h1 is not None else None,
                                   ct.parts[h0], ct.parts[h1] if h1 is not None else None, [d for d, _ in enc])
                for t, (_, size) in zip(tmps, enc):
                    t.lnNoise = t.lnNoise + hc._ln(size)     # tmp.multByConstant(mask, size)
            else:
                tmps = []
                for _, mask in amounts:
                    tmp = ct.clone()
                    if bgv:
                        ea._multByMask(tmp, mask)
                    else:
                        ea.multByConstant(tmp, ea.encodePtxt(mask.astype(np.complex128)))
                    tmps.append(tmp)
            total = None
            for (shamt, _), tmp in zip(amounts, tmps):
                if shamt != 0:
                    tmp.smartAutomorph(pow(g2e, shamt, m))
                if total is None:
                    total = tmp
                else:
                    total += tmp
            ct.assign(total)
        return ct


def _dimensions(ea):
    """[(order, native)] of the array's dimensions; ckks.EncryptedArrayCx is one native dimension of size()"""
    if hasattr(ea, "sizeOfDimension"):
        return [(ea.sizeOfDimension(i), ea.nativeDimension(i)) for i in range(ea.dimension())]
    return [(ea.size(), True)]


class PermIndepPrecomp:
    """what does not depend on the permutation: the generator trees of the array's dimensions under depthBound"""

    def __init__(self, ea, depthBound):
        self.ea = ea
        self.trees = GeneratorTrees()
        gens = [GenDescriptor(order, good, i) for i, (order, good) in enumerate(_dimensions(ea))]
        self.cost = self.trees.buildOptimalTrees(gens, depthBound)

    def getCost(self):
        if self.cost is None:
            raise LogicError("buildOptimalTrees failed")
        return self.cost

    def getDepth(self):
        return self.trees.numLayers()


class PermPrecomp:
    def __init__(self, pip, pi):
        self.ea, self.pi = pip.ea, Permut(pi)
        if len(self.pi) != self.ea.size():
            raise LogicError("pi wrong size")
        if pip.cost is None:
            raise LogicError("buildOptimalTrees failed")
        self.net = PermNetwork(self.pi, pip.trees)

    def apply(self, x, fused=None):
        """a ciphertext: the network, in place; a plain slot array [B, nslots] or [B, nslots, d]: out[:, i] = x[:, pi[i]]"""
        if hasattr(x, "parts"):
            return self.net.applyToCtxt(x, self.ea, fused)
        x = np.asarray(x)
        if x.ndim < 2 or x.shape[1] != len(self.pi):
            raise _invalid("PermPrecomp.apply: a slot array [B, nslots] or [B, nslots, d]")
        return x[:, self.pi]
