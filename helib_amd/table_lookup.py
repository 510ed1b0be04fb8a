"""Table lookup on encrypted indices (src/tableLookup.cpp) over helib_amd.ctxt.Ctxt, with the conventions of
helib_amd.binary_arith: an index is a python list, lowest bit first, of Ctxt or None; inputs are left as they were; every
slot of every batch element is one independent lookup.

  computeAllProducts(array, size=None)     the 2^n subset products of n encrypted bits (:37-78, :204-270):
                                           products[j] = prod_{j_i = 1} array[i] prod_{j_i = 0} (1 - array[i]), i.e. the
                                           indicator [index == j], step for step as recursiveProducts forms them
  tableLookup(ea, table, idx)              sum_i T[i] products[i] (:83-104).  lazy=True: the last level of
                                           computeAllProducts and the weighted sum under ONE relinearisation,
                                             out = reLinearize(sum T[j k + i] (x) tensor(products1[i], products2[j])),
                                           fused=True: that sum as one hx_table_tensor_sum
  tableWriteIn(table_cts, idx)             table_cts[i] += products[i], in place (:109-129)
  buildLookupTable(ea, f, ...)             T[x] = f(x 2^scale_in) 2^-scale_out, rounded, saturated, packed into the slots
                                           (:139-198) -> LookupTable
  LookupTable / LookupTable.fromSlots      the plaintext table: slots, zzX, sizes, and the encoded table per prime set

Not built: packedRecrypt and the unpackSlotEncoding argument.  Where the reference would recrypt, computeAllProducts
raises what it raises when it cannot: LogicError("not enough levels for table lookup").  Nothing here imports oracle/."""
import math

import numpy as np

from . import binary_arith as ba
from . import capi, intraslot
from . import ctxt as hc
from .ckks import LogicError
from .linalg import _NoData, _like, _shadow

# lazy=None in tableLookup: the one-relinearisation form wherever it applies.  True because it was ahead of the reference's
# form in every alternated pair at index widths 5 and 8, with every output correct and the same capacity left
# (tools/bench_table_lookup.py, profiles/table_lookup.json); set it to False, or pass lazy=False, for the
# reference's one multiplyBy per table entry
lazyLookup = True

MAX_BITS = 16       # "Output cannot be bigger than 2^16" (src/tableLookup.cpp:51)


def _invalid(msg):
    return capi.InvalidArgument(capi.HX_ERR_INVALID, msg)


def NumBits(n):
    """NTL::NumBits of a non-negative integer"""
    return int(n).bit_length()


def splitSizes(nBits):
    """(k, l) of recursiveProducts' split (:243-247): n1 = the largest power of two below nBits, k = 2^n1 products of the
    low n1 bits, l = 2^(nBits - n1) of the rest"""
    n1 = 1 << (NumBits(nBits) - 1)
    if nBits <= n1:
        n1 //= 2
    return 1 << n1, 1 << (nBits - n1)


def _halves(N, array, like):
    """recursiveProducts' split of `array` for N outputs -> (products1, products2, k, l)"""
    nBits = len(array)
    k, l = splitSizes(nBits)
    n1 = k.bit_length() - 1
    return _recursiveProducts(k, array[:n1], like), _recursiveProducts(l, array[n1:nBits], like), k, l


def _effective(N, nBits):
    """recursiveProducts' opening (:206-214): the outputs formed and the bits they need"""
    if N > (1 << nBits):
        N = 1 << nBits
    elif N < (1 << (nBits - 1)):
        nBits = NumBits(N - 1)
    return N, nBits


def _recursiveProducts(N, array, like):
    """recursiveProducts (:204-270) -> the first min(N, 2^len(array)) products, new ciphertexts"""
    nBits = len(array)
    if nBits == 0 or N == 0:
        return []
    N, nBits = _effective(N, nBits)
    array = array[:nBits]
    if N <= 2:                                           # edge condition
        p0 = ba._copy(array[0], like)
        p0.negate()
        p0.addScalar(1)                                  # out[0] = 1 - in
        return [p0] + ([ba._copy(array[0], like)] if N > 1 else [])
    if N <= 4:                                           # a single multiplication instead of 4
        x0, x1 = ba._copy(array[0], like), ba._copy(array[1], like)
        p0 = x1.clone()
        ba._multiplyBy(p0, x0)                           # x1 x0
        p1 = x0.clone()
        p1 -= p0                                         # (1 - x1) x0
        p2 = x1.clone()
        p2 -= p0                                         # x1 (1 - x0)
        out = [p0, p1, p2]
        if N > 3:
            out.append(p0.clone())                       # x1 x0
        p0.addScalar(1)
        p0 -= x1
        p0 -= x0                                         # (1 - x1)(1 - x0)
        return out
    products1, products2, k, _ = _halves(N, array, like)
    out = []
    for ii in range(N):
        j = ii // k
        c = products1[ii - j * k].clone()
        ba._multiplyBy(c, products2[j])
        out.append(c)
    return out


def _prepare(array, size):
    """computeAllProducts up to the recursion (:42-74) -> (nBits, like), nBits = 0: nothing to do"""
    for c in array:
        if c is not None and c.context.ckks:
            raise _invalid("table lookup takes BGV ciphertexts")
    nBits = len(array)
    if size is not None and size > 0:
        nBits = min(nBits, NumBits(size - 1))            # ignore extra bits in 'array'
    if nBits < 1:
        return 0, None
    if nBits > MAX_BITS:
        raise _invalid("Output cannot be bigger than 2^16")
    like = ba.ptr2nonNull(array)
    if like is None:
        raise _invalid("Invalid array (could not find non-null Ctxt)")
    if ba.findMinBitCapacity(array) < (NumBits(nBits) + 1) * ba.BPL_ESTIMATE:    # (the reference recrypts here)
        raise LogicError("not enough levels for table lookup")
    return nBits, like


def computeAllProducts(array, size=None):
    """The subset products of the encrypted bits `array` (:37-78): a list of `size` ciphertexts (default 2^len(array)),
    products[j] encrypting [index == j]; nBits = min(len(array), NumBits(size - 1)) <= 16 bits are used and the entries
    from 2^nBits on stay empty.  Any plaintext space: 1 - x is negate and addConstant(1)."""
    nBits, like = _prepare(array, size)
    if nBits == 0:
        like = ba.ptr2nonNull(array)
        return [like._emptyLike() for _ in range(size or 0)] if like is not None else []
    n = (1 << nBits) if not size else size
    out = _recursiveProducts(n, list(array[:nBits]), like)
    return out + [like._emptyLike() for _ in range(n - len(out))]


# ---- the plaintext table ----
class LookupTable:
    """A plaintext table for tableLookup: slots [size, nslots(, d)], the zzX [size, phi(m)] of every entry, each
    entry's embeddingLargestCoeff (measured once, on the whole batch), the plaintext space, and the encoded table per
    prime set (one batched encode, split into entries)."""

    def __init__(self, ea, slots):
        self.ea = ea
        self.slots = np.ascontiguousarray(ea._slots(slots))
        self.zzX = np.asarray(ea.encodeCoeffs(self.slots))
        self.sizes = [float(x) for x in np.asarray(ea.enc.norm(self.zzX)).reshape(-1)]
        self.ptxtSpace = ea.cc.ptxtSpace
        self._encoded = {}

    @classmethod
    def fromSlots(cls, ea, values):
        """values: integers [size, nslots] or [size, nslots, d], entry i of the table in every slot (they may differ
        from slot to slot)"""
        v = np.asarray(values)
        if v.ndim not in (2, 3):
            raise _invalid("a table of slots is [size, nslots] or [size, nslots, d]")
        return cls(ea, v)

    def __len__(self):
        return len(self.sizes)

    def encoded(self, primes, n=None):
        """-> (the first n entries as ONE DoubleCRT of batch n on `primes`, the same split into n entries)"""
        n = len(self) if n is None else n
        key = (tuple(primes), n)
        hit = self._encoded.get(key)
        if hit is None:
            poly = self.ea.enc.encode(self.slots[:n], 1, list(primes))
            hit = self._encoded[key] = (poly, self.ea.enc.split(poly))
        return hit


def _table(ea, table):
    return table if isinstance(table, LookupTable) else LookupTable.fromSlots(ea, table)


def buildLookupTable(ea, f, nbits_in, scale_in, sign_in, nbits_out, scale_out, sign_out):
    """buildLookupTable (:139-198): for every x of nbits_in bits (two's complement when sign_in),
    T[x] = round(f(x 2^scale_in) 2^-scale_out), saturated to nbits_out bits (two's complement when sign_out), NaN -> 0,
    masked to nbits_out bits and packed into every slot by intraslot.packConstant -> LookupTable of 2^nbits_in entries"""
    if nbits_in > MAX_BITS:
        raise _invalid("tables of size > 2^{16} are not supported")
    values = tableValues(f, nbits_in, scale_in, sign_in, nbits_out, scale_out, sign_out)
    CB = intraslot.normalBasisMatrices(ea)[0]
    polys = np.stack([intraslot._int2Poly(ea, CB, v, nbits_out) for v in values])       # packConstant's slot, [size, d]
    return LookupTable(ea, np.broadcast_to(polys[:, None, :], (len(values), ea.size(), ea.getDegree())))


def tableValues(f, nbits_in, scale_in, sign_in, nbits_out, scale_out, sign_out):
    """the integers buildLookupTable packs (:155-194), one per index.  f is called with a python float; what it raises
    (1 / 0.0 raises in python where C++ gives an infinity) is not caught: use numpy floats for C's division"""
    pow2_in, pow2_out = math.ldexp(1.0, scale_in), math.ldexp(1.0, -scale_out)
    if sign_out:
        largest, smallest = (1 << (nbits_out - 1)) - 1, -(1 << (nbits_out - 1))
    else:
        largest, smallest = (1 << nbits_out) - 1, 0
    out = []
    for i in range(1 << nbits_in):
        x = i - 2 * ((1 << (nbits_in - 1)) & i) if sign_in else i
        y = float(f(float(x) * pow2_in)) * pow2_out
        if math.isnan(y):
            value = 0
        else:
            y = _round(y)
            value = largest if y > largest else smallest if y < smallest else int(y)
        out.append(value & ((1 << nbits_out) - 1))
    return out


def _round(y):
    """C's round(): half away from zero; infinities stay"""
    if math.isinf(y):
        return y
    return math.floor(y + 0.5) if y >= 0 else math.ceil(y - 0.5)


# ---- the lookup ----
def _default(products, tab, n):
    """:97-103 on the first n products: multByConstant of entry i with its embeddingLargestCoeff, then += in order"""
    live = [c for c in products[:n] if c.parts]
    out = products[0]._emptyLike()
    if not live:
        return out
    primes = sorted(frozenset().union(*[c.primeSet for c in live]))
    consts = tab.encoded(primes, n)[1]
    for i in range(n):
        products[i].multByConstant(consts[i], tab.sizes[i])
    for i in range(n):
        out += products[i]
    return out


def tableLookup(ea, table, idx, lazy=None, fused=None):
    """T[index] for the encrypted index `idx` (:83-104) as a new ciphertext.  table: a LookupTable, or integer slots
    [size, nslots] / [size, nslots, d]; entries from 2^len(idx) on are not used.  The default form is the reference's:
    computeAllProducts, multByConstant on every product with size = the entry's embeddingLargestCoeff, += in index
    order; the constants come from one batched encode of the table onto the products' primes.

    lazy=True (lazy=None follows the module flag lazyLookup), when the last level of computeAllProducts is a k x l grid
    of multiplications (3 bits or more): products1 and products2 are formed as recursiveProducts forms them, brought to
    one prime set chosen by multLowLvl's rule on the operand of least capacity of each half, and
    sum T[j k + i] tensor(products1[i], products2[j]) is relinearised ONCE.  lnNoise and ptxtMag are those of the
    pairs' tensor products, multByConstant and += in index order.  The slots decrypt to the same values as the default
    form's; the words are not the reference's.  The sum runs through multByConstant, += and tensorProduct on a backend
    with neither mulAddMany nor tensorSum, else through l mulAddMany and one tensorSum, or with fused=True (fused=None
    follows Ctxt.fuseTableSum) through one tableTensorSum (hx_table_tensor_sum); the three give the same words.
    fused=True on a backend without tableTensorSum raises.  Where the lazy form does not apply (fewer than 3 bits,
    operands that are not canonical, pairs that would not share one ptxtSpace and intFactor) the default form runs."""
    tab = _table(ea, table)
    idx = list(idx)
    like = ba.ptr2nonNull(idx)
    has = like is not None and hasattr(like.ops, "tableTensorSum")
    if fused and not has:
        raise RuntimeError("tableLookup: fused=True, but this backend has no tableTensorSum")
    if len(tab) == 0:
        if like is None:
            raise _invalid("Invalid array (could not find non-null Ctxt)")
        return like._emptyLike()
    nBits, like = _prepare(idx, len(tab))
    if nBits == 0:
        return ba.ptr2nonNull(idx)._emptyLike()
    n = min(len(tab), 1 << nBits)
    if lazyLookup if lazy is None else lazy:
        want = bool((hc.Ctxt.fuseTableSum if fused is None else fused) and has)
        out = _lazy(tab, idx[:nBits], n, like, want)
        if out is not None:
            return out
    return _default(_recursiveProducts(n, idx[:nBits], like), tab, n)


def _lazy(tab, array, N, like, fused):
    """the lazy form, or None where it does not apply (the inputs are as they were)"""
    N, nBits = _effective(N, len(array))
    if nBits < 3 or N <= 4:
        return None
    array = array[:nBits]
    A, Bs, k, l = _halves(N, array, like)
    l = (N + k - 1) // k                                 # the rows of the grid that hold an entry
    Bs = Bs[:l]
    ops = like.ops
    cts = A + Bs
    if any(set(c.parts) != {"1", "s"} for c in cts):
        return None
    g = 0
    for c in cts:
        g = math.gcd(g, c.ptxtSpace)
    if g <= 1:
        return None
    if g > 2 and len({a.intFactor % g * (b.intFactor % g) % g for a in A for b in Bs}) != 1:
        return None
    for c in cts:
        c.ptxtSpace = g
        c.intFactor %= g
    ctx = like.context
    cap = lambda c: c.logOfPrimeSet() - max(c.lnNoise, 0.0)          # noqa: E731
    lo, hi = hc.Ctxt.computeIntervalForMul(min(A, key=cap), min(Bs, key=cap))
    inter = frozenset.intersection(*[c.primeSet for c in cts])
    common = ctx.modSizes.getSet4Size(lo, hi, inter, inter, False)
    common = frozenset(common) if common else frozenset([ctx.ctxtPrimes[0]])
    groups = {}
    for c in cts:                                        # _bringManyToSet takes ciphertexts on one prime set
        groups.setdefault(c.primeSet, []).append(c)
    for group in groups.values():
        hc.Ctxt._bringManyToSet(group, common)
    rows = A[0].parts["1"].getIndexSet()
    if any(c.parts[h].getIndexSet() != rows for c in cts for h in ("1", "s")):
        return None
    a0, a1 = [c.parts["1"] for c in A], [c.parts["s"] for c in A]
    b0, b1 = [c.parts["1"] for c in Bs], [c.parts["s"] for c in Bs]
    poly, consts = tab.encoded(rows, N)
    # the data first: reading lnNoise waits for the mod-switches' norms, and the device works meanwhile
    if fused:
        t = ops.tableTensorSum(a0, a1, b0, b1, poly, N)
    elif hasattr(ops, "mulAddMany") and hasattr(ops, "tensorSum"):
        w0, w1 = [], []
        for j in range(l):
            kj = min(k, N - j * k)
            u0, u1 = ops.likeUninit(a0[0]), ops.likeUninit(a0[0])
            ops.mulAddMany(u0, u1, consts[j * k:j * k + kj], a0[:kj], a1[:kj], accumulate=False)
            w0.append(u0)
            w1.append(u1)
        t = ops.tensorSum(w0, w1, b0, b1)
    else:
        t = None
        for ii in range(N):
            j = ii // k
            i = ii - j * k
            prod = ops.tensorProduct(a0[i], a1[i], b0[j], b1[j])
            for part in prod:
                part *= consts[ii]
            if t is None:
                t = list(prod)
            else:
                for x, y in zip(t, prod):
                    x += y
    # the bookkeeping of the sum on shadows, in index order: _tensorProduct's per pair, multByConstant's, addCtxt's
    acc = _like(A[0], {})
    acc.lnNoise, acc.ptxtMag, acc.intFactor = -math.inf, 1.0, 1
    for ii in range(N):
        j = ii // k
        x, y = A[ii - j * k], Bs[j]
        sh = _shadow(x)
        if sh.ptxtSpace > 2:
            q = ctx.productOfPrimes(sh.primeSet) % sh.ptxtSpace
            sh.intFactor = x.intFactor * y.intFactor % sh.ptxtSpace * q % sh.ptxtSpace
        sh.parts = {"1": _NoData(), "s": _NoData(), "s2": _NoData()}
        sh.lnNoise = x.lnNoise + y.lnNoise
        sh.multByConstant(_NoData(), tab.sizes[ii])
        acc.addCtxt(sh)
    out = _like(acc, {"1": t[0], "s": t[1], "s2": t[2]})
    out.reLinearize()
    return out


def tableWriteIn(table_cts, idx):
    """tableWriteIn (:109-129): table_cts[i] += [index == i], in place on the list's ciphertexts (a None entry is
    replaced by the product)"""
    size = len(table_cts)
    if size == 0:
        return table_cts
    if ba.ptr2nonNull(table_cts) is None:
        raise _invalid("Invalid table (could not find non-null Ctxt)")
    products = computeAllProducts(list(idx), size)
    for i, p in enumerate(products):
        if table_cts[i] is None:
            table_cts[i] = p
        else:
            table_cts[i] += p
    return table_cts
