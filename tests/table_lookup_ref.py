"""TEST INFRASTRUCTURE for tests/test_table_lookup_host.py and tests/test_table_lookup_gpu.py: src/tableLookup.cpp and
hx_table_tensor_sum restated in python integers and floats, sharing nothing with helib_amd.table_lookup."""
import math

import numpy as np

# recursiveProducts' split (src/tableLookup.cpp:243-247), derived by hand: n1 = the largest power of two below nBits,
# (k, l) = (2^n1, 2^(nBits - n1)).  nBits = 1 and 2 never reach the split (the edge cases); the formula gives them too.
#   nBits  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16
#   n1     0  1  2  2  4  4  4  4  8  8  8  8  8  8  8  8
SPLIT = {1: (1, 2), 2: (2, 2), 3: (4, 2), 4: (4, 4), 5: (16, 2), 6: (16, 4), 7: (16, 8), 8: (16, 16), 9: (256, 2),
         10: (256, 4), 11: (256, 8), 12: (256, 16), 13: (256, 32), 14: (256, 64), 15: (256, 128), 16: (256, 256)}


def counts(nBits):
    """(multiplyBy calls of computeAllProducts for 2^nBits outputs, of which in the last level)"""
    if nBits <= 1:
        return 0, 0
    if nBits == 2:
        return 1, 1
    k, l = SPLIT[nBits]
    return counts(k.bit_length() - 1)[0] + counts(l.bit_length() - 1)[0] + k * l, k * l


def table_values(f, nbits_in, scale_in, sign_in, nbits_out, scale_out, sign_out):
    """buildLookupTable's integers (src/tableLookup.cpp:155-194) by direct evaluation: f is given a float and returns one
    (infinities and NaN included)"""
    out = []
    hi = 2 ** (nbits_out - 1) - 1 if sign_out else 2 ** nbits_out - 1
    lo = -2 ** (nbits_out - 1) if sign_out else 0
    for i in range(2 ** nbits_in):
        x = i - 2 ** nbits_in if sign_in and i >= 2 ** (nbits_in - 1) else i
        y = f(x * 2.0 ** scale_in) * 2.0 ** -scale_out
        if y != y:
            v = 0
        elif y == math.inf or y == -math.inf:
            v = hi if y > 0 else lo
        else:
            r = int(abs(y) + 0.5)                        # round(): half away from zero
            r = r if y >= 0 else -r
            v = min(max(r, lo), hi)
        out.append(v % 2 ** nbits_out)
    return out


def logaddexp(a, b):
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    hi, lo = max(a, b), min(a, b)
    return hi + math.log1p(math.exp(lo - hi))


def lazy_bookkeeping(lnA, lnB, magA, sizes, k, N):
    """lnNoise and ptxtMag of sum_{ii < N} T[ii] tensor(A[ii mod k], B[ii div k]) before its relinearisation, as the
    reference's own steps would leave them: per pair Ctxt::tensorProduct (noise = the product of the two bounds, BGV
    leaves ptxtMag alone), multByConstant (times the constant's size), then operator+= in index order (the sum of the
    bounds, the sum of ptxtMag)."""
    ln, mag = None, None
    for ii in range(N):
        i, j = ii % k, ii // k
        pair = lnA[i] + lnB[j] + (math.log(sizes[ii]) if sizes[ii] > 0 else -math.inf)
        if ln is None:
            ln, mag = pair, magA[i]
        else:
            ln, mag = logaddexp(ln, pair), mag + magA[i]
    return ln, mag


def table_tensor_sum(a0, a1, b0, b1, table, size, qs):
    """hx_table_tensor_sum in python integers.  a0, a1: k arrays [rows, B, N] (dtype object); b0, b1: l of them; table:
    [rows, size, N] on the outputs' primes; qs: [rows] -> three arrays [rows, B, N] of residues"""
    k, l = len(a0), len(b0)
    qcol = [[[q]] for q in qs]
    o = [0, 0, 0]
    for j in range(l):
        u0 = u1 = 0
        for i in range(k):
            e = j * k + i
            if e >= size:
                break
            t = table[:, e:e + 1, :]
            u0 = u0 + t * a0[i]
            u1 = u1 + t * a1[i]
        o[0] = o[0] + u0 * b0[j]
        o[1] = o[1] + u0 * b1[j] + u1 * b0[j]
        o[2] = o[2] + u1 * b1[j]
    qa = np.array(qcol, dtype=object)
    return [x % qa for x in o]
