"""TEST INFRASTRUCTURE shared by tests/test_matmul_full_host.py and tests/test_hoisted_blend_gpu.py:
hx_hoisted_blend in python integers, word by word, as include/helib_amd.h states it (each operand's key switch first, the
blend of the two results last), and the same as an op of the CPU oracle backend."""
import numpy as np

from tests.thin_ref import perm


def hoisted_blend(m, qs, L, psp, digA, a0, digB, b0, ks, keys, M):
    """qs: the primes of the nall output rows, the first L the operands'; psp[r] = the product of the special primes
    modulo qs[r]; digA, digB [ndig, nall, B, N]; a0, b0 [L, B, N]; keys[t] = (b, a), each [ndig, nall, N] on the output
    rows; M[t]: a mask [nall, 1 or B, N] on the output rows
    -> out0, out1: lists of n uint64 arrays [nall, B, N]"""
    digA, digB = np.asarray(digA).astype(object), np.asarray(digB).astype(object)
    ndig, nall, nb, N = digA.shape
    assert digB.shape == digA.shape
    outs0, outs1 = [], []
    for t, k in enumerate(ks):
        pm = perm(m, k % m)
        kb, ka = keys[t]
        o0 = np.zeros((nall, nb, N), dtype=object)
        o1 = np.zeros((nall, nb, N), dtype=object)
        for r in range(nall):
            q = qs[r]
            mk = np.asarray(M[t][r]).astype(object)
            xy = []
            for dig, c0 in ((digA, a0), (digB, b0)):
                in0 = np.zeros((nb, N), dtype=object)
                in1 = np.zeros((nb, N), dtype=object)
                if r < L:
                    in0 = in0 + psp[r] * np.asarray(c0[r]).astype(object)[:, pm]
                for j in range(ndig):
                    g = dig[j, r][:, pm]
                    in0 = in0 + g * np.asarray(kb[j][r]).astype(object)[None, :]
                    in1 = in1 + g * np.asarray(ka[j][r]).astype(object)[None, :]
                xy.append((in0 % q, in1 % q))
            (x0, x1), (y0, y1) = xy
            o0[r] = (mk * x0 + y0 - mk * y0) % q
            o1[r] = (mk * x1 + y1 - mk * y1) % q
        outs0.append(o0.astype(np.uint64))
        outs1.append(o1.astype(np.uint64))
    return outs0, outs1


def oracle_hoisted_blend(o, calls=None):
    """-> hoistedBlend(self, digA, a0, a1, digB, b0, b1, ks, Ws, masks, special) over oracle.backend's OPoly / OKeySwitch
    (batch 1); calls, a list, receives (n, ndig) per call"""
    from oracle.backend import OPoly

    def hoistedBlend(self, digA, a0, a1, digB, b0, b1, ks, Ws, masks, special):
        allp = list(a0.idx) + list(special)
        nall, L, n = len(allp), len(a0.idx), len(ks)
        assert a1.idx == a0.idx == b0.idx == b1.idx and len(digA.idx) % nall == 0 and len(Ws) == len(masks) == n
        ndig = len(digA.idx) // nall
        assert digA.idx == allp * ndig == digB.idx
        qs = [o.primes[i] for i in allp]
        psp = []
        for q in qs:
            f = 1
            for i in special:
                f = f * o.primes[i] % q
            psp.append(f)
        keys = []
        for W in Ws:
            sel = [W.row_idx.index(i) for i in allp]
            assert W.b.shape[0] >= ndig
            keys.append((W.b[:ndig][:, sel], W.a[:ndig][:, sel]))
        M = [np.stack([x.rows[list(x.idx).index(i)] for i in allp])[:, None, :] for x in masks]
        if calls is not None:
            calls.append((n, ndig))
        o0, o1 = hoisted_blend(o.m, qs, L, psp, digA.rows.reshape(ndig, nall, 1, -1), a0.rows[:, None, :],
                               digB.rows.reshape(ndig, nall, 1, -1), b0.rows[:, None, :], ks, keys, M)
        return ([OPoly(o, allp, x[:, 0, :]) for x in o0], [OPoly(o, allp, x[:, 0, :]) for x in o1])
    return hoistedBlend
