"""TEST INFRASTRUCTURE shared by tests/test_replicate_host.py and tests/test_hoisted_mask_fan_gpu.py:
hx_hoisted_mask_fan in python integers, word by word, as include/helib_amd.h states it, and the same as an op of the CPU
oracle backend."""
import numpy as np

from tests.thin_ref import perm


def hoisted_mask_fan(m, qs, L, psp, dig, c0, c1, ks, keys, A, B):
    """qs: the primes of the nall output rows, the first L the ciphertext's; psp[r] = the product of the special primes
    modulo qs[r]; dig [ndig, nall, B, N]; c0, c1 [L, B, N]; keys[t] = (b, a), each [ndig, nall, N] on the output rows;
    A[t], B[t]: None (the constant 1) or a mask [nall, 1 or B, N] on the output rows
    -> out0, out1: lists of n uint64 arrays [nall, B, N]"""
    dig = np.asarray(dig).astype(object)
    ndig, nall, nb, N = dig.shape
    outs0, outs1 = [], []
    for t, k in enumerate(ks):
        pm = perm(m, k % m)
        kb, ka = keys[t]
        o0 = np.zeros((nall, nb, N), dtype=object)
        o1 = np.zeros((nall, nb, N), dtype=object)
        for r in range(nall):
            q = qs[r]
            in0 = np.zeros((nb, N), dtype=object)
            in1 = np.zeros((nb, N), dtype=object)
            if r < L:
                in0 = in0 + psp[r] * np.asarray(c0[r]).astype(object)[:, pm]
            for j in range(ndig):
                g = dig[j, r][:, pm]
                in0 = in0 + g * np.asarray(kb[j][r]).astype(object)[None, :]
                in1 = in1 + g * np.asarray(ka[j][r]).astype(object)[None, :]
            bm = 1 if B[t] is None else np.asarray(B[t][r]).astype(object)
            o0[r] = (in0 % q) * bm
            o1[r] = (in1 % q) * bm
            if r < L:
                am = 1 if A[t] is None else np.asarray(A[t][r]).astype(object)
                o0[r] = o0[r] + am * (psp[r] * np.asarray(c0[r]).astype(object) % q)
                o1[r] = o1[r] + am * (psp[r] * np.asarray(c1[r]).astype(object) % q)
            o0[r] %= q
            o1[r] %= q
        outs0.append(o0.astype(np.uint64))
        outs1.append(o1.astype(np.uint64))
    return outs0, outs1


def oracle_hoisted_mask_fan(o, calls=None):
    """-> hoistedMaskFan(self, digits, c0, c1, ks, Ws, A, B, special) over oracle.backend's OPoly / OKeySwitch (batch 1);
    calls, a list, receives (n, ndig) per call"""
    from oracle.backend import OPoly

    def hoistedMaskFan(self, digits, c0, c1, ks, Ws, A, B, special):
        allp = list(c0.idx) + list(special)
        nall, L, n = len(allp), len(c0.idx), len(ks)
        assert c1.idx == c0.idx and len(digits.idx) % nall == 0 and len(Ws) == n
        ndig = len(digits.idx) // nall
        assert digits.idx == allp * ndig
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

        def masks(M):
            if M is None:
                return [None] * n
            assert len(M) == n
            return [None if x is None else np.stack([x.rows[list(x.idx).index(i)] for i in allp])[:, None, :] for x in M]
        if calls is not None:
            calls.append((n, ndig))
        o0, o1 = hoisted_mask_fan(o.m, qs, L, psp, digits.rows.reshape(ndig, nall, 1, -1), c0.rows[:, None, :],
                                  c1.rows[:, None, :], ks, keys, masks(A), masks(B))
        return ([OPoly(o, allp, x[:, 0, :]) for x in o0], [OPoly(o, allp, x[:, 0, :]) for x in o1])
    return hoistedMaskFan
