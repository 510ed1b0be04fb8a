"""TEST INFRASTRUCTURE shared by tests/test_thin_recrypt_host.py, tests/test_hoisted_sum_gpu.py and
tests/test_thin_recrypt_gpu.py: hx_hoisted_automorph_sum in python integers, word by word, as include/helib_amd.h states
it; the same as an op of the CPU oracle backend; and the rings of the thin tests."""
from math import gcd

import numpy as np

# the rings of thinReCrypt's tests: (m, r), from tests/evalmap_tables.RINGS
THIN_RINGS = [(57, 1), (85, 1), (85, 2)]


def perm(m, k):
    """sigma_k on evaluation rows: out[j] = in[perm[j]], perm[j] the position of Z_m^*[j] k mod m in Z_m^*"""
    zms = [i for i in range(1, m) if gcd(i, m) == 1]
    at = {t: i for i, t in enumerate(zms)}
    return np.array([at[t * k % m] for t in zms], dtype=np.int64)


def hoisted_sum(m, qs, L, psp, dig, c0, c1, ks, keys):
    """qs: the primes of the nall output rows, the first L the ciphertext's; psp[r] = the product of the special primes
    modulo qs[r]; dig [ndig, nall, B, N]; c0, c1 [L, B, N]; keys[t] = (b, a), each [ndig, nall, N] on the output rows
    -> out0, out1 uint64 [nall, B, N]"""
    dig = np.asarray(dig).astype(object)
    ndig, nall, B, N = dig.shape
    out = [np.zeros((nall, B, N), dtype=object), np.zeros((nall, B, N), dtype=object)]
    perms = [perm(m, k % m) for k in ks]
    for r in range(nall):
        q = qs[r]
        if r < L:
            x0 = np.asarray(c0[r]).astype(object)
            out[0][r] = psp[r] * (x0 + sum(x0[:, pm] for pm in perms))
            out[1][r] = psp[r] * np.asarray(c1[r]).astype(object)
        for pm, (kb, ka) in zip(perms, keys):
            for j in range(ndig):
                g = dig[j, r][:, pm]
                out[0][r] = out[0][r] + g * np.asarray(kb[j][r]).astype(object)[None, :]
                out[1][r] = out[1][r] + g * np.asarray(ka[j][r]).astype(object)[None, :]
        out[0][r] %= q
        out[1][r] %= q
    return out[0].astype(np.uint64), out[1].astype(np.uint64)


def oracle_hoisted_sum(o, calls=None):
    """-> hoistedSum(self, digits, c0, c1, ks, Ws, special) over oracle.backend's OPoly / OKeySwitch (batch 1); calls, a
    list, receives (n, ndig) per call"""
    from oracle.backend import OPoly

    def hoistedSum(self, digits, c0, c1, ks, Ws, special):
        allp = list(c0.idx) + list(special)
        nall, L = len(allp), len(c0.idx)
        assert c1.idx == c0.idx and len(digits.idx) % nall == 0
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
        if calls is not None:
            calls.append((len(ks), ndig))
        o0, o1 = hoisted_sum(o.m, qs, L, psp, digits.rows.reshape(ndig, nall, 1, -1), c0.rows[:, None, :], c1.rows[:, None, :],
                             ks, keys)
        return OPoly(o, allp, o0[:, 0, :]), OPoly(o, allp, o1[:, 0, :])
    return hoistedSum
