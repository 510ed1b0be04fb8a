"""BGV slots for d > 1 (helib_amd.bgv_crt) on the ring the project is measured on: m = 21845, p = 2 (d = 16, 1024
slots, both dimensions non-native), bits = 950, batch 64.  Records the table construction time and bytes, the encode
alone, decrypt_batch, and rotate1D along both dimensions (the masked two-automorphism branch), and writes one JSON
object to profiles/bgv_crt.json.  Wall clock around synchronising calls, best of --reps.

  python tools/bench_bgv_crt.py          # MI355X
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=21845)
    ap.add_argument("--p", type=int, default=2)
    ap.add_argument("--bits", type=int, default=950)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgv_crt.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import bgv_crt, capi, ctxt as hc, keys as hk
    m, p, B = a.m, a.p, a.batch
    cc = hc.ChainContext(m, p, 1, bits=a.bits, c=3)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey()
    t0 = time.perf_counter()
    ea = bgv_crt.EncryptedArray(cc, g)
    table_s = time.perf_counter() - t0
    sk.zMStar = ea.zMStar
    z = ea.zMStar
    for i in range(ea.dimension()):       # rotate1D by 1: g^1 and, on a non-native dimension, g^-ord
        for k in {z.genToPow(i, 1)} | (set() if ea.nativeDimension(i) else {z.genToPow(i, -ea.sizeOfDimension(i))}):
            sk.GenKeySWmatrix(1, k)
    sk.setKeySwitchMap()
    idx = list(cc.ctxtPrimes)
    L, N, n = len(idx), cc.phim, ea.size()
    v = np.random.default_rng(1).integers(0, p, size=(B, n))

    def wall(fn, reps):
        fn()   # warm: buffers, the mask cache
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            g.sync()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best

    enc_ms = wall(lambda: ea.encode(v, idx, mul=1), a.reps)
    ct = ea.encrypt_batch(sk, v)
    dec_ms = wall(lambda: ea.decrypt_batch(ct, sk), a.reps)
    assert np.array_equal(ea.decrypt_batch(ct, sk), v)
    rot_ms = []
    for i in range(ea.dimension()):
        rot_ms.append(round(wall(lambda: ea.rotate1D(ct.clone(), i, 1), a.reps), 2))
        r = ct.clone()
        ea.rotate1D(r, i, 1)
        shape = [ea.sizeOfDimension(j) for j in range(ea.dimension())]
        assert np.array_equal(ea.decrypt_batch(r, sk), np.roll(v.reshape(B, *shape), 1, axis=1 + i).reshape(B, n))
    tb = ea.enc.table.table_bytes
    out = {
        "tool": "bench_bgv_crt", "m": m, "p": p, "d": ea.getDegree(), "nslots": n, "signed_orders": z.signedOrds(),
        "bits": a.bits, "L": L, "batch": B, "table_build_s": round(table_s, 2), "table_bytes": tb,
        "encode_ms": round(enc_ms, 2),
        "encode_alg_bytes": tb // 2 * ((B + 15) // 16) + 8 * B * n + 8 * B * N + (1 + L) * N * 8 * B,
        "decrypt_batch_ms": round(dec_ms, 2), "rotate1D_ms_per_dimension": rot_ms,
    }
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
