"""BGV slots in GF(p^d) (helib_amd.bgv_gf) on the ring the project is measured on: m = 21845, p = 2 (d = 16, 1024
slots of GF(2^16)), bits = 950, batch 64.  Records the table construction time and bytes, the GF encode, the GF
decrypt_batch and -- in the same run, on the same context -- the integer encode of helib_amd.bgv_crt with the ratio of
the two encodes, and writes one JSON object to profiles/bgv_gf.json.  The GF encode does d times the multiply-adds of
the integer encode over the same bytes of E: a ratio near d means issue-bound, a lower one that the table traffic still
matters.  Wall clock around synchronising calls, best of --reps.

  python tools/bench_bgv_gf.py          # MI355X
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgv_gf.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import bgv_crt, bgv_gf, capi, ctxt as hc, keys as hk
    m, p, B = a.m, a.p, a.batch
    cc = hc.ChainContext(m, p, 1, bits=a.bits, c=3)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey()
    t0 = time.perf_counter()
    ea = bgv_gf.EncryptedArray(cc, g)
    table_s = time.perf_counter() - t0
    ints = bgv_crt.EncryptedArray(cc, g)
    idx = list(cc.ctxtPrimes)
    L, N, n, d = len(idx), cc.phim, ea.size(), ea.getDegree()
    rng = np.random.default_rng(1)
    v = rng.integers(0, p, size=(B, n, d))
    k = rng.integers(0, p, size=(B, n))

    def wall(fn, reps):
        fn()   # warm: buffers
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            g.sync()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best

    gf_ms = wall(lambda: ea.encode(v, idx, mul=1), a.reps)
    int_ms = wall(lambda: ints.encode(k, idx, mul=1), a.reps)
    ct = ea.encrypt_batch(sk, v)
    dec_ms = wall(lambda: ea.decrypt_batch(ct, sk), a.reps)
    assert np.array_equal(ea.decrypt_batch(ct, sk), v)
    assert np.array_equal(ea.encodeCoeffs(k), ints.encodeCoeffs(k))
    tb = ea.enc.table.table_bytes
    out = {
        "tool": "bench_bgv_gf", "m": m, "p": p, "d": d, "nslots": n, "signed_orders": ea.zMStar.signedOrds(),
        "bits": a.bits, "L": L, "batch": B, "table_build_s": round(table_s, 2), "table_bytes": tb,
        "gf_encode_ms": round(gf_ms, 2), "int_encode_ms": round(int_ms, 2), "gf_over_int_encode": round(gf_ms / int_ms, 2),
        "gf_encode_multiply_adds": B * n * d * (N + d - 1) + B * n * d * d + B * N * (d - 1),
        "gf_decrypt_batch_ms": round(dec_ms, 2),
    }
    print(json.dumps(out))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
