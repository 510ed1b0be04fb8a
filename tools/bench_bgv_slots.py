#!/usr/bin/env python3
"""BGV slot encryption / decryption on the device (helib_amd.bgv.EncryptedArray: hx_bgv_encode / hx_bgv_decode) against
the path that existed before it, at the headline ring: m = 32768, p = 65537, bits = 950, a batch of 64.

  encrypt_batch   encode (scatter, transform mod p, lift, transforms) + PubKey.EncryptBatch; host samplers included
      vs          B x PubKey.Encrypt of polynomials that are already encoded (balanced_MulMod in a python loop,
                  residues on the host, a batch-1 upload each)
  decrypt_batch   inner product + hx_bgv_decode (one download)
      vs          B x SecKey.Decrypt (hx_poly_rem + the factor in python) + a decode through the public transform
                  (upload mod p, FFT, download, permutation)

Both sides run in this process, wall clock around calls that synchronise; the old path is timed on --host-elems
elements and scaled to the batch.  One JSON line on stdout.

  python tools/bench_bgv_slots.py          # MI355X
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=32768)
    ap.add_argument("--p", type=int, default=65537)
    ap.add_argument("--bits", type=int, default=950)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-elems", type=int, default=2)
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import bgv, capi, ctxt as hc, keys as hk
    m, p, B = a.m, a.p, a.batch
    cc = hc.ChainContext(m, p, 1, bits=a.bits, c=3)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey()
    ea = bgv.EncryptedArray(cc, g)
    idx = list(cc.ctxtPrimes)
    L, N = len(idx), cc.phim
    v = np.random.default_rng(1).integers(0, p, size=(B, N))

    def wall(fn, reps):
        fn()   # warm: tables, buffers
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            g.sync()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best

    enc_ms = wall(lambda: ea.encode(v, idx, mul=3), a.reps)
    encb_ms = wall(lambda: ea.encrypt_batch(sk, v), a.reps)
    ct = ea.encrypt_batch(sk, v)
    decb_ms = wall(lambda: ea.decrypt_batch(ct, sk), a.reps)
    assert np.array_equal(ea.decrypt_batch(ct, sk), v)

    # the old path, on host-elems elements
    E = a.host_elems
    polys = ea.encodeCoeffs(v[:E])
    old_cts = []

    def old_encrypt():
        old_cts[:] = [sk.Encrypt([int(x) for x in polys[b]]) for b in range(E)]
    old_enc_ms = wall(old_encrypt, 1) * B / E
    side = capi.Context(m)
    side.add_prime(p)
    # row position of every slot, from a decode of the identity-like vector through the same public transform
    probe = np.arange(N, dtype=np.int64) % p
    ev = capi.DoubleCRT(side, [0], 1, (ea.encodeCoeffs(probe) % p).astype(np.uint64)[None]).FFT().download()[0, 0]
    assert N <= p and sorted(ev.tolist()) == list(range(N))
    perm = np.argsort(ev)

    def old_decrypt():
        out = []
        for c in old_cts:
            f = np.array(sk.Decrypt(c), dtype=np.uint64)
            out.append(capi.DoubleCRT(side, [0], 1, f[None, None, :]).FFT().download()[0, 0][perm])
        return out
    old_dec_ms = wall(old_decrypt, 1) * B / E
    assert np.array_equal(np.array(old_decrypt(), dtype=np.int64), v[:E])
    out = {
        "tool": "bench_bgv_slots", "m": m, "p": p, "bits": a.bits, "L": L, "batch": B,
        "encode_ms": round(enc_ms, 2), "encode_alg_bytes": (1 + L) * N * 8 * B,
        "encrypt_batch_ms": round(encb_ms, 1), "old_encrypt_ms": round(old_enc_ms, 1),
        "encrypt_speedup": round(old_enc_ms / encb_ms, 1),
        "decrypt_batch_ms": round(decb_ms, 1), "old_decrypt_decode_ms": round(old_dec_ms, 1),
        "decrypt_speedup": round(old_dec_ms / decb_ms, 1), "old_path_elems_timed": E,
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
