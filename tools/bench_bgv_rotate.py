#!/usr/bin/env python3
"""The BGV linear-array rotate at the headline ring (m = 32768, p = 65537, bits = 950, a batch of 64), in one process:

  (a) hx_mask_split (take = keep * mask, keep -= take) against the sequence it replaces -- hx_poly_copy,
      hx_mul, hx_sub per part -- on a two-part ciphertext at the full ctxt prime set, destinations allocated up front:
      device time between two events on the context's stream around --inner calls, alternating sides, medians of
      --reps runs
  (b) ea.rotate(ct, 1), fused against fused=False: wall clock around calls that end in a synchronise (key switching
      dominates; the ciphertext is cloned outside the timed region)
  (c) ea.totalSums on the same ciphertext, --sums-reps runs (14 + 1 rotations each; matrices are generated for exactly
      the automorphisms it walks through)

Writes profiles/bgv_rotate.json (--out) and prints the same JSON line.

  python tools/bench_bgv_rotate.py          # MI355X
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=32768)
    ap.add_argument("--p", type=int, default=65537)
    ap.add_argument("--bits", type=int, default=950)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--sums-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgv_rotate.json"))
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
    sk.zMStar = ea.zMStar
    z, n = ea.zMStar, ea.size()

    # the rotations totalSums makes (src/EncryptedArray.cpp:708-736) and the automorphisms behind them
    rot, e = [], 1
    for i in range(n.bit_length() - 2, -1, -1):
        rot.append(e)
        e *= 2
        if (n >> i) & 1:
            rot.append(e)
            e += 1
    need = set()
    for amt in rot + [1]:
        for i in range(ea.dimension()):
            v = ea.coordinate(i, amt % n)
            need |= {z.genToPow(i, v), z.genToPow(i, (v + 1) % ea.sizeOfDimension(i))}
    for k in sorted(need - {1}):
        sk.GenKeySWmatrix(1, k)
    sk.setKeySwitchMap()

    v = np.random.default_rng(1).integers(0, p, size=(B, n))
    ct = ea.encrypt_batch(sk, v)
    idx = sorted(ct.primeSet)
    L = len(idx)

    # ---- (a) the kernel against the three calls ----
    mask, _ = ea._encodedMask(ea.maskSlots(ea.dimension() - 1, 1), ct.primeSet)
    work = ct.clone()
    keep = [work.parts["1"], work.parts["s"]]
    take = [capi.likeUninit(k) for k in keep]
    lib = capi.lib()

    def fused():
        capi.maskSplit(keep[0], keep[1], take[0], take[1], mask)

    def three():
        for k, t in zip(keep, take):
            capi._chk(lib.hx_poly_copy(t.h, k.h))
            capi._chk(lib.hx_mul(t.h, mask.h))
            capi._chk(lib.hx_sub(k.h, t.h))

    def device_ms(fn):
        g.sync()
        g.timerBegin()
        for _ in range(a.inner):
            fn()
        return g.timerEnd() / a.inner
    for fn in (fused, three):                       # warm: code objects, slabs
        fn()
    tf, t3 = [], []
    for _ in range(a.reps):
        tf.append(device_ms(fused))
        t3.append(device_ms(three))
    split_ms, three_ms = statistics.median(tf), statistics.median(t3)
    word_bytes = 2 * L * B * n * 8                  # one pass over both parts

    # ---- (b), (c) ----
    def wall(fn, reps):
        times = []
        for r in range(reps + 1):                    # the first run warms tables and buffers
            c = ct.clone()
            g.sync()
            t0 = time.perf_counter()
            fn(c)
            c.lnNoise  # noqa: B018 -- completes the deferred norms
            g.sync()
            if r:
                times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times), c
    rot_f, c1 = wall(lambda c: ea.rotate(c, 1, fused=True), a.reps)
    rot_t, c2 = wall(lambda c: ea.rotate(c, 1, fused=False), a.reps)
    assert np.array_equal(ea.decrypt_batch(c1, sk), np.roll(v, 1, axis=1))
    assert np.array_equal(ea.decrypt_batch(c2, sk), np.roll(v, 1, axis=1))
    sum_f, s1 = wall(lambda c: ea.totalSums(c, fused=True), a.sums_reps)
    sum_t, s2 = wall(lambda c: ea.totalSums(c, fused=False), a.sums_reps)
    want = np.repeat(v.sum(axis=1, keepdims=True) % p, n, axis=1)
    sums_ok = bool(np.array_equal(ea.decrypt_batch(s1, sk), want) and np.array_equal(ea.decrypt_batch(s2, sk), want))

    out = {
        "tool": "bench_bgv_rotate", "m": m, "p": p, "bits": a.bits, "L": L, "batch": B, "reps": a.reps,
        "inner": a.inner,
        "mask_split_ms": round(split_ms, 4), "copy_mul_sub_ms": round(three_ms, 4),
        "mask_split_over_sequence": round(split_ms / three_ms, 3), "byte_model_ratio": round(3 / 7, 3),
        "mask_split_faster": bool(split_ms < three_ms),
        "mask_split_GBps": round(3 * word_bytes / split_ms / 1e6, 1),
        "copy_mul_sub_GBps": round(7 * word_bytes / three_ms / 1e6, 1),
        "mask_split_runs_ms": [round(x, 4) for x in tf], "copy_mul_sub_runs_ms": [round(x, 4) for x in t3],
        "rotate1_fused_ms": round(rot_f, 2), "rotate1_termwise_ms": round(rot_t, 2),
        "totalSums_fused_ms": round(sum_f, 1), "totalSums_termwise_ms": round(sum_t, 1),
        "totalSums_rotations": len(rot), "totalSums_capacity_after": round(s1.capacity(), 1),
        "totalSums_correct": sums_ok,
        "fused_default": bool(bgv.EncryptedArray.fuseMaskSplit),
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
