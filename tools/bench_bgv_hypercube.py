#!/usr/bin/env python3
"""The masked rotations over non-native dimensions at the flagship ring (m = 21845, p = 2: 1024 slots, signed orders
-128, -8; bits = 950, a batch of 64), in one process:

  (a) hx_mask_blend (c = c*mask + t - t*mask) against the sequence it replaces -- hx_mul, hx_add, hx_mul,
      hx_sub per part -- on the same two-part operands at the full ctxt prime set: device time between two events on
      the context's stream around --inner calls, the two sides alternated, --reps runs each (3: the default
      fuseMaskBlend may become True only if the kernel wins every pair)
  (b) ea.rotate(ct, 1) and ea.totalSums(ct), fused=True against fused=False: wall clock around calls that end in a
      synchronise (key switching dominates; the ciphertext is cloned outside the timed region; matrices are generated
      for exactly the automorphisms walked through)

Writes profiles/bgv_hypercube.json (--out) and prints the same JSON line.

  python tools/bench_bgv_hypercube.py          # MI355X
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
    ap.add_argument("--m", type=int, default=21845)
    ap.add_argument("--p", type=int, default=2)
    ap.add_argument("--bits", type=int, default=950)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rotate-reps", type=int, default=5)
    ap.add_argument("--sums-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgv_hypercube.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import bgv_hypercube, capi, ctxt as hc, keys as hk
    m, p, B = a.m, a.p, a.batch
    cc = hc.ChainContext(m, p, 1, bits=a.bits, c=3)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey()
    ea = bgv_hypercube.EncryptedArray(cc, g)
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
            v, ord_ = ea.coordinate(i, amt % n), ea.sizeOfDimension(i)
            need |= {z.genToPow(i, v), z.genToPow(i, (v + 1) % ord_)}
            if not ea.nativeDimension(i):
                need.add(z.genToPow(i, -ord_))
    for k in sorted(need - {1}):
        sk.GenKeySWmatrix(1, k)
    sk.setKeySwitchMap()

    v = np.random.default_rng(1).integers(0, p, size=(B, n))
    ct = ea.encrypt_batch(sk, v)
    idx = sorted(ct.primeSet)
    L = len(idx)

    # ---- (a) the kernel against the four calls ----
    mask, _ = ea._encodedMask(ea.maskSlots(ea.dimension() - 1, 1), ct.primeSet)
    wc, wt = ct.clone(), ea.encrypt_batch(sk, v)
    c = [wc.parts["1"], wc.parts["s"]]
    t = [wt.parts["1"], wt.parts["s"]]
    lib = capi.lib()

    def fused():
        capi.maskBlend(c[0], c[1], t[0], t[1], mask)

    def four():
        for x, y in zip(c, t):
            capi._chk(lib.hx_mul(x.h, mask.h))
            capi._chk(lib.hx_add(x.h, y.h))
            capi._chk(lib.hx_mul(y.h, mask.h))
            capi._chk(lib.hx_sub(x.h, y.h))

    def device_ms(fn):
        g.sync()
        g.timerBegin()
        for _ in range(a.inner):
            fn()
        return g.timerEnd() / a.inner
    for fn in (fused, four):                        # warm: code objects, slabs (and c no longer shares rows)
        fn()
    tf, t4 = [], []
    for _ in range(a.reps):
        tf.append(device_ms(fused))
        t4.append(device_ms(four))
    blend_ms, four_ms = statistics.median(tf), statistics.median(t4)
    word_bytes = 2 * L * B * g.phim * 8             # one pass over both parts

    # ---- (b) ----
    def wall(fn, reps):
        times = []
        for r in range(reps + 1):                    # the first run warms tables and buffers
            x = ct.clone()
            g.sync()
            t0 = time.perf_counter()
            fn(x)
            x.lnNoise  # noqa: B018 -- completes the deferred norms
            g.sync()
            if r:
                times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times), x
    rot_f, c1 = wall(lambda x: ea.rotate(x, 1, fused=True), a.rotate_reps)
    rot_t, c2 = wall(lambda x: ea.rotate(x, 1, fused=False), a.rotate_reps)
    rot_ok = bool(np.array_equal(ea.decrypt_batch(c1, sk), np.roll(v, 1, axis=1))
                  and np.array_equal(ea.decrypt_batch(c2, sk), np.roll(v, 1, axis=1)))
    sum_f, s1 = wall(lambda x: ea.totalSums(x, fused=True), a.sums_reps)
    sum_t, s2 = wall(lambda x: ea.totalSums(x, fused=False), a.sums_reps)
    want = np.repeat(v.sum(axis=1, keepdims=True) % p, n, axis=1)
    sums_ok = bool(np.array_equal(ea.decrypt_batch(s1, sk), want) and np.array_equal(ea.decrypt_batch(s2, sk), want))

    out = {
        "tool": "bench_bgv_hypercube", "m": m, "p": p, "phim": g.phim, "nslots": n, "ords": z.signedOrds(),
        "bits": a.bits, "L": L, "batch": B, "reps": a.reps, "inner": a.inner,
        "mask_blend_ms": round(blend_ms, 4), "mul_add_mul_sub_ms": round(four_ms, 4),
        "mask_blend_over_sequence": round(blend_ms / four_ms, 3), "byte_model_ratio": round(3 / 10, 3),
        "mask_blend_faster_in_every_pair": bool(all(x < y for x, y in zip(tf, t4))),
        "mask_blend_GBps": round(3 * word_bytes / blend_ms / 1e6, 1),
        "mul_add_mul_sub_GBps": round(10 * word_bytes / four_ms / 1e6, 1),
        "mask_blend_runs_ms": [round(x, 4) for x in tf], "mul_add_mul_sub_runs_ms": [round(x, 4) for x in t4],
        "rotate1_fused_ms": round(rot_f, 2), "rotate1_termwise_ms": round(rot_t, 2), "rotate1_correct": rot_ok,
        "totalSums_fused_ms": round(sum_f, 1), "totalSums_termwise_ms": round(sum_t, 1),
        "totalSums_rotations": len(rot), "totalSums_capacity_after": round(s1.capacity(), 1),
        "totalSums_correct": sums_ok,
        "fused_default": bool(bgv_hypercube.EncryptedArray.fuseMaskBlend),
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
