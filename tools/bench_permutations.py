#!/usr/bin/env python3
"""Slot permutations at the flagship ring (m = 21845, p = 2: 1024 slots, signed orders -128, -8; bits = 950, a batch of
32), in one process, for two depth bounds -- one that leaves the optimiser room for uncollapsed Benes levels (--deep)
and a smaller one that makes it collapse them into layers of many shift amounts (--shallow):

  (a) host: GeneratorTrees.buildOptimalTrees (PermIndepPrecomp) and PermNetwork.buildNetwork (PermPrecomp) for one
      seeded random permutation; wall clock
  (b) keys.addMatrices4Network: wall clock around a call that ends in a synchronise, and the number of matrices
  (c) PermNetwork.applyToCtxt, fused=True against fused=False from clones of one ciphertext: wall clock around calls
      that end in a synchronise; the words of every part are asserted equal, the decryption is compared with
      applyPermToVec
  (d) the mask stage of one layer (the widest of the network) alone -- capi.maskFan into K lazy copies of the
      ciphertext's parts against K x (clone, multByConstant) on the same ciphertext -- device time between two events on
      the context's stream around --inner repetitions, the two sides alternated, --reps pairs (at least 5: the default
      PermNetwork.fuseMaskFan may become True only if the kernel wins every pair); the words are asserted equal every
      time

Writes profiles/permutations.json (--out) and prints the same JSON line.

  python tools/bench_permutations.py          # MI355X
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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--deep", type=int, default=15)
    ap.add_argument("--shallow", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--apply-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "permutations.json"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: at least 5 alternated pairs")
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import bgv_hypercube, capi, ctxt as hc, keys as hk, permutations as P
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
    rng = np.random.default_rng(1)
    pi = P.randomPerm(n, rng)
    v = rng.integers(0, p, size=(B, n))
    want = P.applyPermToVec(v.T, pi).T

    # ---- (a), (b): the networks and their matrices, before anything is encrypted ----
    runs = {}
    for name, depth in (("deep", a.deep), ("shallow", a.shallow)):
        t0 = time.perf_counter()
        pip = P.PermIndepPrecomp(ea, depth)
        t1 = time.perf_counter()
        pp = P.PermPrecomp(pip, pi)
        t2 = time.perf_counter()
        before = len(sk.keySwitching)
        g.sync()
        t3 = time.perf_counter()
        hk.addMatrices4Network(sk, pp.net)
        g.sync()
        t4 = time.perf_counter()
        ks = [len(pp.net.getLayer(i).amounts()) for i in range(pp.net.depth()) if not pp.net.getLayer(i).isID]
        runs[name] = {"pp": pp, "depth_bound": depth, "layers": pp.net.depth(), "cost": pip.getCost(),
                      "shift_amounts_per_layer": ks,
                      "leaves": [[(d.size, d.good, d.e, d.frstBenes, d.scndBenes) for d in T.leaves()] for T in pip.trees.trees],
                      "trees_ms": round((t1 - t0) * 1e3, 2), "buildNetwork_ms": round((t2 - t1) * 1e3, 2),
                      "matrices_added": len(sk.keySwitching) - before, "addMatrices4Network_ms": round((t4 - t3) * 1e3, 1)}
    ct = ea.encrypt_batch(sk, v)
    L = len(ct.primeSet)

    def words(c):
        return {h: part.download() for h, part in c.parts.items()}

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

    # ---- (c) ----
    for name, r in runs.items():
        pp = r["pp"]
        tf, cf = wall(lambda x: pp.apply(x, fused=True), a.apply_reps)
        tu, cu = wall(lambda x: pp.apply(x, fused=False), a.apply_reps)
        wf, wu = words(cf), words(cu)
        assert list(wf) == list(wu) and all(np.array_equal(wf[h], wu[h]) for h in wf), "fused and unfused words differ"
        assert (cf.lnNoise, cf.ptxtMag, cf.primeSet, cf.intFactor) == (cu.lnNoise, cu.ptxtMag, cu.primeSet, cu.intFactor)
        r.update({"applyToCtxt_fused_ms": round(tf, 1), "applyToCtxt_unfused_ms": round(tu, 1),
                  "applyToCtxt_correct": bool(np.array_equal(ea.decrypt_batch(cf, sk), want)),
                  "isCorrect_after": bool(cf.isCorrect()), "capacity_after": round(cf.capacity(), 1)})

    # ---- (d) the mask stage of the widest layer of each network, on the fresh ciphertext ----
    def device_ms(fn):
        g.sync()
        g.timerBegin()
        for _ in range(a.inner):
            out = fn()
        return g.timerEnd() / a.inner, out
    for name, r in runs.items():
        net = r["pp"].net
        lyr = max((net.getLayer(i) for i in range(net.depth()) if not net.getLayer(i).isID), key=lambda x: len(x.amounts()))
        masks = [mk for _, mk in lyr.amounts()]
        K = len(masks)
        enc = [ea._encodedMask(mk, ct.primeSet) for mk in masks]     # (held here: the array's cache keeps 32)
        hs = list(ct.parts)

        def fused():
            tmps = [ct.clone() for _ in range(K)]
            capi.maskFan([t.parts[hs[0]] for t in tmps], [t.parts[hs[1]] for t in tmps], ct.parts[hs[0]], ct.parts[hs[1]],
                         [d for d, _ in enc])
            return tmps

        def unfused():
            tmps = []
            for d, size in enc:
                t = ct.clone()
                t.multByConstant(d, size)
                tmps.append(t)
            return tmps
        for fn in (fused, unfused):                   # warm: code objects, slabs
            fn()
        tf, tu = [], []
        for _ in range(a.reps):
            x, of = device_ms(fused)
            y, ou = device_ms(unfused)
            tf.append(x)
            tu.append(y)
            for s, t in zip(of, ou):
                for h in hs:
                    assert np.array_equal(s.parts[h].download(), t.parts[h].download()), "mask stage: words differ"
            del of, ou
        part_bytes = L * B * g.phim * 8                # one pass over one part
        fan_ms, seq_ms = statistics.median(tf), statistics.median(tu)
        r.update({"mask_stage_K": K, "mask_fan_ms": round(fan_ms, 4), "copy_mul_ms": round(seq_ms, 4),
                  "mask_fan_over_sequence": round(fan_ms / seq_ms, 3),
                  "byte_model_ratio": round((1 + K) / (4 * K), 3),
                  "mask_fan_faster_in_every_pair": bool(all(x < y for x, y in zip(tf, tu))),
                  "mask_fan_GBps": round(2 * (1 + K) * part_bytes / fan_ms / 1e6, 1),
                  "copy_mul_GBps": round(2 * 4 * K * part_bytes / seq_ms / 1e6, 1),
                  "mask_fan_runs_ms": [round(x, 4) for x in tf], "copy_mul_runs_ms": [round(x, 4) for x in tu]})
        del r["pp"]

    out = {"tool": "bench_permutations", "m": m, "p": p, "phim": g.phim, "nslots": n, "ords": z.signedOrds(),
           "bits": a.bits, "L": L, "batch": B, "reps": a.reps, "inner": a.inner, "apply_reps": a.apply_reps,
           "deep": runs["deep"], "shallow": runs["shallow"],
           "mask_fan_faster_in_every_pair": bool(all(r["mask_fan_faster_in_every_pair"] for r in runs.values())),
           "fused_default": bool(P.PermNetwork.fuseMaskFan)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
