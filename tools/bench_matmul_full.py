#!/usr/bin/env python3
"""matmul_full.MatMulFullExec at the ring of the other slot benchmarks (m = 21845, p = 2: orders (128, 8), both
non-native; 1024 slots; batch 32, add1DMatrices: HELIB_KSS_FULL in both dimensions), in one process:

  stage   the outer stage of the recursion alone -- the 7 masked offsets of the size-8 dimension, from the two digit
          decompositions of a fresh ciphertext and of its copy moved by g^(-8) -- in three forms:
            (a) the four-call sequence per offset (two hoisted automorphisms, multByConstant, +=, multByConstant, -=)
            (b) the sequence with the blend as one hx_mask_blend per offset
            (c) one hx_hoisted_blend for the 7 offsets
          wall clock around calls that end in a synchronise, the forms alternated, --reps rounds after one warm round;
          the words and the bookkeeping of the three forms are compared every round
  whole   MatMulFullExec.mul of a random 1024 x 1024 0/1 matrix in forms (b) (fused=None with Ctxt.fuseHoistedBlend off)
          and (c) (fused=True), alternated likewise; every product is decrypted and checked against bgv_matmul.mulPlain, and the
          two forms' words are compared

Ctxt.fuseHoistedBlend may become True only if (c) is ahead of (b) in every pair of the stage and of the whole product with
the same words.  Writes profiles/matmul_full.json (--out) and prints the same JSON line.

  python tools/bench_matmul_full.py          # MI355X
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
    ap.add_argument("--bits", type=int, default=950)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stage-only", action="store_true", help="skip the whole product")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matmul_full.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import bgv_hypercube, bgv_matmul as bm, capi, ctxt as hc, keys as hk, matmul_full as mf
    m, B = a.m, a.batch
    rng = np.random.default_rng(1)
    shipped = bool(hc.Ctxt.fuseHoistedBlend)

    def note(*what):
        print("[bench_matmul_full]", *what, file=sys.stderr, flush=True)

    t0 = time.perf_counter()
    cc = hc.ChainContext(m, 2, 1, bits=a.bits, c=3)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey()
    ea = bgv_hypercube.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    hk.add1DMatrices(sk)
    note("setup:", round(time.perf_counter() - t0, 1), "s")
    z, n = ea.zMStar, ea.size()
    dims = [(ea.sizeOfDimension(i), bool(ea.nativeDimension(i))) for i in range(ea.dimension())]

    mallocs = {}

    def wall(fn, name):
        """-> (ms, fn()); mallocs[name] counts the arena's hipMalloc calls inside timed runs: a warm loop makes none"""
        g.sync()
        before = g.arenaStats()["sys_calls"]
        t0 = time.perf_counter()
        out = fn()
        for c in out:
            c.lnNoise  # noqa: B018 -- completes the deferred norms
        g.sync()
        ms = (time.perf_counter() - t0) * 1e3
        mallocs[name] = mallocs.get(name, 0) + g.arenaStats()["sys_calls"] - before
        return ms, out

    def runs(xs):
        return [round(x, 3) for x in xs]

    def same_ctxt(x, y):
        return bool(x.primeSet == y.primeSet and x.intFactor == y.intFactor and x.lnNoise == y.lnNoise and
                    x.ptxtMag == y.ptxtMag and all(np.array_equal(x.parts[h].download(), y.parts[h].download()) for h in x.parts))

    def table(times, names):
        r = {}
        for name in names:
            r[name + "_ms"] = round(statistics.median(times[name]), 3)
            r[name + "_runs_ms"] = runs(times[name])
        return r

    v = rng.integers(0, 2, size=(B, n))
    ct = ea.encrypt_batch(sk, v)
    hc.BasicAutomorphPrecon(ct)                         # (warms the digit tables before anything is timed)

    # ---- the stage ----
    dim = sorted(range(ea.dimension()), key=lambda i: (ea.sizeOfDimension(i), not ea.nativeDimension(i)))[0]   # MatMulDimComp
    sdim = ea.sizeOfDimension(dim)
    ct1 = ct.clone()
    ct1.smartAutomorph(z.genToPow(dim, -sdim))
    pre, pre1 = hc.BasicAutomorphPrecon(ct), hc.BasicAutomorphPrecon(ct1)
    offs = list(range(1, sdim))
    ks = [z.genToPow(dim, i) for i in offs]
    primes = set(pre.ctxt.primeSet) | set(pre1.ctxt.primeSet) | set(cc.specialPrimes)
    enc = [ea._encodedMask(ea.maskSlots(dim, i), primes) for i in offs]
    masks, sizes = [mk for mk, _ in enc], [sz for _, sz in enc]

    def per_offset(fused):
        out = []
        for k, mk, sz in zip(ks, masks, sizes):
            out.append(ea._maskBlend(pre.automorph(k), pre1.automorph(k), mk, sz, fused=fused))
        return out
    forms = {"four_calls": lambda: hc.automorphBlend(pre, pre1, ks, masks, sizes, fused=False),
             "mask_blend": lambda: per_offset(True),
             "hoisted_blend": lambda: hc.automorphBlend(pre, pre1, ks, masks, sizes, fused=True)}
    seen, real = [], capi.hoistedBlend
    capi.hoistedBlend = lambda *args: (seen.append(len(args[6])), real(*args))[1]
    times = {name: [] for name in forms}
    last, same = {}, True
    want = [np.roll(v.reshape([B] + [d for d, _ in dims]), i, axis=1 + dim).reshape(B, n) for i in offs]
    right = True
    for rep in range(a.reps + 1):                       # the first round warms tables and buffers
        if rep == 1:
            mallocs.clear()
        for name, fn in forms.items():
            ms, last[name] = wall(fn, name)
            if rep:
                times[name].append(ms)
        same = same and all(same_ctxt(x, y) and same_ctxt(x, w)
                            for x, y, w in zip(last["four_calls"], last["mask_blend"], last["hoisted_blend"]))
        right = right and bool(all(c.isCorrect() and np.array_equal(ea.decrypt_batch(c, sk), w)
                                   for c, w in zip(last["hoisted_blend"], want)))
        last.clear()                                    # the next round reuses this round's blocks
    stage = {"dim": dim, "offsets": len(offs), "ndig": len(pre.digits), "rows": len(pre.ctxt.primeSet) + len(cc.specialPrimes),
             "hoisted_blend_calls": seen[:], "same_words_and_bookkeeping": bool(same), "all_correct": right,
             "hipMallocs_in_timed_runs": dict(mallocs)}
    # the device call alone: stream time between two events around three calls on the blocks the rounds left free
    c, c1 = pre.ctxt, pre1.ctxt
    args = (pre.polyDigits, c.parts["1"], c.parts["s"], pre1.polyDigits, c1.parts["1"], c1.parts["s"], ks,
            [c.ksw_auto[k] for k in ks], masks, list(cc.specialPrimes))
    g.sync()
    g.timerBegin()
    for _ in range(3):
        outs = real(*args)
    stage["hoisted_blend_device_ms"] = round(g.timerEnd() / 3, 3)
    del outs, args, c, c1
    stage.update(table(times, forms))
    stage["hoisted_over_mask_blend"] = round(stage["hoisted_blend_ms"] / stage["mask_blend_ms"], 3)
    stage["hoisted_over_four_calls"] = round(stage["hoisted_blend_ms"] / stage["four_calls_ms"], 3)
    stage["hoisted_faster_than_mask_blend_in_every_pair"] = bool(all(x < y for x, y in zip(times["hoisted_blend"], times["mask_blend"])))
    note("stage", stage)
    del pre, pre1, ct1, masks, enc

    # ---- the whole product ----
    whole = None
    if not a.stage_only:
        A = rng.integers(0, 2, size=(n, n))
        mat = bm.MatMulFull(ea, A)
        t0 = time.perf_counter()
        ex = mf.MatMulFullExec(ea, mat)
        build_s = time.perf_counter() - t0
        note("MatMulFullExec built:", round(build_s, 1), "s;", len(ex.transforms), "transforms, g =", ex.transforms[0].g)
        truth = bm.mulPlain(ea, v, mat)
        forms = {"mask_blend": None, "hoisted_blend": True}
        times = {name: [] for name in forms}
        last, same, right = {}, True, True
        del seen[:]
        for rep in range(a.reps + 1):
            if rep == 1:
                mallocs.clear()
            for name, fused in forms.items():
                hc.Ctxt.fuseHoistedBlend = False     # form (b) is fused=None without the switch, whatever it ships as
                ms, out = wall(lambda: [ex.mul(ct.clone(), pk=sk, fused=fused)], name)
                hc.Ctxt.fuseHoistedBlend = shipped
                last[name] = out[0]
                if rep:
                    times[name].append(ms)
                right = right and bool(out[0].isCorrect() and np.array_equal(ea.decrypt_batch(out[0], sk), truth))
            same = same and same_ctxt(last["mask_blend"], last["hoisted_blend"])
        whole = {"build_s": round(build_s, 1), "transforms": len(ex.transforms), "D": ex.transforms[0].D, "g": ex.transforms[0].g,
                 "all_correct": right, "same_words_and_bookkeeping": bool(same), "hoisted_blend_calls_per_mul": seen[:1],
                 "bitCapacity": int(last["hoisted_blend"].bitCapacity()), "hipMallocs_in_timed_runs": dict(mallocs)}
        whole.update(table(times, forms))
        whole["hoisted_over_mask_blend"] = round(whole["hoisted_blend_ms"] / whole["mask_blend_ms"], 3)
        whole["hoisted_faster_than_mask_blend_in_every_pair"] = bool(all(x < y for x, y in zip(times["hoisted_blend"], times["mask_blend"])))
        note("whole", whole)
    capi.hoistedBlend = real
    qualifies = bool(whole is not None and stage["same_words_and_bookkeeping"] and stage["all_correct"] and
                     stage["hoisted_faster_than_mask_blend_in_every_pair"] and whole["all_correct"] and
                     whole["same_words_and_bookkeeping"] and whole["hoisted_faster_than_mask_blend_in_every_pair"])
    out = {"tool": "bench_matmul_full", "m": m, "p": 2, "phim": g.phim, "nslots": n, "dims": dims, "bits": a.bits, "batch": B,
           "reps": a.reps, "fresh_capacity": int(ct.bitCapacity()), "stage": stage, "whole": whole,
           "hoisted_blend_qualifies": qualifies, "fuseHoistedBlend_default": shipped}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
