#!/usr/bin/env python3
"""Binary arithmetic on encrypted bits at the ring of the other slot benchmarks (m = 21845, p = 2, batch 32), in one
process:

  (a) hx_tensor_sum against the calls it replaces -- n x hx_tensor and the part-wise hx_add of the products
      -- on the parts of fresh ciphertexts, n = 2 and n = 8: device time between two events on the context's stream
      around --inner repetitions, the two sides alternated, --reps pairs after one warm pair
  (b) Ctxt.innerProduct(fused=True) against fused=False on the same ciphertexts, n = 2 and n = 8, measured the same way
  (c) addTwoNumbers (8 + 8 bits), multTwoNumbers (8 x 8 -> 16 bits) and compareTwoNumbers (8 bits) with the lazy carry
      off and on: wall clock around calls that end in a synchronise, alternated, --reps pairs after one warm pair; the
      decrypted results are checked against python integers and the capacity left is recorded.  The lazy side runs its
      inner products through hx_tensor_sum when (a) and (b) found it ahead in every pair, through the loop otherwise.

The words of both sides are compared every time in (a) and (b).  --bits 0 looks for the smallest multiple of 100 at
which the reference-order 8 x 8-bit product completes with every output isCorrect().  Ctxt.fuseTensorSum may become True
only if the fused side is ahead in every pair of (a) and (b); binary_arith.lazyCarry only if the lazy side is ahead in
every pair of (c) and every output is correct.  Writes profiles/binary_arith.json (--out) and prints the same JSON line.

  python tools/bench_binary_arith.py          # MI355X
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
    ap.add_argument("--bits", type=int, default=0, help="0: search upwards from --first-bits in steps of 100")
    ap.add_argument("--first-bits", type=int, default=100)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=8, help="bits per operand in (c)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binary_arith.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import binary_arith as ba, binary_compare as bc, bgv_crt, capi, ctxt as hc, keys as hk
    m, B, S = a.m, a.batch, a.size
    rng = np.random.default_rng(1)

    def note(*what):
        print("[bench_binary_arith]", *what, file=sys.stderr, flush=True)

    def setup(bits):
        cc = hc.ChainContext(m, 2, 1, bits=bits, c=3)
        g = capi.Context(m)
        for q in cc.primes:
            g.add_prime(q)
        sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
        sk.GenSecKey()
        ea = bgv_crt.EncryptedArray(cc, g)
        return cc, g, sk, ea

    def correct(number):
        return bool(all(c.isCorrect() for c in number if c is not None and c.parts))

    def capacity(number):
        return round(min(c.capacity() for c in number if c is not None and c.parts), 1)

    def numbers(ea, sk):
        va = rng.integers(0, 1 << S, size=(B, ea.size()))
        vb = rng.integers(0, 1 << S, size=(B, ea.size()))
        va[0, :2], vb[0, :2] = [0, (1 << S) - 1], [(1 << S) - 1, (1 << S) - 1]
        return va, vb, ba.encryptBinaryNums(ea, sk, va, S), ba.encryptBinaryNums(ea, sk, vb, S)

    # ---- the chain size ----
    search = []
    bits = a.bits or a.first_bits
    while True:
        cc, g, sk, ea = setup(bits)
        va, vb, A, Bn = numbers(ea, sk)
        if a.bits:
            break
        try:
            prod = ba.multTwoNumbers(A, Bn, lazy=False)
            ok = correct(prod)
            search.append({"bits": bits, "completed": True, "isCorrect": ok, "capacity_left": capacity(prod)})
        except RuntimeError as e:                    # the planner's refusals, or a chain that ran out
            ok = False
            search.append({"bits": bits, "completed": False, "refused": str(e)})
        note("chain size", search[-1])
        if ok:
            break
        del cc, g, sk, ea, A, Bn
        bits += 100
    n = ea.size()

    def device_ms(fn):
        g.sync()
        g.timerBegin()
        for _ in range(a.inner):
            out = fn()
        return g.timerEnd() / a.inner, out

    def wall(fn):
        g.sync()
        t0 = time.perf_counter()
        out = fn()
        for c in (out if isinstance(out, list) else [out]):
            if c is not None and c.parts:
                c.lnNoise  # noqa: B018 -- completes the deferred norms
        g.sync()
        return (time.perf_counter() - t0) * 1e3, out

    def pairs(timer, new, old, same):
        tn, to, ok = [], [], True
        for k in range(a.reps + 1):                  # the first pair warms tables and buffers
            ms_n, yn = timer(new)
            ms_o, yo = timer(old)
            ok = ok and same(yn, yo)
            if k:
                tn.append(ms_n)
                to.append(ms_o)
        return tn, to, ok, yn, yo

    def summary(prefix, tn, to, names=("fused", "sequence")):
        return {prefix + names[0] + "_ms": round(statistics.median(tn), 4), prefix + names[1] + "_ms": round(statistics.median(to), 4),
                prefix + names[0] + "_runs_ms": [round(x, 4) for x in tn], prefix + names[1] + "_runs_ms": [round(x, 4) for x in to],
                prefix + names[0] + "_over_" + names[1]: round(statistics.median(tn) / statistics.median(to), 3),
                prefix + names[0] + "_faster_in_every_pair": bool(all(x < y for x, y in zip(tn, to)))}

    # ---- (a), (b) ----
    fresh = [ea.encrypt_batch(sk, rng.integers(0, 2, size=(B, n))) for _ in range(16)]
    rows = len(fresh[0].parts["1"].getIndexSet())
    row_bytes = B * g.phim * 8

    def sequence(cols):
        acc = None
        for t in range(len(cols[0])):
            prod = capi.tensorProduct(cols[0][t], cols[1][t], cols[2][t], cols[3][t])
            if acc is None:
                acc = prod
            else:
                for x, y in zip(acc, prod):
                    x += y
        return acc

    def same_polys(x, y):
        return bool(all(np.array_equal(p.download(), q.download()) for p, q in zip(x, y)))

    def same_ctxt(x, y):
        return bool(x.primeSet == y.primeSet and x.intFactor == y.intFactor and x.lnNoise == y.lnNoise and
                    x.ptxtMag == y.ptxtMag and all(np.array_equal(x.parts[h].download(), y.parts[h].download()) for h in x.parts))
    kernel, inner = {}, {}
    for nt in (2, 8):
        v1, v2 = fresh[:nt], fresh[8:8 + nt]
        cols = [[c.parts["1"] for c in v1], [c.parts["s"] for c in v1], [c.parts["1"] for c in v2], [c.parts["s"] for c in v2]]
        tn, to, ok, _, _ = pairs(device_ms, lambda: capi.tensorSum(*cols), lambda: sequence(cols), same_polys)
        r = summary("tensor_sum_", tn, to)
        r.update({"same_words": ok, "byte_model_ratio": round((4 * nt + 3) / (16 * nt - 9), 3),
                  "tensor_sum_GBps": round((4 * nt + 3) * rows * row_bytes / statistics.median(tn) / 1e6, 1),
                  "sequence_GBps": round((16 * nt - 9) * rows * row_bytes / statistics.median(to) / 1e6, 1)})
        kernel["n%d" % nt] = r
        tn, to, ok, y, _ = pairs(device_ms, lambda: hc.Ctxt.innerProduct(v1, v2, fused=True),
                                 lambda: hc.Ctxt.innerProduct(v1, v2, fused=False), same_ctxt)
        r = summary("inner_product_", tn, to, ("fused", "loop"))
        r.update({"same_words_and_bookkeeping": ok, "isCorrect": bool(y.isCorrect()), "capacity_left": round(y.capacity(), 1)})
        inner["n%d" % nt] = r
        note("n =", nt, kernel["n%d" % nt], r)
    fused_wins = bool(all(r["tensor_sum_fused_faster_in_every_pair"] and r["same_words"] for r in kernel.values()) and
                      all(r["inner_product_fused_faster_in_every_pair"] and r["same_words_and_bookkeeping"]
                          for r in inner.values()))
    del fresh

    # ---- (c) ----
    flags = (hc.Ctxt.fuseTensorSum, ba.lazyCarry)

    def run(fn, lazy):
        hc.Ctxt.fuseTensorSum, ba.lazyCarry = (fused_wins and lazy), lazy
        try:
            return fn()
        finally:
            hc.Ctxt.fuseTensorSum, ba.lazyCarry = flags
    circuits = {}
    wants = {"addTwoNumbers": lambda out: np.array_equal(ba.decryptBinaryNums(out, sk, ea), va + vb),
             "multTwoNumbers": lambda out: np.array_equal(ba.decryptBinaryNums(out, sk, ea), va * vb),
             "compareTwoNumbers": lambda out: (np.array_equal(ba.decryptBinaryNums(out[:S], sk, ea), np.maximum(va, vb)) and
                                               np.array_equal(ba.decryptBinaryNums(out[S:2 * S], sk, ea), np.minimum(va, vb)) and
                                               np.array_equal(ba.decryptBinaryNums(out[2 * S:2 * S + 1], sk, ea), (va > vb) * 1) and
                                               np.array_equal(ba.decryptBinaryNums(out[2 * S + 1:], sk, ea), (va < vb) * 1))}

    def compare():
        mx, mn, mu, ni = bc.compareTwoNumbers(A, Bn)
        return mx + mn + [mu, ni]
    calls = {"addTwoNumbers": lambda: ba.addTwoNumbers(A, Bn), "multTwoNumbers": lambda: ba.multTwoNumbers(A, Bn),
             "compareTwoNumbers": compare}
    for name, fn in calls.items():
        tl, tr, _, yl, yr = pairs(wall, lambda: run(fn, True), lambda: run(fn, False), lambda x, y: True)
        r = summary("", tl, tr, ("lazy", "reference"))
        r.update({"lazy_correct": bool(wants[name](yl)), "reference_correct": bool(wants[name](yr)),
                  "lazy_isCorrect": correct(yl), "reference_isCorrect": correct(yr),
                  "lazy_capacity_left": capacity(yl), "reference_capacity_left": capacity(yr)})
        circuits[name] = r
        note(name, r)
    lazy_wins = bool(all(r["lazy_faster_in_every_pair"] and r["lazy_correct"] and r["reference_correct"] and
                         r["lazy_isCorrect"] and r["reference_isCorrect"] for r in circuits.values()))

    out = {"tool": "bench_binary_arith", "m": m, "p": 2, "phim": g.phim, "nslots": n, "bits": bits, "bits_search": search,
           "fresh_capacity": round(A[0].capacity(), 1), "batch": B, "operand_bits": S, "reps": a.reps, "inner": a.inner,
           "ctxt_rows": rows, "tensor_sum": kernel, "inner_product": inner, "circuits": circuits,
           "lazy_side_used_tensor_sum": fused_wins,
           "tensor_sum_faster_in_every_pair": fused_wins, "lazy_faster_in_every_pair": lazy_wins,
           "fuseTensorSum_default": bool(hc.Ctxt.fuseTensorSum), "lazyCarry_default": bool(ba.lazyCarry)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
