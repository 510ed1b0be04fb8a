#!/usr/bin/env python3
"""Table lookup on encrypted indices at the ring of the other slot benchmarks (m = 21845, p = 2, batch 32), index widths
5 and 8, in one process:

  (a) hx_table_tensor_sum against the l + 1 calls it replaces -- l x hx_mul_add_many and one hx_tensor_sum
      -- on the parts of fresh ciphertexts brought to one prime set, (k, l) = (16, 2) and (16, 16): device time between
      two events on the context's stream around --inner repetitions, the two sides alternated, --reps pairs after one warm
      pair; the words of both sides are compared every time
  (b) whole tableLookup calls in three forms -- default (the reference's), lazy through the existing calls, lazy through
      hx_table_tensor_sum -- wall clock around calls that end in a synchronise, alternated, --reps rounds after one warm
      round; every result is decrypted and checked against the table, the two lazy forms' words are compared, and the
      capacity left by each form is recorded

--bits 0 looks for the smallest multiple of 100 at which the default form at the widest index keeps its output
isCorrect().  Ctxt.fuseTableSum may become True only if the fused side is ahead in every pair of (a) and of (b) with the
same words; table_lookup.lazyLookup only if the lazy side (its faster path) is ahead of the default in every pair of (b)
and every output is correct.  Writes profiles/table_lookup.json (--out) and prints the same JSON line.

  python tools/bench_table_lookup.py          # MI355X
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
    ap.add_argument("--first-bits", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--widths", type=int, nargs="+", default=[5, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_lookup.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import bgv_gf, capi, ctxt as hc, keys as hk, table_lookup as tl
    m, B = a.m, a.batch
    rng = np.random.default_rng(1)

    def note(*what):
        print("[bench_table_lookup]", *what, file=sys.stderr, flush=True)

    def setup(bits):
        cc = hc.ChainContext(m, 2, 1, bits=bits, c=3)
        g = capi.Context(m)
        for q in cc.primes:
            g.add_prime(q)
        sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
        sk.GenSecKey()
        return cc, g, sk, bgv_gf.EncryptedArray(cc, g)

    def problem(ea, sk, nBits):
        n, d = ea.size(), ea.getDegree()
        index = rng.integers(0, 1 << nBits, size=(B, n))
        index[0, :2] = [0, (1 << nBits) - 1]
        slots = rng.integers(0, 2, size=(1 << nBits, n, d))
        idx = [ea.encrypt_batch(sk, (index >> i) & 1) for i in range(nBits)]
        return tl.LookupTable.fromSlots(ea, slots), idx, slots[index, np.arange(n)[None, :]]

    # ---- the chain size ----
    search = []
    bits = a.bits or a.first_bits
    widest = max(a.widths)
    while True:
        cc, g, sk, ea = setup(bits)
        if a.bits:
            break
        table, idx, want = problem(ea, sk, widest)
        try:
            out = tl.tableLookup(ea, table, idx, lazy=False)
            ok = bool(out.isCorrect() and np.array_equal(ea.decrypt_batch(out, sk), want))
            search.append({"bits": bits, "completed": True, "isCorrect_and_right": ok, "capacity_left": round(out.capacity(), 1)})
        except RuntimeError as e:                    # the level check's refusal, or a chain that ran out
            ok = False
            search.append({"bits": bits, "completed": False, "refused": str(e)})
        note("chain size", search[-1])
        del table, idx
        if ok:
            break
        del cc, g, sk, ea
        bits += 100

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
        out.lnNoise  # noqa: B018 -- completes the deferred norms
        g.sync()
        return (time.perf_counter() - t0) * 1e3, out

    def runs(xs):
        return [round(x, 4) for x in xs]

    def same_polys(x, y):
        return bool(all(np.array_equal(p.download(), q.download()) for p, q in zip(x, y)))

    def same_ctxt(x, y):
        return bool(x.primeSet == y.primeSet and x.intFactor == y.intFactor and x.lnNoise == y.lnNoise and
                    x.ptxtMag == y.ptxtMag and all(np.array_equal(x.parts[h].download(), y.parts[h].download()) for h in x.parts))

    kernel, lookups = {}, {}
    fresh_capacity = None
    for nBits in a.widths:
        k, l = tl.splitSizes(nBits)
        size = k * l
        table, idx, want = problem(ea, sk, nBits)
        fresh_capacity = round(idx[0].capacity(), 1)
        # ---- (a): k + l fresh ciphertexts stand in for products1 and products2 ----
        fresh = [ea.encrypt_batch(sk, rng.integers(0, 2, size=(B, ea.size()))) for _ in range(min(k + l, 32))]
        A, Bs = [fresh[i % len(fresh)] for i in range(k)], [fresh[(k + j) % len(fresh)] for j in range(l)]
        a0, a1 = [c.parts["1"] for c in A], [c.parts["s"] for c in A]
        b0, b1 = [c.parts["1"] for c in Bs], [c.parts["s"] for c in Bs]
        rows = a0[0].getIndexSet()
        poly, consts = table.encoded(rows, size)

        def sequence():
            w0, w1 = [], []
            for j in range(l):
                u0, u1 = capi.likeUninit(a0[0]), capi.likeUninit(a0[0])
                capi.mulAddMany(u0, u1, consts[j * k:(j + 1) * k], a0, a1, accumulate=False)
                w0.append(u0)
                w1.append(u1)
            return capi.tensorSum(w0, w1, b0, b1)
        tn, to, ok = [], [], True
        for rep in range(a.reps + 1):                # the first pair warms tables and buffers
            ms_n, yn = device_ms(lambda: capi.tableTensorSum(a0, a1, b0, b1, poly, size))
            ms_o, yo = device_ms(sequence)
            ok = ok and same_polys(yn, yo)
            if rep:
                tn.append(ms_n)
                to.append(ms_o)
        row_bytes = B * g.phim * 8
        r = {"k": k, "l": l, "size": size, "rows": len(rows),
             "fused_ms": round(statistics.median(tn), 4), "sequence_ms": round(statistics.median(to), 4),
             "fused_runs_ms": runs(tn), "sequence_runs_ms": runs(to),
             "fused_over_sequence": round(statistics.median(tn) / statistics.median(to), 3),
             "fused_faster_in_every_pair": bool(all(x < y for x, y in zip(tn, to))), "same_words": ok,
             # passes over a row of the batch: the table's entries are 1 / B of one each
             "fused_passes": round(k * l / 2 + k * l / B + 2 * l + 3, 1),
             "sequence_passes": round(2 * k * l + k * l / B + 2 * l + 4 * l + 3, 1),
             "fused_GBps": round((k * l / 2 + k * l / B + 2 * l + 3) * len(rows) * row_bytes / statistics.median(tn) / 1e6, 1),
             "sequence_GBps": round((2 * k * l + k * l / B + 6 * l + 3) * len(rows) * row_bytes / statistics.median(to) / 1e6, 1)}
        kernel["w%d" % nBits] = r
        note("kernel, width", nBits, r)
        del fresh, A, Bs, a0, a1, b0, b1, poly, consts
        # ---- (b) ----
        forms = {"default": lambda: tl.tableLookup(ea, table, idx, lazy=False),
                 "lazy": lambda: tl.tableLookup(ea, table, idx, lazy=True, fused=False),
                 "fused": lambda: tl.tableLookup(ea, table, idx, lazy=True, fused=True)}
        times = {name: [] for name in forms}
        last, same = {}, True
        for rep in range(a.reps + 1):
            for name, fn in forms.items():
                ms, last[name] = wall(fn)
                if rep:
                    times[name].append(ms)
            same = same and same_ctxt(last["lazy"], last["fused"])
        r = {"same_words_and_bookkeeping_lazy_fused": same}
        for name in forms:
            r.update({name + "_ms": round(statistics.median(times[name]), 3), name + "_runs_ms": runs(times[name]),
                      name + "_right": bool(np.array_equal(ea.decrypt_batch(last[name], sk), want)),
                      name + "_isCorrect": bool(last[name].isCorrect()), name + "_capacity_left": round(last[name].capacity(), 1)})
        r["fused_faster_than_lazy_in_every_pair"] = bool(all(x < y for x, y in zip(times["fused"], times["lazy"])))
        r["lazy_faster_than_default_in_every_pair"] = bool(all(x < y for x, y in zip(times["lazy"], times["default"])))
        r["fused_faster_than_default_in_every_pair"] = bool(all(x < y for x, y in zip(times["fused"], times["default"])))
        r["lazy_over_default"] = round(r["lazy_ms"] / r["default_ms"], 3)
        r["fused_over_default"] = round(r["fused_ms"] / r["default_ms"], 3)
        r["fused_over_lazy"] = round(r["fused_ms"] / r["lazy_ms"], 3)
        lookups["w%d" % nBits] = r
        note("lookup, width", nBits, r)
        del table, idx, last
    right = all(r[n + "_right"] and r[n + "_isCorrect"] for r in lookups.values() for n in ("default", "lazy", "fused"))
    fused_wins = bool(right and all(r["fused_faster_in_every_pair"] and r["same_words"] for r in kernel.values()) and
                      all(r["fused_faster_than_lazy_in_every_pair"] and r["same_words_and_bookkeeping_lazy_fused"]
                          for r in lookups.values()))
    lazy_wins = bool(right and all(r["fused_faster_than_default_in_every_pair" if fused_wins else
                                     "lazy_faster_than_default_in_every_pair"] for r in lookups.values()))
    out = {"tool": "bench_table_lookup", "m": m, "p": 2, "phim": g.phim, "nslots": ea.size(), "d": ea.getDegree(), "bits": bits,
           "bits_search": search, "fresh_capacity": fresh_capacity, "batch": B, "widths": a.widths, "reps": a.reps,
           "inner": a.inner, "table_tensor_sum": kernel, "table_lookup": lookups,
           "table_tensor_sum_faster_in_every_pair": fused_wins, "lazy_faster_in_every_pair": lazy_wins,
           "fuseTableSum_default": bool(hc.Ctxt.fuseTableSum), "lazyLookup_default": bool(tl.lazyLookup)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
