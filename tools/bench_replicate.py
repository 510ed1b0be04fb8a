#!/usr/bin/env python3
"""replicateAll at the ring of the other slot benchmarks (m = 21845, p = 2, batch 32, add1DMatrices), in one process:

  (a) hx_hoisted_mask_fan against the calls it replaces at n = 1 and n = 2 -- per term a copy and
      hx_automorph of the digit block and of c0, hx_add_primes_and_scale, a zero part, hx_key_switch_digits, two hx_mul,
      two masked copies of the input, hx_add_primes_and_scale and two hx_add -- on the digit block of a fresh ciphertext:
      device time between two events on the context's stream around --inner repetitions, the two sides alternated, --reps
      pairs after one warm pair; the words of both sides are compared every time
  (b) a whole replicateAll, stopped by its handler after the first --outputs outputs, in three forms -- the reference's,
      hoisted through the existing calls, hoisted through hx_hoisted_mask_fan -- wall clock around calls that end in a
      synchronise, alternated, --reps rounds after one warm round; every produced output is decrypted and checked and its
      bitCapacity recorded, and the two hoisted forms' words are compared

--bits 0 looks for the smallest multiple of 100 at which the reference's form gives every checked output correct.
Ctxt.fuseHoistedFan may become True only if the kernel is ahead of the calls in every pair of (a) and of (b) with the same
words; replicate.hoistNodes only if the hoisted form (its faster path) is ahead of the reference's in every pair of (b),
every output is correct, and its capacity at the deepest recorded output is within 2 bits of the reference's.  Writes
profiles/replicate.json (--out) and prints the same JSON line.

  python tools/bench_replicate.py          # MI355X
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


class _Enough(Exception):
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=21845)
    ap.add_argument("--bits", type=int, default=0, help="0: search upwards from --first-bits in steps of 100")
    ap.add_argument("--first-bits", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--outputs", type=int, default=64)
    ap.add_argument("--recBound", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replicate.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import bgv_gf, capi, ctxt as hc, keys as hk, replicate as R
    m, B = a.m, a.batch
    rng = np.random.default_rng(1)

    def note(*what):
        print("[bench_replicate]", *what, file=sys.stderr, flush=True)

    def setup(bits):
        cc = hc.ChainContext(m, 2, 1, bits=bits, c=3)
        g = capi.Context(m)
        for q in cc.primes:
            g.add_prime(q)
        sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
        sk.GenSecKey()
        ea = bgv_gf.EncryptedArray(cc, g)
        sk.zMStar = ea.zMStar
        hk.add1DMatrices(sk)
        return cc, g, sk, ea

    class First(R.ReplicateHandler):
        """keeps the first --outputs outputs (lazy copies), then stops the recursion"""

        def __init__(self):
            self.v = []

        def handle(self, ct):
            self.v.append(ct.clone())
            if len(self.v) >= a.outputs:
                raise _Enough()

    def run(ea, ct, aux, **kw):
        h = First()
        try:
            R.replicateAll(ea, ct, h, a.recBound, aux, **kw)
        except _Enough:
            pass
        return h.v

    def problem(ea, sk):
        # integers in the slots: a rotation that goes around a non-native dimension applies the Frobenius map
        v = np.zeros((B, ea.size(), ea.getDegree()), dtype=np.int64)
        v[:, :, 0] = rng.integers(0, 2, size=(B, ea.size()))
        return v, ea.encrypt_batch(sk, v)

    def checked(ea, sk, v, outs):
        ok = [bool(c.isCorrect() and np.array_equal(ea.decrypt_batch(c, sk), R.replicatePlain(v, i, axis=1)))
              for i, c in enumerate(outs)]
        return all(ok), [int(c.bitCapacity()) for c in outs]

    # ---- the chain size ----
    search = []
    bits = a.bits or a.first_bits
    while True:
        t0 = time.perf_counter()
        cc, g, sk, ea = setup(bits)
        note("setup at", bits, "bits:", round(time.perf_counter() - t0, 1), "s")
        if a.bits:
            break
        v, ct = problem(ea, sk)
        outs = run(ea, ct, None, hoisted=False)
        ok, caps = checked(ea, sk, v, outs)
        search.append({"bits": bits, "outputs": len(outs), "all_correct": ok, "least_capacity": min(caps)})
        note("chain size", search[-1])
        del outs, ct
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
        for c in out:
            c.lnNoise  # noqa: B018 -- completes the deferred norms
        g.sync()
        return (time.perf_counter() - t0) * 1e3, out

    def runs(xs):
        return [round(x, 4) for x in xs]

    def same_ctxt(x, y):
        return bool(x.primeSet == y.primeSet and x.intFactor == y.intFactor and x.lnNoise == y.lnNoise and
                    x.ptxtMag == y.ptxtMag and all(np.array_equal(x.parts[h].download(), y.parts[h].download()) for h in x.parts))

    v, ct = problem(ea, sk)
    fresh_capacity = int(ct.bitCapacity())
    sp = list(cc.specialPrimes)
    z = ea.zMStar

    # ---- (a) ----
    pre = hc.BasicAutomorphPrecon(ct)
    c0, c1, dg = pre.ctxt.parts["1"], pre.ctxt.parts["s"], pre.polyDigits
    ndig, rows = len(pre.digits), len(c0.getIndexSet()) + len(sp)
    masks = [R._encode(ea, rng.integers(0, 2, ea.size()))[0] for _ in range(4)]
    kernel = {}
    for n in (1, 2):
        ks = [z.genToPow(0, 1), z.genToPow(0, ea.sizeOfDimension(0) - 1)][:n]
        Ws = [pre.ctxt.ksw_auto[k] for k in ks]
        A, Bm = masks[:n], masks[2:2 + n]

        def fused():
            o0, o1 = capi.hoistedMaskFan(dg, c0, c1, ks, Ws, A, Bm, sp)
            return o0 + o1

        def sequence():
            o0, o1 = [], []
            for t in range(n):
                d2, p0 = dg.copy(), c0.copy()
                d2.automorph(ks[t])
                p0.automorph(ks[t])
                p0.addPrimesAndScale(sp)
                p1 = capi.zerosLike(p0)
                capi.keySwitchDigits(d2, Ws[t], p0, p1)
                p0 *= Bm[t]
                p1 *= Bm[t]
                a0, a1 = c0.copy(), c1.copy()
                a0 *= A[t]
                a1 *= A[t]
                a0.addPrimesAndScale(sp)
                a1.addPrimesAndScale(sp)
                a0 += p0
                a1 += p1
                o0.append(a0)
                o1.append(a1)
            return o0 + o1
        tn, to, ok = [], [], True
        for rep in range(a.reps + 1):                # the first pair warms tables and buffers
            ms_n, yn = device_ms(fused)
            ms_o, yo = device_ms(sequence)
            ok = ok and bool(all(np.array_equal(p.download(), q.download()) for p, q in zip(yn, yo)))
            if rep:
                tn.append(ms_n)
                to.append(ms_o)
        r = {"n": n, "ndig": ndig, "rows": rows,
             "fused_ms": round(statistics.median(tn), 4), "sequence_ms": round(statistics.median(to), 4),
             "fused_runs_ms": runs(tn), "sequence_runs_ms": runs(to),
             "fused_over_sequence": round(statistics.median(tn) / statistics.median(to), 3),
             "fused_faster_in_every_pair": bool(all(x < y for x, y in zip(tn, to))), "same_words": ok}
        kernel["n%d" % n] = r
        note("kernel, n =", n, r)
    del pre, dg, masks

    # ---- (b) ----
    forms = {"reference": dict(hoisted=False), "hoisted_calls": dict(hoisted=True, fused=False),
             "hoisted_kernel": dict(hoisted=True, fused=True)}
    aux = {name: R.RepAuxDim() for name in forms}     # the masks are encoded in the warm round
    times = {name: [] for name in forms}
    last, same = {}, True
    for rep in range(a.reps + 1):
        for name, kw in forms.items():
            ms, last[name] = wall(lambda: run(ea, ct, aux[name], **kw))
            if rep:
                times[name].append(ms)
        same = same and all(same_ctxt(x, y) for x, y in zip(last["hoisted_calls"], last["hoisted_kernel"]))
    whole = {"same_words_and_bookkeeping_calls_kernel": bool(same), "outputs": len(last["reference"])}
    for name in forms:
        ok, caps = checked(ea, sk, v, last[name])
        whole.update({name + "_ms": round(statistics.median(times[name]), 3), name + "_runs_ms": runs(times[name]),
                      name + "_all_correct": ok, name + "_bitCapacity": caps, name + "_least_capacity": min(caps)})
    whole["kernel_faster_than_calls_in_every_pair"] = bool(all(x < y for x, y in zip(times["hoisted_kernel"], times["hoisted_calls"])))
    whole["calls_faster_than_reference_in_every_pair"] = bool(all(x < y for x, y in zip(times["hoisted_calls"], times["reference"])))
    whole["kernel_faster_than_reference_in_every_pair"] = bool(all(x < y for x, y in zip(times["hoisted_kernel"], times["reference"])))
    whole["calls_over_reference"] = round(whole["hoisted_calls_ms"] / whole["reference_ms"], 3)
    whole["kernel_over_reference"] = round(whole["hoisted_kernel_ms"] / whole["reference_ms"], 3)
    whole["kernel_over_calls"] = round(whole["hoisted_kernel_ms"] / whole["hoisted_calls_ms"], 3)
    deepest = int(np.argmin(whole["reference_bitCapacity"]))
    whole["deepest_output"] = deepest
    whole["capacity_loss_at_deepest"] = {name: whole["reference_bitCapacity"][deepest] - whole[name + "_bitCapacity"][deepest]
                                         for name in ("hoisted_calls", "hoisted_kernel")}
    note("replicateAll", whole)
    right = all(whole[name + "_all_correct"] for name in forms)
    fan_wins = bool(right and all(r["fused_faster_in_every_pair"] and r["same_words"] for r in kernel.values()) and
                    whole["kernel_faster_than_calls_in_every_pair"] and same)
    best = "hoisted_kernel" if fan_wins else "hoisted_calls"
    hoist_wins = bool(right and whole[("kernel" if fan_wins else "calls") + "_faster_than_reference_in_every_pair"] and
                      whole["capacity_loss_at_deepest"][best] <= 2)
    dims = [(ea.sizeOfDimension(i), bool(ea.nativeDimension(i))) for i in range(ea.dimension())]
    out = {"tool": "bench_replicate", "m": m, "p": 2, "phim": g.phim, "nslots": ea.size(), "d": ea.getDegree(), "dims": dims,
           "bits": bits, "bits_search": search, "fresh_capacity": fresh_capacity, "batch": B, "recBound": a.recBound,
           "reps": a.reps, "inner": a.inner, "hoisted_mask_fan": kernel, "replicate_all": whole,
           "hoisted_mask_fan_faster_in_every_pair": fan_wins, "hoisted_form_qualifies": hoist_wins,
           "fuseHoistedFan_default": bool(hc.Ctxt.fuseHoistedFan), "hoistNodes_default": bool(R.hoistNodes)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
