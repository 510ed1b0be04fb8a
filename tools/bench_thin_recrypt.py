#!/usr/bin/env python3
"""Thin recryption (helib_amd.recryption.thinReCrypt) beside the packed reCrypt, and the hoisted sum of traceMap in one
device call (hx_hoisted_automorph_sum) against the loop it replaces, at the row of tools/bench_recrypt.py:
m = 21845, p = 2, r = 1, mvec (17, 5, 257), d = 16, a bootstrappable chain with c = 3, batch 32.  One process, one key:
minimal 1D matrices and all the Frobenius matrices (keys.addFrbMatrices: HELIB_KSS_FULL, the strategy under which
traceMap hoists).

  thinReCrypt   on a batch of thinly packed slots whose capacity has been used up: the time per phase (the reference's
                named timers AAA_slotToCoeff, AAA_bootKeySwitch, AAA_coeffToSlot, AAA_extractDigitsThin), the capacity
                before and after, and whether the slots came back
  reCrypt       the packed form on the same input, per phase (AAA_preProcess, AAA_LinearTransform1,
                AAA_extractDigitsPacked, AAA_LinearTransform2)
  hoisted sum   BasicAutomorphPrecon(ct).automorphSum of p^1 .. p^(d-1), fused=True against fused=False, in alternated
                pairs on one digit block; the words of every pair are compared (same_words)

Wall clock around calls that end in a synchronise; one warm run, then --reps.  Ctxt.fuseHoistedSum goes to True only if
the fused side wins every pair here.  Writes profiles/thin_recrypt.json (--out) and prints the same JSON line.

  python tools/bench_thin_recrypt.py          # MI355X
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
    ap.add_argument("--r", type=int, default=1)
    ap.add_argument("--mvec", type=int, nargs="+", default=[17, 5, 257])
    ap.add_argument("--gens", type=int, nargs="+", default=[8996, 17477, 21591])
    ap.add_argument("--ords", type=int, nargs="+", default=[16, 4, -16])
    ap.add_argument("--bits", type=int, default=400)        # profiles/recrypt.json: the smallest at which reCrypt held
    ap.add_argument("--bits-max", type=int, default=600)    # up to here in steps of 100, until thinReCrypt gives the slots back
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thin_recrypt.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    out = None
    for bits in range(a.bits, max(a.bits, a.bits_max) + 1, 100):
        out = measure(a, bits)
        if out["thin"].get("correct") and out["thin"].get("same_slots"):
            break
    line = json.dumps(out, default=lambda o: o.item() if hasattr(o, "item") else str(o))   # (numpy scalars)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


def measure(a, bits):
    from helib_amd import capi, ctxt as hc, keys as hk, recryption as RC, thin_evalmap as TE, timing
    m, p, r, B = a.m, a.p, a.r, a.batch
    cc = hc.ChainContext(m, p, r, bits=bits, c=3, bootstrappable=True)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    rc = RC.ThinRecryptData(cc, g, a.mvec, gens=a.gens, ords=a.ords, alsoThick=True)
    ea = rc.ea
    d = ea.getDegree()
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey()
    sk.zMStar = ea.zMStar
    hk.addMinimal1DMatrices(sk)
    hk.addFrbMatrices(sk)
    sk.genRecryptData(rc)
    v = np.random.default_rng(1).integers(0, p ** r, size=(B, ea.size()))
    want, ct = ea._slots(v), ea.encrypt_batch(sk, v)
    while ct.bitCapacity() > 60:
        ct.multiplyBy(ea.encrypt_batch(sk, v))
        want = ea.mulPlain(want, v)
    before = ct.bitCapacity()

    def run(fn, names):
        """one warm run, one timed -> (ms, {timer: ms}, capacity after, correct, slots came back)"""
        out = None
        for k in range(2):
            x = ct.clone()
            timing.resetAllTimers()
            g.sync()
            t0 = time.perf_counter()
            try:
                fn(x, sk, rc, seed=7)
            except RC.LogicError as ex:
                return {"ms": None, "why": str(ex)[:80]}
            g.sync()
            ms = (time.perf_counter() - t0) * 1e3
            out = {"ms": round(ms, 2), "phases_ms": {n: round(timing.getTimerByName(n).counter * 1e3, 2) for n in names},
                   "capacity_after": x.bitCapacity(), "correct": bool(x.isCorrect()),
                   "same_slots": bool(np.array_equal(ea.decrypt_batch(x, sk), want)), "why": ""}
            print("run %d: %s" % (k, out), file=sys.stderr, flush=True)
        return out
    thin = run(RC.thinReCrypt, ("AAA_slotToCoeff", "AAA_bootKeySwitch", "AAA_coeffToSlot", "AAA_extractDigitsThin"))
    branch = TE.traceMap.last
    thick = run(RC.reCrypt, ("AAA_preProcess", "AAA_LinearTransform1", "AAA_extractDigitsPacked", "AAA_LinearTransform2"))

    # the hoisted sum on one digit block, fused against the loop
    x = ea.encrypt_batch(sk, v)
    x.multiplyBy(ea.encrypt_batch(sk, v))
    precon = hc.BasicAutomorphPrecon(x)
    ks = [ea.zMStar.genToPow(-1, i) for i in range(1, d)]

    def wall(fused):
        g.sync()
        t0 = time.perf_counter()
        out = precon.automorphSum(ks, fused=fused)
        g.sync()
        return (time.perf_counter() - t0) * 1e3, out
    t_f, t_l, same = [], [], True
    for k in range(a.reps + 1):                      # the first pair warms buffers
        ms_f, zf = wall(True)
        ms_l, zl = wall(False)
        same = same and all(np.array_equal(zf.parts[h].download(), zl.parts[h].download()) for h in ("1", "s")) \
            and (zf.lnNoise, zf.primeSet) == (zl.lnNoise, zl.primeSet)
        print("pair %d: fused %.3f ms, loop %.3f ms, same words %s" % (k, ms_f, ms_l, same), file=sys.stderr, flush=True)
        if k:
            t_f.append(ms_f)
            t_l.append(ms_l)
    rows = len(precon.polyDigits.getIndexSet()) // len(precon.digits)
    return {"tool": "bench_thin_recrypt", "m": m, "p": p, "r": r, "mvec": list(a.mvec), "phim": g.phim, "bits": bits, "batch": B,
            "d": d, "nslots": ea.size(), "e": rc.e, "ePrime": rc.ePrime, "capacity_before": before, "trace_branch": branch,
            "thin": thin, "packed": thick,
            "hoisted_terms": len(ks), "hoisted_digits": len(precon.digits), "hoisted_rows": rows, "reps": a.reps,
            "hoisted_fused_ms": round(statistics.median(t_f), 3), "hoisted_loop_ms": round(statistics.median(t_l), 3),
            "hoisted_fused_runs_ms": [round(t, 3) for t in t_f], "hoisted_loop_runs_ms": [round(t, 3) for t in t_l],
            "same_words": bool(same), "fused_wins_every_pair": bool(all(f < l for f, l in zip(t_f, t_l)))}


if __name__ == "__main__":
    main()
