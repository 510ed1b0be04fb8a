#!/usr/bin/env python3
"""polyEval at the flagship ring (m = 21845) with plaintext space 127^2, in one process:

  (a) hx_lin_comb against the call sequence it replaces -- per term a copy, the mod-up, the products by a
      scalar and the add, then the constant -- as Ctxt.linearCombination(fused=True / False) over the first --terms
      powers of one ciphertext (they sit on different prime sets) with the digit polynomial's low coefficients: wall
      clock around calls that end in a synchronise, the two sides alternated, --reps pairs after one warm pair
  (b) one polyEval of the digit polynomial of 127^2 (degree 127: k = 8 baby steps, n = 16) with fused=True against
      fused=False, alternated, wall clock; the products dominate, so this is the figure that decides whether
      Ctxt.fuseLinComb may become True (only if fused wins every pair)

Both sides of every pair are checked to give the same words.  Writes profiles/polyeval.json (--out) and prints the same
JSON line.

  python tools/bench_polyeval.py          # MI355X
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
    ap.add_argument("--p", type=int, default=127)
    ap.add_argument("--r", type=int, default=2)
    ap.add_argument("--bits", type=int, default=600)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--terms", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polyeval.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import bgv_pr, capi, ctxt as hc, keys as hk, polyeval
    m, p, r, B = a.m, a.p, a.r, a.batch
    P = p ** r
    cc = hc.ChainContext(m, p, r, bits=a.bits, c=3)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey()
    ea = bgv_pr.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    n = ea.size()
    v = np.random.default_rng(1).integers(0, P, size=(B, n))
    ct = ea.encrypt_batch(sk, v)
    poly = polyeval.buildDigitPolynomial(p, r)

    def wall(fn):
        g.sync()
        t0 = time.perf_counter()
        out = fn()
        out.lnNoise  # noqa: B018 -- completes the deferred norms
        g.sync()
        return (time.perf_counter() - t0) * 1e3, out

    def same(x, y):
        return bool(x.primeSet == y.primeSet and x.intFactor == y.intFactor and x.lnNoise == y.lnNoise and all(
            np.array_equal(x.parts[h].download(), y.parts[h].download()) for h in x.parts))

    def pairs(fn):
        tf, tu, ok = [], [], True
        for k in range(a.reps + 1):                  # the first pair warms tables and buffers
            ms_f, yf = wall(lambda: fn(True))
            ms_u, yu = wall(lambda: fn(False))
            ok = ok and same(yf, yu)
            if k:
                tf.append(ms_f)
                tu.append(ms_u)
        return tf, tu, ok, yf

    # ---- (a) ----
    pw = hc.DynamicCtxtPowers(ct, a.terms)
    bal = lambda c: c % P - P if c % P > P // 2 else c % P      # noqa: E731
    terms = [(pw.getPower(i), bal(poly[i]) or 1) for i in range(1, a.terms + 1)]
    sets = len({t.primeSet for t, _ in terms})
    lf, lu, l_ok, y = pairs(lambda fz: hc.Ctxt.linearCombination(terms, 5, fused=fz))
    rows = len(y.primeSet)

    # ---- (b) ----
    st = {}
    polyeval.polyEval(ct, poly, stats=st)
    ef, eu, e_ok, y = pairs(lambda fz: polyeval.polyEval(ct, poly, fused=fz))
    got = ea.decrypt_batch(y, sk)
    want = np.array([[sum(c * pow(int(x), i, P) for i, c in enumerate(poly)) % P for x in row] for row in v])

    out = {
        "tool": "bench_polyeval", "m": m, "p": p, "r": r, "phim": g.phim, "nslots": n, "bits": a.bits, "batch": B,
        "reps": a.reps, "terms": a.terms, "term_prime_sets": sets, "output_rows": rows,
        "lin_comb_fused_ms": round(statistics.median(lf), 3), "lin_comb_sequence_ms": round(statistics.median(lu), 3),
        "lin_comb_fused_runs_ms": [round(x, 3) for x in lf], "lin_comb_sequence_runs_ms": [round(x, 3) for x in lu],
        "lin_comb_fused_over_sequence": round(statistics.median(lf) / statistics.median(lu), 3),
        "lin_comb_fused_faster_in_every_pair": bool(all(x < y for x, y in zip(lf, lu))), "lin_comb_same_words": l_ok,
        "polyEval_degree": len(poly) - 1, "polyEval_products": st["mults"], "polyEval_leaves": st["leaves"],
        "polyEval_fused_ms": round(statistics.median(ef), 1), "polyEval_unfused_ms": round(statistics.median(eu), 1),
        "polyEval_fused_runs_ms": [round(x, 1) for x in ef], "polyEval_unfused_runs_ms": [round(x, 1) for x in eu],
        "polyEval_fused_faster_in_every_pair": bool(all(x < y for x, y in zip(ef, eu))), "polyEval_same_words": e_ok,
        "polyEval_correct": bool(np.array_equal(got, want)), "polyEval_capacity": round(y.capacity(), 1),
        "fused_default": bool(hc.Ctxt.fuseLinComb),
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
