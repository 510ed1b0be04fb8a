#!/usr/bin/env python3
"""Slots modulo p^r at the flagship ring (m = 21845, p = 2, r = 8: 1024 slots mod 256), in one process:

  (a) encode (hx_bgv_crt_encode through the p^r tables, onto the ctxt primes) and decrypt_batch of a batch: wall clock
      around calls that end in a synchronise, the median of --reps runs after one warm run; the table build once
  (b) hx_scaled_sub (c = c*u - t*v) against the sequence it replaces -- hx_mul_scalar, hx_poly_copy,
      hx_mul_scalar, hx_sub per part -- on the same two-part operands at the full ctxt prime set: device time between
      two events on the context's stream around --inner calls, the two sides alternated, --reps runs each
  (c) extractDigits(ea, ct, --digits) with fused=True against fused=False, alternated, wall clock; the squares dominate,
      so this is the figure that decides whether Ctxt.fuseScaledSub may become True (only if fused wins every pair)

Writes profiles/bgv_pr.json (--out) and prints the same JSON line.

  python tools/bench_bgv_pr.py          # MI355X
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
    ap.add_argument("--r", type=int, default=8)
    ap.add_argument("--bits", type=int, default=600)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--digits", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgv_pr.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import bgv_pr, capi, ctxt as hc, keys as hk
    m, p, r, B = a.m, a.p, a.r, a.batch
    P = p ** r
    cc = hc.ChainContext(m, p, r, bits=a.bits, c=3)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey()
    t0 = time.perf_counter()
    ea = bgv_pr.EncryptedArray(cc, g)
    build_s = time.perf_counter() - t0
    sk.zMStar = ea.zMStar
    n = ea.size()
    v = np.random.default_rng(1).integers(0, P, size=(B, n))

    def wall(fn, reps):
        times, out = [], None
        for k in range(reps + 1):                    # the first run warms tables and buffers
            g.sync()
            t0 = time.perf_counter()
            out = fn()
            g.sync()
            if k:
                times.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(times), times, out

    # ---- (a) ----
    idx = list(cc.ctxtPrimes)
    enc_ms, _, _ = wall(lambda: ea.encode(v, idx), a.reps)
    ct = ea.encrypt_batch(sk, v)
    dec_ms, _, got = wall(lambda: ea.decrypt_batch(ct, sk), a.reps)
    roundtrip_ok = bool(np.array_equal(got, v))
    L = len(sorted(ct.primeSet))

    # ---- (b) ----
    wc, wt = ct.clone(), ea.encrypt_batch(sk, v)
    c = [wc.parts["1"], wc.parts["s"]]
    t = [wt.parts["1"], wt.parts["s"]]
    qs = [cc.primes[i] for i in c[0].getIndexSet()]
    u = [pow(p, -1, q) for q in qs]
    w = [(q - 3) * pow(p, -1, q) % q for q in qs]
    lib = capi.lib()

    def fused():
        capi.scaledSub(c[0], c[1], t[0], t[1], u, w)

    def four():
        for x, y in zip(c, t):
            x.mulConstant(u)
            y2 = y.copy()
            y2.mulConstant(w)
            capi._chk(lib.hx_sub(x.h, y2.h))

    def device_ms(fn):
        g.sync()
        g.timerBegin()
        for _ in range(a.inner):
            fn()
        return g.timerEnd() / a.inner
    for fn in (fused, four):
        fn()
    tf, t4 = [], []
    for _ in range(a.reps):
        tf.append(device_ms(fused))
        t4.append(device_ms(four))
    sub_ms, four_ms = statistics.median(tf), statistics.median(t4)
    word_bytes = 2 * L * B * g.phim * 8             # one pass over both parts

    # ---- (c) ----
    def run(fz):
        d = bgv_pr.extractDigits(ea, ct, a.digits, fused=fz)
        d[-1].lnNoise  # noqa: B018 -- completes the deferred norms
        return d
    xf, xu, df, du = [], [], None, None
    run(True)
    run(False)
    for _ in range(a.reps):
        ms, _, df = wall(lambda: run(True), 1)
        xf.append(ms)
        ms, _, du = wall(lambda: run(False), 1)
        xu.append(ms)
    digits_ok = bool(all(np.array_equal(ea.decrypt_batch(d, sk) % p, (v >> j) & 1) for j, d in enumerate(df))
                     and all(np.array_equal(ea.decrypt_batch(d, sk) % p, (v >> j) & 1) for j, d in enumerate(du))) if p == 2 else None

    out = {
        "tool": "bench_bgv_pr", "m": m, "p": p, "r": r, "phim": g.phim, "nslots": n, "d": ea.getDegree(),
        "bits": a.bits, "L": L, "batch": B, "reps": a.reps, "inner": a.inner, "digits": len(df),
        "table_bytes": ea.enc.table.table_bytes, "tables_build_s": round(build_s, 2),
        "encode_ms": round(enc_ms, 3), "decrypt_batch_ms": round(dec_ms, 3), "roundtrip_correct": roundtrip_ok,
        "scaled_sub_ms": round(sub_ms, 4), "four_calls_ms": round(four_ms, 4),
        "scaled_sub_over_sequence": round(sub_ms / four_ms, 3), "byte_model_ratio": round(3 / 9, 3),
        "scaled_sub_faster_in_every_pair": bool(all(x < y for x, y in zip(tf, t4))),
        "scaled_sub_GBps": round(3 * word_bytes / sub_ms / 1e6, 1), "four_calls_GBps": round(9 * word_bytes / four_ms / 1e6, 1),
        "scaled_sub_runs_ms": [round(x, 4) for x in tf], "four_calls_runs_ms": [round(x, 4) for x in t4],
        "extractDigits_fused_ms": round(statistics.median(xf), 1), "extractDigits_unfused_ms": round(statistics.median(xu), 1),
        "extractDigits_fused_runs_ms": [round(x, 1) for x in xf], "extractDigits_unfused_runs_ms": [round(x, 1) for x in xu],
        "extractDigits_fused_faster_in_every_pair": bool(all(x < y for x, y in zip(xf, xu))),
        "extractDigits_correct": digits_ok, "last_digit_capacity": round(df[-1].capacity(), 1),
        "fused_default": bool(hc.Ctxt.fuseScaledSub),
    }
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
