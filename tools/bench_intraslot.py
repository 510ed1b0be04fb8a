#!/usr/bin/env python3
"""unpack (src/intraSlot.cpp:78-117) at the ring the other slot tools use -- m = 21845, p = 2: d = 16, 1024 slots,
bits = 950, batch 32 -- at r = 1 and at one r > 1 (p^r = 4, Galois-ring slots), fused against unfused in one process:

  (a) the d^2 multiply-adds alone: Ctxt.circulantCombination(fused=True) -- one hx_mul_add_circulant --
      against fused=False, the reference's call sequence (per output and term a copy, a product by a constant and an
      add), on the same d Frobenius images; wall clock around calls that end in a synchronise, the two sides alternated,
      --reps pairs after one warm pair
  (b) the whole unpack (the d Frobenius automorphisms with their key switches included) with fused=True against
      fused=False, alternated the same way: the figure that decides whether Ctxt.fuseCirculant may become True (only if
      fused wins every pair)
  (c) the kernel alone: capi.mulAddCirculant on the same operands, bytes/s against its algorithmic bytes
      8 N rows batch (nb (PARTS d + d + OB - 1) + PARTS nout), nb = ceil(nout / OB)

Both sides of every pair are checked to give the same words and bookkeeping, and the unpacked ciphertexts to decrypt to
unpackPlain.  Writes profiles/intraslot.json (--out) and prints the same JSON line.

  python tools/bench_intraslot.py          # MI355X
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


def case(a, p, r):
    from helib_amd import bgv_gf, bgv_gr, capi, ctxt as hc, intraslot, keys as hk
    m, B = a.m, a.batch
    P = p ** r
    cc = hc.ChainContext(m, p, r, bits=a.bits, c=3)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey()
    ea = (bgv_gf if r == 1 else bgv_gr).EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    n, d = ea.size(), ea.getDegree()
    (hk.addFrbMatrices if d <= 8 else hk.addMinimalFrbMatrices)(sk)
    v = np.random.default_rng(1).integers(0, P, size=(B, n, d))
    ct = ea.encrypt_batch(sk, v)
    enc = intraslot.buildUnpackSlotEncoding(ea)

    def wall(fn):
        g.sync()
        t0 = time.perf_counter()
        out = fn()
        for c in out:
            c.lnNoise  # noqa: B018 -- completes the deferred norms
        g.sync()
        return (time.perf_counter() - t0) * 1e3, out

    def same(xs, ys):
        return bool(len(xs) == len(ys) and all(
            x.primeSet == y.primeSet and x.intFactor == y.intFactor and x.lnNoise == y.lnNoise and x.ptxtSpace == y.ptxtSpace
            and x.ptxtMag == y.ptxtMag and all(np.array_equal(x.parts[h].download(), y.parts[h].download()) for h in x.parts)
            for x, y in zip(xs, ys)))

    def pairs(fn):
        tf, tu, ok = [], [], True
        for k in range(a.reps + 1):                  # the first pair warms tables and buffers
            ms_f, yf = wall(lambda: fn(True))
            ms_u, yu = wall(lambda: fn(False))
            if k == 0:
                ok = same(yf, yu)
            else:
                tf.append(ms_f)
                tu.append(ms_u)
        return tf, tu, ok, yf

    # ---- (a) the multiply-adds on fixed Frobenius images ----
    frob = []
    for j in range(d):
        f = ct.clone()
        f.frobeniusAutomorph(j)
        f.cleanUp()
        frob.append(f)
    primes = sorted(frozenset().union(*[f.primeSet for f in frob]))
    consts = [ea.enc.encode(e.v, 1, primes) for e in enc]
    one_set = len({f.primeSet for f in frob}) == 1
    cf, cu, c_ok, _ = pairs(lambda fz: hc.Ctxt.circulantCombination(frob, consts, d, fused=fz))

    # ---- (b) the whole unpack ----
    uf, uu, u_ok, y = pairs(lambda fz: intraslot.unpack(ea, ct, enc, fused=fz))
    want = intraslot.unpackPlain(ea, v)
    correct = True
    for i in (0, d - 1):
        got = ea.decrypt_batch(y[i], sk)
        correct = correct and bool(np.array_equal(got[:, :, 0], want[:, :, i]) and not np.any(got[:, :, 1:]))

    # ---- (c) the kernel alone ----
    out = {"p": p, "r": r, "d": d, "nslots": n, "frobenius_images_on_one_prime_set": one_set}
    if one_set:
        rows = len(frob[0].parts["1"].getIndexSet())
        o0 = [capi.likeUninit(frob[0].parts["1"]) for _ in range(d)]
        o1 = [capi.likeUninit(frob[0].parts["s"]) for _ in range(d)]
        in0, in1 = [f.parts["1"] for f in frob], [f.parts["s"] for f in frob]
        ks = []
        for k in range(a.reps * 4 + 1):
            g.sync()
            t0 = time.perf_counter()
            capi.mulAddCirculant(o0, o1, consts, in0, in1)
            g.sync()
            if k:
                ks.append((time.perf_counter() - t0) * 1e3)
        ob = 4 if d <= 4 else 8
        nb = -(-d // ob)
        algo = 8 * g.phim * rows * B * (nb * (2 * d + d + ob - 1) + 2 * d)
        replaced = 8 * g.phim * rows * B * d * d * 2 * 8          # per part and term: copy 1r 1w, product 2r 1w, add 2r 1w
        kms = statistics.median(ks)
        out.update({"kernel_rows": rows, "kernel_output_block": ob, "kernel_ms": round(kms, 3),
                    "kernel_runs_ms": [round(x, 3) for x in ks], "kernel_algorithmic_bytes": algo,
                    "kernel_algorithmic_GBps": round(algo / kms / 1e6, 1), "sequence_algorithmic_bytes": replaced})
    out.update({
        "muladd_fused_ms": round(statistics.median(cf), 3), "muladd_sequence_ms": round(statistics.median(cu), 3),
        "muladd_fused_runs_ms": [round(x, 3) for x in cf], "muladd_sequence_runs_ms": [round(x, 3) for x in cu],
        "muladd_fused_over_sequence": round(statistics.median(cf) / statistics.median(cu), 3),
        "muladd_fused_faster_in_every_pair": bool(all(x < y for x, y in zip(cf, cu))), "muladd_same_words_and_fields": c_ok,
        "unpack_fused_ms": round(statistics.median(uf), 2), "unpack_unfused_ms": round(statistics.median(uu), 2),
        "unpack_fused_runs_ms": [round(x, 2) for x in uf], "unpack_unfused_runs_ms": [round(x, 2) for x in uu],
        "unpack_fused_over_unfused": round(statistics.median(uf) / statistics.median(uu), 3),
        "unpack_fused_faster_in_every_pair": bool(all(x < y for x, y in zip(uf, uu))), "unpack_same_words_and_fields": u_ok,
        "unpack_correct": correct, "unpack_capacity": round(y[0].capacity(), 1),
    })
    return out, g.phim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=21845)
    ap.add_argument("--bits", type=int, default=950)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="2:1,2:2", help="p:r, comma separated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intraslot.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import ctxt as hc
    cases, phim = [], 0
    for spec in a.cases.split(","):
        p, r = (int(x) for x in spec.split(":"))
        res, phim = case(a, p, r)
        cases.append(res)
    out = {"tool": "bench_intraslot", "m": a.m, "phim": phim, "bits": a.bits, "batch": a.batch, "reps": a.reps,
           "fused_default": bool(hc.Ctxt.fuseCirculant), "cases": cases}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
