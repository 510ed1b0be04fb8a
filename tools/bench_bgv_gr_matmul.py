#!/usr/bin/env python3
"""The constants of one BlockMatMul1DExec over Galois-ring slots (helib_amd.bgv_gr_matmul) at the ring the other slot
tools use -- m = 21845, p = 2, r = 2: d = 16, 1024 slots, bits = 950 -- formed three ways in one process:

  host     numpy gathers and twists, ea.enc.encode uploads                    (device_diagonals=False)
  device   bgv_gf_gather_kernel, the slot arrays hop to the host and back into ea.enc.encode   (today's form)
  fused    hx_bgv_gf_encode_gathered: bgv_gf_gather_map_kernel feeds the encode on the device   (fused=True)

The matrix is uploaded (and its linearized-polynomial coefficients formed) once, ahead of the clock, for the two device
paths.  Wall clock around constructions that end in a synchronise; fused and device are alternated, --reps pairs after
one warm pair, and the host path is timed once per pair beside them.  The comparison that decides whether
BlockMatMul1DExec.fuseConstants may become True is fused against device on the same commit and the same box: only if
fused wins every pair.  All three are checked to give the same words and sizes; one mul is timed and checked against
mulPlain.  Writes profiles/bgv_gr_matmul.json (--out) and prints the same JSON line.

  python tools/bench_bgv_gr_matmul.py          # MI355X
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
    ap.add_argument("--r", type=int, default=2)
    ap.add_argument("--bits", type=int, default=950)
    ap.add_argument("--dim", type=int, default=1, help="the dimension of the matrix (at m = 21845: D = 8, non-native)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgv_gr_matmul.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import bgv_gr, bgv_gr_matmul as RM, capi, ctxt as hc, keys as hk
    m, p, r = a.m, a.p, a.r
    P = p ** r
    cc = hc.ChainContext(m, p, r, bits=a.bits, c=3)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey()
    ea = bgv_gr.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    n, d = ea.size(), ea.getDegree()
    if d <= 8:
        hk.addSome1DMatrices(sk)
        hk.addFrbMatrices(sk)
    else:
        hk.addMinimal1DMatrices(sk)
        hk.addMinimalFrbMatrices(sk)
    D = ea.sizeOfDimension(a.dim)
    rng = np.random.default_rng(1)
    mat = RM.BlockMatMul1D(ea, rng.integers(0, P, size=(D, D, d, d)), a.dim)

    def wall(fn):
        g.sync()
        t0 = time.perf_counter()
        out = fn()
        g.sync()
        return (time.perf_counter() - t0) * 1e3, out

    ms_matrix, _ = wall(lambda: mat.handle(ea.enc))

    def same(x, y):
        lists = [("vec", x.vec, y.vec)] + ([("vec1", x.vec1, y.vec1)] if x.vec1 is not None else [])
        return bool(all(len(u) == len(w) and all((s is None) == (t is None) and (s is None or (
            s[1] == t[1] and np.array_equal(s[0].download(), t[0].download()))) for s, t in zip(u, w)) for _, u, w in lists))

    tf, td, th, ok = [], [], [], True
    for k in range(a.reps + 1):                      # the first pair warms tables and buffers
        ms_f, xf = wall(lambda: RM.BlockMatMul1DExec(ea, mat, fused=True))
        ms_d, xd = wall(lambda: RM.BlockMatMul1DExec(ea, mat, fused=False))
        ms_h, xh = wall(lambda: RM.BlockMatMul1DExec(ea, mat, device_diagonals=False))
        if k == 0:
            ok = same(xf, xd) and same(xd, xh)
        else:
            tf.append(ms_f)
            td.append(ms_d)
            th.append(ms_h)
    live = sum(c is not None for lst in (xd.vec, xd.vec1 or []) for c in lst)
    v = rng.integers(0, P, size=(1, n, d))
    ct = ea.encrypt_batch(sk, v)
    ms_mul, _ = wall(lambda: xd.mul(ct, pk=sk))
    correct = bool(ct.isCorrect() and np.array_equal(ea.decrypt_batch(ct, sk), RM.mulPlain(ea, v, mat)))
    wins = bool(all(x < y for x, y in zip(tf, td)))
    out = {"tool": "bench_bgv_gr_matmul", "m": m, "p": p, "r": r, "phim": g.phim, "bits": a.bits, "d": d, "nslots": n, "dim": a.dim,
           "D": D, "native": bool(xd.native), "strategy": xd.strategy, "constants": live, "rows_per_constant": len(cc.ctxtPrimes) +
           len(cc.specialPrimes), "reps": a.reps, "matrix_upload_and_linpoly_ms": round(ms_matrix, 2),
           "construct_fused_ms": round(statistics.median(tf), 2), "construct_device_ms": round(statistics.median(td), 2),
           "construct_host_ms": round(statistics.median(th), 2),
           "construct_fused_runs_ms": [round(x, 2) for x in tf], "construct_device_runs_ms": [round(x, 2) for x in td],
           "construct_host_runs_ms": [round(x, 2) for x in th],
           "fused_over_device": round(statistics.median(tf) / statistics.median(td), 3),
           "fused_faster_in_every_pair": wins, "same_words_and_sizes": ok, "mul_ms": round(ms_mul, 2), "mul_correct": correct,
           "fused_default": bool(RM.BlockMatMul1DExec.fuseConstants)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
