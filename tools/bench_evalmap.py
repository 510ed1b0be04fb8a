#!/usr/bin/env python3
"""EvalMap and the powerful basis (helib_amd.evalmap, helib_amd.powerful) at the ring the other slot tools use, with the
hypercube the reference's bootstrapping parameters choose for it: m = 21845 = 17 * 5 * 257, p = 2, r = 2, mvec (17, 5,
257), gens (8996, 17477, 21591), ords (16, 4, -16): d = 16, 1024 slots, bits = 950, batch 32.  In one process:

  construct   EvalMap forward and inverse: the matrices (numpy) and the execs with their encoded constants (fused path)
  apply       forward on an encrypted batch of powerful cubes, inverse on the result; decrypted and checked against
              applyPlain, and the round trip against the cubes
  powerful    both conversions on the coefficient rows of one ciphertext part: powerful_kernel on the device
              (hx_poly_to_powerful / hx_powerful_to_poly, the rows stay where they are) against the numpy form of
              helib_amd.powerful on the same rows downloaded (row by row modulo the row's prime; transfers not timed)

Wall clock around calls that end in a synchronise; the device path and the numpy form are alternated, --reps rounds after
one warm round.  No default depends on these numbers.  Writes profiles/evalmap.json (--out) and prints the same JSON line.

  python tools/bench_evalmap.py          # MI355X
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
    ap.add_argument("--mvec", type=int, nargs="+", default=[17, 5, 257])
    ap.add_argument("--gens", type=int, nargs="+", default=[8996, 17477, 21591])
    ap.add_argument("--ords", type=int, nargs="+", default=[16, 4, -16])
    ap.add_argument("--bits", type=int, default=950)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evalmap.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import bgv_gr, capi, ctxt as hc, evalmap, keys as hk, powerful as PW
    m, p, r, mvec, B = a.m, a.p, a.r, list(a.mvec), a.batch
    P = p ** r
    cc = hc.ChainContext(m, p, r, bits=a.bits, c=3)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey()
    ea = bgv_gr.EncryptedArray(cc, g, gens=a.gens, ords=a.ords)
    sk.zMStar = ea.zMStar
    n, d = ea.size(), ea.getDegree()
    if d <= 8:
        hk.addSome1DMatrices(sk)
        hk.addFrbMatrices(sk)
    else:
        hk.addMinimal1DMatrices(sk)
        hk.addMinimalFrbMatrices(sk)

    def wall(fn):
        g.sync()
        t0 = time.perf_counter()
        out = fn()
        g.sync()
        return (time.perf_counter() - t0) * 1e3, out

    rng = np.random.default_rng(1)
    conv = PW.PowerfulConversion(mvec)
    F = rng.integers(0, P, size=(B, n * d))
    cube = conv.polyToPowerful(F, P).reshape(B, n, d)

    def note(*x):
        print(*x, file=sys.stderr, flush=True)

    note("keys and tables ready: d = %d, %d slots" % (d, n))
    t_fw, t_inv, t_afw, t_ainv, correct = [], [], [], [], True
    for k in range(a.reps + 1):                      # the first round warms tables and buffers
        ms_fw, fw = wall(lambda: evalmap.EvalMap(ea, mvec).upgrade())
        ms_inv, inv = wall(lambda: evalmap.EvalMap(ea, mvec, invert=True).upgrade())
        ct = ea.encrypt_batch(sk, cube)
        ms_afw, _ = wall(lambda: fw.apply(ct, pk=sk))
        ok = bool(ct.isCorrect())
        slots = ea.decrypt_batch(ct, sk)
        ok = ok and np.array_equal(slots, fw.applyPlain(cube))
        ct = ea.encrypt_batch(sk, slots)             # a fresh encryption: each direction is timed from the same level
        ms_ainv, _ = wall(lambda: inv.apply(ct, pk=sk))
        ok = ok and bool(ct.isCorrect()) and np.array_equal(ea.decrypt_batch(ct, sk), cube)
        correct = correct and bool(ok)
        note("round %d: construct %.0f / %.0f ms, apply %.0f / %.0f ms, correct %s" % (k, ms_fw, ms_inv, ms_afw, ms_ainv, ok))
        if k:
            t_fw.append(ms_fw)
            t_inv.append(ms_inv)
            t_afw.append(ms_afw)
            t_ainv.append(ms_ainv)

    # the powerful basis on one ciphertext part's rows
    pd = PW.PowerfulDCRT(g, mvec)
    idx = list(cc.ctxtPrimes)
    rows = np.stack([rng.integers(0, cc.primes[i], size=(B, g.phim), dtype=np.uint64) for i in idx])
    part = capi.DoubleCRT(g, idx, B, data=rows)
    t_dev_to, t_dev_back, t_np_to, t_np_back, same = [], [], [], [], True
    for k in range(a.reps + 1):
        ms_dt, _ = wall(lambda: pd.dcrtToPowerful(part))
        dev = part.download()
        t0 = time.perf_counter()
        host = np.stack([conv.polyToPowerful(rows[j].astype(np.int64), cc.primes[i]) for j, i in enumerate(idx)])
        ms_nt = (time.perf_counter() - t0) * 1e3
        ms_db, _ = wall(lambda: pd.powerfulToDCRT(part))
        t0 = time.perf_counter()
        back = np.stack([conv.powerfulToPoly(host[j], cc.primes[i]) for j, i in enumerate(idx)])
        ms_nb = (time.perf_counter() - t0) * 1e3
        same = same and np.array_equal(dev.astype(np.int64), host) and np.array_equal(part.download(), rows) and \
            np.array_equal(back.astype(np.uint64), rows)
        if k:
            t_dev_to.append(ms_dt)
            t_dev_back.append(ms_db)
            t_np_to.append(ms_nt)
            t_np_back.append(ms_nb)

    def med(x):
        return round(statistics.median(x), 2)

    def runs(x):
        return [round(v, 2) for v in x]
    out = {"tool": "bench_evalmap", "m": m, "p": p, "r": r, "mvec": mvec, "gens": list(a.gens), "ords": ea.zMStar.signedOrds(),
           "phim": g.phim, "bits": a.bits, "d": d, "nslots": n, "batch": B, "rows_per_part": len(idx), "reps": a.reps,
           "fused_constants": bool(fw.mat1.fusedConstants),
           "construct_forward_ms": med(t_fw), "construct_inverse_ms": med(t_inv),
           "apply_forward_ms": med(t_afw), "apply_inverse_ms": med(t_ainv),
           "construct_forward_runs_ms": runs(t_fw), "construct_inverse_runs_ms": runs(t_inv),
           "apply_forward_runs_ms": runs(t_afw), "apply_inverse_runs_ms": runs(t_ainv), "apply_correct": bool(correct),
           "to_powerful_device_ms": med(t_dev_to), "to_powerful_numpy_ms": med(t_np_to),
           "to_poly_device_ms": med(t_dev_back), "to_poly_numpy_ms": med(t_np_back),
           "to_powerful_device_runs_ms": runs(t_dev_to), "to_powerful_numpy_runs_ms": runs(t_np_to),
           "to_poly_device_runs_ms": runs(t_dev_back), "to_poly_numpy_runs_ms": runs(t_np_back),
           "device_and_numpy_same_words": bool(same)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
