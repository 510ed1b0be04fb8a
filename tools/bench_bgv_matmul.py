"""BGV MatMul1DExec along dimension 0 at m = 32768, p = 65537, bits = 950, batch 64, for a banded matrix of 64 and of
1024 non-zero diagonals, in one process:
  construction   the device path (the matrix uploaded once, hx_bgv_encode_diagonals) against the host path (numpy
                 gather + hx_bgv_encode), a warm-up and then the median of --reps runs each, device-synchronised
  mul            baby steps / multiply-add / giant steps, fused (hx_mul_add_many) against forced term by term, as
                 tools/bench_matmul.py has them for CKKS
Prints one JSON line and saves it as profiles/bgv_matmul.json.  Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=32768)
    ap.add_argument("--p", type=int, default=65537)
    ap.add_argument("--bits", type=int, default=950)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--diagonals", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--reps", type=int, default=3, help="timed runs per leg after one warm-up; medians are reported")
    a = ap.parse_args()
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    from helib_amd import bgv, bgv_matmul as M, capi as hx, ctxt as hc, keys as hk
    m, p, B = a.m, a.p, a.batch
    cc = hc.ChainContext(m, p, 1, bits=a.bits, c=3)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey()
    ea = bgv.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    D = ea.sizeOfDimension(0)
    z, gs = ea.zMStar, hk.KSGiantStepSize(D)
    for j in list(range(1, gs)) + list(range(gs, D, gs)):     # addBSGS1DMatrices for dimension 0 alone
        sk.GenKeySWmatrix(1, z.genToPow(0, j))
    hk._setKSStrategy(sk, 0, hk.HELIB_KSS_BSGS)
    sk.setKeySwitchMap()
    rng = np.random.default_rng(0)
    v = rng.integers(0, p, size=(B, ea.size()))
    ct0 = ea.encrypt_batch(sk, v)
    out = {"m": m, "p": p, "bits": a.bits, "batch": B, "primes": len(cc.ctxtPrimes), "D": D, "cases": []}
    j = np.arange(D)
    for nd in a.diagonals:
        dense = np.zeros((D, D), dtype=np.int64)
        for i in range(nd):
            dense[(j - i) % D, j] = rng.integers(1, p, size=D)
        case = {"diagonals": nd}
        ex = None
        for label, dev in (("construct_host_s", False), ("construct_device_s", True)):
            ts = []
            for rep in range(a.reps + 1):
                ex = None                                      # free the constants of the run before
                g.sync()
                t0 = time.perf_counter()
                ex = M.MatMul1DExec(ea, M.MatMul1D(ea, dense, 0), device_diagonals=dev)   # the upload is inside
                g.sync()
                if rep:
                    ts.append(time.perf_counter() - t0)
            assert ex.onDevice == dev and sum(mm is not None for mm in ex.multiplier) == nd
            case[label] = float(np.median(ts))
            print(nd, label, case[label], file=sys.stderr, flush=True)
        case["g"] = ex.g
        case["construct_speedup"] = case["construct_host_s"] / case["construct_device_s"]
        ex.sync = g.sync
        results, samples = {}, {"fused": [], "term_by_term": []}
        for rep in range(a.reps + 1):
            for label, fused in (("fused", True), ("term_by_term", False)):
                for k in ("baby", "muladd", "giant"):
                    ex.times[k] = 0.0
                ct = ct0.clone()
                ex.mul(ct, sk, fused=fused)
                g.sync()
                results[label] = ct
                if rep:
                    samples[label].append({k: ex.times[k] for k in ("baby", "muladd", "giant")})
        for label, ss in samples.items():
            case[label] = {k: float(np.median([x[k] for x in ss])) for k in ("baby", "muladd", "giant")}
        case["reps"] = a.reps
        case["equal"] = bool(all(np.array_equal(results["fused"].parts[h].download(),
                                                results["term_by_term"].parts[h].download())
                                 for h in results["fused"].parts))
        case["correct"] = bool(np.array_equal(ea.decrypt_batch(results["fused"], sk)[:2], M.mulPlain(ea, v[:2], ex.mat)))
        case["muladd_speedup"] = case["term_by_term"]["muladd"] / case["fused"]["muladd"]
        case["fallbacks"] = M.MatMul1DExec.fallbacks
        out["cases"].append(case)
        del results, ex
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "bgv_matmul.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
