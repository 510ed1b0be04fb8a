"""MatMul1DExec.mul at m = 65536, bits = 1400, batch 64 with 64 and 1024 non-zero diagonals: fused
(hx_mul_add_many) against forced term by term in one process, split into baby steps (hoisting), the multiply-add,
giant-step rotations and construction.  Each phase is the median of --reps runs, device-synchronised.  The multiply-add phase is everything MulAdd stands
for: on the fused side the host bookkeeping on data-less operands, the zeroed outputs and one hx_mul_add_many per
giant step; so the bytes per second derived from it are a lower bound on the kernel's own rate.
Prints one JSON line and saves it as profiles/ckks_matmul_bench.json.
Not part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING = 6.29e12     # bytes/s of a float4 device copy measured on an MI355X (read + write): the streaming ceiling


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=65536)
    ap.add_argument("--bits", type=int, default=1400)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--diagonals", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--reps", type=int, default=5, help="timed runs per leg; the median of each phase is reported")
    a = ap.parse_args()
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    from helib_amd import capi as hx, ckks, ctxt as hc, keys as hk
    m, B, D = a.m, a.batch, a.m // 4
    cc = hc.ChainContext(m, -1, 20, bits=a.bits, c=3, ckks=True)
    g = hx.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey(maxDegKswitch=2)
    hk.addBSGS1DMatrices(sk)
    ea = ckks.EncryptedArrayCx(cc, g)
    rng = np.random.default_rng(0)
    v = (rng.uniform(-1, 1, (B, D)) + 1j * rng.uniform(-1, 1, (B, D))) / 2
    ct0 = ea.encrypt_batch(sk, v)
    out = {"m": m, "bits": a.bits, "batch": B, "primes": len(cc.ctxtPrimes), "cases": []}
    for nd in a.diagonals:
        diags = {int(i): (rng.uniform(-1, 1, D) + 1j * rng.uniform(-1, 1, D)) / nd for i in range(nd)}
        # the dense form would be D x D complex (4 GiB at D = 16384): feed the diagonals through processDiagonal

        class Mat(ckks.MatMul1D_CKKS):
            def processDiagonal(self, i):
                return diags.get(i, np.zeros(D, dtype=np.complex128))
        ex = ckks.MatMul1DExec(ea, Mat(ea, lambda r, c: 0.0))
        ex.sync = g.sync
        g.sync()
        case = {"diagonals": nd, "g": ex.g, "construct_s": ex.times["construct"]}
        results, samples = {}, {"fused": [], "term_by_term": []}
        for rep in range(a.reps + 1):           # the first round warms up
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
            case[label]["muladd_min"] = float(min(x["muladd"] for x in ss))
        case["reps"] = a.reps
        same = all(np.array_equal(results["fused"].parts[h].download(), results["term_by_term"].parts[h].download())
                   for h in results["fused"].parts)
        case["equal"] = bool(same)
        case["muladd_speedup"] = case["term_by_term"]["muladd"] / case["fused"]["muladd"]
        # bytes by the kernel's formula: (n / B' + n parts + parts (1 + accumulate)) * 8 per coefficient, prime and
        # batch element, B' = 4, summed over the giant steps (n = diagonals of that step, accumulate = 0)
        rows = len(results["fused"].primeSet)
        groups = {}
        for i in diags:
            groups[i // ex.g] = groups.get(i // ex.g, 0) + 1
        byts = sum((n / 4 + 2 * n + 2) * 8 for n in groups.values()) * (m // 2) * len(cc.ctxtPrimes) * B
        case["muladd_bytes"] = byts
        case["muladd_bytes_per_s"] = byts / case["fused"]["muladd"]
        case["fraction_of_copy_ceiling"] = case["muladd_bytes_per_s"] / COPY_CEILING
        case["result_rows"] = rows
        out["cases"].append(case)
        del results
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ckks_matmul_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
