"""Times the construction of BlockMatMul1DExec constants over GF(2^16) slots at m = 21845, p = 2 (n = 1024, d = 16) on the
device and on the host, and one mul each; writes profiles/bgv_gf_matmul.json.  Every measurement is bracketed by a
device sync.  Nothing is gated: these are the first figures for this path.

  python tools/bench_bgv_gf_matmul.py [--bits 300] [--out profiles/bgv_gf_matmul.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=300)
    ap.add_argument("--out", default=os.path.join("profiles", "bgv_gf_matmul.json"))
    args = ap.parse_args()
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    from helib_amd import bgv_gf, bgv_gf_matmul as gm, capi, ctxt as hc, keys as hk
    m, p = 21845, 2
    cc = hc.ChainContext(m, p, 1, bits=args.bits, c=3)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=5)
    sk.GenSecKey()
    ea = bgv_gf.EncryptedArray(cc, g)
    sk.zMStar = ea.zMStar
    hk.addSome1DMatrices(sk)
    hk.addFrbMatrices(sk)
    n, d = ea.size(), ea.getDegree()
    res = {"m": m, "p": p, "nslots": n, "d": d, "bits": args.bits, "seconds": {}}

    def timed(name, fn):
        g.sync()
        t0 = time.perf_counter()
        out = fn()
        g.sync()
        res["seconds"][name] = time.perf_counter() - t0
        print("%-44s %.4f s" % (name, res["seconds"][name]), file=sys.stderr)
        return out
    timed("table build (host, C++)", lambda: capi.bgvGfLinalgTables(p, d, ea.getG()))
    timed("table build (host, numpy)", lambda: gm.linPolyTable(ea))
    rng = np.random.default_rng(1)
    cases = {"special dimension (nb = n)": gm.BlockMatMul1D(ea, rng.integers(0, p, size=(n, 1, 1, d, d)), ea.dimension()),
             "dimension 1 (D = 8)": gm.BlockMatMul1D(ea, rng.integers(0, p, size=(8, 8, d, d)), 1)}
    v = rng.integers(0, p, size=(1, n, d))
    for name, mat in cases.items():
        timed(name + ": matrix upload + linpoly", lambda: mat.handle(ea.enc))
        dev = timed(name + ": gather + encode, device", lambda: gm.BlockMatMul1DExec(ea, mat))
        timed(name + ": gather + encode, host", lambda: gm.BlockMatMul1DExec(ea, mat, device_diagonals=False))
        ct = ea.encrypt_batch(sk, v)
        timed(name + ": mul", lambda: dev.mul(ct, pk=sk))
        res[name + ": correct"] = bool(np.array_equal(ea.decrypt_batch(ct, sk), gm.mulPlain(ea, v, mat)))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
