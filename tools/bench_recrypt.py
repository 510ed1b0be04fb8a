#!/usr/bin/env python3
"""The pre-processing of recryption (hx_recrypt_prep, helib_amd.recryption.rawModSwitch) at the reference's bootstrapping
row for m = 21845 (tests/GTestBootstrapping.cpp:113): p = 2, r = 1, mvec (17, 5, 257), a bootstrappable chain, batch 32.
The two parts of a ciphertext as reCrypt leaves them before the step: three ciphertext primes and the special primes,
uniform rows.  In one process, in alternated pairs:

  prep, fused     recrypt_prep_kernel on both parts: coefficient rows in, rows on the key's primes out, on the device
  prep, python    the same arithmetic the way the tree could do it before: download both parts, lift every coefficient
                  to a Python integer (object arrays), scale, correct, reduce, make divisible, divide, reduce modulo
                  every prime of the key, upload -- the words are compared with the kernel's
  pipeline        per part iFFT, dcrtToPowerful, prep, powerfulToDCRT, FFT: what rawModSwitch runs

Then the whole reCrypt (--gens / --ords choose the slot hypercube): bits = the smallest multiple of 100, from
--bits-from up to --bits-max, at which a batch whose capacity has been used up is recrypted with isCorrect(), positive
capacity and the exact plaintext; there the time per phase (the reference's named timers: AAA_preProcess,
AAA_LinearTransform1, AAA_extractDigitsPacked, AAA_LinearTransform2) and the capacity before and after.  --no-recrypt
leaves that part out; its fields are then null: not measured.

Wall clock around calls that end in a synchronise, --reps pairs after one warm pair.  No default depends on these numbers.
Writes profiles/recrypt.json (--out) and prints the same JSON line.

  python tools/bench_recrypt.py          # MI355X
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

M64 = np.uint64((1 << 64) - 1)


def _mix(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def tie_words(seed, part, B, n):
    """recrypt_core.h's tie word of every (batch element, coefficient), uint64 [B, n]"""
    with np.errstate(over="ignore"):
        s = _mix(np.array([seed & ((1 << 64) - 1)], dtype=np.uint64)) + np.uint64(part)
        b = _mix(s) + np.arange(B, dtype=np.uint64)
        return _mix(_mix(b)[:, None] + np.arange(n, dtype=np.uint64)[None, :])


def prep_python(rows, src, tgt, q, p, p2r, p2e, seed, part):
    """hx_recrypt_prep's definition (include/helib_amd.h) on Python integers held in object arrays"""
    k, B, n = rows.shape
    Q = 1
    for s in src:
        Q *= s
    c = np.zeros((B, n), dtype=object)
    for i, s in enumerate(src):
        Qi = Q // s
        c = c + rows[i].astype(object) * (Qi * pow(Qi, -1, s))
    c = c % Q
    c = np.where(c > Q // 2, c - Q, c)
    cq = c * q
    X = cq // Q
    Y = cq - X * Q
    wrap = Y > Q // 2
    Y = np.where(wrap, Y - Q, Y)
    X = np.where(wrap, X + 1, X)
    t = tie_words(seed, part, B, n)
    bit = [((t >> np.uint64(61 + w)) & np.uint64(1)).astype(bool) for w in range(3)]
    delta = (Y % p2r) * pow(Q, -1, p2r) % p2r
    down = delta > p2r // 2
    if p2r % 2 == 0:
        down = down | ((delta == p2r // 2) & ((Y < 0) | ((Y == 0) & bit[0])))
    x = X + np.where(down, delta - p2r, delta)
    hi = x > q // 2
    lo = x < -(q // 2)
    if q % 2 == 0:
        hi = hi | ((x == q // 2) & bit[1])
        lo = lo | ((x == -(q // 2)) & bit[1])
    x = np.where(hi, x - q, np.where(~hi & lo, x + q, x))
    if p2e == 1:
        v = np.zeros((B, n), dtype=object)
    else:
        z = x % p2e
        up = z > p2e // 2
        if p == 2:
            up = up | ((z == p2e // 2) & bit[2])
        v = np.where(up, p2e - z, -z)
    w = (x + q * v) // p2e
    return np.stack([(w % tq).astype(np.uint64) for tq in tgt])


def recrypt_at_smallest_bits(a):
    from helib_amd import capi, ctxt as hc, keys as hk, recryption as RC, timing
    m, p, r, B = a.m, a.p, a.r, a.batch
    tried = []
    for bits in range(a.bits_from, a.bits_max + 1, 100):
        cc = hc.ChainContext(m, p, r, bits=bits, c=3, bootstrappable=True)
        g = capi.Context(m)
        for qq in cc.primes:
            g.add_prime(qq)
        rc = RC.RecryptData(cc, g, a.mvec, gens=a.gens, ords=a.ords, maps=True)
        ea = rc.ea
        sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
        sk.GenSecKey()
        sk.zMStar = ea.zMStar
        if ea.getDegree() <= 8:
            hk.addSome1DMatrices(sk)
            hk.addFrbMatrices(sk)
        else:
            hk.addMinimal1DMatrices(sk)
            hk.addMinimalFrbMatrices(sk)
        sk.genRecryptData(rc)
        v = np.random.default_rng(1).integers(0, p ** r, size=(B, ea.size(), ea.getDegree()))
        want, ct = v, ea.encrypt_batch(sk, v)
        while ct.bitCapacity() > 60:
            ct.multiplyBy(ea.encrypt_batch(sk, v))
            want = ea.mulPlain(want, v)
        before = ct.bitCapacity()
        timing.resetAllTimers()
        g.sync()
        t0 = time.perf_counter()
        try:
            RC.reCrypt(ct, sk, rc, seed=7)
            g.sync()
            ms = (time.perf_counter() - t0) * 1e3
            ok = bool(ct.isCorrect()) and ct.bitCapacity() > 0 and np.array_equal(ea.decrypt_batch(ct, sk), want)
            why = "" if ok else "not correct"
        except RC.LogicError as ex:
            ok, ms, why = False, None, str(ex)[:80]
        tried.append({"bits": bits, "ok": bool(ok), "why": why})
        print("bits %d: %s %s" % (bits, ok, why), file=sys.stderr, flush=True)
        if ok:
            def t(name):
                return round(timing.getTimerByName(name).counter * 1e3, 2)
            return {"recrypt_bits": bits, "recrypt_tried": tried, "recrypt_ms": round(ms, 2), "pre_process_ms": t("AAA_preProcess"),
                    "first_map_ms": t("AAA_LinearTransform1"), "digit_extraction_ms": t("AAA_extractDigitsPacked"),
                    "second_map_ms": t("AAA_LinearTransform2"), "capacity_before": before, "capacity_after": ct.bitCapacity(),
                    "d": ea.getDegree(), "nslots": ea.size(), "not_measured": None}
        del ct, sk, rc, ea, g
    return {"recrypt_bits": None, "recrypt_tried": tried, "first_map_ms": None, "digit_extraction_ms": None, "second_map_ms": None,
            "pre_process_ms": None, "recrypt_ms": None, "capacity_before": None, "capacity_after": None,
            "not_measured": "no bits up to %d gave a correct recryption" % a.bits_max}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=21845)
    ap.add_argument("--p", type=int, default=2)
    ap.add_argument("--r", type=int, default=1)
    ap.add_argument("--mvec", type=int, nargs="+", default=[17, 5, 257])
    ap.add_argument("--bits", type=int, default=300)
    ap.add_argument("--gens", type=int, nargs="+", default=[8996, 17477, 21591])
    ap.add_argument("--ords", type=int, nargs="+", default=[16, 4, -16])
    ap.add_argument("--bits-from", type=int, default=300)
    ap.add_argument("--bits-max", type=int, default=1200)
    ap.add_argument("--no-recrypt", action="store_true")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recrypt.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import capi, ctxt as hc, recryption as RC
    m, p, r, B = a.m, a.p, a.r, a.batch
    cc = hc.ChainContext(m, p, r, bits=a.bits, c=3, bootstrappable=True)
    g = capi.Context(m)
    for qq in cc.primes:
        g.add_prime(qq)
    rc = RC.RecryptData(cc, g, a.mvec)
    src_idx = sorted(cc.ctxtPrimes)[:3] + sorted(cc.specialPrimes)
    tgt_idx = sorted(cc.ctxtPrimes)
    src, tgt = [cc.primes[i] for i in src_idx], [cc.primes[i] for i in tgt_idx]
    q, p2r, p2e = rc.q, rc.p2r, rc.p2ePrime
    rng = np.random.default_rng(1)
    rows = [np.stack([rng.integers(0, s, size=(B, g.phim), dtype=np.uint64) for s in src]) for _ in range(2)]
    parts = [capi.DoubleCRT(g, src_idx, B, data=x) for x in rows]

    def wall(fn):
        g.sync()
        t0 = time.perf_counter()
        out = fn()
        g.sync()
        return (time.perf_counter() - t0) * 1e3, out

    def fused():
        return [capi.recryptPrep(parts[i], tgt_idx, q, p, p2r, p2e, 7, i) for i in range(2)]

    def python():
        host = [x.download() for x in parts]
        return [capi.DoubleCRT(g, tgt_idx, B, data=prep_python(host[i], src, tgt, q, p, p2r, p2e, 7, i)) for i in range(2)]

    def pipeline():
        out = []
        for i in range(2):
            part = parts[i].copy()
            part.iFFT()
            rc.p2dConv.dcrtToPowerful(part)
            z = capi.recryptPrep(part, tgt_idx, q, p, p2r, p2e, 7, i)
            rc.p2dConv.powerfulToDCRT(z)
            out.append(z.FFT())
        return out

    t_f, t_p, t_pipe, same = [], [], [], True
    for k in range(a.reps + 1):                      # the first pair warms buffers
        ms_f, zf = wall(fused)
        ms_p, zp = wall(python)
        ms_pipe, _ = wall(pipeline)
        same = same and all(np.array_equal(x.download(), y.download()) for x, y in zip(zf, zp))
        print("pair %d: fused %.3f ms, python %.0f ms, pipeline %.2f ms, same words %s" % (k, ms_f, ms_p, ms_pipe, same),
              file=sys.stderr, flush=True)
        if k:
            t_f.append(ms_f)
            t_p.append(ms_p)
            t_pipe.append(ms_pipe)

    whole = {"first_map_ms": None, "digit_extraction_ms": None, "second_map_ms": None, "pre_process_ms": None,
             "capacity_before": None, "capacity_after": None, "recrypt_bits": None, "recrypt_ms": None,
             "not_measured": "the whole reCrypt was not run"}
    phim, e, ePrime = g.phim, rc.e, rc.ePrime        # (the objects go before the search builds its own)
    if not a.no_recrypt:
        del parts, rc, g
        whole = recrypt_at_smallest_bits(a)

    def med(x):
        return round(statistics.median(x), 3)

    def runs(x):
        return [round(v, 3) for v in x]
    out = {"tool": "bench_recrypt", "m": m, "p": p, "r": r, "mvec": list(a.mvec), "phim": phim, "bits": a.bits, "batch": B,
           "e": e, "ePrime": ePrime, "q": q, "rows_in": len(src_idx), "rows_out": len(tgt_idx), "parts": 2, "reps": a.reps,
           "coefficients": 2 * B * phim, "algorithmic_bytes": 2 * B * phim * 8 * (len(src_idx) + len(tgt_idx)),
           "prep_fused_ms": med(t_f), "prep_python_ms": med(t_p), "prep_fused_runs_ms": runs(t_f), "prep_python_runs_ms": runs(t_p),
           "raw_mod_switch_pipeline_ms": med(t_pipe), "raw_mod_switch_pipeline_runs_ms": runs(t_pipe),
           "fused_and_python_same_words": bool(same)}
    out.update(whole)
    line = json.dumps(out, default=lambda o: o.item() if hasattr(o, "item") else str(o))   # (numpy scalars)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
