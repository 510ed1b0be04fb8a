#!/usr/bin/env python3
"""CKKS slot encoding / decoding on the device (hx_ckks_encode / hx_ckks_decode, helib_amd.ckks) against the host
path each one replaces, at BASELINE configs[3]'s shape: m = 65536, bits = 1400 (24 ctxt primes), a batch of 64.

  encode + NTT       hx_ckks_encode into the ctxt primes      vs  numpy CKKS_embedInSlots + fromCoeffs (upload + FFT)
  encryptBatch       EncryptedArrayCx.encrypt_batch (encode + PubKey.CKKSencryptBatch; host samplers included)
  hx_ckks_decode     Garner / ratFactor + embedding + download vs  iFFT + one download, python big-integer CRT
                                                                  (keys.crt_centred) + numpy embedding per element
  rawDecryptBatch    inner product + hx_ckks_decode

Device times are HIP events on the context's stream (hx_ctx_timer_begin / _end; the calls synchronise, so they also
hold the host-side set-up and the copies); host times are wall clock.  The host decode is timed on --host-elems
elements and scaled to the batch.  Algorithmic bytes: encode writes L*N*8 per element (the evaluation-form rows), the
decode reads them.  One JSON line on stdout.

  python tools/bench_ckks_slots.py          # MI355X
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8e12   # HBM bytes/s


def host_encode(v, m, T, scaling):
    """CKKS_embedInSlots in numpy (src/norms.cpp:574-615)"""
    B = v.shape[0]
    buf = np.zeros((B, m // 2), dtype=np.complex128)
    ii = m // 4 - 1 - np.arange(m // 4)
    buf[:, T >> 1] = np.conj(v[:, ii])
    buf[:, (m - T) >> 1] = v[:, ii]
    x = (np.fft.fft(buf, axis=-1) * np.exp(-2j * np.pi * np.arange(m // 2) / m)).real * (scaling / (m // 2))
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def host_embed(f, m, T):
    """CKKS_canonicalEmbedding in numpy (src/norms.cpp:495-519)"""
    buf = np.fft.fft(f * np.exp(-2j * np.pi * np.arange(m // 2) / m), axis=-1)
    v = np.empty((f.shape[0], m // 4), dtype=np.complex128)
    v[:, m // 4 - 1 - np.arange(m // 4)] = buf[:, T >> 1]
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=65536)
    ap.add_argument("--bits", type=int, default=1400)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-elems", type=int, default=1)
    a = ap.parse_args()
    try:
        import torch  # noqa: F401   (first: see tests/test_gpu_parity.py)
    except ImportError:
        pass
    from helib_amd import capi, ckks, ctxt as hc, hostnt, keys as hk
    m, B = a.m, a.batch
    cc = hc.ChainContext(m, -1, 20, bits=a.bits, c=3, ckks=True)
    g = capi.Context(m)
    for q in cc.primes:
        g.add_prime(q)
    sk = hk.SecKey(cc, hk.HxBackend(g, cc), seed=1)
    sk.GenSecKey(maxDegKswitch=2)
    ea = ckks.EncryptedArrayCx(cc, g)
    T = np.array(hostnt.ZmStar(m, -1).reps())
    idx = list(cc.ctxtPrimes)
    L, N = len(idx), cc.phim
    rng = np.random.default_rng(1)
    v = (rng.uniform(-1, 1, (B, m // 4)) + 1j * rng.uniform(-1, 1, (B, m // 4))) / math.sqrt(2)
    f = ea.factor(v)

    def dev(fn):
        fn()   # warm: tables, buffers
        best = float("inf")
        for _ in range(a.reps):
            g.timerBegin()
            fn()
            best = min(best, g.timerEnd() * 1e3)
        return best

    def wall(fn, reps=1):
        best = float("inf")
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            best = min(best, (time.perf_counter() - t0) * 1e6)
        return best

    enc_us = dev(lambda: capi.ckksEncode(g, v, f, idx))

    def host_enc():
        cf = host_encode(v, m, T, f)
        rows = np.empty((L, B, N), dtype=np.uint64)
        for r, i in enumerate(idx):
            rows[r] = np.mod(cf, np.int64(cc.primes[i])).astype(np.uint64)
        capi.DoubleCRT(g, idx, B, rows).FFT()
        g.sync()
    host_enc_us = wall(host_enc, 2)
    encb_us = dev(lambda: ea.encrypt_batch(sk, v))
    ct = ea.encrypt_batch(sk, v)
    acc = ckks.innerProduct(sk, ct)
    dec_us = dev(lambda: capi.ckksDecode(acc, ct.lnRatFactor))
    rdb_us = dev(lambda: ea.rawDecrypt_batch(ct, sk))
    got = capi.ckksDecode(acc, ct.lnRatFactor)
    err = float(np.max(np.abs(got - v)))

    # the host path: inverse transform + ONE download of the whole batch, then per element the centred CRT in
    # python big integers (helib_amd.keys.crt_centred, what HxBackend.toPoly does) and the numpy embedding; the
    # per-element part is timed on --host-elems elements and scaled to the batch
    rows_all = [None]

    def host_fetch():
        rows_all[0] = acc.copy().iFFT().download()

    def host_dec():
        for b in range(a.host_elems):
            vals = hk.crt_centred([cc.primes[i] for i in acc.getIndexSet()], rows_all[0][:, b])
            fl = np.array([float(x) for x in vals]) / math.exp(ct.lnRatFactor)
            host_embed(fl[None, :], m, T)
    fetch_us = wall(host_fetch)
    host_dec_us = fetch_us + wall(host_dec) * B / a.host_elems
    bytes_ = L * N * 8 * B
    out = {
        "tool": "bench_ckks_slots", "m": m, "bits": a.bits, "L": L, "batch": B,
        "encode_ntt_us": round(enc_us, 1), "host_encode_upload_us": round(host_enc_us, 1),
        "encode_speedup": round(host_enc_us / enc_us, 1),
        "encrypt_batch_us": round(encb_us, 1),
        "decode_us": round(dec_us, 1), "host_crt_embed_us": round(host_dec_us, 1),
        "host_decode_path": "iFFT + 1 download; python big-integer crt_centred + numpy embedding per element",
        "host_decrypt_elems_timed": a.host_elems, "decode_speedup": round(host_dec_us / dec_us, 1),
        "raw_decrypt_batch_us": round(rdb_us, 1),
        "alg_bytes": bytes_, "alg_bytes_at_8TBs_us": round(bytes_ / PEAK * 1e6, 1),
        "encode_frac_of_peak": round(bytes_ / PEAK * 1e6 / enc_us, 3),
        "decode_frac_of_peak": round(bytes_ / PEAK * 1e6 / dec_us, 3),
        "max_slot_error": err, "errorBound": ckks.errorBound(ct),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
