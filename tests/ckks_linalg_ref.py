"""Restatements of the reference's plaintext maps between CKKS slots, from their definitions:

  rotate(v, k)      tmp[((i + k) % n + n) % n] = data[i]          (rotate_pa_impl, src/EncryptedArray.cpp:887-905)
  shift(v, k)       data[j] = 0 where j + k >= n or j + k < 0, then rotate   (shift_pa_impl, :946-963)
  totalSums(v)      every slot <- the sum                          (:1974-1990)
  runningSums(v)    data[i] += data[i - 1], i = 1..n-1             (:1995-2007)
  matmul(A, v)      w[j] = sum_r get(r, j) v[r]                    (mul(PlaintextArray, MatMul1D), src/matmul.cpp:2673-2696)

and the CPU stand-in for the device encoder that lets helib_amd.ckks / helib_amd.linalg run over the oracle backend."""
import math

import numpy as np

from tests import ckks_ref as R


def rotate(v, k):
    v = np.asarray(v)
    n = len(v)
    out = np.empty_like(v)
    for i in range(n):
        out[((i + k) % n + n) % n] = v[i]
    return out


def shift(v, k):
    v = np.array(v)
    n = len(v)
    for j in range(n):
        if j + k >= n or j + k < 0:
            v[j] = 0
    return rotate(v, k)


def totalSums(v):
    return np.full(len(v), np.sum(v), dtype=np.complex128)


def runningSums(v):
    v = np.array(v, dtype=np.complex128)
    for i in range(1, len(v)):
        v[i] += v[i - 1]
    return v


def matmul(get, v):
    n = len(v)
    return np.array([sum(get(r, j) * v[r] for r in range(n)) for j in range(n)], dtype=np.complex128)


class HostEncoder:
    """CKKS_embedInSlots in numpy, then the backend's fromCoeffs: one vector at a time"""
    max_batch = 1

    def __init__(self, backend, m, coeffs=None):
        self.be, self.m, self.coeffs = backend, m, coeffs

    def encode(self, v, scaling, idx):
        v = np.atleast_2d(v)
        assert v.shape[0] == 1
        cf = self.coeffs(v, scaling) if self.coeffs else R.embed_in_slots(v, self.m, scaling)
        return self.be.fromCoeffs(list(idx), [int(c) for c in cf[0]])

    def split(self, poly):
        return [poly]


def decrypt(sk, ct, m):
    """SecKey.Decrypt, then the numpy decode"""
    if not ct.parts:
        return np.zeros(m // 4, dtype=np.complex128)
    f = np.array([float(x) for x in sk.Decrypt(ct)]) / math.exp(ct.lnRatFactor)
    return R.canonical_embedding(f, m)[0]
