"""numpy restatement of the reference's CKKS slot maps, written from their definitions (src/norms.cpp:495-615,
include/helib/PGFFT.h:38-41: dst[i] = sum_j src[j] W^(ij), W = exp(-2 pi i/n) -- numpy's forward FFT):

  canonical_embedding(f)   v[m/4-1-i] = f(zeta^-T[i]),  zeta = exp(2 pi i/m)
  embed_in_slots(v, s)     buf[T[i]>>1] = conj(v[m/4-1-i]), buf[(m-T[i])>>1] = v[m/4-1-i], the (m/2)-point FFT,
                           f_k = round(Re(buf_k pow_k) s/(m/2)), pow_k = exp(-2 pi i k/m), halves away from zero

T = PAlgebra's ith_rep table of Z_m^*/<-1> (helib_amd.hostnt.ZmStar(m, -1))."""
import functools

import numpy as np

from helib_amd import hostnt


@functools.lru_cache(maxsize=None)
def zmstar(m):
    return hostnt.ZmStar(m, -1)


def reps(m):
    return np.array(zmstar(m).reps(), dtype=np.int64)


def _pow(m):
    return np.exp(-2j * np.pi * np.arange(m // 2) / m)


def canonical_embedding(f, m, T=None):
    """f: [B, m/2] real -> [B, m/4] complex"""
    T = reps(m) if T is None else T
    f = np.atleast_2d(np.asarray(f, dtype=np.float64))
    buf = np.fft.fft(f * _pow(m), axis=-1)
    v = np.empty((f.shape[0], m // 4), dtype=np.complex128)
    v[:, m // 4 - 1 - np.arange(m // 4)] = buf[:, T >> 1]
    return v


def embed_unrounded(v, m, scaling, T=None):
    """the values CKKS_embedInSlots rounds: [B, m/2] float"""
    T = reps(m) if T is None else T
    v = np.atleast_2d(np.asarray(v, dtype=np.complex128))
    B, ns = v.shape
    buf = np.zeros((B, m // 2), dtype=np.complex128)
    i = np.arange(m // 4)
    ii = m // 4 - i - 1
    keep = ii < ns
    buf[:, T[keep] >> 1] = np.conj(v[:, ii[keep]])
    buf[:, (m - T[keep]) >> 1] = v[:, ii[keep]]
    buf = np.fft.fft(buf, axis=-1)
    return (buf * _pow(m)).real * (scaling / (m // 2))


def round_away(x):
    """std::round"""
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def embed_in_slots(v, m, scaling, T=None):
    return round_away(embed_unrounded(v, m, scaling, T)).astype(np.int64)


def direct_embedding(f, m, T=None):
    """O(n^2) evaluation v[m/4-1-i] = f(zeta^-T[i]) (the definition the FFT form is checked against)"""
    T = reps(m) if T is None else T
    f = np.atleast_2d(np.asarray(f, dtype=np.float64))
    n = m // 2
    pts = np.exp(-2j * np.pi * np.outer(T, np.arange(n)) / m)     # [m/4, n]: zeta^(-T_i k)
    vals = f @ pts.T                                                  # [B, m/4]
    v = np.empty_like(vals)
    v[:, m // 4 - 1 - np.arange(m // 4)] = vals
    return v
