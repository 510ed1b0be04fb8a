// ckks_slots.h -- device side of CKKS slot encoding (EncryptedArrayCx, src/EaCx.cpp) for m = 2N a power of
// two, 16 <= m <= 2^17.  W = exp(2 pi i/m), omega = W^2; wtab[k] = W^k for k < N (W^(k+N) = -W^k).
//
// Slot order (PAlgebra's table T of Z_m^*/<-1>, src/PAlgebra.cpp:520-570): slot s holds f(W^-T[m/4-1-s]), i.e.
// f(W^(2j+1)) for j = jdec(s) = (m - T[m/4-1-s] - 1)/2; jinfo[j] = s and jinfo[N-1-j] = s | CKKS_CONJ (the
// conjugate root, which no slot keeps).  One table serves both directions:
//
//   embed  (CKKS_canonicalEmbedding, src/norms.cpp:495-519):  F_j = f(W^(2j+1)) = sum_n (f_n W^n) omega^(nj)
//   encode (CKKS_embedInSlots, src/norms.cpp:574-615): the reference fills buf[T>>1] = conj(v), buf[(m-T)>>1] = v
//          and takes f_k = round(Re(W^-k sum_j buf_j omega^(-jk)) scaling/N) = round(Re(W^k Y_k) scaling/N) with
//          Y = the omega-DFT of x = conj(buf): x_jdec(s) = conj(v_s), x_(N-1-jdec(s)) = v_s.
//
// Both are N-point complex DFTs with the root omega, held in LDS as S = N/H sub-transforms of H <= 8192 points
// (one workgroup each), the first log2(S) decimation levels folded into the load (embed_norm_kernel's form):
// sub-transform s gives the outputs k = s + S k', k' = brev(p) at LDS position p (dif_fft_lds, fft_lds.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_common.h"
#include "fft_lds.h"

namespace hx {

constexpr uint32_t CKKS_CONJ = 0x80000000u;
constexpr int CKKS_MAXPRIMES = 64;   // rows of one decode

// W^e for any e (mod 2N)
__device__ __forceinline__ double2 ckks_wpow(const double2* __restrict__ wtab, unsigned e, unsigned N)
{
  e &= 2 * N - 1;
  double2 w = wtab[e & (N - 1)];
  if (e >= N)
    w = make_double2(-w.x, -w.y);
  return w;
}

// real coefficients f[row][N] -> slots[row][N/2]
__global__ void __launch_bounds__(NORM_THREADS)
ckks_embed_kernel(const double* __restrict__ f, const double2* __restrict__ wtab, const uint32_t* __restrict__ jinfo,
                  int logn, int logh, double2* __restrict__ slots)
{
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const unsigned N = 1u << logn, H = 1u << logh, S = N >> logh;
  double* re = sm;
  double* im = sm + H;
  const unsigned row = blockIdx.x / S, s = blockIdx.x % S;
  const unsigned tid = threadIdx.x, nth = blockDim.x;
  const double* fr = f + (size_t)row * N;
  // h_i = sum_t f_n W^(n (2s+1)), n = i + tH
  for (unsigned i = tid; i < H; i += nth) {
    double ar = 0, ai = 0;
    for (unsigned t = 0; t < S; t++) {
      const unsigned n = i + t * H;
      const double2 w = ckks_wpow(wtab, n * (2 * s + 1), N);
      const double x = fr[n];
      ar += x * w.x;
      ai += x * w.y;
    }
    re[i] = ar;
    im[i] = ai;
  }
  __syncthreads();
  // H-point root omega^S = W^(2N/H): the table stride dif_fft_lds expects for tw_half = N
  dif_fft_lds(re, im, logh, N, wtab, tid, nth);
  double2* out = slots + (size_t)row * (N >> 1);
  for (unsigned p = tid; p < H; p += nth) {
    const unsigned j = s + S * (__brev(p) >> (32 - logh));
    const uint32_t u = jinfo[j];
    if (!(u & CKKS_CONJ))
      out[u] = make_double2(re[p], im[p]);
  }
}

// slots v[row][nslots] (missing slots are 0) -> coef[row][N] = round(Re(W^k Y_k) * scale), scale = scaling/N.
// A value that does not fit an int64 sets *overflow (the reference's "overflow in encoding") and is stored as 0.
__global__ void __launch_bounds__(NORM_THREADS)
ckks_encode_kernel(const double2* __restrict__ v, unsigned nslots, const double2* __restrict__ wtab,
                   const uint32_t* __restrict__ jinfo, int logn, int logh, double scale, int64_t* __restrict__ coef,
                   unsigned* __restrict__ overflow)
{
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const unsigned N = 1u << logn, H = 1u << logh, S = N >> logh;
  double* re = sm;
  double* im = sm + H;
  const unsigned row = blockIdx.x / S, s = blockIdx.x % S;
  const unsigned tid = threadIdx.x, nth = blockDim.x;
  const double2* vr = v + (size_t)row * nslots;
  // h_i = sum_t x_n omega^(n s) = sum_t x_n W^(2 n s), n = i + tH
  for (unsigned i = tid; i < H; i += nth) {
    double ar = 0, ai = 0;
    for (unsigned t = 0; t < S; t++) {
      const unsigned n = i + t * H;
      const uint32_t u = jinfo[n];
      const unsigned sl = u & ~CKKS_CONJ;
      if (sl >= nslots)
        continue;
      const double2 x = vr[sl];
      const double xr = x.x, xi = (u & CKKS_CONJ) ? x.y : -x.y;
      const double2 w = ckks_wpow(wtab, 2 * n * s, N);
      ar += xr * w.x - xi * w.y;
      ai += xr * w.y + xi * w.x;
    }
    re[i] = ar;
    im[i] = ai;
  }
  __syncthreads();
  dif_fft_lds(re, im, logh, N, wtab, tid, nth);
  int64_t* out = coef + (size_t)row * N;
  bool bad = false;
  for (unsigned kq = tid; kq < H; kq += nth) {   // natural output order: stride-S stores
    const unsigned p = __brev(kq) >> (32 - logh), k = s + S * kq;
    const double2 w = wtab[k];
    double y = round((re[p] * w.x - im[p] * w.y) * scale);   // std::round: halves away from zero
    // a long holds [-2^63, 2^63): the reference's round trip f[i] != f_i
    if (!(y >= -9223372036854775808.0 && y < 9223372036854775808.0)) {
      bad = true;
      y = 0;
    }
    out[k] = (int64_t)y;
  }
  if (bad)
    atomicOr(overflow, 1u);
}

// coef[i] (i < words = batch*N) -> rows[r][i] = coef[i] mod q_r, canonical; qm[r] = (q, floor(2^64/q))
__global__ void __launch_bounds__(256)
ckks_residues_kernel(const int64_t* __restrict__ coef, size_t words, const ulonglong2* __restrict__ qm, int nrows,
                     uint64_t* __restrict__ rows)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= words)
    return;
  const int64_t x = coef[i];
  const uint64_t ax = x < 0 ? (uint64_t)0 - (uint64_t)x : (uint64_t)x;
  for (int r = 0; r < nrows; r++) {
    const ulonglong2 c = qm[r];
    const uint64_t a = red64(ax, c.x, c.y);
    rows[(size_t)r * words + i] = (x < 0 && a) ? c.x - a : a;
  }
}

// DecryptCKKS (include/helib_amd_keys.hpp) on the device: coefficient rows[k][i] (k < n primes, i < words) ->
// out[i] = centred CRT value / ratFactor.  Garner digits a_k (value = a_0 + a_1 q_0 + a_2 q_0 q_1 + ...), the sign
// from value/Q > 1/2, then sum_k d_k P_k / ratFactor with P_k = prod_(j<k) q_j, the weights given as
// wm_k 2^we_k = P_k / ratFactor (they may exceed the double range; a digit that is 0 contributes nothing).
struct CkksCrtTab {
  ulonglong2 qm[CKKS_MAXPRIMES];   // (q_k, floor(2^64/q_k))
  double wm[CKKS_MAXPRIMES];
  int we[CKKS_MAXPRIMES];
};
template <int NMAX>
__global__ void __launch_bounds__(256)
ckks_crt_double_kernel(const uint64_t* __restrict__ rows, size_t words, int n, const CkksCrtTab* __restrict__ tab,
                       const ulonglong2* __restrict__ ginv /* [k*n + l] = (q_l^-1 mod q_k, its Shoup factor) */,
                       double* __restrict__ out)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= words)
    return;
  uint64_t a[NMAX];
#pragma unroll
  for (int k = 0; k < NMAX; k++) {
    if (k < n) {
      const ulonglong2 c = tab->qm[k];
      uint64_t x = rows[(size_t)k * words + i];
#pragma unroll
      for (int l = 0; l < NMAX; l++) {
        if (l < k) {
          const ulonglong2 g = ginv[k * n + l];
          x = mul_shoup(sub_mod(x, red64(a[l], c.x, c.y), c.x), g.x, g.y, c.x);
        }
      }
      a[k] = x;
    }
  }
  double frac = 0;   // value / Q
#pragma unroll
  for (int k = 0; k < NMAX; k++)
    if (k < n)
      frac = (frac + (double)a[k]) / (double)tab->qm[k].x;
  const bool neg = frac > 0.5;
  double v = neg ? ldexp(tab->wm[0], tab->we[0]) : 0.0;   // Q - value = (Q - 1 - value) + 1
#pragma unroll
  for (int k = 0; k < NMAX; k++) {
    if (k < n) {
      const uint64_t d = neg ? tab->qm[k].x - 1 - a[k] : a[k];
      if (d)
        v += ldexp((double)d * tab->wm[k], tab->we[k]);
    }
  }
  out[i] = neg ? -v : v;
}

}  // namespace hx
