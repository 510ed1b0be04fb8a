// fft_lds.h -- the complex-double DFT held in LDS that the canonical-embedding kernels share: the norm kernels
// (norm_kernels.h) and CKKS slot encoding (ckks_slots.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hx {

constexpr int NORM_MAX_LOGH = 13;  // 2^13 complex doubles = 128 KiB LDS
constexpr int NORM_THREADS = 1024;

struct cplx {
  double x, y;
};
__device__ __forceinline__ cplx cmul(cplx a, double2 w) { return {a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cplx cmul_i(cplx a) { return {-a.y, a.x}; }

// In-place decimation-in-frequency DFT of the H = 2^logh points in (re, im).  Both callers use a
// root for which the stage of half-length len multiplies position j by W^(j*N/len) = wtab[j*N/len]
// (N = table size): the H-point root is W^(2N/H).
// Two stages are fused into one radix-4 pass (one barrier, one LDS round trip per two stages):
//   stage len  : x0=a0+a2, x2=(a0-a2)T, x1=a1+a3, x3=(a1-a3)T*i      (T = T_len(j), T_len(j+len/2) = i T)
//   stage len/2: y0=x0+x1, y1=(x0-x1)T2, y2=x2+x3, y3=(x2-x3)T2     (T2 = T_(len/2)(j))
// Output order is bit-reversed; the norm callers only take maxima (or pair positions p and H-1-p), the CKKS slot
// kernels place each output through the bit reversal.
// CLOGH / CNTH: compile-time transform size and thread count (0 = take the runtime arguments).  With
// both known the loops over a thread's butterflies have constant trip counts and are unrolled, so that
// the twiddle and LDS loads of all of a thread's butterflies in a pass are in flight together -- with
// runtime bounds every iteration exposed its own global-memory round trip (the norm kernels were
// latency-bound: 40 us per 8192-point transform, one workgroup per CU).
template <int CLOGH = 0, int CNTH = 0>
__device__ __forceinline__ void dif_fft_lds(double* re, double* im, int logh_rt, unsigned tw_half,
                                            const double2* __restrict__ wtab, unsigned tid, unsigned nth_rt)
{
  // tw_half: the table size N
  const int logh = CLOGH ? CLOGH : logh_rt;
  const unsigned nth = CNTH ? (unsigned)CNTH : nth_rt;
  const unsigned H = 1u << logh;
  int stages = logh;
  unsigned len = H >> 1;
#pragma unroll
  while (stages >= 2) {
    const unsigned hl = len >> 1;        // j < len/2
    const unsigned s1 = tw_half / len;   // T_len(j)      = wtab[j * s1]
    const unsigned s2 = s1 * 2;          // T_(len/2)(j)  = wtab[j * s2]
#pragma unroll
    for (unsigned q = tid; q < (H >> 2); q += nth) {
      const unsigned j = q & (hl - 1), blk = q / hl, k = blk * 2 * len + j;
      const cplx a0{re[k], im[k]}, a1{re[k + hl], im[k + hl]}, a2{re[k + len], im[k + len]},
          a3{re[k + len + hl], im[k + len + hl]};
      const double2 T = wtab[j * s1], T2 = wtab[j * s2];
      const cplx x0 = cadd(a0, a2), x2 = cmul(csub(a0, a2), T);
      const cplx x1 = cadd(a1, a3), x3 = cmul_i(cmul(csub(a1, a3), T));
      const cplx y0 = cadd(x0, x1), y1 = cmul(csub(x0, x1), T2);
      const cplx y2 = cadd(x2, x3), y3 = cmul(csub(x2, x3), T2);
      re[k] = y0.x, im[k] = y0.y;
      re[k + hl] = y1.x, im[k + hl] = y1.y;
      re[k + len] = y2.x, im[k + len] = y2.y;
      re[k + len + hl] = y3.x, im[k + len + hl] = y3.y;
    }
    __syncthreads();
    len >>= 2;
    stages -= 2;
  }
  if (stages == 1) {  // len == 1: twiddle 1
#pragma unroll
    for (unsigned k2 = tid; k2 < (H >> 1); k2 += nth) {
      const unsigned k = 2 * k2;
      const double ar = re[k], ai = im[k], br = re[k + 1], bi = im[k + 1];
      re[k] = ar + br, im[k] = ai + bi;
      re[k + 1] = ar - br, im[k + 1] = ai - bi;
    }
    __syncthreads();
  }
}

}  // namespace hx
