// norm_r16.h -- register-tiled form of the canonical-embedding norm for N = 2^14 (the benchmark ring) and 2^15:
// the 8192-point complex transform of the "quarter" trick (norm_kernels.h, src/norms.cpp:200-262) as
// THREE radix-16 register passes of 512 threads x 16 points, the last stage as a lane exchange, and a pairing
// pass that forms every pair once.  The round-1/2 kernel (embed_norm_quarter_kernel) makes seven radix-4
// passes through LDS with 1024 threads x 2 butterflies each, nine barriers, every pass exposing an LDS
// round trip per two stages: 40 us per element on a CU against 7.5 us of LDS bandwidth.
//
// Decimation in frequency, output in bit-reversed order (only maxima are taken).  Stage with half-length
// len: (a, b) = (x[k], x[k+len]) -> x[k] = a + b, x[k+len] = (a - b) T_len(j), j = k mod len,
// T_len(j) = W^(j N / len) = wtab[j N/len]  (N = 16384, W = exp(2 pi i / 2N) ... as dif_fft_lds).
//   pass A  len = 4096, 2048, 1024, 512   positions  t + 512 k            (t < 512,  k < 16)
//   pass B  len =  256,  128,   64,  32   positions  512 b + j + 32 k     (b = t>>5, j = t&31)
//   pass C  len =   16,    8,    4,   2   positions   32 b + j +  2 k     (b = t>>1, j = t&1)
//   stage len = 1 between lanes t and t ^ 1: Z[p] = x[p] + x[p+1] (p even), x[p-1] - x[p] (p odd)
// Between the passes the real parts cross ONE padded array (index i stored at i + (i >> 5): pass C's stride-32
// block starts then fall on different banks), then the imaginary parts: 66 KiB, two workgroups per CU.
// The phase functions are plain C++ (HXD) so that tests/cpp/norm_replay.cpp runs them thread by thread
// on the CPU against the definition.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#ifndef HXD
#if defined(__HIPCC__)
#define HXD __host__ __device__ __forceinline__
#else
#define HXD inline
#endif
#endif

namespace hx {

struct cplx16 {
  double x, y;
};
struct tw16 {   // layout-compatible with double2
  double x, y;
};
constexpr unsigned R16_LOGN = 14, R16_N = 1u << R16_LOGN, R16_M = R16_N >> 1, R16_THREADS = 512;
constexpr unsigned R16_LDS_DOUBLES = R16_M + (R16_M >> 5);   // one of the two arrays (re / im), padded
HXD unsigned r16_pad(unsigned i) { return i + (i >> 5); }

HXD tw16 r16_cmul(tw16 a, tw16 b) { return tw16{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
// four DIF stages on 16 points S apart (S = 2^LOGS): v[k] <-> position base + j0 + S k, j0 < S.
// LOGTAB: log2 of the twiddle table's size (T_len(j) = wtab[j 2^LOGTAB / len]): 14 for N = 2^14; 15 when the
// 8192-point transform is one of the two sub-transforms of N = 2^15 (embed_norm_r16_split_kernel).
// Twiddles: the stage with len = S h multiplies position j0 + S k' (k' < h) by
//   T = W^((j0 + S k') 2^LOGTAB / (S h)) = B_h * exp(pi i k' / h),   B_h = W^(j0 2^LOGTAB / (S h)),
// so ONE table entry per pass and thread is loaded (B_8; B_4 = B_8^2, B_2 = B_4^2, B_1 = B_2^2) and the
// rest are its products with the 16th roots of unity exp(pi i k / 8), read from the table at wave-uniform
// addresses (wtab[k 2^LOGTAB / 8]) -- the first version loaded all 15 twiddles of a pass per thread from the
// strided table and was latency-bound on them (slower than the LDS-pass kernel it was to replace).
// TAB: anything that gives a tw16 by value for an index (a plain pointer; R16ConstTab below on the device).
template <int LOGS, int LOGTAB = 14, class TAB = const tw16*>
HXD void r16_pass(cplx16 (&v)[16], unsigned j0, TAB wtab)
{
  constexpr unsigned S = 1u << LOGS;
  tw16 B = wtab[j0 * ((1u << LOGTAB) / (S * 8u))];
#pragma unroll
  for (unsigned h = 8; h >= 1; h >>= 1) {
#pragma unroll
    for (unsigned k = 0; k < 16; k++) {
      if (k & h)
        continue;
      const unsigned kp = k & (h - 1);
      // exp(pi i kp / h) = W^(kp 2^LOGTAB / h)
      const tw16 T = kp == 0 ? B : r16_cmul(B, wtab[kp * ((1u << LOGTAB) / h)]);
      const cplx16 a = v[k], b = v[k + h];
      const double dx = a.x - b.x, dy = a.y - b.y;
      v[k].x = a.x + b.x;
      v[k].y = a.y + b.y;
      v[k + h].x = dx * T.x - dy * T.y;
      v[k + h].y = dx * T.y + dy * T.x;
    }
    B = r16_cmul(B, B);
  }
}
// where thread t keeps its 16 points of each pass: position of v[k]
HXD unsigned r16_pos_A(unsigned t, unsigned k) { return t + 512u * k; }
HXD unsigned r16_pos_B(unsigned t, unsigned k) { return 512u * (t >> 5) + (t & 31u) + 32u * k; }
HXD unsigned r16_pos_C(unsigned t, unsigned k) { return 32u * (t >> 1) + (t & 1u) + 2u * k; }

// max of |f|^2 at the two evaluation points that Z_j = z and Z_(M-1-j) = partner give, w = W^(2j+1)
// (embed_norm_quarter_kernel's formula)
HXD double r16_pair_norm2(cplx16 z, cplx16 partner, tw16 w)
{
  const double cr = partner.x, ci = -partner.y;
  const double er = 0.5 * (z.x + cr), ei = 0.5 * (z.y + ci);
  const double dr = z.x - cr, di = z.y - ci;
  const double orr = 0.5 * di, oi = -0.5 * dr;
  const double tr = orr * w.x - oi * w.y, ti = orr * w.y + oi * w.x;
  const double a = (er + tr) * (er + tr) + (ei + ti) * (ei + ti);
  const double b = (er - tr) * (er - tr) + (ei - ti) * (ei - ti);
  return a > b ? a : b;
}
HXD unsigned r16_brev4(unsigned i) { return ((i & 1u) << 3) | ((i & 2u) << 1) | ((i & 4u) >> 1) | ((i & 8u) >> 3); }
// ---- the last stage and the pairing ----
// After pass C thread t holds
// positions p = 32 (t>>1) + (t&1) + 2k: the partner p ^ 1 of the last stage (len = 1) is the same k of lane t ^ 1,
// so that stage is a lane exchange and the finished Z stay in registers:
HXD cplx16 r16_last_lane(cplx16 own, cplx16 other, unsigned t)   // other: the value lane t ^ 1 holds at the same k
{
  return (t & 1u) ? cplx16{other.x - own.x, other.y - own.y} : cplx16{own.x + other.x, own.y + other.y};
}
// Pairing: Z at p meets Z at M - 1 - p = pos_C(511 - t, 15 - k); (p, M-1-p) and (M-1-p, p) give the same two
// evaluation points, so thread t pairs its k < 8 with what thread 511 - t holds at 15 - k >= 8 -- every unordered
// pair once (the two-array kernel formed each twice).  The upper halves cross through the array at
// [kk][t], kk = k - 8 (real parts; imaginary parts R16_XCHG_IM further on).
constexpr unsigned R16_XCHG_IM = 4096;
HXD unsigned r16_xchg_idx(unsigned t, unsigned kk) { return kk * 512u + t; }
HXD unsigned r16_brev8(unsigned x)
{
  unsigned r = 0;
  for (int i = 0; i < 8; i++)
    r |= ((x >> i) & 1u) << (7 - i);
  return r;
}
// j = brev13(p) = 4096 (t&1) + 256 brev4(k) + brev8(t>>1):  W^(2j+1) = wtab[r16_pair_tw_thread(t)] * wtab[r16_pair_tw_k(k)]
HXD unsigned r16_pair_tw_thread(unsigned t) { return 8192u * (t & 1u) + 2u * r16_brev8(t >> 1) + 1u; }
HXD unsigned r16_pair_tw_k(unsigned k) { return 512u * r16_brev4(k); }

// ---- the direct form: no pairing pass ----
// Split f by HALVES instead of by parity.  With M = N/2, W^M = i and W^(4jM) = 1:
//   f(W^(4j+1)) = sum_{p<M} (f_p + i f_(p+M)) W^p exp(2 pi i jp / M),   j < M,
// the SAME M-point transform (root W^4, passes A/B/C and the lane stage above) of z_p = (f_p + i f_(p+M)) W^p, and
// every output is an evaluation of f itself -- at W^(4j+1), one from each conjugate pair of the primitive 2N-th
// roots (W^(4j+3) = conj W^(4(M-1-j)+1)), and |f| is the same at both of a pair because f is real.  The norm is
// max_j |Z_j|: no partner, no exchange through the array, no pairing twiddles.  Pass A's thread t takes f at
// t + 512 k and t + 512 (k + 16): of the row transform's inverse (ntt_core.h: coef_const<14>(e) = 512 e) these are
// the thread's OWN registers e = k and e = k + 16, which is what lets the mod-switch prep kernel go on into the norm
// without a data exchange (ntt_kernels.hip: PrepFuseIO).
// Load twist W^(t + 512 k) = wtab[t] * wtab[512 k]: one table entry per thread, 16 wave-uniform constants.
HXD unsigned r16_direct_tw_k(unsigned k) { return 512u * k; }
HXD cplx16 r16_direct_twist(double lo, double hi, tw16 wth, tw16 wk, unsigned k)   // lo = f_p, hi = f_(p+M), p = t + 512 k
{
  const tw16 w = k == 0 ? wth : r16_cmul(wth, wk);
  return cplx16{lo * w.x - hi * w.y, lo * w.y + hi * w.x};
}
HXD double r16_abs2(cplx16 z) { return z.x * z.x + z.y * z.y; }

// N = 2^15 as S = 2 sub-transforms of H = 8192 points (norm_kernels.h, embed_norm_quarter_split_kernel):
// input point i of sub-transform `sub`: h_i = sum_{t<2} z_(i+tH) U^((i+tH) sub),
//   z_n U^(n sub) = (f_2n + i f_(2n+1)) W^(2n (2 sub + 1)),  W = exp(2 pi i / 2N),  wtab[k] = W^k for k < N
HXD cplx16 r16_split_input(const double* f, const tw16* wtab, unsigned i, unsigned sub)
{
  constexpr unsigned N = 1u << 15, H = 8192u, mmask = 2u * N - 1u;
  cplx16 acc{0.0, 0.0};
  for (unsigned t = 0; t < 2; t++) {
    const unsigned idx = i + t * H;
    const unsigned e = (2u * idx * (2u * sub + 1u)) & mmask;
    const tw16 w = wtab[e & (N - 1u)];
    const double vx = f[2 * idx], vy = f[2 * idx + 1];
    const double zr = vx * w.x - vy * w.y, zi = vx * w.y + vy * w.x;
    acc.x += e >= N ? -zr : zr;
    acc.y += e >= N ? -zi : zi;
  }
  return acc;
}
// N = 2^15 with both sub-transforms at once (embed_norm_r16x2_kernel): 1024 threads, half h = sub-transform h in its
// own array; after the lane-exchange stage Z_h sits in registers at pos_C(t, k).  Z0 at p meets Z1 at 8191 - p, i.e.
// what thread 511 - t of the OTHER half holds at 15 - k: half 0 forms the pairs of its k < 8, half 1 those of its
// own k < 8 (the pairs of half 0's k >= 8) -- every pair once, the upper halves crossing through the arrays as in the
// N = 2^14 kernel.  Twiddle W^(4 brev13(p) + 1) for the Z0 position p of the pair (W = exp(2 pi i / 2^16)):
//   half 0, own p:        4 j + 1,       j = 4096 (t&1) + 256 brev4(k) + brev8(t>>1)
//   half 1, p = 8191 - p': 32765 - 4 j'  (j' from its own t, k) = thread part * conj(W^(1024 brev4(k)))
HXD unsigned r16x2_pair_tw_thread(unsigned h, unsigned t)
{
  const unsigned a = 16384u * (t & 1u) + 4u * r16_brev8(t >> 1);
  return h ? 32765u - a : a + 1u;
}
HXD unsigned r16x2_pair_tw_k(unsigned k) { return 1024u * r16_brev4(k); }
HXD double r16x2_pair(unsigned h, cplx16 own, cplx16 other, tw16 wth, tw16 wk, unsigned k)
{
  const tw16 u = h ? tw16{wk.x, -wk.y} : wk;
  const tw16 w = k == 0 ? wth : r16_cmul(wth, u);
  return h ? r16_pair_norm2(other, own, w) : r16_pair_norm2(own, other, w);
}

#if defined(__HIPCC__)
// ---- device side of the phases above, shared by the norm kernels (norm_kernels.h) and by the mod-switch prep
// kernels that carry the norm in their own workgroup (ntt_kernels.hip) ----
__device__ __forceinline__ void block_max_to(double mx, double* sm, unsigned tid, unsigned nth,
                                             unsigned long long* dst, bool direct = false)
{
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(mx, off, 64);
    mx = o > mx ? o : mx;
  }
  __syncthreads();
  if ((tid & 63u) == 0)
    sm[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    const unsigned nw = (nth + 63) >> 6;
    for (unsigned w = 1; w < nw; w++)
      mx = sm[w] > mx ? sm[w] : mx;
    // direct: this workgroup is the only writer of *dst (one workgroup per polynomial) -- a plain store, which may go
    // to device-visible host memory; otherwise several workgroups meet in a zeroed word
    if (direct)
      *dst = (unsigned long long)__double_as_longlong(mx);
    else
      atomicMax(dst, (unsigned long long)__double_as_longlong(mx));
  }
}
__device__ __forceinline__ double lane_xor1(double v)
{
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, true);   // quad_perm [1, 0, 3, 2]
  hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// FROM -> TO: positions of the 16 values before / after (r16_pos_A / _B / _C)
template <unsigned (*FROM)(unsigned, unsigned), unsigned (*TO)(unsigned, unsigned)>
__device__ __forceinline__ void r16_transpose(cplx16 (&v)[16], double* sm, unsigned t)
{
#pragma unroll
  for (unsigned k = 0; k < 16; k++)
    sm[r16_pad(FROM(t, k))] = v[k].x;
  __syncthreads();
#pragma unroll
  for (unsigned k = 0; k < 16; k++)
    v[k].x = sm[r16_pad(TO(t, k))];
  __syncthreads();
#pragma unroll
  for (unsigned k = 0; k < 16; k++)
    sm[r16_pad(FROM(t, k))] = v[k].y;
  __syncthreads();
#pragma unroll
  for (unsigned k = 0; k < 16; k++)
    v[k].y = sm[r16_pad(TO(t, k))];
}
// The table behind a constant-address-space pointer.  A kernel that has stored to global memory before it reads the
// table (the prep kernels: x and S) gets its wave-uniform entries as VECTOR loads through a plain pointer -- the
// compiler cannot rule the stores out as writers of the table -- four registers per constant, some sixty per pass;
// from the constant address space they are scalar loads, as in a kernel that stores nothing first.  (The table is
// written once, when the context makes it.)
struct R16ConstTab {
  const double __attribute__((address_space(4)))* p;
  __device__ explicit R16ConstTab(const double* q) : p((const double __attribute__((address_space(4)))*)(uintptr_t)q) {}
  __device__ __forceinline__ tw16 operator[](unsigned i) const { return tw16{p[2u * i], p[2u * i + 1u]}; }
};
// the direct form from the twisted points (v[k] at r16_pos_A(t, k)) to the thread's largest |Z|^2
template <class TAB>
__device__ __forceinline__ double r16_direct_max2(cplx16 (&v)[16], double* sm, unsigned t, TAB wt)
{
  r16_pass<9>(v, t, wt);
  r16_transpose<r16_pos_A, r16_pos_B>(v, sm, t);
  r16_pass<5>(v, t & 31u, wt);
  __syncthreads();
  r16_transpose<r16_pos_B, r16_pos_C>(v, sm, t);
  r16_pass<1>(v, t & 1u, wt);
  double mx = 0;
#pragma unroll
  for (unsigned k = 0; k < 16; k++) {
    const double n2 = r16_abs2(r16_last_lane(v[k], cplx16{lane_xor1(v[k].x), lane_xor1(v[k].y)}, t));
    mx = n2 > mx ? n2 : mx;
  }
  return mx;
}
#endif

}  // namespace hx
