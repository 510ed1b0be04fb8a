// bgv_slots.h -- device kernels of BGV slot encoding and decoding for d = ord_m(p) = 1 (bgv_slots.hip).
//
// With p = 1 mod m the slots of EncryptedArray are the values of the plaintext polynomial at the primitive m-th
// roots of unity modulo p, i.e. one row of the engine's transform for the prime p in another order.  The transform
// itself is the engine's (a side context holding p); the kernels here are the glue around it, all streaming:
//   bgv_scatter_kernel  slots -> row order, reduced mod p      reads 8 B/slot (random inside one row) + 4 B index,
//                                                              writes 8 B/word coalesced
//   bgv_diag_scatter_kernel  the same for a diagonal of a device-resident matrix: 4 B index + 8 B matrix word per word
//                                                              (one word per 128 B line at worst), writes 8 B/word coalesced
//   bgv_lift_kernel     coefficients mod p -> balanced(mul * h mod p) modulo every prime of the output
//                                                              reads 8 B/word once, writes 8 L B/word (+ 8 for the zzX)
//   bgv_redmul_kernel   signed words -> (w mod p) * f mod p    reads 8, writes 8 B/word
//   bgv_gather_kernel   row order -> slot order                reads 8 B/word (random inside one row) + 4 B index,
//                                                              writes 8 B/word coalesced
// The streaming sides use 16-byte accesses (two words per lane) when the buffers allow it; grids are capped and
// stride (BGV_MAX_BLOCKS).  Two units include this header (bgv_slots.hip, bgv_crt.hip): the kernels that are no templates
// have internal linkage.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hx {

constexpr int BGV_MAXPRIMES = 512;       // rows of an encode's output (the chain plus the special primes)
constexpr unsigned BGV_MAX_BLOCKS = 2048;
constexpr uint32_t BGV_NO_SLOT = 0xffffffffu;

// x mod q for any x < 2^64 and any modulus q >= 2 (prime or not), mu = floor(2^64 / q): the quotient estimate is short
// by at most 1
__device__ __forceinline__ uint64_t bgv_red(uint64_t x, uint64_t q, uint64_t mu)
{
  uint64_t r = x - __umul64hi(x, mu) * q;
  return r >= q ? r - q : r;
}
// the residue in [0, q) of a signed word
__device__ __forceinline__ uint64_t bgv_red_signed(int64_t v, uint64_t q, uint64_t mu)
{
  const uint64_t a = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
  const uint64_t r = bgv_red(a, q, mu);
  return (v < 0 && r) ? q - r : r;
}
// x * w mod q, x < q, ws = floor(w 2^64 / q)
__device__ __forceinline__ uint64_t bgv_mul_shoup(uint64_t x, uint64_t w, uint64_t ws, uint64_t q)
{
  uint64_t r = x * w - __umul64hi(x, ws) * q;
  return r >= q ? r - q : r;
}

// rows[b][j] = slots[b][row2slot[j]] mod p (0 where the row position holds a slot >= nslots): one thread per word
static __global__ void __launch_bounds__(256)
bgv_scatter_kernel(const int64_t* __restrict__ slots, uint32_t nslots, const uint32_t* __restrict__ row2slot, uint32_t N,
                   size_t words, uint64_t p, uint64_t mu, uint64_t* __restrict__ rows)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
    const size_t b = i / N;
    const uint32_t s = row2slot[i - b * N];
    rows[i] = s < nslots ? bgv_red_signed(slots[b * nslots + s], p, mu) : 0;
  }
}

// The hypercube of the slots, by value: slot s has coordinate (s / stride[i]) % ord[i] in dimension i (the last
// dimension fastest).  dim = -1: the matrix is phi(m) x phi(m), indexed by slot; dim = i: ord[i] x ord[i], indexed by
// the coordinate in dimension i.
struct BgvDiagGeom {
  int32_t nd, dim;
  uint32_t ord[8], stride[8];
  uint32_t cols;
};
// one diagonal (hx_bgv_diag with off[i] and rot_amt brought into [0, ord) by the host)
struct BgvDiag {
  int32_t off[8];
  int32_t rot_dim, rot_amt;
};

// rows[t][j] = A[.] mod p, the slot row2slot[j] of diagonal t read straight out of the matrix (MatMul1D's
// processDiagonal1 / MatMulFullHelper::processDiagonal, then plaintextAutomorph, src/matmul.cpp:449-504, 1998-2024,
// 375-389): with c the coordinates of the slot, c[rot_dim] -= rot_amt gives the slot s0 the value comes from,
//   full matrix    A[r, s0],  r the slot with coordinates c_i(s0) - off[i]
//   dimension dim  A[c_dim(s0) - off[dim], c_dim(s0)]
// all mod the orders.  One thread per word; rows = nullptr only raises the flags.  nz[t] |= 1 where a word is non-zero
// (a vector atomic, skipped once the flag is seen set).  Per word: 4 B index + 8 B matrix word, one per 128 B line in
// the worst case, + 8 B coalesced store; the descriptors are 40 B per diagonal, cached.
static __global__ void __launch_bounds__(256)
bgv_diag_scatter_kernel(const int64_t* __restrict__ A, BgvDiagGeom g, const BgvDiag* __restrict__ diags,
                        const uint32_t* __restrict__ row2slot, uint32_t N, size_t words, uint64_t p, uint64_t mu,
                        uint64_t* __restrict__ rows, uint32_t* nz)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
    const size_t t = i / N;
    const uint32_t s = row2slot[i - t * N];
    uint64_t w = 0;
    if (s < N) {
      const BgvDiag* d = diags + t;
      const int32_t rot_dim = d->rot_dim;
      const uint32_t rot_amt = (uint32_t)d->rot_amt;
      size_t s0 = 0, r = 0, cd = 0, rd = 0;
      for (int k = 0; k < g.nd; k++) {
        const uint32_t o = g.ord[k];
        uint32_t c = (s / g.stride[k]) % o;
        if (k == rot_dim) {
          c += o - rot_amt;
          c = c >= o ? c - o : c;
        }
        uint32_t rr = c + o - (uint32_t)d->off[k];
        rr = rr >= o ? rr - o : rr;
        s0 += (size_t)c * g.stride[k];
        r += (size_t)rr * g.stride[k];
        if (k == g.dim) {
          cd = c;
          rd = rr;
        }
      }
      const size_t at = g.dim < 0 ? r * g.cols + s0 : rd * g.cols + cd;
      w = bgv_red_signed(A[at], p, mu);
    }
    if (rows)
      rows[i] = w;
    if (w && __atomic_load_n(nz + t, __ATOMIC_RELAXED) == 0)
      atomicOr(nz + t, 1u);
  }
}

// out[b][s] = rows[b][slot2row[s]]
static __global__ void __launch_bounds__(256)
bgv_gather_kernel(const uint64_t* __restrict__ rows, const uint32_t* __restrict__ slot2row, uint32_t N, size_t words,
                  int64_t* __restrict__ out)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
    const size_t b = i / N;
    out[i] = (int64_t)rows[b * N + slot2row[i - b * N]];
  }
}

// out[i] = (in[i] mod p) * f mod p, f < p, fs its Shoup companion; V words per lane
template <int V>
__global__ void __launch_bounds__(256)
bgv_redmul_kernel(const int64_t* __restrict__ in, size_t words, uint64_t p, uint64_t mu, uint64_t f, uint64_t fs,
                  uint64_t* __restrict__ out)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x * V;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V; i < words; i += stride) {
    if (V == 2) {
      const longlong2 x = *reinterpret_cast<const longlong2*>(in + i);
      ulonglong2 y;
      y.x = bgv_mul_shoup(bgv_red_signed(x.x, p, mu), f, fs, p);
      y.y = bgv_mul_shoup(bgv_red_signed(x.y, p, mu), f, fs, p);
      *reinterpret_cast<ulonglong2*>(out + i) = y;
    } else {
      out[i] = bgv_mul_shoup(bgv_red_signed(in[i], p, mu), f, fs, p);
    }
  }
}

// The lift: c = balanced(mul * h[i] mod p) in (-p/2, p/2], rows[r][i] = c mod q_r for the L primes
// qm[r] = (q_r, floor(2^64 / q_r)); coeffs (optional) receives c itself.  One read, L coalesced writes.  p is any
// modulus below 2^63 (a prime, or p^r for Hensel-lifted slots).  An odd p has no tie.  At an even p a word equal to
// p/2 stays +p/2: the reference's balanced_zzX and balanced_MulMod draw that sign at random (src/zzX.cpp:122-137,
// 156-170; for p = 2, where every 1 is such a word, :139-154), both signs being the same residue; the project takes
// the positive one always, so that an encoding is a function of its input.
template <int V>
__global__ void __launch_bounds__(256)
bgv_lift_kernel(const uint64_t* __restrict__ h, size_t words, uint64_t p, uint64_t mul, uint64_t muls,
                const ulonglong2* __restrict__ qm, int L, uint64_t* __restrict__ rows, int64_t* __restrict__ coeffs)
{
  const uint64_t half = p >> 1;
  const size_t stride = (size_t)gridDim.x * blockDim.x * V;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * V; i < words; i += stride) {
    int64_t c[V];
    if (V == 2) {
      const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(h + i);
      c[0] = (int64_t)bgv_mul_shoup(x.x, mul, muls, p);
      c[V - 1] = (int64_t)bgv_mul_shoup(x.y, mul, muls, p);
    } else {
      c[0] = (int64_t)bgv_mul_shoup(h[i], mul, muls, p);
    }
#pragma unroll
    for (int k = 0; k < V; k++)
      if ((uint64_t)c[k] > half)
        c[k] -= (int64_t)p;
    if (coeffs) {
      if (V == 2)
        *reinterpret_cast<longlong2*>(coeffs + i) = make_longlong2(c[0], c[V - 1]);
      else
        coeffs[i] = c[0];
    }
    for (int r = 0; r < L; r++) {
      const ulonglong2 q = qm[r];   // uniform over the wave: a scalar load
      uint64_t* dst = rows + (size_t)r * words + i;
      if (V == 2)
        *reinterpret_cast<ulonglong2*>(dst) = make_ulonglong2(bgv_red_signed(c[0], q.x, q.y), bgv_red_signed(c[V - 1], q.x, q.y));
      else
        *dst = bgv_red_signed(c[0], q.x, q.y);
    }
  }
}

}  // namespace hx
