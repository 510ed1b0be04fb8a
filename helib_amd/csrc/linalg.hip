// linalg.hip -- C ABI of the fused multiply-add of the matrix product (include/helib_amd.h: hx_mul_add_many):
//   out0 (+)= sum_t c[t] * in0[t],  out1 (+)= sum_t c[t] * in1[t]
// the inner loop of MatMul1DExec::mul, n x MulAdd (src/matmul.cpp:391-408: tmp = b; tmp *= a; x += tmp, the product
// being DoubleCRT::Mul with matchIndexSets = false), in one pass over the data; and of the mask split of the
// linear-array rotate / shift (hx_mask_split):
//   take = keep * mask,  keep -= take
// (src/EncryptedArray.cpp:270-274: tmp = ctxt; tmp.multByConstant(mask); ctxt -= tmp), in one pass as well; and of the
// tail of the non-native rotate1D (hx_mask_blend):
//   c = c * mask + t - t * mask
// (src/EncryptedArray.cpp:120-124), one pass instead of four; and of the inner step of digit extraction
// (hx_scaled_sub):
//   c = c * u - t * v,  u and v one scalar per prime row
// (src/extractDigits.cpp:106-107: tmp -= digits[j]; tmp.divideByP()), one pass instead of four; and of the leaf of
// polyEval (hx_lin_comb):
//   out = sum_t w[t] * in[t] + addend,  the terms on prime sets of their own, w and the addend one scalar per prime row
// (src/polyEval.cpp:240-253: tmp = X^i; tmp.multByConstant(f_i); ret += tmp; then ret.addConstant), one read of every
// term and one write of the sum; and of the inner loop of unpack (hx_mul_add_circulant):
//   out[i] = sum_j c[(i + j) mod d] * in[j],  i < nout <= d
// (src/intraSlot.cpp:108-115: unpacked[i] = frob[0] * C[i]; then += frob[j] * C[(i + j) mod d]), the d Frobenius images
// read once per block of outputs instead of once per output; and of the hoisted loop of traceMap
// (hx_hoisted_automorph_sum):
//   out = ctxt + sum_t keySwitch(sigma_k[t](ctxt)),  the digits of the s-part broken once
// (src/matmul.cpp:2878-2887: acc += *precon.automorph(p^i)), every digit word and key word read once per term and the two
// outputs written once; and of the mask stage of a permutation-network layer (hx_mask_fan):
//   out[k] = c * mask[k],  k < K
// (src/PermNetwork.cpp:239-242: tmp = c; tmp.multByConstant(mask_k) per shift amount), c read once for the K products;
// and of the loop of innerProduct before its relinearisation (hx_tensor_sum):
//   (o0, o1, o2) = sum_t tensor((a0[t], a1[t]), (b0[t], b1[t]))
// (src/Ctxt.cpp:2885-2891: tmp = *v1[i]; tmp.multLowLvl(*v2[i]); result += tmp), the 4 n operand rows read once and the
// three parts of the sum written once; and of the last level of computeAllProducts with the weighted sum of tableLookup
// in front of ONE relinearisation (hx_table_tensor_sum):
//   (o0, o1, o2) = sum_(i<k, j<l) T[j k + i] tensor((a0[i], a1[i]), (b0[j], b1[j]))
// (src/tableLookup.cpp:261-267: *products[ii] = products1[i]; products[ii]->multiplyBy(products2[j]); and :94-103:
// products[i].multByConstant(table[i]); out += products[i]), every a read once per four values of j and every table word
// once per two batch elements; and of an inner node of replicateAll's recursion over one digit decomposition
// (hx_hoisted_mask_fan):
//   out[t] = A[t] * ctxt + B[t] * keySwitch(sigma_k[t](ctxt)),  t < n
// (src/replicate.cpp:432-483 and :411-415 over BasicAutomorphPrecon, src/matmul.cpp:48-184), every digit word and key
// word read once per term, the ciphertext once for all terms, each output written once; and of the inner step of
// MatMulFullExec's recursion along a non-native dimension over two digit decompositions (hx_hoisted_blend):
//   out[t] = M[t] * X + Y - M[t] * Y,  X = keySwitch(sigma_k[t](ctxt)),  Y = keySwitch(sigma_k[t](ctxt1)),  t < n
// (src/matmul.cpp:2174-2204), every digit word of both blocks and every key word read once per term, each output written
// once.
// The unit reaches the context only through ckks_bridge.h (stream, lock, a state slot, the prime table, a poly's rows, a
// key-switching matrix's rows, the tables of Z_m^*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <vector>

#include "../../include/helib_amd.h"
#include "ckks_bridge.h"
#include "dev_common.h"
#include "hostmath.h"
#include "prof.h"

namespace hx {

// Products of canonical residues are accumulated unreduced in 128 bits.  With q <= QMAX = 2^60 - 1 (hx_ctx_add_prime
// admits primes below 2^60) the accumulator starts from a residue (the old output word, or the value the previous
// reduction left) and takes MAD_CHUNK products:
//   (q - 1) + MAD_CHUNK (q - 1)^2 <= (2^60 - 2) + 256 (2^60 - 2)^2 < 2^128,
// so one reduction per MAD_CHUNK = 256 terms, and one at the end, is enough.
constexpr int MAD_CHUNK = 256;
constexpr u128 MAD_QMAX = ((u128)1 << 60) - 1;
static_assert((~(u128)0 - (MAD_QMAX - 1)) / ((MAD_QMAX - 1) * (MAD_QMAX - 1)) >= (u128)MAD_CHUNK,
              "MAD_CHUNK products of residues and one residue must fit 128 bits");

struct MadRows {
  uint16_t p[MAX_ROWS];   // prime index of output row r
};

// x mod q for any 128-bit x: x = hi 2^64 + lo = (hi mod q)(2^64 mod q) + (lo mod q) (mod q), a value below
// q^2 + q < 8 q^2, which is red128_wide's domain.  2^64 mod q = 2^64 - mu64 q (mu64 = floor(2^64 / q)), the low word
// of -mu64 q.
__device__ __forceinline__ uint64_t mad_reduce(u128 x, uint64_t q, uint64_t mu, uint64_t mu64, uint32_t k)
{
  const uint64_t r64 = 0 - mu64 * q;
  const u128 y = (u128)red64((uint64_t)(x >> 64), q, mu64) * r64 + red64((uint64_t)x, q, mu64);
  return red128_wide(y, q, mu, k);
}

// Table (device, uint64 words): [0, n) the bases of in0[t]; [n, 2n) of in1[t]; then per output row r and term t the
// base of the matching row of c[t], bit 0 set when c[t] has one row per batch element (bases are 16-byte aligned).
// It is read through the constant address space: the entries are wave-uniform, so they are scalar loads.
//
// One thread owns two adjacent coefficients of one prime row for BP batch elements.  Per term it loads the two
// constant words once and uses them for all BP elements, loads PARTS * BP operand vectors (16 bytes each,
// non-temporal: every operand word is read once) and multiplies into 128-bit accumulators; it stores PARTS * BP
// vectors at the end.  No LDS: nothing is shared between threads.
template <int PARTS, int BP>
__global__ void __launch_bounds__(256)
mul_add_many_kernel(uint64_t* __restrict__ out0, uint64_t* __restrict__ out1, ro_u64 tab, int n, int batch, uint32_t N,
                    int accumulate, MadRows map, const PrimeDev* __restrict__ primes)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // vector index inside one polynomial
  if (2 * i >= N)
    return;
  const int row = blockIdx.y;
  const int b0 = blockIdx.z * BP;
  const PrimeDev pd = primes[map.p[row]];
  const uint64_t q = pd.q, mu = pd.mu, mu64 = pd.mu64;
  const uint32_t k = pd.k;
  const size_t row_off = (size_t)row * batch * N;
  // batch elements past the end repeat the last one (loads of valid rows; their stores are skipped)
  size_t boff[BP];
#pragma unroll
  for (int b = 0; b < BP; b++)
    boff[b] = (size_t)(b0 + b < batch ? b0 + b : batch - 1) * N + 2 * (size_t)i;
  u128 a0[BP][2], a1[BP][2];
#pragma unroll
  for (int b = 0; b < BP; b++) {
    a0[b][0] = a0[b][1] = a1[b][0] = a1[b][1] = 0;
    if (accumulate) {
      const ulonglong2 v = ld_stream2(out0 + row_off + boff[b]);
      a0[b][0] = v.x;
      a0[b][1] = v.y;
      if (PARTS == 2) {
        const ulonglong2 w = ld_stream2(out1 + row_off + boff[b]);
        a1[b][0] = w.x;
        a1[b][1] = w.y;
      }
    }
  }
  ro_u64 ctab = tab + 2 * (size_t)n + (size_t)row * n;
  for (int t0 = 0; t0 < n; t0 += MAD_CHUNK) {
    const int t1 = t0 + MAD_CHUNK < n ? t0 + MAD_CHUNK : n;
    for (int t = t0; t < t1; t++) {
      const uint64_t ce = ctab[t];
      const uint64_t* cp = reinterpret_cast<const uint64_t*>(ce & ~(uint64_t)1);
      const bool per_elem = ce & 1;
      const uint64_t* p0 = reinterpret_cast<const uint64_t*>(tab[t]) + row_off;
      const uint64_t* p1 = PARTS == 2 ? reinterpret_cast<const uint64_t*>(tab[n + t]) + row_off : nullptr;
      ulonglong2 c = *reinterpret_cast<const ulonglong2*>(cp + (per_elem ? boff[0] : 2 * (size_t)i));
#pragma unroll
      for (int b = 0; b < BP; b++) {
        if (b > 0 && per_elem)
          c = *reinterpret_cast<const ulonglong2*>(cp + boff[b]);
        const ulonglong2 x = ld_stream2(p0 + boff[b]);
        a0[b][0] += (u128)c.x * x.x;
        a0[b][1] += (u128)c.y * x.y;
        if (PARTS == 2) {
          const ulonglong2 y = ld_stream2(p1 + boff[b]);
          a1[b][0] += (u128)c.x * y.x;
          a1[b][1] += (u128)c.y * y.y;
        }
      }
    }
#pragma unroll
    for (int b = 0; b < BP; b++) {
      a0[b][0] = mad_reduce(a0[b][0], q, mu, mu64, k);
      a0[b][1] = mad_reduce(a0[b][1], q, mu, mu64, k);
      if (PARTS == 2) {
        a1[b][0] = mad_reduce(a1[b][0], q, mu, mu64, k);
        a1[b][1] = mad_reduce(a1[b][1], q, mu, mu64, k);
      }
    }
  }
#pragma unroll
  for (int b = 0; b < BP; b++) {
    if (b0 + b >= batch)
      break;
    st_stream2(out0 + row_off + boff[b], make_ulonglong2((uint64_t)a0[b][0], (uint64_t)a0[b][1]));
    if (PARTS == 2)
      st_stream2(out1 + row_off + boff[b], make_ulonglong2((uint64_t)a1[b][0], (uint64_t)a1[b][1]));
  }
}

// o0 = sum_t a0[t] b0[t], o1 = sum_t (a0[t] b1[t] + a1[t] b0[t]), o2 = sum_t a1[t] b1[t], t < n (hx_tensor_sum): the
// words that n x hx_tensor and the part-wise hx_add of the products leave, since the canonical residue of an exact sum
// of products does not depend on the order of its terms.  The accumulators start from zero; o1 takes two products per
// term, so a reduction every TSUM_CHUNK = MAD_CHUNK / 2 terms keeps it within mul_add_many_kernel's bound.
constexpr int TSUM_CHUNK = 128;
static_assert(2 * TSUM_CHUNK <= MAD_CHUNK &&
                  (~(u128)0 - (MAD_QMAX - 1)) / ((MAD_QMAX - 1) * (MAD_QMAX - 1)) >= (u128)(2 * TSUM_CHUNK),
              "2 TSUM_CHUNK products of residues and one residue must fit 128 bits");

// Table (device, uint64 words, read through the constant address space: wave-uniform scalar loads): [0, n) the bases
// of a0[t]; [n, 2n) of a1[t]; [2n, 3n) of b0[t]; [3n, 4n) of b1[t].  All of them and the three outputs share one prime
// set and batch, so one row offset serves every operand.  The thread shape is mul_add_many_kernel's: two adjacent
// coefficients of one prime row for BP batch elements; per term 4 BP operand vectors loaded (16 bytes each,
// non-temporal), 8 BP products into 6 BP 128-bit accumulators; 3 BP vectors stored at the end.  No LDS.  Operands may
// repeat (a square, one poly in several terms): they are only read.
template <int BP>
__global__ void __launch_bounds__(256)
tensor_sum_kernel(uint64_t* __restrict__ out0, uint64_t* __restrict__ out1, uint64_t* __restrict__ out2, ro_u64 tab, int n,
                  int batch, uint32_t N, MadRows map, const PrimeDev* __restrict__ primes)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // vector index inside one polynomial
  if (2 * i >= N)
    return;
  const int row = blockIdx.y;
  const int b0 = blockIdx.z * BP;
  const PrimeDev pd = primes[map.p[row]];
  const uint64_t q = pd.q, mu = pd.mu, mu64 = pd.mu64;
  const uint32_t k = pd.k;
  const size_t row_off = (size_t)row * batch * N;
  // batch elements past the end repeat the last one (loads of valid rows; their stores are skipped)
  size_t boff[BP];
#pragma unroll
  for (int b = 0; b < BP; b++)
    boff[b] = row_off + (size_t)(b0 + b < batch ? b0 + b : batch - 1) * N + 2 * (size_t)i;
  u128 s0[BP][2], s1[BP][2], s2[BP][2];
#pragma unroll
  for (int b = 0; b < BP; b++)
    s0[b][0] = s0[b][1] = s1[b][0] = s1[b][1] = s2[b][0] = s2[b][1] = 0;
  for (int t0 = 0; t0 < n; t0 += TSUM_CHUNK) {
    const int t1 = t0 + TSUM_CHUNK < n ? t0 + TSUM_CHUNK : n;
    for (int t = t0; t < t1; t++) {
      const uint64_t* pa0 = reinterpret_cast<const uint64_t*>(tab[t]);
      const uint64_t* pa1 = reinterpret_cast<const uint64_t*>(tab[(size_t)n + t]);
      const uint64_t* pb0 = reinterpret_cast<const uint64_t*>(tab[2 * (size_t)n + t]);
      const uint64_t* pb1 = reinterpret_cast<const uint64_t*>(tab[3 * (size_t)n + t]);
#pragma unroll
      for (int b = 0; b < BP; b++) {
        const ulonglong2 x0 = ld_stream2(pa0 + boff[b]);
        const ulonglong2 x1 = ld_stream2(pa1 + boff[b]);
        const ulonglong2 y0 = ld_stream2(pb0 + boff[b]);
        const ulonglong2 y1 = ld_stream2(pb1 + boff[b]);
        s0[b][0] += (u128)x0.x * y0.x;
        s0[b][1] += (u128)x0.y * y0.y;
        s1[b][0] += (u128)x0.x * y1.x;
        s1[b][1] += (u128)x0.y * y1.y;
        s1[b][0] += (u128)x1.x * y0.x;
        s1[b][1] += (u128)x1.y * y0.y;
        s2[b][0] += (u128)x1.x * y1.x;
        s2[b][1] += (u128)x1.y * y1.y;
      }
    }
#pragma unroll
    for (int b = 0; b < BP; b++) {
#pragma unroll
      for (int j = 0; j < 2; j++) {
        s0[b][j] = mad_reduce(s0[b][j], q, mu, mu64, k);
        s1[b][j] = mad_reduce(s1[b][j], q, mu, mu64, k);
        s2[b][j] = mad_reduce(s2[b][j], q, mu, mu64, k);
      }
    }
  }
#pragma unroll
  for (int b = 0; b < BP; b++) {
    if (b0 + b >= batch)
      break;
    st_stream2(out0 + boff[b], make_ulonglong2((uint64_t)s0[b][0], (uint64_t)s0[b][1]));
    st_stream2(out1 + boff[b], make_ulonglong2((uint64_t)s1[b][0], (uint64_t)s1[b][1]));
    st_stream2(out2 + boff[b], make_ulonglong2((uint64_t)s2[b][0], (uint64_t)s2[b][1]));
  }
}

// o0 = sum T[j k + i] a0[i] b0[j], o1 = sum T[j k + i] (a0[i] b1[j] + a1[i] b0[j]), o2 = sum T[j k + i] a1[i] b1[j] over
// i < k, j < l, j k + i < size (hx_table_tensor_sum): the words that, per j, one hx_mul_add_many of k terms
// (W_j = sum_i T[j k + i] a[i]) and then one hx_tensor_sum of the l pairs (W_j, b[j]) leave.  Per j the two inner sums
// U0_j, U1_j take k <= MAD_CHUNK products from zero and one mad_reduce; the outer sums then take 4 products of residues
// per j, two of them in o1, which is tensor_sum_kernel's count: a reduction every TSUM_CHUNK values of j.  A thread
// works on TTS_JB values of j at once, so TSUM_CHUNK is a multiple of it and the reduction falls between two blocks.
constexpr int TTS_MAX = 256;   // k and l
constexpr int TTS_JB = 4;
static_assert(TTS_MAX <= MAD_CHUNK, "an inner sum of k products is reduced once");
static_assert(TSUM_CHUNK % TTS_JB == 0, "the outer sums are reduced between two blocks of j, every TSUM_CHUNK values of j");

// Table (device, uint64 words, constant address space): [0, k) the bases of a0[i]; [k, 2k) of a1[i]; [2k, 2k + l) of
// b0[j]; [2k + l, 2k + 2l) of b1[j]; all of them and the outputs share one prime set and batch.  tbl: the table poly's
// rows, [its rows][size][N]; map.brow[row] is its row on the prime of output row `row`; entry e of that row serves every
// batch element.  The thread shape is the family's: two adjacent coefficients of one prime row for BP batch elements.
// Per block of TTS_JB values of j and per i the thread loads 2 BP operand vectors (non-temporal: they come back only
// l / TTS_JB times, far apart) and TTS_JB table vectors (plain loads: the other batch groups read them too), each
// table word used for BP elements and each operand word for TTS_JB values of j; 4 TTS_JB BP 128-bit accumulators for the
// inner sums and 6 BP for the outer ones (DESIGN.md 3.9s has the register counts).  Entries past `size` (a ragged row
// of the grid, rows without an entry) and values of j past l contribute nothing: neither their table words nor the b
// of an empty row are loaded.  No LDS.
template <int BP>
__global__ void __launch_bounds__(256)
table_tensor_sum_kernel(uint64_t* __restrict__ out0, uint64_t* __restrict__ out1, uint64_t* __restrict__ out2, ro_u64 tab,
                        const uint64_t* __restrict__ tbl, int k, int l, int size, int batch, uint32_t N, RowMap2 map,
                        const PrimeDev* __restrict__ primes)
{
  const uint32_t i2 = blockIdx.x * blockDim.x + threadIdx.x;   // vector index inside one polynomial
  if (2 * i2 >= N)
    return;
  const int row = blockIdx.y;
  const int b0 = blockIdx.z * BP;
  const PrimeDev pd = primes[map.p[row]];
  const uint64_t q = pd.q, mu = pd.mu, mu64 = pd.mu64;
  const uint32_t kb = pd.k;
  const size_t row_off = (size_t)row * batch * N;
  // batch elements past the end repeat the last one (loads of valid rows; their stores are skipped)
  size_t boff[BP];
#pragma unroll
  for (int b = 0; b < BP; b++)
    boff[b] = row_off + (size_t)(b0 + b < batch ? b0 + b : batch - 1) * N + 2 * (size_t)i2;
  const uint64_t* trow = tbl + (size_t)map.brow[row] * (size_t)size * N + 2 * (size_t)i2;
  ro_u64 ta0 = tab, ta1 = tab + k, tb0 = tab + 2 * (size_t)k, tb1 = tab + 2 * (size_t)k + l;
  u128 s0[BP][2], s1[BP][2], s2[BP][2];
#pragma unroll
  for (int b = 0; b < BP; b++)
    s0[b][0] = s0[b][1] = s1[b][0] = s1[b][1] = s2[b][0] = s2[b][1] = 0;
  for (int j0 = 0; j0 < l; j0 += TTS_JB) {
    u128 u0[TTS_JB][BP][2], u1[TTS_JB][BP][2];
    int cnt[TTS_JB];   // the entries of row j0 + jj of the grid that exist: k, fewer in the ragged last row, 0 past l
#pragma unroll
    for (int jj = 0; jj < TTS_JB; jj++) {
      const int left = size - (j0 + jj) * k;
      cnt[jj] = left < 0 ? 0 : left < k ? left : k;
#pragma unroll
      for (int b = 0; b < BP; b++)
        u0[jj][b][0] = u0[jj][b][1] = u1[jj][b][0] = u1[jj][b][1] = 0;
    }
    const uint64_t* tj = trow + (size_t)j0 * k * N;
    for (int i = 0; i < k; i++) {
      const uint64_t* pa0 = reinterpret_cast<const uint64_t*>(ta0[i]);
      const uint64_t* pa1 = reinterpret_cast<const uint64_t*>(ta1[i]);
      ulonglong2 x0[BP], x1[BP];
#pragma unroll
      for (int b = 0; b < BP; b++) {
        x0[b] = ld_stream2(pa0 + boff[b]);
        x1[b] = ld_stream2(pa1 + boff[b]);
      }
#pragma unroll
      for (int jj = 0; jj < TTS_JB; jj++) {
        if (i < cnt[jj]) {   // (wave-uniform)
          const ulonglong2 c = *reinterpret_cast<const ulonglong2*>(tj + ((size_t)jj * k + i) * N);
#pragma unroll
          for (int b = 0; b < BP; b++) {
            u0[jj][b][0] += (u128)c.x * x0[b].x;
            u0[jj][b][1] += (u128)c.y * x0[b].y;
            u1[jj][b][0] += (u128)c.x * x1[b].x;
            u1[jj][b][1] += (u128)c.y * x1[b].y;
          }
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < TTS_JB; jj++) {
      if (cnt[jj] > 0) {
        const uint64_t* pb0 = reinterpret_cast<const uint64_t*>(tb0[j0 + jj]);
        const uint64_t* pb1 = reinterpret_cast<const uint64_t*>(tb1[j0 + jj]);
#pragma unroll
        for (int b = 0; b < BP; b++) {
          const ulonglong2 y0 = ld_stream2(pb0 + boff[b]);
          const ulonglong2 y1 = ld_stream2(pb1 + boff[b]);
          const uint64_t w0x = mad_reduce(u0[jj][b][0], q, mu, mu64, kb), w0y = mad_reduce(u0[jj][b][1], q, mu, mu64, kb);
          const uint64_t w1x = mad_reduce(u1[jj][b][0], q, mu, mu64, kb), w1y = mad_reduce(u1[jj][b][1], q, mu, mu64, kb);
          s0[b][0] += (u128)w0x * y0.x;
          s0[b][1] += (u128)w0y * y0.y;
          s1[b][0] += (u128)w0x * y1.x;
          s1[b][1] += (u128)w0y * y1.y;
          s1[b][0] += (u128)w1x * y0.x;
          s1[b][1] += (u128)w1y * y0.y;
          s2[b][0] += (u128)w1x * y1.x;
          s2[b][1] += (u128)w1y * y1.y;
        }
      }
    }
    if ((j0 + TTS_JB) % TSUM_CHUNK == 0 || j0 + TTS_JB >= l) {
#pragma unroll
      for (int b = 0; b < BP; b++) {
#pragma unroll
        for (int c = 0; c < 2; c++) {
          s0[b][c] = mad_reduce(s0[b][c], q, mu, mu64, kb);
          s1[b][c] = mad_reduce(s1[b][c], q, mu, mu64, kb);
          s2[b][c] = mad_reduce(s2[b][c], q, mu, mu64, kb);
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < BP; b++) {
    if (b0 + b >= batch)
      break;
    st_stream2(out0 + boff[b], make_ulonglong2((uint64_t)s0[b][0], (uint64_t)s0[b][1]));
    st_stream2(out1 + boff[b], make_ulonglong2((uint64_t)s1[b][0], (uint64_t)s1[b][1]));
    st_stream2(out2 + boff[b], make_ulonglong2((uint64_t)s2[b][0], (uint64_t)s2[b][1]));
  }
}

// out0[i] = sum_(j<d) c[(i + j) mod d] * in0[j], out1[i] likewise, i < nout <= d <= CIRC_MAX_D (hx_mul_add_circulant): the
// words that the loop of unpack (src/intraSlot.cpp:108-115) leaves through hx_poly_copy / hx_mul / hx_add, since the
// canonical residue of an exact sum of products does not depend on the order of its terms.  The arithmetic is
// mul_add_many_kernel's: canonical residues accumulated unreduced in 128 bits, from zero; with d <= 64 < MAD_CHUNK
// products per output word, 64 (2^60 - 2)^2 < 2^126, one reduction at the end is enough.
//
// Table (device, uint64 words, read through the constant address space: wave-uniform scalar loads): [0, d) the bases
// of in0[j]; [d, 2d) of in1[j]; [2d, 2d + nout) of out0[i]; [2d + nout, 2d + 2 nout) of out1[i]; then per output row r
// and t < d the base of the matching row of c[t], bit 0 set when c[t] has one row per batch element.
//
// One thread owns two adjacent coefficients of one prime row of one batch element for a block of OB outputs
// i0 .. i0 + OB - 1: OB x PARTS x 2 accumulators of 128 bits (OB = 8, PARTS = 2: 128 VGPRs).  It walks j = 0 .. d - 1
// once: per step it loads in0[j] and in1[j] (16 bytes each, non-temporal) and ONE constant vector -- the OB constants
// that the block needs at step j, c[(i0 + k + j) mod d], are a window of the circulant that slides by one per step, kept
// in registers by unrolled moves.  The loads of step j + 1 are issued before the products of step j.  Outputs of the
// last block past nout are neither accumulated nor stored.  No LDS: nothing is shared between threads.
// Algorithmic bytes per prime row, batch element and block of OB outputs, in rows of 8 N bytes: PARTS d input rows and
// d + OB - 1 constant rows read, PARTS OB output rows written; with nb = ceil(nout / OB) blocks the call moves
//   8 N rows batch (nb (PARTS d + d + OB - 1) + PARTS nout)  bytes
// against 8 N rows batch nout d PARTS 8 of the d^2 copies, products and additions it replaces (per part and term a copy
// reads a row and writes one, a product reads two and writes one, a sum the same: 2 + 3 + 3 rows).  For d <= OB every operand word leaves
// HBM once (batch-1 constants are re-read per batch element, out of the L2).
constexpr int CIRC_MAX_D = 64;
static_assert(CIRC_MAX_D <= MAD_CHUNK, "one reduction per output word");

template <int PARTS, int OB>
__global__ void __launch_bounds__(256)
mul_add_circulant_kernel(ro_u64 tab, int d, int nout, int nblocks, int batch, uint32_t N, MadRows map,
                         const PrimeDev* __restrict__ primes)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // vector index inside one polynomial
  if (2 * i >= N)
    return;
  const int row = blockIdx.y;
  const int b = (int)(blockIdx.z / (uint32_t)nblocks);
  const int i0 = (int)(blockIdx.z % (uint32_t)nblocks) * OB;
  const int live = nout - i0 < OB ? nout - i0 : OB;           // outputs of this block (wave-uniform)
  const PrimeDev pd = primes[map.p[row]];
  const size_t off = ((size_t)row * batch + b) * N + 2 * (size_t)i;   // in an input or output poly
  const size_t coff_b = (size_t)b * N + 2 * (size_t)i, coff_1 = 2 * (size_t)i;
  ro_u64 ctab = tab + 2 * (size_t)d + 2 * (size_t)nout + (size_t)row * d;
  const auto ldc = [&](int t) {
    const uint64_t ce = ctab[t];
    const uint64_t* cp = reinterpret_cast<const uint64_t*>(ce & ~(uint64_t)1);
    return *reinterpret_cast<const ulonglong2*>(cp + ((ce & 1) ? coff_b : coff_1));
  };
  u128 a0[OB][2], a1[OB][2];
  ulonglong2 w[OB];
  int t = i0 % d;                                             // the constant the next load takes
#pragma unroll
  for (int k = 0; k < OB; k++) {
    a0[k][0] = a0[k][1] = a1[k][0] = a1[k][1] = 0;
    w[k] = ldc(t);
    t = t + 1 == d ? 0 : t + 1;
  }
  ulonglong2 nx = ld_stream2(reinterpret_cast<const uint64_t*>(tab[0]) + off), ny = nx;
  if (PARTS == 2)
    ny = ld_stream2(reinterpret_cast<const uint64_t*>(tab[d]) + off);
  for (int j = 0; j < d; j++) {
    const ulonglong2 x = nx, y = ny;
    ulonglong2 cn = w[OB - 1];
    if (j + 1 < d) {                                          // the next step's operands, in flight during the products
      nx = ld_stream2(reinterpret_cast<const uint64_t*>(tab[j + 1]) + off);
      if (PARTS == 2)
        ny = ld_stream2(reinterpret_cast<const uint64_t*>(tab[d + j + 1]) + off);
      cn = ldc(t);
      t = t + 1 == d ? 0 : t + 1;
    }
#pragma unroll
    for (int k = 0; k < OB; k++) {
      if (k < live) {
        a0[k][0] += (u128)w[k].x * x.x;
        a0[k][1] += (u128)w[k].y * x.y;
        if (PARTS == 2) {
          a1[k][0] += (u128)w[k].x * y.x;
          a1[k][1] += (u128)w[k].y * y.y;
        }
      }
    }
#pragma unroll
    for (int k = 0; k + 1 < OB; k++)
      w[k] = w[k + 1];
    w[OB - 1] = cn;
  }
  const uint64_t q = pd.q, mu = pd.mu, mu64 = pd.mu64;
  const uint32_t kk = pd.k;
#pragma unroll
  for (int k = 0; k < OB; k++) {
    if (k >= live)
      break;
    uint64_t* o0 = reinterpret_cast<uint64_t*>(tab[2 * d + i0 + k]) + off;
    st_stream2(o0, make_ulonglong2(mad_reduce(a0[k][0], q, mu, mu64, kk), mad_reduce(a0[k][1], q, mu, mu64, kk)));
    if (PARTS == 2) {
      uint64_t* o1 = reinterpret_cast<uint64_t*>(tab[2 * d + nout + i0 + k]) + off;
      st_stream2(o1, make_ulonglong2(mad_reduce(a1[k][0], q, mu, mu64, kk), mad_reduce(a1[k][1], q, mu, mu64, kk)));
    }
  }
}

// take = keep * mask, keep = keep - take (hx_mask_split): what hx_poly_copy, hx_mul and hx_sub leave, word for word --
// the product is ew_binary_kernel<EW_MUL>'s mul_mod, the difference its sub_mod.  One thread owns two adjacent
// coefficients of one prime row for BP batch elements: it loads the two mask words once when the mask has batch 1
// (mask_per_elem = 0) and uses them for all BP elements, loads PARTS * BP keep vectors (16 bytes each, non-temporal:
// every word is read once) and stores 2 * PARTS * BP vectors.  map.brow[r] is the mask's row for output row r.  No
// LDS: nothing is shared between threads.  All addresses are kernel arguments, so a launch can be captured.
template <int PARTS, int BP>
__global__ void __launch_bounds__(256)
mask_split_kernel(uint64_t* __restrict__ keep0, uint64_t* __restrict__ keep1, uint64_t* __restrict__ take0,
                  uint64_t* __restrict__ take1, const uint64_t* __restrict__ mask, int mask_per_elem, int batch,
                  uint32_t N, RowMap2 map, const PrimeDev* __restrict__ primes)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // vector index inside one polynomial
  if (2 * i >= N)
    return;
  const int row = blockIdx.y;
  const int b0 = blockIdx.z * BP;
  const PrimeDev pd = primes[map.p[row]];
  const uint64_t q = pd.q, mu = pd.mu;
  const uint32_t k = pd.k;
  const size_t row_off = (size_t)row * batch * N;
  const uint64_t* mrow = mask + (size_t)map.brow[row] * (mask_per_elem ? batch : 1) * N;
  // batch elements past the end repeat the last one (loads of valid rows; their stores are skipped)
  size_t boff[BP];
#pragma unroll
  for (int b = 0; b < BP; b++)
    boff[b] = (size_t)(b0 + b < batch ? b0 + b : batch - 1) * N + 2 * (size_t)i;
  ulonglong2 x0[BP], x1[BP];
#pragma unroll
  for (int b = 0; b < BP; b++) {
    x0[b] = ld_stream2(keep0 + row_off + boff[b]);
    if (PARTS == 2)
      x1[b] = ld_stream2(keep1 + row_off + boff[b]);
  }
  ulonglong2 c = *reinterpret_cast<const ulonglong2*>(mrow + (mask_per_elem ? boff[0] : 2 * (size_t)i));
#pragma unroll
  for (int b = 0; b < BP; b++) {
    if (b0 + b >= batch)
      break;
    if (b > 0 && mask_per_elem)
      c = *reinterpret_cast<const ulonglong2*>(mrow + boff[b]);
    ulonglong2 t;
    t.x = mul_mod(x0[b].x, c.x, q, mu, k);
    t.y = mul_mod(x0[b].y, c.y, q, mu, k);
    st_stream2(take0 + row_off + boff[b], t);
    st_stream2(keep0 + row_off + boff[b], make_ulonglong2(sub_mod(x0[b].x, t.x, q), sub_mod(x0[b].y, t.y, q)));
    if (PARTS == 2) {
      t.x = mul_mod(x1[b].x, c.x, q, mu, k);
      t.y = mul_mod(x1[b].y, c.y, q, mu, k);
      st_stream2(take1 + row_off + boff[b], t);
      st_stream2(keep1 + row_off + boff[b], make_ulonglong2(sub_mod(x1[b].x, t.x, q), sub_mod(x1[b].y, t.y, q)));
    }
  }
}

// c = c * mask + t - t * mask (hx_mask_blend): the words hx_mul(c, mask), hx_add(c, t), hx_mul(t, mask), hx_sub(c, t)
// leave in c.  Every operand is canonical, so the canonical residue of (c - t) * mask + t is that word: one mul_mod on
// sub_mod(c, t), then add_mod.  t is read only.  The thread shape is mask_split_kernel's: two adjacent coefficients of
// one prime row for BP batch elements, the two mask words loaded once when the mask has batch 1, PARTS * BP vectors of
// c and of t loaded (16 bytes each, non-temporal: every word is read once) and PARTS * BP vectors stored.
// map.brow[r] is the mask's row for output row r.  No LDS.  All addresses are kernel arguments, so a launch can be
// captured.
template <int PARTS, int BP>
__global__ void __launch_bounds__(256)
mask_blend_kernel(uint64_t* __restrict__ c0, uint64_t* __restrict__ c1, const uint64_t* __restrict__ t0,
                  const uint64_t* __restrict__ t1, const uint64_t* __restrict__ mask, int mask_per_elem, int batch,
                  uint32_t N, RowMap2 map, const PrimeDev* __restrict__ primes)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // vector index inside one polynomial
  if (2 * i >= N)
    return;
  const int row = blockIdx.y;
  const int b0 = blockIdx.z * BP;
  const PrimeDev pd = primes[map.p[row]];
  const uint64_t q = pd.q, mu = pd.mu;
  const uint32_t k = pd.k;
  const size_t row_off = (size_t)row * batch * N;
  const uint64_t* mrow = mask + (size_t)map.brow[row] * (mask_per_elem ? batch : 1) * N;
  // batch elements past the end repeat the last one (loads of valid rows; their stores are skipped)
  size_t boff[BP];
#pragma unroll
  for (int b = 0; b < BP; b++)
    boff[b] = (size_t)(b0 + b < batch ? b0 + b : batch - 1) * N + 2 * (size_t)i;
  ulonglong2 x0[BP], x1[BP], y0[BP], y1[BP];
#pragma unroll
  for (int b = 0; b < BP; b++) {
    x0[b] = ld_stream2(c0 + row_off + boff[b]);
    y0[b] = ld_stream2(t0 + row_off + boff[b]);
    if (PARTS == 2) {
      x1[b] = ld_stream2(c1 + row_off + boff[b]);
      y1[b] = ld_stream2(t1 + row_off + boff[b]);
    }
  }
  ulonglong2 c = *reinterpret_cast<const ulonglong2*>(mrow + (mask_per_elem ? boff[0] : 2 * (size_t)i));
#pragma unroll
  for (int b = 0; b < BP; b++) {
    if (b0 + b >= batch)
      break;
    if (b > 0 && mask_per_elem)
      c = *reinterpret_cast<const ulonglong2*>(mrow + boff[b]);
    ulonglong2 r;
    r.x = add_mod(mul_mod(sub_mod(x0[b].x, y0[b].x, q), c.x, q, mu, k), y0[b].x, q);
    r.y = add_mod(mul_mod(sub_mod(x0[b].y, y0[b].y, q), c.y, q, mu, k), y0[b].y, q);
    st_stream2(c0 + row_off + boff[b], r);
    if (PARTS == 2) {
      r.x = add_mod(mul_mod(sub_mod(x1[b].x, y1[b].x, q), c.x, q, mu, k), y1[b].x, q);
      r.y = add_mod(mul_mod(sub_mod(x1[b].y, y1[b].y, q), c.y, q, mu, k), y1[b].y, q);
      st_stream2(c1 + row_off + boff[b], r);
    }
  }
}

// out0[k] = c0 * masks[k], out1[k] = c1 * masks[k], k < nout (hx_mask_fan): per output the words hx_poly_copy(out, c) and
// hx_mul(out, masks[k]) leave -- ew_binary_kernel<EW_MUL>'s mul_mod on canonical residues.  It is the mask stage of one
// layer of a permutation network (src/PermNetwork.cpp:239-242), K masked copies of one ciphertext.
//
// Table (device, uint64 words, read through the constant address space: wave-uniform scalar loads): [0, nout) the bases
// of out0[k]; [nout, 2 nout) of out1[k]; then per row r and k < nout, at 2 nout + r nout + k, the base of masks[k]'s row
// on the prime of row r, bit 0 set when that mask has one row per batch element (bases are 16-byte aligned).
//
// The thread shape is mask_split_kernel's: one thread owns two adjacent coefficients of one prime row for BP batch
// elements.  It loads its PARTS * BP vectors of c once (16 bytes each, non-temporal: every word is read once), then walks
// the nout masks: per step the mask's two words (one load for all BP elements when the mask has batch 1, else BP loads)
// and PARTS * BP products stream-stored.  The words of mask k + 1 are loaded before the products of mask k.  No LDS:
// nothing is shared between threads.  Algorithmic bytes per part, in passes over the part: 1 read and K written (and the
// K masks read once each), against K (2 read + 2 written) (and the masks) of the K copies and K products.
template <int PARTS, int BP>
__global__ void __launch_bounds__(256)
mask_fan_kernel(const uint64_t* __restrict__ c0, const uint64_t* __restrict__ c1, ro_u64 tab, int nout, int batch,
                uint32_t N, MadRows map, const PrimeDev* __restrict__ primes)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // vector index inside one polynomial
  if (2 * i >= N)
    return;
  const int row = blockIdx.y;
  const int b0 = blockIdx.z * BP;
  const PrimeDev pd = primes[map.p[row]];
  const uint64_t q = pd.q, mu = pd.mu;
  const uint32_t k = pd.k;
  const size_t row_off = (size_t)row * batch * N;
  // batch elements past the end repeat the last one (loads of valid rows; their stores are skipped)
  size_t boff[BP];
#pragma unroll
  for (int b = 0; b < BP; b++)
    boff[b] = (size_t)(b0 + b < batch ? b0 + b : batch - 1) * N + 2 * (size_t)i;
  ulonglong2 x0[BP], x1[BP];
#pragma unroll
  for (int b = 0; b < BP; b++) {
    x0[b] = ld_stream2(c0 + row_off + boff[b]);
    if (PARTS == 2)
      x1[b] = ld_stream2(c1 + row_off + boff[b]);
  }
  ro_u64 mtab = tab + 2 * (size_t)nout + (size_t)row * nout;
  // step t loads the words of mask t and then forms the products of mask t - 1, whose words the step before loaded: the
  // loads are in flight during the products
  uint64_t nx[BP] = {}, ny[BP] = {};
  for (int t = 0; t <= nout; t++) {
    uint64_t mx[BP], my[BP];
#pragma unroll
    for (int b = 0; b < BP; b++) {
      mx[b] = nx[b];
      my[b] = ny[b];
    }
    if (t < nout) {
      const uint64_t e = mtab[t];
      const uint64_t* mp = reinterpret_cast<const uint64_t*>(e & ~(uint64_t)1);
      const bool per_elem = e & 1;
#pragma unroll
      for (int b = 0; b < BP; b++) {
        if (b == 0 || per_elem) {
          const ulonglong2 w = *reinterpret_cast<const ulonglong2*>(mp + (per_elem ? boff[b] : 2 * (size_t)i));
          nx[b] = w.x;
          ny[b] = w.y;
        } else {
          nx[b] = nx[0];
          ny[b] = ny[0];
        }
      }
    }
    if (t == 0)
      continue;
    uint64_t* o0 = reinterpret_cast<uint64_t*>(tab[t - 1]) + row_off;
    uint64_t* o1 = PARTS == 2 ? reinterpret_cast<uint64_t*>(tab[nout + t - 1]) + row_off : nullptr;
#pragma unroll
    for (int b = 0; b < BP; b++) {
      if (b0 + b < batch) {
        st_stream2(o0 + boff[b], make_ulonglong2(mul_mod(x0[b].x, mx[b], q, mu, k), mul_mod(x0[b].y, my[b], q, mu, k)));
        if (PARTS == 2)
          st_stream2(o1 + boff[b], make_ulonglong2(mul_mod(x1[b].x, mx[b], q, mu, k), mul_mod(x1[b].y, my[b], q, mu, k)));
      }
    }
  }
}

// the most outputs one hx_mask_fan takes (its table holds nout (2 + rows) words)
constexpr int FAN_MAX_OUT = 256;

// A table written from the kernel's own arguments (Table::commit under a graph capture): TS_WORDS words per launch, by
// value, so that a replay finds them without reading host memory.  One thread per word.
constexpr int TS_WORDS = 448;
struct TableWords {
  uint64_t w[TS_WORDS];
};
static_assert(sizeof(TableWords) + 64 <= 4096, "the words travel as kernel arguments");
__global__ void __launch_bounds__(256)
table_store_kernel(uint64_t* __restrict__ dst, TableWords words, int n)
{
  for (int t = threadIdx.x; t < n; t += blockDim.x)
    dst[t] = words.w[t];
}

// Per-row scalars of one scaled_sub_kernel launch, by value (the kernel-argument segment holds 4 KiB, so a launch takes
// SS_ROWS rows and the host issues one per SS_ROWS rows of the operand)
constexpr int SS_ROWS = 48;
struct ScaledSubRows {
  uint16_t p[SS_ROWS];                              // prime index of row row_base + r
  uint64_t u[SS_ROWS], up[SS_ROWS];                 // u in [0, q) and its Shoup companion floor(u 2^64 / q)
  uint64_t v[SS_ROWS], vp[SS_ROWS];
};
static_assert(sizeof(ScaledSubRows) + 64 <= 4096, "the scalars travel as kernel arguments");

// c = c * u[row] - t * v[row] (hx_scaled_sub): the words hx_mul_scalar(c, u), hx_poly_copy(t', t), hx_mul_scalar(t', v),
// hx_sub(c, t') leave in c.  Every operand is canonical and mul_shoup returns the canonical product, so sub_mod of the
// two products is that word.  t is read only.  The thread shape is mask_blend_kernel's: two adjacent coefficients of
// one prime row for BP batch elements, PARTS * BP vectors of c and of t loaded (16 bytes each, non-temporal: every word
// is read once) and PARTS * BP vectors stored; the four scalars of the row are wave-uniform reads of the kernel
// arguments.  HBM bound: per part 16 B read and 8 B written per coefficient, against 40 B read and 32 B written by the
// four calls.  No LDS.  All addresses and scalars are kernel arguments, so a launch can be captured.
template <int PARTS, int BP>
__global__ void __launch_bounds__(256)
scaled_sub_kernel(uint64_t* __restrict__ c0, uint64_t* __restrict__ c1, const uint64_t* __restrict__ t0,
                  const uint64_t* __restrict__ t1, int batch, uint32_t N, int row_base, ScaledSubRows rows,
                  const PrimeDev* __restrict__ primes)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // vector index inside one polynomial
  if (2 * i >= N)
    return;
  const int row = blockIdx.y;
  const int b0 = blockIdx.z * BP;
  const uint64_t q = primes[rows.p[row]].q;
  const uint64_t u = rows.u[row], up = rows.up[row], v = rows.v[row], vp = rows.vp[row];
  const size_t row_off = (size_t)(row_base + row) * batch * N;
  // batch elements past the end repeat the last one (loads of valid rows; their stores are skipped)
  size_t boff[BP];
#pragma unroll
  for (int b = 0; b < BP; b++)
    boff[b] = (size_t)(b0 + b < batch ? b0 + b : batch - 1) * N + 2 * (size_t)i;
  ulonglong2 x0[BP], x1[BP], y0[BP], y1[BP];
#pragma unroll
  for (int b = 0; b < BP; b++) {
    x0[b] = ld_stream2(c0 + row_off + boff[b]);
    y0[b] = ld_stream2(t0 + row_off + boff[b]);
    if (PARTS == 2) {
      x1[b] = ld_stream2(c1 + row_off + boff[b]);
      y1[b] = ld_stream2(t1 + row_off + boff[b]);
    }
  }
#pragma unroll
  for (int b = 0; b < BP; b++) {
    if (b0 + b >= batch)
      break;
    ulonglong2 r;
    r.x = sub_mod(mul_shoup(x0[b].x, u, up, q), mul_shoup(y0[b].x, v, vp, q), q);
    r.y = sub_mod(mul_shoup(x0[b].y, u, up, q), mul_shoup(y0[b].y, v, vp, q), q);
    st_stream2(c0 + row_off + boff[b], r);
    if (PARTS == 2) {
      r.x = sub_mod(mul_shoup(x1[b].x, u, up, q), mul_shoup(y1[b].x, v, vp, q), q);
      r.y = sub_mod(mul_shoup(x1[b].y, u, up, q), mul_shoup(y1[b].y, v, vp, q), q);
      st_stream2(c1 + row_off + boff[b], r);
    }
  }
}

// out0 = sum_t w[t][row] * in0[t] + addend[row], out1 = sum_t w[t][row] * in1[t] (hx_lin_comb): the words that the
// loop of simplePolyEval (src/polyEval.cpp:240-253) leaves -- per term a copy, addPrimesAndScale, one or two
// hx_mul_scalar and hx_add, then hx_add_scalar -- since every one of those steps is exact arithmetic modulo the row's
// prime and the caller has folded the integers they multiply by into w.  Table (device, uint64 words): per output row r
// and term t three words at 3 (r n + t): the address of the term's row for the prime of r in in0[t] and in in1[t]
// (0: the term has no such row and adds nothing), and the weight in [0, q); behind them, at 3 rows n + r, the addend of
// row r in [0, q).  It is read through the constant address space: the entries are wave-uniform, so they are scalar
// loads, and the branch on an absent row is uniform.  The thread shape is mul_add_many_kernel's: two adjacent
// coefficients of one prime row for BP batch elements, PARTS * BP operand vectors per term (16 bytes each,
// non-temporal: every operand word is read once), 128-bit accumulators that start from the addend and take n <=
// MAD_CHUNK products, one reduction, PARTS * BP vectors stored.  No LDS: nothing is shared between threads.
template <int PARTS, int BP>
__global__ void __launch_bounds__(256)
lin_comb_kernel(uint64_t* __restrict__ out0, uint64_t* __restrict__ out1, ro_u64 tab, int n, int rows, int batch,
                uint32_t N, MadRows map, const PrimeDev* __restrict__ primes)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;   // vector index inside one polynomial
  if (2 * i >= N)
    return;
  const int row = blockIdx.y;
  const int b0 = blockIdx.z * BP;
  const PrimeDev pd = primes[map.p[row]];
  const uint64_t q = pd.q, mu = pd.mu, mu64 = pd.mu64;
  const uint32_t k = pd.k;
  const size_t row_off = (size_t)row * batch * N;
  // batch elements past the end repeat the last one (loads of valid rows; their stores are skipped)
  size_t boff[BP];
#pragma unroll
  for (int b = 0; b < BP; b++)
    boff[b] = (size_t)(b0 + b < batch ? b0 + b : batch - 1) * N + 2 * (size_t)i;
  const uint64_t addend = tab[3 * (size_t)rows * n + row];
  u128 a0[BP][2], a1[BP][2];
#pragma unroll
  for (int b = 0; b < BP; b++) {
    a0[b][0] = a0[b][1] = addend;
    a1[b][0] = a1[b][1] = 0;
  }
  ro_u64 e = tab + 3 * (size_t)row * n;
  for (int t = 0; t < n; t++) {
    const uint64_t* p0 = reinterpret_cast<const uint64_t*>(e[3 * t]);
    if (!p0)
      continue;
    const uint64_t* p1 = PARTS == 2 ? reinterpret_cast<const uint64_t*>(e[3 * t + 1]) : nullptr;
    const uint64_t w = e[3 * t + 2];
#pragma unroll
    for (int b = 0; b < BP; b++) {
      const ulonglong2 x = ld_stream2(p0 + boff[b]);
      a0[b][0] += (u128)w * x.x;
      a0[b][1] += (u128)w * x.y;
      if (PARTS == 2) {
        const ulonglong2 y = ld_stream2(p1 + boff[b]);
        a1[b][0] += (u128)w * y.x;
        a1[b][1] += (u128)w * y.y;
      }
    }
  }
#pragma unroll
  for (int b = 0; b < BP; b++) {
    if (b0 + b >= batch)
      break;
    st_stream2(out0 + row_off + boff[b], make_ulonglong2(mad_reduce(a0[b][0], q, mu, mu64, k),
                                                         mad_reduce(a0[b][1], q, mu, mu64, k)));
    if (PARTS == 2)
      st_stream2(out1 + row_off + boff[b], make_ulonglong2(mad_reduce(a1[b][0], q, mu, mu64, k),
                                                           mad_reduce(a1[b][1], q, mu, mu64, k)));
  }
}

// The hoisted trace sum (hx_hoisted_automorph_sum): per output row r, with sigma_t the gather of DoubleCRT::automorph
// by k[t] (out[j] = in[perm_t[j]]),
//   out0 = Psp (c0 + sum_t sigma_t(c0)) + sum_t sum_d sigma_t(dig_d) b[t][d],   out1 = Psp c1 + sum_t sum_d sigma_t(dig_d) a[t][d]
// on the ciphertext's rows (r < L) and the two double sums alone on the special rows.
//
// hoisted_perm_kernel writes the n gather tables [n][N] uint32 once per call: perm_build_kernel's rule
// (zms_index[zms[j] k mod m]) for a general m, gather_kernel's closed form for a power of two.  They are shared by every
// row and batch element.
__global__ void __launch_bounds__(256)
hoisted_perm_kernel(uint32_t* __restrict__ perm, const uint32_t* __restrict__ zms, const int32_t* __restrict__ zms_index,
                    uint32_t N, uint64_t m, ro_u64 ks, int pow2)
{
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N)
    return;
  const uint64_t k = ks[blockIdx.y];
  uint32_t s;
  if (pow2)
    s = (uint32_t)(((((uint64_t)(2 * j + 1)) * k) & (m - 1)) >> 1);
  else
    s = (uint32_t)zms_index[((uint64_t)zms[j] * k) % m];
  perm[(size_t)blockIdx.y * N + j] = s;
}

// Table (device, uint64 words): [0, n) the k[t] (hoisted_perm_kernel's); then per output row r and term t three words at
// n + 3 (r n + t): the address of row r's words of digit 0 in b[t] and in a[t] and the words between two digits of that
// matrix; behind them, at n + 3 rows n + r, Psp modulo the prime of row r.  It is read through the constant address space:
// the entries are wave-uniform, so they are scalar loads.
//
// One thread owns one output coefficient j of one prime row for BP batch elements.  Per term it reads its gather index
// once, per term and digit the two key words once (at j: coalesced, and kept for all BP elements) and BP digit words at
// the gathered index (element-granular, through L2, as gather_kernel reads), and multiplies into 128-bit accumulators:
// 1 + n + n ndig <= MAD_CHUNK products in out0's, so one reduction at the end is enough (the host checks the count).
// No LDS: nothing is shared between threads.
template <int BP>
__global__ void __launch_bounds__(256)
hoisted_sum_kernel(uint64_t* __restrict__ out0, uint64_t* __restrict__ out1, const uint64_t* __restrict__ dig,
                   const uint64_t* __restrict__ c0, const uint64_t* __restrict__ c1, const uint32_t* __restrict__ perm,
                   ro_u64 tab, int n, int ndig, int L, int nall, int batch, uint32_t N, MadRows map,
                   const PrimeDev* __restrict__ primes)
{
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N)
    return;
  const int row = blockIdx.y;
  const int b0 = blockIdx.z * BP;
  const PrimeDev pd = primes[map.p[row]];
  const uint64_t q = pd.q, mu = pd.mu, mu64 = pd.mu64;
  const uint32_t k = pd.k;
  const size_t rw = (size_t)batch * N;
  const size_t row_off = (size_t)row * rw;
  // batch elements past the end repeat the last one (loads of valid rows; their stores are skipped)
  size_t boff[BP];
#pragma unroll
  for (int b = 0; b < BP; b++)
    boff[b] = (size_t)(b0 + b < batch ? b0 + b : batch - 1) * N;
  const bool own = row < L;
  const uint64_t psp = tab[n + 3 * (size_t)nall * n + row];
  u128 a0[BP], a1[BP];
#pragma unroll
  for (int b = 0; b < BP; b++) {
    a0[b] = own ? (u128)psp * c0[row_off + boff[b] + j] : (u128)0;
    a1[b] = own ? (u128)psp * c1[row_off + boff[b] + j] : (u128)0;
  }
  ro_u64 e = tab + n + 3 * (size_t)row * n;
  const size_t dstride = (size_t)nall * rw;   // words between two digits of the block
  for (int t = 0; t < n; t++) {
    const uint32_t s = perm[(size_t)t * N + j];
    const uint64_t* kb = reinterpret_cast<const uint64_t*>(e[3 * t]);
    const uint64_t* ka = reinterpret_cast<const uint64_t*>(e[3 * t + 1]);
    const size_t kstride = e[3 * t + 2];
    if (own) {
#pragma unroll
      for (int b = 0; b < BP; b++)
        a0[b] += (u128)psp * c0[row_off + boff[b] + s];
    }
    for (int d = 0; d < ndig; d++) {
      const uint64_t wb = kb[d * kstride + j], wa = ka[d * kstride + j];
      const uint64_t* dp = dig + d * dstride + row_off + s;
#pragma unroll
      for (int b = 0; b < BP; b++) {
        const uint64_t x = dp[boff[b]];
        a0[b] += (u128)x * wb;
        a1[b] += (u128)x * wa;
      }
    }
  }
#pragma unroll
  for (int b = 0; b < BP; b++) {
    if (b0 + b >= batch)
      break;
    st_stream1(out0 + row_off + boff[b] + j, mad_reduce(a0[b], q, mu, mu64, k));
    st_stream1(out1 + row_off + boff[b] + j, mad_reduce(a1[b], q, mu, mu64, k));
  }
}

// The hoisted masked fan-out (hx_hoisted_mask_fan), hoisted_sum_kernel's sibling with one output pair per term: an inner
// node of recursiveReplicateDim (src/replicate.cpp:432-483) and its leaf (:411-415) over BasicAutomorphPrecon
// (src/matmul.cpp:48-184).  Per output row r and term t, with sigma_t the gather by k[t] and A_t, B_t the two masks read
// at the thread's own index,
//   out0[t] = A_t (Psp c0) + B_t (Psp sigma_t(c0) + sum_d sigma_t(dig_d) b[t][d])
//   out1[t] = A_t (Psp c1) + B_t (              sum_d sigma_t(dig_d) a[t][d])
// on the ciphertext's rows (r < L) and B_t times the sum over d alone on the special rows.
//
// Table (device, uint64 words): [0, n) the k[t] (hoisted_perm_kernel's); [n, 2n) and [2n, 3n) the bases of out0[t] and
// out1[t]; then per output row r and term t five words at 3 n + 5 (r n + t): the address of row r's words of digit 0 in
// b[t] and in a[t], the words between two digits of that matrix, and the address of the row of A_t and of B_t on the prime
// of r, bit 0 set when the mask has one row per batch element (0: the constant 1); behind them, at 3 n + 5 rows n + r, Psp
// modulo the prime of row r.  It is read through the constant address space: the entries are wave-uniform, so they are
// scalar loads and the branches on them are uniform.
//
// The thread shape is hoisted_sum_kernel's: one output coefficient j of one prime row for BP batch elements.  Psp c0[j]
// and Psp c1[j] are formed once (reduced: they are multiplied again) and serve all n terms.  Per term the thread reads its
// gather index once, per digit the two key words once and BP digit words at the gathered index, into 128-bit accumulators
// of 1 + ndig <= MAD_CHUNK products, reduced; then out = A (Psp c) + B inner, two products in a second 128-bit sum,
// reduced once and stored non-temporally.  No LDS: nothing is shared between threads.
template <int BP>
__global__ void __launch_bounds__(256)
hoisted_mask_fan_kernel(const uint64_t* __restrict__ dig, const uint64_t* __restrict__ c0, const uint64_t* __restrict__ c1,
                        const uint32_t* __restrict__ perm, ro_u64 tab, int n, int ndig, int L, int nall, int batch, uint32_t N,
                        MadRows map, const PrimeDev* __restrict__ primes)
{
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= N)
    return;
  const int row = blockIdx.y;
  const int b0 = blockIdx.z * BP;
  const PrimeDev pd = primes[map.p[row]];
  const uint64_t q = pd.q, mu = pd.mu, mu64 = pd.mu64;
  const uint32_t k = pd.k;
  const size_t rw = (size_t)batch * N;
  const size_t row_off = (size_t)row * rw;
  // batch elements past the end repeat the last one (loads of valid rows; their stores are skipped)
  size_t boff[BP];
#pragma unroll
  for (int b = 0; b < BP; b++)
    boff[b] = (size_t)(b0 + b < batch ? b0 + b : batch - 1) * N;
  const bool own = row < L;
  const uint64_t psp = tab[3 * (size_t)n + 5 * (size_t)nall * n + row];
  uint64_t pc0[BP], pc1[BP];   // Psp c0[j], Psp c1[j]
#pragma unroll
  for (int b = 0; b < BP; b++) {
    pc0[b] = own ? mad_reduce((u128)psp * c0[row_off + boff[b] + j], q, mu, mu64, k) : 0;
    pc1[b] = own ? mad_reduce((u128)psp * c1[row_off + boff[b] + j], q, mu, mu64, k) : 0;
  }
  ro_u64 e = tab + 3 * (size_t)n + 5 * (size_t)row * n;
  const size_t dstride = (size_t)nall * rw;   // words between two digits of the block
  for (int t = 0; t < n; t++) {
    const uint32_t s = perm[(size_t)t * N + j];
    const uint64_t* kb = reinterpret_cast<const uint64_t*>(e[5 * t]);
    const uint64_t* ka = reinterpret_cast<const uint64_t*>(e[5 * t + 1]);
    const size_t kstride = e[5 * t + 2];
    const uint64_t ae = e[5 * t + 3], be = e[5 * t + 4];
    const uint64_t* ap = reinterpret_cast<const uint64_t*>(ae & ~(uint64_t)1);
    const uint64_t* bp = reinterpret_cast<const uint64_t*>(be & ~(uint64_t)1);
    u128 a0[BP], a1[BP];
#pragma unroll
    for (int b = 0; b < BP; b++) {
      a0[b] = own ? (u128)psp * c0[row_off + boff[b] + s] : (u128)0;
      a1[b] = 0;
    }
    for (int d = 0; d < ndig; d++) {
      const uint64_t wb = kb[d * kstride + j], wa = ka[d * kstride + j];
      const uint64_t* dp = dig + d * dstride + row_off + s;
#pragma unroll
      for (int b = 0; b < BP; b++) {
        const uint64_t x = dp[boff[b]];
        a0[b] += (u128)x * wb;
        a1[b] += (u128)x * wa;
      }
    }
    uint64_t* o0 = reinterpret_cast<uint64_t*>(tab[n + t]) + row_off + j;
    uint64_t* o1 = reinterpret_cast<uint64_t*>(tab[2 * (size_t)n + t]) + row_off + j;
#pragma unroll
    for (int b = 0; b < BP; b++) {
      if (b0 + b >= batch)
        break;
      const uint64_t am = ap ? ap[((ae & 1) ? boff[b] : 0) + j] : 1;
      const uint64_t bm = bp ? bp[((be & 1) ? boff[b] : 0) + j] : 1;
      const u128 r0 = (u128)am * pc0[b] + (u128)bm * mad_reduce(a0[b], q, mu, mu64, k);
      const u128 r1 = (u128)am * pc1[b] + (u128)bm * mad_reduce(a1[b], q, mu, mu64, k);
      st_stream1(o0 + boff[b], mad_reduce(r0, q, mu, mu64, k));
      st_stream1(o1 + boff[b], mad_reduce(r1, q, mu, mu64, k));
    }
  }
}

// The hoisted blend (hx_hoisted_blend), hoisted_mask_fan_kernel's sibling with two operands: the inner step of
// MatMulFullExec::rec_mul along a non-native dimension (src/matmul.cpp:2174-2204) over two BasicAutomorphPrecon
// (:48-184), of ctxt (digA, a0) and of ctxt1 = ctxt moved by g^(-ord) (digB, b0).  Per output row r and term t, with
// sigma_t the gather by k[t] and M_t the mask read at the thread's own index,
//   out0[t] = M_t X0 + Y0 - M_t Y0,  X0 = Psp sigma_t(a0) + sum_d sigma_t(digA_d) b[t][d],  Y0 likewise from b0, digB
//   out1[t] = M_t X1 + Y1 - M_t Y1,  X1 =                   sum_d sigma_t(digA_d) a[t][d],  Y1 likewise from digB
// the Psp terms on the ciphertext's rows (r < L) alone.  Both operands meet the same key words and the same mask word,
// so the blend is taken on the operand words, z = M x + y - M y (reduced: it is multiplied again), before the products:
//   out0[t] = Psp z(sigma_t(a0), sigma_t(b0)) + sum_d z(sigma_t(digA_d), sigma_t(digB_d)) b[t][d]
// which is the same residue, all of it being exact arithmetic modulo the row's prime.  One accumulator pair per batch
// element instead of one per operand, 3 + ndig reductions per output pair instead of 6, and each key word read once.
//
// Table (device, uint64 words): [0, n) the k[t] (hoisted_perm_kernel's); [n, 2n) and [2n, 3n) the bases of out0[t] and
// out1[t]; then per output row r and term t four words at 3 n + 4 (r n + t): the address of row r's words of digit 0 in
// b[t] and in a[t], the words between two digits of that matrix, and the address of the row of M_t on the prime of r, bit
// 0 set when the mask has one row per batch element; behind them, at 3 n + 4 rows n + r, Psp modulo the prime of row r.
// It is read through the constant address space: the entries are wave-uniform, so they are scalar loads.
//
// The thread shape is hoisted_mask_fan_kernel's: one output coefficient j of one prime row for BP batch elements.  Per
// term the thread reads its gather index once and BP mask words, per digit the two key words once and 2 BP digit words at
// the gathered index, into 128-bit accumulators of 1 + ndig <= MAD_CHUNK products, reduced once and stored
// non-temporally.  No LDS: nothing is shared between threads.  (The second launch bound asks for hoisted_mask_fan_kernel's
// five waves per SIMD: BP = 4 is 96 VGPRs with it and 98, four waves, without; no scratch either way.)
template <int BP>
__global__ void __launch_bounds__(256, 5)
hoisted_blend_kernel(const uint64_t* __restrict__ digA, const uint64_t* __restrict__ digB, const uint64_t* __restrict__ a0,
                     const uint64_t* __restrict__ b0, const uint32_t* __restrict__ perm, ro_u64 tab, int n, int ndig, int L,
                     int nall, int batch, uint32_t N, MadRows map, const PrimeDev* __restrict__ primes)
{
  // The 2 BP (ndig + 1) rows a workgroup gathers from are those of every workgroup with its (y, z); workgroups go round
  // the 8 XCDs by their linear index, x fastest, so unchanged each row would be fetched into all 8 L2s.  The remap (a
  // bijection for any grid) gives each XCD a contiguous run of (x, y, z): a row's workgroups share one L2.
  const uint32_t gx = gridDim.x, gy = gridDim.y, nwg = gx * gy * gridDim.z;
  const uint32_t lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
  const uint32_t xcd = lin % 8, per = nwg / 8, rem = nwg % 8;
  const uint32_t wg = (xcd < rem ? xcd * (per + 1) : rem * (per + 1) + (xcd - rem) * per) + lin / 8;
  const uint32_t j = (wg % gx) * blockDim.x + threadIdx.x;
  if (j >= N)
    return;
  const int row = (wg / gx) % gy;
  const int bb = (wg / (gx * gy)) * BP;
  const PrimeDev pd = primes[map.p[row]];
  const uint64_t q = pd.q, mu = pd.mu, mu64 = pd.mu64;
  const uint32_t k = pd.k;
  const size_t rw = (size_t)batch * N;
  const size_t row_off = (size_t)row * rw;
  // batch elements past the end repeat the last one (loads of valid rows; their stores are skipped)
  size_t boff[BP];
#pragma unroll
  for (int b = 0; b < BP; b++)
    boff[b] = (size_t)(bb + b < batch ? bb + b : batch - 1) * N;
  const bool own = row < L;
  const uint64_t psp = tab[3 * (size_t)n + 4 * (size_t)nall * n + row];
  ro_u64 e = tab + 3 * (size_t)n + 4 * (size_t)row * n;
  const size_t dstride = (size_t)nall * rw;   // words between two digits of a block
  // m x + y - m y = m (x + q - y) + y <= (q - 1)(2 q - 1) + q - 1 < 2 q^2 for canonical words: red128_wide's domain
  // (below 8 q^2), a third of mad_reduce's multiplies; so is the sum of 1 + ndig <= 8 products (wave-uniform branch)
  auto blend = [&](uint64_t x, uint64_t y, uint64_t m) { return red128_wide((u128)m * (x + q - y) + y, q, mu, k); };
  const bool few = ndig + 1 <= 8;
  auto reduce = [&](u128 x) { return few ? red128_wide(x, q, mu, k) : mad_reduce(x, q, mu, mu64, k); };
  for (int t = 0; t < n; t++) {
    const uint32_t s = perm[(size_t)t * N + j];
    const uint64_t* kb = reinterpret_cast<const uint64_t*>(e[4 * t]);
    const uint64_t* ka = reinterpret_cast<const uint64_t*>(e[4 * t + 1]);
    const size_t kstride = e[4 * t + 2];
    const uint64_t me = e[4 * t + 3];
    const uint64_t* mp = reinterpret_cast<const uint64_t*>(me & ~(uint64_t)1) + j;
    uint64_t mk[BP];
    u128 r0[BP], r1[BP];
#pragma unroll
    for (int b = 0; b < BP; b++) {
      mk[b] = mp[(me & 1) ? boff[b] : 0];
      r0[b] = own ? (u128)psp * blend(a0[row_off + boff[b] + s], b0[row_off + boff[b] + s], mk[b]) : (u128)0;
      r1[b] = 0;
    }
    for (int d = 0; d < ndig; d++) {
      const uint64_t wb = kb[d * kstride + j], wa = ka[d * kstride + j];
      const size_t at = d * dstride + row_off + s;
#pragma unroll
      for (int b = 0; b < BP; b++) {
        const uint64_t z = blend(digA[at + boff[b]], digB[at + boff[b]], mk[b]);
        r0[b] += (u128)z * wb;
        r1[b] += (u128)z * wa;
      }
    }
    uint64_t* o0 = reinterpret_cast<uint64_t*>(tab[n + t]) + row_off + j;
    uint64_t* o1 = reinterpret_cast<uint64_t*>(tab[2 * (size_t)n + t]) + row_off + j;
#pragma unroll
    for (int b = 0; b < BP; b++) {
      if (bb + b >= batch)
        break;
      st_stream1(o0 + boff[b], reduce(r0[b]));
      st_stream1(o1 + boff[b], reduce(r1[b]));
    }
  }
}

}  // namespace hx

namespace {

using hxi::err;

constexpr int RING = 4;  // calls whose table copy may still be in flight

// per-context state: pinned staging buffers for the pointer table (one per call in flight) and its device copy
struct LinState {
  uint64_t* h_tab[RING] = {nullptr, nullptr, nullptr, nullptr};
  size_t h_cap[RING] = {0, 0, 0, 0};
  hipEvent_t copied[RING] = {nullptr, nullptr, nullptr, nullptr};
  bool pending[RING] = {false, false, false, false};
  int next = 0;
  uint64_t* d_tab = nullptr;
  size_t d_cap = 0;
  uint32_t* d_perm = nullptr;   // hx_hoisted_automorph_sum's gather tables
  size_t perm_cap = 0;          // (bytes)
  std::vector<void*> recorded;  // the tables of calls recorded in a graph capture (Table::acquire_recorded)
};
void state_free(void* p)
{
  LinState* s = static_cast<LinState*>(p);
  if (!s)
    return;
  for (int i = 0; i < RING; i++) {
    if (s->h_tab[i])
      hipHostFree(s->h_tab[i]);
    if (s->copied[i])
      hipEventDestroy(s->copied[i]);
  }
  hipFree(s->d_tab);
  hipFree(s->d_perm);
  for (void* p : s->recorded)
    hipFree(p);
  delete s;
}

// The pieces an entry point is put together from: its own argument checks, then a Frame, the shared
// checks of its operands, what is particular to it, a Table where it uploads one, and HX_LAUNCH_PW.

int shape_of(const hx_poly* p, int* batch, std::vector<int>* idx)
{
  int n = 0;
  RC(hx_poly_shape(p, batch, &n, nullptr));
  idx->assign(n > 0 ? n : 1, 0);
  RC(hx_poly_primes(p, idx->data()));
  idx->resize(n);
  return HX_OK;
}

// the position of `prime` among the n of list, or -1
int row_of(const int* list, size_t n, int prime)
{
  const int* at = std::find(list, list + n, prime);
  return at == list + n ? -1 : (int)(at - list);
}

// every address given is 16-byte aligned (a null one passes)
template <class... P>
bool aligned16(const P*... p)
{
  return ((... | (uintptr_t)p) & 15) == 0;
}

// What a call works in: the context's view under its lock, and the shape every operand is held against -- that of the
// reference poly (the first output).
struct Frame {
  hx_ctx* ctx = nullptr;
  hxi::CtxView v{};
  std::unique_lock<std::recursive_mutex> lk;
  int batch = 0, rows = 0, bp = 1;   // bp: the batch elements one thread takes (the kernels' BP)
  std::vector<int> idx;              // the prime of every row
  uint32_t N = 0;
  const hx::PrimeDev* primes = nullptr;
  hx::MadRows map{};                 // idx for the kernels

  // no_capture: the sentence that refuses an open graph capture; nullptr for a call that can be captured (it then
  // waits for nothing and allocates nothing)
  int enter(hx_ctx* c, const char* no_capture)
  {
    ctx = c;
    RC(hxi::ctx_enter(c, &v));
    lk = std::unique_lock<std::recursive_mutex>(*v.mu);
    if (no_capture && v.capturing)
      return err(HX_ERR_UNSUPPORTED, "%s", no_capture);
    N = v.phim;
    primes = static_cast<const hx::PrimeDev*>(v.d_primes);
    return HX_OK;
  }
  int set_rows(const std::vector<int>& primes_of_rows)
  {
    if (primes_of_rows.size() > (size_t)hx::MAX_ROWS)
      return err(HX_ERR_UNSUPPORTED, "too many rows");
    if (&idx != &primes_of_rows)
      idx = primes_of_rows;
    rows = (int)idx.size();
    for (int r = 0; r < rows; r++)
      map.p[r] = (uint16_t)idx[r];
    bp = batch == 1 ? 1 : 4;
    return HX_OK;
  }
  int open(hx_ctx* c, const hx_poly* ref, const char* no_capture)
  {
    RC(enter(c, no_capture));
    RC(shape_of(ref, &batch, &idx));
    return set_rows(idx);
  }
  // the kernels take two coefficients per thread
  int even(const char* who) const
  {
    if (N < 2 || (N & 1))
      return err(HX_ERR_UNSUPPORTED, "%s needs an even number of coefficients", who);
    return HX_OK;
  }
  // the prime of every row
  int moduli(std::vector<uint64_t>* qs) const
  {
    qs->resize(rows);
    for (int r = 0; r < rows; r++)
      RC(hx_ctx_prime(ctx, idx[r], &(*qs)[r], nullptr));
    return HX_OK;
  }
  // one thread per two coefficients, one row, bp batch elements
  dim3 grid() const { return dim3((N / 2 + 255) / 256, (unsigned)rows, (unsigned)((batch + bp - 1) / bp)); }
};

// refuses, with the caller's sentence, a poly whose batch or prime set is not the frame's
int same_shape(const hx_poly* p, const Frame& f, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
int same_shape(const hx_poly* p, const Frame& f, const char* fmt, ...)
{
  int b = 0;
  std::vector<int> idx;
  RC(shape_of(p, &b, &idx));
  if (b == f.batch && idx == f.idx)
    return HX_OK;
  char msg[400];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(msg, sizeof msg, fmt, ap);
  va_end(ap);
  return err(HX_ERR_INVALID, "%s", msg);
}

// The terms (c[t], in0[t], in1[t]) of hx_mul_add_many and hx_mul_add_circulant, checked against the frame: in0[t] and
// in1[t] have its shape (`outs`: what the refusal calls it), c[t] has batch 1 or the frame's, and a row for every prime.
struct Terms {
  const hx_poly* const* c;
  const hx_poly* const* in0;
  const hx_poly* const* in1;   // null for one-part operands
  int n;
  std::vector<int> crow;       // [r n + t]: the row of c[t] on the prime of output row r
  std::vector<int> cper;       // [t]: c[t] has one row per batch element
};
int check_terms(const Frame& f, const char* outs, Terms* T)
{
  const int n = T->n;
  T->crow.resize((size_t)f.rows * n);
  T->cper.resize(n);
  for (int t = 0; t < n; t++) {
    RC(same_shape(T->in0[t], f, "in0[%d] differs from %s in batch or prime set", t, outs));
    if (T->in1)
      RC(same_shape(T->in1[t], f, "in1[%d] differs from %s in batch or prime set", t, outs));
    int b = 0;
    std::vector<int> cidx;
    RC(shape_of(T->c[t], &b, &cidx));
    if (b != f.batch && b != 1)
      return err(HX_ERR_INVALID, "c[%d]: batch %d is neither 1 nor %d", t, b, f.batch);
    T->cper[t] = b == f.batch && f.batch > 1;
    for (int r = 0; r < f.rows; r++) {
      const int at = row_of(cidx.data(), cidx.size(), f.idx[r]);
      if (at < 0)
        return err(HX_ERR_INVALID, "c[%d] has no row for prime %d", t, f.idx[r]);
      T->crow[(size_t)r * n + t] = at;
    }
  }
  return HX_OK;
}
// The terms' words of a pointer table (read after the outputs own their rows): in[t] and in[n + t] the bases of in0[t]
// and in1[t], crows[r n + t] the base of c[t]'s row for output row r, bit 0 set when c[t] has one row per batch
// element.  -> the first term with a base that is not 16-byte aligned, or -1
int fill_terms(const Frame& f, const Terms& T, uint64_t* in, uint64_t* crows)
{
  const int n = T.n;
  const size_t rw = (size_t)f.batch * f.N;
  int bad = -1;
  for (int t = 0; t < n; t++) {
    const uint64_t* p0 = hxi::poly_rows_read(T.in0[t]);
    const uint64_t* p1 = T.in1 ? hxi::poly_rows_read(T.in1[t]) : nullptr;
    const uint64_t* cb = hxi::poly_rows_read(T.c[t]);
    in[t] = (uint64_t)(uintptr_t)p0;
    in[n + t] = (uint64_t)(uintptr_t)p1;
    const size_t crw = T.cper[t] ? rw : (size_t)f.N;
    for (int r = 0; r < f.rows; r++)
      crows[(size_t)r * n + t] = (uint64_t)(uintptr_t)(cb + (size_t)T.crow[(size_t)r * n + t] * crw) | (uint64_t)T.cper[t];
    if (bad < 0 && !aligned16(p0, p1, cb))
      bad = t;
  }
  return bad;
}

// The mask of hx_mask_split and hx_mask_blend: batch 1 or the frame's, and a row for every prime (map->brow).
int check_mask(const Frame& f, const hx_poly* mask, int* per_elem, hx::RowMap2* map)
{
  int b = 0;
  std::vector<int> midx;
  RC(shape_of(mask, &b, &midx));
  if (b != f.batch && b != 1)
    return err(HX_ERR_INVALID, "mask: batch %d is neither 1 nor %d", b, f.batch);
  *per_elem = b == f.batch && f.batch > 1;
  for (int r = 0; r < f.rows; r++) {
    const int at = row_of(midx.data(), midx.size(), f.idx[r]);
    if (at < 0)
      return err(HX_ERR_PRIMESET, "DoubleCRT::Op: incompatible index sets (the mask has no row for prime %d)", f.idx[r]);
    map->p[r] = (uint16_t)f.idx[r];
    map->brow[r] = (uint16_t)at;
  }
  return HX_OK;
}

// Which of the four operands may not be the mask as well.
enum MaskAlias { NO_MASK, OUTPUTS_NOT_MASK, NOTHING_IS_MASK };

// The opening of a call on the one or two parts of a ciphertext, op = (c0, t0, c1, t1) or (keep0, take0, keep1, take1)
// with their names: the second pair is there or not as one, the handles are distinct (and not the mask, as `alias`
// says), everything belongs to one context; then the frame of op[0], whose shape the others have.  Nothing is written.
int open_four(Frame* f, const hx_poly* const op[4], const char* const name[4], const hx_poly* mask, MaskAlias alias)
{
  if (!op[0] || !op[1] || (alias != NO_MASK && !mask))
    return err(HX_ERR_INVALID, "null argument");
  if ((op[2] == nullptr) != (op[3] == nullptr))
    return err(HX_ERR_INVALID, "%s and %s go together (both null for a one-part ciphertext)", name[2], name[3]);
  const int nops = op[2] ? 4 : 2;
  for (int a = 0; a < nops; a++) {
    if (op[a] == mask && (alias == NOTHING_IS_MASK || (alias == OUTPUTS_NOT_MASK && (a & 1) == 0)))
      return err(HX_ERR_INVALID, "an output is also the mask");
    for (int b = a + 1; b < nops; b++)
      if (op[a] == op[b])
        return err(HX_ERR_INVALID, "%s, %s, %s and %s must be different polys", name[0], name[2], name[1], name[3]);
  }
  hx_ctx* ctx = hxi::poly_ctx(op[0]);
  for (int a = 1; a < nops; a++)
    if (hxi::poly_ctx(op[a]) != ctx)
      return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  if (alias != NO_MASK && hxi::poly_ctx(mask) != ctx)
    return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  RC(f->open(ctx, op[0], nullptr));
  for (int a = 1; a < nops; a++)
    RC(same_shape(op[a], *f, "%s differs from %s in batch or prime set", name[a], name[0]));
  return HX_OK;
}

// c first: one that still shares t's rows (a lazy hx_poly_copy) takes its own copy, and t's rows stay where they are
int update_c_then_read_t(hx_poly* c0, hx_poly* c1, const hx_poly* t0, const hx_poly* t1, uint64_t* c[2], const uint64_t* t[2])
{
  c[0] = c[1] = nullptr;
  RC(hxi::poly_rows_update(c0, &c[0]));
  if (c1)
    RC(hxi::poly_rows_update(c1, &c[1]));
  t[0] = hxi::poly_rows_read(t0);
  t[1] = t1 ? hxi::poly_rows_read(t1) : nullptr;
  return HX_OK;
}

// the device buffer *p of at least `bytes`: the stream is waited for before a smaller one is replaced
int grow(hipStream_t st, void** p, size_t* cap, size_t bytes)
{
  if (*cap >= bytes)
    return HX_OK;
  CK(hipStreamSynchronize(st));   // an earlier launch may still read the old buffer
  hipFree(*p);
  *p = nullptr;
  *cap = 0;
  CK(hipMalloc(p, bytes));
  *cap = bytes;
  return HX_OK;
}

// The table a call uploads.  acquire: the next staging buffer of the context's ring (h, to be filled) and the device
// table (d), both of at least `words`; it waits for the copy that last read the staging buffer.  commit: the copy, the
// event that marks it done, and the buffer's `pending` flag.  An entry point acquires after its last check and before
// it takes an output, so that a failure here touches none.
//
// Under a graph capture (acquire_recorded, hx_mask_fan's) neither the ring nor the shared device table will do: a replay
// runs after later calls have rewritten both, and a table grown since has been freed.  The recorded call gets a device
// table of its own, kept until the context goes, and commit writes it by table_store_kernel launches whose words are
// kernel arguments, so the recording holds them.  Nothing is waited for; the one allocation is the table.
struct Table {
  LinState* s = nullptr;
  int slot = 0;
  size_t bytes = 0;
  uint64_t* h = nullptr;
  uint64_t* d = nullptr;
  std::vector<uint64_t> own;   // h of a recorded call
  bool recorded = false;
  void state(const Frame& f)
  {
    if (!*f.v.linalg) {
      *f.v.linalg = new LinState();
      *f.v.linalg_free = state_free;
    }
    s = static_cast<LinState*>(*f.v.linalg);
  }
  int acquire_recorded(const Frame& f, size_t words)
  {
    state(f);
    recorded = true;
    bytes = words * 8;
    void* p = nullptr;
    CK(hipMalloc(&p, bytes));
    s->recorded.push_back(p);
    own.assign(words, 0);
    h = own.data();
    d = static_cast<uint64_t*>(p);
    return HX_OK;
  }
  int acquire(const Frame& f, size_t words)
  {
    state(f);
    bytes = words * 8;
    slot = s->next;
    s->next = (slot + 1) % RING;
    if (s->pending[slot]) {   // the copy that last read this staging buffer
      CK(hipEventSynchronize(s->copied[slot]));
      s->pending[slot] = false;
    }
    if (s->h_cap[slot] < bytes) {
      if (s->h_tab[slot])
        CK(hipHostFree(s->h_tab[slot]));
      s->h_tab[slot] = nullptr;
      s->h_cap[slot] = 0;
      CK(hipHostMalloc((void**)&s->h_tab[slot], bytes, hipHostMallocDefault));
      s->h_cap[slot] = bytes;
    }
    if (!s->copied[slot])
      CK(hipEventCreateWithFlags(&s->copied[slot], hipEventDisableTiming));
    RC(grow(f.v.stream, (void**)&s->d_tab, &s->d_cap, bytes));
    h = s->h_tab[slot];
    d = s->d_tab;
    return HX_OK;
  }
  // hx_hoisted_automorph_sum's gather tables, `words` of 32 bits
  int perm(const Frame& f, size_t words, uint32_t** out)
  {
    RC(grow(f.v.stream, (void**)&s->d_perm, &s->perm_cap, words * 4));
    *out = s->d_perm;
    return HX_OK;
  }
  int commit(hipStream_t st)
  {
    if (recorded) {
      const size_t words = bytes / 8;
      for (size_t at = 0; at < words; at += hx::TS_WORDS) {
        const int n = (int)std::min(words - at, (size_t)hx::TS_WORDS);
        hx::TableWords tw{};
        std::copy(h + at, h + at + n, tw.w);
        HX_LAUNCH(hx::table_store_kernel, dim3(1), dim3(256), 0, st, d + at, tw, n);
        CK(hipGetLastError());
      }
      return HX_OK;
    }
    CK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
    CK(hipEventRecord(s->copied[slot], st));
    s->pending[slot] = true;
    return HX_OK;
  }
};

// One launch of 256 threads per workgroup on one of two kernels, and on one of K<PARTS, X> for PARTS in {1, 2} and X
// in {NARROW, WIDE}.  HX_LAUNCH names a kernel to the profiler by the text of its argument, so every case is written
// out with literal template arguments.
#define HX_LAUNCH_W(wide, KN, KW, grid, st, ...)               \
  do {                                                         \
    if (!(wide))                                               \
      HX_LAUNCH(KN, grid, dim3(256), 0, st, __VA_ARGS__);      \
    else                                                       \
      HX_LAUNCH(KW, grid, dim3(256), 0, st, __VA_ARGS__);      \
  } while (0)
#define HX_LAUNCH_PW(K, parts, wide, NARROW, WIDE, grid, st, ...)                                  \
  do {                                                                                             \
    if ((parts) == 2)                                                                              \
      HX_LAUNCH_W(wide, (hx::K<2, NARROW>), (hx::K<2, WIDE>), grid, st, __VA_ARGS__);              \
    else                                                                                           \
      HX_LAUNCH_W(wide, (hx::K<1, NARROW>), (hx::K<1, WIDE>), grid, st, __VA_ARGS__);              \
  } while (0)

}  // namespace

extern "C" int hx_mul_add_many(hx_poly* out0, hx_poly* out1, const hx_poly* const* c, const hx_poly* const* in0,
                               const hx_poly* const* in1, int n, int accumulate)
{
  if (!out0 || !c || !in0)
    return err(HX_ERR_INVALID, "null argument");
  if ((out1 == nullptr) != (in1 == nullptr))
    return err(HX_ERR_INVALID, "out1 and in1 go together (both null for a one-part ciphertext)");
  if (n < 1)
    return err(HX_ERR_INVALID, "hx_mul_add_many needs at least one term (n = %d)", n);
  if (out0 == out1)
    return err(HX_ERR_INVALID, "out0 and out1 are the same poly");
  hx_ctx* ctx = hxi::poly_ctx(out0);
  for (int t = 0; t < n; t++) {
    if (!c[t] || !in0[t] || (in1 && !in1[t]))
      return err(HX_ERR_INVALID, "null poly (term %d)", t);
    if (hxi::poly_ctx(c[t]) != ctx || hxi::poly_ctx(in0[t]) != ctx || (in1 && hxi::poly_ctx(in1[t]) != ctx))
      return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects (term %d)", t);
    if (in0[t] == out0 || in0[t] == out1 || (in1 && (in1[t] == out0 || in1[t] == out1)) || c[t] == out0 ||
        c[t] == out1)
      return err(HX_ERR_INVALID, "an output is also an input (term %d)", t);
  }
  if (out1 && hxi::poly_ctx(out1) != ctx)
    return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  Frame f;
  RC(f.open(ctx, out0, "hx_mul_add_many uploads a pointer table and cannot be captured in a graph"));
  if (out1)
    RC(same_shape(out1, f, "out0 and out1 differ in batch or prime set"));
  RC(f.even("hx_mul_add_many"));
  Terms T{c, in0, in1, n, {}, {}};
  RC(check_terms(f, "the output", &T));
  if (f.rows == 0)
    return HX_OK;
  // table (kernel's layout): the bases of in0, of in1, then the rows of c
  Table tab;
  RC(tab.acquire(f, (size_t)n * (2 + f.rows)));
  // the outputs first: one that still shares an input's rows (a lazy hx_poly_copy) owns its rows before the inputs'
  // addresses are read into the table
  uint64_t *o0 = nullptr, *o1 = nullptr;
  RC(accumulate ? hxi::poly_rows_update(out0, &o0) : hxi::poly_rows_write(out0, &o0));
  if (out1)
    RC(accumulate ? hxi::poly_rows_update(out1, &o1) : hxi::poly_rows_write(out1, &o1));
  const int bad = fill_terms(f, T, tab.h, tab.h + 2 * (size_t)n);
  if (bad >= 0)
    return err(HX_ERR_INVALID, "term %d: rows are not 16-byte aligned", bad);
  if (!aligned16(o0, o1))
    return err(HX_ERR_INVALID, "output rows are not 16-byte aligned");
  RC(tab.commit(f.v.stream));
  HX_LAUNCH_PW(mul_add_many_kernel, out1 ? 2 : 1, f.bp != 1, 1, 4, f.grid(), f.v.stream, o0, o1, hx::as_ro(tab.d), n, f.batch,
               f.N, accumulate ? 1 : 0, f.map, f.primes);
  CK(hipGetLastError());
  return HX_OK;
}

extern "C" int hx_mul_add_circulant(hx_poly* const* out0, hx_poly* const* out1, int nout, const hx_poly* const* c,
                                    const hx_poly* const* in0, const hx_poly* const* in1, int d)
{
  if (!out0 || !c || !in0)
    return err(HX_ERR_INVALID, "null argument");
  if ((out1 == nullptr) != (in1 == nullptr))
    return err(HX_ERR_INVALID, "out1 and in1 go together (both null for one-part operands)");
  if (d < 1 || d > hx::CIRC_MAX_D)
    return err(d < 1 ? HX_ERR_INVALID : HX_ERR_UNSUPPORTED, "hx_mul_add_circulant takes 1 <= d <= %d (d = %d)", hx::CIRC_MAX_D, d);
  if (nout < 1 || nout > d)
    return err(HX_ERR_INVALID, "hx_mul_add_circulant takes 1 <= nout <= d (nout = %d, d = %d)", nout, d);
  // every poly, null checks and aliasing first: a refused call touches no output
  std::vector<const hx_poly*> outs, ins;
  for (int i = 0; i < nout; i++) {
    if (!out0[i] || (out1 && !out1[i]))
      return err(HX_ERR_INVALID, "null poly (output %d)", i);
    outs.push_back(out0[i]);
    if (out1)
      outs.push_back(out1[i]);
  }
  for (int t = 0; t < d; t++) {
    if (!c[t] || !in0[t] || (in1 && !in1[t]))
      return err(HX_ERR_INVALID, "null poly (term %d)", t);
    ins.push_back(c[t]);
    ins.push_back(in0[t]);
    if (in1)
      ins.push_back(in1[t]);
  }
  {
    std::vector<const hx_poly*> so(outs), si(ins);
    std::sort(so.begin(), so.end());
    std::sort(si.begin(), si.end());
    if (std::adjacent_find(so.begin(), so.end()) != so.end())
      return err(HX_ERR_INVALID, "an output appears twice");
    for (const hx_poly* o : so)
      if (std::binary_search(si.begin(), si.end(), o))
        return err(HX_ERR_INVALID, "an output is also an input");
  }
  hx_ctx* ctx = hxi::poly_ctx(out0[0]);
  for (const hx_poly* p : outs)
    if (hxi::poly_ctx(p) != ctx)
      return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  for (const hx_poly* p : ins)
    if (hxi::poly_ctx(p) != ctx)
      return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  Frame f;
  RC(f.open(ctx, out0[0], "hx_mul_add_circulant uploads a pointer table and cannot be captured in a graph"));
  for (size_t i = 1; i < outs.size(); i++)
    RC(same_shape(outs[i], f, "the outputs differ in batch or prime set"));
  RC(f.even("hx_mul_add_circulant"));
  Terms T{c, in0, in1, d, {}, {}};
  RC(check_terms(f, "the outputs", &T));
  if (f.rows == 0)
    return HX_OK;
  const int ob = nout <= 4 ? 4 : 8;   // the kernel's OB: outputs per block
  const int nblocks = (nout + ob - 1) / ob;
  if ((size_t)f.batch * nblocks > 65535)
    return err(HX_ERR_UNSUPPORTED, "batch %d x %d output blocks exceeds the grid", f.batch, nblocks);
  // table (kernel's layout): the bases of in0, of in1, of out0, of out1, then the rows of c
  Table tab;
  RC(tab.acquire(f, 2 * (size_t)d + 2 * (size_t)nout + (size_t)f.rows * d));
  uint64_t* ho = tab.h + 2 * (size_t)d;
  bool aligned = true;
  for (int i = 0; i < nout; i++) {
    uint64_t *o0 = nullptr, *o1 = nullptr;
    RC(hxi::poly_rows_write(out0[i], &o0));
    if (out1)
      RC(hxi::poly_rows_write(out1[i], &o1));
    ho[i] = (uint64_t)(uintptr_t)o0;
    ho[nout + i] = (uint64_t)(uintptr_t)o1;
    aligned = aligned && aligned16(o0, o1);
  }
  if (fill_terms(f, T, tab.h, ho + 2 * (size_t)nout) >= 0 || !aligned)
    return err(HX_ERR_INVALID, "rows are not 16-byte aligned");
  RC(tab.commit(f.v.stream));
  const dim3 grid((f.N / 2 + 255) / 256, (unsigned)f.rows, (unsigned)(f.batch * nblocks));
  HX_LAUNCH_PW(mul_add_circulant_kernel, out1 ? 2 : 1, ob == 8, 4, 8, grid, f.v.stream, hx::as_ro(tab.d), d, nout, nblocks,
               f.batch, f.N, f.map, f.primes);
  CK(hipGetLastError());
  return HX_OK;
}

extern "C" int hx_mask_split(hx_poly* keep0, hx_poly* keep1, hx_poly* take0, hx_poly* take1, const hx_poly* mask)
{
  const hx_poly* const ops[4] = {keep0, take0, keep1, take1};
  static const char* const name[4] = {"keep0", "take0", "keep1", "take1"};
  Frame f;
  RC(open_four(&f, ops, name, mask, NOTHING_IS_MASK));
  int per_elem = 0;
  hx::RowMap2 map;
  RC(check_mask(f, mask, &per_elem, &map));
  RC(f.even("hx_mask_split"));
  if (f.rows == 0)
    return HX_OK;
  const int parts = keep1 ? 2 : 1;
  hx_poly* const keep[2] = {keep0, keep1};
  hx_poly* const take[2] = {take0, take1};
  if (f.v.no_mask_split) {   // HX_NO_MASK_SPLIT: the sequence the kernel replaces
    for (int a = 0; a < parts; a++) {
      RC(hx_poly_copy(take[a], keep[a]));
      RC(hx_mul(take[a], mask));
      RC(hx_sub(keep[a], take[a]));
    }
    return HX_OK;
  }
  // take first: one that still shares keep's rows (a lazy hx_poly_copy) lets go of them, and keep is then updated in
  // place without a copy
  uint64_t *k[2] = {nullptr, nullptr}, *t[2] = {nullptr, nullptr};
  for (int a = 0; a < parts; a++)
    RC(hxi::poly_rows_write(take[a], &t[a]));
  for (int a = 0; a < parts; a++)
    RC(hxi::poly_rows_update(keep[a], &k[a]));
  const uint64_t* mp = hxi::poly_rows_read(mask);
  if (!aligned16(k[0], k[1], t[0], t[1], mp))
    return err(HX_ERR_INVALID, "rows are not 16-byte aligned");
  HX_LAUNCH_PW(mask_split_kernel, parts, f.bp != 1, 1, 4, f.grid(), f.v.stream, k[0], k[1], t[0], t[1], mp, per_elem, f.batch,
               f.N, map, f.primes);
  CK(hipGetLastError());
  return HX_OK;
}

extern "C" int hx_mask_fan(hx_poly* const* out0, hx_poly* const* out1, int nout, const hx_poly* c0, const hx_poly* c1,
                           const hx_poly* const* masks)
{
  if (!out0 || !c0 || !masks)
    return err(HX_ERR_INVALID, "null argument");
  if ((out1 == nullptr) != (c1 == nullptr))
    return err(HX_ERR_INVALID, "out1 and c1 go together (both null for a one-part operand)");
  if (nout < 1)
    return err(HX_ERR_INVALID, "hx_mask_fan needs at least one output (nout = %d)", nout);
  if (nout > hx::FAN_MAX_OUT)
    return err(HX_ERR_UNSUPPORTED, "hx_mask_fan: too many outputs (nout = %d, at most %d)", nout, hx::FAN_MAX_OUT);
  // every poly, null checks and aliasing first: a refused call touches no output
  std::vector<const hx_poly*> outs, ins{c0};
  if (c1)
    ins.push_back(c1);
  for (int t = 0; t < nout; t++) {
    if (!out0[t] || (out1 && !out1[t]) || !masks[t])
      return err(HX_ERR_INVALID, "null poly (output %d)", t);
    outs.push_back(out0[t]);
    if (out1)
      outs.push_back(out1[t]);
    ins.push_back(masks[t]);
  }
  if (c0 == c1)
    return err(HX_ERR_INVALID, "c0 and c1 are the same poly");
  {
    std::vector<const hx_poly*> so(outs), si(ins);
    std::sort(so.begin(), so.end());
    std::sort(si.begin(), si.end());
    if (std::adjacent_find(so.begin(), so.end()) != so.end())
      return err(HX_ERR_INVALID, "an output appears twice");
    for (const hx_poly* o : so)
      if (std::binary_search(si.begin(), si.end(), o))
        return err(HX_ERR_INVALID, "an output is also c0, c1 or a mask");
  }
  hx_ctx* ctx = hxi::poly_ctx(c0);
  for (const hx_poly* p : outs)
    if (hxi::poly_ctx(p) != ctx)
      return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  for (const hx_poly* p : ins)
    if (hxi::poly_ctx(p) != ctx)
      return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  Frame f;
  RC(f.open(ctx, c0, nullptr));
  if (c1)
    RC(same_shape(c1, f, "c0 and c1 differ in batch or prime set"));
  for (size_t i = 0; i < outs.size(); i++)
    RC(same_shape(outs[i], f, "output %d differs from c0 in batch or prime set", (int)(i / (out1 ? 2 : 1))));
  // mrow[r nout + t]: the row of masks[t] on the prime of row r; mper[t]: masks[t] has one row per batch element
  std::vector<int> mrow((size_t)f.rows * nout), mper(nout);
  for (int t = 0; t < nout; t++) {
    hx::RowMap2 map;
    RC(check_mask(f, masks[t], &mper[t], &map));
    for (int r = 0; r < f.rows; r++)
      mrow[(size_t)r * nout + t] = map.brow[r];
  }
  RC(f.even("hx_mask_fan"));
  if (f.rows == 0)
    return HX_OK;
  const int parts = c1 ? 2 : 1;
  if (f.v.no_mask_fan) {   // HX_NO_MASK_FAN: the sequence the kernel replaces
    for (int t = 0; t < nout; t++) {
      RC(hx_poly_copy(out0[t], c0));
      RC(hx_mul(out0[t], masks[t]));
      if (c1) {
        RC(hx_poly_copy(out1[t], c1));
        RC(hx_mul(out1[t], masks[t]));
      }
    }
    return HX_OK;
  }
  // table (kernel's layout): the bases of out0, of out1, then the masks' rows
  Table tab;
  const size_t words = (size_t)nout * (2 + (size_t)f.rows);
  RC(f.v.capturing ? tab.acquire_recorded(f, words) : tab.acquire(f, words));
  // the outputs first: one that still shares c's rows (a lazy hx_poly_copy) lets go of them, and c's rows stay where
  // they are
  bool aligned = true;
  for (int t = 0; t < nout; t++) {
    uint64_t *o0 = nullptr, *o1 = nullptr;
    RC(hxi::poly_rows_write(out0[t], &o0));
    if (out1)
      RC(hxi::poly_rows_write(out1[t], &o1));
    tab.h[t] = (uint64_t)(uintptr_t)o0;
    tab.h[nout + t] = (uint64_t)(uintptr_t)o1;
    aligned = aligned && aligned16(o0, o1);
  }
  const uint64_t* p0 = hxi::poly_rows_read(c0);
  const uint64_t* p1 = c1 ? hxi::poly_rows_read(c1) : nullptr;
  aligned = aligned && aligned16(p0, p1);
  const size_t rw = (size_t)f.batch * f.N;
  for (int t = 0; t < nout; t++) {
    const uint64_t* mb = hxi::poly_rows_read(masks[t]);
    aligned = aligned && aligned16(mb);
    const size_t mrw = mper[t] ? rw : (size_t)f.N;
    for (int r = 0; r < f.rows; r++)
      tab.h[2 * (size_t)nout + (size_t)r * nout + t] =
          (uint64_t)(uintptr_t)(mb + (size_t)mrow[(size_t)r * nout + t] * mrw) | (uint64_t)mper[t];
  }
  if (!aligned)
    return err(HX_ERR_INVALID, "rows are not 16-byte aligned");
  RC(tab.commit(f.v.stream));
  HX_LAUNCH_PW(mask_fan_kernel, parts, f.bp != 1, 1, 4, f.grid(), f.v.stream, p0, p1, hx::as_ro(tab.d), nout, f.batch, f.N,
               f.map, f.primes);
  CK(hipGetLastError());
  return HX_OK;
}

extern "C" int hx_mask_blend(hx_poly* c0, hx_poly* c1, const hx_poly* t0, const hx_poly* t1, const hx_poly* mask)
{
  const hx_poly* const ops[4] = {c0, t0, c1, t1};
  static const char* const name[4] = {"c0", "t0", "c1", "t1"};
  Frame f;
  RC(open_four(&f, ops, name, mask, OUTPUTS_NOT_MASK));   // (t is read only: it may be the mask)
  int per_elem = 0;
  hx::RowMap2 map;
  RC(check_mask(f, mask, &per_elem, &map));
  RC(f.even("hx_mask_blend"));
  if (f.rows == 0)
    return HX_OK;
  uint64_t* c[2];
  const uint64_t* t[2];
  RC(update_c_then_read_t(c0, c1, t0, t1, c, t));
  const uint64_t* mp = hxi::poly_rows_read(mask);
  if (!aligned16(c[0], c[1], t[0], t[1], mp))
    return err(HX_ERR_INVALID, "rows are not 16-byte aligned");
  HX_LAUNCH_PW(mask_blend_kernel, c1 ? 2 : 1, f.bp != 1, 1, 4, f.grid(), f.v.stream, c[0], c[1], t[0], t[1], mp, per_elem,
               f.batch, f.N, map, f.primes);
  CK(hipGetLastError());
  return HX_OK;
}

extern "C" int hx_scaled_sub(hx_poly* c0, hx_poly* c1, const hx_poly* t0, const hx_poly* t1, const uint64_t* u_per_row,
                             const uint64_t* v_per_row)
{
  if (!u_per_row || !v_per_row)
    return err(HX_ERR_INVALID, "null argument");
  const hx_poly* const ops[4] = {c0, t0, c1, t1};
  static const char* const name[4] = {"c0", "t0", "c1", "t1"};
  Frame f;
  RC(open_four(&f, ops, name, nullptr, NO_MASK));
  RC(f.even("hx_scaled_sub"));
  std::vector<uint64_t> qs;
  RC(f.moduli(&qs));
  for (int r = 0; r < f.rows; r++)
    if (u_per_row[r] >= qs[r] || v_per_row[r] >= qs[r])
      return err(HX_ERR_INVALID, "row %d: the scalars are not reduced modulo the row's prime %llu", r,
                 (unsigned long long)qs[r]);
  if (f.rows == 0)
    return HX_OK;
  uint64_t* c[2];
  const uint64_t* t[2];
  RC(update_c_then_read_t(c0, c1, t0, t1, c, t));
  if (!aligned16(c[0], c[1], t[0], t[1]))
    return err(HX_ERR_INVALID, "rows are not 16-byte aligned");
  // the scalars travel in the kernel's argument block, SS_ROWS rows of them per launch
  dim3 grid = f.grid();
  for (int base = 0; base < f.rows; base += hx::SS_ROWS) {
    const int nr = std::min(f.rows - base, (int)hx::SS_ROWS);
    hx::ScaledSubRows sr{};
    for (int r = 0; r < nr; r++) {
      const uint64_t q = qs[base + r];
      sr.p[r] = (uint16_t)f.idx[base + r];
      sr.u[r] = u_per_row[base + r];
      sr.up[r] = hxh::shoup(sr.u[r], q);
      sr.v[r] = v_per_row[base + r];
      sr.vp[r] = hxh::shoup(sr.v[r], q);
    }
    grid.y = (unsigned)nr;
    HX_LAUNCH_PW(scaled_sub_kernel, c1 ? 2 : 1, f.bp != 1, 1, 4, grid, f.v.stream, c[0], c[1], t[0], t[1], f.batch, f.N, base,
                 sr, f.primes);
    CK(hipGetLastError());
  }
  return HX_OK;
}

extern "C" int hx_lin_comb(hx_poly* out0, hx_poly* out1, const hx_poly* const* in0, const hx_poly* const* in1, int n,
                           const uint64_t* w, const uint64_t* addend)
{
  if (!out0 || !in0 || !w)
    return err(HX_ERR_INVALID, "null argument");
  if ((out1 == nullptr) != (in1 == nullptr))
    return err(HX_ERR_INVALID, "out1 and in1 go together (both null for a one-part ciphertext)");
  if (n < 1)
    return err(HX_ERR_INVALID, "hx_lin_comb needs at least one term (n = %d)", n);
  if (n > hx::MAD_CHUNK)
    return err(HX_ERR_UNSUPPORTED, "hx_lin_comb takes at most %d terms (n = %d)", hx::MAD_CHUNK, n);
  if (out0 == out1)
    return err(HX_ERR_INVALID, "out0 and out1 are the same poly");
  hx_ctx* ctx = hxi::poly_ctx(out0);
  for (int t = 0; t < n; t++) {
    if (!in0[t] || (in1 && !in1[t]))
      return err(HX_ERR_INVALID, "null poly (term %d)", t);
    if (hxi::poly_ctx(in0[t]) != ctx || (in1 && hxi::poly_ctx(in1[t]) != ctx))
      return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects (term %d)", t);
    if (in0[t] == out0 || in0[t] == out1 || (in1 && (in1[t] == out0 || in1[t] == out1)))
      return err(HX_ERR_INVALID, "an output is also an input (term %d)", t);
  }
  if (out1 && hxi::poly_ctx(out1) != ctx)
    return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  Frame f;
  RC(f.open(ctx, out0, "hx_lin_comb uploads a table of pointers and weights and cannot be captured in a graph"));
  if (out1)
    RC(same_shape(out1, f, "out0 and out1 differ in batch or prime set"));
  RC(f.even("hx_lin_comb"));
  const int rows = f.rows;
  std::vector<uint64_t> qs;
  RC(f.moduli(&qs));
  for (int r = 0; r < rows; r++) {
    if (addend && addend[r] >= qs[r])
      return err(HX_ERR_INVALID, "row %d: the addend is not reduced modulo the row's prime %llu", r,
                 (unsigned long long)qs[r]);
    for (int t = 0; t < n; t++)
      if (w[(size_t)t * rows + r] >= qs[r])
        return err(HX_ERR_INVALID, "term %d, row %d: the weight is not reduced modulo the row's prime %llu", t, r,
                   (unsigned long long)qs[r]);
  }
  // trow[r n + t]: the row of term t that holds the prime of output row r, or -1 (a term has a prime set of its own)
  std::vector<int> trow((size_t)rows * n, -1);
  for (int t = 0; t < n; t++) {
    int b = 0, b1 = 0;
    std::vector<int> tidx, tidx1;
    RC(shape_of(in0[t], &b, &tidx));
    if (b != f.batch)
      return err(HX_ERR_INVALID, "in0[%d]: batch %d, the output has %d", t, b, f.batch);
    if (in1) {
      RC(shape_of(in1[t], &b1, &tidx1));
      if (b1 != f.batch || tidx1 != tidx)
        return err(HX_ERR_INVALID, "in1[%d] differs from in0[%d] in batch or prime set", t, t);
    }
    for (size_t j = 0; j < tidx.size(); j++) {
      const int at = row_of(f.idx.data(), f.idx.size(), tidx[j]);
      if (at < 0)
        return err(HX_ERR_PRIMESET, "DoubleCRT::Op: incompatible index sets (the output has no row for prime %d of term %d)",
                   tidx[j], t);
      if (trow[(size_t)at * n + t] >= 0)
        return err(HX_ERR_INVALID, "term %d lists prime %d twice", t, tidx[j]);
      trow[(size_t)at * n + t] = (int)j;
    }
    if (!aligned16(hxi::poly_rows_read(in0[t]), in1 ? hxi::poly_rows_read(in1[t]) : nullptr))
      return err(HX_ERR_INVALID, "term %d: rows are not 16-byte aligned", t);
  }
  if (rows == 0)
    return HX_OK;
  // table (kernel's layout): per output row and term the two row bases and the weight, then the addends
  Table tab;
  RC(tab.acquire(f, (size_t)rows * (3 * (size_t)n + 1)));
  // the outputs first: one that still shares an input's rows (a lazy hx_poly_copy) lets go of them before the inputs'
  // addresses are read into the table
  uint64_t *o0 = nullptr, *o1 = nullptr;
  RC(hxi::poly_rows_write(out0, &o0));
  if (out1)
    RC(hxi::poly_rows_write(out1, &o1));
  if (!aligned16(o0, o1))
    return err(HX_ERR_INVALID, "output rows are not 16-byte aligned");
  const size_t rw = (size_t)f.batch * f.N;
  for (int t = 0; t < n; t++) {
    const uint64_t* p0 = hxi::poly_rows_read(in0[t]);
    const uint64_t* p1 = in1 ? hxi::poly_rows_read(in1[t]) : nullptr;
    for (int r = 0; r < rows; r++) {
      const int at = trow[(size_t)r * n + t];
      uint64_t* e = tab.h + 3 * ((size_t)r * n + t);
      e[0] = at < 0 ? 0 : (uint64_t)(uintptr_t)(p0 + (size_t)at * rw);
      e[1] = at < 0 || !p1 ? 0 : (uint64_t)(uintptr_t)(p1 + (size_t)at * rw);
      e[2] = w[(size_t)t * rows + r];
    }
  }
  for (int r = 0; r < rows; r++)
    tab.h[3 * (size_t)rows * n + r] = addend ? addend[r] : 0;
  RC(tab.commit(f.v.stream));
  HX_LAUNCH_PW(lin_comb_kernel, out1 ? 2 : 1, f.bp != 1, 1, 4, f.grid(), f.v.stream, o0, o1, hx::as_ro(tab.d), n, rows, f.batch,
               f.N, f.map, f.primes);
  CK(hipGetLastError());
  return HX_OK;
}

extern "C" int hx_tensor_sum(hx_poly* o0, hx_poly* o1, hx_poly* o2, const hx_poly* const* a0, const hx_poly* const* a1,
                             const hx_poly* const* b0, const hx_poly* const* b1, int n)
{
  if (!o0 || !o1 || !o2 || !a0 || !a1 || !b0 || !b1)
    return err(HX_ERR_INVALID, "null argument");
  if (n < 1)
    return err(HX_ERR_INVALID, "hx_tensor_sum needs at least one term (n = %d)", n);
  if (o0 == o1 || o0 == o2 || o1 == o2)
    return err(HX_ERR_INVALID, "two outputs are the same poly");
  const hx_poly* const* in[4] = {a0, a1, b0, b1};
  static const char* const name[4] = {"a0", "a1", "b0", "b1"};
  hx_ctx* ctx = hxi::poly_ctx(o0);
  if (hxi::poly_ctx(o1) != ctx || hxi::poly_ctx(o2) != ctx)
    return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  for (int t = 0; t < n; t++)
    for (int j = 0; j < 4; j++) {
      const hx_poly* p = in[j][t];
      if (!p)
        return err(HX_ERR_INVALID, "null poly (%s[%d])", name[j], t);
      if (hxi::poly_ctx(p) != ctx)
        return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects (%s[%d])", name[j], t);
      if (p == o0 || p == o1 || p == o2)
        return err(HX_ERR_INVALID, "an output is also an input (%s[%d])", name[j], t);
    }
  Frame f;
  RC(f.open(ctx, o0, "hx_tensor_sum uploads a pointer table and cannot be captured in a graph"));
  RC(same_shape(o1, f, "o1 differs from o0 in batch or prime set"));
  RC(same_shape(o2, f, "o2 differs from o0 in batch or prime set"));
  RC(f.even("hx_tensor_sum"));
  for (int t = 0; t < n; t++)
    for (int j = 0; j < 4; j++) {
      RC(same_shape(in[j][t], f, "%s[%d] differs from o0 in batch or prime set", name[j], t));
      if (!aligned16(hxi::poly_rows_read(in[j][t])))
        return err(HX_ERR_INVALID, "%s[%d]: rows are not 16-byte aligned", name[j], t);
    }
  if (f.rows == 0)
    return HX_OK;
  // table (kernel's layout): the bases of a0, a1, b0, b1
  Table tab;
  RC(tab.acquire(f, 4 * (size_t)n));
  // the outputs first: one that still shares a poly's rows (a lazy hx_poly_copy) lets go of them before the inputs'
  // addresses are read into the table
  uint64_t* o[3] = {nullptr, nullptr, nullptr};
  RC(hxi::poly_rows_write(o0, &o[0]));
  RC(hxi::poly_rows_write(o1, &o[1]));
  RC(hxi::poly_rows_write(o2, &o[2]));
  if (!aligned16(o[0], o[1], o[2]))
    return err(HX_ERR_INVALID, "output rows are not 16-byte aligned");
  for (int j = 0; j < 4; j++)
    for (int t = 0; t < n; t++)
      tab.h[(size_t)j * n + t] = (uint64_t)(uintptr_t)hxi::poly_rows_read(in[j][t]);
  RC(tab.commit(f.v.stream));
  // (BP = 4 holds 24 128-bit accumulators and 16 operand vectors without scratch: DESIGN.md 3.9r)
  HX_LAUNCH_W(f.bp != 1, (hx::tensor_sum_kernel<1>), (hx::tensor_sum_kernel<4>), f.grid(), f.v.stream, o[0], o[1], o[2],
              hx::as_ro(tab.d), n, f.batch, f.N, f.map, f.primes);
  CK(hipGetLastError());
  return HX_OK;
}

extern "C" int hx_table_tensor_sum(hx_poly* o0, hx_poly* o1, hx_poly* o2, const hx_poly* const* a0, const hx_poly* const* a1,
                                   int k, const hx_poly* const* b0, const hx_poly* const* b1, int l, const hx_poly* table,
                                   int size)
{
  if (!o0 || !o1 || !o2 || !a0 || !a1 || !b0 || !b1 || !table)
    return err(HX_ERR_INVALID, "null argument");
  if (k < 1 || l < 1)
    return err(HX_ERR_INVALID, "hx_table_tensor_sum needs at least one a and one b (k = %d, l = %d)", k, l);
  if (k > hx::TTS_MAX || l > hx::TTS_MAX)
    return err(HX_ERR_UNSUPPORTED, "hx_table_tensor_sum takes at most %d a and %d b (k = %d, l = %d)", hx::TTS_MAX,
               hx::TTS_MAX, k, l);
  if (size < 1 || size > k * l)
    return err(HX_ERR_INVALID, "hx_table_tensor_sum: size %d is not in [1, k l] = [1, %d]", size, k * l);
  if (o0 == o1 || o0 == o2 || o1 == o2)
    return err(HX_ERR_INVALID, "two outputs are the same poly");
  if (table == o0 || table == o1 || table == o2)
    return err(HX_ERR_INVALID, "an output is also the table");
  const hx_poly* const* in[4] = {a0, a1, b0, b1};
  const int cnt[4] = {k, k, l, l};
  static const char* const name[4] = {"a0", "a1", "b0", "b1"};
  hx_ctx* ctx = hxi::poly_ctx(o0);
  if (hxi::poly_ctx(o1) != ctx || hxi::poly_ctx(o2) != ctx || hxi::poly_ctx(table) != ctx)
    return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  for (int j = 0; j < 4; j++)
    for (int t = 0; t < cnt[j]; t++) {
      const hx_poly* p = in[j][t];
      if (!p)
        return err(HX_ERR_INVALID, "null poly (%s[%d])", name[j], t);
      if (hxi::poly_ctx(p) != ctx)
        return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects (%s[%d])", name[j], t);
      if (p == o0 || p == o1 || p == o2)
        return err(HX_ERR_INVALID, "an output is also an input (%s[%d])", name[j], t);
    }
  Frame f;
  RC(f.open(ctx, o0, "hx_table_tensor_sum uploads a pointer table and cannot be captured in a graph"));
  RC(same_shape(o1, f, "o1 differs from o0 in batch or prime set"));
  RC(same_shape(o2, f, "o2 differs from o0 in batch or prime set"));
  RC(f.even("hx_table_tensor_sum"));
  for (int j = 0; j < 4; j++)
    for (int t = 0; t < cnt[j]; t++) {
      RC(same_shape(in[j][t], f, "%s[%d] differs from o0 in batch or prime set", name[j], t));
      if (!aligned16(hxi::poly_rows_read(in[j][t])))
        return err(HX_ERR_INVALID, "%s[%d]: rows are not 16-byte aligned", name[j], t);
    }
  // the table: its batch axis is the table index, and it has a row for every prime of o0 (in any order, among others)
  int tbatch = 0;
  std::vector<int> tidx;
  RC(shape_of(table, &tbatch, &tidx));
  if (tbatch != size)
    return err(HX_ERR_INVALID, "the table has batch %d, not size = %d", tbatch, size);
  hx::RowMap2 map;
  for (int r = 0; r < f.rows; r++) {
    const int at = row_of(tidx.data(), tidx.size(), f.idx[r]);
    if (at < 0)
      return err(HX_ERR_PRIMESET, "DoubleCRT::Op: incompatible index sets (the table has no row for prime %d)", f.idx[r]);
    map.p[r] = (uint16_t)f.idx[r];
    map.brow[r] = (uint16_t)at;
  }
  const uint64_t* tp = hxi::poly_rows_read(table);
  if (!aligned16(tp))
    return err(HX_ERR_INVALID, "table: rows are not 16-byte aligned");
  if (f.rows == 0)
    return HX_OK;
  // table (kernel's layout): the bases of a0, a1, b0, b1
  Table tab;
  RC(tab.acquire(f, 2 * ((size_t)k + l)));
  // the outputs first: one that still shares a poly's rows (a lazy hx_poly_copy) lets go of them before the inputs'
  // addresses are read into the table
  uint64_t* o[3] = {nullptr, nullptr, nullptr};
  RC(hxi::poly_rows_write(o0, &o[0]));
  RC(hxi::poly_rows_write(o1, &o[1]));
  RC(hxi::poly_rows_write(o2, &o[2]));
  if (!aligned16(o[0], o[1], o[2]))
    return err(HX_ERR_INVALID, "output rows are not 16-byte aligned");
  uint64_t* w = tab.h;
  for (int j = 0; j < 4; j++)
    for (int t = 0; t < cnt[j]; t++)
      *w++ = (uint64_t)(uintptr_t)hxi::poly_rows_read(in[j][t]);
  RC(tab.commit(f.v.stream));
  // (a thread takes 2 batch elements and 4 values of j: 44 128-bit accumulators without scratch)
  f.bp = f.batch == 1 ? 1 : 2;
  HX_LAUNCH_W(f.bp != 1, (hx::table_tensor_sum_kernel<1>), (hx::table_tensor_sum_kernel<2>), f.grid(), f.v.stream, o[0], o[1],
              o[2], hx::as_ro(tab.d), hxi::poly_rows_read(table), k, l, size, f.batch, f.N, map, f.primes);
  CK(hipGetLastError());
  return HX_OK;
}

extern "C" int hx_hoisted_automorph_sum(const hx_poly* digits, const hx_poly* c0, const hx_poly* c1, const uint64_t* k,
                                        const hx_ksk* const* W, int n, const int* sp_idx, int nsp, hx_poly* out0,
                                        hx_poly* out1)
{
  if (!digits || !c0 || !c1 || !k || !W || !out0 || !out1 || (nsp > 0 && !sp_idx) || nsp < 0)
    return err(HX_ERR_INVALID, "null argument");
  if (n < 1)
    return err(HX_ERR_INVALID, "hx_hoisted_automorph_sum needs at least one term (n = %d)", n);
  if (out0 == out1 || out0 == digits || out0 == c0 || out0 == c1 || out1 == digits || out1 == c0 || out1 == c1)
    return err(HX_ERR_INVALID, "an output is also an input, or out0 and out1 are the same poly");
  hx_ctx* ctx = hxi::poly_ctx(c0);
  if (hxi::poly_ctx(digits) != ctx || hxi::poly_ctx(c1) != ctx || hxi::poly_ctx(out0) != ctx || hxi::poly_ctx(out1) != ctx)
    return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  std::vector<hxi::KskView> kv(n);
  for (int t = 0; t < n; t++) {
    if (!W[t])
      return err(HX_ERR_INVALID, "null key-switching matrix (term %d)", t);
    hxi::ksk_view(W[t], &kv[t]);
    if (kv[t].ctx != ctx)
      return err(HX_ERR_INVALID, "the key-switching matrix of term %d belongs to another context", t);
  }
  // the frame's rows are the outputs': c0's primes followed by the special primes (set once those are checked)
  Frame f;
  RC(f.enter(ctx, "hx_hoisted_automorph_sum uploads a table of key rows and cannot be captured in a graph"));
  const uint64_t m = f.v.m;
  for (int t = 0; t < n; t++)
    if (hxh::gcd(k[t] % m, m) != 1)
      return err(HX_ERR_INVALID, "DoubleCRT::automorph: k[%d] = %llu is not in Zm*", t, (unsigned long long)k[t]);
  RC(shape_of(c0, &f.batch, &f.idx));
  RC(same_shape(c1, f, "c0 and c1 differ in batch or prime set"));
  const int L = (int)f.idx.size();
  if (L == 0)
    return err(HX_ERR_INVALID, "c0 has no rows");
  int nprimes = 0;
  RC(hx_ctx_num_primes(ctx, &nprimes));
  std::vector<int> all(f.idx);
  for (int i = 0; i < nsp; i++) {
    if (sp_idx[i] < 0 || sp_idx[i] >= nprimes || row_of(all.data(), all.size(), sp_idx[i]) >= 0)
      return err(HX_ERR_INVALID, "special prime %d is not a prime of the context, or is listed twice or among c0's", sp_idx[i]);
    all.push_back(sp_idx[i]);
  }
  RC(f.set_rows(all));
  const int nall = f.rows;
  int b2 = 0;
  std::vector<int> other;
  RC(shape_of(digits, &b2, &other));
  if (b2 != f.batch || other.empty() || other.size() % nall != 0)
    return err(HX_ERR_INVALID, "the digit block differs in batch, or is not a whole number of digits on %d rows", nall);
  const int ndig = (int)other.size() / nall;
  for (int d = 0; d < ndig; d++)
    for (int r = 0; r < nall; r++)
      if (other[(size_t)d * nall + r] != all[r])
        return err(HX_ERR_INVALID, "digit rows do not match the ciphertext's primes followed by the special primes");
  for (hx_poly* o : {out0, out1}) {
    RC(shape_of(o, &b2, &other));
    if (b2 != f.batch)
      return err(HX_ERR_INVALID, "an output has batch %d, the operands %d", b2, f.batch);
  }
  // wrow[r n + t]: the row of W[t] on the prime of output row r (rows by prime index, the leading ndig digits)
  std::vector<int> wrow((size_t)nall * n);
  for (int t = 0; t < n; t++) {
    if (kv[t].ndig < ndig)
      return err(HX_ERR_INVALID, "W must have as many columns as there are digits (term %d: %d, the block has %d)", t,
                 kv[t].ndig, ndig);
    for (int r = 0; r < nall; r++) {
      const int at = row_of(kv[t].row_idx, kv[t].nrows, all[r]);
      if (at < 0)
        return err(HX_ERR_PRIMESET, "No key-switching matrix row for prime %d (term %d)", all[r], t);
      wrow[(size_t)r * n + t] = at;
    }
  }
  // out0's accumulator takes Psp c0, n times Psp sigma(c0) and n ndig products of a digit word by a key word
  if ((long long)n * (ndig + 1) + 1 > hx::MAD_CHUNK)
    return err(HX_ERR_UNSUPPORTED, "hx_hoisted_automorph_sum: n (ndig + 1) + 1 = %lld products per word, the accumulators take %d",
               (long long)n * (ndig + 1) + 1, hx::MAD_CHUNK);
  const uint32_t N = f.N;
  const hipStream_t st = f.v.stream;
  // table (kernels' layout): k[t] mod m; per output row and term the two key row bases and the digit stride; Psp per row
  Table tab;
  RC(tab.acquire(f, (size_t)n + (size_t)nall * (3 * (size_t)n + 1)));
  uint32_t* perm = nullptr;
  RC(tab.perm(f, (size_t)n * N, &perm));
  // all checks have passed: the outputs take their shape
  uint64_t *o0 = nullptr, *o1 = nullptr;
  RC(hxi::poly_rows_reshape(out0, all.data(), nall, &o0));
  RC(hxi::poly_rows_reshape(out1, all.data(), nall, &o1));
  uint64_t* h = tab.h;
  for (int t = 0; t < n; t++)
    h[t] = k[t] % m;
  for (int r = 0; r < nall; r++) {
    uint64_t q = 0;
    RC(hx_ctx_prime(ctx, all[r], &q, nullptr));
    for (int t = 0; t < n; t++) {
      uint64_t* e = h + n + 3 * ((size_t)r * n + t);
      const size_t at = (size_t)wrow[(size_t)r * n + t] * N;
      e[0] = (uint64_t)(uintptr_t)(kv[t].d_b + at);
      e[1] = (uint64_t)(uintptr_t)(kv[t].d_a + at);
      e[2] = (uint64_t)kv[t].nrows * N;
    }
    uint64_t psp = 1 % q;
    for (int i = 0; i < nsp; i++) {
      uint64_t qs = 0;
      RC(hx_ctx_prime(ctx, sp_idx[i], &qs, nullptr));
      psp = hxh::mulmod(psp, qs % q, q);
    }
    h[n + 3 * (size_t)nall * n + r] = psp;
  }
  RC(tab.commit(st));
  HX_LAUNCH(hx::hoisted_perm_kernel, dim3((N + 255) / 256, (unsigned)n), dim3(256), 0, st, perm, f.v.d_zms, f.v.d_zms_index, N, m,
            hx::as_ro(tab.d), (int)f.v.pow2);
  CK(hipGetLastError());
  dim3 grid = f.grid();
  grid.x = (N + 255) / 256;   // one coefficient per thread
  const uint64_t *dg = hxi::poly_rows_read(digits), *p0 = hxi::poly_rows_read(c0), *p1 = hxi::poly_rows_read(c1);
  HX_LAUNCH_W(f.bp != 1, (hx::hoisted_sum_kernel<1>), (hx::hoisted_sum_kernel<4>), grid, st, o0, o1, dg, p0, p1, perm,
              hx::as_ro(tab.d), n, ndig, L, nall, f.batch, N, f.map, f.primes);
  CK(hipGetLastError());
  return HX_OK;
}

extern "C" int hx_hoisted_mask_fan(const hx_poly* digits, const hx_poly* c0, const hx_poly* c1, const uint64_t* k,
                                   const hx_ksk* const* W, const hx_poly* const* A, const hx_poly* const* B, int n,
                                   const int* sp_idx, int nsp, hx_poly* const* out0, hx_poly* const* out1)
{
  if (!digits || !c0 || !c1 || !k || !W || !out0 || !out1 || (nsp > 0 && !sp_idx) || nsp < 0)
    return err(HX_ERR_INVALID, "null argument");
  if (n < 1)
    return err(HX_ERR_INVALID, "hx_hoisted_mask_fan needs at least one term (n = %d)", n);
  if (n > hx::MAD_CHUNK)
    return err(HX_ERR_UNSUPPORTED, "hx_hoisted_mask_fan takes at most %d terms (n = %d)", hx::MAD_CHUNK, n);
  hx_ctx* ctx = hxi::poly_ctx(c0);
  if (hxi::poly_ctx(digits) != ctx || hxi::poly_ctx(c1) != ctx)
    return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  // the frame's rows are the outputs': c0's primes followed by the special primes (set once those are checked)
  Frame f;
  RC(f.enter(ctx, "hx_hoisted_mask_fan uploads a table of key rows and cannot be captured in a graph"));
  RC(f.even("hx_hoisted_mask_fan"));
  std::vector<hxi::KskView> kv(n);
  std::vector<const hx_poly*> outs, ins = {digits, c0, c1};
  for (int t = 0; t < n; t++) {
    if (!out0[t] || !out1[t])
      return err(HX_ERR_INVALID, "null output (term %d)", t);
    if (!W[t])
      return err(HX_ERR_INVALID, "null key-switching matrix (term %d)", t);
    hxi::ksk_view(W[t], &kv[t]);
    if (kv[t].ctx != ctx)
      return err(HX_ERR_INVALID, "the key-switching matrix of term %d belongs to another context", t);
    if (hxi::poly_ctx(out0[t]) != ctx || hxi::poly_ctx(out1[t]) != ctx || (A && A[t] && hxi::poly_ctx(A[t]) != ctx) ||
        (B && B[t] && hxi::poly_ctx(B[t]) != ctx))
      return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects (term %d)", t);
    outs.push_back(out0[t]);
    outs.push_back(out1[t]);
    if (A && A[t])
      ins.push_back(A[t]);
    if (B && B[t])
      ins.push_back(B[t]);
  }
  std::sort(outs.begin(), outs.end());
  if (std::adjacent_find(outs.begin(), outs.end()) != outs.end())
    return err(HX_ERR_INVALID, "two outputs are the same poly");
  for (const hx_poly* p : ins)
    if (std::binary_search(outs.begin(), outs.end(), p))
      return err(HX_ERR_INVALID, "an output is also an input or a mask");
  const uint64_t m = f.v.m;
  for (int t = 0; t < n; t++)
    if (hxh::gcd(k[t] % m, m) != 1)
      return err(HX_ERR_INVALID, "DoubleCRT::automorph: k[%d] = %llu is not in Zm*", t, (unsigned long long)k[t]);
  RC(shape_of(c0, &f.batch, &f.idx));
  RC(same_shape(c1, f, "c0 and c1 differ in batch or prime set"));
  const int L = (int)f.idx.size();
  if (L == 0)
    return err(HX_ERR_INVALID, "c0 has no rows");
  int nprimes = 0;
  RC(hx_ctx_num_primes(ctx, &nprimes));
  std::vector<int> all(f.idx);
  for (int i = 0; i < nsp; i++) {
    if (sp_idx[i] < 0 || sp_idx[i] >= nprimes || row_of(all.data(), all.size(), sp_idx[i]) >= 0)
      return err(HX_ERR_INVALID, "special prime %d is not a prime of the context, or is listed twice or among c0's", sp_idx[i]);
    all.push_back(sp_idx[i]);
  }
  RC(f.set_rows(all));
  const int nall = f.rows;
  int b2 = 0;
  std::vector<int> other;
  RC(shape_of(digits, &b2, &other));
  if (b2 != f.batch || other.empty() || other.size() % nall != 0)
    return err(HX_ERR_INVALID, "the digit block differs in batch, or is not a whole number of digits on %d rows", nall);
  const int ndig = (int)other.size() / nall;
  for (int d = 0; d < ndig; d++)
    for (int r = 0; r < nall; r++)
      if (other[(size_t)d * nall + r] != all[r])
        return err(HX_ERR_INVALID, "digit rows do not match the ciphertext's primes followed by the special primes");
  for (const hx_poly* o : outs) {
    RC(shape_of(o, &b2, &other));
    if (b2 != f.batch)
      return err(HX_ERR_INVALID, "an output has batch %d, the operands %d", b2, f.batch);
  }
  // wrow[r n + t]: the row of W[t] on the prime of output row r (rows by prime index, the leading ndig digits);
  // mrow[(2 t + i) nall + r]: the row of A_t (i = 0) or B_t (i = 1) on that prime, mper[2 t + i]: one row per batch element
  std::vector<int> wrow((size_t)nall * n), mrow((size_t)2 * n * nall, 0), mper((size_t)2 * n, 0);
  for (int t = 0; t < n; t++) {
    if (kv[t].ndig < ndig)
      return err(HX_ERR_INVALID, "W must have as many columns as there are digits (term %d: %d, the block has %d)", t,
                 kv[t].ndig, ndig);
    for (int r = 0; r < nall; r++) {
      const int at = row_of(kv[t].row_idx, kv[t].nrows, all[r]);
      if (at < 0)
        return err(HX_ERR_PRIMESET, "No key-switching matrix row for prime %d (term %d)", all[r], t);
      wrow[(size_t)r * n + t] = at;
    }
    for (int i = 0; i < 2; i++) {
      const hx_poly* mk = i == 0 ? (A ? A[t] : nullptr) : (B ? B[t] : nullptr);
      if (!mk)
        continue;
      int mb = 0;
      std::vector<int> midx;
      RC(shape_of(mk, &mb, &midx));
      if (mb != f.batch && mb != 1)
        return err(HX_ERR_INVALID, "%s[%d]: batch %d is neither 1 nor %d", i == 0 ? "A" : "B", t, mb, f.batch);
      mper[2 * (size_t)t + i] = mb == f.batch && f.batch > 1;
      for (int r = 0; r < nall; r++) {
        const int at = row_of(midx.data(), midx.size(), all[r]);
        if (at < 0)
          return err(HX_ERR_PRIMESET, "DoubleCRT::Op: incompatible index sets (%s[%d] has no row for prime %d)",
                     i == 0 ? "A" : "B", t, all[r]);
        mrow[(2 * (size_t)t + i) * nall + r] = at;
      }
    }
  }
  // the inner accumulators take Psp sigma(c0) and ndig products of a digit word by a key word
  if (ndig + 1 > hx::MAD_CHUNK)
    return err(HX_ERR_UNSUPPORTED, "hx_hoisted_mask_fan: ndig + 1 = %d products per word, the accumulators take %d", ndig + 1,
               hx::MAD_CHUNK);
  const uint32_t N = f.N;
  const hipStream_t st = f.v.stream;
  // table (kernels' layout): k[t] mod m; the output bases; per output row and term the two key row bases, the digit stride
  // and the two mask rows; Psp per row
  Table tab;
  RC(tab.acquire(f, 3 * (size_t)n + (size_t)nall * (5 * (size_t)n + 1)));
  uint32_t* perm = nullptr;
  RC(tab.perm(f, (size_t)n * N, &perm));
  // all checks have passed: the outputs take their shape, and one that still shares an input's rows (a lazy hx_poly_copy)
  // lets go of them before the inputs' addresses are read into the table
  uint64_t* h = tab.h;
  for (int t = 0; t < n; t++) {
    uint64_t *o0 = nullptr, *o1 = nullptr;
    RC(hxi::poly_rows_reshape(out0[t], all.data(), nall, &o0));
    RC(hxi::poly_rows_reshape(out1[t], all.data(), nall, &o1));
    h[t] = k[t] % m;
    h[n + t] = (uint64_t)(uintptr_t)o0;
    h[2 * (size_t)n + t] = (uint64_t)(uintptr_t)o1;
  }
  const size_t rw = (size_t)f.batch * N;
  for (int r = 0; r < nall; r++) {
    uint64_t q = 0;
    RC(hx_ctx_prime(ctx, all[r], &q, nullptr));
    for (int t = 0; t < n; t++) {
      uint64_t* e = h + 3 * (size_t)n + 5 * ((size_t)r * n + t);
      const size_t at = (size_t)wrow[(size_t)r * n + t] * N;
      e[0] = (uint64_t)(uintptr_t)(kv[t].d_b + at);
      e[1] = (uint64_t)(uintptr_t)(kv[t].d_a + at);
      e[2] = (uint64_t)kv[t].nrows * N;
      for (int i = 0; i < 2; i++) {
        const hx_poly* mk = i == 0 ? (A ? A[t] : nullptr) : (B ? B[t] : nullptr);
        const int per = mper[2 * (size_t)t + i];
        e[3 + i] = !mk ? 0
                       : (uint64_t)(uintptr_t)(hxi::poly_rows_read(mk) +
                                               (size_t)mrow[(2 * (size_t)t + i) * nall + r] * (per ? rw : (size_t)N)) |
                             (uint64_t)per;
      }
    }
    uint64_t psp = 1 % q;
    for (int i = 0; i < nsp; i++) {
      uint64_t qs = 0;
      RC(hx_ctx_prime(ctx, sp_idx[i], &qs, nullptr));
      psp = hxh::mulmod(psp, qs % q, q);
    }
    h[3 * (size_t)n + 5 * (size_t)nall * n + r] = psp;
  }
  RC(tab.commit(st));
  HX_LAUNCH(hx::hoisted_perm_kernel, dim3((N + 255) / 256, (unsigned)n), dim3(256), 0, st, perm, f.v.d_zms, f.v.d_zms_index, N, m,
            hx::as_ro(tab.d), (int)f.v.pow2);
  CK(hipGetLastError());
  dim3 grid = f.grid();
  grid.x = (N + 255) / 256;   // one coefficient per thread
  const uint64_t *dg = hxi::poly_rows_read(digits), *p0 = hxi::poly_rows_read(c0), *p1 = hxi::poly_rows_read(c1);
  // (BP = 4: DESIGN.md 3.9t has the register budget)
  HX_LAUNCH_W(f.bp != 1, (hx::hoisted_mask_fan_kernel<1>), (hx::hoisted_mask_fan_kernel<4>), grid, st, dg, p0, p1, perm,
              hx::as_ro(tab.d), n, ndig, L, nall, f.batch, N, f.map, f.primes);
  CK(hipGetLastError());
  return HX_OK;
}

extern "C" int hx_hoisted_blend(const hx_poly* digA, const hx_poly* a0, const hx_poly* a1, const hx_poly* digB,
                                const hx_poly* b0, const hx_poly* b1, const uint64_t* k, const hx_ksk* const* W,
                                const hx_poly* const* M, int n, const int* sp_idx, int nsp, hx_poly* const* out0,
                                hx_poly* const* out1)
{
  if (!digA || !a0 || !a1 || !digB || !b0 || !b1 || !k || !W || !M || !out0 || !out1 || (nsp > 0 && !sp_idx) || nsp < 0)
    return err(HX_ERR_INVALID, "null argument");
  if (n < 1)
    return err(HX_ERR_INVALID, "hx_hoisted_blend needs at least one term (n = %d)", n);
  if (n > hx::MAD_CHUNK)
    return err(HX_ERR_UNSUPPORTED, "hx_hoisted_blend takes at most %d terms (n = %d)", hx::MAD_CHUNK, n);
  hx_ctx* ctx = hxi::poly_ctx(a0);
  for (const hx_poly* p : {digA, a1, digB, b0, b1})
    if (hxi::poly_ctx(p) != ctx)
      return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  // the frame's rows are the outputs': a0's primes followed by the special primes (set once those are checked)
  Frame f;
  RC(f.enter(ctx, "hx_hoisted_blend uploads a table of key rows and cannot be captured in a graph"));
  RC(f.even("hx_hoisted_blend"));
  std::vector<hxi::KskView> kv(n);
  std::vector<const hx_poly*> outs, ins = {digA, a0, a1, digB, b0, b1};
  for (int t = 0; t < n; t++) {
    if (!out0[t] || !out1[t])
      return err(HX_ERR_INVALID, "null output (term %d)", t);
    if (!W[t])
      return err(HX_ERR_INVALID, "null key-switching matrix (term %d)", t);
    if (!M[t])
      return err(HX_ERR_INVALID, "null mask (term %d)", t);
    hxi::ksk_view(W[t], &kv[t]);
    if (kv[t].ctx != ctx)
      return err(HX_ERR_INVALID, "the key-switching matrix of term %d belongs to another context", t);
    if (hxi::poly_ctx(out0[t]) != ctx || hxi::poly_ctx(out1[t]) != ctx || hxi::poly_ctx(M[t]) != ctx)
      return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects (term %d)", t);
    outs.push_back(out0[t]);
    outs.push_back(out1[t]);
    ins.push_back(M[t]);
  }
  std::sort(outs.begin(), outs.end());
  if (std::adjacent_find(outs.begin(), outs.end()) != outs.end())
    return err(HX_ERR_INVALID, "two outputs are the same poly");
  for (const hx_poly* p : ins)
    if (std::binary_search(outs.begin(), outs.end(), p))
      return err(HX_ERR_INVALID, "an output is also an input or a mask");
  const uint64_t m = f.v.m;
  for (int t = 0; t < n; t++)
    if (hxh::gcd(k[t] % m, m) != 1)
      return err(HX_ERR_INVALID, "DoubleCRT::automorph: k[%d] = %llu is not in Zm*", t, (unsigned long long)k[t]);
  RC(shape_of(a0, &f.batch, &f.idx));
  RC(same_shape(a1, f, "a0 and a1 differ in batch or prime set"));
  RC(same_shape(b0, f, "the two operands differ in batch or prime set"));
  RC(same_shape(b1, f, "the two operands differ in batch or prime set"));
  const int L = (int)f.idx.size();
  if (L == 0)
    return err(HX_ERR_INVALID, "a0 has no rows");
  int nprimes = 0;
  RC(hx_ctx_num_primes(ctx, &nprimes));
  std::vector<int> all(f.idx);
  for (int i = 0; i < nsp; i++) {
    if (sp_idx[i] < 0 || sp_idx[i] >= nprimes || row_of(all.data(), all.size(), sp_idx[i]) >= 0)
      return err(HX_ERR_INVALID, "special prime %d is not a prime of the context, or is listed twice or among a0's", sp_idx[i]);
    all.push_back(sp_idx[i]);
  }
  RC(f.set_rows(all));
  const int nall = f.rows;
  int b2 = 0, ndig = 0;
  std::vector<int> other;
  for (int w = 0; w < 2; w++) {
    RC(shape_of(w == 0 ? digA : digB, &b2, &other));
    if (b2 != f.batch || other.empty() || other.size() % nall != 0)
      return err(HX_ERR_INVALID, "the digit block differs in batch, or is not a whole number of digits on %d rows", nall);
    if (w == 1 && (int)other.size() != ndig * nall)
      return err(HX_ERR_INVALID, "the two digit blocks differ in their number of digits (%d and %d)", ndig,
                 (int)other.size() / nall);
    ndig = (int)other.size() / nall;
    for (int d = 0; d < ndig; d++)
      for (int r = 0; r < nall; r++)
        if (other[(size_t)d * nall + r] != all[r])
          return err(HX_ERR_INVALID, "digit rows do not match the ciphertext's primes followed by the special primes");
  }
  for (const hx_poly* o : outs) {
    RC(shape_of(o, &b2, &other));
    if (b2 != f.batch)
      return err(HX_ERR_INVALID, "an output has batch %d, the operands %d", b2, f.batch);
  }
  // wrow[r n + t]: the row of W[t] on the prime of output row r (rows by prime index, the leading ndig digits);
  // mrow[t nall + r]: the row of M_t on that prime, mper[t]: one row per batch element
  std::vector<int> wrow((size_t)nall * n), mrow((size_t)n * nall, 0), mper(n, 0);
  for (int t = 0; t < n; t++) {
    if (kv[t].ndig < ndig)
      return err(HX_ERR_INVALID, "W must have as many columns as there are digits (term %d: %d, the block has %d)", t,
                 kv[t].ndig, ndig);
    for (int r = 0; r < nall; r++) {
      const int at = row_of(kv[t].row_idx, kv[t].nrows, all[r]);
      if (at < 0)
        return err(HX_ERR_PRIMESET, "No key-switching matrix row for prime %d (term %d)", all[r], t);
      wrow[(size_t)r * n + t] = at;
    }
    int mb = 0;
    std::vector<int> midx;
    RC(shape_of(M[t], &mb, &midx));
    if (mb != f.batch && mb != 1)
      return err(HX_ERR_INVALID, "M[%d]: batch %d is neither 1 nor %d", t, mb, f.batch);
    mper[t] = mb == f.batch && f.batch > 1;
    for (int r = 0; r < nall; r++) {
      const int at = row_of(midx.data(), midx.size(), all[r]);
      if (at < 0)
        return err(HX_ERR_PRIMESET, "DoubleCRT::Op: incompatible index sets (M[%d] has no row for prime %d)", t, all[r]);
      mrow[(size_t)t * nall + r] = at;
    }
  }
  // the accumulators take Psp times the blended word of the 1-part and ndig products of a blended digit word by a key word
  if (ndig + 1 > hx::MAD_CHUNK)
    return err(HX_ERR_UNSUPPORTED, "hx_hoisted_blend: ndig + 1 = %d products per word, the accumulators take %d", ndig + 1,
               hx::MAD_CHUNK);
  const uint32_t N = f.N;
  const hipStream_t st = f.v.stream;
  // table (kernels' layout): k[t] mod m; the output bases; per output row and term the two key row bases, the digit stride
  // and the mask row; Psp per row
  Table tab;
  RC(tab.acquire(f, 3 * (size_t)n + (size_t)nall * (4 * (size_t)n + 1)));
  uint32_t* perm = nullptr;
  RC(tab.perm(f, (size_t)n * N, &perm));
  // all checks have passed: the outputs take their shape, and one that still shares an input's rows (a lazy hx_poly_copy)
  // lets go of them before the inputs' addresses are read into the table
  uint64_t* h = tab.h;
  for (int t = 0; t < n; t++) {
    uint64_t *o0 = nullptr, *o1 = nullptr;
    RC(hxi::poly_rows_reshape(out0[t], all.data(), nall, &o0));
    RC(hxi::poly_rows_reshape(out1[t], all.data(), nall, &o1));
    h[t] = k[t] % m;
    h[n + t] = (uint64_t)(uintptr_t)o0;
    h[2 * (size_t)n + t] = (uint64_t)(uintptr_t)o1;
  }
  const size_t rw = (size_t)f.batch * N;
  for (int r = 0; r < nall; r++) {
    uint64_t q = 0;
    RC(hx_ctx_prime(ctx, all[r], &q, nullptr));
    for (int t = 0; t < n; t++) {
      uint64_t* e = h + 3 * (size_t)n + 4 * ((size_t)r * n + t);
      const size_t at = (size_t)wrow[(size_t)r * n + t] * N;
      e[0] = (uint64_t)(uintptr_t)(kv[t].d_b + at);
      e[1] = (uint64_t)(uintptr_t)(kv[t].d_a + at);
      e[2] = (uint64_t)kv[t].nrows * N;
      e[3] = (uint64_t)(uintptr_t)(hxi::poly_rows_read(M[t]) + (size_t)mrow[(size_t)t * nall + r] * (mper[t] ? rw : (size_t)N)) |
             (uint64_t)mper[t];
    }
    uint64_t psp = 1 % q;
    for (int i = 0; i < nsp; i++) {
      uint64_t qs = 0;
      RC(hx_ctx_prime(ctx, sp_idx[i], &qs, nullptr));
      psp = hxh::mulmod(psp, qs % q, q);
    }
    h[3 * (size_t)n + 4 * (size_t)nall * n + r] = psp;
  }
  RC(tab.commit(st));
  HX_LAUNCH(hx::hoisted_perm_kernel, dim3((N + 255) / 256, (unsigned)n), dim3(256), 0, st, perm, f.v.d_zms, f.v.d_zms_index, N, m,
            hx::as_ro(tab.d), (int)f.v.pow2);
  CK(hipGetLastError());
  dim3 grid = f.grid();
  grid.x = (N + 255) / 256;   // one coefficient per thread
  const uint64_t *da = hxi::poly_rows_read(digA), *db = hxi::poly_rows_read(digB);
  const uint64_t *pa = hxi::poly_rows_read(a0), *pb = hxi::poly_rows_read(b0);
  // (BP = 4: DESIGN.md 3.9u has the register budget; a1 and b1 are checked, not read -- the key switch replaces them)
  HX_LAUNCH_W(f.bp != 1, (hx::hoisted_blend_kernel<1>), (hx::hoisted_blend_kernel<4>), grid, st, da, db, pa, pb, perm,
              hx::as_ro(tab.d), n, ndig, L, nall, f.batch, N, f.map, f.primes);
  CK(hipGetLastError());
  return HX_OK;
}

extern "C" int hx_poly_extract(hx_poly* dst, const hx_poly* src, int b)
{
  if (!dst || !src || dst == src)
    return err(HX_ERR_INVALID, "null argument");
  hx_ctx* ctx = hxi::poly_ctx(src);
  if (hxi::poly_ctx(dst) != ctx)
    return err(HX_ERR_INVALID, "DoubleCRT::Op: incompatible objects");
  Frame f;   // (src's shape: any number of rows, any N)
  RC(f.enter(ctx, nullptr));
  int db = 0;
  std::vector<int> didx;
  RC(shape_of(src, &f.batch, &f.idx));
  RC(shape_of(dst, &db, &didx));
  if (db != 1 || didx != f.idx)
    return err(HX_ERR_INVALID, "hx_poly_extract: dst must have batch 1 and the prime set of src");
  if (b < 0 || b >= f.batch)
    return err(HX_ERR_INVALID, "hx_poly_extract: batch element %d of %d", b, f.batch);
  if (f.idx.empty())
    return HX_OK;
  uint64_t* d = nullptr;
  RC(hxi::poly_rows_write(dst, &d));
  const uint64_t* sp = hxi::poly_rows_read(src);
  const size_t rowb = (size_t)f.N * 8;
  CK(hipMemcpy2DAsync(d, rowb, sp + (size_t)b * f.N, rowb * f.batch, rowb, f.idx.size(), hipMemcpyDeviceToDevice,
                      f.v.stream));
  return HX_OK;
}
