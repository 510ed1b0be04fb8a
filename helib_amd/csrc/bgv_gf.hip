// bgv_gf.hip -- C ABI of BGV slot encoding and decoding with slots in GF(p^d) = Z_p[X] / G, G = F_0, d = ord_m(p), r = 1
// (include/helib_amd.h: hx_bgv_gf_create, hx_bgv_gf_create_pr, hx_bgv_gf_create_gens, hx_bgv_gf_space, hx_bgv_gf_info, hx_bgv_gf_encode,
// hx_bgv_gf_decode, hx_bgv_gf_embed):
// EncryptedArray(context, G) over the G = F_0 branches of PAlgebraModDerived (src/PAlgebra.cpp:1064-1067, 1096-1100,
// 1168-1186, 1243-1278).  The tables are bgv_gf.h's; with B elements, n slots, N = phi(m):
//   encode   c[b][i] = alpha[b][i] A_i                                   (bgv_gf_map_kernel: B n d^2 multiply-adds)
//            W[b][k] = sum_i sum_(j<d) c[b][i][j] E[i][k - j],  k < N + d - 1   (bgv_gf_encode_kernel: B n d (N + d - 1))
//            H[b][k] = W[b][k] + sum_(u<d-1) W[b][N + u] T[u][k]         (bgv_gf_fold_kernel: B N (d - 1))
//   decode   u[b][i][j] = sum_k w[b][k] Rx[i][k + j]                     (bgv_gf_decode_kernel: B n d N)
//            alpha[b][i] = M_i u[b][i]                                   (bgv_gf_map_kernel)
// all modulo p on the vector ALU as in bgv_crt.hip: 32-bit operands, 64-bit accumulators reduced once every `limit`
// multiply-adds of ONE accumulator (a slot contributes d of them to an encode accumulator).  c = alpha A is formed by a
// kernel of its own ahead of the encode: formed while staging it would be redone for each of the N / 256 coefficient
// tiles.  The fold is a launch of its own: the top words of W belong to the last coefficient tile, another workgroup.
// Around them the pieces every BGV slot path shares (bgv_encode.h).  Everything of an encode behind "c is on the device"
// is hxg::gf_encode_words (bgv_gf_tail.h): hx_bgv_gf_encode fills c with the upload and bgv_gf_map_kernel,
// hx_bgv_gf_encode_gathered (bgv_gf_linalg.hip) with bgv_gf_gather_map_kernel.
// At r > 1 (hx_bgv_gf_create_pr: slots in the Galois ring Z_(p^r)[X] / G, G the Hensel lift of F_0) the modulus of all of
// these is p^r < 2^31 (in the kernels' `p`; the table keeps the prime beside it) and the kernels are the same code: as
// in bgv_crt.hip none of them needs a prime -- bgv_red's quotient estimate is short by at most 1 for any q >= 2, Shoup's
// product lies in [0, 2q) for any q and w < q -- and every accumulator is bounded by `limit` = floor(2^64 / p^(2r)),
// which build_crt computes from p^r (lazy_limit) and which is >= 4 because p^r < 2^31.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "bgv_gf.h"
#include "bgv_encode.h"
#include "bgv_gf_tail.h"

namespace hx {

constexpr int GF_TB = 16;     // batch elements of a tile (four per thread)
constexpr int GF_EK = 256;    // encode: coefficients of a tile (lane + 64 kk)
constexpr int GF_ES = 16;     // encode: most slots staged per step
constexpr int GF_ET = 64;     // encode: most (slot, tap) terms staged per step, >= GF_MAX_D
constexpr int GF_HALO = 64;   // encode: words kept in front of a staged row of E (>= d - 1 rounded up to 4)
constexpr int GF_DI = 64;     // decode: slots of a tile (one per lane)
constexpr int GF_DK = 32;     // decode: coefficients staged per step
static_assert(GF_ET >= (int)hxc::GF_MAX_D && GF_HALO >= (int)hxc::GF_MAX_D - 1 && GF_HALO % 4 == 0, "staging sizes");

// out[b][i][j] = sum_l (in[b][i][l] mod p) mat[i][l][j] mod p: the per-slot d x d maps (A in front of an encode, M
// behind a decode).  One thread per output word; `total` = batch nslots d.
template <typename TO>
__global__ void __launch_bounds__(256)
bgv_gf_map_kernel(const int64_t* __restrict__ in, const uint32_t* __restrict__ mat, uint32_t nslots, uint32_t d, size_t total,
                  uint64_t p, uint64_t mu, uint32_t limit, TO* __restrict__ out)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const size_t bi = idx / d;
    const uint32_t j = (uint32_t)(idx - bi * d), i = (uint32_t)(bi % nslots);
    const int64_t* v = in + bi * d;
    const uint32_t* mt = mat + (size_t)i * d * d + j;
    uint64_t acc = 0;
    uint32_t left = limit;
    for (uint32_t l = 0; l < d; l++) {
      acc += bgv_red_signed(v[l], p, mu) * mt[(size_t)l * d];
      if (--left == 0) {
        acc = bgv_red(acc, p, mu);
        left = limit;
      }
    }
    out[idx] = (TO)bgv_red(acc, p, mu);
  }
}

// W[b][k] = sum_i sum_(j<d) c[b][i][j] E[i][k - j] mod p for k < Nw = N + d - 1 (E = 0 outside its row).
// c: [batch][nslots d] words < p, E: [nslots][ld] words < p, ld a multiple of 4 with zeros behind N, W: [batch][Nw].
// A workgroup takes tiles of 16 elements x 256 coefficients; thread (cg, bg) holds elements 4 bg .. 4 bg + 3 at the
// coefficients k0 + cg + 64 kk, so that a wave reads 64 consecutive words of a staged row whatever the tap.  Per step S
// = min(16, 64 / d) slots go through the LDS: their rows of E from k0 - halo to k0 + 255 (16-byte loads) and their S d
// words of c for the 16 elements.  Algorithmic bytes: 4 nslots (ld + halo N / 256) per 16 elements + 4 batch nslots d
// per coefficient tile read, 8 batch Nw written.
__global__ void __launch_bounds__(256)
bgv_gf_encode_kernel(const uint32_t* __restrict__ c, const uint32_t* __restrict__ E, uint32_t nslots, uint32_t d, uint32_t Nw,
                     uint32_t ld, int batch, uint64_t p, uint64_t mu, uint32_t limit, uint64_t* __restrict__ W)
{
  __shared__ __attribute__((aligned(16))) uint32_t sE[GF_ES][GF_HALO + GF_EK];
  __shared__ uint4 sC[GF_ET][GF_TB / 4];   // [term][element]
  const uint32_t tid = threadIdx.x, cg = tid & 63, bg = tid >> 6;
  const uint32_t S = min((uint32_t)GF_ES, max(1u, (uint32_t)GF_ET / d));
  const uint32_t halo = (d - 1 + 3) / 4 * 4, rowq = (halo + GF_EK) / 4;
  const size_t terms = (size_t)nslots * d;
  const uint32_t ktiles = (Nw + GF_EK - 1) / GF_EK, btiles = ((uint32_t)batch + GF_TB - 1) / GF_TB;
  for (uint32_t tile = blockIdx.x; tile < ktiles * btiles; tile += gridDim.x) {
    const uint32_t k0 = (tile % ktiles) * GF_EK, b0 = (tile / ktiles) * GF_TB;
    uint64_t acc[4][4] = {};
    uint32_t left = limit;
    for (uint32_t i0 = 0; i0 < nslots; i0 += S) {
      const uint32_t sn = min(S, nslots - i0), tn = sn * d;
      __syncthreads();   // the previous step's readers are done
      for (uint32_t idx = tid; idx < sn * rowq; idx += 256) {
        const uint32_t s = idx / rowq, q = idx - s * rowq;
        const int64_t k = (int64_t)k0 - halo + 4 * q;   // a multiple of 4: the four words are inside the row or outside
        *reinterpret_cast<uint4*>(&sE[s][GF_HALO - halo + 4 * q]) =
            (k >= 0 && k < (int64_t)ld) ? *reinterpret_cast<const uint4*>(E + (size_t)(i0 + s) * ld + k) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint32_t bl = bg + 4 * r, b = b0 + bl;
        reinterpret_cast<uint32_t*>(sC)[cg * GF_TB + bl] =
            (cg < tn && b < (uint32_t)batch) ? c[(size_t)b * terms + (size_t)i0 * d + cg] : 0u;
      }
      __syncthreads();
      for (uint32_t s = 0; s < sn; s++) {
        const uint32_t* er = &sE[s][GF_HALO + cg];
        const uint4* cr = &sC[s * d][bg];
#pragma unroll 2
        for (uint32_t j = 0; j < d; j++) {
          const uint4 cv = cr[j * (GF_TB / 4)];
          const uint32_t bv[4] = {cv.x, cv.y, cv.z, cv.w};
          uint32_t ev[4];
#pragma unroll
          for (int kk = 0; kk < 4; kk++)
            ev[kk] = er[64 * kk - (int)j];
#pragma unroll
          for (int bb = 0; bb < 4; bb++)
#pragma unroll
            for (int kk = 0; kk < 4; kk++)
              acc[bb][kk] += (uint64_t)bv[bb] * ev[kk];
          if (--left == 0) {   // (uniform) one more term could pass 2^64
#pragma unroll
            for (int bb = 0; bb < 4; bb++)
#pragma unroll
              for (int kk = 0; kk < 4; kk++)
                acc[bb][kk] = bgv_red(acc[bb][kk], p, mu);
            left = limit;
          }
        }
      }
    }
#pragma unroll
    for (int bb = 0; bb < 4; bb++) {
      const uint32_t b = b0 + 4 * bg + bb;
      if (b >= (uint32_t)batch)
        continue;
#pragma unroll
      for (int kk = 0; kk < 4; kk++) {
        const uint32_t k = k0 + cg + 64 * kk;
        if (k < Nw)
          W[(size_t)b * Nw + k] = bgv_red(acc[bb][kk], p, mu);
      }
    }
  }
}

// H[b][k] = W[b][k] + sum_(u<d-1) W[b][N + u] T[u][k] mod p for k < N: the top words of the sliding window brought
// back below Phi_m.  One thread per output word.  Reads 8 batch Nw + 4 (d - 1) N per element, writes 8 batch N.
__global__ void __launch_bounds__(256)
bgv_gf_fold_kernel(const uint64_t* __restrict__ W, const uint32_t* __restrict__ T, uint32_t N, uint32_t Nw, uint32_t ld, uint32_t d,
                   size_t total, uint64_t p, uint64_t mu, uint32_t limit, uint64_t* __restrict__ H)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const size_t b = idx / N;
    const uint32_t k = (uint32_t)(idx - b * N);
    const uint64_t* w = W + b * Nw;
    uint64_t acc = w[k];
    uint32_t left = limit;
    for (uint32_t u = 0; u + 1 < d; u++) {
      acc += w[N + u] * T[(size_t)u * ld + k];
      if (--left == 0) {
        acc = bgv_red(acc, p, mu);
        left = limit;
      }
    }
    H[idx] = bgv_red(acc, p, mu);
  }
}

// u[b][i][j] = sum_k w[b][k] Rx[i][k + j] mod p for j < d.  w: [batch][N] words < p (N even; wvec: the buffer is
// 16-byte aligned), Rx: [nslots][ldr] words < p, ldr a multiple of 4 with zeros behind N + d - 1, u: [batch][nslots][d].
// A workgroup takes tiles of 16 elements x 64 slots x JC values of j (j0 a multiple of JC); lane = slot, a thread
// holds 4 x JC accumulators.  Per 32 coefficients: 64 rows of 32 + JC - 1 words of Rx from k0 + j0 on (16-byte loads)
// and 16 x 32 of w go through the LDS; a thread reads a window of 4 + JC - 1 words of its row for four coefficients.
// JC = 1 is bgv_crt_decode_kernel.  Algorithmic bytes: 4 nslots ldr (1 + (JC - 1) / 32) d / JC per 16 elements +
// 8 batch N d / JC per 64 slots read, 8 batch nslots d written.
template <int JC>
__global__ void __launch_bounds__(256)
bgv_gf_decode_kernel(const uint64_t* __restrict__ w, const uint32_t* __restrict__ Rx, uint32_t nslots, uint32_t N, uint32_t ldr,
                     uint32_t d, int batch, uint64_t p, uint64_t mu, uint32_t limit, int wvec, int64_t* __restrict__ u)
{
  constexpr int EXT = JC > 1 ? (JC - 1 + 3) / 4 * 4 : 0;   // words staged behind the 32
  constexpr int RQ = (GF_DK + EXT) / 4;                    // 16-byte loads per staged row
  constexpr int RLD = JC > 1 ? 44 : 36;                    // words between LDS rows (16-byte aligned, spread over the banks)
  constexpr int NQ = (4 + JC - 1 + 3) / 4;                 // 16-byte reads per window
  static_assert(GF_DK + EXT <= RLD && 4 * (GF_DK / 4 - 1) + 4 * NQ <= GF_DK + EXT, "the window stays inside the staged row");
  __shared__ __attribute__((aligned(16))) uint32_t sR[GF_DI][RLD];
  __shared__ __attribute__((aligned(16))) uint32_t sW[GF_TB][36];
  const uint32_t tid = threadIdx.x, si = tid & 63, bg = tid >> 6;
  const uint32_t itiles = (nslots + GF_DI - 1) / GF_DI, btiles = ((uint32_t)batch + GF_TB - 1) / GF_TB, jchunks = (d + JC - 1) / JC;
  for (uint32_t tile = blockIdx.x; tile < itiles * btiles * jchunks; tile += gridDim.x) {
    const uint32_t j0 = (tile % jchunks) * JC, rest = tile / jchunks;
    const uint32_t i0 = (rest % itiles) * GF_DI, b0 = (rest / itiles) * GF_TB;
    uint64_t acc[4][JC] = {};
    uint32_t left = limit;
    for (uint32_t k0 = 0; k0 < N; k0 += GF_DK) {
      __syncthreads();
      for (uint32_t idx = tid; idx < GF_DI * RQ; idx += 256) {
        const uint32_t row = idx / RQ, q = idx % RQ, i = i0 + row, k = k0 + j0 + 4 * q;
        *reinterpret_cast<uint4*>(&sR[row][4 * q]) =
            (i < nslots && k < ldr) ? *reinterpret_cast<const uint4*>(Rx + (size_t)i * ldr + k) : make_uint4(0, 0, 0, 0);
      }
      {
        const uint32_t row = tid >> 4, c = tid & 15, b = b0 + row, k = k0 + 2 * c;
        ulonglong2 v = make_ulonglong2(0, 0);
        if (b < (uint32_t)batch && k < N) {
          const uint64_t* src = w + (size_t)b * N + k;
          if (wvec) {
            v = *reinterpret_cast<const ulonglong2*>(src);   // k + 1 < N: both are even
          } else {
            v.x = src[0];
            v.y = k + 1 < N ? src[1] : 0;
          }
        }
        sW[row][2 * c] = (uint32_t)v.x;
        sW[row][2 * c + 1] = (uint32_t)v.y;
      }
      __syncthreads();
#pragma unroll 2
      for (int c = 0; c < GF_DK / 4; c++) {
        uint32_t r[4 * NQ];
#pragma unroll
        for (int q = 0; q < NQ; q++) {
          const uint4 r4 = *reinterpret_cast<const uint4*>(&sR[si][4 * c + 4 * q]);
          r[4 * q] = r4.x;
          r[4 * q + 1] = r4.y;
          r[4 * q + 2] = r4.z;
          r[4 * q + 3] = r4.w;
        }
#pragma unroll
        for (int bb = 0; bb < 4; bb++) {
          const uint4 w4 = *reinterpret_cast<const uint4*>(&sW[4 * bg + bb][4 * c]);
#pragma unroll
          for (int jj = 0; jj < JC; jj++) {
            acc[bb][jj] += (uint64_t)r[jj] * w4.x;
            acc[bb][jj] += (uint64_t)r[jj + 1] * w4.y;
            acc[bb][jj] += (uint64_t)r[jj + 2] * w4.z;
            acc[bb][jj] += (uint64_t)r[jj + 3] * w4.w;
          }
        }
        left -= 4;
        if (left < 4) {
#pragma unroll
          for (int bb = 0; bb < 4; bb++)
#pragma unroll
            for (int jj = 0; jj < JC; jj++)
              acc[bb][jj] = bgv_red(acc[bb][jj], p, mu);
          left = limit;
        }
      }
    }
    const uint32_t i = i0 + si;
#pragma unroll
    for (int bb = 0; bb < 4; bb++) {
      const uint32_t b = b0 + 4 * bg + bb;
      if (b >= (uint32_t)batch || i >= nslots)
        continue;
#pragma unroll
      for (int jj = 0; jj < JC; jj++)
        if (j0 + jj < d)
          u[((size_t)b * nslots + i) * d + j0 + jj] = (int64_t)bgv_red(acc[bb][jj], p, mu);
    }
  }
}

}  // namespace hx

struct hx_bgv_gf : hxb::SlotBase {
  uint64_t prime = 0;          // p; SlotBase's p is the modulus p^r the maps work in
  uint32_t r = 1;
  uint32_t d = 0, nslots = 0, ld = 0, ldr = 0, limit = 0;
  std::vector<uint64_t> gens;
  std::vector<int64_t> ords;   // signed
  std::vector<uint32_t> G;     // d + 1 words
  uint32_t* d_E = nullptr;
  uint32_t* d_Rx = nullptr;
  uint32_t* d_A = nullptr;
  uint32_t* d_M = nullptr;
  uint32_t* d_T = nullptr;
  // grow-only scratch beside SlotBase's: the CRT components c / the d constant terms u, the sliding window W
  void* xbuf[2] = {nullptr, nullptr};
  size_t xcap[2] = {0, 0};
};

using namespace hxb;

namespace {

int ensure_xbuf(hx_bgv_gf* t, hipStream_t st, int slot, size_t bytes)
{
  if (t->xcap[slot] >= bytes)
    return HX_OK;
  CK(hipStreamSynchronize(st));
  hipFree(t->xbuf[slot]);
  t->xbuf[slot] = nullptr;
  t->xcap[slot] = 0;
  CK(hipMalloc(&t->xbuf[slot], bytes));
  t->xcap[slot] = bytes;
  return HX_OK;
}

unsigned tiles_for(size_t a, size_t b)
{
  return (unsigned)std::min<size_t>(std::max<size_t>(a * b, 1), hx::BGV_MAX_BLOCKS);
}
size_t batch_tiles(int batch) { return ((size_t)batch + hx::GF_TB - 1) / hx::GF_TB; }
uint64_t mu_of(uint64_t p) { return (uint64_t)(((hxh::u128)1 << 64) / p); }

// w (batch x phi(m) words < p on the device) -> slots -> host
int decode_out(hx_bgv_gf* t, hipStream_t st, const uint64_t* w, int batch, int64_t* slots_out)
{
  const size_t total = (size_t)batch * t->nslots * t->d, bytes = total * 8;
  RC(ensure_xbuf(t, st, 0, bytes));
  RC(ensure_buf(t, st, 2, bytes));
  const uint64_t p = t->p, mu = mu_of(p);
  const size_t itiles = (t->nslots + hx::GF_DI - 1) / hx::GF_DI;
  int64_t* u = (int64_t*)t->xbuf[0];
#define GF_DECODE(JC)                                                                                                       \
  HX_LAUNCH(hx::bgv_gf_decode_kernel<JC>, dim3(tiles_for(itiles * ((t->d + JC - 1) / JC), batch_tiles(batch))), dim3(256), 0, st, w, \
            t->d_Rx, t->nslots, t->N, t->ldr, t->d, batch, p, mu, t->limit, (int)aligned16(w), u)
  if (t->d == 1)
    GF_DECODE(1);
  else if (t->d <= 4)
    GF_DECODE(4);
  else
    GF_DECODE(8);
#undef GF_DECODE
  CK(hipGetLastError());
  HX_LAUNCH(hx::bgv_gf_map_kernel<int64_t>, dim3(blocks_for(total)), dim3(256), 0, st, (const int64_t*)u, t->d_M, t->nslots, t->d,
            total, p, mu, t->limit, (int64_t*)t->buf[2]);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(slots_out, t->buf[2], bytes, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return HX_OK;
}

}  // namespace

extern "C" int hx_bgv_gf_destroy(hx_bgv_gf* t)
{
  if (!t)
    return HX_OK;
  (void)hipSetDevice(t->device);
  (void)hipDeviceSynchronize();
  for (uint32_t* tab : {t->d_E, t->d_Rx, t->d_A, t->d_M, t->d_T})
    hipFree(tab);
  for (void* b : t->buf)
    hipFree(b);
  for (void* b : t->xbuf)
    hipFree(b);
  delete t;
  return HX_OK;
}

// hx_bgv_gf_create_pr and hx_bgv_gf_create_gens: ngens = 0 is the hypercube of find_generators
static int gf_create(hx_ctx* ctx, uint64_t p, int r, const uint64_t* gens, const int64_t* ords, int ngens, hx_bgv_gf** out)
{
  if (!ctx || !out || (ngens > 0 && (!gens || !ords)))
    return err(HX_ERR_INVALID, "null argument");
  *out = nullptr;
  if (ngens < 0 || ngens > (int)hxc::CRT_MAX_GENS)
    return err(HX_ERR_INVALID, "%d generators: between 0 and %d are taken", ngens, (int)hxc::CRT_MAX_GENS);
  hxi::CtxView v{};
  RC(hxi::ctx_enter(ctx, &v));
  std::unique_lock<std::recursive_mutex> lk(*v.mu);
  if (v.capturing)
    return err(HX_ERR_INVALID, "hx_bgv_gf_create while a graph is being captured");
  const uint64_t m = v.m;
  if (p < 2 || !hxh::is_prime(p))
    return err(HX_ERR_INVALID, "the plaintext modulus p = %llu is not a prime", (unsigned long long)p);
  if (r < 1)
    return err(HX_ERR_INVALID, "the exponent r = %d of the plaintext space p^r is less than 1", r);
  if (p >= hxc::CRT_MAX_P)
    return err(HX_ERR_UNSUPPORTED, "p = %llu: the CRT tables hold 32-bit words and take p < 2^31 = %llu", (unsigned long long)p,
               (unsigned long long)hxc::CRT_MAX_P);
  const uint64_t P = hxc::crt_modulus(p, (uint32_t)r);
  if (!P)
    return err(HX_ERR_UNSUPPORTED, "p^r = %llu^%d: the CRT tables hold 32-bit words and take p^r < 2^31 = %llu",
               (unsigned long long)p, r, (unsigned long long)hxc::CRT_MAX_P);
  if (m % p == 0)
    return err(HX_ERR_INVALID, "p = %llu divides m = %llu", (unsigned long long)p, (unsigned long long)m);
  if (m < 3 || v.phim % 2 != 0)
    return err(HX_ERR_UNSUPPORTED, "BGV slots need m >= 3 (m = %llu)", (unsigned long long)m);
  hxc::GfTables tab;
  const std::vector<uint64_t> sg(gens, gens + (ngens > 0 ? ngens : 0));
  const std::vector<int64_t> so(ords, ords + (ngens > 0 ? ngens : 0));
  const std::string why = ngens > 0 ? hxc::build_gf(m, p, tab, (uint32_t)r, &sg, &so) : hxc::build_gf(m, p, tab, (uint32_t)r);
  if (!why.empty())
    return err(why.rfind("internal", 0) == 0 ? HX_ERR_DEVICE : why.rfind("generators:", 0) == 0 ? HX_ERR_INVALID : HX_ERR_UNSUPPORTED,
               "%s", why.c_str());
  const hxc::CrtTables& c = tab.crt;
  if (c.phim != v.phim)
    return err(HX_ERR_DEVICE, "internal: phi(m) = %u, the context says %u", c.phim, v.phim);
  hx_bgv_gf* t = new hx_bgv_gf();
  struct Guard {
    hx_bgv_gf* t;
    ~Guard() { hx_bgv_gf_destroy(t); }
  } guard{t};
  t->ctx = ctx;
  t->m = m;
  t->p = P;
  t->prime = p;
  t->r = (uint32_t)r;
  t->N = v.phim;
  t->device = v.device;
  t->d = c.d;
  if (c.limit < 1)
    return err(HX_ERR_DEVICE, "internal: no multiply-add fits a 64-bit accumulator modulo %llu", (unsigned long long)P);
  t->nslots = c.nslots;
  t->ld = c.ld;
  t->ldr = tab.ldr;
  t->limit = (uint32_t)c.limit;
  t->gens = c.gens;
  t->ords = c.ords;
  t->G = tab.G;
  const auto upload = [](uint32_t** dst, const std::vector<uint32_t>& src) -> hipError_t {
    if (src.empty())
      return hipSuccess;
    hipError_t e = hipMalloc((void**)dst, sizeof(uint32_t) * src.size());
    return e != hipSuccess ? e : hipMemcpy(*dst, src.data(), sizeof(uint32_t) * src.size(), hipMemcpyHostToDevice);
  };
  CK(upload(&t->d_E, c.E));
  CK(upload(&t->d_Rx, tab.Rx));
  CK(upload(&t->d_A, tab.A));
  {   // bgv_gf_map_kernel multiplies a row vector: alpha = M u goes up as u M^T
    const size_t dd = (size_t)c.d * c.d;
    std::vector<uint32_t> Mt(tab.M.size());
    for (size_t i = 0; i < c.nslots; i++)
      for (uint32_t l = 0; l < c.d; l++)
        for (uint32_t j = 0; j < c.d; j++)
          Mt[i * dd + (size_t)j * c.d + l] = tab.M[i * dd + (size_t)l * c.d + j];
    CK(upload(&t->d_M, Mt));
  }
  CK(upload(&t->d_T, tab.T));   // empty at d = 1
  guard.t = nullptr;
  *out = t;
  return HX_OK;
}

extern "C" int hx_bgv_gf_create_pr(hx_ctx* ctx, uint64_t p, int r, hx_bgv_gf** out) { return gf_create(ctx, p, r, nullptr, nullptr, 0, out); }
extern "C" int hx_bgv_gf_create(hx_ctx* ctx, uint64_t p, hx_bgv_gf** out) { return hx_bgv_gf_create_pr(ctx, p, 1, out); }
extern "C" int hx_bgv_gf_create_gens(hx_ctx* ctx, uint64_t p, int r, const uint64_t* gens, const int64_t* ords, int ngens,
                                     hx_bgv_gf** out)
{
  return gf_create(ctx, p, r, gens, ords, ngens, out);
}

extern "C" int hx_bgv_gf_space(const hx_bgv_gf* t, int* r, uint64_t* modulus)
{
  if (!t)
    return err(HX_ERR_INVALID, "null argument");
  if (r)
    *r = (int)t->r;
  if (modulus)
    *modulus = t->p;
  return HX_OK;
}

extern "C" int hx_bgv_gf_info(const hx_bgv_gf* t, uint64_t* p, int* d, int* nslots, int* ndims, uint64_t* gens, int64_t* ords,
                              uint64_t* table_bytes, uint64_t* G)
{
  if (!t)
    return err(HX_ERR_INVALID, "null argument");
  if (p)
    *p = t->prime;
  if (d)
    *d = (int)t->d;
  if (nslots)
    *nslots = (int)t->nslots;
  if (ndims)
    *ndims = (int)t->gens.size();
  for (size_t i = 0; i < t->gens.size() && i < 8; i++) {
    if (gens)
      gens[i] = t->gens[i];
    if (ords)
      ords[i] = t->ords[i];
  }
  if (table_bytes)
    *table_bytes = sizeof(uint32_t) * ((uint64_t)t->nslots * (t->ld + t->ldr + 2ull * t->d * t->d) + (uint64_t)(t->d - 1) * t->ld);
  if (G)
    for (uint32_t i = 0; i <= t->d; i++)
      G[i] = t->G[i];
  return HX_OK;
}

int hxg::gf_view(const hx_bgv_gf* t, GfView* v)
{
  if (!t || !v)
    return err(HX_ERR_INVALID, "null argument");
  *v = GfView{t->ctx, t->p, t->d, t->nslots, t->limit, t->d_A};
  return HX_OK;
}

int hxg::gf_encode_words(hx_bgv_gf* t, const char* what, int batch, uint64_t mul, hx_poly* out, int64_t* coeffs_out, const GfFill& fill)
{
  Encode e{t, out, batch};
  RC(e.check());
  uint64_t* h;
  RC(e.open(what, coeffs_out != nullptr, &h));
  const hipStream_t st = e.st;
  const uint64_t p = t->p, mu = mu_of(p);
  const uint32_t d = t->d, Nw = t->N + d - 1;
  const size_t total = (size_t)batch * t->nslots * d;
  RC(ensure_buf(t, st, 0, std::max<size_t>(total * 8, 16)));
  RC(ensure_xbuf(t, st, 0, std::max<size_t>(total * 8, 16)));   // (decode keeps 8-byte words there)
  uint64_t* W = h;   // d = 1: no top words, the window is H
  if (d > 1) {
    RC(ensure_xbuf(t, st, 1, (size_t)batch * Nw * 8));
    W = (uint64_t*)t->xbuf[1];
  }
  RC(fill(st, (uint32_t*)t->xbuf[0]));
  HX_LAUNCH(hx::bgv_gf_encode_kernel, dim3(tiles_for((Nw + hx::GF_EK - 1) / hx::GF_EK, batch_tiles(batch))), dim3(256), 0, st,
            (const uint32_t*)t->xbuf[0], t->d_E, t->nslots, d, Nw, t->ld, batch, p, mu, t->limit, W);
  CK(hipGetLastError());
  if (d > 1) {
    const size_t words = (size_t)batch * t->N;
    HX_LAUNCH(hx::bgv_gf_fold_kernel, dim3(blocks_for(words)), dim3(256), 0, st, (const uint64_t*)W, t->d_T, t->N, Nw, t->ld, d, words, p,
              mu, t->limit, h);
    CK(hipGetLastError());
  }
  return e.finish(mul % p, coeffs_out);
}

extern "C" int hx_bgv_gf_encode(const hx_bgv_gf* tc, const int64_t* slots, int batch, uint64_t mul, hx_poly* out, int64_t* coeffs_out)
{
  if (!tc || !out || !slots)
    return err(HX_ERR_INVALID, "null argument");
  hx_bgv_gf* t = const_cast<hx_bgv_gf*>(tc);   // (its scratch buffers grow; the caller's lock covers them)
  if (batch < 1)
    return err(HX_ERR_INVALID, "bad batch %d", batch);
  const size_t total = (size_t)batch * t->nslots * t->d;
  return hxg::gf_encode_words(t, "hx_bgv_gf_encode", batch, mul, out, coeffs_out, [&](hipStream_t st, uint32_t* c) -> int {
    CK(hipMemcpyAsync(t->buf[0], slots, total * 8, hipMemcpyHostToDevice, st));
    HX_LAUNCH(hx::bgv_gf_map_kernel<uint32_t>, dim3(blocks_for(total)), dim3(256), 0, st, (const int64_t*)t->buf[0], t->d_A, t->nslots,
              t->d, total, t->p, mu_of(t->p), t->limit, c);
    CK(hipGetLastError());
    return HX_OK;
  });
}

extern "C" int hx_bgv_gf_embed(const hx_bgv_gf* tc, const int64_t* coeffs, int batch, int64_t* slots_out)
{
  if (!tc || !coeffs || !slots_out)
    return err(HX_ERR_INVALID, "null argument");
  if (batch < 1)
    return err(HX_ERR_INVALID, "bad batch %d", batch);
  hx_bgv_gf* t = const_cast<hx_bgv_gf*>(tc);
  Enter E;
  RC(E.open(t, "hx_bgv_gf_embed"));
  const hipStream_t st = E.v.stream;
  DrainOnExit drain{st};
  const size_t words = (size_t)batch * t->N;
  RC(ensure_buf(t, st, 0, words * 8));
  RC(ensure_buf(t, st, 3, words * 8));
  CK(hipMemcpyAsync(t->buf[0], coeffs, words * 8, hipMemcpyHostToDevice, st));
  RC(launch_redmul(t, st, (const int64_t*)t->buf[0], words, 1 % t->p, (uint64_t*)t->buf[3]));
  return decode_out(t, st, (const uint64_t*)t->buf[3], batch, slots_out);
}

extern "C" int hx_bgv_gf_decode(const hx_bgv_gf* tc, const hx_poly* acc, uint64_t factor_inv, int64_t* slots_out)
{
  if (!tc || !acc || !slots_out)
    return err(HX_ERR_INVALID, "null argument");
  hx_bgv_gf* t = const_cast<hx_bgv_gf*>(tc);
  if (hxi::poly_ctx(acc) != t->ctx)
    return err(HX_ERR_INVALID, "the poly belongs to another context than the slot table");
  Enter E;
  RC(E.open(t, "hx_bgv_gf_decode"));
  int batch = 0, n = 0;
  RC(hx_poly_shape(acc, &batch, &n, nullptr));
  if (n == 0) {   // the zero polynomial
    memset(slots_out, 0, (size_t)batch * t->nslots * t->d * 8);
    return HX_OK;
  }
  const hipStream_t st = E.v.stream;
  DrainOnExit drain{st};
  const size_t words = (size_t)batch * t->N;
  const uint64_t* d_rem;
  RC(hxi::poly_rem_device(acc, t->p, &d_rem));   // toPoly + PolyRed(p), exact, in [0, p)
  RC(ensure_buf(t, st, 3, words * 8));
  RC(launch_redmul(t, st, (const int64_t*)d_rem, words, factor_inv % t->p, (uint64_t*)t->buf[3]));
  return decode_out(t, st, (const uint64_t*)t->buf[3], batch, slots_out);
}
