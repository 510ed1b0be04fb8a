// bgv_gf_linalg.hip -- the constants of linear maps on slots in GF(p^d) (include/helib_amd.h: hx_bgv_gf_linalg_tables,
// hx_bgv_gf_matrix_create, hx_bgv_gf_matrix_destroy, hx_bgv_gf_matrix_coeffs, hx_bgv_gf_gather): what
// BlockMatMul1D_derived_impl::processDiagonal1/2 (src/matmul.cpp:1329-1478), MatMul1D's processDiagonal with entries in
// GF(p^d) (:449-560) and the plaintext automorphisms of BlockMatMul1DExec_construct / MatMul1DExec_construct (:1537-1658,
// 626-688) compute on the host, polynomial by polynomial.  The tables are bgv_gf_linalg.h's.
//   bgv_gf_linpoly_kernel   C = E T mod p for every entry of a block matrix: [R, d^2] x [d^2, d^2], R = nb D D entries
//                           (buildLinPolyCoeffs per entry); R d^4 multiply-adds, once per matrix
//   bgv_gf_gather_kernel    per descriptor the slot array [nslots, d] of one constant: slot s takes coefficient k of the
//                           entry its source slot names on diagonal i (or the GF entry itself), pushed through Frob^e
//                           (d multiply-adds per word when e != 0), or zero where the map masks the slot
//   bgv_gf_gather_map_kernel  the gather, the Frobenius and the per-slot map A of an encode in one pass: per descriptor
//                           the CRT components c[nslots d] that bgv_gf_encode_kernel reads, formed on the device
//                           (hx_bgv_gf_encode_gathered); the thread-to-work map is gather_map.h's
// Over a table of hx_bgv_gf_create_pr (hx_bgv_gr_matrix_create, hx_bgv_gr_linalg_tables) the modulus of all of them is
// P = p^r and the tables are build_gr_linalg's; the kernels take the modulus as an argument and need no prime.
// modulo p on the vector ALU as bgv_gf.hip: 32-bit operands, 64-bit accumulators reduced once every `limit` =
// floor(2^64 / p^2) multiply-adds of ONE accumulator.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "bgv_gf_linalg.h"
#include "bgv_encode.h"
#include "bgv_gf_tail.h"
#include "gather_map.h"

namespace hx {

constexpr int LP_TM = 64;    // entries (rows of E) of a tile
constexpr int LP_TN = 64;    // columns of T of a tile
constexpr int LP_TK = 16;    // terms staged per step
constexpr int LP_LD = 68;    // words between LDS rows: 16-byte aligned, and bank (4 k + row) mod 64 differs over a staged store

// C[r][c] = sum_t E[r][t] T[t][c] mod p, E: [R][W] words < p, T: [W][W] words < p, W = d^2.  A workgroup takes tiles of 64
// entries x 64 columns; thread (tx, ty) = (tid & 15, tid >> 4) holds rows 4 ty .. 4 ty + 3 at columns 4 tx .. 4 tx + 3.  Per
// step 16 terms go through the LDS, E transposed ([term][row]) so that both operands are read as one 16-byte word per
// term: the 16 tx of a lane group read 64 consecutive words of T's row (every bank once), the ty broadcast.  LDS
// 2 x 16 x 68 x 4 = 8704 B.  Algorithmic bytes: 4 R W (W / 64) + 4 W W (R / 64) read, 4 R W written.
__global__ void __launch_bounds__(256)
bgv_gf_linpoly_kernel(const uint32_t* __restrict__ E, const uint32_t* __restrict__ T, uint32_t R, uint32_t W, uint64_t p, uint64_t mu,
                      uint32_t limit, uint32_t* __restrict__ C)
{
  __shared__ __attribute__((aligned(16))) uint32_t sE[LP_TK][LP_LD];
  __shared__ __attribute__((aligned(16))) uint32_t sT[LP_TK][LP_LD];
  const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const uint32_t rtiles = (R + LP_TM - 1) / LP_TM, ctiles = (W + LP_TN - 1) / LP_TN;
  for (uint32_t tile = blockIdx.x; tile < rtiles * ctiles; tile += gridDim.x) {
    const uint32_t r0 = (tile / ctiles) * LP_TM, c0 = (tile % ctiles) * LP_TN;
    uint64_t acc[4][4] = {};
    uint32_t left = limit;
    for (uint32_t t0 = 0; t0 < W; t0 += LP_TK) {
      __syncthreads();   // the previous step's readers are done
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t idx = tid + 256 * q;
        {   // E: 16 consecutive terms of a row per 16 lanes
          const uint32_t row = idx >> 4, k = idx & 15, r = r0 + row, t = t0 + k;
          sE[k][row] = (r < R && t < W) ? E[(size_t)r * W + t] : 0u;
        }
        {   // T: 64 consecutive columns of a row per wave
          const uint32_t k = idx >> 6, col = idx & 63, t = t0 + k, c = c0 + col;
          sT[k][col] = (t < W && c < W) ? T[(size_t)t * W + c] : 0u;
        }
      }
      __syncthreads();
#pragma unroll 4
      for (int k = 0; k < LP_TK; k++) {
        const uint4 e4 = *reinterpret_cast<const uint4*>(&sE[k][4 * ty]);
        const uint4 t4 = *reinterpret_cast<const uint4*>(&sT[k][4 * tx]);
        const uint32_t ev[4] = {e4.x, e4.y, e4.z, e4.w}, tv[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
          for (int b = 0; b < 4; b++)
            acc[a][b] += (uint64_t)ev[a] * tv[b];
        if (--left == 0) {   // (uniform) one more term could pass 2^64
#pragma unroll
          for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++)
              acc[a][b] = bgv_red(acc[a][b], p, mu);
          left = limit;
        }
      }
    }
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const uint32_t r = r0 + 4 * ty + a;
      if (r >= R)
        continue;
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const uint32_t c = c0 + 4 * tx + b;
        if (c < W)
          C[(size_t)r * W + c] = (uint32_t)bgv_red(acc[a][b], p, mu);
      }
    }
  }
}

struct GfDesc {   // hx_bgv_gf_desc, checked on the host
  int32_t diag, k, map;
};

// out[q][s][c] for descriptor q: with (src, e) = maps[desc.map][s], zero when src < 0, else the value of the source
// slot -- words [d] at val + (((blk[src] D + (col[src] - diag) mod D) D + col[src]) stride + k d) -- pushed through
// Frob^e: sum_l v[l] frob[e][l][c] mod p (e = 0: the words themselves).  stride = d^2 and k the coefficient index for a
// block matrix, stride = d and k = 0 for GF entries.  One thread per output word; nz[q] is set when any word of q is not
// zero.  Reads 8 B of map and <= 4 d B of value + 4 d B of frob per word, writes 8 B per word.
__global__ void __launch_bounds__(256)
bgv_gf_gather_kernel(const uint32_t* __restrict__ val, const int32_t* __restrict__ blk, const int32_t* __restrict__ col,
                     const GfDesc* __restrict__ descs, const int32_t* __restrict__ maps, const uint32_t* __restrict__ frob, uint32_t nslots,
                     uint32_t d, uint32_t D, uint32_t stride, size_t total, uint64_t p, uint64_t mu, uint32_t limit,
                     int64_t* __restrict__ out, uint32_t* __restrict__ nz)
{
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += step) {
    const size_t qs = idx / d;
    const uint32_t c = (uint32_t)(idx - qs * d), s = (uint32_t)(qs % nslots), q = (uint32_t)(qs / nslots);
    const GfDesc ds = descs[q];
    const int32_t* mp = maps + ((size_t)ds.map * nslots + s) * 2;
    const int32_t src = mp[0];
    uint64_t w = 0;
    if (src >= 0) {
      const uint32_t e = (uint32_t)mp[1], cc = (uint32_t)col[src];
      const uint32_t row = cc >= (uint32_t)ds.diag ? cc - (uint32_t)ds.diag : cc + D - (uint32_t)ds.diag;
      const uint32_t* v = val + (((size_t)blk[src] * D + row) * D + cc) * stride + (size_t)ds.k * d;
      if (e == 0) {
        w = v[c];
      } else {
        const uint32_t* f = frob + (size_t)e * d * d + c;
        uint64_t acc = 0;
        uint32_t left = limit;
        for (uint32_t l = 0; l < d; l++) {
          acc += (uint64_t)v[l] * f[(size_t)l * d];
          if (--left == 0) {
            acc = bgv_red(acc, p, mu);
            left = limit;
          }
        }
        w = bgv_red(acc, p, mu);
      }
    }
    out[idx] = (int64_t)w;
    if (w && __atomic_load_n(nz + q, __ATOMIC_RELAXED) == 0)
      atomicOr(nz + q, 1u);
  }
}

// c[q][s d + j] for descriptor q and slot s (one unit; gather_map.h maps threads to units): with (src, e) =
// maps[desc.map][s], v = the d words the source slot names (as bgv_gf_gather_kernel) or zero when src < 0,
// w = v frob[e] (sigma^e), c = w A_s (the CRT component of the slot, bgv_gf_map_kernel's product) -- no intermediate
// array in memory.  A group of dp lanes holds the unit: lane j loads v[j] (coalesced), forms w[j], then c[j]; operand l
// of either product comes from lane l of the group by a width-dp shuffle, so there is no LDS and no barrier, and every
// lane of a wave runs every pass (a lane without work carries zeros).  Table words frob[e][l][j] and A[s][l][j] are
// 4-byte loads that run along j across the lanes; both tables are shared by all descriptors.  c = nullptr: flags only
// (frob[e] and A_s are invertible, so c != 0 exactly when v != 0) and no table is read.  nz[q] is set by the first lane
// of a wave that holds a non-zero word of q: one atomic per wave and descriptor present in it, none once the flag is up.
// Reads 12 B of descriptor + 8 B of map + 8 B of geometry per unit, 4 d B of value and 4 d^2 B of A (+ 4 d^2 B of frob
// when e != 0, L2 resident) per unit; writes 4 d B per unit.
__global__ void __launch_bounds__(256)
bgv_gf_gather_map_kernel(const uint32_t* __restrict__ val, const int32_t* __restrict__ blk, const int32_t* __restrict__ col,
                         const GfDesc* __restrict__ descs, const int32_t* __restrict__ maps, const uint32_t* __restrict__ frob,
                         const uint32_t* __restrict__ A, uint32_t nslots, uint32_t d, uint32_t dp, uint32_t D, uint32_t stride,
                         unsigned long long units, uint32_t passes, uint64_t p, uint64_t mu, uint32_t limit, uint32_t* __restrict__ c,
                         uint32_t* __restrict__ nz)
{
  const uint32_t lane = threadIdx.x & 63u;
  const size_t dd = (size_t)d * d;
  for (uint32_t pass = 0; pass < passes; pass++) {   // the same trips for every thread: the shuffles need whole groups
    const GmWork wk = gm_work(blockIdx.x, threadIdx.x, gridDim.x, pass, units, d, dp);
    const uint32_t j = wk.j;
    uint32_t v = 0, e = 0, s = 0, q = 0;
    if (wk.unit < units) {
      q = (uint32_t)(wk.unit / nslots);
      s = (uint32_t)(wk.unit - (unsigned long long)q * nslots);
      const GfDesc ds = descs[q];
      const int32_t* mp = maps + ((size_t)ds.map * nslots + s) * 2;
      const int32_t src = mp[0];
      if (src >= 0) {
        e = (uint32_t)mp[1];
        const uint32_t cc = (uint32_t)col[src];
        const uint32_t row = cc >= (uint32_t)ds.diag ? cc - (uint32_t)ds.diag : cc + D - (uint32_t)ds.diag;
        if (j < d)
          v = val[(((size_t)blk[src] * D + row) * D + cc) * stride + (size_t)ds.k * d + j];
      }
    }
    {   // flags: the lanes of one descriptor are consecutive in a wave
      const unsigned long long hot = __ballot(v != 0);
      if (v != 0) {
        const unsigned long long unit0 = wk.unit - (lane / dp);   // the unit of the wave's lane 0
        const unsigned long long first = (unsigned long long)q * nslots;
        const uint32_t lane0 = first > unit0 ? (uint32_t)(first - unit0) * dp : 0u;   // the first lane of q in this wave
        const unsigned long long below = hot & ((1ull << lane) - 1ull) & ~((1ull << lane0) - 1ull);
        if (below == 0 && __atomic_load_n(nz + q, __ATOMIC_RELAXED) == 0)
          atomicOr(nz + q, 1u);
      }
      if (!c || hot == 0) {   // (wave-uniform) nothing to write but zeros
        if (c && wk.owns)
          c[wk.unit * d + j] = 0u;
        continue;
      }
    }
    uint32_t w = v;
    if (__ballot(e != 0) != 0) {   // (wave-uniform) some unit of the wave is twisted: w = v frob[e], frob[0] the identity
      const uint32_t* f = frob + (size_t)e * dd + j;
      const bool load = e != 0 && j < d;
      uint64_t acc = 0;
      uint32_t left = limit;
      for (uint32_t l = 0; l < d; l++) {
        const uint32_t vl = (uint32_t)__shfl((int)v, (int)l, (int)dp);
        const uint32_t fw = load ? f[(size_t)l * d] : (l == j ? 1u : 0u);
        acc += (uint64_t)vl * fw;
        if (--left == 0) {   // (uniform) one more term could pass 2^64
          acc = bgv_red(acc, p, mu);
          left = limit;
        }
      }
      w = (uint32_t)bgv_red(acc, p, mu);
    }
    {
      const uint32_t* a = A + (size_t)s * dd + j;
      uint64_t acc = 0;
      uint32_t left = limit;
      for (uint32_t l = 0; l < d; l++) {
        const uint32_t wl = (uint32_t)__shfl((int)w, (int)l, (int)dp);
        const uint32_t aw = wk.owns ? a[(size_t)l * d] : 0u;
        acc += (uint64_t)wl * aw;
        if (--left == 0) {
          acc = bgv_red(acc, p, mu);
          left = limit;
        }
      }
      if (wk.owns)
        c[wk.unit * d + j] = (uint32_t)bgv_red(acc, p, mu);
    }
  }
}

}  // namespace hx

struct hx_bgv_gf_matrix {
  hx_ctx* ctx = nullptr;
  int device = 0;
  uint64_t p = 0;
  uint32_t d = 0, nslots = 0, D = 0, nb = 0, stride = 0, limit = 0;
  bool block = false;
  uint32_t* d_val = nullptr;    // block: the linearized-polynomial coefficients [nb D D][d][d]; GF: the entries [nb D D][d]
  uint32_t* d_frob = nullptr;   // [d][d][d]
  int32_t* d_blk = nullptr;     // [nslots] each
  int32_t* d_col = nullptr;
  void* buf[3] = {nullptr, nullptr, nullptr};   // grow-only: descriptors + maps, slot arrays, flags
  size_t cap[3] = {0, 0, 0};
};

using namespace hxb;

namespace {

int ensure(hx_bgv_gf_matrix* a, hipStream_t st, int slot, size_t bytes)
{
  if (a->cap[slot] >= bytes)
    return HX_OK;
  CK(hipStreamSynchronize(st));
  hipFree(a->buf[slot]);
  a->buf[slot] = nullptr;
  a->cap[slot] = 0;
  CK(hipMalloc(&a->buf[slot], bytes));
  a->cap[slot] = bytes;
  return HX_OK;
}

// p: the prime; r (null: a table with r > 1 is refused) and the words of G modulo p^r
int gf_geometry(const hx_bgv_gf* t, uint64_t* p, int* d, int* n, std::vector<uint32_t>& G, int* rout = nullptr)
{
  int r = 1;
  RC(hx_bgv_gf_space(t, &r, nullptr));
  if (r != 1 && !rout)
    return err(HX_ERR_UNSUPPORTED, "matrices over Galois-ring slots at p^r with r > 1 are not built (r = %d)", r);
  if (rout)
    *rout = r;
  RC(hx_bgv_gf_info(t, p, d, n, nullptr, nullptr, nullptr, nullptr, nullptr));
  std::vector<uint64_t> g((size_t)*d + 1);
  RC(hx_bgv_gf_info(t, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, g.data()));
  G.assign(g.begin(), g.end());
  return HX_OK;
}

}  // namespace

extern "C" int hx_bgv_gf_linalg_tables(uint64_t p, int d, const uint64_t* G, uint32_t* frob_out, uint32_t* K_out, uint32_t* T_out)
{
  if (!G)
    return err(HX_ERR_INVALID, "null argument");
  if (d < 1 || d > (int)hxc::GF_MAX_D || p < 2 || p >= hxc::CRT_MAX_P)
    return err(HX_ERR_UNSUPPORTED, "linear maps on GF(p^d) slots are built for d <= %u and p < 2^31 (d = %d, p = %llu)", hxc::GF_MAX_D, d,
               (unsigned long long)p);
  std::vector<uint32_t> g((size_t)d + 1);
  for (int i = 0; i <= d; i++)
    g[i] = (uint32_t)(G[i] % p);
  hxc::GfLinTables tab;
  const std::string why = hxc::build_gf_linalg(g.data(), (uint32_t)d, p, tab);
  if (!why.empty())
    return err(why.rfind("internal", 0) == 0 ? HX_ERR_DEVICE : HX_ERR_UNSUPPORTED, "%s", why.c_str());
  if (frob_out)
    memcpy(frob_out, tab.frob.data(), tab.frob.size() * 4);
  if (K_out)
    memcpy(K_out, tab.K.data(), tab.K.size() * 4);
  if (T_out)
    memcpy(T_out, tab.T.data(), tab.T.size() * 4);
  return HX_OK;
}

extern "C" int hx_bgv_gr_linalg_tables(uint64_t p, int r, int d, const uint64_t* G, uint32_t* frob_out, uint32_t* K_out, uint32_t* T_out)
{
  if (!G)
    return err(HX_ERR_INVALID, "null argument");
  if (r < 1)
    return err(HX_ERR_INVALID, "the exponent r = %d of the plaintext space p^r is less than 1", r);
  const uint64_t P = hxc::crt_modulus(p, (uint32_t)r);
  if (d < 1 || d > (int)hxc::GF_MAX_D || !P)
    return err(HX_ERR_UNSUPPORTED, "linear maps on Galois-ring slots are built for d <= %u and p^r < 2^31 (d = %d, p^r = %llu^%d)",
               hxc::GF_MAX_D, d, (unsigned long long)p, r);
  std::vector<uint32_t> g((size_t)d + 1);
  for (int i = 0; i <= d; i++)
    g[i] = (uint32_t)(G[i] % P);
  hxc::GfLinTables tab;
  const std::string why = hxc::build_gr_linalg(g.data(), (uint32_t)d, p, (uint32_t)r, tab);
  if (!why.empty())
    return err(why.rfind("internal", 0) == 0 ? HX_ERR_DEVICE : HX_ERR_UNSUPPORTED, "%s", why.c_str());
  if (frob_out)
    memcpy(frob_out, tab.frob.data(), tab.frob.size() * 4);
  if (K_out)
    memcpy(K_out, tab.K.data(), tab.K.size() * 4);
  if (T_out)
    memcpy(T_out, tab.T.data(), tab.T.size() * 4);
  return HX_OK;
}

extern "C" int hx_bgv_gf_matrix_destroy(hx_bgv_gf_matrix* a)
{
  if (!a)
    return HX_OK;
  (void)hipSetDevice(a->device);
  (void)hipDeviceSynchronize();
  hipFree(a->d_val);
  hipFree(a->d_frob);
  hipFree(a->d_blk);
  hipFree(a->d_col);
  for (void* b : a->buf)
    hipFree(b);
  delete a;
  return HX_OK;
}

namespace {

// hx_bgv_gf_matrix_create (any_r = false: a table with r > 1 is refused) and hx_bgv_gr_matrix_create
int matrix_create(const char* what, bool any_r, hx_ctx* ctx, const hx_bgv_gf* t, int block, int nb, int D, const uint32_t* words,
                  const int32_t* blk, const int32_t* col, hx_bgv_gf_matrix** out)
{
  if (!ctx || !t || !words || !blk || !col || !out)
    return err(HX_ERR_INVALID, "null argument");
  *out = nullptr;
  uint64_t prime = 0, p = 0;
  int d = 0, n = 0, r = 1;
  std::vector<uint32_t> G;
  RC(gf_geometry(t, &prime, &d, &n, G, any_r ? &r : nullptr));
  RC(hx_bgv_gf_space(t, nullptr, &p));   // the modulus of the words: p^r
  if (nb < 1 || D < 1 || (uint64_t)nb * D > (uint64_t)n)
    return err(HX_ERR_INVALID, "nb = %d blocks of a %d x %d matrix over %d slots", nb, D, D, n);
  for (int s = 0; s < n; s++)
    if (blk[s] < 0 || blk[s] >= nb || col[s] < 0 || col[s] >= D)
      return err(HX_ERR_INVALID, "slot %d: block %d / column %d outside [0, %d) x [0, %d)", s, blk[s], col[s], nb, D);
  const size_t dd = (size_t)d * d, R = (size_t)nb * D * D, per = block ? dd : (size_t)d;
  if (R > 0xffffffffu / 2 || R * per > ((size_t)1 << 31))
    return err(HX_ERR_UNSUPPORTED, "a matrix of %zu entries of %zu words is larger than 2^31 words", R, per);
  for (size_t i = 0; i < R * per; i++)
    if (words[i] >= p)
      return err(HX_ERR_INVALID, "word %zu = %u of the matrix is not below p = %llu", i, words[i], (unsigned long long)p);
  hxc::GfLinTables tab;
  const std::string why = hxc::build_gr_linalg(G.data(), (uint32_t)d, prime, (uint32_t)r, tab);
  if (!why.empty())
    return err(why.rfind("internal", 0) == 0 ? HX_ERR_DEVICE : HX_ERR_UNSUPPORTED, "%s", why.c_str());
  hxi::CtxView v{};
  RC(hxi::ctx_enter(ctx, &v));
  std::unique_lock<std::recursive_mutex> lk(*v.mu);
  if (v.capturing)
    return err(HX_ERR_INVALID, "%s while a graph is being captured", what);
  const hipStream_t st = v.stream;
  hx_bgv_gf_matrix* a = new hx_bgv_gf_matrix();
  struct Guard {
    hx_bgv_gf_matrix* a;
    ~Guard() { hx_bgv_gf_matrix_destroy(a); }
  } guard{a};
  a->ctx = ctx;
  a->device = v.device;
  a->p = p;
  a->d = (uint32_t)d;
  a->nslots = (uint32_t)n;
  a->D = (uint32_t)D;
  a->nb = (uint32_t)nb;
  a->block = block != 0;
  a->stride = (uint32_t)per;
  a->limit = (uint32_t)tab.limit;
  CK(hipMalloc((void**)&a->d_val, R * per * 4));
  CK(hipMalloc((void**)&a->d_frob, dd * d * 4));
  CK(hipMalloc((void**)&a->d_blk, (size_t)n * 4));
  CK(hipMalloc((void**)&a->d_col, (size_t)n * 4));
  CK(hipMemcpyAsync(a->d_frob, tab.frob.data(), dd * d * 4, hipMemcpyHostToDevice, st));
  CK(hipMemcpyAsync(a->d_blk, blk, (size_t)n * 4, hipMemcpyHostToDevice, st));
  CK(hipMemcpyAsync(a->d_col, col, (size_t)n * 4, hipMemcpyHostToDevice, st));
  if (!block) {
    CK(hipMemcpyAsync(a->d_val, words, R * per * 4, hipMemcpyHostToDevice, st));
    CK(hipStreamSynchronize(st));
  } else {
    uint32_t *d_E = nullptr, *d_T = nullptr;
    struct Tmp {
      uint32_t **e, **t;
      ~Tmp()
      {
        hipFree(*e);
        hipFree(*t);
      }
    } tmp{&d_E, &d_T};
    CK(hipMalloc((void**)&d_E, R * dd * 4));
    CK(hipMalloc((void**)&d_T, dd * dd * 4));
    CK(hipMemcpyAsync(d_E, words, R * dd * 4, hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(d_T, tab.T.data(), dd * dd * 4, hipMemcpyHostToDevice, st));
    const size_t tiles = ((R + hx::LP_TM - 1) / hx::LP_TM) * ((dd + hx::LP_TN - 1) / hx::LP_TN);
    HX_LAUNCH(hx::bgv_gf_linpoly_kernel, dim3((unsigned)std::min<size_t>(tiles, hx::BGV_MAX_BLOCKS)), dim3(256), 0, st,
              (const uint32_t*)d_E, (const uint32_t*)d_T, (uint32_t)R, (uint32_t)dd, p, (uint64_t)(((hxh::u128)1 << 64) / p), a->limit,
              a->d_val);
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st));
  }
  guard.a = nullptr;
  *out = a;
  return HX_OK;
}

}  // namespace

extern "C" int hx_bgv_gf_matrix_create(hx_ctx* ctx, const hx_bgv_gf* t, int block, int nb, int D, const uint32_t* words,
                                       const int32_t* blk, const int32_t* col, hx_bgv_gf_matrix** out)
{
  return matrix_create("hx_bgv_gf_matrix_create", false, ctx, t, block, nb, D, words, blk, col, out);
}

extern "C" int hx_bgv_gr_matrix_create(hx_ctx* ctx, const hx_bgv_gf* t, int block, int nb, int D, const uint32_t* words,
                                       const int32_t* blk, const int32_t* col, hx_bgv_gf_matrix** out)
{
  return matrix_create("hx_bgv_gr_matrix_create", true, ctx, t, block, nb, D, words, blk, col, out);
}

extern "C" int hx_bgv_gf_matrix_coeffs(const hx_bgv_gf_matrix* a, uint32_t* out)
{
  if (!a || !out)
    return err(HX_ERR_INVALID, "null argument");
  hxi::CtxView v{};
  RC(hxi::ctx_enter(a->ctx, &v));
  std::unique_lock<std::recursive_mutex> lk(*v.mu);
  if (v.capturing)
    return err(HX_ERR_INVALID, "hx_bgv_gf_matrix_coeffs waits for the device and cannot be captured in a graph");
  CK(hipMemcpyAsync(out, a->d_val, (size_t)a->nb * a->D * a->D * a->stride * 4, hipMemcpyDeviceToHost, v.stream));
  CK(hipStreamSynchronize(v.stream));
  return HX_OK;
}

namespace {

// the ranges of descriptors and maps, on the host
int check_descs(const hx_bgv_gf_matrix* a, const hx_bgv_gf_desc* descs, int ndesc, const int32_t* maps, int nmaps)
{
  static_assert(sizeof(hx_bgv_gf_desc) == sizeof(hx::GfDesc), "descriptor layout");
  if (ndesc < 1 || nmaps < 1)
    return err(HX_ERR_INVALID, "bad number of descriptors %d or maps %d", ndesc, nmaps);
  const uint32_t n = a->nslots, d = a->d;
  for (int q = 0; q < ndesc; q++) {
    const hx_bgv_gf_desc& x = descs[q];
    if (x.diag < 0 || (uint32_t)x.diag >= a->D || x.map < 0 || x.map >= nmaps || x.k < 0 || (uint32_t)x.k >= (a->block ? d : 1u))
      return err(HX_ERR_INVALID, "descriptor %d: diagonal %d, coefficient %d, map %d out of range", q, x.diag, x.k, x.map);
  }
  for (size_t i = 0; i < (size_t)nmaps * n; i++)
    if (maps[2 * i] < -1 || maps[2 * i] >= (int32_t)n || maps[2 * i + 1] < 0 || (uint32_t)maps[2 * i + 1] >= d)
      return err(HX_ERR_INVALID, "map word %zu: source slot %d, Frobenius exponent %d out of range", i, maps[2 * i], maps[2 * i + 1]);
  return HX_OK;
}

size_t desc_bytes(int ndesc) { return (sizeof(hx::GfDesc) * (size_t)ndesc + 15) / 16 * 16; }

// descriptors and maps into the matrix's scratch (buf[0]), the flags (buf[2]) cleared
int upload_descs(hx_bgv_gf_matrix* a, hipStream_t st, const hx_bgv_gf_desc* descs, int ndesc, const int32_t* maps, int nmaps)
{
  const size_t dbytes = desc_bytes(ndesc), mbytes = (size_t)nmaps * a->nslots * 8;
  RC(ensure(a, st, 0, dbytes + mbytes));
  RC(ensure(a, st, 2, (size_t)ndesc * 4));
  char* base = (char*)a->buf[0];
  CK(hipMemcpyAsync(base, descs, sizeof(hx::GfDesc) * (size_t)ndesc, hipMemcpyHostToDevice, st));
  CK(hipMemcpyAsync(base + dbytes, maps, mbytes, hipMemcpyHostToDevice, st));
  CK(hipMemsetAsync(a->buf[2], 0, (size_t)ndesc * 4, st));
  return HX_OK;
}

}  // namespace

extern "C" int hx_bgv_gf_gather(const hx_bgv_gf_matrix* ac, const hx_bgv_gf_desc* descs, int ndesc, const int32_t* maps, int nmaps,
                                int64_t* slots_out, int* nonzero_out)
{
  if (!ac || !descs || !maps || !slots_out || !nonzero_out)
    return err(HX_ERR_INVALID, "null argument");
  hx_bgv_gf_matrix* a = const_cast<hx_bgv_gf_matrix*>(ac);   // (its scratch buffers grow; the context's lock covers them)
  RC(check_descs(a, descs, ndesc, maps, nmaps));
  const uint32_t n = a->nslots, d = a->d;
  hxi::CtxView v{};
  RC(hxi::ctx_enter(a->ctx, &v));
  std::unique_lock<std::recursive_mutex> lk(*v.mu);
  if (v.capturing)
    return err(HX_ERR_INVALID, "hx_bgv_gf_gather waits for the device and cannot be captured in a graph");
  const hipStream_t st = v.stream;
  DrainOnExit drain{st};
  const size_t dbytes = desc_bytes(ndesc);
  const size_t total = (size_t)ndesc * n * d;
  RC(upload_descs(a, st, descs, ndesc, maps, nmaps));
  RC(ensure(a, st, 1, total * 8));
  char* base = (char*)a->buf[0];
  HX_LAUNCH(hx::bgv_gf_gather_kernel, dim3(blocks_for(total)), dim3(256), 0, st, (const uint32_t*)a->d_val, (const int32_t*)a->d_blk,
            (const int32_t*)a->d_col, (const hx::GfDesc*)base, (const int32_t*)(base + dbytes), (const uint32_t*)a->d_frob, n, d, a->D,
            a->stride, total, a->p, (uint64_t)(((hxh::u128)1 << 64) / a->p), a->limit, (int64_t*)a->buf[1], (uint32_t*)a->buf[2]);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(slots_out, a->buf[1], total * 8, hipMemcpyDeviceToHost, st));
  CK(hipMemcpyAsync(nonzero_out, a->buf[2], (size_t)ndesc * 4, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return HX_OK;
}

extern "C" int hx_bgv_gf_encode_gathered(const hx_bgv_gf* tc, const hx_bgv_gf_matrix* ac, const hx_bgv_gf_desc* descs, int ndesc,
                                         const int32_t* maps, int nmaps, uint64_t mul, hx_poly* out, int64_t* coeffs_out,
                                         int* nonzero_out)
{
  if (!tc || !ac || !descs || !maps || !nonzero_out || (!out && coeffs_out))
    return err(HX_ERR_INVALID, "null argument");
  hx_bgv_gf* t = const_cast<hx_bgv_gf*>(tc);
  hx_bgv_gf_matrix* a = const_cast<hx_bgv_gf_matrix*>(ac);   // (their scratch buffers grow; the context's lock covers them)
  hxg::GfView tv{};
  RC(hxg::gf_view(t, &tv));
  if (tv.ctx != a->ctx)
    return err(HX_ERR_INVALID, "the matrix belongs to another context than the slot table");
  if (tv.p != a->p || tv.d != a->d || tv.nslots != a->nslots)
    return err(HX_ERR_INVALID, "the matrix was built over another slot table (modulus %llu, d = %u, %u slots)", (unsigned long long)a->p,
               a->d, a->nslots);
  RC(check_descs(a, descs, ndesc, maps, nmaps));
  const uint32_t n = a->nslots, d = a->d, dp = hx::gm_group(d);
  const unsigned long long units = (unsigned long long)ndesc * n;
  const unsigned blocks = hx::gm_blocks(units, dp, hx::BGV_MAX_BLOCKS), passes = hx::gm_passes(units, dp, blocks);
  const auto fill = [&](hipStream_t st, uint32_t* c) -> int {
    RC(upload_descs(a, st, descs, ndesc, maps, nmaps));
    const char* base = (const char*)a->buf[0];
    HX_LAUNCH(hx::bgv_gf_gather_map_kernel, dim3(blocks), dim3(hx::GM_THREADS), 0, st, (const uint32_t*)a->d_val, (const int32_t*)a->d_blk,
              (const int32_t*)a->d_col, (const hx::GfDesc*)base, (const int32_t*)(base + desc_bytes(ndesc)), (const uint32_t*)a->d_frob,
              tv.d_A, n, d, dp, a->D, a->stride, units, passes, a->p, (uint64_t)(((hxh::u128)1 << 64) / a->p), a->limit, c,
              (uint32_t*)a->buf[2]);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(nonzero_out, a->buf[2], (size_t)ndesc * 4, hipMemcpyDeviceToHost, st));
    return HX_OK;
  };
  if (out)
    return hxg::gf_encode_words(t, "hx_bgv_gf_encode_gathered", ndesc, mul, out, coeffs_out, fill);
  // the flags alone: no row is written, no table read
  hxi::CtxView v{};
  RC(hxi::ctx_enter(a->ctx, &v));
  std::unique_lock<std::recursive_mutex> lk(*v.mu);
  if (v.capturing)
    return err(HX_ERR_INVALID, "hx_bgv_gf_encode_gathered waits for the device and cannot be captured in a graph");
  DrainOnExit drain{v.stream};
  RC(fill(v.stream, nullptr));
  CK(hipStreamSynchronize(v.stream));
  return HX_OK;
}
