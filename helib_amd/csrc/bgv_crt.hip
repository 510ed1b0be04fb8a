// bgv_crt.hip -- C ABI of BGV slot encoding and decoding for any d = ord_m(p), slots in Z_p or, Hensel-lifted, in
// Z_(p^r) (include/helib_amd.h: hx_bgv_crt_create, hx_bgv_crt_create_pr, hx_bgv_crt_encode, hx_bgv_crt_decode,
// hx_bgv_crt_embed): the default-constructed EncryptedArray
// (G = X) over PAlgebraMod (src/EncryptedArray.cpp, src/PAlgebra.cpp:680-772, 885-936, 1007-1045, 1243-1261).  For
// d > 1 the plaintext prime is no transform prime of the ring, so there is no transform to borrow as bgv_slots.hip
// does: the maps are two matrices modulo p built on the host (bgv_crt.h),
//   encode   H[b][k] = sum_i a[b][i] E[i][k] mod p     E_i the idempotent of factor i        (bgv_crt_encode_kernel)
//   decode   s[b][i] = sum_k w[b][k] R[i][k] mod p     R_i[k] = [X^0](X^k mod F_i)          (bgv_crt_decode_kernel)
// small-modulus matrix products on the vector ALU: 32-bit operands, 64-bit accumulators reduced once every `limit`
// terms (floor(2^64 / p^2), per table), operand tiles staged through the LDS, 16-byte accesses along the rows of E, R
// and the coefficients.  Around them the d = 1 path's own pieces (bgv_encode.h): bgv_lift_kernel and the engine's
// forward transforms behind an encode, hxi::poly_rem_device and bgv_redmul_kernel in front of a decode.
// At r > 1 the modulus of all of these is p^r < 2^31 (in the kernels' `p`; the table keeps the prime beside it).  None
// of them needs a prime: bgv_red's quotient estimate floor(x mu / 2^64), mu = floor(2^64 / q), is short by at most 1
// for any q >= 2, Shoup's product x w - floor(x ws / 2^64) q lies in [0, 2q) for any q and w < q, and the accumulators
// are bounded by `limit` = floor(2^64 / p^(2r)).  The one place that knows the parity is the lift's balancing, below.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "bgv_crt.h"
#include "bgv_encode.h"

namespace hx {

constexpr int CRT_TB = 16;    // batch elements of a tile (four per thread)
constexpr int CRT_EK = 256;   // encode: coefficients of a tile (64 lanes x 4)
constexpr int CRT_EI = 16;    // encode: slots staged per step
constexpr int CRT_DI = 64;    // decode: slots of a tile (one per lane)
constexpr int CRT_DK = 32;    // decode: coefficients staged per step
constexpr int CRT_DLD = 36;   // decode: words between LDS rows (16-byte aligned, rows spread over the banks)

// H[b][k] = sum_i (a[b][i] mod p) E[i][k] mod p.  a: [batch][nslots] signed words, E: [nslots][ld] words < p, ld a
// multiple of 4 with zeros behind N, H: [batch][N], N even.  A workgroup takes tiles of 16 elements x 256 coefficients;
// a thread holds 4 x 4 accumulators.  Per 16 slots: the 16 x 256 words of E (16-byte loads) and the 16 x 16 slots,
// reduced mod p, go through the LDS.  Algorithmic bytes: 4 nslots ld per 16 elements + 8 batch nslots read,
// 8 batch N written.
__global__ void __launch_bounds__(256)
bgv_crt_encode_kernel(const int64_t* __restrict__ a, const uint32_t* __restrict__ E, uint32_t nslots, uint32_t N, uint32_t ld,
                      int batch, uint64_t p, uint64_t mu, uint32_t limit, uint64_t* __restrict__ H)
{
  __shared__ uint4 sE[CRT_EI][CRT_EK / 4];
  __shared__ uint4 sA[CRT_EI][CRT_TB / 4];   // [slot][element]
  const uint32_t tid = threadIdx.x, cg = tid & 63, bg = tid >> 6;
  const uint32_t ktiles = (ld + CRT_EK - 1) / CRT_EK, btiles = ((uint32_t)batch + CRT_TB - 1) / CRT_TB;
  for (uint32_t tile = blockIdx.x; tile < ktiles * btiles; tile += gridDim.x) {
    const uint32_t k0 = (tile % ktiles) * CRT_EK, b0 = (tile / ktiles) * CRT_TB;
    uint64_t acc[4][4] = {};
    uint32_t left = limit;
    for (uint32_t i0 = 0; i0 < nslots; i0 += CRT_EI) {
      __syncthreads();   // the previous step's readers are done
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const uint32_t row = bg + 4 * r, i = i0 + row, k = k0 + 4 * cg;
        sE[row][cg] = (i < nslots && k < ld) ? *reinterpret_cast<const uint4*>(E + (size_t)i * ld + k) : make_uint4(0, 0, 0, 0);
      }
      {
        const uint32_t b = b0 + (tid >> 4), i = i0 + (tid & 15);
        reinterpret_cast<uint32_t*>(sA)[(tid & 15) * CRT_TB + (tid >> 4)] =
            (b < (uint32_t)batch && i < nslots) ? (uint32_t)bgv_red_signed(a[(size_t)b * nslots + i], p, mu) : 0u;
      }
      __syncthreads();
#pragma unroll
      for (int g = 0; g < CRT_EI / 4; g++) {
#pragma unroll
        for (int ii = 0; ii < 4; ii++) {
          const uint4 e = sE[g * 4 + ii][cg], av = sA[g * 4 + ii][bg];
          const uint32_t ev[4] = {e.x, e.y, e.z, e.w}, bv[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
          for (int bb = 0; bb < 4; bb++)
#pragma unroll
            for (int kk = 0; kk < 4; kk++)
              acc[bb][kk] += (uint64_t)bv[bb] * ev[kk];
        }
        left -= 4;
        if (left < 4) {   // (uniform) the next four terms could pass 2^64
#pragma unroll
          for (int bb = 0; bb < 4; bb++)
#pragma unroll
            for (int kk = 0; kk < 4; kk++)
              acc[bb][kk] = bgv_red(acc[bb][kk], p, mu);
          left = limit;
        }
      }
    }
    const uint32_t k = k0 + 4 * cg;
#pragma unroll
    for (int bb = 0; bb < 4; bb++) {
      const uint32_t b = b0 + 4 * bg + bb;
      if (b >= (uint32_t)batch)
        continue;
      uint64_t* dst = H + (size_t)b * N + k;   // N and k are even: 16-byte aligned pairs
      if (k < N)
        *reinterpret_cast<ulonglong2*>(dst) = make_ulonglong2(bgv_red(acc[bb][0], p, mu), bgv_red(acc[bb][1], p, mu));
      if (k + 2 < N)
        *reinterpret_cast<ulonglong2*>(dst + 2) = make_ulonglong2(bgv_red(acc[bb][2], p, mu), bgv_red(acc[bb][3], p, mu));
    }
  }
}

// s[b][i] = sum_k w[b][k] R[i][k] mod p.  w: [batch][N] words < p (N even; wvec: the buffer is 16-byte aligned),
// R: [nslots][ld] words < p, out: [batch][nslots].  A workgroup takes tiles of 16 elements x 64 slots; lane = slot, a
// thread holds 4 accumulators.  Per 32 coefficients: 64 x 32 words of R (16-byte loads) and 16 x 32 of w (16-byte
// loads, kept as 32-bit words) go through the LDS and are read back four coefficients at a time.  Algorithmic bytes:
// 4 nslots ld per 16 elements + 8 batch N per 64 slots read, 8 batch nslots written.
__global__ void __launch_bounds__(256)
bgv_crt_decode_kernel(const uint64_t* __restrict__ w, const uint32_t* __restrict__ R, uint32_t nslots, uint32_t N, uint32_t ld,
                      int batch, uint64_t p, uint64_t mu, uint32_t limit, int wvec, int64_t* __restrict__ out)
{
  __shared__ __attribute__((aligned(16))) uint32_t sR[CRT_DI][CRT_DLD];
  __shared__ __attribute__((aligned(16))) uint32_t sW[CRT_TB][CRT_DLD];
  const uint32_t tid = threadIdx.x, si = tid & 63, bg = tid >> 6;
  const uint32_t itiles = (nslots + CRT_DI - 1) / CRT_DI, btiles = ((uint32_t)batch + CRT_TB - 1) / CRT_TB;
  for (uint32_t tile = blockIdx.x; tile < itiles * btiles; tile += gridDim.x) {
    const uint32_t i0 = (tile % itiles) * CRT_DI, b0 = (tile / itiles) * CRT_TB;
    uint64_t acc[4] = {};
    uint32_t left = limit;
    for (uint32_t k0 = 0; k0 < N; k0 += CRT_DK) {
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 2; r++) {
        const uint32_t idx = tid + 256 * r, row = idx >> 3, c = idx & 7, i = i0 + row, k = k0 + 4 * c;
        *reinterpret_cast<uint4*>(&sR[row][4 * c]) =
            (i < nslots && k < ld) ? *reinterpret_cast<const uint4*>(R + (size_t)i * ld + k) : make_uint4(0, 0, 0, 0);
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
#pragma unroll
      for (int c = 0; c < CRT_DK / 4; c++) {
        const uint4 r4 = *reinterpret_cast<const uint4*>(&sR[si][4 * c]);
#pragma unroll
        for (int bb = 0; bb < 4; bb++) {
          const uint4 w4 = *reinterpret_cast<const uint4*>(&sW[4 * bg + bb][4 * c]);
          acc[bb] += (uint64_t)r4.x * w4.x;
          acc[bb] += (uint64_t)r4.y * w4.y;
          acc[bb] += (uint64_t)r4.z * w4.z;
          acc[bb] += (uint64_t)r4.w * w4.w;
        }
        left -= 4;
        if (left < 4) {
#pragma unroll
          for (int bb = 0; bb < 4; bb++)
            acc[bb] = bgv_red(acc[bb], p, mu);
          left = limit;
        }
      }
    }
    const uint32_t i = i0 + si;
#pragma unroll
    for (int bb = 0; bb < 4; bb++) {
      const uint32_t b = b0 + 4 * bg + bb;
      if (b < (uint32_t)batch && i < nslots)
        out[(size_t)b * nslots + i] = (int64_t)bgv_red(acc[bb], p, mu);
    }
  }
}

}  // namespace hx

struct hx_bgv_crt : hxb::SlotBase {   // SlotBase::p is the modulus p^r of the maps
  uint64_t prime = 0;
  uint32_t r = 1;
  uint32_t d = 0, nslots = 0, ld = 0, limit = 0;
  std::vector<uint64_t> gens;
  std::vector<int64_t> ords;   // signed
  uint32_t* d_E = nullptr;
  uint32_t* d_R = nullptr;
};

using namespace hxb;

namespace {

unsigned tiles_for(uint32_t cols, uint32_t per, int batch)
{
  const size_t t = (size_t)((cols + per - 1) / per) * (((size_t)batch + hx::CRT_TB - 1) / hx::CRT_TB);
  return (unsigned)std::min<size_t>(std::max<size_t>(t, 1), hx::BGV_MAX_BLOCKS);
}

// w (batch x phi(m) words < p on the device) -> slots -> host
int decode_out(hx_bgv_crt* t, hipStream_t st, const uint64_t* w, int batch, int64_t* slots_out)
{
  const size_t bytes = (size_t)batch * t->nslots * 8;
  RC(ensure_buf(t, st, 2, bytes));
  const uint64_t p = t->p;
  HX_LAUNCH(hx::bgv_crt_decode_kernel, dim3(tiles_for(t->nslots, hx::CRT_DI, batch)), dim3(256), 0, st, w, t->d_R, t->nslots, t->N,
            t->ld, batch, p, (uint64_t)(((hxh::u128)1 << 64) / p), t->limit, (int)aligned16(w), (int64_t*)t->buf[2]);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(slots_out, t->buf[2], bytes, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return HX_OK;
}

}  // namespace

extern "C" int hx_bgv_crt_destroy(hx_bgv_crt* t)
{
  if (!t)
    return HX_OK;
  (void)hipSetDevice(t->device);
  (void)hipDeviceSynchronize();
  hipFree(t->d_E);
  hipFree(t->d_R);
  for (void* b : t->buf)
    hipFree(b);
  delete t;
  return HX_OK;
}

extern "C" int hx_bgv_crt_create_pr(hx_ctx* ctx, uint64_t p, int r, hx_bgv_crt** out)
{
  if (!ctx || !out)
    return err(HX_ERR_INVALID, "null argument");
  *out = nullptr;
  hxi::CtxView v{};
  RC(hxi::ctx_enter(ctx, &v));
  std::unique_lock<std::recursive_mutex> lk(*v.mu);
  if (v.capturing)
    return err(HX_ERR_INVALID, "hx_bgv_crt_create while a graph is being captured");
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
  hxc::CrtTables tab;
  const std::string why = hxc::build_crt(m, p, tab, true, (uint32_t)r);
  if (!why.empty())
    return err(why.rfind("internal", 0) == 0 ? HX_ERR_DEVICE : HX_ERR_UNSUPPORTED, "%s", why.c_str());
  if (tab.phim != v.phim)
    return err(HX_ERR_DEVICE, "internal: phi(m) = %u, the context says %u", tab.phim, v.phim);
  hx_bgv_crt* t = new hx_bgv_crt();
  struct Guard {
    hx_bgv_crt* t;
    ~Guard() { hx_bgv_crt_destroy(t); }
  } guard{t};
  t->ctx = ctx;
  t->m = m;
  t->p = P;
  t->prime = p;
  t->r = (uint32_t)r;
  t->N = v.phim;
  t->device = v.device;
  t->d = tab.d;
  t->nslots = tab.nslots;
  t->ld = tab.ld;
  t->limit = (uint32_t)tab.limit;
  t->gens = tab.gens;
  t->ords = tab.ords;
  const size_t bytes = sizeof(uint32_t) * (size_t)tab.nslots * tab.ld;
  CK(hipMalloc((void**)&t->d_E, bytes));
  CK(hipMalloc((void**)&t->d_R, bytes));
  CK(hipMemcpy(t->d_E, tab.E.data(), bytes, hipMemcpyHostToDevice));
  CK(hipMemcpy(t->d_R, tab.R.data(), bytes, hipMemcpyHostToDevice));
  guard.t = nullptr;
  *out = t;
  return HX_OK;
}

extern "C" int hx_bgv_crt_create(hx_ctx* ctx, uint64_t p, hx_bgv_crt** out) { return hx_bgv_crt_create_pr(ctx, p, 1, out); }

extern "C" int hx_bgv_crt_space(const hx_bgv_crt* t, int* r, uint64_t* modulus)
{
  if (!t)
    return err(HX_ERR_INVALID, "null argument");
  if (r)
    *r = (int)t->r;
  if (modulus)
    *modulus = t->p;
  return HX_OK;
}

extern "C" int hx_bgv_crt_info(const hx_bgv_crt* t, uint64_t* p, int* d, int* nslots, int* ndims, uint64_t* gens, int64_t* ords,
                               uint64_t* table_bytes)
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
    *table_bytes = 2 * sizeof(uint32_t) * (uint64_t)t->nslots * t->ld;
  return HX_OK;
}

extern "C" int hx_bgv_crt_encode(const hx_bgv_crt* tc, const int64_t* slots, int batch, uint64_t mul, hx_poly* out,
                                 int64_t* coeffs_out)
{
  if (!tc || !out || !slots)
    return err(HX_ERR_INVALID, "null argument");
  hx_bgv_crt* t = const_cast<hx_bgv_crt*>(tc);   // (its scratch buffers grow; the caller's lock covers them)
  if (batch < 1)
    return err(HX_ERR_INVALID, "bad batch %d", batch);
  Encode e{t, out, batch};
  RC(e.check());
  uint64_t* h;
  RC(e.open("hx_bgv_crt_encode", coeffs_out != nullptr, &h));
  const hipStream_t st = e.st;
  const uint64_t p = t->p;
  const size_t vbytes = (size_t)batch * t->nslots * 8;
  RC(ensure_buf(t, st, 0, std::max<size_t>(vbytes, 16)));
  CK(hipMemcpyAsync(t->buf[0], slots, vbytes, hipMemcpyHostToDevice, st));
  HX_LAUNCH(hx::bgv_crt_encode_kernel, dim3(tiles_for(t->ld, hx::CRT_EK, batch)), dim3(256), 0, st, (const int64_t*)t->buf[0],
            t->d_E, t->nslots, t->N, t->ld, batch, p, (uint64_t)(((hxh::u128)1 << 64) / p), t->limit, h);
  CK(hipGetLastError());
  return e.finish(mul % p, coeffs_out);
}

extern "C" int hx_bgv_crt_embed(const hx_bgv_crt* tc, const int64_t* coeffs, int batch, int64_t* slots_out)
{
  if (!tc || !coeffs || !slots_out)
    return err(HX_ERR_INVALID, "null argument");
  if (batch < 1)
    return err(HX_ERR_INVALID, "bad batch %d", batch);
  hx_bgv_crt* t = const_cast<hx_bgv_crt*>(tc);
  Enter E;
  RC(E.open(t, "hx_bgv_crt_embed"));
  const hipStream_t st = E.v.stream;
  DrainOnExit drain{st};
  const size_t words = (size_t)batch * t->N;
  RC(ensure_buf(t, st, 0, words * 8));
  RC(ensure_buf(t, st, 3, words * 8));
  CK(hipMemcpyAsync(t->buf[0], coeffs, words * 8, hipMemcpyHostToDevice, st));
  RC(launch_redmul(t, st, (const int64_t*)t->buf[0], words, 1 % t->p, (uint64_t*)t->buf[3]));
  return decode_out(t, st, (const uint64_t*)t->buf[3], batch, slots_out);
}

extern "C" int hx_bgv_crt_decode(const hx_bgv_crt* tc, const hx_poly* acc, uint64_t factor_inv, int64_t* slots_out)
{
  if (!tc || !acc || !slots_out)
    return err(HX_ERR_INVALID, "null argument");
  hx_bgv_crt* t = const_cast<hx_bgv_crt*>(tc);
  if (hxi::poly_ctx(acc) != t->ctx)
    return err(HX_ERR_INVALID, "the poly belongs to another context than the slot table");
  Enter E;
  RC(E.open(t, "hx_bgv_crt_decode"));
  int batch = 0, n = 0;
  RC(hx_poly_shape(acc, &batch, &n, nullptr));
  if (n == 0) {   // the zero polynomial
    memset(slots_out, 0, (size_t)batch * t->nslots * 8);
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
