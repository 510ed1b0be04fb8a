// recrypt.hip -- the pre-processing of recryption on the device (include/helib_amd.h: hx_recrypt_prep): Ctxt::rawModSwitch
// (src/Ctxt.cpp:2949-3049), newMakeDivisible (src/recryption.cpp:73-136) and the division by p^e' (:495-497) of one
// ciphertext part, from its coefficient rows on the ciphertext's primes to rows on the primes of the encrypted
// recryption key.  The arithmetic of one coefficient is recrypt_core.h's, shared with the host replay.
//
// recrypt_prep_kernel<K>: one thread per (batch element, coefficient), the batch element being the grid's y; the rows are [row][batch][phi(m)], so a wave reads
// 64 consecutive words of each of the K input rows and writes 64 consecutive words of each output row.  K is a template
// argument (1..16) so that the mixed-radix digits live in registers; the plan (a few KB of per-prime constants, uniform
// over the grid) is read through scalar loads.  Per coefficient the kernel moves 8 (K + |T|) bytes and does about K^2
// modular products: at phi(m) = 16384, batch 32, K = 5, |T| = 8 that is 55 MB -- bandwidth-trivial.  The kernel exists
// to keep the step on the device between two transforms, not to win a roofline.
#include <mutex>
#include <string>
#include <vector>

#include "bgv_encode.h"
#include "recrypt_core.h"

namespace hx {

constexpr int RC_T = 256;

template <int K>
__global__ void __launch_bounds__(RC_T)
recrypt_prep_kernel(const hxrc::Plan* __restrict__ plan, const uint64_t* __restrict__ in, uint64_t* __restrict__ out, size_t row_words,
                    uint32_t phim, int64_t* __restrict__ x_out, int64_t* __restrict__ v_out)
{
  const uint32_t j = blockIdx.x * RC_T + threadIdx.x, b = blockIdx.y;   // (the grid's y is the batch: no division)
  if (j >= phim)
    return;
  const size_t idx = (size_t)b * phim + j;
  const hxrc::Plan& P = *plan;
  uint64_t c[K];
#pragma unroll
  for (int i = 0; i < K; i++)
    c[i] = in[(size_t)i * row_words + idx];
  const hxrc::Result R = hxrc::prep_one<K>(P, c, b, j);
  if (x_out)
    x_out[idx] = R.x;
  if (v_out)
    v_out[idx] = R.v;
  const uint32_t nt = P.nt;
  for (uint32_t t = 0; t < nt; t++)
    out[(size_t)t * row_words + idx] = hxrc::residue(R.w, P.tgt[t]);
}

}  // namespace hx

using namespace hxb;

namespace {

// the plan's place on the device, one per context (freed with it): written and read under the context's lock, every
// call draining the stream before it returns
void free_plan(void* p) { (void)hipFree(p); }

template <int K>
void launch(hipStream_t st, dim3 grid, const hxrc::Plan* d_plan, const uint64_t* in, uint64_t* out, size_t rw, uint32_t phim,
            int64_t* dx, int64_t* dv)
{
  HX_LAUNCH(hx::recrypt_prep_kernel<K>, grid, dim3(hx::RC_T), 0, st, d_plan, in, out, rw, phim, dx, dv);
}

struct FreeOnExit {
  void* p = nullptr;
  ~FreeOnExit() { (void)hipFree(p); }
};

}  // namespace

extern "C" int hx_recrypt_prep(const hx_poly* in, hx_poly* out, uint64_t q, uint64_t p, uint64_t p2r, uint64_t p2ePrime,
                               uint64_t tie_seed, int part, int64_t* x_host, int64_t* v_host)
{
  if (!in || !out)
    return err(HX_ERR_INVALID, "null argument");
  if (in == out)
    return err(HX_ERR_INVALID, "hx_recrypt_prep: the output is the input");
  if (part < 0)
    return err(HX_ERR_INVALID, "hx_recrypt_prep: part %d", part);
  hx_ctx* ctx = hxi::poly_ctx(in);
  if (hxi::poly_ctx(out) != ctx)
    return err(HX_ERR_INVALID, "hx_recrypt_prep: the output belongs to another context than the input");
  hxi::CtxView v{};
  RC(hxi::ctx_enter(ctx, &v));
  std::unique_lock<std::recursive_mutex> lk(*v.mu);
  if (v.capturing)
    return err(HX_ERR_INVALID, "hx_recrypt_prep waits for the device and cannot be captured in a graph");
  int batch = 0, k = 0, bo = 0, nt = 0;
  RC(hx_poly_shape(in, &batch, &k, nullptr));
  RC(hx_poly_shape(out, &bo, &nt, nullptr));
  if (bo != batch)
    return err(HX_ERR_INVALID, "hx_recrypt_prep: the input holds %d batch elements, the output %d", batch, bo);
  if (k < 1 || nt < 1)
    return err(HX_ERR_INVALID, "hx_recrypt_prep: %d input rows, %d output rows", k, nt);
  if (k > hxrc::MAX_K)
    return err(HX_ERR_UNSUPPORTED, "the part has %d rows; the exact lift of recryption's pre-processing takes 1 to %d", k, hxrc::MAX_K);
  if (nt > hxrc::MAX_T)
    return err(HX_ERR_UNSUPPORTED, "the output has %d rows; recryption's pre-processing writes 1 to %d", nt, hxrc::MAX_T);
  std::vector<int> si(k), ti(nt);
  RC(hx_poly_primes(in, si.data()));
  RC(hx_poly_primes(out, ti.data()));
  std::vector<uint64_t> sq(k), tq(nt);
  for (int i = 0; i < k; i++)
    RC(hx_ctx_prime(ctx, si[i], &sq[i], nullptr));
  for (int i = 0; i < nt; i++)
    RC(hx_ctx_prime(ctx, ti[i], &tq[i], nullptr));
  for (int i = 0; i < k; i++)
    for (int l = 0; l < i; l++)
      if (si[i] == si[l])
        return err(HX_ERR_INVALID, "hx_recrypt_prep: prime %d appears twice among the input's rows", si[i]);
  hxrc::Plan P;
  const std::string why = hxrc::build_plan(sq, tq, q, p, p2r, p2ePrime, P);
  if (!why.empty())
    return err(HX_ERR_INVALID, "hx_recrypt_prep: %s", why.c_str());
  P.seed = tie_seed;
  P.part = (uint64_t)part;
  const size_t rw = (size_t)batch * v.phim;
  if (batch > 65535)
    return err(HX_ERR_UNSUPPORTED, "hx_recrypt_prep: %d batch elements are more than the grid's 65535", batch);
  const hipStream_t st = v.stream;
  if (!*v.recrypt) {
    CK(hipMalloc(v.recrypt, sizeof(hxrc::Plan)));
    *v.recrypt_free = free_plan;
  }
  hxrc::Plan* d_plan = (hxrc::Plan*)*v.recrypt;
  FreeOnExit xv;
  int64_t *dx = nullptr, *dv = nullptr;
  if (x_host || v_host) {
    CK(hipMalloc(&xv.p, 2 * rw * 8));
    dx = (int64_t*)xv.p;
    dv = dx + rw;
  }
  const uint64_t* d_in = hxi::poly_rows_read(in);
  uint64_t* d_out = nullptr;
  RC(hxi::poly_rows_write(out, &d_out));
  DrainOnExit drain{st};   // (declared after xv: the stream is drained before the buffer is freed)
  CK(hipMemcpyAsync(d_plan, &P, sizeof P, hipMemcpyHostToDevice, st));
  const dim3 grid((v.phim + hx::RC_T - 1) / hx::RC_T, (unsigned)batch);
  switch (k) {
#define HXRC_CASE(K)                                                    \
  case K:                                                               \
    launch<K>(st, grid, d_plan, d_in, d_out, rw, v.phim, dx, dv);       \
    break;
    HXRC_CASE(1) HXRC_CASE(2) HXRC_CASE(3) HXRC_CASE(4) HXRC_CASE(5) HXRC_CASE(6) HXRC_CASE(7) HXRC_CASE(8)
    HXRC_CASE(9) HXRC_CASE(10) HXRC_CASE(11) HXRC_CASE(12) HXRC_CASE(13) HXRC_CASE(14) HXRC_CASE(15) HXRC_CASE(16)
#undef HXRC_CASE
  }
  CK(hipGetLastError());
  if (x_host)
    CK(hipMemcpyAsync(x_host, dx, rw * 8, hipMemcpyDeviceToHost, st));
  if (v_host)
    CK(hipMemcpyAsync(v_host, dv, rw * 8, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return HX_OK;
}
