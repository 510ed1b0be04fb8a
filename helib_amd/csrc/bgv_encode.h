// bgv_encode.h -- what bgv_slots.hip (d = 1: the engine's transform mod p) and bgv_crt.hip (any d: a CRT matrix product)
// share on the host side of BGV slot encoding: error plumbing, the grow-only scratch of a slot table, entering the
// caller's context, and the tail of an encode -- the lift of H mod p to the output's primes (bgv_lift_kernel), the
// engine's forward transforms and the zzX.  Included by those two units only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <vector>

#include "../../include/helib_amd.h"
#include "bgv_slots.h"
#include "ckks_bridge.h"
#include "hostmath.h"
#include "prof.h"

namespace hxb {

// the part of a slot table the shared code works on
struct SlotBase {
  hx_ctx* ctx = nullptr;    // the caller's context (not owned)
  hx_ctx* side = nullptr;   // d = 1: holds p as its only prime; the CRT tables have none
  uint64_t m = 0, p = 0;
  uint32_t N = 0;           // phi(m)
  int device = 0;
  // grow-only scratch: slots / coefficients, the prime table, results, H mod p where no side context holds it
  void* buf[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t cap[4] = {0, 0, 0, 0};
};

using hxi::err;           // (with CK and RC: ckks_bridge.h)
using hxi::DrainOnExit;   // every return waits for the stream: no copy still reads a host buffer, no kernel a temporary

inline int ensure_buf(SlotBase* t, hipStream_t st, int slot, size_t bytes)
{
  if (t->cap[slot] >= bytes)
    return HX_OK;
  CK(hipStreamSynchronize(st));   // the old buffer may still be read by work in flight
  hipFree(t->buf[slot]);
  t->buf[slot] = nullptr;
  t->cap[slot] = 0;
  CK(hipMalloc(&t->buf[slot], bytes));
  t->cap[slot] = bytes;
  return HX_OK;
}

// the caller's context: view, lock, no open capture; the side context follows its stream
struct Enter {
  hxi::CtxView v{};
  std::unique_lock<std::recursive_mutex> lk;
  int open(const SlotBase* t, const char* what)
  {
    RC(hxi::ctx_enter(t->ctx, &v));
    lk = std::unique_lock<std::recursive_mutex>(*v.mu);
    if (v.capturing)
      return err(HX_ERR_INVALID, "%s waits for the device and cannot be captured in a graph", what);
    return t->side ? hx_ctx_set_stream(t->side, (void*)v.stream) : HX_OK;
  }
};
struct Drop {
  hx_poly* t;
  ~Drop() { hx_poly_destroy(t); }
};

inline unsigned blocks_for(size_t items)
{
  const size_t b = (items + 255) / 256;
  return (unsigned)std::min<size_t>(std::max<size_t>(b, 1), hx::BGV_MAX_BLOCKS);
}
inline bool aligned16(const void* a) { return ((uintptr_t)a & 15) == 0; }

// a batch of rows modulo p on the side context (one row per element)
inline int side_poly(const SlotBase* t, int batch, hx_poly** out)
{
  const int zero = 0;
  return hx_poly_create_uninit(t->side, batch, &zero, 1, out);
}

// dst = (src mod p) * f mod p over `words` signed words
inline int launch_redmul(const SlotBase* t, hipStream_t st, const int64_t* src, size_t words, uint64_t f, uint64_t* dst)
{
  const uint64_t p = t->p, mu = (uint64_t)(((hxh::u128)1 << 64) / p), fs = hxh::shoup(f, p);
  if (words % 2 == 0 && aligned16(src) && aligned16(dst))
    HX_LAUNCH(hx::bgv_redmul_kernel<2>, dim3(blocks_for(words / 2)), dim3(256), 0, st, src, words, p, mu, f, fs, dst);
  else
    HX_LAUNCH(hx::bgv_redmul_kernel<1>, dim3(blocks_for(words)), dim3(256), 0, st, src, words, p, mu, f, fs, dst);
  CK(hipGetLastError());
  return HX_OK;
}

// What hx_bgv_encode, hx_bgv_encode_diagonals and hx_bgv_crt_encode share.  check: the output's shape.  open: the
// caller's context, the prime table (buf[1]) and where the caller's kernel writes -- the side poly's rows (values at the roots, for a scatter
// kernel) or, without a side context, buf[3] (H mod p itself).  finish: with a side context the inverse transform mod p
// (CRT_reconstruct: the H with the given values at the roots); then the lift, the forward transforms, the zzX.
struct Encode {
  SlotBase* t;
  hx_poly* out;
  int batch, nrows = 0;
  size_t words = 0;
  Enter E;
  hx_poly* sp = nullptr;
  hipStream_t st = nullptr;
  std::vector<ulonglong2> qm;
  ~Encode()
  {
    if (st)
      (void)hipStreamSynchronize(st);   // no copy still reads a host buffer, no kernel a temporary
    if (sp)
      hx_poly_destroy(sp);
  }
  int check()
  {
    if (!out)
      return HX_OK;
    if (hxi::poly_ctx(out) != t->ctx)
      return err(HX_ERR_INVALID, "the output poly belongs to another context than the slot table");
    int pb = 0;
    RC(hx_poly_shape(out, &pb, &nrows, nullptr));
    if (pb != batch)
      return err(HX_ERR_INVALID, "output batch %d != %d", pb, batch);
    if (nrows > hx::BGV_MAXPRIMES)
      return err(HX_ERR_UNSUPPORTED, "more than %d primes", hx::BGV_MAXPRIMES);
    return HX_OK;
  }
  int open(const char* what, bool coeffs, uint64_t** h)
  {
    RC(E.open(t, what));
    std::vector<int> idx(nrows > 0 ? nrows : 1);
    if (out)
      RC(hx_poly_primes(out, idx.data()));
    qm.resize(nrows > 0 ? nrows : 1);
    for (int r = 0; r < nrows; r++) {
      uint64_t q;
      RC(hx_ctx_prime(t->ctx, idx[r], &q, nullptr));
      qm[r] = make_ulonglong2(q, (uint64_t)(((hxh::u128)1 << 64) / q));
    }
    st = E.v.stream;
    words = (size_t)batch * t->N;
    if (t->side)
      RC(side_poly(t, batch, &sp));
    else
      RC(ensure_buf(t, st, 3, words * 8));
    RC(ensure_buf(t, st, 1, sizeof(ulonglong2) * qm.size()));
    if (coeffs)
      RC(ensure_buf(t, st, 2, words * 8));
    CK(hipMemcpyAsync(t->buf[1], qm.data(), sizeof(ulonglong2) * qm.size(), hipMemcpyHostToDevice, st));
    if (sp)
      return hxi::poly_rows_write(sp, h);
    *h = (uint64_t*)t->buf[3];
    return HX_OK;
  }
  int finish(uint64_t mul, int64_t* coeffs_out)
  {
    const uint64_t p = t->p;
    if (sp)
      RC(hx_ntt_inverse(sp));
    const uint64_t* hc = sp ? hxi::poly_rows_read(sp) : (const uint64_t*)t->buf[3];
    uint64_t* rows = nullptr;
    if (nrows > 0)
      RC(hxi::poly_rows_write(out, &rows));
    int64_t* d_coeffs = coeffs_out ? (int64_t*)t->buf[2] : nullptr;
    if (nrows > 0 || d_coeffs) {
      const uint64_t muls = hxh::shoup(mul, p);
      if (words % 2 == 0 && aligned16(hc) && aligned16(rows) && aligned16(d_coeffs))
        HX_LAUNCH(hx::bgv_lift_kernel<2>, dim3(blocks_for(words / 2)), dim3(256), 0, st, hc, words, p, mul, muls,
                  (const ulonglong2*)t->buf[1], nrows, rows, d_coeffs);
      else
        HX_LAUNCH(hx::bgv_lift_kernel<1>, dim3(blocks_for(words)), dim3(256), 0, st, hc, words, p, mul, muls,
                  (const ulonglong2*)t->buf[1], nrows, rows, d_coeffs);
      CK(hipGetLastError());
    }
    if (nrows > 0)
      RC(hx_ntt_forward(out));
    if (coeffs_out)
      CK(hipMemcpyAsync(coeffs_out, d_coeffs, words * 8, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    return HX_OK;
  }
};

}  // namespace hxb
