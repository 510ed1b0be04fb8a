// ckks_slots.hip -- C ABI of CKKS slot encoding and decoding (include/helib_amd.h: hx_ckks_encode, hx_ckks_embed,
// hx_ckks_decode): EncryptedArrayCx's CKKS_embedInSlots / CKKS_canonicalEmbedding (src/norms.cpp:495-615) and the
// decode half of rawDecrypt (src/EaCx.cpp:62-86) on the device.  Kernels: ckks_slots.h.  The unit reaches the
// context only through ckks_bridge.h (stream, lock, a state slot, a poly's rows); transforms, copies and polys go
// through the C ABI itself.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/helib_amd.h"
#include "ckks_bridge.h"
#include "ckks_slots.h"
#include "prof.h"

namespace {

typedef unsigned __int128 u128h;

// per-context state: tables of the ring and grow-only scratch buffers (freed with the context)
struct CkksState {
  uint64_t m = 0;
  double2* wtab = nullptr;    // W^k, k < N
  uint32_t* jinfo = nullptr;  // ckks_slots.h
  void* buf[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t cap[4] = {0, 0, 0, 0};
  unsigned* flag = nullptr;
};
void state_free(void* p)
{
  CkksState* s = static_cast<CkksState*>(p);
  if (!s)
    return;
  hipFree(s->wtab);
  hipFree(s->jinfo);
  for (void* b : s->buf)
    hipFree(b);
  hipFree(s->flag);
  delete s;
}

using hxi::err;   // (with CK, RC and DrainOnExit: ckks_bridge.h)
using hxi::DrainOnExit;

// the range of the slot kernels: CKKS needs m a power of two (PAlgebra, src/PAlgebra.cpp:463-467); the device
// transforms cover N = phi(m) <= 2^16 (the norm kernels' range)
int check_ring(uint64_t m, int* logn)
{
  if (m < 2 || (m & (m - 1)))
    return err(HX_ERR_INVALID, "CKKS scheme only supports m as a power of two.");
  if (m < 16 || m > (1u << 17))
    return err(HX_ERR_UNSUPPORTED, "CKKS slot encoding on the device needs 16 <= m <= 2^17 (m = %llu)",
               (unsigned long long)m);
  int k = 0;
  while ((2ull << k) < m)
    k++;
  *logn = k;   // N = m/2 = 2^k
  return HX_OK;
}

// T[i] = 3^i mod m: PAlgebra's table for p = -1 and m = 2^k (findGenerators picks the single generator 3, of order
// m/4 in Z_m^*/<-1>; tests/test_ckks_slots_host.py checks it against the host's ZmStar)
int ensure_tables(CkksState* s, uint64_t m)
{
  if (s->m == m)
    return HX_OK;
  const uint32_t N = (uint32_t)(m / 2), Q = N / 2;
  std::vector<double> w(2 * (size_t)N);
  const long double two_pi = 6.283185307179586476925286766559005768394L;
  for (uint32_t k = 0; k < N; k++) {
    const long double ang = two_pi * (long double)k / (long double)m;
    w[2 * (size_t)k] = (double)cosl(ang);
    w[2 * (size_t)k + 1] = (double)sinl(ang);
  }
  std::vector<uint32_t> T(Q), jinfo(N, 0xffffffffu);
  uint64_t t = 1;
  for (uint32_t i = 0; i < Q; i++, t = t * 3 % m)
    T[i] = (uint32_t)t;
  for (uint32_t sl = 0; sl < Q; sl++) {
    const uint32_t j = (uint32_t)((m - T[Q - 1 - sl] - 1) / 2);
    if (jinfo[j] != 0xffffffffu || jinfo[N - 1 - j] != 0xffffffffu)
      return err(HX_ERR_INVALID, "internal: slot table collision at m = %llu", (unsigned long long)m);
    jinfo[j] = sl;
    jinfo[N - 1 - j] = sl | hx::CKKS_CONJ;
  }
  hipFree(s->wtab);
  hipFree(s->jinfo);
  s->wtab = nullptr;
  s->jinfo = nullptr;
  s->m = 0;
  CK(hipMalloc((void**)&s->wtab, sizeof(double2) * N));
  CK(hipMalloc((void**)&s->jinfo, sizeof(uint32_t) * N));
  CK(hipMemcpy(s->wtab, w.data(), sizeof(double2) * N, hipMemcpyHostToDevice));
  CK(hipMemcpy(s->jinfo, jinfo.data(), sizeof(uint32_t) * N, hipMemcpyHostToDevice));
  if (!s->flag)
    CK(hipMalloc((void**)&s->flag, sizeof(unsigned)));
  s->m = m;
  return HX_OK;
}

int ensure_buf(CkksState* s, hipStream_t st, int slot, size_t bytes)
{
  if (s->cap[slot] >= bytes)
    return HX_OK;
  CK(hipStreamSynchronize(st));   // the old buffer may still be read by work in flight
  hipFree(s->buf[slot]);
  s->buf[slot] = nullptr;
  s->cap[slot] = 0;
  CK(hipMalloc(&s->buf[slot], bytes));
  s->cap[slot] = bytes;
  return HX_OK;
}

// the context's view, lock and slot state
struct Enter {
  hxi::CtxView v{};
  std::unique_lock<std::recursive_mutex> lk;
  CkksState* s = nullptr;
  int logn = 0;
  int open(hx_ctx* c, const char* what)
  {
    RC(hxi::ctx_enter(c, &v));
    lk = std::unique_lock<std::recursive_mutex>(*v.mu);
    if (v.capturing)
      return err(HX_ERR_INVALID, "%s waits for the device and cannot be captured in a graph", what);
    RC(check_ring(v.m, &logn));
    if (!*v.state) {
      *v.state = new CkksState();
      *v.state_free = state_free;
    }
    s = static_cast<CkksState*>(*v.state);
    return ensure_tables(s, v.m);
  }
};

// the two transform launches: S = N/H workgroups per row, H <= 8192 points each
void geometry(int logn, int* logh, unsigned* S, unsigned* nth)
{
  *logh = logn < hx::NORM_MAX_LOGH ? logn : hx::NORM_MAX_LOGH;
  *S = 1u << (logn - *logh);
  const unsigned H = 1u << *logh;
  *nth = H / 4 < 64 ? 64 : (H / 4 > (unsigned)hx::NORM_THREADS ? (unsigned)hx::NORM_THREADS : H / 4);
}

int launch_embed(Enter& E, const double* d_f, int batch, double2* d_slots)
{
  int logh;
  unsigned S, nth;
  geometry(E.logn, &logh, &S, &nth);
  const int lds = (int)(16u << logh);
  CK(hxp::dyn_lds((const void*)hx::ckks_embed_kernel, lds));
  HX_LAUNCH(hx::ckks_embed_kernel, dim3((unsigned)batch * S), dim3(nth), lds, E.v.stream, d_f, E.s->wtab, E.s->jinfo,
            E.logn, logh, d_slots);
  CK(hipGetLastError());
  return HX_OK;
}

uint64_t powmod(uint64_t a, uint64_t e, uint64_t q)
{
  uint64_t r = 1 % q;
  a %= q;
  for (; e; e >>= 1, a = (uint64_t)((u128h)a * a % q))
    if (e & 1)
      r = (uint64_t)((u128h)r * a % q);
  return r;
}

}  // namespace

extern "C" int hx_ckks_encode(hx_ctx* ctx, const double* slots, int batch, int nslots, double scaling, hx_poly* out,
                              int64_t* coeffs_out)
{
  if (!ctx || !out || (nslots > 0 && !slots))
    return err(HX_ERR_INVALID, "null argument");
  Enter E;
  RC(E.open(ctx, "hx_ckks_encode"));
  const uint32_t N = E.v.phim;
  if (batch < 1 || nslots < 0 || (uint32_t)nslots > N / 2)
    return err(HX_ERR_INVALID, "bad batch / slot count (batch %d, %d slots of at most %u)", batch, nslots, N / 2);
  if (!std::isfinite(scaling))
    return err(HX_ERR_INVALID, "scaling must be finite");
  if (hxi::poly_ctx(out) != ctx)
    return err(HX_ERR_INVALID, "the output poly belongs to another context");
  int pb = 0, nrows = 0;
  RC(hx_poly_shape(out, &pb, &nrows, nullptr));
  if (pb != batch)
    return err(HX_ERR_INVALID, "output batch %d != %d", pb, batch);
  if (nrows > hx::CKKS_MAXPRIMES)
    return err(HX_ERR_UNSUPPORTED, "more than %d primes", hx::CKKS_MAXPRIMES);
  std::vector<int> idx(nrows > 0 ? nrows : 1);
  RC(hx_poly_primes(out, idx.data()));
  std::vector<ulonglong2> qm(nrows > 0 ? nrows : 1);
  for (int r = 0; r < nrows; r++) {
    uint64_t q, root;
    RC(hx_ctx_prime(ctx, idx[r], &q, &root));
    qm[r] = make_ulonglong2(q, (uint64_t)(((u128h)1 << 64) / q));
  }
  CkksState* s = E.s;
  const hipStream_t st = E.v.stream;
  DrainOnExit drain{st};
  const size_t words = (size_t)batch * N, vbytes = (size_t)batch * nslots * 16;
  RC(ensure_buf(s, st, 0, vbytes > 16 ? vbytes : 16));
  RC(ensure_buf(s, st, 1, words * 8));
  RC(ensure_buf(s, st, 2, sizeof(ulonglong2) * qm.size()));
  if (vbytes)
    CK(hipMemcpyAsync(s->buf[0], slots, vbytes, hipMemcpyHostToDevice, st));
  CK(hipMemcpyAsync(s->buf[2], qm.data(), sizeof(ulonglong2) * qm.size(), hipMemcpyHostToDevice, st));
  CK(hipMemsetAsync(s->flag, 0, sizeof(unsigned), st));
  int logh;
  unsigned S, nth;
  geometry(E.logn, &logh, &S, &nth);
  const int lds = (int)(16u << logh);
  CK(hxp::dyn_lds((const void*)hx::ckks_encode_kernel, lds));
  // CKKS_embedInSlots: scaling /= (m/2), the inverse DFT's 1/N
  HX_LAUNCH(hx::ckks_encode_kernel, dim3((unsigned)batch * S), dim3(nth), lds, st, (const double2*)s->buf[0],
            (unsigned)nslots, s->wtab, s->jinfo, E.logn, logh, scaling / (double)N, (int64_t*)s->buf[1], s->flag);
  CK(hipGetLastError());
  if (nrows > 0) {
    uint64_t* rows;
    RC(hxi::poly_rows_write(out, &rows));
    HX_LAUNCH(hx::ckks_residues_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st,
              (const int64_t*)s->buf[1], words, (const ulonglong2*)s->buf[2], nrows, rows);
    CK(hipGetLastError());
    RC(hx_ntt_forward(out));
  }
  unsigned flag = 0;
  CK(hipMemcpyAsync(&flag, s->flag, sizeof flag, hipMemcpyDeviceToHost, st));
  if (coeffs_out)
    CK(hipMemcpyAsync(coeffs_out, s->buf[1], words * 8, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  if (flag)
    return err(HX_ERR_INVALID, "overflow in encoding");
  return HX_OK;
}

extern "C" int hx_ckks_embed(hx_ctx* ctx, const double* coeffs, int batch, double* slots_out)
{
  if (!ctx || !coeffs || !slots_out)
    return err(HX_ERR_INVALID, "null argument");
  Enter E;
  RC(E.open(ctx, "hx_ckks_embed"));
  if (batch < 1)
    return err(HX_ERR_INVALID, "bad batch %d", batch);
  const uint32_t N = E.v.phim;
  CkksState* s = E.s;
  const hipStream_t st = E.v.stream;
  DrainOnExit drain{st};
  const size_t words = (size_t)batch * N;
  RC(ensure_buf(s, st, 0, words * 8));
  RC(ensure_buf(s, st, 1, words * 8));   // batch * N/2 complex
  CK(hipMemcpyAsync(s->buf[0], coeffs, words * 8, hipMemcpyHostToDevice, st));
  RC(launch_embed(E, (const double*)s->buf[0], batch, (double2*)s->buf[1]));
  CK(hipMemcpyAsync(slots_out, s->buf[1], words * 8, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return HX_OK;
}

extern "C" int hx_ckks_decode(const hx_poly* p, double ln_rat_factor, double* slots_out)
{
  if (!p || !slots_out)
    return err(HX_ERR_INVALID, "null argument");
  if (!std::isfinite(ln_rat_factor))
    return err(HX_ERR_INVALID, "ln(ratFactor) must be finite");
  hx_ctx* ctx = hxi::poly_ctx(p);
  Enter E;
  RC(E.open(ctx, "hx_ckks_decode"));
  const uint32_t N = E.v.phim;
  int batch = 0, n = 0;
  RC(hx_poly_shape(p, &batch, &n, nullptr));
  const size_t words = (size_t)batch * N;
  if (n == 0) {   // the zero polynomial
    memset(slots_out, 0, words * 8);
    return HX_OK;
  }
  if (n > hx::CKKS_MAXPRIMES)
    return err(HX_ERR_UNSUPPORTED, "decode from more than %d primes", hx::CKKS_MAXPRIMES);
  std::vector<int> idx(n);
  RC(hx_poly_primes(p, idx.data()));
  // DecryptCKKS's constants: Garner inverses, weights P_k / ratFactor = 2^(sum_(j<k) log2 q_j - log2 ratFactor)
  hx::CkksCrtTab tab;
  memset(&tab, 0, sizeof tab);
  std::vector<uint64_t> q(n);
  long double run = -(long double)ln_rat_factor;
  for (int k = 0; k < n; k++) {
    uint64_t root;
    RC(hx_ctx_prime(ctx, idx[k], &q[k], &root));
    tab.qm[k] = make_ulonglong2(q[k], (uint64_t)(((u128h)1 << 64) / q[k]));
    const long double l2 = run / logl(2.0L);
    const long double e = floorl(l2);
    tab.wm[k] = (double)exp2l(l2 - e);
    tab.we[k] = (int)e;
    run += logl((long double)q[k]);
  }
  std::vector<ulonglong2> ginv((size_t)n * n, make_ulonglong2(0, 0));
  for (int k = 0; k < n; k++)
    for (int l = 0; l < k; l++) {
      const uint64_t g = powmod(q[l] % q[k], q[k] - 2, q[k]);
      ginv[(size_t)k * n + l] = make_ulonglong2(g, (uint64_t)(((u128h)g << 64) / q[k]));
    }
  CkksState* s = E.s;
  const hipStream_t st = E.v.stream;
  // the rows in coefficient form: a copy of p, inverse-transformed (p itself is unchanged)
  hx_poly* tmp = nullptr;
  RC(hx_poly_create_uninit(ctx, batch, idx.data(), n, &tmp));
  struct Drop {
    hx_poly* t;
    ~Drop() { hx_poly_destroy(t); }
  } drop{tmp};
  DrainOnExit drain{st};
  RC(hx_poly_copy(tmp, p));
  RC(hx_ntt_inverse(tmp));
  const size_t tbytes = sizeof tab + sizeof(ulonglong2) * ginv.size();
  RC(ensure_buf(s, st, 0, words * 8));
  RC(ensure_buf(s, st, 1, words * 8));
  RC(ensure_buf(s, st, 3, tbytes));
  CK(hipMemcpyAsync(s->buf[3], &tab, sizeof tab, hipMemcpyHostToDevice, st));
  ulonglong2* d_ginv = (ulonglong2*)((char*)s->buf[3] + sizeof tab);
  CK(hipMemcpyAsync(d_ginv, ginv.data(), sizeof(ulonglong2) * ginv.size(), hipMemcpyHostToDevice, st));
  const uint64_t* rows = hxi::poly_rows_read(tmp);
  const dim3 grid((unsigned)((words + 255) / 256)), blk(256);
  const hx::CkksCrtTab* d_tab = (const hx::CkksCrtTab*)s->buf[3];
  double* d_f = (double*)s->buf[0];
  if (n <= 8)
    HX_LAUNCH(hx::ckks_crt_double_kernel<8>, grid, blk, 0, st, rows, words, n, d_tab, d_ginv, d_f);
  else if (n <= 16)
    HX_LAUNCH(hx::ckks_crt_double_kernel<16>, grid, blk, 0, st, rows, words, n, d_tab, d_ginv, d_f);
  else if (n <= 32)
    HX_LAUNCH(hx::ckks_crt_double_kernel<32>, grid, blk, 0, st, rows, words, n, d_tab, d_ginv, d_f);
  else
    HX_LAUNCH(hx::ckks_crt_double_kernel<64>, grid, blk, 0, st, rows, words, n, d_tab, d_ginv, d_f);
  CK(hipGetLastError());
  RC(launch_embed(E, d_f, batch, (double2*)s->buf[1]));
  CK(hipMemcpyAsync(slots_out, s->buf[1], words * 8, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));   // (tables and the temporary stay alive until here)
  return HX_OK;
}
