// powerful.hip -- the powerful basis on the device (include/helib_amd.h: hx_powerful_create, hx_powerful_destroy,
// hx_poly_to_powerful, hx_powerful_to_poly, hx_powerful_words): the per-prime step of PowerfulDCRT::dcrtToPowerful /
// powerfulToZZX (src/powerful.cpp:354-415) on the coefficient rows of a poly, and PowerfulConversion::polyToPowerful /
// powerfulToPoly (:199-244) on host words modulo any q < 2^62.  The tables and the pass list are powerful.h's.
//
// powerful_kernel: one workgroup of 1024 threads per (row, batch element); a workgroup keeps three buffers of m words (the
// long cube and a ping-pong pair) in global scratch -- at m = 21845 the cube alone is 175 KB, above the LDS -- and runs
// the pass list with a barrier between passes (a workgroup barrier orders its own global stores).  A grid of at most
// PW_MAX_BLOCKS workgroups walks the items, so the scratch is PW_MAX_BLOCKS x 3 m words whatever the batch.
//   elementwise passes (REV, MUL, REVW, SUB): one thread per word, the inner coordinate fastest (coalesced)
//   DIV by 1 - x^e: nfibres e independent running sums ("chains").  With at least 1024 chains a thread walks a chain.
//     With fewer, a chain is cut into S = 1024 / chains segments: a thread sums its segment, the S partial sums of a
//     chain meet in the LDS, every thread adds the ones before it and walks its segment again.  e = 1 on one fibre (any
//     squarefree m, to_poly) is the plain workgroup scan over up to m words.
// Every word is below q and sums stay below 2^63; there is no multiplication.  Per item the kernel reads and writes
// 8 phi(m) bytes of the row and about 16 m bytes per pass of scratch, which stays in the L2.
#include <cstring>
#include <vector>

#include "bgv_encode.h"
#include "powerful.h"

namespace hx {

constexpr int PW_T = 1024;
constexpr int PW_MAX_BLOCKS = 256;

__device__ __forceinline__ uint64_t pw_add(uint64_t a, uint64_t b, uint64_t q)
{
  const uint64_t s = a + b;
  return s >= q ? s - q : s;
}
__device__ __forceinline__ uint64_t pw_sub(uint64_t a, uint64_t b, uint64_t q) { return a >= b ? a - b : a + q - b; }

// data: [rows][batch][phim] words below the row's modulus qs[row]; in place.  scat[phim]: where word j goes in the
// zeroed cube; gath[phim] (null: the identity): where word j comes from.  scratch: gridDim.x x 3 m words.
__global__ void __launch_bounds__(PW_T)
powerful_kernel(uint64_t* __restrict__ data, const uint64_t* __restrict__ qs, uint32_t items, uint32_t batch, uint32_t phim, uint32_t m,
                const uint32_t* __restrict__ scat, const uint32_t* __restrict__ gath, const hxpw::Dim* __restrict__ dims,
                const uint32_t* __restrict__ outer, const hxpw::Pass* __restrict__ passes, uint32_t npass, uint64_t* __restrict__ scratch)
{
  __shared__ uint64_t part[PW_T];
  const uint32_t tid = threadIdx.x;
  uint64_t* const buf0 = scratch + (size_t)blockIdx.x * 3 * m;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    uint64_t* const row = data + (size_t)item * phim;
    const uint64_t q = qs[item / batch];
    for (uint32_t x = tid; x < m; x += PW_T)
      buf0[x] = 0;
    __syncthreads();
    for (uint32_t j = tid; j < phim; j += PW_T)
      buf0[scat[j]] = row[j];
    __syncthreads();
    for (uint32_t pi = 0; pi < npass; pi++) {
      const hxpw::Pass ps = passes[pi];
      const hxpw::Dim d = dims[ps.dim];
      const uint64_t* const src = buf0 + (size_t)ps.src * m;
      uint64_t* const dst = buf0 + (size_t)ps.dst * m;
      const uint32_t s = d.stride, L = ps.L, e = ps.e;
      if (ps.op != hxpw::OP_DIV) {
        const uint32_t per = L * s, total = d.nouter * per;   // <= m
        for (uint32_t idx = tid; idx < total; idx += PW_T) {
          const uint32_t o = idx / per, rest = idx - o * per, k = rest / s, in = rest - k * s;
          const uint32_t base = outer[d.outer_off + o] + in, at = base + k * s;
          uint64_t v;
          switch (ps.op) {
          case hxpw::OP_REV:
            v = src[base + (d.n - 1 - k) * s];
            break;
          case hxpw::OP_MUL:
            v = k >= e ? pw_sub(src[at], src[at - e * s], q) : src[at];
            break;
          case hxpw::OP_REVW:
            v = k <= e ? src[base + (e - k) * s] : 0;
            break;
          default:   // OP_SUB
            v = pw_sub(dst[at], src[at], q);
            break;
          }
          dst[at] = v;
        }
      } else {
        const uint32_t per = e * s, chains = d.nouter * per;   // e < L: chains < m
        if (chains >= (uint32_t)PW_T) {
          for (uint32_t c = tid; c < chains; c += PW_T) {
            const uint32_t o = c / per, rest = c - o * per, r = rest / s, in = rest - r * s;
            const uint32_t base = outer[d.outer_off + o] + in;
            uint64_t run = 0;
            for (uint32_t k = r; k < L; k += e) {
              run = pw_add(run, dst[base + k * s], q);
              dst[base + k * s] = run;
            }
          }
        } else {
          const uint32_t S = (uint32_t)PW_T / chains, c = tid % chains, sg = tid / chains;
          const uint32_t o = c / per, rest = c - o * per, r = rest / s, in = rest - r * s;
          const uint32_t base = outer[d.outer_off + o] + in;
          const uint32_t Lc = r < L ? (L - r + e - 1) / e : 0, seg = (Lc + S - 1) / S;
          const uint32_t t0 = min(sg * seg, Lc), t1 = sg < S ? min(t0 + seg, Lc) : t0;   // (sg >= S: the idle tail of the workgroup)
          uint64_t sum = 0;
          for (uint32_t t = t0; t < t1; t++)
            sum = pw_add(sum, dst[base + (r + t * e) * s], q);
          part[tid] = sum;
          __syncthreads();
          uint64_t run = 0;
          for (uint32_t g = 0; g < sg && g < S; g++)
            run = pw_add(run, part[g * chains + c], q);
          for (uint32_t t = t0; t < t1; t++) {
            const uint32_t at = base + (r + t * e) * s;
            run = pw_add(run, dst[at], q);
            dst[at] = run;
          }
        }
      }
      __syncthreads();
    }
    for (uint32_t j = tid; j < phim; j += PW_T)
      row[j] = buf0[gath ? gath[j] : j];
    __syncthreads();   // the next item zeroes the cube
  }
}

}  // namespace hx

using namespace hxb;

struct hx_powerful {
  hx_ctx* ctx = nullptr;
  int device = 0;
  hxpw::Tables tab;
  uint32_t* d_p2c = nullptr;   // the first phi(m) words of p2c
  uint32_t* d_s2l = nullptr;
  uint32_t* d_s2e = nullptr;
  struct Prog {
    hxpw::Dim* dims = nullptr;
    uint32_t* outer = nullptr;
    hxpw::Pass* passes = nullptr;
    uint32_t npass = 0;
  } prog[2];   // 0: to_poly, 1: to_powerful
  uint64_t* scratch = nullptr;   // PW_MAX_BLOCKS x 3 m words
  uint64_t* d_q = nullptr;       // the rows' moduli
  size_t qcap = 0;
  uint64_t* d_words = nullptr;   // hx_powerful_words' rows
  size_t wcap = 0;
};

namespace {

template <typename T>
hipError_t upload(T** dst, const std::vector<T>& src)
{
  if (src.empty())
    return hipSuccess;
  hipError_t e = hipMalloc((void**)dst, sizeof(T) * src.size());
  return e != hipSuccess ? e : hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice);
}

// rows x batch items of phi(m) words on the device, row r modulo q[r]
int run(hx_powerful* t, hipStream_t st, int to_powerful, uint64_t* d_data, const std::vector<uint64_t>& q, int batch)
{
  if (t->qcap < q.size()) {
    CK(hipStreamSynchronize(st));
    hipFree(t->d_q);
    t->d_q = nullptr;
    t->qcap = 0;
    CK(hipMalloc((void**)&t->d_q, 8 * q.size()));
    t->qcap = q.size();
  }
  CK(hipMemcpyAsync(t->d_q, q.data(), 8 * q.size(), hipMemcpyHostToDevice, st));
  const size_t items = q.size() * (size_t)batch;
  if (items > 0xffffffffu)
    return err(HX_ERR_UNSUPPORTED, "%zu rows x %d elements are more than 2^32 - 1 items", q.size(), batch);
  const hx_powerful::Prog& p = t->prog[to_powerful ? 1 : 0];
  const unsigned grid = (unsigned)std::min<size_t>(items, hx::PW_MAX_BLOCKS);
  HX_LAUNCH(hx::powerful_kernel, dim3(grid), dim3(hx::PW_T), 0, st, d_data, (const uint64_t*)t->d_q, (uint32_t)items, (uint32_t)batch,
            t->tab.phim, (uint32_t)t->tab.m, (const uint32_t*)(to_powerful ? t->d_p2c : t->d_s2e),
            (const uint32_t*)(to_powerful ? t->d_s2l : nullptr), (const hxpw::Dim*)p.dims, (const uint32_t*)p.outer,
            (const hxpw::Pass*)p.passes, p.npass, t->scratch);
  CK(hipGetLastError());
  return HX_OK;
}

int convert_poly(const hx_powerful* tc, hx_poly* a, int to_powerful, const char* what)
{
  if (!tc || !a)
    return err(HX_ERR_INVALID, "null argument");
  hx_powerful* t = const_cast<hx_powerful*>(tc);   // (its scratch is the caller's lock's)
  if (hxi::poly_ctx(a) != t->ctx)
    return err(HX_ERR_INVALID, "the poly belongs to another context than the powerful-basis tables");
  hxi::CtxView v{};
  RC(hxi::ctx_enter(t->ctx, &v));
  std::unique_lock<std::recursive_mutex> lk(*v.mu);
  if (v.capturing)
    return err(HX_ERR_INVALID, "%s waits for the device and cannot be captured in a graph", what);
  int batch = 0, nrows = 0;
  RC(hx_poly_shape(a, &batch, &nrows, nullptr));
  if (nrows == 0)
    return HX_OK;
  std::vector<int> idx(nrows);
  RC(hx_poly_primes(a, idx.data()));
  std::vector<uint64_t> q(nrows);
  for (int r = 0; r < nrows; r++)
    RC(hx_ctx_prime(t->ctx, idx[r], &q[r], nullptr));
  uint64_t* d = nullptr;
  RC(hxi::poly_rows_update(a, &d));
  DrainOnExit drain{v.stream};
  return run(t, v.stream, to_powerful, d, q, batch);
}

}  // namespace

extern "C" int hx_powerful_destroy(hx_powerful* t)
{
  if (!t)
    return HX_OK;
  (void)hipSetDevice(t->device);
  (void)hipDeviceSynchronize();
  for (void* b : {(void*)t->d_p2c, (void*)t->d_s2l, (void*)t->d_s2e, (void*)t->scratch, (void*)t->d_q, (void*)t->d_words})
    hipFree(b);
  for (auto& p : t->prog)
    for (void* b : {(void*)p.dims, (void*)p.outer, (void*)p.passes})
      hipFree(b);
  delete t;
  return HX_OK;
}

extern "C" int hx_powerful_create(hx_ctx* ctx, const uint64_t* mvec, int k, hx_powerful** out)
{
  if (!ctx || !mvec || !out)
    return err(HX_ERR_INVALID, "null argument");
  *out = nullptr;
  hxi::CtxView v{};
  RC(hxi::ctx_enter(ctx, &v));
  std::unique_lock<std::recursive_mutex> lk(*v.mu);
  if (v.capturing)
    return err(HX_ERR_INVALID, "hx_powerful_create while a graph is being captured");
  hx_powerful* t = new hx_powerful();
  struct Guard {
    hx_powerful* t;
    ~Guard() { hx_powerful_destroy(t); }
  } guard{t};
  t->ctx = ctx;
  t->device = v.device;
  const std::string why = hxpw::build(mvec, k, t->tab);
  if (!why.empty())
    return err(HX_ERR_INVALID, "%s", why.c_str());
  if (t->tab.m != v.m || t->tab.phim != v.phim)
    return err(HX_ERR_INVALID, "the factors multiply to %llu, the context's m is %llu", (unsigned long long)t->tab.m,
               (unsigned long long)v.m);
  const hxpw::Tables& tab = t->tab;
  CK(upload(&t->d_p2c, std::vector<uint32_t>(tab.p2c.begin(), tab.p2c.begin() + tab.phim)));
  CK(upload(&t->d_s2l, tab.s2l));
  CK(upload(&t->d_s2e, tab.s2e));
  const hxpw::Program* src[2] = {&tab.to_poly, &tab.to_powerful};
  for (int i = 0; i < 2; i++) {
    CK(upload(&t->prog[i].dims, src[i]->dims));
    CK(upload(&t->prog[i].outer, src[i]->outer));
    CK(upload(&t->prog[i].passes, src[i]->passes));
    t->prog[i].npass = (uint32_t)src[i]->passes.size();
  }
  CK(hipMalloc((void**)&t->scratch, (size_t)hx::PW_MAX_BLOCKS * 3 * tab.m * 8));
  guard.t = nullptr;
  *out = t;
  return HX_OK;
}

extern "C" int hx_poly_to_powerful(const hx_powerful* t, hx_poly* a) { return convert_poly(t, a, 1, "hx_poly_to_powerful"); }
extern "C" int hx_powerful_to_poly(const hx_powerful* t, hx_poly* a) { return convert_poly(t, a, 0, "hx_powerful_to_poly"); }

extern "C" int hx_powerful_words(const hx_powerful* tc, int to_powerful, uint64_t q, const int64_t* in, int batch, int64_t* out)
{
  if (!tc || !in || !out)
    return err(HX_ERR_INVALID, "null argument");
  if (batch < 1)
    return err(HX_ERR_INVALID, "bad batch %d", batch);
  if (q < 2 || q >= hxpw::MAX_Q)
    return err(HX_ERR_INVALID, "the modulus q = %llu is not in [2, 2^62)", (unsigned long long)q);
  hx_powerful* t = const_cast<hx_powerful*>(tc);
  hxi::CtxView v{};
  RC(hxi::ctx_enter(t->ctx, &v));
  std::unique_lock<std::recursive_mutex> lk(*v.mu);
  if (v.capturing)
    return err(HX_ERR_INVALID, "hx_powerful_words waits for the device and cannot be captured in a graph");
  const size_t words = (size_t)batch * t->tab.phim;
  std::vector<uint64_t> h(words);
  for (size_t i = 0; i < words; i++) {   // any int64 is reduced into [0, q)
    const int64_t x = in[i] % (int64_t)q;
    h[i] = (uint64_t)(x < 0 ? x + (int64_t)q : x);
  }
  const hipStream_t st = v.stream;
  if (t->wcap < words) {
    CK(hipStreamSynchronize(st));
    hipFree(t->d_words);
    t->d_words = nullptr;
    t->wcap = 0;
    CK(hipMalloc((void**)&t->d_words, words * 8));
    t->wcap = words;
  }
  DrainOnExit drain{st};
  CK(hipMemcpyAsync(t->d_words, h.data(), words * 8, hipMemcpyHostToDevice, st));
  RC(run(t, st, to_powerful, t->d_words, std::vector<uint64_t>(1, q), batch));
  CK(hipMemcpyAsync(out, t->d_words, words * 8, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return HX_OK;
}
