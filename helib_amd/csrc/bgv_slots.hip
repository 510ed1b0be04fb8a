// bgv_slots.hip -- C ABI of BGV slot encoding and decoding (include/helib_amd.h: hx_bgv_slots_create, hx_bgv_encode,
// hx_bgv_decode, hx_bgv_embed): EncryptedArray over PAlgebraMod (src/EncryptedArray.cpp, src/PAlgebra.cpp:680-772) for
// the case d = ord_m(p) = 1, r = 1, where a slot is an element of Z_p and everything PAlgebraMod computes has a closed
// form:
//   factors of Phi_m mod p   X - a, a the primitive m-th roots of unity mod p; factor 0 is the smallest by poly_comp
//                            (constant coefficient p - a first): F_0 = X - rho, rho the LARGEST primitive m-th root
//   factor i                 F_i = X - rho^(1/t_i mod m), t_i = ith_rep(i) of Z_m^* (/ <p> = {1})
//   encode                   the H of degree < phi(m) with H(rho^(1/t_i)) = a_i mod p, balanced
//   decode                   slot i = H(rho^(1/t_i)) mod p
// The engine's transform for the prime p evaluates at zeta^j, j in Z_m^* ascending (zeta = the engine's root for a
// power-of-two m, its square otherwise).  With rho = zeta^k, slot i sits at the row position of k / t_i mod m: one
// permutation table and its inverse, built here on the host.  p lives in a side context of its own, so the chain
// primes of the caller's context keep their numbering.  Kernels: bgv_slots.h.  The unit reaches the contexts only
// through ckks_bridge.h and the C ABI.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "bgv_encode.h"

struct hx_bgv_slots : hxb::SlotBase {
  uint64_t rho = 0, k = 0;
  std::vector<uint64_t> gens, ords;
  uint32_t* d_row2slot = nullptr;
  uint32_t* d_slot2row = nullptr;
};

using namespace hxb;

namespace {

// findGenerators (src/NumbTh.cpp:276-430) for the quotient of Z_m^* by the trivial group (p = 1 mod m): the next
// generator is an element of largest order in the running quotient, the smallest one whose order there is its order
// in Z_m^* if there is one.  m < 2^24, so products fit 64 bits.
void conj_classes(std::vector<uint32_t>& cl, uint64_t g, uint64_t m)
{
  for (uint64_t i = 0; i < m; i++) {
    if (cl[i] == 0)
      continue;
    if (cl[i] < i) {
      cl[i] = cl[cl[i]];
      continue;
    }
    for (uint64_t j = i * g % m; cl[j] != i; j = j * g % m)
      cl[cl[j]] = (uint32_t)i;
  }
}
void find_generators(uint64_t m, std::vector<uint64_t>& gens, std::vector<uint64_t>& ords)
{
  std::vector<uint32_t> cl(m), order(m);
  for (uint64_t i = 0; i < m; i++)
    cl[i] = hxh::gcd(i, m) == 1 ? (uint32_t)i : 0;
  conj_classes(cl, 1, m);
  for (;;) {
    std::fill(order.begin(), order.end(), 0u);
    if (m > 1)
      order[1] = 1;
    uint32_t largest = 1;
    for (uint64_t i = 2; i < m; i++) {
      if (cl[i] <= 1) {
        order[i] = cl[i] == 1 ? 1 : 0;
        continue;
      }
      if (cl[i] < i) {
        order[i] = order[cl[i]];
        continue;
      }
      uint32_t o = 2;
      for (uint64_t j = i * i % m; cl[j] != 1; j = j * i % m)
        o++;
      order[i] = o;
      largest = std::max(largest, o);
    }
    if (largest <= 1)
      break;
    uint64_t best = 0;
    for (uint64_t i = 0; i < m; i++)
      if (order[i] == largest && hxh::powmod(i, largest, m) == 1) {   // "quality 2"; the power of any other
        best = i;                                                      // candidate would have to lie in <p> = {1}
        break;
      }
    if (!best)
      break;
    gens.push_back(best);
    ords.push_back(largest);
    conj_classes(cl, best, m);
  }
}

// rows (side poly, evaluation form modulo p, row order) -> slot order -> host
int gather_out(hx_bgv_slots* t, hipStream_t st, hx_poly* sp, size_t words, int64_t* slots_out)
{
  RC(ensure_buf(t, st, 2, words * 8));
  HX_LAUNCH(hx::bgv_gather_kernel, dim3(blocks_for(words)), dim3(256), 0, st, hxi::poly_rows_read(sp), t->d_slot2row, t->N,
            words, (int64_t*)t->buf[2]);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(slots_out, t->buf[2], words * 8, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  return HX_OK;
}

}  // namespace

extern "C" int hx_bgv_slots_destroy(hx_bgv_slots* t)
{
  if (!t)
    return HX_OK;
  (void)hipSetDevice(t->device);
  if (t->side)
    hx_ctx_destroy(t->side);   // waits for the device
  hipFree(t->d_row2slot);
  hipFree(t->d_slot2row);
  for (void* b : t->buf)
    hipFree(b);
  delete t;
  return HX_OK;
}

extern "C" int hx_bgv_slots_create(hx_ctx* ctx, uint64_t p, hx_bgv_slots** out)
{
  if (!ctx || !out)
    return err(HX_ERR_INVALID, "null argument");
  *out = nullptr;
  hxi::CtxView v{};
  RC(hxi::ctx_enter(ctx, &v));
  std::unique_lock<std::recursive_mutex> lk(*v.mu);
  if (v.capturing)
    return err(HX_ERR_INVALID, "hx_bgv_slots_create while a graph is being captured");
  const uint64_t m = v.m;
  if (p < 2 || p >= (1ull << 60) || !hxh::is_prime(p))
    return err(HX_ERR_INVALID, "the plaintext modulus p = %llu is not a prime below 2^60", (unsigned long long)p);
  if (m % p == 0)
    return err(HX_ERR_INVALID, "p = %llu divides m = %llu", (unsigned long long)p, (unsigned long long)m);
  if (p % m != 1) {
    uint64_t d = 1;
    for (uint64_t x = p % m; x != 1; x = x * (p % m) % m)
      d++;
    return err(HX_ERR_UNSUPPORTED,
               "d = ord_m(p) = %llu for p = %llu, m = %llu: only d = 1 (p = 1 mod m, slots in Z_p) is built",
               (unsigned long long)d, (unsigned long long)p, (unsigned long long)m);
  }
  const bool pow2 = (m & (m - 1)) == 0;
  if (pow2 ? (m < 16 || m > (1u << 17)) : (m < 3))
    return err(HX_ERR_UNSUPPORTED, "BGV slots on the device need a power-of-two m in [16, 2^17] or another m >= 3 (m = %llu)",
               (unsigned long long)m);
  if (!pow2 && m % 2 == 0 && (p - 1) % (2 * m) != 0)
    return err(HX_ERR_UNSUPPORTED, "even m = %llu that is not a power of two needs 2m | p - 1 (p = %llu)",
               (unsigned long long)m, (unsigned long long)p);
  hx_bgv_slots* t = new hx_bgv_slots();
  struct Guard {
    hx_bgv_slots* t;
    ~Guard() { hx_bgv_slots_destroy(t); }
  } guard{t};
  t->ctx = ctx;
  t->m = m;
  t->p = p;
  t->N = v.phim;
  t->device = v.device;
  RC(hx_ctx_create(&t->side, v.device, m));
  RC(hx_ctx_set_stream(t->side, (void*)v.stream));
  int pidx = -1;
  uint64_t root = 0;
  RC(hx_ctx_add_prime(t->side, p, 0, &pidx));
  RC(hx_ctx_prime(t->side, pidx, nullptr, &root));
  // the evaluation points of the engine's rows: zeta^j, j in Z_m^* ascending
  const uint64_t zeta = pow2 ? root : hxh::mulmod(root, root, p);
  std::vector<uint32_t> zidx(m, hx::BGV_NO_SLOT);
  uint32_t n = 0;
  uint64_t pw = 1;
  for (uint64_t j = 0; j < m; j++, pw = hxh::mulmod(pw, zeta, p))
    if (hxh::gcd(j, m) == 1) {
      zidx[j] = n++;
      if (pw > t->rho) {   // the largest primitive m-th root: the factor X - rho is the smallest by poly_comp
        t->rho = pw;
        t->k = j;
      }
    }
  if (n != t->N || hxh::powmod(zeta, m, p) != 1)
    return err(HX_ERR_DEVICE, "internal: the transform's root for p = %llu is not an m-th root of unity", (unsigned long long)p);
  find_generators(m, t->gens, t->ords);
  uint64_t nslots = 1;
  for (uint64_t o : t->ords)
    nslots *= o;
  if (nslots != t->N)
    return err(HX_ERR_DEVICE, "internal: the hypercube of Z_%llu^* has %llu points, not phi(m)", (unsigned long long)m,
               (unsigned long long)nslots);
  // slot i: exponent vector of i over gens, the last generator's exponent fastest (ith_rep)
  std::vector<uint32_t> slot2row(t->N), row2slot(t->N, hx::BGV_NO_SLOT);
  const size_t ng = t->gens.size();
  std::vector<uint64_t> e(ng, 0), part(ng + 1, 1);   // part[g] = prod_(g' < g) gens^e
  for (uint32_t i = 0; i < t->N; i++) {
    const uint64_t ti = part[ng];
    const uint64_t pos = hxh::mulmod(t->k, hxh::invmod(ti, m), m);
    const uint32_t r = zidx[pos];
    if (r == hx::BGV_NO_SLOT || row2slot[r] != hx::BGV_NO_SLOT)
      return err(HX_ERR_DEVICE, "internal: slot table collision at m = %llu", (unsigned long long)m);
    slot2row[i] = r;
    row2slot[r] = i;
    // next exponent vector
    size_t g = ng;
    while (g-- > 0) {
      if (++e[g] < t->ords[g])
        break;
      e[g] = 0;
    }
    if (g == (size_t)-1)
      break;
    for (size_t h = g; h < ng; h++)
      part[h + 1] = hxh::mulmod(part[h], hxh::powmod(t->gens[h], e[h], m), m);
  }
  CK(hipMalloc((void**)&t->d_row2slot, sizeof(uint32_t) * t->N));
  CK(hipMalloc((void**)&t->d_slot2row, sizeof(uint32_t) * t->N));
  CK(hipMemcpy(t->d_row2slot, row2slot.data(), sizeof(uint32_t) * t->N, hipMemcpyHostToDevice));
  CK(hipMemcpy(t->d_slot2row, slot2row.data(), sizeof(uint32_t) * t->N, hipMemcpyHostToDevice));
  guard.t = nullptr;
  *out = t;
  return HX_OK;
}

extern "C" int hx_bgv_slots_info(const hx_bgv_slots* t, uint64_t* p, uint64_t* rho, int* ndims, uint64_t* gens, uint64_t* ords)
{
  if (!t)
    return err(HX_ERR_INVALID, "null argument");
  if (p)
    *p = t->p;
  if (rho)
    *rho = t->rho;
  if (ndims)
    *ndims = (int)t->gens.size();
  for (size_t i = 0; i < t->gens.size() && i < 8; i++) {
    if (gens)
      gens[i] = t->gens[i];
    if (ords)
      ords[i] = t->ords[i];
  }
  return HX_OK;
}


extern "C" int hx_bgv_encode(const hx_bgv_slots* tc, const int64_t* slots, int batch, int nslots, uint64_t mul, hx_poly* out,
                             int64_t* coeffs_out)
{
  if (!tc || !out || (nslots > 0 && !slots))
    return err(HX_ERR_INVALID, "null argument");
  hx_bgv_slots* t = const_cast<hx_bgv_slots*>(tc);   // (its scratch buffers grow; the caller's lock covers them)
  if (hxi::poly_ctx(out) != t->ctx)
    return err(HX_ERR_INVALID, "the output poly belongs to another context than the slot table");
  const uint32_t N = t->N;
  if (batch < 1 || nslots < 0 || (uint32_t)nslots > N)
    return err(HX_ERR_INVALID, "bad batch / slot count (batch %d, %d slots of at most %u)", batch, nslots, N);
  Encode e{t, out, batch};
  RC(e.check());
  uint64_t* h;
  RC(e.open("hx_bgv_encode", coeffs_out != nullptr, &h));
  const hipStream_t st = e.st;
  const uint64_t p = t->p;
  const size_t vbytes = (size_t)batch * nslots * 8;
  RC(ensure_buf(t, st, 0, std::max<size_t>(vbytes, 16)));
  if (vbytes)
    CK(hipMemcpyAsync(t->buf[0], slots, vbytes, hipMemcpyHostToDevice, st));
  HX_LAUNCH(hx::bgv_scatter_kernel, dim3(blocks_for(e.words)), dim3(256), 0, st, (const int64_t*)t->buf[0], (uint32_t)nslots,
            t->d_row2slot, N, e.words, p, (uint64_t)(((hxh::u128)1 << 64) / p), h);
  CK(hipGetLastError());
  return e.finish(mul % p, coeffs_out);
}

// ---- diagonals of a device-resident matrix (MatMul1DExec / MatMulFullExec construction, src/matmul.cpp) ----
static_assert(sizeof(hx::BgvDiag) == sizeof(hx_bgv_diag) && sizeof(hx_bgv_diag) == 40, "hx_bgv_diag layout");
struct hx_bgv_matrix {
  const hx_bgv_slots* table = nullptr;
  int64_t* d = nullptr;     // rows x cols words as given; the gather reduces mod p
  hx::BgvDiagGeom g{};
};

extern "C" int hx_bgv_matrix_destroy(hx_bgv_matrix* a)
{
  if (!a)
    return HX_OK;
  if (a->table)
    (void)hipSetDevice(a->table->device);
  hipFree(a->d);
  delete a;
  return HX_OK;
}

extern "C" int hx_bgv_matrix_create(const hx_bgv_slots* t, const int64_t* a_host, int rows, int cols, int dim, hx_bgv_matrix** out)
{
  if (!t || !a_host || !out)
    return err(HX_ERR_INVALID, "null argument");
  *out = nullptr;
  const int nd = (int)t->gens.size();
  if (nd > 8)
    return err(HX_ERR_UNSUPPORTED, "more than 8 generators");
  if (dim < -1 || dim >= nd)
    return err(HX_ERR_INVALID, "dim = %d is neither -1 (a full matrix) nor a dimension of the hypercube (%d)", dim, nd);
  const uint64_t D = dim < 0 ? t->N : t->ords[dim];
  if (rows < 1 || (uint64_t)rows != D || (uint64_t)cols != D)
    return err(HX_ERR_INVALID, "a %d x %d matrix where dim = %d takes %llu x %llu", rows, cols, dim, (unsigned long long)D,
               (unsigned long long)D);
  Enter E;
  RC(E.open(t, "hx_bgv_matrix_create"));
  hx_bgv_matrix* a = new hx_bgv_matrix();
  struct Guard {
    hx_bgv_matrix* a;
    ~Guard() { hx_bgv_matrix_destroy(a); }
  } guard{a};
  a->table = t;
  a->g.nd = nd;
  a->g.dim = dim;
  a->g.cols = (uint32_t)cols;
  uint64_t stride = 1;
  for (int i = nd - 1; i >= 0; i--) {
    a->g.ord[i] = (uint32_t)t->ords[i];
    a->g.stride[i] = (uint32_t)stride;
    stride *= t->ords[i];
  }
  const size_t bytes = (size_t)rows * (size_t)cols * 8;
  CK(hipMalloc((void**)&a->d, bytes));
  CK(hipMemcpyAsync(a->d, a_host, bytes, hipMemcpyHostToDevice, E.v.stream));
  CK(hipStreamSynchronize(E.v.stream));
  guard.a = nullptr;
  *out = a;
  return HX_OK;
}

extern "C" int hx_bgv_encode_diagonals(const hx_bgv_slots* tc, const hx_bgv_matrix* a, const hx_bgv_diag* d, int ndiag,
                                       hx_poly* out, int64_t* coeffs_out, int* nonzero_out)
{
  if (!tc || !a || !d || !nonzero_out)
    return err(HX_ERR_INVALID, "null argument");
  hx_bgv_slots* t = const_cast<hx_bgv_slots*>(tc);
  if (a->table != tc)
    return err(HX_ERR_INVALID, "the matrix belongs to another slot table");
  if (ndiag < 1)
    return err(HX_ERR_INVALID, "bad number of diagonals %d", ndiag);
  if (!out && coeffs_out)
    return err(HX_ERR_INVALID, "coefficients without an output poly: pass a poly on no primes");
  const hx::BgvDiagGeom& g = a->g;
  std::vector<hx::BgvDiag> dd(ndiag);
  for (int k = 0; k < ndiag; k++) {
    const int rd = d[k].rot_dim;
    if (rd < -1 || rd >= g.nd)
      return err(HX_ERR_INVALID, "diagonal %d: rot_dim = %d is neither -1 nor a dimension of the hypercube (%d)", k, rd, g.nd);
    for (int i = 0; i < 8; i++) {
      const int64_t o = i < g.nd ? (int64_t)g.ord[i] : 1;
      dd[k].off[i] = (int32_t)((((int64_t)d[k].off[i] % o) + o) % o);
    }
    const int64_t o = rd >= 0 ? (int64_t)g.ord[rd] : 1;
    dd[k].rot_dim = rd;
    dd[k].rot_amt = (int32_t)((((int64_t)d[k].rot_amt % o) + o) % o);
  }
  std::vector<uint32_t> nz(ndiag);   // (outlives e, whose destructor waits for the copies)
  Encode e{t, out, ndiag};
  RC(e.check());
  const uint32_t N = t->N;
  const uint64_t p = t->p, mu = (uint64_t)(((hxh::u128)1 << 64) / p);
  const size_t dbytes = (sizeof(hx::BgvDiag) * (size_t)ndiag + 15) / 16 * 16, fbytes = sizeof(uint32_t) * (size_t)ndiag;
  uint64_t* h = nullptr;
  if (out) {
    RC(e.open("hx_bgv_encode_diagonals", coeffs_out != nullptr, &h));
  } else {   // the flags alone: no transform, no scratch rows
    RC(e.E.open(t, "hx_bgv_encode_diagonals"));
    e.st = e.E.v.stream;
    e.words = (size_t)ndiag * N;
  }
  const hipStream_t st = e.st;
  RC(ensure_buf(t, st, 0, dbytes + fbytes));
  uint32_t* d_nz = (uint32_t*)((char*)t->buf[0] + dbytes);
  CK(hipMemcpyAsync(t->buf[0], dd.data(), sizeof(hx::BgvDiag) * (size_t)ndiag, hipMemcpyHostToDevice, st));
  CK(hipMemsetAsync(d_nz, 0, fbytes, st));
  HX_LAUNCH(hx::bgv_diag_scatter_kernel, dim3(blocks_for(e.words)), dim3(256), 0, st, (const int64_t*)a->d, g,
            (const hx::BgvDiag*)t->buf[0], t->d_row2slot, N, e.words, p, mu, h, d_nz);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(nz.data(), d_nz, fbytes, hipMemcpyDeviceToHost, st));
  if (out)
    RC(e.finish(1, coeffs_out));
  else
    CK(hipStreamSynchronize(st));
  for (int k = 0; k < ndiag; k++)
    nonzero_out[k] = nz[k] ? 1 : 0;
  return HX_OK;
}

extern "C" int hx_bgv_embed(const hx_bgv_slots* tc, const int64_t* coeffs, int batch, int64_t* slots_out)
{
  if (!tc || !coeffs || !slots_out)
    return err(HX_ERR_INVALID, "null argument");
  if (batch < 1)
    return err(HX_ERR_INVALID, "bad batch %d", batch);
  hx_bgv_slots* t = const_cast<hx_bgv_slots*>(tc);
  Enter E;
  RC(E.open(t, "hx_bgv_embed"));
  const hipStream_t st = E.v.stream;
  hx_poly* sp = nullptr;
  RC(side_poly(t, batch, &sp));
  Drop drop{sp};
  DrainOnExit drain{st};
  const size_t words = (size_t)batch * t->N;
  RC(ensure_buf(t, st, 0, words * 8));
  CK(hipMemcpyAsync(t->buf[0], coeffs, words * 8, hipMemcpyHostToDevice, st));
  uint64_t* h;
  RC(hxi::poly_rows_write(sp, &h));
  RC(launch_redmul(t, st, (const int64_t*)t->buf[0], words, 1, h));
  RC(hx_ntt_forward(sp));
  return gather_out(t, st, sp, words, slots_out);
}

extern "C" int hx_bgv_decode(const hx_bgv_slots* tc, const hx_poly* acc, uint64_t factor_inv, int64_t* slots_out)
{
  if (!tc || !acc || !slots_out)
    return err(HX_ERR_INVALID, "null argument");
  hx_bgv_slots* t = const_cast<hx_bgv_slots*>(tc);
  if (hxi::poly_ctx(acc) != t->ctx)
    return err(HX_ERR_INVALID, "the poly belongs to another context than the slot table");
  Enter E;
  RC(E.open(t, "hx_bgv_decode"));
  int batch = 0, n = 0;
  RC(hx_poly_shape(acc, &batch, &n, nullptr));
  const size_t words = (size_t)batch * t->N;
  if (n == 0) {   // the zero polynomial
    memset(slots_out, 0, words * 8);
    return HX_OK;
  }
  const hipStream_t st = E.v.stream;
  hx_poly* sp = nullptr;
  RC(side_poly(t, batch, &sp));
  Drop drop{sp};
  DrainOnExit drain{st};
  const uint64_t* d_rem;
  RC(hxi::poly_rem_device(acc, t->p, &d_rem));   // toPoly + PolyRed(p), exact, in [0, p)
  uint64_t* h;
  RC(hxi::poly_rows_write(sp, &h));
  RC(launch_redmul(t, st, (const int64_t*)d_rem, words, factor_inv % t->p, h));
  RC(hx_ntt_forward(sp));
  return gather_out(t, st, sp, words, slots_out);
}
