// norm_direct_replay.cpp -- CPU replay of the pairing-free radix-16 norm (helib_amd/csrc/norm_r16.h, "the direct
// form") thread by thread with the barriers where the kernels have them: the load twist, passes A / B / C, the two
// transposes through the one padded array, the last stage as a lane exchange, and the per-thread maxima -- as
// embed_norm_r16_kernel runs them from memory and as the mod-switch prep kernels run them from the registers their
// inverse transform ends in (ntt_kernels.hip: PrepFuseIO).  Checked against the definition
//   max_j | f(W^(2j+1)) |,  j < N,  W = exp(2 pi i / 2N),  N = 16384
// in long double over ALL N evaluation points, and output by output (Z at position p is f(W^(4 brev13(p) + 1)));
// and the claim the fused kernels rest on -- the inverse row transform leaves coefficient tid + 512 e in register e
// of thread tid -- is checked by replaying that transform (helib_amd/csrc/ntt_core.h) into a store-all functor.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../helib_amd/csrc/norm_r16.h"
#include "../../helib_amd/csrc/ntt_core.h"

using namespace hx;

static const long double NORM_RTOL = 1e-9L;   // the project's tolerance for device norms

template <class FROM, class TO>
static void transpose(std::vector<cplx16>& regs, std::vector<double>& sm, FROM from, TO to)
{
  const unsigned T = R16_THREADS;
  for (int comp = 0; comp < 2; comp++) {
    for (unsigned t = 0; t < T; t++)
      for (unsigned k = 0; k < 16; k++)
        sm[r16_pad(from(t, k))] = comp ? regs[(size_t)t * 16 + k].y : regs[(size_t)t * 16 + k].x;
    for (unsigned t = 0; t < T; t++)
      for (unsigned k = 0; k < 16; k++)
        (comp ? regs[(size_t)t * 16 + k].y : regs[(size_t)t * 16 + k].x) = sm[r16_pad(to(t, k))];
  }
}
// file[t * 32 + e]: what thread t holds in register e when the form starts (coefficient t + 512 e).
// Returns the norm; Z[p] = the finished output at transform position p.
static double replay(const std::vector<double>& file, const std::vector<tw16>& wtab, std::vector<cplx16>& Z)
{
  const unsigned T = R16_THREADS;
  std::vector<double> sm(R16_LDS_DOUBLES, 0.0);
  std::vector<cplx16> regs((size_t)T * 16);
  for (unsigned t = 0; t < T; t++) {
    cplx16 v[16];
    const tw16 wth = wtab[t];
    for (unsigned k = 0; k < 16; k++)
      v[k] = r16_direct_twist(file[(size_t)t * 32 + k], file[(size_t)t * 32 + k + 16], wth, wtab[r16_direct_tw_k(k)], k);
    r16_pass<9>(v, t, wtab.data());
    for (unsigned k = 0; k < 16; k++)
      regs[(size_t)t * 16 + k] = v[k];
  }
  transpose(regs, sm, r16_pos_A, r16_pos_B);
  for (unsigned t = 0; t < T; t++) {
    cplx16 v[16];
    for (unsigned k = 0; k < 16; k++)
      v[k] = regs[(size_t)t * 16 + k];
    r16_pass<5>(v, t & 31u, wtab.data());
    for (unsigned k = 0; k < 16; k++)
      regs[(size_t)t * 16 + k] = v[k];
  }
  transpose(regs, sm, r16_pos_B, r16_pos_C);
  for (unsigned t = 0; t < T; t++) {
    cplx16 v[16];
    for (unsigned k = 0; k < 16; k++)
      v[k] = regs[(size_t)t * 16 + k];
    r16_pass<1>(v, t & 1u, wtab.data());
    for (unsigned k = 0; k < 16; k++)
      regs[(size_t)t * 16 + k] = v[k];
  }
  // the lane exchange with t ^ 1, the per-thread maxima, the maximum over the threads
  Z.assign(R16_M, cplx16{0, 0});
  double mx = 0;
  for (unsigned t = 0; t < T; t++) {
    double tmx = 0;
    for (unsigned k = 0; k < 16; k++) {
      const cplx16 z = r16_last_lane(regs[(size_t)t * 16 + k], regs[(size_t)(t ^ 1u) * 16 + k], t);
      Z[r16_pos_C(t, k)] = z;
      const double n2 = r16_abs2(z);
      tmx = n2 > tmx ? n2 : tmx;
    }
    mx = tmx > mx ? tmx : mx;
  }
  return std::sqrt(mx);
}
static std::vector<double> file_of(const std::vector<double>& f)   // as the standalone kernel loads it
{
  std::vector<double> file((size_t)R16_THREADS * 32);
  for (unsigned t = 0; t < R16_THREADS; t++)
    for (unsigned e = 0; e < 32; e++)
      file[(size_t)t * 32 + e] = f[r16_pos_A(t, e & 15u) + (e >> 4) * R16_M];
  return file;
}
static unsigned brev13(unsigned p)
{
  unsigned r = 0;
  for (int i = 0; i < 13; i++)
    r |= ((p >> i) & 1u) << (12 - i);
  return r;
}

static std::vector<long double> g_cos, g_sin;   // W^e, e < 2N
// f(W^(2j+1)) for every j < N
static void evaluate_all(const std::vector<double>& f, std::vector<long double>& re, std::vector<long double>& im)
{
  const unsigned N = R16_N;
  re.assign(N, 0);
  im.assign(N, 0);
  for (unsigned i = 0; i < N; i++) {
    if (f[i] == 0.0)
      continue;
    for (unsigned j = 0; j < N; j++) {
      const unsigned e = (unsigned)(((unsigned long)i * (2ul * j + 1ul)) & (2ul * N - 1ul));
      re[j] += f[i] * g_cos[e];
      im[j] += f[i] * g_sin[e];
    }
  }
}
// the replay of f against the definition; returns the larger of the two relative errors (norm; worst output / norm)
static long double check(const char* what, const std::vector<double>& f, const std::vector<double>& file,
                         const std::vector<tw16>& wtab, bool& ok)
{
  std::vector<long double> re, im;
  evaluate_all(f, re, im);
  long double want = 0;
  for (unsigned j = 0; j < R16_N; j++) {
    const long double v = sqrtl(re[j] * re[j] + im[j] * im[j]);
    want = v > want ? v : want;
  }
  std::vector<cplx16> Z;
  const double got = replay(file, wtab, Z);
  const long double enorm = fabsl((long double)got - want) / want;
  long double eout = 0;
  for (unsigned p = 0; p < R16_M; p++) {
    const unsigned j2 = 2u * brev13(p);   // W^(4j+1) = W^(2 (2j) + 1)
    const long double dx = (long double)Z[p].x - re[j2], dy = (long double)Z[p].y - im[j2];
    const long double d = sqrtl(dx * dx + dy * dy) / want;
    eout = d > eout ? d : eout;
  }
  printf("norm_direct_replay %-22s norm %.17g  rel. error of the norm %.3Lg, of the worst output %.3Lg\n", what, got, enorm,
         eout);
  if (!(enorm <= NORM_RTOL) || !(eout <= NORM_RTOL)) {
    printf("norm_direct_replay FAILED (%s): got %.17g want %.17Lg\n", what, got, want);
    ok = false;
  }
  return enorm > eout ? enorm : eout;
}

// ---- the register file the inverse row transform ends in ----
typedef unsigned __int128 u128;
static uint64_t mm(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)(((u128)a * b) % q); }
static uint64_t pw(uint64_t a, uint64_t e, uint64_t q)
{
  uint64_t r = 1;
  while (e) {
    if (e & 1)
      r = mm(r, a, q);
    a = mm(a, a, q);
    e >>= 1;
  }
  return r;
}
static bool is_prime(uint64_t n)
{
  uint64_t d = n - 1;
  int s = 0;
  while (!(d & 1))
    d >>= 1, s++;
  for (uint64_t a : {2ull, 3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull}) {
    uint64_t x = pw(a % n, d, n);
    if (x == 0 || x == 1 || x == n - 1)
      continue;
    bool comp = true;
    for (int i = 1; i < s && comp; i++) {
      x = mm(x, x, n);
      comp = x != n - 1;
    }
    if (comp)
      return false;
  }
  return true;
}
// the store-all hook of ntt_core.h (io_inv_store_all): records the canonical register file instead of storing
struct RecordIO : PtrIO {
  static constexpr bool INV_STORE_ALL = true;
  uint64_t* file;
  template <int LOGN, class AR>
  void inv_store_all(unsigned tid, uint64_t (&v)[32], uint32_t*, const QC& c) const
  {
    for (int e = 0; e < 32; e++)
      file[(size_t)tid * 32 + e] = norm_from<AR::INV_OUT>(v[e], c);
  }
};
template <int PH, bool INV, class AR, class IO>
static void run_phase(std::vector<uint64_t>& V, std::vector<uint32_t>& NL, std::vector<uint32_t>& lds, const IO& io,
                      const typename AR::Tw* tw, uint64_t q)
{
  using R = RowNTT<14, AR>;
  for (unsigned tid = 0; tid < (unsigned)Geo<14>::T; tid++) {
    uint64_t(&v)[32] = *reinterpret_cast<uint64_t(*)[32]>(&V[(size_t)tid * 32]);
    uint32_t(&nl)[32] = *reinterpret_cast<uint32_t(*)[32]>(&NL[(size_t)tid * 32]);
    if (INV)
      R::template inv<PH>(tid, v, nl, lds.data(), io, tw, make_qc(q));
    else
      R::template fwd<PH>(tid, v, nl, lds.data(), io, tw, make_qc(q));
  }
}
template <bool INV, class AR, class IO>
static void transform(const IO& io, const typename AR::Tw* tw, uint64_t q)
{
  using G = Geo<14>;
  std::vector<uint64_t> V((size_t)G::T * 32);
  std::vector<uint32_t> NL((size_t)G::T * 32), lds(G::LDS_WORDS, 0xdeadbeef);
  run_phase<0, INV, AR>(V, NL, lds, io, tw, q);
  run_phase<1, INV, AR>(V, NL, lds, io, tw, q);
  run_phase<2, INV, AR>(V, NL, lds, io, tw, q);
  run_phase<3, INV, AR>(V, NL, lds, io, tw, q);
  run_phase<4, INV, AR>(V, NL, lds, io, tw, q);
  run_phase<5, INV, AR>(V, NL, lds, io, tw, q);
  run_phase<6, INV, AR>(V, NL, lds, io, tw, q);
  run_phase<7, INV, AR>(V, NL, lds, io, tw, q);
}
// the tables in the arithmetic's own form (Shoup pairs; Proth form: w 2^64 mod q -- as tests/cpp/ntt_replay.cpp)
template <class AR>
static std::vector<typename AR::Tw> table_of(const std::vector<TW>& t, uint64_t q);
template <>
std::vector<TW> table_of<ArShoup>(const std::vector<TW>& t, uint64_t) { return t; }
template <>
std::vector<TWM> table_of<ArProth>(const std::vector<TW>& t, uint64_t q)
{
  std::vector<TWM> o(t.size());
  tw_tables_to_mont(t.data(), (int)t.size(), q, o.data());
  return o;
}
// coefficients x -> (forward transform) -> (inverse transform into a RecordIO) -> the register file
template <class AR>
static bool inverse_register_file(const std::vector<uint64_t>& x, uint64_t q, uint64_t psi, std::vector<uint64_t>& file)
{
  using G = Geo<14>;
  static_assert(G::T == (int)R16_THREADS && G::N == (int)R16_N, "one thread per 32 coefficients");
  static_assert((size_t)G::LDS_WORDS * 4 == (size_t)R16_LDS_DOUBLES * 8, "the norm takes over the transform's array");
  std::vector<TW> f(G::TW_TOTAL), i(G::TW_TOTAL);
  build_tw_tables<14>(q, psi, pw(psi, q - 2, q), pw((uint64_t)G::N % q, q - 2, q), mm, f.data(), i.data());
  const std::vector<typename AR::Tw> ft = table_of<AR>(f, q), it = table_of<AR>(i, q);
  std::vector<uint64_t> row(G::N), back(G::N);
  PtrIO fio{x.data(), row.data()};
  transform<false, AR>(fio, ft.data(), q);
  file.assign((size_t)G::T * 32, ~0ull);
  RecordIO rio{{row.data(), back.data()}, file.data()};
  transform<true, AR>(rio, it.data(), q);
  for (unsigned tid = 0; tid < (unsigned)G::T; tid++)
    for (int e = 0; e < 32; e++) {
      if (coef_const<14>(e) != 512u * (unsigned)e)
        return false;
      if (file[(size_t)tid * 32 + e] != x[tid + 512u * (unsigned)e])
        return false;
    }
  return true;
}
// the replayed register file of a dropped row with chosen coefficients, and the norm of the centred x / qd from it
template <class AR>
static void check_from_inverse(const char* what, uint64_t q, unsigned long long seed, const std::vector<tw16>& wtab, bool& ok)
{
  const unsigned N = R16_N;
  uint64_t psi = 0;
  for (uint64_t g = 2; !psi; g++) {
    const uint64_t c = pw(g, (q - 1) / (2ull * N), q);
    if (pw(c, N, q) == q - 1)
      psi = c;
  }
  unsigned long long s = seed;
  std::vector<uint64_t> x(N), file;
  for (auto& v : x)
    v = (s = s * 6364136223846793005ull + 1442695040888963407ull) % q;
  x[0] = 0, x[511] = 1, x[512] = (q - 1) / 2, x[8191] = (q - 1) / 2 + 1, x[8192] = q - 1, x[16383] = (q - 1) / 2;
  if (!inverse_register_file<AR>(x, q, psi, file)) {
    printf("norm_direct_replay FAILED (%s): register e of thread tid is not coefficient tid + 512 e\n", what);
    ok = false;
    return;
  }
  printf("norm_direct_replay inverse row transform (%s): register e of thread tid = coefficient tid + 512 e\n", what);
  const double inv_qd = 1.0 / (double)q;
  std::vector<double> f(N), dfile(file.size());
  for (unsigned i = 0; i < N; i++)
    f[i] = (double)x[i] * inv_qd - (x[i] > (q - 1) / 2 ? 1.0 : 0.0);
  for (size_t i = 0; i < file.size(); i++)
    dfile[i] = (double)file[i] * inv_qd - (file[i] > (q - 1) / 2 ? 1.0 : 0.0);
  check(what, f, dfile, wtab, ok);
}

int main()
{
  const unsigned N = R16_N, M = R16_M;
  const long double two_pi = 6.283185307179586476925286766559005768394L;
  std::vector<tw16> wtab(N);
  for (unsigned k = 0; k < N; k++) {
    const long double ang = two_pi * (long double)k / (long double)(2 * N);
    wtab[k] = {(double)cosl(ang), (double)sinl(ang)};
  }
  g_cos.resize(2 * N);
  g_sin.resize(2 * N);
  for (unsigned e = 0; e < 2 * N; e++) {
    g_cos[e] = cosl(two_pi * (long double)e / (long double)(2 * N));
    g_sin[e] = sinl(two_pi * (long double)e / (long double)(2 * N));
  }
  unsigned long long s = 12345;
  auto next = [&]() { return s = s * 6364136223846793005ull + 1442695040888963407ull; };
  bool ok = true;
  // single monomials: a wrong pairing of e and e + 16 or a wrong twist exponent moves every output
  for (unsigned p : {0u, 1u, M - 1u, M, N - 1u}) {
    std::vector<double> f(N, 0.0);
    f[p] = 3.0;
    char what[32];
    snprintf(what, sizeof what, "monomial at %u", p);
    check(what, f, file_of(f), wtab, ok);
  }
  // dense random coefficients
  {
    std::vector<double> f(N);
    for (auto& v : f)
      v = (double)(long long)(next() >> 11) / 9007199254740992.0 - 0.5;
    check("dense", f, file_of(f), wtab, ok);
  }
  // the fused kernels' input: a dropped row's inverse transform ends with coefficient tid + 512 e in register e of
  // thread tid; d = x / qd - [x > (qd - 1) / 2] from those registers gives the norm of the centred x / qd.  In both
  // arithmetics of the row kernels: Shoup pairs, and the Proth form every prime of the benchmark chains takes.
  {
    uint64_t q = ((uint64_t)1 << 59) + 1;
    while (!is_prime(q))
      q += 2ull * N;   // q = 1 mod 2N
    check_from_inverse<ArShoup>("inverse's file, Shoup", q, 777, wtab, ok);
    uint64_t qp = ((uint64_t)1 << 59) + 1;
    while (!is_prime(qp))
      qp += (uint64_t)1 << 32;   // q = 1 mod 2^32
    check_from_inverse<ArProth>("inverse's file, Proth", qp, 778, wtab, ok);
  }
  if (!ok)
    return 1;
  printf("norm_direct_replay OK\n");
  return 0;
}
