// CPU replay of the fused key switch's store loop on rows of Proth-form primes (helib_amd/csrc/ks_proth.h, called as
// KsLastIO::store_rows of ntt_kernels.hip calls it: same slot order, same masks, same constants), built with
// HX_CHECK_BOUNDS so that every bound the static_asserts of KsProth state is also checked on the values.
// TEST INFRASTRUCTURE: built by tests/, never linked into the product library.
#include <cstdint>
#include <vector>

#include "../../helib_amd/csrc/ks_proth.h"

typedef unsigned __int128 u128;

// the D products of both sums, digit words in key order (each at its own compile-time bound)
template <class KP, int S, int ND>
static void term_all(const uint64_t (&x)[ND], const int (&kd)[ND], const uint64_t* kb, const uint64_t* ka, int n, int i,
                     uint64_t r2, const hx::QC& qc, uint64_t& s0, uint64_t& s1)
{
  if constexpr (S < ND) {
    s0 = KP::template term<S>(x[S], hx::ksp_to_mont(kb[(size_t)kd[S] * n + i], r2, qc), s0, qc);
    s1 = KP::template term<S>(x[S], hx::ksp_to_mont(ka[(size_t)kd[S] * n + i], r2, qc), s1, qc);
    term_all<KP, S + 1, ND>(x, kd, kb, ka, n, i, r2, qc, s0, s1);
  }
}

// One row, n coefficients.  Digit-indexed inputs: dig[d][n] the canonical digit words (the owner's entry is ignored: it
// is rebuilt), vf[n] the fused digit's word as the transform leaves it (dig[fd] + j q below B q), kb / ka[d][n] the
// canonical key words, pinv[e] = P_e^-1 mod q, ps = the parts' scale factor or 0 when they stand scaled, acc1 null: no
// (s) part.  owner < 0: a special-prime row.
template <int LOGN, int ND, bool OWNED>
static int run(int owner, uint64_t q, int n, const uint64_t* dig, const uint64_t* vf, const uint64_t* own_src,
               const uint64_t* acc0, const uint64_t* acc1, const uint64_t* kb, const uint64_t* ka, const uint64_t* pinv,
               uint64_t ps, uint64_t* o0, uint64_t* o1)
{
  constexpr int B = hx::RowNTT<LOGN, hx::ArProth>::template fwd_store_bound<2>();
  using KP = hx::KsProth<ND, OWNED, B>;
  constexpr int NMEM = KP::NMEM;
  const hx::QC qc = hx::make_qc(q);
  const uint64_t r2 = hx::tw_mont_form(hx::tw_mont_form(1, q), q), one = hx::tw_mont_form(1, q);
  typename KP::Consts kc;
  for (int e = 0; e < ND - 1; e++)
    kc.pinv[e] = (OWNED && e < owner) ? hx::tw_mont_form(pinv[e], q) : one;
  kc.ps0 = ps ? hx::tw_mont_form(ps, q) : one;
  kc.ps1 = acc1 ? kc.ps0 : 0;
  kc.xoff = KP::xoff(qc);
  const int fd = (OWNED && owner == ND - 1) ? ND - 2 : ND - 1;
  int kd[ND];   // digit of: the memory slots, the fused digit, the owner
  for (int s = 0; s < NMEM; s++)
    kd[s] = (OWNED && s >= owner) ? s + 1 : s;
  kd[NMEM] = fd;
  if (OWNED)
    kd[NMEM + 1] = owner;
  auto masked = [](uint64_t x, bool m) { return m ? x : (uint64_t)0; };
  for (int i = 0; i < n; i++) {
    const uint64_t xf = KP::fused_word(vf[i], qc);
    uint64_t x[ND];
    for (int s = 0; s < NMEM; s++)
      x[s] = dig[(size_t)kd[s] * n + i];
    x[NMEM] = xf;
    uint64_t s0 = 0, s1 = 0;
    if constexpr (OWNED) {
      uint64_t own = own_src[i];
      for (int s = 0; s < NMEM; s++)
        own = KP::rebuild_mem(own, masked(x[s], s < owner), kc.pinv[s], qc);
      x[NMEM + 1] = KP::rebuild_last(own, masked(xf, owner == ND - 1), kc, qc);
      s0 = KP::part(acc0[i], kc.ps0, qc);
      s1 = KP::part(acc1 ? acc1[i] : acc0[i], kc.ps1, qc);
    }
    term_all<KP, 0, ND>(x, kd, kb, ka, n, i, r2, qc, s0, s1);
    o0[i] = KP::reduce(s0, qc);
    o1[i] = KP::reduce(s1, qc);
  }
  return 0;
}

template <int LOGN, int ND>
static int run_nd(int owner, uint64_t q, int n, const uint64_t* dig, const uint64_t* vf, const uint64_t* own_src,
                  const uint64_t* acc0, const uint64_t* acc1, const uint64_t* kb, const uint64_t* ka, const uint64_t* pinv,
                  uint64_t ps, uint64_t* o0, uint64_t* o1)
{
  if (owner >= ND)
    return -3;
  if (owner >= 0)
    return run<LOGN, ND, true>(owner, q, n, dig, vf, own_src, acc0, acc1, kb, ka, pinv, ps, o0, o1);
  return run<LOGN, ND, false>(owner, q, n, dig, vf, own_src, acc0, acc1, kb, ka, pinv, ps, o0, o1);
}
template <int LOGN>
static int run_logn(int nd, int owner, uint64_t q, int n, const uint64_t* dig, const uint64_t* vf, const uint64_t* own_src,
                    const uint64_t* acc0, const uint64_t* acc1, const uint64_t* kb, const uint64_t* ka, const uint64_t* pinv,
                    uint64_t ps, uint64_t* o0, uint64_t* o1)
{
  switch (nd) {
    case 2: return run_nd<LOGN, 2>(owner, q, n, dig, vf, own_src, acc0, acc1, kb, ka, pinv, ps, o0, o1);
    case 3: return run_nd<LOGN, 3>(owner, q, n, dig, vf, own_src, acc0, acc1, kb, ka, pinv, ps, o0, o1);
    case 4: return run_nd<LOGN, 4>(owner, q, n, dig, vf, own_src, acc0, acc1, kb, ka, pinv, ps, o0, o1);
  }
  return -1;
}

extern "C" {
// -2: not a Proth-form prime; -1 / -3: bad shape
int ks_proth_store_replay(int logn, int nd, int owner, uint64_t q, int n, const uint64_t* dig, const uint64_t* vf,
                          const uint64_t* own_src, const uint64_t* acc0, const uint64_t* acc1, const uint64_t* kb,
                          const uint64_t* ka, const uint64_t* pinv, uint64_t ps, uint64_t* o0, uint64_t* o1)
{
  if (!hx::is_proth32(q))
    return -2;
  switch (logn) {
    case 13: return run_logn<13>(nd, owner, q, n, dig, vf, own_src, acc0, acc1, kb, ka, pinv, ps, o0, o1);
    case 14: return run_logn<14>(nd, owner, q, n, dig, vf, own_src, acc0, acc1, kb, ka, pinv, ps, o0, o1);
    case 15: return run_logn<15>(nd, owner, q, n, dig, vf, own_src, acc0, acc1, kb, ka, pinv, ps, o0, o1);
  }
  return -1;
}
// the bound, in whole q, of the fused digit's word at ring size 2^logn (what the largest lazy test input is made from)
int ks_proth_fused_bound(int logn)
{
  switch (logn) {
    case 13: return hx::RowNTT<13, hx::ArProth>::fwd_store_bound<2>();
    case 14: return hx::RowNTT<14, hx::ArProth>::fwd_store_bound<2>();
    case 15: return hx::RowNTT<15, hx::ArProth>::fwd_store_bound<2>();
  }
  return -1;
}
// the key conversion of engine.hip ksk_mont_kernel: out = k 2^64 mod q
int ks_proth_key_to_mont(uint64_t q, int n, const uint64_t* k, uint64_t* out)
{
  if (!hx::is_proth32(q))
    return -2;
  const hx::QC qc = hx::make_qc(q);
  const uint64_t r2 = hx::tw_mont_form(hx::tw_mont_form(1, q), q);
  for (int i = 0; i < n; i++)
    out[i] = hx::ksp_to_mont(k[i], r2, qc);
  return 0;
}
}
