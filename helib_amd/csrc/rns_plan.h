// rns_plan.h -- the plan of one exact RNS basis extension, built on the host, and the route a launch of it takes.
// Host-only and free of HIP: engine.hip (get_plan, launch_extend) uploads what build() returns and switches on what
// extend_route() returns; tests/cpp/rns_plan_test.cpp prints both for tests/test_rns_plan_host.py, which recomputes
// every word from Python integers.  The kernels that read the plan: rns_kernels.h, rns_mfma_kernels.hip (ExtPlanDev in
// rns_types.h binds one pointer per section below).
//
// Precondition, stated once: every modulus -- source or target -- lies in [2, 2^60).  build()
// checks it and refuses otherwise; through today's entry points that refusal is unreachable (sources and context
// targets passed hx_ctx_add_prime, which refuses q >= 2^60; explicit targets come from hx_poly_rem and
// hxi::poly_rem_device, which refuse t >= 2^60 and t < 2).  Everything below relies on it: red128_wide's domain, the
// 30-bit limb pairs of the wide record, pack_balanced's top limb (mfma_ext.h).  What still varies between plans is
// whether every prime is ABOVE 2^32 (the fast, wide and matrix-core kernels take 32-bit reciprocals): `big` below.
#pragma once
#include <cstdint>
#include <cstring>

#include <algorithm>
#include <vector>

#include "hostmath.h"
#include "mfma_ext.h"

namespace hx {
namespace rnsplan {

typedef hxh::u128 u128;

// ntt_core.h's is_proth32, restated: q = qh 2^32 + 1 with 0 < qh < 2^28.  (That header does not pass plain
// g++ -Wall -Werror -- its "#pragma unroll" lines -- and this one has to.)
inline bool is_proth32(uint64_t q) { return (uint32_t)q == 1u && (q >> 32) != 0 && (q >> 60) == 0; }

// the environment switches a plan depends on (switches.h)
struct Switches {
  bool no_proth = false, no_proth_rns = false, no_mfma_ext = false;
  int mfma_min_n = 9;
  double hps_eps = 1.0 / (double)(1u << 30);
};

// The blob's sections, in blob order, in 64-bit words (every section starts on 16 bytes).  TW sections hold (w, Shoup
// companion floor(w 2^64 / q)) pairs; u32 sections hold two entries per word, the even one in the low half.
enum Section {
  SRC_Q,         // [n]      source primes p_k
  SRC_MU64,      // [n]      floor(2^64 / p_k)
  GINV,          // [n*n] TW p_l^-1 mod p_k at k n + l (l < k)
  HALF,          // [n]      mixed-radix digits of (P - 1) / 2
  TGT_Q,         // [nt]     targets t
  TGT_MU64,      // [nt]     floor(2^64 / t)
  TGT_MU,        // [nt]     floor(2^(2 bitlen t) / t)
  TGT_K,         // [nt] u32 bitlen t
  PMOD,          // [nt]     P mod t (scaled: 1 mod t)
  W,             // [nt*n] TW (p_0 .. p_(k-1)) mod t (scaled: / P)
  UPD,           // [nt] TW  P^-1 mod t (0 when P is not invertible there)
  WP,            // [n] TW   (p_0 .. p_(k-1)) mod ptxt
  TGT_LAZY,      // [nt] u32 sum_k p_k <= 8 t
  SRC_RQ,        // [n] f64  1.0 / p_k
  TGT_PACK,      // [nt][10 + 2n]  TgtRec (rns_kernels.h), Garner-form multipliers (W)
  TGT_PACK_HPS,  // [nt][10 + 2n]  TgtRec, HPS multipliers (P / p_k) mod t (scaled: / P)
  HPS_INV,       // [n] TW   (P / p_k)^-1 mod p_k
  WP_HPS,        // [n] TW   (P / p_k) mod ptxt
  GINV_M,        // [n*n]    p_l^-1 2^64 mod p_k at k n + l (l < k)
  WIDE_PACK,     // [nt][wide_stride(n)]  WideRec; offset 0 and no words when the plan has no wide record
  NSECTIONS
};

// words of one target's wide record: 8 header words + the multipliers padded to a multiple of four, so that the last
// record's group-of-four multiplier reads stay inside the blob (rns_types.h states the same for the device)
constexpr int wide_stride(int n) { return 8 + ((n + 3) & ~3); }
constexpr size_t pack_stride(int n) { return 10 + 2 * (size_t)n; }

enum Error { OK = 0, OUT_OF_RANGE, NOT_COPRIME, NOT_INVERTIBLE_TGT, NOT_INVERTIBLE_PTXT };
inline const char* message(Error e)
{
  static const char* const text[] = {"", "basis extension: every modulus must lie in [2, 2^60)", "source primes are not pairwise coprime",
                                     "dropped primes are not invertible modulo a kept prime",
                                     "dropped primes are not invertible modulo ptxtSpace"};
  return text[e];
}

struct Plan {
  Error err = OK;                 // anything else: the plan is not usable (engine.hip reports HX_ERR_INVALID)
  std::vector<uint64_t> blob;
  size_t off[NSECTIONS] = {}, words[NSECTIONS] = {};   // where each section starts and how many words it holds
  std::vector<uint8_t> mfma;      // the matrix-core table (mfma_ext.h build_tables); empty: not built
  int n = 0, nt = 0;
  // scalars of ExtPlanDev, under the same names
  uint64_t ptxt = 0, ptxt_mu64 = 0, pinv_ptxt = 0, pmod_ptxt = 0, ptxt_mu = 0;
  uint32_t ptxt_k = 0;
  double hps_eps = 0;
  uint32_t garner_cs = 0, src_mont = 0, corr_unit = 0, mfma_steps = 0;
  uint32_t fast_ok = 0, fast16_ok = 0, hps_ok = 0, wide_ok = 0, lazy_tight_ok = 0;

  uint64_t* at(Section s) { return blob.data() + off[s]; }
  const uint64_t* at(Section s) const { return blob.data() + off[s]; }
};

// what the pieces below share: the inputs, and the few facts about them that more than one piece wants
struct Build {
  const std::vector<uint64_t>& p;   // sources
  const std::vector<uint64_t>& tq;  // targets
  uint64_t ptxt;
  bool scaled;
  Switches sw;
  int n, nt;
  u128 sum_src = 0;
  uint64_t max_src = 0, min_src = ~0ull;
  bool wide_cand;    // 17 .. 40 sources: rns_extend_wide_kernel's plans (record of 8 + n words)
  bool mfma_small;   // 9 .. 16 sources (the dropped primes of a CKKS level-2 mod-switch; from mfma_min_n on, at least 4):
                     // the fast kernels' plans, whose HPS-form launches go to the matrix-core kernel too -- it reads
                     // the wide record's header for its rarer constants
  bool rns_proth;    // Proth-form primes take Montgomery products in the fast kernels (n <= 16)
  bool hps_tables;   // the HPS front end's tables are built
  Build(const std::vector<uint64_t>& p_, const std::vector<uint64_t>& tq_, uint64_t ptxt_, bool scaled_, const Switches& sw_)
      : p(p_), tq(tq_), ptxt(ptxt_), scaled(scaled_), sw(sw_), n((int)p_.size()), nt((int)tq_.size())
  {
    for (uint64_t q : p) {
      sum_src += q;
      max_src = std::max(max_src, q);
      min_src = std::min(min_src, q);
    }
    wide_cand = n > 16 && n <= 40;
    mfma_small = n >= sw.mfma_min_n && n <= 16 && n >= 4 && !sw.no_mfma_ext;
    rns_proth = !sw.no_proth && !sw.no_proth_rns && n <= 16;
    // "lazy" needs room for up to n + 1 extra multiples of t in the sum, the correction for ptxt below 2^58 (2^56)
    hps_tables = n >= 2 && (n <= 16 || wide_cand) && (ptxt <= 1 || ptxt < ((uint64_t)1 << (wide_cand ? 56 : 58)));
  }
  bool wide_rec() const { return wide_cand || mfma_small; }
  bool tgt_mont(int t) const { return rns_proth && is_proth32(tq[(size_t)t]); }
};

inline uint64_t mont64(uint64_t x, uint64_t q) { return (uint64_t)(((u128)(x % q) << 64) % q); }   // x 2^64 mod q
inline void put_tw(uint64_t* tw, uint64_t w, uint64_t q)
{
  tw[0] = w;
  tw[1] = hxh::shoup(w, q);
}
inline void put_u32(uint64_t* sec, int i, uint32_t v) { sec[i / 2] |= (uint64_t)v << (32 * (i & 1)); }

inline void layout(const Build& b, Plan& pl)
{
  const size_t n = (size_t)b.n, nt = (size_t)b.nt;
  size_t* words = pl.words;
  words[SRC_Q] = words[SRC_MU64] = words[HALF] = words[SRC_RQ] = n;
  words[GINV] = 2 * n * n;
  words[GINV_M] = n * n;
  words[TGT_Q] = words[TGT_MU64] = words[TGT_MU] = words[PMOD] = nt;
  words[TGT_K] = words[TGT_LAZY] = (nt + 1) / 2;
  words[W] = 2 * nt * n;
  words[UPD] = 2 * nt;
  words[WP] = words[HPS_INV] = words[WP_HPS] = 2 * n;
  words[TGT_PACK] = words[TGT_PACK_HPS] = nt * pack_stride(b.n);
  words[WIDE_PACK] = b.wide_rec() ? nt * (size_t)wide_stride(b.n) : 0;
  size_t off = 0;
  for (int s = 0; s < NSECTIONS; s++) {
    pl.off[s] = words[s] ? off : 0;
    off += (words[s] + 1) & ~(size_t)1;   // keep 16-byte alignment
  }
  pl.blob.assign(off, 0);
}

// SRC_*, GINV, GINV_M, HALF
inline Error source_tables(const Build& b, Plan& pl)
{
  const int n = b.n;
  hxh::BigU P(1);
  for (int k = 0; k < n; k++) {
    const uint64_t pk = b.p[(size_t)k];
    pl.at(SRC_Q)[k] = pk;
    pl.at(SRC_MU64)[k] = (uint64_t)((((u128)1) << 64) / pk);
    const double rq = 1.0 / (double)pk;
    memcpy(&pl.at(SRC_RQ)[k], &rq, 8);
    for (int l = 0; l < k; l++) {
      const uint64_t inv = hxh::invmod(b.p[(size_t)l] % pk, pk);
      if (inv == 0)
        return NOT_COPRIME;
      put_tw(&pl.at(GINV)[2 * ((size_t)k * n + l)], inv, pk);
      pl.at(GINV_M)[(size_t)k * n + l] = mont64(inv, pk);
    }
    P.mul_word(pk);
  }
  hxh::BigU H = P;  // (P-1)/2 ; P is odd
  H.sub_word(1);
  H.shr1();
  for (int k = 0; k < n; k++)
    pl.at(HALF)[k] = H.divmod_word(b.p[(size_t)k]);
  return OK;
}

// TGT_*, W, PMOD, UPD of target t: the per-target tables the generic kernel reads, and the source of the records
inline Error target_header(const Build& b, Plan& pl, int t)
{
  const int n = b.n;
  const uint64_t q = b.tq[(size_t)t];
  const int kb = hxh::bitlen(q);
  pl.at(TGT_Q)[t] = q;
  pl.at(TGT_MU64)[t] = (uint64_t)((((u128)1) << 64) / q);
  pl.at(TGT_MU)[t] = (uint64_t)((((u128)1) << (2 * kb)) / q);
  put_u32(pl.at(TGT_K), t, (uint32_t)kb);
  // lazy 128-bit accumulation is exact when sum_k a_k*W_k < (sum_k q_k)*q_t <= 8*q_t^2 (red128_wide's domain)
  put_u32(pl.at(TGT_LAZY), t, b.sum_src <= (u128)8 * q ? 1u : 0u);
  uint64_t* w = &pl.at(W)[2 * (size_t)t * n];
  uint64_t run = 1 % q;
  for (int k = 0; k < n; k++) {
    put_tw(w + 2 * k, run, q);
    run = hxh::mulmod(run, b.p[(size_t)k] % q, q);
  }
  const uint64_t pinv = hxh::invmod(run, q);   // P^-1 mod t
  pl.at(PMOD)[t] = run;
  put_tw(&pl.at(UPD)[2 * (size_t)t], pinv, q);
  if (b.scaled) {   // every target residue comes out times P^-1: the kernels themselves are unchanged
    if (pinv == 0)
      return NOT_INVERTIBLE_TGT;
    for (int k = 0; k < n; k++)
      put_tw(w + 2 * k, hxh::mulmod(w[2 * k], pinv, q), q);
    pl.at(PMOD)[t] = 1 % q;
  }
  return OK;
}

// WP and the scalars of the plaintext-space correction (BGV scaleDownToSet); ptxt <= 1 leaves them zero
inline Error ptxt_tables(const Build& b, Plan& pl)
{
  const uint64_t ptxt = b.ptxt;
  if (ptxt <= 1)
    return OK;
  uint64_t run = 1 % ptxt;
  for (int k = 0; k < b.n; k++) {
    put_tw(&pl.at(WP)[2 * (size_t)k], run, ptxt);
    run = hxh::mulmod(run, b.p[(size_t)k] % ptxt, ptxt);
  }
  const uint64_t pinv = hxh::invmod(run, ptxt);
  if (pinv == 0)
    return NOT_INVERTIBLE_PTXT;
  const int kb = hxh::bitlen(ptxt);
  pl.ptxt = ptxt;
  pl.ptxt_mu64 = (uint64_t)((((u128)1) << 64) / ptxt);
  pl.ptxt_k = (uint32_t)kb;
  pl.ptxt_mu = (uint64_t)((((u128)1) << (2 * kb)) / ptxt);
  pl.pinv_ptxt = pinv;
  pl.pmod_ptxt = run;
  return OK;
}

// TgtRec of target t (rns_kernels.h): everything the fast kernels need of one target in one record
//   0 t   1 P mod t   2 floor(2^(63 + k) / t), k = bitlen t (red128_q8)   3 floor(2^64 / t)
//   4 k | lazy << 8 | chunk7 << 9 | mont << 10   5, 6 P^-1 mod t (TW)   7 floor(2^2k / t)
//   8 .. 8 + n multipliers, 8 + n .. 8 + 2n their Shoup companions, then 2^64 mod t (TW; red128_any's constant)
// lazy: see TGT_LAZY (`slack` more on the left: the HPS sum carries extra multiples of t); chunk7: every source prime
// <= t, so the limb sum may be taken seven terms at a time with the remainder carried (r + 7 max_src t < 8 t^2).
// mult: n multipliers below t.  The header is the same for the Garner and the HPS form but for `slack`.
inline void target_record(const Build& b, const Plan& pl, int t, const uint64_t* mult, unsigned slack, uint64_t* rec)
{
  const int n = b.n;
  const uint64_t q = b.tq[(size_t)t];
  const int kb = hxh::bitlen(q);
  const uint64_t lazy = b.sum_src + slack <= (u128)8 * q, chunk7 = b.max_src <= q;
  rec[0] = q;
  rec[1] = pl.at(PMOD)[t];
  rec[2] = (uint64_t)((((u128)1) << (63 + kb)) / q);   // < 2^64: q > 2^(kb-1)
  rec[3] = pl.at(TGT_MU64)[t];
  rec[4] = (uint64_t)kb | (lazy << 8) | (chunk7 << 9);
  rec[5] = pl.at(UPD)[2 * (size_t)t];
  rec[6] = pl.at(UPD)[2 * (size_t)t + 1];
  rec[7] = pl.at(TGT_MU)[t];
  for (int k = 0; k < n; k++) {
    rec[8 + k] = mult[k];
    rec[8 + n + k] = hxh::shoup(mult[k], q);
  }
  put_tw(&rec[8 + 2 * n], (uint64_t)((((u128)1) << 64) % q), q);
  if (!b.tgt_mont(t))
    return;
  // a Proth-form target (TgtRec::mont): the multipliers, -P mod t (in word 2) and P^-1 mod t (in the slot of
  // 2^64 mod t) times 2^64 -- the fast kernels reduce such a target's limb sum by mont_redc128.  The Shoup companions
  // stay those of the plain multipliers.
  rec[2] = mont64(q - rec[1] % q, q);
  rec[4] |= (uint64_t)1 << 10;
  for (int k = 0; k < n; k++)
    rec[8 + k] = mont64(rec[8 + k], q);
  rec[8 + 2 * n] = mont64(rec[5], q);
}

// The HPS front end: y_k = a_k (P/p_k)^-1 mod p_k, value = sum_k y_k (P/p_k) - v P.  HPS_INV, WP_HPS, and per target
// the multipliers (P/p_k) mod t (scaled plans: / P, i.e. p_k^-1 mod t), computed ONCE and written into both record
// formats: TGT_PACK_HPS (n <= 16) and the wide record (17 .. 40 sources, and the matrix-core plans of 9 .. 16).
// mult [nt*n], negp [nt]: kept for the matrix-core table.
inline void hps_records(const Build& b, Plan& pl, std::vector<uint64_t>& mult, std::vector<uint64_t>& negp)
{
  const int n = b.n, nt = b.nt;
  auto prod_except = [&](int k, uint64_t m) {   // (P / p_k) mod m
    uint64_t r = 1 % m;
    for (int l = 0; l < n; l++)
      if (l != k)
        r = hxh::mulmod(r, b.p[(size_t)l] % m, m);
    return r;
  };
  for (int k = 0; k < n; k++) {   // (invertible: the sources are pairwise coprime)
    const uint64_t pk = b.p[(size_t)k];
    put_tw(&pl.at(HPS_INV)[2 * (size_t)k], hxh::invmod(prod_except(k, pk), pk), pk);
    if (b.ptxt > 1)
      put_tw(&pl.at(WP_HPS)[2 * (size_t)k], prod_except(k, b.ptxt), b.ptxt);
  }
  mult.assign((size_t)nt * n, 0);
  negp.assign((size_t)nt, 0);
  for (int t = 0; t < nt; t++) {
    const uint64_t q = b.tq[(size_t)t], pinv_t = pl.at(UPD)[2 * (size_t)t];
    uint64_t* w = &mult[(size_t)t * n];
    for (int k = 0; k < n; k++)
      w[k] = b.scaled ? hxh::mulmod(prod_except(k, q), pinv_t, q) : prod_except(k, q);
    if (!b.wide_cand)
      target_record(b, pl, t, w, 32, &pl.at(TGT_PACK_HPS)[(size_t)t * pack_stride(n)]);
    if (!b.wide_rec())
      continue;
    // WideRec: t, P mod t (scaled: 1), 2^64 mod t (TW), floor(2^64 / t), P^-1 mod t (TW), the companion of P mod t;
    // then the multipliers as 30-bit limb pairs (low limb in bits 0 .. 29, high limb from bit 32)
    uint64_t* rec = &pl.at(WIDE_PACK)[(size_t)t * wide_stride(n)];
    const uint64_t pmod = pl.at(PMOD)[t];
    rec[0] = q;
    rec[1] = pmod;
    put_tw(&rec[2], (uint64_t)((((u128)1) << 64) % q), q);
    rec[4] = pl.at(TGT_MU64)[t];
    rec[5] = pinv_t;
    rec[6] = pl.at(UPD)[2 * (size_t)t + 1];
    rec[7] = hxh::shoup(pmod, q);
    for (int k = 0; k < n; k++)
      rec[8 + k] = (w[k] & 0x3fffffffull) | ((w[k] >> 30) << 32);
    negp[(size_t)t] = (q - pmod % q) % q;
  }
}

// The capability flags, from two facts about the primes and the bounds on n.  `big`: every source and every target
// is above 2^32 (below 2^60 they all are: the precondition).
//
//   flag           garner_cs  big  sources   further
//   fast_ok            x       x   n <= 8                         break_digits_fast_kernel
//   fast16_ok          x       x   n <= 16                        rns_extend_fast_kernel, Garner form
//   hps_ok             x       x   2 .. 16   HPS tables           ... its HPS front end (it lives in the fast kernels only)
//   wide_ok                    x   17 .. 40  HPS tables           rns_extend_wide_kernel
//   mfma_steps != 0   hps_ok (mfma_min_n .. 16, at least 4) or wide_ok, and not no_mfma_ext: the table is built
//   lazy_tight_ok     no Proth-form target is left on the Barrett branch while its row transform is Proth-form
//   src_mont          rns_proth and every source is Proth-form: the Garner steps run on GINV_M
//   corr_unit         scaled, ptxt > 1 and ptxt <= every target: the correction of a target is the remainder itself
//
// The matrix-core gate for 9 .. 16 sources thus rests on the same `big` as the wide one (and, through hps_ok, on
// garner_cs, which the Garner pass over its redo list needs).
inline void flags(const Build& b, Plan& pl)
{
  const int n = b.n;
  const auto& tq = b.tq;
  const bool tgt_big = std::all_of(tq.begin(), tq.end(), [](uint64_t t) { return (t >> 32) != 0; });
  const bool big = (b.min_src >> 32) != 0 && tgt_big;
  // a_l < q_l <= max < 2*min <= 2*p_k, or the sources ascend (a_l < p_l <= p_k for l < k)
  const bool garner_cs = b.max_src / 2 < b.min_src || std::is_sorted(b.p.begin(), b.p.end());
  const bool fast16 = garner_cs && big && n <= 16;
  const bool hps = fast16 && b.hps_tables;
  const bool wide = big && b.wide_cand && b.hps_tables;
  pl.garner_cs = garner_cs;
  pl.fast_ok = fast16 && n <= 8;
  pl.fast16_ok = fast16;
  pl.hps_ok = hps;
  pl.wide_ok = wide;
  pl.mfma_steps = (!b.sw.no_mfma_ext && (wide || (hps && b.mfma_small))) ? (uint32_t)hx::mfx::steps_for(n) : 0;
  // lazy output is read at the Proth rows' tight bounds: legal only when the kernel that wrote a Proth-form target row
  // took its Montgomery branch
  pl.lazy_tight_ok = b.sw.no_proth || b.rns_proth || std::none_of(tq.begin(), tq.end(), is_proth32);
  pl.src_mont = b.rns_proth && std::all_of(b.p.begin(), b.p.end(), is_proth32);
  pl.corr_unit = b.scaled && b.ptxt > 1 && std::all_of(tq.begin(), tq.end(), [&](uint64_t t) { return b.ptxt <= t; });
}

// The plan of the extension from the residues modulo p (n = 1 .. any) to the moduli tq; ptxt > 1: with the
// plaintext-space correction; scaled: every target residue comes out multiplied by P^-1 mod t.
inline Plan build(const std::vector<uint64_t>& p, const std::vector<uint64_t>& tq, uint64_t ptxt, bool scaled,
                  const Switches& sw)
{
  Plan pl;
  auto in_range = [](uint64_t q) { return q >= 2 && (q >> 60) == 0; };
  if (p.empty() || !std::all_of(p.begin(), p.end(), in_range) || !std::all_of(tq.begin(), tq.end(), in_range)) {
    pl.err = OUT_OF_RANGE;
    return pl;
  }
  const Build b(p, tq, ptxt, scaled, sw);
  pl.n = b.n;
  pl.nt = b.nt;
  pl.hps_eps = sw.hps_eps;
  layout(b, pl);
  pl.err = source_tables(b, pl);
  for (int t = 0; t < b.nt && !pl.err; t++)
    pl.err = target_header(b, pl, t);
  if (!pl.err)
    pl.err = ptxt_tables(b, pl);
  if (pl.err)
    return pl;
  std::vector<uint64_t> garner((size_t)b.n);
  for (int t = 0; t < b.nt; t++) {
    for (int k = 0; k < b.n; k++)
      garner[(size_t)k] = pl.at(W)[2 * ((size_t)t * b.n + k)];
    target_record(b, pl, t, garner.data(), 0, &pl.at(TGT_PACK)[(size_t)t * pack_stride(b.n)]);
  }
  std::vector<uint64_t> mult, negp;
  if (b.hps_tables)
    hps_records(b, pl, mult, negp);
  flags(b, pl);
  if (pl.mfma_steps)   // the same extension on the matrix cores: multipliers as balanced 8-bit limbs in MFMA operand order
    hx::mfx::build_tables(b.n, b.nt, tq.data(), mult.data(), negp.data(), pl.at(UPD), pl.mfma);
  return pl;
}

// ------------------------------------------------------------------ the route of one launch
// FAST_*: rns_extend_fast_kernel<n, .> (n <= 16).  GARNER: Garner over everything.  HPS: the HPS form, then Garner
// over its redo list.  MFMA: the HPS form with its target sums on the matrix cores, then Garner over its redo list.
// WIDE_*: 17 .. 40 sources, rns_extend_wide_kernel or the matrix-core kernel, rns_extend_kernel<40> over the redo list.
// GENERIC: rns_extend_kernel<8 / 16 / 40 / 64 / EXT_MAXSRC>, which takes any plan.
enum Route { FAST_GARNER, FAST_HPS, FAST_MFMA, WIDE_VALU, WIDE_MFMA, GENERIC };

struct RouteFlags {
  uint32_t fast16_ok, hps_ok, wide_ok, mfma_steps;
};

constexpr size_t WIDE_LDS_MAX = 160 * 1024;   // bytes of LDS a workgroup of the wide kernel may ask for

// The HPS form of the fast kernels pays from nine source primes on (hps_min_n; switches.h): measured same-box
// (round 3), the digit kernel with 5-8 primes per digit is 3-5 % SLOWER with it (366 vs 350 us at BGV L=16,
// 828 vs 808 us at CKKS L=24: eight u64 -> double conversions cost what the 10-28 dependent Garner products cost), the
// basis extension of 11 dropped primes is faster (Garner there is 55 products and spills 62 dwords; CKKS level 2
// +3 %).  HX_HPS_MIN_N overrides (tests force 2).
// HX_HPS_MIN_N and HX_MFMA_MIN_N: a plan that carries the matrix-core table (from mfma_min_n sources on) takes the HPS
// form on the matrix cores BELOW hps_min_n too -- raising HX_HPS_MIN_N alone does not select the Garner control for
// such a plan; HX_NO_MFMA_EXT=1 (or a higher HX_MFMA_MIN_N) with it does.
// upd: the launch updates rows in place (breakIntoDigits).  The fast kernels' HPS form cannot redo such a row, so it
// takes Garner; the wide route leaves untrusted coefficients untouched, so its redo pass is correct there too.
// row_words >= 2^32: the redo list holds 32-bit coefficient indices.
inline Route extend_route(const RouteFlags& f, int n, int nt, bool upd, size_t row_words, int hps_min_n)
{
  const bool listable = row_words < ((size_t)1 << 32);
  if (f.fast16_ok) {
    const bool hps = f.hps_ok && !upd && listable;
    if (hps && f.mfma_steps != 0)
      return FAST_MFMA;
    return hps && n >= hps_min_n ? FAST_HPS : FAST_GARNER;
  }
  // the plan's multipliers once per workgroup.  With nt <= MAX_ROWS = 160 (dev_common.h) and n <= 40 this is at most
  // 160 * 48 * 8 = 61440 bytes, so the last test never fails today; it stays as the guard of a larger MAX_ROWS
  // (such a plan goes to the generic kernel, which handles any plan)
  const size_t wide_lds = (size_t)nt * (size_t)wide_stride(n) * 8;
  if (f.wide_ok && listable && wide_lds <= WIDE_LDS_MAX)
    return f.mfma_steps != 0 ? WIDE_MFMA : WIDE_VALU;
  return GENERIC;
}

}  // namespace rnsplan
}  // namespace hx
