// ks_proth.h -- the per-coefficient arithmetic of the fused key switch's store loop on rows of Proth-form primes
// (ntt_kernels.hip KsLastIO::store_rows), as host/device functions so that the CPU replay
// (tests/cpp/ks_proth_store_replay.cpp) runs exactly what the kernel runs.
//
// One coefficient of output row j:   out = sum_d x_d k_d  +  acc ps   (mod q), twice (kb -> out0, ka -> out1), with
//   x_d   the digit words: NMEM canonical words from memory, the fused digit's word straight out of the transform
//         (lazy, below B q), and on an owned row the owner's word rebuilt from the s^2 row,
//         own = ((c - d_0) P_0^-1 - d_1) P_1^-1 ...;
//   k_d   the key words in MONTGOMERY form, k 2^64 mod q (hx_ksk: d_bm / d_am, converted once per matrix);
//   ps    the addPrimesAndScale factor of the parts (1), (s), as ps 2^64 mod q (or 2^64 mod q: parts already scaled).
// Every product is a word-wise Montgomery product that adds onto the running sum (mont_acc: six multiply-adds, the
// addition free), so each term is x_d k_d exactly (mod q) as a lazy word below 2q, and the sum of D + 1 of them is
// normalised ONCE, through the 32-bit reciprocal.  No 128-bit sum is formed: the compiler's 128-bit product costs ten
// instructions and four more to add it, against the four multiplications it needs.  The Barrett loop this replaces
// took, per output word, a Shoup product for the parts, D 128-bit products, a 128-bit shift, seven multiplications and
// three conditional subtractions.
// The rebuild's steps are Montgomery products by P_e^-1 2^64 mod q (8-byte constants); the subtraction rides on the
// lazy operand, own + X q - d; an absent step multiplies a zeroed digit through by 2^64 mod q (no branch).
//
// Bounds, in SIXTEENTHS of q as the Proth butterflies track them (ntt_core.h).  mont_acc(y, W, c, x) of an operand
// y below Y/16 q returns x plus a word below (16 + Y/16 + 2^-28)/16 q; y must stay below P16_YMAX/16 q.
#pragma once
#include "ntt_core.h"

namespace hx {

constexpr int ksp_after(int y16) { return 16 + (y16 + 15) / 16 + 1; }   // bound of one Montgomery product
constexpr int KSP_OWN16 = 20;   // the rebuilt word between steps: ksp_after(20 + 16) = 20, and it starts canonical
static_assert(ksp_after(KSP_OWN16 + 16) <= KSP_OWN16, "own-row rebuild: fixed point of the memory steps");

template <int ND, bool OWNED, int B>
struct KsProth {
  static constexpr int NMEM = OWNED ? ND - 2 : ND - 1;
  // the fused word enters as the transform left it where it is a legal multiplied operand -- in the sums and, on an
  // owned row, in the rebuild's last step -- else after ONE conditional subtraction of 8q (the normalisation to
  // [0, q) of the Barrett loop is gone either way)
  static constexpr bool fits(int xf16) { return xf16 <= P16_YMAX && (!OWNED || KSP_OWN16 + xf16 <= P16_YMAX); }
  static constexpr bool CSUB8 = !fits(B * 16);
  static constexpr int XF16 = CSUB8 ? 128 : B * 16;
  static constexpr int OWN_LAST16 = ksp_after(KSP_OWN16 + XF16);
  // the digit words in key order: the memory slots, the fused digit, the owner's rebuilt word
  template <int S>
  static constexpr int xbound16() { return S < NMEM ? 16 : S == NMEM ? XF16 : OWN_LAST16; }
  static constexpr int SUM16 = NMEM * ksp_after(16) + ksp_after(XF16) + (OWNED ? ksp_after(OWN_LAST16) + ksp_after(16) : 0);
  static constexpr int SUMQ = (SUM16 + 15) / 16;   // the sum of all terms, in whole q
  static_assert(B <= 16 && (!CSUB8 || B > 8), "transform output bound");
  static_assert(fits(XF16), "multiplied operands stay below 12.9375 q");
  static_assert(XF16 % 16 == 0, "the rebuild's offset is a whole multiple of q");
  static_assert(SUMQ <= 16, "the running sum stays inside 64 bits and norm_from's domain");

  struct Consts {
    uint64_t pinv[ND > 1 ? ND - 1 : 1];   // P_e^-1 2^64 mod q for e < owner, else 2^64 mod q
    uint64_t ps0, ps1;                    // ps 2^64 mod q (or 2^64 mod q); ps1 = 0 without an (s) part
    uint64_t xoff;                        // (XF16 / 16) q
  };
  static HXD uint64_t xoff(const QC& c) { return (uint64_t)(XF16 / 16) * c.q; }

  static HXD uint64_t fused_word(uint64_t v, const QC& c)
  {
    HX_BOUND(v, B, c.q);
    if constexpr (CSUB8)
      v = csub(v, c.q8);
    HX_BOUND16(v, XF16, c.q);
    return v;
  }
  // one step on a digit read from memory (canonical; `d` zeroed when the step is absent)
  static HXD uint64_t rebuild_mem(uint64_t own, uint64_t d, uint64_t pinv_m, const QC& c)
  {
    HX_BOUND16(own, KSP_OWN16, c.q);
    HX_BOUND(d, 1, c.q);
    return mont_mul(own + c.q - d, pinv_m, c);
  }
  // the last step: on the fused digit's word (zeroed unless that digit lies before the owner)
  static HXD uint64_t rebuild_last(uint64_t own, uint64_t xf, const Consts& k, const QC& c)
  {
    HX_BOUND16(own, KSP_OWN16, c.q);
    HX_BOUND16(xf, XF16, c.q);
    const uint64_t r = mont_mul(own + k.xoff - xf, k.pinv[ND - 2], c);
    HX_BOUND16(r, OWN_LAST16, c.q);
    return r;
  }
  // sum + x k for digit word S of the key order (km = k 2^64 mod q, canonical)
  template <int S>
  static HXD uint64_t term(uint64_t x, uint64_t km, uint64_t sum, const QC& c)
  {
    HX_BOUND16(x, xbound16<S>(), c.q);
    HX_BOUND(km, 1, c.q);
    return mont_acc(x, km, c, sum);
  }
  // the parts (1), (s): acc ps, the sum's first term (psm = 0: no such part -- a multiple of q all the same)
  static HXD uint64_t part(uint64_t acc, uint64_t psm, const QC& c)
  {
    HX_BOUND(acc, 1, c.q);
    return mont_mul(acc, psm, c);
  }
  // the canonical output word (EST: the 32-bit reciprocal of norm_from; the host sends no prime below 2^32 here)
  static HXD uint64_t reduce(uint64_t sum, const QC& c)
  {
    HX_BOUND16(sum, SUM16, c.q);
    return norm_from<SUMQ, true>(sum, c);
  }
};

// k 2^64 mod q for a canonical k and a Proth-form q: the conversion of one key word (engine.hip ksk_mont_kernel);
// r2 = 2^128 mod q (PrimeDev::r2)
HXD uint64_t ksp_to_mont(uint64_t k, uint64_t r2, const QC& c) { return csub(mont_mul(k, r2, c), c.q); }

}  // namespace hx
