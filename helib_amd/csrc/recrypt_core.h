// recrypt_core.h -- the per-coefficient arithmetic of recryption's pre-processing (include/helib_amd.h: hx_recrypt_prep),
// shared word for word by recrypt_prep_kernel (recrypt.hip) and by host programs that replay it
// (tests/cpp/recrypt_core_replay.cpp).  No HIP header is needed on the host.
//
// What is computed, per coefficient, is Ctxt::rawModSwitch (src/Ctxt.cpp:2949-3049) followed by newMakeDivisible
// (src/recryption.cpp:73-136) and the division by p^e' (src/recryption.cpp:495-497), as exact integers:
//   c      the centred lift of the k residues, in [-Q/2, Q/2), Q = prod q_i (odd)
//   c q  = Q X + Y, floor division, then Y > floor(Q/2): Y -= Q, X += 1
//   delta = (Y mod p2r) (Q^-1 mod p2r) mod p2r, centred (ties below)
//   x    = X + delta, reduced symmetrically modulo q
//   v      the small multiple of q that makes x + q v divisible by p2e = p^e' (q = 1 mod p2e, so v = -x centred mod p2e)
//   w    = (x + q v) / p2e, and row t of the output is w mod t
// The reference converts powerful -> polynomial basis between x and v and back after the division; both maps are
// integer-linear and mutually inverse, and nothing here depends on which basis a coefficient is written in, so doing
// the whole chain on the powerful cube gives the cube of what the reference gets (given the same tie bits).
//
// No big integers and no floating point:
//   * Garner mixed-radix digits a_i of a residue vector: value = a_0 + a_1 q_0 + a_2 q_0 q_1 + ... in [0, Q); the sign
//     of the centred value by comparing digits with those of (Q - 1) / 2, the top digit first.
//   * Y's residues are c_i q mod q_i; its digits give its sign, Y mod p2r and Y mod 2^64.
//   * Q is odd, so it is invertible modulo 2^64: X = (c q - Y) Q^-1 mod 2^64 in wrapping arithmetic, read as a signed
//     word.  That is exact because c q - Y = Q X holds over the integers and |X| <= q / 2 + 1 < 2^63.
//   * everything after X fits a signed word: |x| <= q / 2 + p2r, |q v| < 2^59.
//   * nothing divides on the device: remainders modulo p2r and p2e go through floor(2^64 / modulus) (reduce()), the
//     exact division by p2e is a shift for p = 2 and a product with p2e^-1 modulo 2^64 for odd p.
// Multiplications modulo a 60-bit prime are by constants, done Shoup's way: with ws = floor(w 2^64 / q),
// x w - floor(x ws / 2^64) q lies in [0, 2 q) for EVERY 64-bit x (w < q < 2^63), so digits of one prime can be
// multiplied modulo another without reducing them first.
//
// Tie bits.  The reference draws NTL::RandomBnd(2) at each tie, which cannot be reproduced.  Here tie number `which`
// (0: delta at p2r / 2 with Y = 0; 1: x at +-q / 2; 2: x mod p2e at p2e / 2) of coefficient j of batch element b of
// part `part` is bit 61 + which of
//     mix(mix(mix(mix(seed) + part) + b) + j),     mix = the splitmix64 finaliser over z + 0x9E3779B97F4A7C15
// -- a counter-based function of the seed, the same on both sides, balanced (E[v] = 0 needs that).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HXRC_HD __host__ __device__ __forceinline__
#define HXRC_UNROLL _Pragma("unroll")
#else
#define HXRC_HD inline
#define HXRC_UNROLL
#endif

namespace hxrc {

constexpr int MAX_K = 16;   // source primes (the ciphertext's: three ciphertext primes and the special primes)
constexpr int MAX_T = 64;   // target primes (the encrypted recryption key's)
constexpr uint64_t Q_BOUND = 1ull << 30;   // q = p^e + 1 < 2^30: the reference's e_bnd (src/recryption.cpp:211-217)

struct Plan {
  uint32_t k, nt;
  uint32_t p_is_2, pad;
  uint64_t q, p2r, p2e;
  uint64_t seed, part;
  uint64_t src_q[MAX_K];
  uint64_t qmul[MAX_K], qmul_s[MAX_K];     // q mod q_i and its Shoup companion
  uint64_t pinv[MAX_K], pinv_s[MAX_K];     // (q_0 .. q_(i-1))^-1 mod q_i
  uint64_t w[MAX_K][MAX_K], w_s[MAX_K][MAX_K];   // [i][l], l < i: q_0 .. q_(l-1) mod q_i
  uint64_t half[MAX_K];                    // the digits of (Q - 1) / 2
  uint64_t p64[MAX_K], Q64, Qinv64;        // q_0 .. q_(i-1) mod 2^64, Q mod 2^64, Q^-1 mod 2^64
  uint64_t pr[MAX_K], Qr, Qinv_r;          // the same modulo p2r
  // no 64-bit division on the device: floor(2^64 / p2r) and floor(2^64 / p2e) for reduce(), a multiple of p2e in
  // [2^30, 2^31) that makes x non-negative before it is reduced, and the exact division by p2e as a shift (p = 2) or
  // as a product with p2e^-1 modulo 2^64 (p odd)
  uint64_t mu_r, mu_e, zoff, p2e_inv64;
  uint32_t e_shift, pad2;
  uint64_t tgt[MAX_T];
};

struct Result {
  int64_t x, v, w;
};

HXRC_HD uint64_t mulhi64(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// x w mod q for any 64-bit x; w < q < 2^63, ws = floor(w 2^64 / q)
HXRC_HD uint64_t shoup_mul(uint64_t x, uint64_t w, uint64_t ws, uint64_t q)
{
  const uint64_t r = x * w - mulhi64(x, ws) * q;
  return r >= q ? r - q : r;
}

// x mod m for any 64-bit x, mu = floor(2^64 / m), m >= 2: floor(x mu / 2^64) is floor(x / m) or one less, so the
// remainder estimate lies in [0, 2 m)
HXRC_HD uint64_t reduce(uint64_t x, uint64_t m, uint64_t mu)
{
  const uint64_t r = x - mulhi64(x, mu) * m;
  return r >= m ? r - m : r;
}

HXRC_HD uint64_t mix(uint64_t z)
{
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
HXRC_HD uint64_t tie_word(uint64_t seed, uint64_t part, uint64_t b, uint64_t j) { return mix(mix(mix(mix(seed) + part) + b) + j); }
HXRC_HD bool tie_bit(uint64_t word, int which) { return ((word >> (61 + which)) & 1) != 0; }

// what the digits of one value give: is it above (Q - 1) / 2, is it zero, its value modulo 2^64 and modulo p2r -- the
// last two of the CENTRED value
struct Lift {
  bool neg, zero;
  uint64_t m64, mr;
};

// x[i] < q_i.  K is the number of primes, a compile-time constant so that the digits stay in registers.
template <int K>
HXRC_HD Lift lift(const Plan& P, const uint64_t (&x)[K], bool want_r)
{
  uint64_t a[K];
  HXRC_UNROLL
  for (int i = 0; i < K; i++) {
    const uint64_t qi = P.src_q[i];
    uint64_t s = 0;
  HXRC_UNROLL
    for (int l = 0; l < i; l++) {
      s += shoup_mul(a[l], P.w[i][l], P.w_s[i][l], qi);   // < 2^61
      s = s >= qi ? s - qi : s;
    }
    const uint64_t t = x[i] >= s ? x[i] - s : x[i] + qi - s;
    a[i] = shoup_mul(t, P.pinv[i], P.pinv_s[i], qi);
  }
  Lift L;
  int cmp = 0;   // the sign of value - (Q - 1) / 2, the top digit deciding
  bool zero = true;
  uint64_t m64 = 0, mr = 0;
  HXRC_UNROLL
  for (int i = K - 1; i >= 0; i--) {
    if (cmp == 0)
      cmp = a[i] > P.half[i] ? 1 : (a[i] < P.half[i] ? -1 : 0);
    zero = zero && a[i] == 0;
    m64 += a[i] * P.p64[i];
    if (want_r)
      mr = reduce(mr + reduce(a[i], P.p2r, P.mu_r) * P.pr[i], P.p2r, P.mu_r);   // (both factors below 2^30)
  }
  L.neg = cmp > 0;
  L.zero = zero;
  if (L.neg) {
    m64 -= P.Q64;
    mr = reduce(mr + P.p2r - P.Qr, P.p2r, P.mu_r);
  }
  L.m64 = m64;
  L.mr = mr;
  return L;
}

// c[i]: the coefficient's residue modulo q_i; b, j: its batch element and its index in the row
template <int K>
HXRC_HD Result prep_one(const Plan& P, const uint64_t (&c)[K], uint64_t b, uint64_t j)
{
  const int64_t q = (int64_t)P.q, p2r = (int64_t)P.p2r, p2e = (int64_t)P.p2e;
  uint64_t y[K];
  HXRC_UNROLL
  for (int i = 0; i < K; i++)
    y[i] = shoup_mul(c[i], P.qmul[i], P.qmul_s[i], P.src_q[i]);
  const Lift C = lift<K>(P, c, false);
  const Lift Y = lift<K>(P, y, true);
  const uint64_t ties = tie_word(P.seed, P.part, b, j);
  // c q = Q X + Y with Y centred
  const int64_t X = (int64_t)((C.m64 * P.q - Y.m64) * P.Qinv64);
  int64_t delta = (int64_t)reduce(Y.mr * P.Qinv_r, P.p2r, P.mu_r);
  if (delta > (p2r >> 1) || ((p2r & 1) == 0 && delta == (p2r >> 1) && (Y.neg || (Y.zero && tie_bit(ties, 0)))))
    delta -= p2r;
  int64_t x = X + delta;
  const bool q_even = (q & 1) == 0;
  const int64_t qh = q >> 1;
  if (x > qh || (q_even && x == qh && tie_bit(ties, 1)))
    x -= q;
  else if (x < -qh || (q_even && x == -qh && tie_bit(ties, 1)))
    x += q;
  Result R;
  R.x = x;
  int64_t v = 0;
  if (p2e > 1) {
    const int64_t z = (int64_t)reduce((uint64_t)(x + (int64_t)P.zoff), P.p2e, P.mu_e);   // |x| <= q / 2 < 2^29 <= zoff / 2
    if (z > (p2e >> 1) || (P.p_is_2 && z == (p2e >> 1) && tie_bit(ties, 2)))
      v = p2e - z;
    else
      v = -z;
  }
  R.v = v;
  const int64_t n = x + q * v;   // divisible by p2e: q = 1 mod p2e
  R.w = P.p_is_2 ? (n >> P.e_shift) : (int64_t)((uint64_t)n * P.p2e_inv64);
  return R;
}

// w mod t for |w| < q < 2^30 and t >= 2^31 (build_plan refuses a smaller output modulus): no remainder to take
HXRC_HD uint64_t residue(int64_t w, uint64_t t) { return w < 0 ? t - (uint64_t)(-w) : (uint64_t)w; }

}  // namespace hxrc

// ---------------- the plan, on the host ----------------
#include <stdio.h>

#include <string>
#include <vector>

namespace hxrc {

inline uint64_t h_mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((unsigned __int128)a * b % q); }
inline uint64_t h_powmod(uint64_t a, uint64_t e, uint64_t q)
{
  uint64_t r = 1 % q;
  a %= q;
  for (; e; e >>= 1, a = h_mulmod(a, a, q))
    if (e & 1)
      r = h_mulmod(r, a, q);
  return r;
}
inline uint64_t h_gcd(uint64_t a, uint64_t b)
{
  while (b) {
    const uint64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}
// a^-1 mod n for gcd(a, n) = 1, n < 2^63 (extended Euclid on signed 128-bit words)
inline uint64_t h_invmod(uint64_t a, uint64_t n)
{
  __int128 r0 = n, r1 = a % n, t0 = 0, t1 = 1;
  while (r1 != 0) {
    const __int128 qq = r0 / r1, r2 = r0 - qq * r1, t2 = t0 - qq * t1;
    r0 = r1;
    r1 = r2;
    t0 = t1;
    t1 = t2;
  }
  if (t0 < 0)
    t0 += n;
  return (uint64_t)t0;
}
inline uint64_t h_shoup(uint64_t w, uint64_t q) { return (uint64_t)(((unsigned __int128)w << 64) / q); }
inline bool h_is_power_of(uint64_t x, uint64_t p)
{
  while (x % p == 0)
    x /= p;
  return x == 1;
}

// Fills P (seed and part are the caller's); returns why not, or the empty string.  src: the k primes of the input's
// rows, distinct odd primes below 2^60; tgt: the moduli of the output rows, each in [2^31, 2^63).
inline std::string build_plan(const std::vector<uint64_t>& src, const std::vector<uint64_t>& tgt, uint64_t q, uint64_t p, uint64_t p2r,
                              uint64_t p2e, Plan& P)
{
  char msg[320];
#define HXRC_REFUSE(...)                  \
  do {                                    \
    snprintf(msg, sizeof msg, __VA_ARGS__); \
    return std::string(msg);              \
  } while (0)
  typedef unsigned long long ull;
  const size_t k = src.size(), nt = tgt.size();
  if (k < 1 || k > (size_t)MAX_K)
    HXRC_REFUSE("the part has %zu rows; the exact lift of recryption's pre-processing takes 1 to %d", k, MAX_K);
  if (nt < 1 || nt > (size_t)MAX_T)
    HXRC_REFUSE("the output has %zu rows; recryption's pre-processing writes 1 to %d", nt, MAX_T);
  if (p < 2 || p2r < 2 || p2e < 1 || p2r >= Q_BOUND || p2e >= Q_BOUND || !h_is_power_of(p2r, p) || !h_is_power_of(p2e, p))
    HXRC_REFUSE("p2r = %llu and p2ePrime = %llu are not powers of p = %llu below 2^30 (p2r at least p)", (ull)p2r, (ull)p2e, (ull)p);
  if (q < 2 || q >= Q_BOUND)
    HXRC_REFUSE("q = %llu is not in [2, 2^30) (the reference's e_bnd)", (ull)q);
  if (h_gcd(q, p2r) != 1)
    HXRC_REFUSE("gcd(q, p2r) = gcd(%llu, %llu) = %llu is not 1", (ull)q, (ull)p2r, (ull)h_gcd(q, p2r));
  if ((q - 1) % p2e != 0)
    HXRC_REFUSE("q = %llu is not 1 modulo p2ePrime = %llu", (ull)q, (ull)p2e);
  uint64_t Qq = 1 % q;
  for (size_t i = 0; i < k; i++) {
    if (src[i] < 3 || src[i] % 2 == 0 || src[i] >= (1ull << 60))
      HXRC_REFUSE("the row modulus %llu is not an odd number in [3, 2^60)", (ull)src[i]);
    for (size_t l = 0; l < i; l++)
      if (h_gcd(src[i], src[l]) != 1)
        HXRC_REFUSE("the row moduli %llu and %llu are not coprime", (ull)src[l], (ull)src[i]);
    if (h_gcd(src[i], p) != 1)
      HXRC_REFUSE("the row modulus %llu is not coprime to p = %llu", (ull)src[i], (ull)p);
    Qq = h_mulmod(Qq, src[i] % q, q);
  }
  if (h_gcd(Qq, q) != 1)
    HXRC_REFUSE("gcd(Q mod q, q) = gcd(%llu, %llu) = %llu is not 1", (ull)Qq, (ull)q, (ull)h_gcd(Qq, q));
  for (size_t t = 0; t < nt; t++)
    if (tgt[t] < (1ull << 31) || tgt[t] >= (1ull << 63))
      HXRC_REFUSE("the output modulus %llu is not in [2^31, 2^63) (|w| < q < 2^30 is reduced without a division)", (ull)tgt[t]);
#undef HXRC_REFUSE
  P = Plan();
  P.k = (uint32_t)k;
  P.nt = (uint32_t)nt;
  P.p_is_2 = p == 2 ? 1u : 0u;
  P.q = q;
  P.p2r = p2r;
  P.p2e = p2e;
  uint64_t q64 = 1, qr = 1 % p2r;
  for (size_t i = 0; i < k; i++) {
    const uint64_t qi = src[i];
    P.src_q[i] = qi;
    P.qmul[i] = q % qi;
    P.qmul_s[i] = h_shoup(P.qmul[i], qi);
    uint64_t prod = 1 % qi;
    for (size_t l = 0; l < i; l++) {
      P.w[i][l] = prod;
      P.w_s[i][l] = h_shoup(prod, qi);
      prod = h_mulmod(prod, src[l] % qi, qi);
    }
    P.pinv[i] = h_invmod(prod, qi);
    P.pinv_s[i] = h_shoup(P.pinv[i], qi);
    P.p64[i] = q64;
    P.pr[i] = qr;
    q64 *= qi;
    qr = h_mulmod(qr, qi % p2r, p2r);
  }
  P.Q64 = q64;
  P.Qr = qr;
  P.Qinv_r = h_invmod(qr, p2r);
  P.mu_r = (uint64_t)((((unsigned __int128)1) << 64) / p2r);
  P.mu_e = p2e > 1 ? (uint64_t)((((unsigned __int128)1) << 64) / p2e) : 0;
  P.zoff = p2e * (((1ull << 30) + p2e - 1) / p2e);
  P.e_shift = 0;
  P.p2e_inv64 = 1;
  if (p == 2) {
    while ((1ull << P.e_shift) < p2e)
      P.e_shift++;
  } else {
    for (int it = 0; it < 6; it++)   // Newton modulo 2^64, as for Q below: p2e is odd
      P.p2e_inv64 *= 2 - p2e * P.p2e_inv64;
  }
  uint64_t inv = 1;   // Newton modulo 2^64: Q is odd, so 1 is right to one bit; six doublings give 64
  for (int it = 0; it < 6; it++)
    inv *= 2 - q64 * inv;
  P.Qinv64 = inv;
  // the digits of (Q - 1) / 2: with every q_i odd, (Q - 1) / 2 = sum_i ((q_i - 1) / 2) q_0 .. q_(i-1)
  for (size_t i = 0; i < k; i++)
    P.half[i] = (src[i] - 1) / 2;
  for (size_t t = 0; t < nt; t++)
    P.tgt[t] = tgt[t];
  return std::string();
}

// one coefficient on the host, the switch over k that the kernel's launch makes
inline Result prep_any(const Plan& P, const uint64_t* c, uint64_t b, uint64_t j)
{
  switch (P.k) {
#define HXRC_CASE(K)             \
  case K: {                      \
    uint64_t r[K];               \
    for (int i = 0; i < K; i++)  \
      r[i] = c[i];               \
    return prep_one<K>(P, r, b, j); \
  }
    HXRC_CASE(1) HXRC_CASE(2) HXRC_CASE(3) HXRC_CASE(4) HXRC_CASE(5) HXRC_CASE(6) HXRC_CASE(7) HXRC_CASE(8)
    HXRC_CASE(9) HXRC_CASE(10) HXRC_CASE(11) HXRC_CASE(12) HXRC_CASE(13) HXRC_CASE(14) HXRC_CASE(15) HXRC_CASE(16)
#undef HXRC_CASE
  }
  return Result{0, 0, 0};
}

}  // namespace hxrc
