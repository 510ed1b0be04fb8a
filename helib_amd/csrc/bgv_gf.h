// bgv_gf.h -- host tables of BGV slot encoding and decoding with slots in GF(p^d) = Z_p[X] / G, G = F_0 the first
// factor of Phi_m mod p: EncryptedArray(context, G) with deg G = d = ord_m(p) at r = 1, over the G = F_0 branches of
// PAlgebraModDerived::mapToSlots, embedInSlots, CRT_reconstruct and decodePlaintext (src/PAlgebra.cpp:1064-1067,
// 1096-1100, 1168-1186, 1243-1278).  Plain C++ (no device code), on top of bgv_crt.h's factors, E and R.
//
//   slot i holds alpha_i(X), deg < d, read modulo G; t_i = ith_rep(i)
//   A_i (d x d)   row l = X^(t_i l) mod F_i, so the CRT component is c_i = alpha_i(X^(t_i)) mod F_i = alpha_i A_i
//                 (the reference's matrix_maps)
//   encode        H = sum_i c_i(X) E_i(X) mod Phi_m: a d-tap sliding window over E,
//                   W[k] = sum_i sum_(j < d) c_i[j] E_i[k - j],  0 <= k < phi(m) + d - 1   (E_i = 0 outside [0, phi(m)))
//                 and the d - 1 top words folded back with
//   T (d-1 rows)  T_u = X^(phi(m) + u) mod Phi_m mod p:  H[k] = W[k] + sum_u W[phi(m) + u] T_u[k]
//   Rx            bgv_crt.h's R_i run d - 1 words further along its recurrence: u_i[j] = sum_k w[k] Rx_i[k + j] is the
//                 constant term of X^j w mod F_i
//   M_i (d x d)   alpha_i[l] = sum_j M_i[l][j] u_i[j]: the inverse of alpha -> u.  It exists because b -> [X^0](b c) is
//                 not the zero functional for c != 0 in a field, so the d functionals c -> [X^0](X^j c) are a basis of
//                 the dual; it composes "u -> w mod F_i" with "c -> c(X^(1/t_i)) mod G".
// d = 1: G is linear, A_i = M_i = [1], there is no fold: the integer path of bgv_crt.h, word for word.
// No phi(m) x phi(m) table is built: E stays nslots x ld, Rx is nslots x ldr (ldr = phi(m) + d - 1 rounded up to 4
// words, zero filled, so that a row starts on a 16-byte boundary), A and M nslots d^2 words each, T (d - 1) x ld.
//
// r > 1 (build_gf's last argument): slots in the Galois ring Z_(p^r)[X] / G, G the Hensel lift of F_0.  Every table above
// is the same formula modulo P = p^r over the lifted factors bgv_crt.h computes: the lift of a factorisation is unique,
// so X -> X^(t_i) carries the lifted F_0 to the lifted F_i exactly as it does modulo p, and A_i, T, Rx need no change
// but the modulus.  alpha -> u is invertible modulo P because it is modulo p; only the elimination knows about the
// prime: gf_invert picks a pivot that is a unit, i.e. non-zero modulo p (one exists in every column, the matrix being
// invertible modulo p).  At r = 1 every word is the one built above.
#pragma once
#include "bgv_crt.h"

namespace hxc {

constexpr uint32_t GF_MAX_D = 64;   // the device kernels stage d - 1 <= 63 words of halo

struct GfTables {
  CrtTables crt;                // geometry, factors, E (and R, the first phi(m) words of every row of Rx)
  uint32_t ldr = 0;             // words between the rows of Rx
  std::vector<uint32_t> G;      // d + 1 words, constant coefficient first: F_0
  std::vector<uint32_t> A, M;   // [nslots][d][d]
  std::vector<uint32_t> T;      // [d - 1][ld]
  std::vector<uint32_t> Rx;     // [nslots][ldr]
};

// a b mod the monic f of degree d (d + 1 words), all of d words
inline void gf_mulmod(const uint32_t* a, const uint32_t* b, const uint32_t* f, uint32_t d, uint64_t p, uint32_t* out)
{
  std::vector<uint64_t> r(2 * d - 1, 0);
  for (uint32_t i = 0; i < d; i++)
    if (a[i])
      for (uint32_t j = 0; j < d; j++)
        r[i + j] = (r[i + j] + (uint64_t)a[i] * b[j]) % p;
  for (uint32_t i = 2 * d - 1; i-- > d;) {
    const uint64_t c = r[i];
    if (c)
      for (uint32_t j = 0; j < d; j++)
        r[i - d + j] = (r[i - d + j] + (p - c) * f[j]) % p;
  }
  for (uint32_t i = 0; i < d; i++)
    out[i] = (uint32_t)r[i];
}

// the inverse of the d x d matrix a modulo p (row major) into inv; false: singular.  prime: p is a power of it (0: p
// itself is the prime) and a pivot has to be a unit, non-zero modulo the prime
inline bool gf_invert(std::vector<uint64_t> a, uint32_t d, uint64_t p, uint32_t* inv, uint64_t prime = 0)
{
  if (!prime)
    prime = p;
  std::vector<uint64_t> b((size_t)d * d, 0);
  for (uint32_t i = 0; i < d; i++)
    b[(size_t)i * d + i] = 1 % p;
  for (uint32_t c = 0; c < d; c++) {
    uint32_t piv = c;
    while (piv < d && a[(size_t)piv * d + c] % prime == 0)
      piv++;
    if (piv == d)
      return false;
    for (uint32_t k = 0; k < d && piv != c; k++) {
      std::swap(a[(size_t)piv * d + k], a[(size_t)c * d + k]);
      std::swap(b[(size_t)piv * d + k], b[(size_t)c * d + k]);
    }
    const uint64_t s = hxh::invmod(a[(size_t)c * d + c], p);
    for (uint32_t k = 0; k < d; k++) {
      a[(size_t)c * d + k] = a[(size_t)c * d + k] * s % p;
      b[(size_t)c * d + k] = b[(size_t)c * d + k] * s % p;
    }
    for (uint32_t r = 0; r < d; r++) {
      const uint64_t f = a[(size_t)r * d + c];
      if (r == c || !f)
        continue;
      for (uint32_t k = 0; k < d; k++) {
        a[(size_t)r * d + k] = (a[(size_t)r * d + k] + (p - f) * a[(size_t)c * d + k]) % p;
        b[(size_t)r * d + k] = (b[(size_t)r * d + k] + (p - f) * b[(size_t)c * d + k]) % p;
      }
    }
  }
  for (size_t i = 0; i < (size_t)d * d; i++)
    inv[i] = (uint32_t)b[i];
  return true;
}

// "", or the reason the tables cannot be built.  r: the tables are modulo p^r (the top of this file); sup_gens /
// sup_ords: build_crt's (the hypercube over supplied generators)
inline std::string build_gf(uint64_t m, uint64_t prime, GfTables& t, uint32_t r = 1, const std::vector<uint64_t>* sup_gens = nullptr,
                            const std::vector<int64_t>* sup_ords = nullptr)
{
  char msg[200];
  t = GfTables();
  std::string why = build_crt(m, prime, t.crt, false, r, sup_gens, sup_ords);   // the geometry first: d decides
  if (!why.empty())
    return why;
  if (t.crt.d > GF_MAX_D) {
    snprintf(msg, sizeof msg, "d = ord_m(p) = %u for m = %llu, p = %llu: slots in GF(p^d) are built for d <= %u", t.crt.d,
             (unsigned long long)m, (unsigned long long)prime, GF_MAX_D);
    return msg;
  }
  why = build_crt(m, prime, t.crt, true, r, sup_gens, sup_ords);
  if (!why.empty())
    return why;
  const CrtTables& c = t.crt;
  const uint64_t p = c.modulus;   // p^r: what every table below is a residue of
  const uint32_t d = c.d, n = c.nslots, phim = c.phim, ld = c.ld;
  t.ldr = (phim + d - 1 + 3) / 4 * 4;
  t.G.assign(c.factors.begin(), c.factors.begin() + d + 1);

  // Rx: the recurrence of bgv_crt.h's R, d - 1 words further
  t.Rx.assign((size_t)n * t.ldr, 0);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t* f = c.factors.data() + (size_t)i * (d + 1);
    uint32_t* r = t.Rx.data() + (size_t)i * t.ldr;
    r[0] = 1 % p;
    for (uint32_t k = d; k < phim + d - 1; k++) {
      hxh::u128 s = 0;
      for (uint32_t j = 0; j < d; j++)
        s += (uint64_t)f[j] * r[k - d + j];
      const uint64_t v = (uint64_t)(s % p);
      r[k] = (uint32_t)(v ? p - v : 0);
    }
  }

  // T_u = X^(phi(m) + u) mod Phi_m.  Phi_m = prod (1 - x^e)^(+-1) as a power series cut at x^phi(m) (it is a polynomial
  // of that degree with constant term 1, m >= 2); T_0 = X^phi(m) - Phi_m, T_(u+1) = X T_u mod Phi_m
  if (d > 1) {
    const PhiBinomials pb(m);
    std::vector<uint32_t> phi(phim + 1, 0);
    phi[0] = 1 % p;
    for (uint64_t e : pb.num)
      mul_binomial(phi.data(), phim + 1, e, (uint32_t)p);
    for (uint64_t e : pb.den)
      div_binomial(phi.data(), phim + 1, e, (uint32_t)p);
    if (phi[phim] != 1 % p)
      return "internal: Phi_m mod p is not monic of degree phi(m)";
    t.T.assign((size_t)(d - 1) * ld, 0);
    for (uint32_t k = 0; k < phim; k++)
      t.T[k] = phi[k] ? (uint32_t)(p - phi[k]) : 0;
    for (uint32_t u = 1; u + 1 < d; u++) {
      const uint32_t* prev = t.T.data() + (size_t)(u - 1) * ld;
      uint32_t* cur = t.T.data() + (size_t)u * ld;
      const uint64_t top = prev[phim - 1];
      for (uint32_t k = 0; k < phim; k++)
        cur[k] = (uint32_t)(((k ? prev[k - 1] : 0) + top * t.T[k]) % p);
    }
  }

  // A_i and M_i, slot by slot in hypercube order (the last generator's exponent fastest, as build_crt numbers them)
  t.A.assign((size_t)n * d * d, 0);
  t.M.assign((size_t)n * d * d, 0);
  const size_t ng = c.gens.size();
  std::vector<uint64_t> ex(ng, 0), ao(ng);
  for (size_t g = 0; g < ng; g++)
    ao[g] = (uint64_t)(c.ords[g] < 0 ? -c.ords[g] : c.ords[g]);
  std::vector<uint32_t> x(d), step(d), tmp(d);
  std::vector<uint64_t> U((size_t)d * d);
  for (uint32_t i = 0; i < n; i++) {
    uint64_t ti = 1 % m;
    for (size_t g = 0; g < ng; g++)
      ti = ti * hxh::powmod(c.gens[g], ex[g], m) % m;
    const uint32_t* f = c.factors.data() + (size_t)i * (d + 1);
    uint32_t* A = t.A.data() + (size_t)i * d * d;
    if (d == 1) {
      A[0] = 1 % p;
      t.M[i] = 1 % p;
    } else {
      // step = X^(t_i) mod F_i by square and multiply
      std::fill(step.begin(), step.end(), 0u);
      step[0] = 1;
      std::fill(x.begin(), x.end(), 0u);
      x[1] = 1;
      for (uint64_t e = ti; e; e >>= 1) {
        if (e & 1) {
          gf_mulmod(step.data(), x.data(), f, d, p, tmp.data());
          step = tmp;
        }
        gf_mulmod(x.data(), x.data(), f, d, p, tmp.data());
        x = tmp;
      }
      A[0] = 1;
      for (uint32_t l = 1; l < d; l++)
        gf_mulmod(A + (size_t)(l - 1) * d, step.data(), f, d, p, A + (size_t)l * d);
      // u = alpha U with U[l][j] = sum_k A[l][k] Rx_i[k + j]; alpha = M u as columns: M = (U^T)^-1
      const uint32_t* r = t.Rx.data() + (size_t)i * t.ldr;
      for (uint32_t l = 0; l < d; l++)
        for (uint32_t j = 0; j < d; j++) {
          uint64_t s = 0;
          for (uint32_t k = 0; k < d; k++)
            s = (s + (uint64_t)A[(size_t)l * d + k] * r[k + j]) % p;
          U[(size_t)j * d + l] = s;   // transposed
        }
      if (!gf_invert(U, d, p, t.M.data() + (size_t)i * d * d, prime))
        return "internal: the map from a slot to its d constant terms is singular";
    }
    for (size_t g = ng; g-- > 0;) {
      if (++ex[g] < ao[g])
        break;
      ex[g] = 0;
    }
  }
  return "";
}

}  // namespace hxc
