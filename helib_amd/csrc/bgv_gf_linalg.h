// bgv_gf_linalg.h -- host tables of linear maps on slots in GF(p^d) = Z_p[X] / G (G = F_0, r = 1): what
// EncryptedArrayDerived::buildLinPolyCoeffs (src/EncryptedArray.cpp:760-798) and buildLinPolyMatrix
// (src/NumbTh.cpp:1099-1111) keep as linPolyMatrix.  Plain C++ (no device code), on top of bgv_gf.h's field arithmetic.
//
//   frob (d x d x d)   frob[e][l] = X^(l p^e) mod G: alpha^(p^e) = sum_l alpha_l frob[e][l]
//   M (d x d over the field)   M[i][j] = (X^j)^(p^i) = frob[i][j]                  (buildLinPolyMatrix)
//   K = M^-1           K[j][k] = beta_j^(p^k), beta the dual basis of 1, X, .., X^(d-1) under the trace: M is a Moore matrix
//                      and (K M)[j][j'] = sum_k (beta_j X^j')^(p^k) = Tr(beta_j X^j').  beta comes from the d x d Gram matrix
//                      Tr(X^(i+j)) over Z_p, so the whole inverse costs d^4 word operations where Gauss-Jordan over the field
//                      costs d^5; it is the same matrix (an inverse is unique) and the tests multiply it back.
//   T (d^2 x d^2)      T[(j,b)][(k,c)] = [X^c](X^b K[j][k] mod G).  The linearized polynomial of the Z_p-linear map with
//                      L[j] = image of X^j = sum_b E[j][b] X^b has C[k] = sum_j L[j] K[j][k], i.e. C = E T as flat vectors of
//                      d^2 words: the product the device forms for every entry of a block matrix.
//
// Modulo P = p^r (build_gr_linalg): slots in the Galois ring Z_P[X] / G, G the Hensel lift of F_0.  sigma: X -> X^p is a
// ring automorphism (it fixes the lifted F_0) that fixes Z_P, so frob[e][l] = X^(l p^e) mod G mod P still gives
// sigma^e(alpha) = sum_l alpha_l frob[e][l]; M stays a Moore matrix of sigma and K its inverse over the ring, through the
// same Gram matrix Tr(X^(i+j)), Tr = sum_e sigma^e, which is invertible modulo P because it is modulo p: gf_invert takes
// pivots that are units.  Every line is the r = 1 line with P where it says p, and X^p keeps the prime in the exponent;
// the tables reduced mod p are the r = 1 tables.
#pragma once
#include "bgv_gf.h"

namespace hxc {

struct GfLinTables {
  uint32_t d = 0;
  uint64_t p = 0;               // the modulus of the words: the prime, or p^r
  uint64_t limit = 0;           // lazy_limit(p): multiply-adds a 64-bit accumulator takes between reductions
  std::vector<uint32_t> frob;   // [d][d][d]
  std::vector<uint32_t> K;      // [d][d][d]: K[j][k], d words each
  std::vector<uint32_t> T;      // [d^2][d^2]
};

// a <- X a mod the monic G of degree d (d > 1)
inline void gf_mulx(uint32_t* a, const uint32_t* G, uint32_t d, uint64_t p)
{
  const uint64_t c = a[d - 1];
  for (uint32_t i = d - 1; i > 0; i--)
    a[i] = (uint32_t)((a[i - 1] + (p - c) * G[i]) % p);
  a[0] = (uint32_t)((p - c) * G[0] % p);
}

// "", or the reason the tables cannot be built.  G: d + 1 words below p = prime^r, monic, irreducible modulo the prime
// (prime = 0: p itself is the prime).
inline std::string build_gf_linalg(const uint32_t* G, uint32_t d, uint64_t p, GfLinTables& t, uint64_t prime = 0)
{
  t = GfLinTables();
  if (!prime)
    prime = p;
  if (d < 1 || d > GF_MAX_D || p < 2 || p >= CRT_MAX_P || G[d] != 1)
    return "linear maps on GF(p^d) slots take a monic G of degree d <= 64 and p < 2^31";
  t.d = d;
  t.p = p;
  t.limit = lazy_limit(p);
  const size_t dd = (size_t)d * d;
  t.frob.assign(dd * d, 0);
  t.K.assign(dd * d, 0);
  t.T.assign(dd * dd, 0);
  if (d == 1) {   // the field is Z_p
    t.frob[0] = t.K[0] = t.T[0] = (uint32_t)(1 % p);
    return "";
  }
  std::vector<uint32_t> x(d, 0), xp(d, 0), tmp(d);
  x[1] = 1;
  xp[0] = 1;
  for (uint64_t e = prime; e; e >>= 1) {   // xp = X^p mod G (the prime in the exponent, whatever r)
    if (e & 1) {
      gf_mulmod(xp.data(), x.data(), G, d, p, tmp.data());
      xp = tmp;
    }
    gf_mulmod(x.data(), x.data(), G, d, p, tmp.data());
    x = tmp;
  }
  // frob[0] = identity; frob[1][l] = xp^l; frob[e][l] = the Frobenius of frob[e - 1][l]
  for (uint32_t l = 0; l < d; l++)
    t.frob[(size_t)l * d + l] = 1;
  uint32_t* f1 = t.frob.data() + dd;
  f1[0] = 1;
  for (uint32_t l = 1; l < d; l++)
    gf_mulmod(f1 + (size_t)(l - 1) * d, xp.data(), G, d, p, f1 + (size_t)l * d);
  const auto frobenius = [&](const uint32_t* v, uint32_t* out) {
    for (uint32_t c = 0; c < d; c++) {
      uint64_t s = 0;
      for (uint32_t l = 0; l < d; l++)
        s = (s + (uint64_t)v[l] * f1[(size_t)l * d + c]) % p;
      out[c] = (uint32_t)s;
    }
  };
  for (uint32_t e = 2; e < d; e++)
    for (uint32_t l = 0; l < d; l++)
      frobenius(t.frob.data() + ((size_t)(e - 1) * d + l) * d, t.frob.data() + ((size_t)e * d + l) * d);
  // tr[s] = Tr(X^s) = the trace of multiplying by X^s = sum_b [X^b](X^(s + b) mod G), s <= 2 d - 2
  std::vector<uint32_t> pw((size_t)(3 * d) * d, 0);   // X^s mod G, s < 3 d - 2
  pw[0] = 1;
  for (uint32_t s = 1; s + 2 < 3 * d; s++) {
    std::copy(pw.begin() + (size_t)(s - 1) * d, pw.begin() + (size_t)s * d, pw.begin() + (size_t)s * d);
    gf_mulx(pw.data() + (size_t)s * d, G, d, p);
  }
  std::vector<uint64_t> gram(dd);
  for (uint32_t i = 0; i < d; i++)
    for (uint32_t j = 0; j < d; j++) {
      uint64_t s = 0;
      for (uint32_t b = 0; b < d; b++)
        s += pw[(size_t)(i + j + b) * d + b];
      gram[(size_t)i * d + j] = s % p;
    }
  std::vector<uint32_t> beta(dd);   // row j: beta_j, Tr(beta_j X^i) = [i == j]
  if (!gf_invert(gram, d, p, beta.data(), prime))
    return "internal: the trace form of Z_p[X] / G is degenerate (G is not separable)";
  for (uint32_t j = 0; j < d; j++) {
    uint32_t* row = t.K.data() + (size_t)j * dd;
    std::copy(beta.begin() + (size_t)j * d, beta.begin() + (size_t)(j + 1) * d, row);
    for (uint32_t k = 1; k < d; k++)
      frobenius(row + (size_t)(k - 1) * d, row + (size_t)k * d);
  }
  for (uint32_t j = 0; j < d; j++)
    for (uint32_t k = 0; k < d; k++) {
      std::copy(t.K.begin() + ((size_t)j * d + k) * d, t.K.begin() + ((size_t)j * d + k + 1) * d, tmp.begin());
      for (uint32_t b = 0; b < d; b++) {
        if (b)
          gf_mulx(tmp.data(), G, d, p);
        std::copy(tmp.begin(), tmp.end(), t.T.begin() + ((size_t)j * d + b) * dd + (size_t)k * d);
      }
    }
  return "";
}

// The same tables modulo P = p^r over the Hensel-lifted G (d + 1 words below P): "", or the reason.  r = 1 is
// build_gf_linalg, byte for byte.
inline std::string build_gr_linalg(const uint32_t* G, uint32_t d, uint64_t p, uint32_t r, GfLinTables& t)
{
  t = GfLinTables();
  const uint64_t P = crt_modulus(p, r);
  if (!P)
    return "linear maps on Galois-ring slots take p^r < 2^31 with r >= 1";
  return build_gf_linalg(G, d, P, t, p);
}

}  // namespace hxc
