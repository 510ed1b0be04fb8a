// bgv_crt.h -- host tables of BGV slot encoding and decoding for any d = ord_m(p), slots in Z_p (r = 1) or Z_(p^r): the
// default-constructed EncryptedArray (G = X, include/helib/EncryptedArray.h) over PAlgebraModDerived's constructor
// (src/PAlgebra.cpp:680-772), restated without factoring polynomials.  Plain C++ (no device code): product code, unit
// tested on the CPU like hostmath.h.
//
//   field      GF(p^d) = Z_p[y] / g, g any irreducible of degree d (Rabin's test on pseudo-random monic polynomials);
//              zeta of order m: a^((p^d - 1) / m) for the first pseudo-random a whose power has order exactly m
//   factors    of Phi_m mod p: prod_(k < d) (X - zeta^(j p^k)) over the cosets j<p> of Z_m^*; F_0 the smallest by
//              poly_comp (:67-81: coefficients from the constant one up, compared as residues); F_i the minimal
//              polynomial of X^(1/t_i) mod F_0 (:726-733): the factor of the coset c / t_i, c<p> the coset of F_0,
//              t_i = ith_rep(i) in hypercube order
//   E (encode) row i the idempotent E_i = 1 mod F_i, 0 mod F_j (CRT_reconstruct of constants, :1007-1045, with
//              crtCoeffs :750-756).  Modulo X^m - 1 its coefficients are (1/m) Tr(zeta_i^-k), zeta_i a root of F_i --
//              one lookup in a table of m traces -- and the reduction mod Phi_m is a handful of running sums, since
//              Phi_m = prod_(s | rad m) (X^(m/s) - 1)^mu(s) is a quotient of products of binomials (rem_phi below)
//   R (decode) R_i[k] = the constant term of X^k mod F_i (CRT_decompose :885-936 and decodePlaintext's degG == 1
//              branch :1243-1261): the sequence satisfies the recurrence whose characteristic polynomial is F_i
// so  encode: H[k] = sum_i a_i E[i][k] mod p   and   decode: slot i = sum_k w[k] R[i][k] mod p.
// Rows are ld = phi(m) rounded up to 4 words apart (zero filled), so that a row starts on a 16-byte boundary.
//
// r > 1 (slots in Z_(p^r)): the r > 1 branch of the same constructor (src/PAlgebra.cpp:757-763), where the factors
// found and ordered modulo p (:705-733) are Hensel-lifted by PAlgebraLift (:840-881).  No polynomial is lifted by hand
// here: the work moves to the Galois ring GR(p^r, d) = Z_(p^r)[y] / g with the same monic g (any lift of an
// irreducible serves), and zeta is replaced by its Teichmueller lift  zeta~ = a^(p^(d (r - 1))),  a any lift of zeta:
// it reduces to zeta (zeta^(p^d) = zeta) and has zeta~^m = 1 (a^m = 1 + p u, and (1 + p u)^(p^(r-1)) = 1 mod p^r).
// The Frobenius lift maps zeta~ to zeta~^p, so prod_k (X - zeta~^(j p^k)) over a coset has coefficients in Z_(p^r),
// divides X^m - 1 and reduces to F_i: it is the Hensel lift of F_i (which is unique).  E and R are the same formulas
// modulo p^r; poly_comp still compares residues modulo p.  At r = 1 every step is the one above, word for word.
#pragma once
#include <stdint.h>

#include <cstdio>
#include <string>
#include <vector>

#include "hostmath.h"

namespace hxc {

constexpr uint64_t CRT_MAX_P = 1ull << 31;            // table words are uint32 and a product of two fits 62 bits (bounds p^r)
constexpr uint64_t CRT_MAX_TABLE_BYTES = 1ull << 30;  // each of E and R

struct CrtTables {
  uint64_t m = 0, p = 0;
  uint32_t r = 1;
  uint64_t modulus = 0;                 // p^r: what the words of E, R and the factors are residues of
  uint32_t d = 0, nslots = 0, phim = 0, ld = 0;
  uint64_t limit = 0;                   // terms a 64-bit accumulator takes between reductions: floor(2^64 / p^(2r))
  std::vector<uint64_t> gens;
  std::vector<int64_t> ords;            // signed: a non-native dimension's order negated
  std::vector<uint32_t> factors;        // [nslots][d + 1], constant coefficient first
  std::vector<uint32_t> E, R;           // [nslots][ld]
};

inline uint64_t lazy_limit(uint64_t p)
{
  const hxh::u128 l = ((hxh::u128)1 << 64) / ((hxh::u128)p * p);
  return l > 0xffffffffu ? 0xffffffffu : (uint64_t)l;
}

// ---- Z_m^* / <p> (findGenerators, src/NumbTh.cpp:276-430; the python twin is hostnt.find_generators) ----
inline void conj_classes(std::vector<uint32_t>& cl, uint64_t g, uint64_t m)
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
inline void find_generators(uint64_t m, uint64_t p, std::vector<uint64_t>& gens, std::vector<int64_t>& ords)
{
  std::vector<uint32_t> cl(m), order(m);
  for (uint64_t i = 0; i < m; i++)
    cl[i] = hxh::gcd(i, m) == 1 ? (uint32_t)i : 0;
  conj_classes(cl, p % m, m);
  std::vector<uint8_t> in_p(m);
  for (uint64_t i = 0; i < m; i++)
    in_p[i] = cl[i] == 1;
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
    int quality = 0;
    for (uint64_t i = 0; i < m && quality < 2; i++)
      if (order[i] == largest) {
        const uint64_t j = hxh::powmod(i, largest, m);
        if (j == 1) {
          best = i;
          quality = 2;
        } else if (quality < 1 && in_p[j]) {
          best = i;
          quality = 1;
        }
      }
    if (!best)
      break;
    gens.push_back(best);
    ords.push_back(hxh::powmod(best, largest, m) == 1 ? (int64_t)largest : -(int64_t)largest);
    conj_classes(cl, best, m);
  }
}

// ---- polynomials over Z_p, coefficients lowest first, p < 2^31 (Field::mul and poly_rem take any modulus) ----
typedef std::vector<uint64_t> Poly;

inline void trim(Poly& a)
{
  while (!a.empty() && a.back() == 0)
    a.pop_back();
}
// a mod the monic g
inline void poly_rem(Poly& a, const Poly& g, uint64_t p)
{
  const size_t dg = g.size() - 1;
  for (size_t i = a.size(); i-- > dg;) {
    const uint64_t c = a[i];
    if (c)
      for (size_t j = 0; j <= dg; j++)
        a[i - dg + j] = (a[i - dg + j] + (p - c) * g[j]) % p;
  }
  if (a.size() > dg)
    a.resize(dg);
  trim(a);
}
inline Poly poly_gcd(Poly a, Poly b, uint64_t p)
{
  trim(a);
  trim(b);
  while (!b.empty()) {
    const uint64_t inv = hxh::invmod(b.back(), p);
    for (auto& x : b)
      x = x * inv % p;
    poly_rem(a, b, p);
    std::swap(a, b);
  }
  return a;
}

// GF(p^d) = Z_p[y] / g: elements are d words.  With p a prime power and g irreducible modulo the prime the same code
// is the Galois ring GR(p, d) (mul, one, pow, is_one; is_irreducible and poly_gcd are for a prime only)
struct Field {
  uint64_t p = 0;
  uint32_t d = 0;
  Poly g;   // monic, d + 1 words
  Poly mul(const Poly& a, const Poly& b) const
  {
    std::vector<hxh::u128> acc(2 * d - 1, 0);
    for (uint32_t i = 0; i < d; i++)
      if (a[i])
        for (uint32_t j = 0; j < d; j++)
          acc[i + j] += (hxh::u128)a[i] * b[j];
    Poly r(2 * d - 1);
    for (uint32_t i = 0; i < 2 * d - 1; i++)
      r[i] = (uint64_t)(acc[i] % p);
    for (uint32_t i = 2 * d - 1; i-- > d;) {
      const uint64_t c = r[i];
      if (c)
        for (uint32_t j = 0; j < d; j++)
          r[i - d + j] = (r[i - d + j] + (p - c) * g[j]) % p;
    }
    r.resize(d);
    return r;
  }
  Poly one() const
  {
    Poly r(d, 0);
    r[0] = 1 % p;
    return r;
  }
  // a^e, e given as 64-bit limbs, lowest first
  Poly pow(const Poly& a, const std::vector<uint64_t>& e) const
  {
    Poly r = one();
    for (size_t i = e.size(); i-- > 0;)
      for (int b = 63; b >= 0; b--) {
        r = mul(r, r);
        if ((e[i] >> b) & 1)
          r = mul(r, a);
      }
    return r;
  }
  Poly pow(const Poly& a, uint64_t e) const { return pow(a, std::vector<uint64_t>(1, e)); }
  bool is_one(const Poly& a) const
  {
    for (uint32_t i = 1; i < d; i++)
      if (a[i])
        return false;
    return a[0] == 1 % p;
  }
};

inline uint64_t splitmix(uint64_t& s)
{
  uint64_t z = (s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
inline std::vector<uint64_t> prime_factors(uint64_t x)
{
  std::vector<uint64_t> f;
  for (uint64_t q = 2; q * q <= x; q++)
    if (x % q == 0) {
      f.push_back(q);
      while (x % q == 0)
        x /= q;
    }
  if (x > 1)
    f.push_back(x);
  return f;
}

// Rabin: the monic g of degree d is irreducible iff y^(p^d) = y mod g and gcd(y^(p^(d/q)) - y, g) = 1 for every
// prime q | d
inline bool is_irreducible(const Field& F)
{
  const uint32_t d = F.d;
  Poly y(d, 0);
  y[1] = 1;
  std::vector<Poly> frob(d + 1);   // y^(p^k)
  frob[0] = y;
  for (uint32_t k = 1; k <= d; k++)
    frob[k] = F.pow(frob[k - 1], F.p);
  if (frob[d] != y)
    return false;
  for (uint64_t q : prime_factors(d)) {
    Poly t = frob[d / q];
    t[1] = (t[1] + F.p - 1) % F.p;
    if (poly_gcd(F.g, t, F.p).size() != 1)
      return false;
  }
  return true;
}
inline Field make_field(uint64_t p, uint32_t d, uint64_t& seed)
{
  Field F;
  F.p = p;
  F.d = d;
  F.g.assign(d + 1, 0);
  F.g[d] = 1;
  if (d == 1)
    return F;   // Z_p[y] / y
  for (;;) {
    for (uint32_t i = 0; i < d; i++)
      F.g[i] = splitmix(seed) % p;
    if (F.g[0] && is_irreducible(F))
      return F;
  }
}

// X mod Phi_m for X of m words (degree < m), in place; the first phi(m) words are the remainder.  With n = phi(m),
// dq = m - 1 - n, t = 1/x: the reversed quotient is Xr / Phi_m(t) mod t^(dq+1) (Phi_m is palindromic and
// 1 / (1 - t^m) = 1 there), W = Q Phi_m mod x^n and the remainder X_low - W.  Multiplying by 1 - x^e is
// w_i -= w_(i-e), dividing by it the running sum w_i += w_(i-e).  num / den: the e with mu(m / e) = +1 / -1, m left out.
struct PhiBinomials {
  std::vector<uint64_t> num, den;
  explicit PhiBinomials(uint64_t m)
  {
    const std::vector<uint64_t> ps = prime_factors(m);
    for (uint32_t mask = 1; mask < (1u << ps.size()); mask++) {   // s = 1 is x^m - 1 itself
      uint64_t s = 1;
      int bits = 0;
      for (size_t i = 0; i < ps.size(); i++)
        if (mask >> i & 1) {
          s *= ps[i];
          bits++;
        }
      (bits % 2 ? den : num).push_back(m / s);
    }
  }
};
inline void mul_binomial(uint32_t* w, size_t n, size_t e, uint32_t p)
{
  for (size_t i = n; i-- > e;)
    w[i] = w[i] >= w[i - e] ? w[i] - w[i - e] : w[i] + p - w[i - e];
}
inline void div_binomial(uint32_t* w, size_t n, size_t e, uint32_t p)
{
  for (size_t i = e; i < n; i++) {
    const uint64_t s = (uint64_t)w[i] + w[i - e];
    w[i] = (uint32_t)(s >= p ? s - p : s);
  }
}
inline void rem_phi(std::vector<uint32_t>& X, uint64_t m, uint32_t n, uint32_t p, const PhiBinomials& pb,
                    std::vector<uint32_t>& w)
{
  const size_t dq = m - 1 - n;
  w.assign(std::max<size_t>(dq + 1, n), 0);
  for (size_t k = 0; k <= dq; k++)
    w[k] = X[m - 1 - k];
  for (uint64_t e : pb.den)
    mul_binomial(w.data(), dq + 1, e, p);
  for (uint64_t e : pb.num)
    div_binomial(w.data(), dq + 1, e, p);
  // W = reversed(w), cut or zero filled to n words
  std::vector<uint32_t> W(n, 0);
  for (size_t k = 0; k < n && k <= dq; k++)
    W[k] = w[dq - k];
  for (uint64_t e : pb.num)
    mul_binomial(W.data(), n, e, p);
  for (uint64_t e : pb.den)
    div_binomial(W.data(), n, e, p);
  for (size_t i = 0; i < n; i++)
    X[i] = X[i] >= W[i] ? X[i] - W[i] : X[i] + p - W[i];
}

// p^r, or 0 when it is not below CRT_MAX_P (or r < 1)
inline uint64_t crt_modulus(uint64_t p, uint32_t r)
{
  uint64_t P = 1;
  for (uint32_t i = 0; i < r; i++) {
    if (p < 2 || P > (CRT_MAX_P - 1) / p)
      return 0;
    P *= p;
  }
  return r < 1 ? 0 : P;
}

// 0, or the reason the tables cannot be built.  tables = false: the geometry alone (m, p, d, nslots, gens, ords).
// r: the tables are modulo p^r (the top of this file).
// sup_gens / sup_ords (both or neither): the hypercube follows these generators instead of find_generators', as
// PAlgebra's constructor takes them from ContextBuilder.gens().ords() (src/PAlgebra.cpp:476-507): a supplied sign is
// not trusted -- the order is |ords[i]| and nativeness is recomputed -- and what the caller got wrong is reported with
// a message that starts with "generators:".
constexpr size_t CRT_MAX_GENS = 8;   // what hx_bgv_crt_info / hx_bgv_gf_info write
inline std::string build_crt(uint64_t m, uint64_t p, CrtTables& t, bool tables = true, uint32_t r = 1,
                             const std::vector<uint64_t>* sup_gens = nullptr, const std::vector<int64_t>* sup_ords = nullptr)
{
  char msg[200];
  const bool supplied = sup_gens && sup_ords && !sup_gens->empty();
  if (p < 2 || !hxh::is_prime(p))
    return "the plaintext modulus is not a prime";
  if (r < 1)
    return "the exponent r of the plaintext space p^r is less than 1";
  if (p >= CRT_MAX_P) {
    snprintf(msg, sizeof msg, "p = %llu: the CRT tables hold 32-bit words and take p < 2^31 = %llu", (unsigned long long)p,
             (unsigned long long)CRT_MAX_P);
    return msg;
  }
  const uint64_t P = crt_modulus(p, r);
  if (!P) {
    snprintf(msg, sizeof msg, "p^r = %llu^%u: the CRT tables hold 32-bit words and take p^r < 2^31 = %llu",
             (unsigned long long)p, r, (unsigned long long)CRT_MAX_P);
    return msg;
  }
  if (m < 2 || m >= (1ull << 24) || hxh::gcd(m, p) != 1)
    return "p divides m, or m is not in [2, 2^24)";
  t = CrtTables();
  t.m = m;
  t.p = p;
  t.r = r;
  t.modulus = P;
  t.limit = lazy_limit(P);
  uint32_t phim = 0;
  for (uint64_t j = 0; j < m; j++)
    phim += hxh::gcd(j, m) == 1;
  uint32_t d = 1;
  for (uint64_t x = p % m; x != 1 % m; x = x * (p % m) % m)
    d++;
  t.d = d;
  t.phim = phim;
  t.nslots = phim / d;
  t.ld = (phim + 3) / 4 * 4;
  if (supplied) {
    const size_t ng = sup_gens->size();
    if (ng != sup_ords->size() || ng > CRT_MAX_GENS) {
      snprintf(msg, sizeof msg, "generators: %zu generators with %zu orders; at most %zu of each are taken", ng, sup_ords->size(),
               CRT_MAX_GENS);
      return msg;
    }
    uint64_t cube = 1;
    for (size_t i = 0; i < ng; i++) {
      const uint64_t g = (*sup_gens)[i] % m;
      const int64_t so = (*sup_ords)[i];
      const uint64_t o = (uint64_t)(so < 0 ? -so : so);
      if (hxh::gcd(g, m) != 1) {
        snprintf(msg, sizeof msg, "generators: generator %zu = %llu is not coprime to m = %llu", i, (unsigned long long)(*sup_gens)[i],
                 (unsigned long long)m);
        return msg;
      }
      if (o < 1 || o > phim || cube * o > phim) {
        snprintf(msg, sizeof msg, "generators: order %zu = %lld does not fit a hypercube of phi(m) / d = %u points", i, (long long)so,
                 t.nslots);
        return msg;
      }
      cube *= o;
      t.gens.push_back(g);
      t.ords.push_back(hxh::powmod(g, o, m) == 1 ? (int64_t)o : -(int64_t)o);
    }
    if (cube != t.nslots) {
      snprintf(msg, sizeof msg, "generators: the orders multiply to %llu, Z_m^* / <p> has phi(m) / d = %u elements",
               (unsigned long long)cube, t.nslots);
      return msg;
    }
    // the exponent vectors enumerate Z_m^* / <p> exactly once: every representative lands in a coset of its own
    std::vector<uint8_t> seen(m, 0);
    std::vector<uint64_t> ex(ng, 0);
    for (uint32_t i = 0; i < t.nslots; i++) {
      uint64_t ti = 1 % m;
      for (size_t g = 0; g < ng; g++)
        ti = ti * hxh::powmod(t.gens[g], ex[g], m) % m;
      if (seen[ti]) {
        snprintf(msg, sizeof msg, "generators: the representatives do not enumerate Z_m^* / <p> once: point %u = %llu falls in "
                 "the coset of an earlier one (m = %llu, p = %llu)", i, (unsigned long long)ti, (unsigned long long)m,
                 (unsigned long long)p);
        return msg;
      }
      uint64_t x = ti;
      for (uint32_t k = 0; k < d; k++, x = x * (p % m) % m)
        seen[x] = 1;
      for (size_t g = ng; g-- > 0;) {
        if (++ex[g] < (uint64_t)(t.ords[g] < 0 ? -t.ords[g] : t.ords[g]))
          break;
        ex[g] = 0;
      }
    }
  } else {
    find_generators(m, p, t.gens, t.ords);
    uint64_t cube = 1;
    for (int64_t o : t.ords)
      cube *= (uint64_t)(o < 0 ? -o : o);
    if (cube != t.nslots)
      return "internal: the hypercube of Z_m^* / <p> does not have phi(m) / d points";
  }
  if (!tables)
    return "";
  const uint64_t bytes = (uint64_t)t.nslots * t.ld * 4;
  if (bytes > CRT_MAX_TABLE_BYTES) {
    snprintf(msg, sizeof msg, "a CRT table of %u slots x %u coefficients takes %llu bytes, above the limit of %llu", t.nslots,
             phim, (unsigned long long)bytes, (unsigned long long)CRT_MAX_TABLE_BYTES);
    return msg;
  }
  const uint32_t n = t.nslots;

  // the field and zeta
  uint64_t seed = m * 0x100000001b3ull + p;
  const Field F = make_field(p, d, seed);
  hxh::BigU e(1);
  for (uint32_t i = 0; i < d; i++)
    e.mul_word(p);
  e.sub_word(1);
  if (e.divmod_word(m) != 0)
    return "internal: m does not divide p^d - 1";
  const std::vector<uint64_t> mf = prime_factors(m);
  Poly zeta;
  for (;;) {
    Poly a(d);
    for (auto& x : a)
      x = splitmix(seed) % p;
    zeta = F.pow(a, e.d);
    bool ok = F.is_one(F.pow(zeta, m));   // (fails only for a = 0)
    for (size_t i = 0; ok && i < mf.size(); i++)
      ok = !F.is_one(F.pow(zeta, m / mf[i]));
    if (ok)
      break;
  }
  // from here on modulo P = p^r in G = Z_P[y] / g (r = 1: G is F and nothing changes); zeta becomes its Teichmueller
  // lift a^(p^(d (r - 1))), a = zeta's own words
  Field G = F;
  G.p = P;
  if (r > 1) {
    hxh::BigU te(1);
    for (uint32_t i = 0; i < d * (r - 1); i++)
      te.mul_word(p);
    zeta = G.pow(zeta, te.d);
    if (!G.is_one(G.pow(zeta, m)))
      return "internal: the lifted root of unity does not have order m";
  }
  std::vector<uint64_t> zp((size_t)m * d);   // zeta^j
  {
    Poly cur = G.one();
    for (uint64_t j = 0; j < m; j++) {
      std::copy(cur.begin(), cur.end(), zp.begin() + j * d);
      cur = G.mul(cur, zeta);
    }
  }
  // traces: Tr(zeta^j) = sum_k zeta^(j p^k), an element of Z_P (its constant coordinate; the others cancel)
  std::vector<uint32_t> tr(m);
  for (uint64_t j = 0; j < m; j++) {
    uint64_t s = 0, x = j;
    for (uint32_t k = 0; k < d; k++, x = x * (p % m) % m)
      s += zp[x * d];
    tr[j] = (uint32_t)(s % P);
  }
  // the factor of every coset j<p> of Z_m^*, kept under its smallest element
  std::vector<uint32_t> coset(m, 0xffffffffu);
  std::vector<std::vector<uint32_t>> fac(m);
  uint64_t c0 = 0;
  for (uint64_t j = 1; j < m; j++) {
    if (hxh::gcd(j, m) != 1 || coset[j] != 0xffffffffu)
      continue;
    std::vector<Poly> f(1, G.one());   // the running product, coefficients in the field
    uint64_t x = j;
    for (uint32_t k = 0; k < d; k++, x = x * (p % m) % m) {
      coset[x] = (uint32_t)j;
      const Poly root(zp.begin() + x * d, zp.begin() + (x + 1) * d);
      f.push_back(G.one());   // times (X - root): f[i] = f[i - 1] - root f[i]
      for (size_t i = f.size() - 1; i-- > 0;) {
        Poly pr = G.mul(f[i], root);
        for (uint32_t c = 0; c < d; c++)
          pr[c] = ((i > 0 ? f[i - 1][c] : 0) + P - pr[c]) % P;
        f[i] = pr;
      }
    }
    std::vector<uint32_t>& out = fac[j];
    out.resize(d + 1);
    for (uint32_t i = 0; i <= d; i++) {
      for (uint32_t c = 1; c < d; c++)
        if (f[i][c])
          return "internal: a factor of Phi_m has a coefficient outside Z_p";
      out[i] = (uint32_t)f[i][0];
    }
    // poly_comp: equal degrees, so the first differing coefficient from the constant one up decides -- of the factors
    // modulo p, which is where the reference orders them (:715-721) before it lifts
    if (!c0 || std::lexicographical_compare(out.begin(), out.end(), fac[c0].begin(), fac[c0].end(),
                                            [p](uint32_t a, uint32_t b) { return a % p < b % p; }))
      c0 = j;
  }
  // slot i: the coset of c0 / t_i, t_i = ith_rep(i) (the last generator's exponent fastest)
  const size_t ng = t.gens.size();
  std::vector<uint64_t> ex(ng, 0), ao(ng);
  for (size_t g = 0; g < ng; g++)
    ao[g] = (uint64_t)(t.ords[g] < 0 ? -t.ords[g] : t.ords[g]);
  t.factors.assign((size_t)n * (d + 1), 0);
  t.E.assign((size_t)n * t.ld, 0);
  t.R.assign((size_t)n * t.ld, 0);
  const uint64_t minv = hxh::invmod(m % P, P);
  const PhiBinomials pb(m);
  std::vector<uint32_t> X(m), scratch;
  std::vector<uint8_t> seen(m, 0);
  for (uint32_t i = 0; i < n; i++) {
    uint64_t ti = 1 % m;
    for (size_t g = 0; g < ng; g++)
      ti = ti * hxh::powmod(t.gens[g], ex[g], m) % m;
    const uint64_t u = c0 * hxh::invmod(ti, m) % m;   // zeta^u is a root of F_i
    const uint32_t cs = coset[u];
    if (cs == 0xffffffffu || seen[cs])
      return supplied ? "generators: the representatives of Z_m^* / <p> do not reach every factor once"
                      : "internal: the representatives of Z_m^* / <p> do not reach every factor once";
    seen[cs] = 1;
    const std::vector<uint32_t>& f = fac[cs];
    std::copy(f.begin(), f.end(), t.factors.begin() + (size_t)i * (d + 1));
    // E_i mod X^m - 1: (1/m) Tr(zeta^(-k u)), then mod Phi_m
    uint64_t at = 0;   // -k u mod m
    for (uint64_t k = 0; k < m; k++) {
      X[k] = (uint32_t)(tr[at] * minv % P);
      at = at >= u ? at - u : at + m - u;
    }
    rem_phi(X, m, phim, (uint32_t)P, pb, scratch);
    std::copy(X.begin(), X.begin() + phim, t.E.begin() + (size_t)i * t.ld);
    // R_i[k] = [X^0] (X^k mod F_i): R[k + d] = -sum_j f_j R[k + j], from 1, 0, ..., 0
    uint32_t* rw = t.R.data() + (size_t)i * t.ld;
    rw[0] = 1 % P;
    for (uint32_t k = d; k < phim; k++) {
      hxh::u128 s = 0;
      for (uint32_t j = 0; j < d; j++)
        s += (uint64_t)f[j] * rw[k - d + j];
      const uint64_t v = (uint64_t)(s % P);
      rw[k] = (uint32_t)(v ? P - v : 0);
    }
    // the next exponent vector
    for (size_t g = ng; g-- > 0;) {
      if (++ex[g] < ao[g])
        break;
      ex[g] = 0;
    }
  }
  return "";
}

}  // namespace hxc
