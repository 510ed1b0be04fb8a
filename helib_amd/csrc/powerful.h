// powerful.h -- host tables of the powerful basis: the isomorphism
//     Z_q[X] / Phi_m  ~  Z_q[X_1..X_k] / (Phi_m1(X_1), ..., Phi_mk(X_k)),   m = m_1 ... m_k pairwise coprime,
// X^i -> prod_j X_j^(i_j) with i = sum_j i_j (m / m_j) mod m: PowerfulTranslationIndexes and PowerfulConversion of
// src/powerful.cpp:22-244, restated without polynomial division.  Plain C++ (no device code): product code, unit tested
// on the CPU like bgv_crt.h.
//
//   p2c      exponent in [0, m) -> index in the long cube (m_1, ..., m_k), the last coordinate fastest (polyToCubeMap)
//   s2l      index in the short cube (phi(m_1), ..., phi(m_k)) -> index in the long cube (shortToLongMap)
//   s2e      short-cube index -> exponent (cubeToPolyMap o shortToLongMap)
//   to_powerful  scatter the phi(m) words by p2c into a zeroed long cube; for dimension i = 0..k-1 reduce every fibre
//            (length m_i, stride prod_(j>i) m_j) whose earlier coordinates are below phi(m_j) modulo Phi_(m_i)
//            (recursiveReduce, :114-150); gather by s2l
//   to_poly  scatter the phi(m) words by s2e into m zeroed words, one reduction modulo Phi_m of length m, keep the
//            first phi(m) words
// A reduction modulo Phi_n is bgv_crt.h's rem_phi: Phi_n = prod (1 - x^e)^(+-1) over e = n / s, s | rad n, so the
// quotient and the remainder take additions and subtractions only and the modulus q can be any integer in [2, 2^62)
// -- a 60-bit chain prime without Montgomery or Shoup constants, or p^e + 1.  Both directions are written down once as
// a list of passes over three buffers of m words (Program); the device kernel (powerful.hip) and replay() below
// execute that list, so the CPU tests check the schedule the device runs.
//
//   REV   dst[k] = src[n - 1 - k], k < L = n - phi(n)                      the reversed top of the fibre
//   MUL   dst[k] = src[k] - src[k - e] (k >= e), src[k] (k < e), k < L      times 1 - x^e, out of place: it reads old words
//   DIV   dst[k] += dst[k - e], k = e..L-1 in order                         by 1 - x^e: e independent running sums
//   REVW  dst[k] = src[e - k] (k <= e), 0 (k > e), k < L = phi(n)           the quotient, lowest word first (e = n - 1 - phi(n))
//   SUB   dst[k] -= src[k], k < L = phi(n)
// Word k of fibre f of dimension i sits at outer[o] + k stride + inner, f = o stride + inner, outer[] the long-cube
// offsets of the earlier coordinates (all below their phi(m_j)).
#pragma once
#include <stdint.h>

#include <cstdio>
#include <string>
#include <vector>

#include "bgv_crt.h"

namespace hxpw {

constexpr int MAX_FACTORS = 8;
constexpr uint64_t MAX_Q = 1ull << 62;   // a + b stays below 2^63

enum Op : uint32_t { OP_REV = 0, OP_MUL = 1, OP_DIV = 2, OP_REVW = 3, OP_SUB = 4 };

struct Dim {   // 8 words
  uint32_t n, phi, stride, nouter, outer_off, pad0, pad1, pad2;
};
struct Pass {   // 8 words; src / dst: 0 the cube, 1 and 2 the ping-pong pair
  uint32_t op, dim, e, L, src, dst, pad0, pad1;
};
struct Program {
  std::vector<Dim> dims;
  std::vector<uint32_t> outer;
  std::vector<Pass> passes;
};

struct Tables {
  uint64_t m = 0;
  uint32_t phim = 0;
  std::vector<uint64_t> mvec, phivec;
  std::vector<uint32_t> p2c, c2p;   // [m]
  std::vector<uint32_t> s2l, s2e;   // [phim]
  std::vector<hxc::PhiBinomials> binom;   // of m_0 .. m_(k-1), then of m
  Program to_powerful, to_poly;
};

inline uint64_t phi_of(uint64_t n)
{
  uint64_t r = n;
  for (uint64_t q : hxc::prime_factors(n))
    r = r / q * (q - 1);
  return r;
}

// the passes of one reduction modulo Phi_n of every fibre of dims[dim] (rem_phi of bgv_crt.h, pass for pass)
inline void push_rem_phi(Program& pr, uint32_t dim, const hxc::PhiBinomials& pb)
{
  const Dim& d = pr.dims[dim];
  const uint32_t dq = d.n - 1 - d.phi, Lq = dq + 1;
  uint32_t cur = 1;
  pr.passes.push_back(Pass{OP_REV, dim, 0, Lq, 0, cur, 0, 0});
  for (uint64_t e : pb.den)
    if (e < Lq) {
      pr.passes.push_back(Pass{OP_MUL, dim, (uint32_t)e, Lq, cur, 3 - cur, 0, 0});
      cur = 3 - cur;
    }
  for (uint64_t e : pb.num)
    if (e < Lq)
      pr.passes.push_back(Pass{OP_DIV, dim, (uint32_t)e, Lq, cur, cur, 0, 0});
  pr.passes.push_back(Pass{OP_REVW, dim, dq, d.phi, cur, 3 - cur, 0, 0});
  cur = 3 - cur;
  for (uint64_t e : pb.num)
    if (e < d.phi) {
      pr.passes.push_back(Pass{OP_MUL, dim, (uint32_t)e, d.phi, cur, 3 - cur, 0, 0});
      cur = 3 - cur;
    }
  for (uint64_t e : pb.den)
    if (e < d.phi)
      pr.passes.push_back(Pass{OP_DIV, dim, (uint32_t)e, d.phi, cur, cur, 0, 0});
  pr.passes.push_back(Pass{OP_SUB, dim, 0, d.phi, cur, 0, 0, 0});
}

// "", or why the factorisation is refused
inline std::string build(const uint64_t* mv, int k, Tables& t)
{
  char msg[200];
  t = Tables();
  if (!mv || k < 1 || k > MAX_FACTORS) {
    snprintf(msg, sizeof msg, "%d factors: between 1 and %d are taken", k, MAX_FACTORS);
    return msg;
  }
  uint64_t m = 1;
  for (int i = 0; i < k; i++) {
    if (mv[i] < 2 || mv[i] >= (1ull << 24) || m * mv[i] >= (1ull << 24)) {
      snprintf(msg, sizeof msg, "factor %d = %llu: every factor is at least 2 and the product below 2^24", i, (unsigned long long)mv[i]);
      return msg;
    }
    for (int j = 0; j < i; j++)
      if (hxh::gcd(mv[i], mv[j]) != 1) {
        snprintf(msg, sizeof msg, "the factors %llu and %llu are not coprime", (unsigned long long)mv[j], (unsigned long long)mv[i]);
        return msg;
      }
    m *= mv[i];
  }
  t.m = m;
  t.mvec.assign(mv, mv + k);
  uint64_t phim = 1;
  for (int i = 0; i < k; i++) {
    t.phivec.push_back(phi_of(mv[i]));
    phim *= t.phivec[i];
  }
  t.phim = (uint32_t)phim;
  std::vector<uint64_t> lprod(k + 1, 1), sprod(k + 1, 1), inv(k);   // prod_(j >= i) of the long and short signatures
  for (int i = k; i-- > 0;) {
    lprod[i] = lprod[i + 1] * mv[i];
    sprod[i] = sprod[i + 1] * t.phivec[i];
    inv[i] = hxh::invmod((m / mv[i]) % mv[i], mv[i]);
  }
  t.p2c.resize(m);
  t.c2p.resize(m);
  for (uint64_t i = 0; i < m; i++) {
    uint64_t j = 0;
    for (int d = 0; d < k; d++)
      j += (i % mv[d]) * inv[d] % mv[d] * lprod[d + 1];
    t.p2c[i] = (uint32_t)j;
    t.c2p[j] = (uint32_t)i;
  }
  t.s2l.resize(phim);
  t.s2e.resize(phim);
  for (uint64_t i = 0; i < phim; i++) {
    uint64_t j = 0;
    for (int d = 0; d < k; d++)
      j += i / sprod[d + 1] % t.phivec[d] * lprod[d + 1];
    t.s2l[i] = (uint32_t)j;
    t.s2e[i] = t.c2p[j];
  }
  for (int i = 0; i < k; i++)
    t.binom.emplace_back(mv[i]);
  t.binom.emplace_back(m);
  // to_powerful: dimension i over the fibres whose earlier coordinates are below their phi
  Program& tp = t.to_powerful;
  for (int i = 0; i < k; i++) {
    Dim d{};
    d.n = (uint32_t)mv[i];
    d.phi = (uint32_t)t.phivec[i];
    d.stride = (uint32_t)lprod[i + 1];
    d.nouter = (uint32_t)(phim / sprod[i]);
    d.outer_off = (uint32_t)tp.outer.size();
    for (uint32_t o = 0; o < d.nouter; o++) {   // o: an index in the short cube of the dimensions before i
      uint64_t j = 0, rest = o;
      for (int e = i; e-- > 0;) {
        j += rest % t.phivec[e] * lprod[e + 1];
        rest /= t.phivec[e];
      }
      tp.outer.push_back((uint32_t)j);
    }
    tp.dims.push_back(d);
    push_rem_phi(tp, (uint32_t)i, t.binom[i]);
  }
  Program& pp = t.to_poly;
  Dim d{};
  d.n = (uint32_t)m;
  d.phi = (uint32_t)phim;
  d.stride = 1;
  d.nouter = 1;
  d.outer_off = 0;
  pp.outer.push_back(0);
  pp.dims.push_back(d);
  push_rem_phi(pp, 0, t.binom[k]);
  return "";
}

inline uint64_t addq(uint64_t a, uint64_t b, uint64_t q)
{
  const uint64_t s = a + b;
  return s >= q ? s - q : s;
}
inline uint64_t subq(uint64_t a, uint64_t b, uint64_t q) { return a >= b ? a - b : a + q - b; }

// the 64-bit forms of bgv_crt.h's mul_binomial / div_binomial on a strided fibre
inline void mul_binomial64(const uint64_t* src, uint64_t* dst, size_t L, size_t e, size_t stride, uint64_t q)
{
  for (size_t k = 0; k < L; k++)
    dst[k * stride] = k >= e ? subq(src[k * stride], src[(k - e) * stride], q) : src[k * stride];
}
inline void div_binomial64(uint64_t* w, size_t L, size_t e, size_t stride, uint64_t q)
{
  for (size_t k = e; k < L; k++)
    w[k * stride] = addq(w[k * stride], w[(k - e) * stride], q);
}

// one pass on the three buffers (each m words), every fibre in turn: what one workgroup of the kernel does
inline void replay_pass(const Program& pr, const Pass& ps, std::vector<uint64_t>* buf, uint64_t q)
{
  const Dim& d = pr.dims.at(ps.dim);
  const std::vector<uint64_t>& src = buf[ps.src];
  std::vector<uint64_t>& dst = buf[ps.dst];
  for (uint32_t o = 0; o < d.nouter; o++)
    for (uint32_t in = 0; in < d.stride; in++) {
      const size_t base = (size_t)pr.outer.at(d.outer_off + o) + in, s = d.stride;
      if (ps.L > 0) {   // the last word of the fibre a pass may touch
        (void)src.at(base + (size_t)(ps.op == OP_REV ? d.n - 1 : ps.L - 1) * s);
        (void)dst.at(base + (size_t)(ps.L - 1) * s);
      }
      switch (ps.op) {
      case OP_REV:
        for (size_t k = 0; k < ps.L; k++)
          dst[base + k * s] = src[base + (d.n - 1 - k) * s];
        break;
      case OP_MUL:
        mul_binomial64(src.data() + base, dst.data() + base, ps.L, ps.e, s, q);
        break;
      case OP_DIV:
        div_binomial64(dst.data() + base, ps.L, ps.e, s, q);
        break;
      case OP_REVW:
        for (size_t k = 0; k < ps.L; k++)
          dst[base + k * s] = k <= ps.e ? src[base + (ps.e - k) * s] : 0;
        break;
      case OP_SUB:
        for (size_t k = 0; k < ps.L; k++)
          dst[base + k * s] = subq(dst[base + k * s], src[base + k * s], q);
        break;
      }
    }
}

// in: phi(m) words below q -> out: phi(m) words below q, through the pass list of one direction
inline void replay(const Tables& t, bool to_powerful, const uint64_t* in, uint64_t* out, uint64_t q)
{
  std::vector<uint64_t> buf[3];
  for (auto& b : buf)
    b.assign(t.m, 0);
  const std::vector<uint32_t>& scat = to_powerful ? t.p2c : t.s2e;
  for (uint32_t j = 0; j < t.phim; j++)
    buf[0].at(scat[j]) = in[j];
  const Program& pr = to_powerful ? t.to_powerful : t.to_poly;
  for (const Pass& ps : pr.passes)
    replay_pass(pr, ps, buf, q);
  for (uint32_t j = 0; j < t.phim; j++)
    out[j] = buf[0].at(to_powerful ? t.s2l[j] : j);
}

}  // namespace hxpw
