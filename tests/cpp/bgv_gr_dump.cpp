// bgv_gr_dump.cpp -- TEST INFRASTRUCTURE.  Prints what helib_amd/csrc/bgv_gf.h builds for (m, p, r), for
// tests/bgv_gr_tables.py:  bgv_gr_dump m p r   (r = 0: build_gf's default argument, the r = 1 tables of hx_bgv_gf_create)
//   line 1   "ok m p r modulus d nslots phim ld ldr limit"  or  "error <reason>"
//   line 2   the generators        line 3   the signed orders        line 4   G (d + 1 words, constant first)
//   then nslots lines each of: the factors (d + 1 words), A (d * d words, row major), M (d * d words), E (phim words),
//   d - 1 lines of T (phim words), nslots lines of Rx (phim + d - 1 words)
#include <cstdio>
#include <cstdlib>

#include "../../helib_amd/csrc/bgv_gf.h"

static void row(const uint32_t* w, size_t n)
{
  for (size_t k = 0; k < n; k++)
    printf("%u ", w[k]);
  printf("\n");
}

int main(int argc, char** argv)
{
  if (argc < 4)
    return 2;
  const uint64_t m = strtoull(argv[1], nullptr, 10), p = strtoull(argv[2], nullptr, 10);
  const uint32_t r = (uint32_t)strtoul(argv[3], nullptr, 10);
  hxc::GfTables t;
  const std::string e = r ? hxc::build_gf(m, p, t, r) : hxc::build_gf(m, p, t);
  if (!e.empty()) {
    printf("error %s\n", e.c_str());
    return 0;
  }
  const hxc::CrtTables& c = t.crt;
  const uint32_t d = c.d, n = c.nslots;
  printf("ok %llu %llu %u %llu %u %u %u %u %u %llu\n", (unsigned long long)c.m, (unsigned long long)c.p, c.r,
         (unsigned long long)c.modulus, d, n, c.phim, c.ld, t.ldr, (unsigned long long)c.limit);
  for (uint64_t g : c.gens)
    printf("%llu ", (unsigned long long)g);
  printf("\n");
  for (int64_t o : c.ords)
    printf("%lld ", (long long)o);
  printf("\n");
  row(t.G.data(), d + 1);
  for (uint32_t i = 0; i < n; i++)
    row(c.factors.data() + (size_t)i * (d + 1), d + 1);
  for (uint32_t i = 0; i < n; i++)
    row(t.A.data() + (size_t)i * d * d, (size_t)d * d);
  for (uint32_t i = 0; i < n; i++)
    row(t.M.data() + (size_t)i * d * d, (size_t)d * d);
  for (uint32_t i = 0; i < n; i++)
    row(c.E.data() + (size_t)i * c.ld, c.phim);
  for (uint32_t u = 0; u + 1 < d; u++)
    row(t.T.data() + (size_t)u * c.ld, c.phim);
  for (uint32_t i = 0; i < n; i++)
    row(t.Rx.data() + (size_t)i * t.ldr, c.phim + d - 1);
  return 0;
}
