// bgv_gens_dump.cpp -- TEST INFRASTRUCTURE.  tests/cpp/bgv_gr_dump.cpp's output for build_gf over supplied generators
// (helib_amd/csrc/bgv_gf.h; hx_bgv_gf_create_gens), for tests/test_evalmap_host.py:
//   bgv_gens_dump m p r geom|full ngens g_1 .. g_n o_1 .. o_n
// geom: the first three lines only (the "ok" line, the generators, the signed orders).  ngens = 0 passes no generators
// (empty vectors), which has to be build_gf(m, p, t, r) word for word.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../helib_amd/csrc/bgv_gf.h"

static void row(const uint32_t* w, size_t n)
{
  for (size_t k = 0; k < n; k++)
    printf("%u ", w[k]);
  printf("\n");
}

int main(int argc, char** argv)
{
  if (argc < 6)
    return 2;
  const uint64_t m = strtoull(argv[1], nullptr, 10), p = strtoull(argv[2], nullptr, 10);
  const uint32_t r = (uint32_t)strtoul(argv[3], nullptr, 10);
  const bool geom = !strcmp(argv[4], "geom");
  const int ng = atoi(argv[5]);
  if (ng < 0 || argc != 6 + 2 * ng)
    return 2;
  std::vector<uint64_t> gens;
  std::vector<int64_t> ords;
  for (int i = 0; i < ng; i++) {
    gens.push_back(strtoull(argv[6 + i], nullptr, 10));
    ords.push_back(strtoll(argv[6 + ng + i], nullptr, 10));
  }
  hxc::GfTables t;
  const std::string e = geom ? hxc::build_crt(m, p, t.crt, false, r, &gens, &ords) : hxc::build_gf(m, p, t, r, &gens, &ords);
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
  if (geom)
    return 0;
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
