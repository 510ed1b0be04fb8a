// bgv_gr_linalg_dump.cpp -- TEST INFRASTRUCTURE.  Prints what helib_amd/csrc/bgv_gf_linalg.h builds modulo P = p^r over the
// Hensel-lifted G of (m, p, r), for tests/test_bgv_gr_matmul_host.py:  bgv_gr_linalg_dump m p r
//   line 1   "ok m p r P d limit"  or  "error <reason>"      line 2   G (d + 1 words mod P, constant first)
//   line 3   frob (d^3 words: [e][l][c])    line 4   K (d^3 words: [j][k][c])    line 5   T (d^4 words, row major)
// r = 0 goes through build_gf_linalg (the r = 1 entry) instead of build_gr_linalg.
#include <cstdio>
#include <cstdlib>

#include "../../helib_amd/csrc/bgv_gf_linalg.h"

static void row(const std::vector<uint32_t>& w)
{
  for (uint32_t x : w)
    printf("%u ", x);
  printf("\n");
}

int main(int argc, char** argv)
{
  if (argc < 4)
    return 2;
  const uint64_t m = strtoull(argv[1], nullptr, 10), p = strtoull(argv[2], nullptr, 10);
  const uint32_t r = (uint32_t)strtoul(argv[3], nullptr, 10);
  hxc::GfTables t;
  std::string e = hxc::build_gf(m, p, t, r ? r : 1);
  hxc::GfLinTables lin;
  if (e.empty())
    e = r ? hxc::build_gr_linalg(t.G.data(), t.crt.d, p, r, lin) : hxc::build_gf_linalg(t.G.data(), t.crt.d, p, lin);
  if (!e.empty()) {
    printf("error %s\n", e.c_str());
    return 0;
  }
  printf("ok %llu %llu %u %llu %u %llu\n", (unsigned long long)m, (unsigned long long)p, r, (unsigned long long)lin.p, lin.d,
         (unsigned long long)lin.limit);
  row(t.G);
  row(lin.frob);
  row(lin.K);
  row(lin.T);
  return 0;
}
