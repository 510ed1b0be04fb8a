// bgv_gf_linalg_dump.cpp -- TEST INFRASTRUCTURE.  Prints what helib_amd/csrc/bgv_gf_linalg.h builds for (m, p), for
// tests/test_bgv_gf_matmul_host.py:  bgv_gf_linalg_dump m p
//   line 1   "ok m p d"  or  "error <reason>"        line 2   G (d + 1 words, constant first)
//   line 3   frob (d^3 words: [e][l][c])    line 4   K (d^3 words: [j][k][c])    line 5   T (d^4 words, row major)
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
  if (argc < 3)
    return 2;
  const uint64_t m = strtoull(argv[1], nullptr, 10), p = strtoull(argv[2], nullptr, 10);
  hxc::GfTables t;
  std::string e = hxc::build_gf(m, p, t);
  hxc::GfLinTables lin;
  if (e.empty())
    e = hxc::build_gf_linalg(t.G.data(), t.crt.d, p, lin);
  if (!e.empty()) {
    printf("error %s\n", e.c_str());
    return 0;
  }
  printf("ok %llu %llu %u\n", (unsigned long long)m, (unsigned long long)p, lin.d);
  row(t.G);
  row(lin.frob);
  row(lin.K);
  row(lin.T);
  return 0;
}
