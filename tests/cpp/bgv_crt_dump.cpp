// bgv_crt_dump.cpp -- TEST INFRASTRUCTURE.  Prints what helib_amd/csrc/bgv_crt.h builds for (m, p), for
// tests/test_bgv_crt_host.py:  bgv_crt_dump m p [geom]
//   line 1   "ok m p d nslots phim ld limit"  or  "error <reason>"
//   line 2   the generators        line 3   the signed orders
//   then (without geom) nslots lines each of: the factors (d + 1 words, constant first), E (phim words), R (phim words)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../helib_amd/csrc/bgv_crt.h"

int main(int argc, char** argv)
{
  if (argc < 3)
    return 2;
  const uint64_t m = strtoull(argv[1], nullptr, 10), p = strtoull(argv[2], nullptr, 10);
  const bool geom = argc > 3 && !strcmp(argv[3], "geom");
  hxc::CrtTables t;
  const std::string e = hxc::build_crt(m, p, t, !geom);
  if (!e.empty()) {
    printf("error %s\n", e.c_str());
    return 0;
  }
  printf("ok %llu %llu %u %u %u %u %llu\n", (unsigned long long)t.m, (unsigned long long)t.p, t.d, t.nslots, t.phim, t.ld,
         (unsigned long long)t.limit);
  for (uint64_t g : t.gens)
    printf("%llu ", (unsigned long long)g);
  printf("\n");
  for (int64_t o : t.ords)
    printf("%lld ", (long long)o);
  printf("\n");
  if (geom)
    return 0;
  for (int which = 0; which < 3; which++)
    for (uint32_t i = 0; i < t.nslots; i++) {
      const uint32_t* row = which == 0 ? t.factors.data() + (size_t)i * (t.d + 1) : (which == 1 ? t.E : t.R).data() + (size_t)i * t.ld;
      const uint32_t len = which == 0 ? t.d + 1 : t.phim;
      for (uint32_t k = 0; k < len; k++)
        printf("%u ", row[k]);
      printf("\n");
    }
  return 0;
}
