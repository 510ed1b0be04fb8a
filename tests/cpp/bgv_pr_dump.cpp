// bgv_pr_dump.cpp -- TEST INFRASTRUCTURE.  Prints what helib_amd/csrc/bgv_crt.h builds for (m, p, r), for
// tests/test_bgv_pr_host.py:  bgv_pr_dump m p r [old]
//   line 1   "ok m p r modulus d nslots phim ld limit"  or  "error <reason>"
//   line 2   the generators        line 3   the signed orders
//   then nslots lines each of: the factors (d + 1 words, constant first), E (ld words), R (ld words)
// old: build_crt(m, p) as callers from before the exponent existed spell it (r must be 1).  A stand-alone program: it
// may be built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../helib_amd/csrc/bgv_crt.h"

int main(int argc, char** argv)
{
  if (argc < 4)
    return 2;
  const uint64_t m = strtoull(argv[1], nullptr, 10), p = strtoull(argv[2], nullptr, 10);
  const long r = strtol(argv[3], nullptr, 10);
  const bool old = argc > 4 && !strcmp(argv[4], "old");
  hxc::CrtTables t;
  const std::string e = old ? hxc::build_crt(m, p, t) : hxc::build_crt(m, p, t, true, r < 0 ? 0u : (uint32_t)r);
  if (!e.empty()) {
    printf("error %s\n", e.c_str());
    return 0;
  }
  printf("ok %llu %llu %u %llu %u %u %u %u %llu\n", (unsigned long long)t.m, (unsigned long long)t.p, t.r,
         (unsigned long long)t.modulus, t.d, t.nslots, t.phim, t.ld, (unsigned long long)t.limit);
  for (uint64_t g : t.gens)
    printf("%llu ", (unsigned long long)g);
  printf("\n");
  for (int64_t o : t.ords)
    printf("%lld ", (long long)o);
  printf("\n");
  for (int which = 0; which < 3; which++)
    for (uint32_t i = 0; i < t.nslots; i++) {
      const uint32_t* row = which == 0 ? t.factors.data() + (size_t)i * (t.d + 1) : (which == 1 ? t.E : t.R).data() + (size_t)i * t.ld;
      const uint32_t len = which == 0 ? t.d + 1 : t.ld;
      for (uint32_t k = 0; k < len; k++)
        printf("%u ", row[k]);
      printf("\n");
    }
  return 0;
}
