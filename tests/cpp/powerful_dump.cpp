// powerful_dump.cpp -- TEST INFRASTRUCTURE.  Prints what helib_amd/csrc/powerful.h builds for a factorisation, and both
// conversions from a host replay of the pass list the device kernel executes, for tests/test_evalmap_host.py:
//   powerful_dump tables m_1 ... m_k
//       "ok m phim k" or "error <reason>"; then the lines  phivec, s2e (phim words), p2c (m words), s2l (phim words),
//       and for m_1, ..., m_k, m a line "n num <sorted e ...> den <sorted e ...>"; then "passes <to_powerful> <to_poly>"
//   powerful_dump conv <to_powerful 0|1> q m_1 ... m_k      reads rows of phim words from the standard input (any number
//       of rows), prints one converted row per input row
// A stand-alone program: it links nothing of the library.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../helib_amd/csrc/powerful.h"

static void line(const char* name, const std::vector<uint32_t>& v)
{
  printf("%s", name);
  for (uint32_t x : v)
    printf(" %u", x);
  printf("\n");
}

int main(int argc, char** argv)
{
  if (argc < 3)
    return 2;
  const bool conv = !strcmp(argv[1], "conv");
  const int first = conv ? 4 : 2;
  if (argc <= first)
    return 2;
  std::vector<uint64_t> mv;
  for (int i = first; i < argc; i++)
    mv.push_back(strtoull(argv[i], nullptr, 10));
  hxpw::Tables t;
  const std::string e = hxpw::build(mv.data(), (int)mv.size(), t);
  if (!e.empty()) {
    printf("error %s\n", e.c_str());
    return 0;
  }
  if (!conv) {
    printf("ok %llu %u %zu\n", (unsigned long long)t.m, t.phim, mv.size());
    printf("phivec");
    for (uint64_t x : t.phivec)
      printf(" %llu", (unsigned long long)x);
    printf("\n");
    line("s2e", t.s2e);
    line("p2c", t.p2c);
    line("s2l", t.s2l);
    for (size_t i = 0; i < t.binom.size(); i++) {
      std::vector<uint64_t> num = t.binom[i].num, den = t.binom[i].den;
      std::sort(num.begin(), num.end());
      std::sort(den.begin(), den.end());
      printf("%llu num", (unsigned long long)(i < mv.size() ? mv[i] : t.m));
      for (uint64_t x : num)
        printf(" %llu", (unsigned long long)x);
      printf(" den");
      for (uint64_t x : den)
        printf(" %llu", (unsigned long long)x);
      printf("\n");
    }
    printf("passes %zu %zu\n", t.to_powerful.passes.size(), t.to_poly.passes.size());
    return 0;
  }
  const bool to_powerful = atoi(argv[2]) != 0;
  const uint64_t q = strtoull(argv[3], nullptr, 10);
  if (q < 2 || q >= hxpw::MAX_Q)
    return 2;
  std::vector<uint64_t> in(t.phim), out(t.phim);
  for (;;) {
    for (uint32_t j = 0; j < t.phim; j++) {
      unsigned long long x;
      if (scanf("%llu", &x) != 1)
        return j == 0 ? 0 : 3;
      in[j] = x % q;
    }
    hxpw::replay(t, to_powerful, in.data(), out.data(), q);
    for (uint32_t j = 0; j < t.phim; j++)
      printf("%llu ", (unsigned long long)out[j]);
    printf("\n");
  }
}
