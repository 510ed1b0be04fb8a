// gather_map_test.cpp -- TEST INFRASTRUCTURE.  The thread -> (unit, lane) map of bgv_gf_gather_map_kernel
// (helib_amd/csrc/gather_map.h) on the CPU: for every d in 1 .. 64 and unit counts 1, 64 / dp - 1, 64 / dp + 1, one that is
// no multiple of the units of a workgroup and one that needs more than one pass under a small cap, every (unit, j < d)
// is owned exactly once and no lane with j >= d or unit >= units owns anything.  Prints "ok <cases>" or the first failure.
#include <cstdio>
#include <vector>

#include "../../helib_amd/csrc/gather_map.h"

static int check(unsigned d, unsigned long long units, unsigned cap)
{
  const unsigned dp = hx::gm_group(d);
  if (dp < d || dp > 64 || (dp & (dp - 1)) || (dp > 1 && dp / 2 >= d))
    return printf("d = %u: group %u\n", d, dp), 1;
  const unsigned blocks = hx::gm_blocks(units, dp, cap), passes = hx::gm_passes(units, dp, blocks);
  if (blocks < 1 || blocks > cap)
    return printf("d = %u units = %llu: %u blocks\n", d, units, blocks), 1;
  std::vector<unsigned> owned(units * d, 0);
  for (unsigned pass = 0; pass < passes; pass++)
    for (unsigned b = 0; b < blocks; b++)
      for (unsigned tid = 0; tid < hx::GM_THREADS; tid++) {
        const hx::GmWork w = hx::gm_work(b, tid, blocks, pass, units, d, dp);
        if (w.j != tid % dp || w.j >= dp)
          return printf("d = %u: lane %u of thread %u\n", d, w.j, tid), 1;
        // the lanes of a group are consecutive and inside one wave
        if ((tid / dp) * dp / 64 != (tid / dp * dp + dp - 1) / 64)
          return printf("d = %u: the group of thread %u crosses a wave\n", d, tid), 1;
        if (w.owns != (w.unit < units && w.j < d))
          return printf("d = %u units = %llu: thread %u owns outside\n", d, units, tid), 1;
        if (w.owns)
          owned[w.unit * d + w.j]++;
      }
  for (size_t i = 0; i < owned.size(); i++)
    if (owned[i] != 1)
      return printf("d = %u units = %llu cap = %u: word %zu owned %u times\n", d, units, cap, i, owned[i]), 1;
  return 0;
}

int main()
{
  unsigned cases = 0;
  for (unsigned d = 1; d <= 64; d++) {
    const unsigned dp = hx::gm_group(d), wave = 64 / dp, wg = hx::GM_THREADS / dp;
    const unsigned long long counts[] = {1, wave > 1 ? wave - 1 : 1, wave + 1, 3ull * wg + wg / 2 + 1, 42, 8192};
    for (unsigned long long units : counts)
      for (unsigned cap : {2048u, 3u}) {
        if (check(d, units, cap))
          return 1;
        cases++;
      }
  }
  printf("ok %u\n", cases);
  return 0;
}
