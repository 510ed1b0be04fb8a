// recrypt_core_replay.cpp -- helib_amd/csrc/recrypt_core.h on the CPU: the plan and the per-coefficient arithmetic that
// recrypt_prep_kernel runs, replayed on vectors from tests/recryption_ref.py (tests/test_recryption_host.py builds this
// with -fsanitize=address,undefined and compares every word).
//   stdin:  k nt batch n q p p2r p2e seed part / the k primes / the nt targets / k rows of batch * n residues
//   stdout: "ok", then batch lines of x, batch lines of v, nt * batch lines of w mod t; or "refused: <why>"
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../helib_amd/csrc/recrypt_core.h"

int main()
{
  unsigned long long k, nt, batch, n, q, p, p2r, p2e, seed, part;
  if (scanf("%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", &k, &nt, &batch, &n, &q, &p, &p2r, &p2e, &seed, &part) != 10)
    return 2;
  if (k > 1000 || nt > 1000 || batch * n > (1u << 24))
    return 2;
  std::vector<uint64_t> src(k), tgt(nt);
  for (auto& x : src)
    if (scanf("%" SCNu64, &x) != 1)
      return 2;
  for (auto& x : tgt)
    if (scanf("%" SCNu64, &x) != 1)
      return 2;
  const size_t rw = (size_t)(batch * n);
  std::vector<uint64_t> rows(k * rw);
  for (auto& x : rows)
    if (scanf("%" SCNu64, &x) != 1)
      return 2;
  hxrc::Plan P;
  const std::string why = hxrc::build_plan(src, tgt, q, p, p2r, p2e, P);
  if (!why.empty()) {
    printf("refused: %s\n", why.c_str());
    return 0;
  }
  P.seed = seed;
  P.part = part;
  std::vector<hxrc::Result> res(rw);
  std::vector<uint64_t> c(k);
  for (size_t idx = 0; idx < rw; idx++) {
    for (size_t i = 0; i < k; i++)
      c[i] = rows[i * rw + idx];
    res[idx] = hxrc::prep_any(P, c.data(), idx / n, idx % n);
  }
  printf("ok\n");
  for (int what = 0; what < 2; what++)
    for (size_t b = 0; b < batch; b++) {
      for (size_t j = 0; j < n; j++)
        printf("%" PRId64 " ", what == 0 ? res[b * n + j].x : res[b * n + j].v);
      printf("\n");
    }
  for (size_t t = 0; t < nt; t++)
    for (size_t b = 0; b < batch; b++) {
      for (size_t j = 0; j < n; j++)
        printf("%" PRIu64 " ", hxrc::residue(res[b * n + j].w, P.tgt[t]));
      printf("\n");
    }
  return 0;
}
