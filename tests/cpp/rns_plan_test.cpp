// rns_plan_test -- prints what helib_amd/csrc/rns_plan.h builds, for tests/test_rns_plan_host.py to recompute from
// Python integers (no GPU, no HIP: plain g++ -std=c++17 -Wall -Werror, and once more under -fsanitize=address,undefined).
//
//   rns_plan_test plan SCALED PTXT NO_PROTH NO_PROTH_RNS NO_MFMA_EXT MFMA_MIN_N N p_0 .. p_(N-1) NT t_0 .. t_(NT-1)
//       err E                       the builder's error (0: none; then nothing else follows)
//       scalar NAME VALUE           n, nt, the ptxt constants, hps_eps (as its 64 bits) and every flag
//       section NAME OFFSET WORDS w_0 w_1 ..     every section of the blob, in hexadecimal
//       mfma BYTES                  the size of the matrix-core table (0: not built; "planraw" for "plan": every byte
//                                   behind it), then the table read back through mfma_ext.h (print_mfma below)
//   rns_plan_test route FAST16_OK HPS_OK WIDE_OK MFMA_STEPS N NT UPD ROW_WORDS HPS_MIN_N [nine more ..]
//       route NAME                  one line per group of nine
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../helib_amd/csrc/rns_plan.h"

namespace rp = hx::rnsplan;

static uint64_t u64(const char* s) { return strtoull(s, nullptr, 0); }

// The matrix-core table read back through mfma_ext.h's own index functions, the way the kernel addresses it:
//   mfma_w T SLOT A l_0 .. l_7    the signed limbs of (multiplier of slot SLOT) 2^(8 A) mod t, for every slot and A
//   mfma_x T init_0 .. init_7 mu80 t_lo t_hi upd_lo upd_hi shoup_lo shoup_hi
//   mfma_stray N                  non-zero bytes no index function reaches for a target t < nt
static void print_mfma(const rp::Plan& pl)
{
  namespace mfx = hx::mfx;
  const int steps = (int)pl.mfma_steps, slots = 4 * steps;
  const uint32_t* words = reinterpret_cast<const uint32_t*>(pl.mfma.data());
  std::vector<uint8_t> seen(pl.mfma.size(), 0);
  for (int t = 0; t < pl.nt; t++) {
    const int tau = t / mfx::TILE_TARGETS, tt = t % mfx::TILE_TARGETS;
    for (int k = 0; k < slots; k++)
      for (int a = 0; a < 8; a++) {
        printf("mfma_w %d %d %d", t, k, a);
        for (int b = 0; b < 8; b++) {
          const size_t i = mfx::a_byte_index(steps, tau, k >> 2, mfx::row_of(tt, b) + 32 * ((k >> 1) & 1), 8 * (k & 1) + a);
          seen[i] = 1;
          printf(" %d", (int)(int8_t)pl.mfma[i]);
        }
        printf("\n");
      }
    uint32_t init[8] = {};
    for (int h = 0; h < 2; h++)
      for (int reg = 0; reg < 16; reg++) {
        const int row = mfx::cd_row(reg, h);
        if (mfx::row_target(row) == tt)
          init[mfx::row_limb(row)] = words[mfx::extra_word_index(steps, tau, h, mfx::EX_INIT + reg)];
      }
    printf("mfma_x %d", t);
    for (int b = 0; b < 8; b++)
      printf(" %u", init[b]);
    const int h = tt >> 1, s = tt & 1;
    printf(" %u", words[mfx::extra_word_index(steps, tau, h, mfx::EX_MU80 + s)]);
    for (int e = 0; e < 2; e++)
      printf(" %u", words[mfx::extra_word_index(steps, tau, h, mfx::EX_Q + 2 * s + e)]);
    for (int e = 0; e < 4; e++)
      printf(" %u", words[mfx::extra_word_index(steps, tau, h, mfx::EX_UPD + 4 * s + e)]);
    printf("\n");
  }
  // every extra word belongs to some target slot of its tile; those of targets >= nt must be zero, like every byte
  // the loops above did not reach
  for (int t = 0; t < pl.nt; t++)
    for (int w = 0; w < 32; w++) {
      const size_t i = 4 * mfx::extra_word_index(steps, t / mfx::TILE_TARGETS, (t % mfx::TILE_TARGETS) >> 1, w);
      const int s = t & 1;
      const bool mine = w < 16 ? mfx::row_target(mfx::cd_row(w, (t % mfx::TILE_TARGETS) >> 1)) == t % mfx::TILE_TARGETS
                               : (w < 20 ? w == 16 + s : (w < 24 ? (w - 20) / 2 == s : (w - 24) / 4 == s));
      if (mine)
        seen[i] = seen[i + 1] = seen[i + 2] = seen[i + 3] = 1;
    }
  size_t stray = 0;
  for (size_t i = 0; i < pl.mfma.size(); i++)
    stray += !seen[i] && pl.mfma[i] != 0;
  printf("mfma_stray %zu\n", stray);
}

static int print_plan(int argc, char** argv, bool raw)
{
  if (argc < 9)
    return 2;
  const bool scaled = u64(argv[2]) != 0;
  const uint64_t ptxt = u64(argv[3]);
  rp::Switches sw;
  sw.no_proth = u64(argv[4]) != 0;
  sw.no_proth_rns = u64(argv[5]) != 0;
  sw.no_mfma_ext = u64(argv[6]) != 0;
  sw.mfma_min_n = (int)u64(argv[7]);
  int a = 8;
  std::vector<uint64_t> p, tq;
  for (std::vector<uint64_t>* v : {&p, &tq}) {
    if (a >= argc)
      return 2;
    const int cnt = (int)u64(argv[a++]);
    if (a + cnt > argc)
      return 2;
    for (int i = 0; i < cnt; i++)
      v->push_back(u64(argv[a++]));
  }
  const rp::Plan pl = rp::build(p, tq, ptxt, scaled, sw);
  printf("err %d\n", (int)pl.err);
  if (pl.err) {
    printf("message %s\n", rp::message(pl.err));
    return 0;
  }
  uint64_t eps;
  memcpy(&eps, &pl.hps_eps, 8);
  const struct {
    const char* name;
    uint64_t v;
  } scalars[] = {{"n", (uint64_t)pl.n}, {"nt", (uint64_t)pl.nt}, {"ptxt", pl.ptxt}, {"ptxt_mu64", pl.ptxt_mu64},
                 {"pinv_ptxt", pl.pinv_ptxt}, {"pmod_ptxt", pl.pmod_ptxt}, {"ptxt_mu", pl.ptxt_mu}, {"ptxt_k", pl.ptxt_k},
                 {"hps_eps", eps}, {"garner_cs", pl.garner_cs}, {"src_mont", pl.src_mont}, {"corr_unit", pl.corr_unit},
                 {"mfma_steps", pl.mfma_steps}, {"fast_ok", pl.fast_ok}, {"fast16_ok", pl.fast16_ok}, {"hps_ok", pl.hps_ok},
                 {"wide_ok", pl.wide_ok}, {"lazy_tight_ok", pl.lazy_tight_ok}};
  for (const auto& s : scalars)
    printf("scalar %s %" PRIu64 "\n", s.name, s.v);
  static const char* const names[rp::NSECTIONS] = {
      "src_q", "src_mu64", "ginv", "half", "tgt_q", "tgt_mu64", "tgt_mu", "tgt_k", "pmod", "W", "upd", "Wp", "tgt_lazy",
      "src_rq", "tgt_pack", "tgt_pack_hps", "hps_inv", "Wp_hps", "ginv_m", "wide_pack"};
  for (int s = 0; s < rp::NSECTIONS; s++) {
    printf("section %s %zu %zu", names[s], pl.off[s], pl.words[s]);
    for (size_t i = 0; i < pl.words[s]; i++)
      printf(" %" PRIx64, pl.at((rp::Section)s)[i]);
    printf("\n");
  }
  printf("mfma %zu", pl.mfma.size());
  for (size_t i = 0; raw && i < pl.mfma.size(); i++)
    printf(" %x", pl.mfma[i]);
  printf("\n");
  if (!pl.mfma.empty())
    print_mfma(pl);
  return 0;
}

static int print_route(int argc, char** argv)
{
  if (argc < 11 || (argc - 2) % 9 != 0)
    return 2;
  static const char* const names[] = {"FAST_GARNER", "FAST_HPS", "FAST_MFMA", "WIDE_VALU", "WIDE_MFMA", "GENERIC"};
  for (char** a = argv + 2; a < argv + argc; a += 9) {   // one line per group of nine
    const rp::RouteFlags f = {(uint32_t)u64(a[0]), (uint32_t)u64(a[1]), (uint32_t)u64(a[2]), (uint32_t)u64(a[3])};
    const rp::Route r = rp::extend_route(f, (int)u64(a[4]), (int)u64(a[5]), u64(a[6]) != 0, (size_t)u64(a[7]), (int)u64(a[8]));
    printf("route %s\n", names[(int)r]);
  }
  return 0;
}

int main(int argc, char** argv)
{
  int rc = 2;
  if (argc >= 2 && !strcmp(argv[1], "plan"))
    rc = print_plan(argc, argv, false);
  else if (argc >= 2 && !strcmp(argv[1], "planraw"))
    rc = print_plan(argc, argv, true);
  else if (argc >= 2 && !strcmp(argv[1], "route"))
    rc = print_route(argc, argv);
  if (rc == 2)
    fprintf(stderr, "usage: see the head of tests/cpp/rns_plan_test.cpp\n");
  return rc;
}
