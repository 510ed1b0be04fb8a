// switches.h -- every environment switch of the library, in ONE place (host code only).
//
// None of them is needed in production.  They select the older or more generic form of a path so that tests can
// reach it and same-box A/B measurements can compare it (tools/gpu_calls.sh ab:...); every one leaves results
// bit-identical.  They are listed for users in include/helib_amd.h and read ONCE PER CONTEXT: hx_ctx_create()
// snapshots the environment INTO THE CONTEXT (hx_ctx::sw = hxs::read()), every later decision of the library reads
// that context's copy -- so a test process can change a switch between two contexts without touching the first (no
// process-global state: round 4 kept one struct that every hx_ctx_create rewrote under the running threads of earlier
// contexts), and nothing consults the environment on a hot path.
// A switch earns its place by a test or a tool that sets it (tests/test_host_logic.py checks that): probes that a
// measurement settled are deleted with their path, and DESIGN.md keeps one line on what was tried.
#pragma once
#include <cstdlib>

namespace hxs {

struct Switches {
  // exact RNS kernels (rns_kernels.h)
  double hps_eps = 1.0 / (double)(1u << 30);   // HX_HPS_EPS=x   distance from 0, 1/2, 1 below which an HPS quotient is redone
  int hps_min_n = 9;             // HX_HPS_MIN_N=n       fast kernels: HPS form from n source primes on
  int brk_hps_min_n = 5;         //                      ... the digit kernel's own threshold (round 6: digits of 5 - 8 primes run faster on
                                 //                      the HPS front end + its redo launch than on Garner; HX_HPS_MIN_N overrides both)
  bool no_proth_rns = false;     // HX_NO_PROTH_RNS=1    fast kernels: Barrett / Shoup products on Proth-form primes too (HX_NO_PROTH implies it)
  bool no_mfma_ext = false;      // HX_NO_MFMA_EXT=1     rns_extend_wide_kernel (VALU limb products) instead of the matrix-core form
                                 //                      rns_extend_mfma_kernel (17..40 sources)
  int mfma_min_n = 9;            // HX_MFMA_MIN_N=n      ... from n source primes on (9 .. 16: the fast kernels' plans; 17 .. 40 always)
  bool no_mask_split = false;    // HX_NO_MASK_SPLIT=1   hx_mask_split as hx_poly_copy + hx_mul + hx_sub per part instead of mask_split_kernel
                                 //                      (linalg.hip)
  bool no_mask_fan = false;      // HX_NO_MASK_FAN=1     hx_mask_fan as hx_poly_copy + hx_mul per output and part instead of mask_fan_kernel
                                 //                      (linalg.hip)
  // fused ciphertext-level paths
  bool no_mulrelin_fuse = false; // HX_NO_MULRELIN_FUSE=1 hx_mul_relin with a tensor pass
  bool no_ks_last_fuse = false;  // HX_NO_KS_LAST_FUSE=1 relinearisation: every extension row through ntt_row_kernel<., false, 8> and the
                                 //                      key switch as keyswitch_kernel<D>, instead of each output row's last digit transform
                                 //                      fused into the key switch (ntt_keyswitch_last_kernel)
  bool no_prep_fuse = false;     // HX_NO_PREP_FUSE=1    single-prime mod-switch as before: S by moddown_S_kernel behind the prep kernels, the
                                 //                      (x, S) norm by its own kernel, the radix-16 norm in its paired form -- instead of S
                                 //                      (and at N = 2^14 the norm) formed in the prep kernels' workgroups and the pairing-free
                                 //                      norm
  // row transforms (ntt_core.h)
  bool no_proth = false;         // HX_NO_PROTH=1        Shoup butterflies on every row (Proth-form primes included)
  // general m
  bool blue_old = false;         // HX_BLUE_OLD=1        Bluestein as the round-2 chain of passes instead of ntt_conv_kernel
  bool no_pfa = false;           // HX_NO_PFA=1          m = 21845: Bluestein instead of the Good-Thomas x Rader kernels (pfa_core.h)
  bool pfa_no_rem = false;       // HX_PFA_NO_REM=1      ... their inverse stops at X: rem Phi_m on the convolution kernels, not fused
  // host waits
  int wait_poll_us = 2000;       // HX_WAIT_POLL_US=n    how long a norm read-back is polled for before the thread sleeps in hipEventSynchronize
  // diagnostics
  bool arena_trace = false;      // HX_ARENA_TRACE=1     one line on stderr per hipMalloc the slab arena makes
};

// The environment as it is now, by value: hx_ctx_create() stores it in the context (hx_ctx::sw) and every later decision
// made for that context reads its own copy -- a context created later, under a changed environment, does not touch it.
inline Switches read()
{
  Switches s;
  auto on = [](const char* name) { return std::getenv(name) != nullptr; };
  if (const char* e = std::getenv("HX_HPS_EPS"))
    s.hps_eps = std::atof(e);
  if (const char* e = std::getenv("HX_HPS_MIN_N"))
    s.hps_min_n = s.brk_hps_min_n = std::atoi(e);
  s.no_proth_rns = on("HX_NO_PROTH_RNS");
  s.no_mfma_ext = on("HX_NO_MFMA_EXT");
  if (const char* e = std::getenv("HX_MFMA_MIN_N"))
    s.mfma_min_n = std::atoi(e);
  s.no_mask_split = on("HX_NO_MASK_SPLIT");
  s.no_mask_fan = on("HX_NO_MASK_FAN");
  s.no_mulrelin_fuse = on("HX_NO_MULRELIN_FUSE");
  s.no_ks_last_fuse = on("HX_NO_KS_LAST_FUSE");
  s.no_prep_fuse = on("HX_NO_PREP_FUSE");
  s.no_proth = on("HX_NO_PROTH");
  s.blue_old = on("HX_BLUE_OLD");
  s.no_pfa = on("HX_NO_PFA") || s.blue_old;
  s.pfa_no_rem = on("HX_PFA_NO_REM");
  if (const char* e = std::getenv("HX_WAIT_POLL_US"))
    s.wait_poll_us = std::atoi(e);
  s.arena_trace = on("HX_ARENA_TRACE");
  return s;
}

}  // namespace hxs
