// bgv_gf_tail.h -- what bgv_gf.hip lends bgv_gf_linalg.hip: a view of a GF / Galois-ring slot table and the tail of an
// encode that starts from the CRT components c[batch][nslots d] (32-bit words below the modulus) on the device.
// hx_bgv_gf_encode forms them from host slots (upload + bgv_gf_map_kernel), hx_bgv_gf_encode_gathered from a matrix on
// the device (bgv_gf_gather_map_kernel); both hand `fill` to gf_encode_words, which owns everything else: the checks of
// the output, the caller's context and lock, the scratch, bgv_gf_encode_kernel, the fold and the lift / transform.
#pragma once
#include <functional>

#include "bgv_encode.h"

namespace hxg {

struct GfView {
  hx_ctx* ctx;
  uint64_t p;            // the modulus of the maps: p^r
  uint32_t d, nslots, limit;
  const uint32_t* d_A;   // [nslots][d][d] on the device
};
int gf_view(const hx_bgv_gf* t, GfView* v);

// fill(st, c): enqueue on st whatever writes c[batch][nslots d]; it runs under the context's lock, after the output was
// checked, and a failure ends the encode
using GfFill = std::function<int(hipStream_t, uint32_t*)>;
int gf_encode_words(hx_bgv_gf* t, const char* what, int batch, uint64_t mul, hx_poly* out, int64_t* coeffs_out, const GfFill& fill);

}  // namespace hxg
