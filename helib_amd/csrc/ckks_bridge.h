// ckks_bridge.h -- what ckks_slots.hip, bgv_slots.hip and linalg.hip need of engine.hip's objects (hx_ctx / hx_poly stay private
// to engine.hip; everything else those units do goes through the C ABI, include/helib_amd.h), and the error plumbing
// they share (err, CK, RC, DrainOnExit)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <mutex>

#include "../../include/helib_amd.h"

namespace hxi {
struct CtxView {
  std::recursive_mutex* mu;   // the context's lock (CTX_ENTER)
  hipStream_t stream;
  uint64_t m;
  uint32_t phim;
  bool capturing;             // a graph capture is open
  bool no_mask_split;         // the context's HX_NO_MASK_SPLIT (switches.h)
  bool no_mask_fan;           // the context's HX_NO_MASK_FAN (switches.h)
  void** state;               // the slot unit's per-context state ...
  void (**state_free)(void*); // ... and how the context releases it
  void** linalg;              // the same pair for linalg.hip
  void (**linalg_free)(void*);
  void** recrypt;             // the same pair for recrypt.hip
  void (**recrypt_free)(void*);
  const void* d_primes;       // the per-prime constants (hx::PrimeDev[], dev_common.h) on the device
  int device;
  bool pow2;                  // m is a power of two
  const uint32_t* d_zms;      // Z_m^* in increasing order, [phi(m)] (device) ...
  const int32_t* d_zms_index; // ... and the position of every t in Z_m^* in it, [m] (device; -1 elsewhere)
};
// sets the device and fills v; the caller then takes *v->mu
int ctx_enter(hx_ctx* c, CtxView* v);
int fail_msg(int code, const char* msg);   // sets hx_last_error, returns code
hx_ctx* poly_ctx(const hx_poly* p);
int poly_rows_write(hx_poly* p, uint64_t** d);
// p's rows are about to be read and rewritten in place: a shared slab is copied first
int poly_rows_update(hx_poly* p, uint64_t** d);
const uint64_t* poly_rows_read(const hx_poly* p);
// p becomes a poly on the n primes idx whose rows are all about to be overwritten (the old rows are not kept)
int poly_rows_reshape(hx_poly* p, const int* idx, int n, uint64_t** d);
// a key-switching matrix: b and a are [ndig][nrows][phi(m)] words on the device, row r on prime row_idx[r]
struct KskView {
  hx_ctx* ctx;
  int ndig, nrows;
  const int* row_idx;
  const uint64_t* d_b;
  const uint64_t* d_a;
};
void ksk_view(const hx_ksk* k, KskView* v);
// hx_poly_rem's arithmetic (toPoly + PolyRed(t), exact) with the result kept on the device: *d_out = [batch][phi(m)]
// words in [0, t) in the context's scratch, valid until the next call on that context (hold its lock); a has rows
int poly_rem_device(const hx_poly* a, uint64_t t, const uint64_t** d_out);

// error plumbing of those units (they say `using hxi::err;`): a formatted hx_last_error, and early returns
inline int err(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline int err(int code, const char* fmt, ...)
{
  char b[400];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(b, sizeof b, fmt, ap);
  va_end(ap);
  return fail_msg(code, b);
}
// Declared once work may be enqueued: every return -- an error one included -- waits for the stream, so that no
// copy still reads a host buffer (the constant tables, the caller's arrays) and no kernel a temporary poly that the
// return releases.  (Declared after those objects: destroyed, and so run, before them.)
struct DrainOnExit {
  hipStream_t st;
  ~DrainOnExit() { (void)hipStreamSynchronize(st); }
};
}  // namespace hxi

#define CK(expr)                                                                                                    \
  do {                                                                                                              \
    hipError_t _e = (expr);                                                                                         \
    if (_e != hipSuccess) {                                                                                         \
      (void)hipGetLastError();                                                                                      \
      return hxi::err(HX_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);   \
    }                                                                                                               \
  } while (0)
#define RC(expr)        \
  do {                  \
    int _rc = (expr);   \
    if (_rc != HX_OK)   \
      return _rc;       \
  } while (0)
