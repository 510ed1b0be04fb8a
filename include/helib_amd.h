/*
 * helib_amd.h -- C ABI of the MI355X-native DoubleCRT engine.
 *
 * This is the drop-in boundary for HElib 2.2.0's polynomial-arithmetic hot
 * path.  It replaces, one level above HElib's own accelerator seam (the
 * `intel::` HEXL shim, src/intelExt.h:20-59), the following reference
 * interfaces; each entry point below names the one it stands in for:
 *
 *   Cmodulus  ctor / FFT / iFFT        include/helib/CModulus.h:112-145
 *   DoubleCRT storage + ring ops       include/helib/DoubleCRT.h:212-385
 *   DoubleCRT::breakIntoDigits         src/DoubleCRT.cpp:479-561
 *   DoubleCRT::addPrimes / AndScale    src/DoubleCRT.cpp:565-647
 *   DoubleCRT::scaleDownToSet          src/DoubleCRT.cpp:1464-1516
 *   Ctxt::tensorProduct inner loop     src/Ctxt.cpp:1576-1597
 *   Ctxt::keySwitchDigits              src/Ctxt.cpp:191-230
 *   intel::FFTFwd/FFTRev1/Eltwise*     src/intelExt.h:20-59 (compat layer)
 *
 * Conventions
 *   - plain C: opaque handles, raw pointers, sizes.  No exceptions cross the
 *     ABI: every call returns HX_OK (0) or a negative hx_status; the message
 *     of the last failure on the calling thread is hx_last_error().
 *   - a `hx_poly` is a BATCH of `batch` independent DoubleCRT objects that
 *     share one prime set: device layout [row][batch][phi(m)] of uint64
 *     residues in [0, q_row), row r holding prime `prime_idx[r]`
 *     (HElib: IndexMap<vec_long>, one heap vector per prime,
 *     include/helib/DoubleCRT.h:87-95).  batch = 1 is a single DoubleCRT.
 *   - host buffers passed to upload/download use the same [row][batch][N]
 *     order and are owned by the caller; device memory is owned by the
 *     library unless the poly was created with hx_poly_wrap.
 *   - all work of a context is enqueued on one HIP stream (settable); calls
 *     are asynchronous with respect to the host except upload/download/sync.
 *   - thread-safe: every call takes its context's lock while it updates host-side state and
 *     enqueues its kernels (device work is ordered by the context's stream), so several threads
 *     may operate on DISTINCT polys of one context concurrently -- the re-entrancy HElib's NTL
 *     thread pool relies on (src/CModulus.cpp:580-610).  Two threads must not use the SAME poly.
 *   - results are bit-identical to reference HElib's DoubleCRT rows for the
 *     same (q, root) -- values are canonical residues, there is no rounding.
 *   - the library never falls back to the CPU: without a usable gfx950 device
 *     every compute entry point fails with HX_ERR_DEVICE.
 */
#ifndef HELIB_AMD_H
#define HELIB_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hx_ctx hx_ctx;   /* Context (prime chain) + PAlgebra bits used by the path */
typedef struct hx_poly hx_poly; /* batched DoubleCRT                                         */
typedef struct hx_ksk hx_ksk;   /* one KeySwitch matrix resident on the device               */

typedef enum {
  HX_OK = 0,
  HX_ERR_INVALID = -1,     /* bad argument (helib::InvalidArgument)                       */
  HX_ERR_DEVICE = -2,      /* HIP error / no gfx950 device                                  */
  HX_ERR_PRIMESET = -3,    /* index-set mismatch (helib::RuntimeError, DoubleCRT.cpp:243-253)*/
  HX_ERR_NOT_IN_ZMSTAR = -4, /* automorph: k not in Zm* (DoubleCRT.cpp:1166-1167)          */
  HX_ERR_UNSUPPORTED = -5, /* shape not supported by this build                             */
  HX_ERR_NOMEM = -6
} hx_status;

const char* hx_last_error(void);
const char* hx_version(void);
int hx_device_count(int* count);

/* ---------------- context: Context::moduli + zMStar ---------------- */
/* m > 1.  Builds the Z_m^* tables (PAlgebra, src/PAlgebra.cpp:532-538). */
int hx_ctx_create(hx_ctx** out, int device, uint64_t m);
int hx_ctx_destroy(hx_ctx* ctx);
int hx_ctx_phim(const hx_ctx* ctx, uint64_t* phim);
/* stream: a hipStream_t (void*); NULL = the device's default stream. */
int hx_ctx_set_stream(hx_ctx* ctx, void* hip_stream);
int hx_ctx_sync(hx_ctx* ctx);
/* Cmodulus::Cmodulus(zms, q, rt) (src/CModulus.cpp:64-181).
 * root: m = 2^k  -> w0 = NTL RootTable[0][k], a primitive m-th root of unity
 *                   mod q; it is an INPUT because it only exists inside NTL's
 *                   seeded PRG (src/CModulus.cpp:93-119).  root = 0 selects
 *                   FindPrimRootT(q, m) (src/NumbTh.cpp:436-493).
 *       general m -> the FindPrimitiveRoot output of order 2m (m even) / m
 *                   (m odd); 0 = compute it exactly as the reference does.
 * idx_out: position in Context::moduli order (0,1,2,...).                 */
int hx_ctx_add_prime(hx_ctx* ctx, uint64_t q, uint64_t root, int* idx_out);
int hx_ctx_num_primes(const hx_ctx* ctx, int* n);
int hx_ctx_prime(const hx_ctx* ctx, int idx, uint64_t* q, uint64_t* root);

/* ---------------- DoubleCRT storage ---------------- */
/* DoubleCRT(context, indexSet): zero-initialised rows for primes prime_idx[]. */
int hx_poly_create(hx_ctx* ctx, int batch, const int* prime_idx, int nrows, hx_poly** out);
/* Same without the zero fill, for objects that are about to be overwritten (outputs). */
int hx_poly_create_uninit(hx_ctx* ctx, int batch, const int* prime_idx, int nrows, hx_poly** out);
/* Same, on caller-owned device memory (e.g. a torch tensor's data_ptr) of
 * nrows*batch*phim uint64; not zeroed, never freed by the library. */
int hx_poly_wrap(hx_ctx* ctx, int batch, const int* prime_idx, int nrows, void* device_ptr,
                 hx_poly** out);
int hx_poly_destroy(hx_poly* p);
int hx_poly_shape(const hx_poly* p, int* batch, int* nrows, uint64_t* phim);
int hx_poly_primes(const hx_poly* p, int* prime_idx_out /* nrows */);
void* hx_poly_device_ptr(hx_poly* p);
int hx_poly_upload(hx_poly* p, const uint64_t* host);         /* synchronous */
int hx_poly_download(const hx_poly* p, uint64_t* host);       /* synchronous */
/* DoubleCRT::operator= (src/DoubleCRT.cpp:815-837): dst takes src's prime set
 * (dst capacity must be >= src rows). */
int hx_poly_copy(hx_poly* dst, const hx_poly* src);
int hx_poly_set_zero(hx_poly* p);
/* DoubleCRT::randomize (src/DoubleCRT.cpp:1258-1378): every row of every batch element filled with
 * uniform residues by the reference's rejection sampling (2048-byte buffers, ceil(k/8) bytes per
 * candidate, little endian, masked to k = NumBits(q-1) bits, kept when < q) -- on the device, from
 * a ChaCha20 (RFC 8439) key stream per row: 256-bit key `key32`, nonce = (stream low word, stream
 * high word, prime index | batch element << 16), block counter from 0.  NTL's RandomStream (the
 * reference's source of bytes) cannot be reproduced without NTL; the sampling rule is the
 * reference's, the stream is this library's (known-answer tests: RFC 8439 2.3.2 + the oracle). */
int hx_randomize(hx_poly* p, const uint8_t* key32, uint64_t stream);
/* DoubleCRT::removePrimes: metadata only (rows are compacted on the device). */
int hx_poly_remove_primes(hx_poly* p, const int* prime_idx, int n);

/* ---------------- Cmodulus::FFT / iFFT over all rows ---------------- */
/* In place: coefficient rows (deg < phim, reduced mod q) <-> evaluation rows
 * at the primitive m-th roots, natural (Z_m^*) order.
 * src/CModulus.cpp:358-444 / :486-578 ; DoubleCRT::FFT src/DoubleCRT.cpp:68-105 */
int hx_ntt_forward(hx_poly* p);
int hx_ntt_inverse(hx_poly* p);

/* ---------------- DoubleCRT element-wise ring ops ---------------- */
/* a op= b on the rows of a; requires primes(a) subset of primes(b), otherwise
 * HX_ERR_PRIMESET (DoubleCRT::Op, src/DoubleCRT.cpp:216-273, do_mul :278-337).
 * batch(b) must equal batch(a) or be 1 (broadcast). */
int hx_add(hx_poly* a, const hx_poly* b);
int hx_sub(hx_poly* a, const hx_poly* b);
int hx_mul(hx_poly* a, const hx_poly* b);
int hx_negate(hx_poly* a); /* DoubleCRT::Negate src/DoubleCRT.cpp:363-384 */
/* a op= scalar, scalar given per row already reduced mod that row's prime
 * (DoubleCRT::Op(ZZ) src/DoubleCRT.cpp:339-361). */
int hx_add_scalar(hx_poly* a, const uint64_t* c_per_row);
int hx_sub_scalar(hx_poly* a, const uint64_t* c_per_row);
int hx_mul_scalar(hx_poly* a, const uint64_t* c_per_row);
/* DoubleCRT::operator=(ZZ) (src/DoubleCRT.cpp:866-884): every entry of row r = c_per_row[r] mod q_r */
int hx_set_scalar(hx_poly* a, const uint64_t* c_per_row);
/* DoubleCRT::Exp (src/DoubleCRT.cpp:1142-1156): entry-wise PowerMod(x, e, q_r), e >= 0 */
int hx_exp(hx_poly* a, uint64_t e);
/* DoubleCRT::automorph(k) (src/DoubleCRT.cpp:1160-1202); in place. */
int hx_automorph(hx_poly* a, uint64_t k);
/* DoubleCRT::complexConj (src/DoubleCRT.cpp:1240-1255) */
int hx_complex_conj(hx_poly* a);

/* ---------------- exact RNS basis operations ---------------- */
/* DoubleCRT::addPrimesAndScale (src/DoubleCRT.cpp:603-647): multiply rows by
 * prod(add_idx) and append zero rows for add_idx (capacity permitting). */
int hx_add_primes_and_scale(hx_poly* a, const int* add_idx, int nadd);
/* DoubleCRT::addPrimes (src/DoubleCRT.cpp:565-599): exact centred extension of
 * the RNS basis by add_idx (toPoly + FFT on the new primes), in place. */
int hx_add_primes(hx_poly* a, const int* add_idx, int nadd);
/* DoubleCRT::toPoly (src/DoubleCRT.cpp:925-1113: iFFT of every row, CRT, centring) followed by
 * PolyRed(poly, t, abs=true) (src/NumbTh.cpp:775-803), the tail of SecKey::Decrypt
 * (src/keys.cpp:1383-1405): out_host[b*phi(m) + j] = centred coefficient j of batch element b,
 * reduced into [0,t).  Exact (mixed-radix digits on the device, no big integers); `a` is unchanged.
 * t in [2, 2^60); at most 64 rows.  Synchronous (the result is on the host when it returns). */
int hx_poly_rem(const hx_poly* a, uint64_t t, uint64_t* out_host);
/* DoubleCRT::scaleDownToSet (src/DoubleCRT.cpp:1464-1516): drop drop_idx with
 * exact rounding, delta forced to 0 mod ptxt_space.  In place as far as the caller can tell: the
 * kept rows keep their order; a library-owned poly may move to another slab (hx_poly_device_ptr
 * changes), a poly made with hx_poly_wrap always has its result in the caller's buffer. */
int hx_scale_down(hx_poly* a, const int* drop_idx, int ndrop, uint64_t ptxt_space);
/* The same for several DoubleCRT objects sharing one prime set and batch (all parts of the
 * ciphertexts of one Ctxt::modDownToSet, src/Ctxt.cpp:462-465) in one pair of launches. */
int hx_scale_down_multi(hx_poly** polys, int npoly, const int* drop_idx, int ndrop,
                        uint64_t ptxt_space);
/* Ctxt::bringToSet (src/Ctxt.cpp:373-389) on several parts: modUpToSet by add_idx
 * (addPrimesAndScale) followed by modDownToSet dropping drop_idx; one fused pair of launches
 * when a single prime is dropped. */
int hx_bring_to_set_multi(hx_poly** polys, int npoly, const int* add_idx, int nadd,
                          const int* drop_idx, int ndrop, uint64_t ptxt_space);
/* Ctxt::tensorProduct of two canonical two-part ciphertexts (src/Ctxt.cpp:1563-1608) immediately followed by
 * Ctxt::bringToSet of the product -- what Ctxt::multiplyBy does between multLowLvl's tensor product and the key
 * switch (reLinearize -> dropSmallAndSpecialPrimes, src/Ctxt.cpp:720-760).  c0, c1 / d0, d1: the parts (1), (s) of
 * the two operands on one prime set; o0, o1, o2 receive the product parts (1), (s), (s^2) on that set with add_idx
 * added and drop_idx dropped (their previous contents and prime sets are irrelevant; they must not alias an operand).
 * On a power-of-two ring (N = 2^13..2^15) the product is formed inside the mod-down kernels from the operands' rows
 * and never written on the old prime set -- one dropped prime (a fresh multiply) and several (every later multiply)
 * alike; any other shape runs hx_tensor and hx_bring_to_set_multi one after the other.  Results are identical to
 * that sequence word for word.  _norms: as hx_bring_to_set_multi_norms, three
 * polys. */
int hx_tensor_bring_to_set(const hx_poly* c0, const hx_poly* c1, const hx_poly* d0, const hx_poly* d1,
                           hx_poly* o0, hx_poly* o1, hx_poly* o2, const int* add_idx, int nadd,
                           const int* drop_idx, int ndrop, uint64_t ptxtSpace);
int hx_tensor_bring_to_set_norms(const hx_poly* c0, const hx_poly* c1, const hx_poly* d0, const hx_poly* d1,
                                 hx_poly* o0, hx_poly* o1, hx_poly* o2, const int* add_idx, int nadd,
                                 const int* drop_idx, int ndrop, uint64_t ptxtSpace, double* norms);

/* DoubleCRT::breakIntoDigits (src/DoubleCRT.cpp:479-561).  a has ctxt primes
 * only; digit d = dig_idx[dig_off[d]..dig_off[d+1]); special primes sp_idx.
 * digits_out: poly with ndig*(nrows(a)+nsp) rows, block d holding digit d on
 * primes(a) followed by sp_idx. */
int hx_break_into_digits(const hx_poly* a, const int* dig_idx, const int* dig_off, int ndig,
                         const int* sp_idx, int nsp, hx_poly* digits_out);

/* ---------------- environment switches ----------------
 * None is needed in production: each selects the older or the generic form of a path, for tests that must reach it
 * and for same-box A/B measurements; results are bit-identical either way.  The library snapshots them when a
 * context is created (hx_ctx_create; helib_amd/csrc/switches.h is the one place that reads the environment).
 *   HX_HPS_EPS=x, HX_HPS_MIN_N=n              exact-RNS kernels: the trust margin of an HPS quotient (default 2^-30); the
 *                                            HPS front end instead of Garner from n sources on (9; the digit kernel: 5)
 *   HX_NO_MFMA_EXT, HX_MFMA_MIN_N=n           basis extension: VALU limb products instead of the matrix-core kernel; the
 *                                            matrix-core kernel from n sources on (9)
 *   HX_NO_MASK_SPLIT                          hx_mask_split as hx_poly_copy + hx_mul + hx_sub per part
 *   HX_NO_MASK_FAN                            hx_mask_fan as hx_poly_copy + hx_mul per output and part
 *   HX_NO_MULRELIN_FUSE                       tensor product as a pass of its own inside hx_mul_relin
 *   HX_NO_KS_LAST_FUSE                        relinearisation: every extension row transformed by the row kernel and the key
 *                                            switch as a launch of its own, instead of each output row's last digit transform
 *                                            fused into the key switch
 *   HX_NO_PREP_FUSE                           single-prime mod-switch: S by a kernel of its own behind the prep kernel, the
 *                                            norm of its (x, S) block by a norm kernel, N = 2^14 norms in the paired form --
 *                                            instead of S (and that norm) formed in the prep kernel's workgroup
 *   HX_NO_PROTH                               row transforms: Shoup butterflies on every row (by default rows of primes
 *                                            q = 1 mod 2^32 -- every chain prime of the benchmarks -- run the Proth-form ones)
 *   HX_NO_PROTH_RNS                           exact-RNS kernels: Barrett / Shoup products on Proth-form primes too (by default
 *                                            their Garner steps, target sums and fix-ups are Montgomery products; HX_NO_PROTH
 *                                            implies it)
 *   HX_BLUE_OLD                               general m: the chain of passes instead of one convolution kernel
 *   HX_NO_PFA                                 m = 21845: Bluestein instead of the Good-Thomas x Rader kernels
 *   HX_PFA_NO_REM                             ... their inverse without the fused rem Phi_m (two convolution launches instead)
 *   HX_WAIT_POLL_US=n                         how long a norm read-back is polled for before the thread sleeps (2000)
 *   HX_ARENA_TRACE                            one line on stderr per hipMalloc of the slab arena
 * (The C++ host, include/helib_amd_ctxt.hpp, reads none of its own.) */

/* ---------------- ciphertext-level fused loops ---------------- */
/* KeySwitch matrix W (include/helib/keySwitching.h:86-101) with the a-column
 * expanded once by the host (HElib regenerates it from W.prgSeed on every key
 * switch, src/Ctxt.cpp:196-206).  b, a: host arrays [ndig][nrows][phim] on
 * primes row_idx[nrows] (ctxt primes followed by special primes).
 * On a power-of-two ring with log N in 13 .. 15 the matrix also holds its rows times 2^64 mod q (the fused key
 * switch's Montgomery store loop reads them): twice the device memory, converted here, once. */
int hx_ksk_create(hx_ctx* ctx, int ndig, const int* row_idx, int nrows, const uint64_t* b,
                  const uint64_t* a, hx_ksk** out);
int hx_ksk_destroy(hx_ksk* k);
/* the matrix back on the host, for a checker or for another process that is to hold the same key (one key pair
 * replicated over the GPUs of a node): shape first (row_idx_out may be NULL), then b, a =
 * [ndig][nrows][phim] as hx_ksk_create took them (KeySwitch::b / the expanded a column, include/helib/keySwitching.h:86-101) */
int hx_ksk_shape(const hx_ksk* k, int* ndig, int* nrows, int* row_idx_out /* nrows */);
int hx_ksk_download(const hx_ksk* k, uint64_t* b, uint64_t* a);   /* synchronous */

/* Ctxt::tensorProduct for two 2-part ciphertexts (src/Ctxt.cpp:1576-1597):
 * o0 = c0*d0, o1 = c0*d1 + c1*d0, o2 = c1*d1. */
int hx_tensor(const hx_poly* c0, const hx_poly* c1, const hx_poly* d0, const hx_poly* d1,
              hx_poly* o0, hx_poly* o1, hx_poly* o2);
/* Ctxt::keySwitchDigits (src/Ctxt.cpp:191-230):
 * out0 += sum_d digit_d*b_d ; out1 += sum_d digit_d*a_d */
int hx_key_switch_digits(const hx_poly* digits, const hx_ksk* W, hx_poly* out0, hx_poly* out1);

/* Ctxt::multiplyBy data path at a fixed level: tensorProduct + reLinearize
 * (src/Ctxt.cpp:1563-1608, :720-842).  Inputs: 2-part ciphertexts (c0,c1),
 * (d0,d1) on the same ctxt primes; outputs (out0,out1) on ctxt ∪ special
 * primes (W's row set), exactly what reLinearize leaves in the Ctxt.
 * Digits as in hx_break_into_digits. */
int hx_mul_relin(const hx_poly* c0, const hx_poly* c1, const hx_poly* d0, const hx_poly* d1,
                 const hx_ksk* W, const int* dig_idx, const int* dig_off, int ndig,
                 hx_poly* out0, hx_poly* out1);
/* ... with the digit norms of hx_relinearize_norms: norms[d * batch + b] (what keySwitchPart multiplies by the
 * matrix' noise bound, src/Ctxt.cpp:828-841) */
int hx_mul_relin_norms(const hx_poly* c0, const hx_poly* c1, const hx_poly* d0, const hx_poly* d1,
                       const hx_ksk* W, const int* dig_idx, const int* dig_off, int ndig,
                       hx_poly* out0, hx_poly* out1, double* norms);

/* Ctxt::reLinearize of a 3-part ciphertext (1, s, s^2) (src/Ctxt.cpp:720-786, keySwitchPart
 * :805-842): parts (1),(s) get addPrimesAndScale(special), part s^2 is broken into digits and
 * multiplied by W.  W may cover more ctxt primes than the parts currently have (lower level);
 * digits = the context's digits restricted to the parts' primes (leading digits of W).
 * out0/out1: primes(t0) followed by sp_idx.
 * t1 may be NULL: no part points at s -- the (1, s(X^k)) ciphertext that Ctxt::smartAutomorph
 * relinearises after Ctxt::automorph (src/Ctxt.cpp:2437-2515), t2 then being the s(X^k) part and
 * W the matrix for that automorphism. */
int hx_relinearize(const hx_poly* t0, const hx_poly* t1, const hx_poly* t2, const hx_ksk* W,
                   const int* dig_idx, const int* dig_off, int ndig, const int* sp_idx, int nsp,
                   hx_poly* out0, hx_poly* out1);

/* ---------------- measured noise: canonical-embedding norms ----------------
 * embeddingLargestCoeff (src/norms.cpp:129-262,480-493): max over j in Z_m^* of |f(W^j)|,
 * W = exp(2 pi i/m), evaluated on the device in double precision (the reference uses PGFFT,
 * src/PGFFT.cpp); parity is to a relative tolerance of 1e-9.  m a power of two, or any
 * m <= 131072 (complex-double Bluestein); beyond that HX_ERR_UNSUPPORTED: the host keeps the
 * reference's high-probability bound, src/DoubleCRT.cpp:520-529.  These calls synchronise the stream: the numbers land in host
 * memory.  The arithmetic results are exactly those of the plain calls. */
/* Deferred read-back: after hx_ctx_defer_norms(ctx, 1) the *_norms calls do not synchronise;
 * their `norms` arrays (which must stay valid) are filled by hx_norms_flush(ctx), which waits only
 * for the norm kernels already enqueued, not for work enqueued after them -- the host can keep
 * the GPU fed while it waits for the numbers its next prime-set decision needs.
 * hx_ctx_defer_norms(ctx, 0) flushes and returns to synchronous behaviour. */
int hx_ctx_defer_norms(hx_ctx* ctx, int on);
int hx_norms_flush(hx_ctx* ctx);
/* rows real polynomials of phi(m) coefficients each (host) -> norms_out[rows] (host) */
int hx_embedding_norm(hx_ctx* ctx, const double* f_host, int rows, double* norms_out);
/* hx_scale_down_multi + norms[npoly*batch] = embeddingLargestCoeff(fdelta) with
 * fdelta = delta/diffProd (src/Ctxt.cpp:466-507); fdelta (optional, host,
 * [npoly][batch][phim]) receives the coefficients themselves. */
int hx_scale_down_multi_norms(hx_poly** polys, int npoly, const int* drop_idx, int ndrop,
                              uint64_t ptxt_space, double* norms, double* fdelta);
int hx_bring_to_set_multi_norms(hx_poly** polys, int npoly, const int* add_idx, int nadd,
                                const int* drop_idx, int ndrop, uint64_t ptxt_space,
                                double* norms);
/* hx_break_into_digits + its return value (src/DoubleCRT.cpp:538-545) in pieces:
 * norms[d*batch+b] = embeddingLargestCoeff(digit d of element b) / P_d, P_d = product of the
 * digit's primes (multiplied back by the host in extended range). */
int hx_break_into_digits_norms(const hx_poly* a, const int* dig_idx, const int* dig_off, int ndig,
                               const int* sp_idx, int nsp, hx_poly* digits_out, double* norms);
/* hx_relinearize + the digit norms Ctxt::keySwitchPart multiplies by W.noiseBound
 * (src/Ctxt.cpp:828-829); layout as above. */
int hx_relinearize_norms(const hx_poly* t0, const hx_poly* t1, const hx_poly* t2, const hx_ksk* W,
                         const int* dig_idx, const int* dig_off, int ndig, const int* sp_idx,
                         int nsp, hx_poly* out0, hx_poly* out1, double* norms);

/* ---------------- CKKS slots: EncryptedArrayCx (src/EaCx.cpp) ----------------
 * m a power of two with 16 <= m <= 2^17 (N = phi(m) = m/2 <= 2^16); a larger m is HX_ERR_UNSUPPORTED, an m that is
 * not a power of two HX_ERR_INVALID ("CKKS scheme only supports m as a power of two.", src/PAlgebra.cpp:463-467).
 * Slot vectors are complex doubles (interleaved re, im) in PAlgebra's slot order: slot s is the value at
 * zeta^-T[m/4-1-s], zeta = exp(2 pi i/m), T[i] = 3^i mod m (ith_rep of Z_m^* / <-1>, src/PAlgebra.cpp:520-570).
 * Double precision on the device; all three calls synchronise the context's stream. */
/* CKKS_embedInSlots (src/norms.cpp:574-615) of `batch` vectors of nslots <= m/4 slots each ([batch][nslots]; missing
 * slots are 0), scaled by `scaling`, rounded as std::round; `out` (batch elements, its own prime set) receives the
 * coefficients' residues in evaluation form (the DoubleCRT of the zzX, replacing a host encode + upload + FFT);
 * coeffs_out (optional, host, [batch][phi(m)]) the zzX itself.  A coefficient outside the range of a long:
 * HX_ERR_INVALID "overflow in encoding" (out then holds no meaningful value). */
int hx_ckks_encode(hx_ctx* ctx, const double* slots, int batch, int nslots, double scaling, hx_poly* out,
                   int64_t* coeffs_out);
/* CKKS_canonicalEmbedding (src/norms.cpp:495-519) of `batch` real polynomials of phi(m) coefficients (host
 * [batch][phi(m)]) -> slots_out[batch][m/4] (host, complex). */
int hx_ckks_embed(hx_ctx* ctx, const double* coeffs, int batch, double* slots_out);
/* The decode of EncryptedArrayCx::rawDecrypt (src/EaCx.cpp:62-86 -> CKKS_decode): p = sum_parts part * s^r in
 * evaluation form, as SecKey::Decrypt's inner product leaves it (at most 64 primes; p is unchanged) ->
 * slots_out[batch][m/4] = canonicalEmbedding(centred CRT value / ratFactor), ratFactor = exp(ln_rat_factor).  The
 * division is DecryptCKKS's (include/helib_amd_keys.hpp): Garner digits weighted by P_k / ratFactor, on the device;
 * one download. */
int hx_ckks_decode(const hx_poly* p, double ln_rat_factor, double* slots_out);

/* ---------------- BGV slots: EncryptedArray for d = ord_m(p) = 1, r = 1 (src/EncryptedArray.cpp) ----------------
 * The plaintext prime p splits Phi_m completely (p = 1 mod m): phi(m) slots, each an element of Z_p.  Factor 0 of
 * Phi_m mod p is X - rho with rho the largest primitive m-th root of unity mod p (the smallest factor by poly_comp,
 * src/PAlgebra.cpp:67-81), factor i is X - rho^(1/t_i mod m), t_i = ith_rep(i) of Z_m^* in hypercube order
 * (src/PAlgebra.cpp:520-570, 726-733).  Slot vectors are int64; the encoding of a is the H of degree < phi(m) with
 * H(rho^(1/t_i)) = a_i mod p for every i.  Rings: m a power of two with 16 <= m <= 2^17, or any other m >= 3 through
 * the general transform (an even m that is not a power of two needs 2m | p - 1, else HX_ERR_UNSUPPORTED).  All calls
 * synchronise the context's stream and fail with HX_ERR_INVALID under an open graph capture. */
typedef struct hx_bgv_slots hx_bgv_slots; /* the tables of one (context, p) pair */
/* p not a prime below 2^60, or p | m: HX_ERR_INVALID.  d = ord_m(p) > 1: HX_ERR_UNSUPPORTED, the message names d.  p
 * becomes the only prime of a side context of the table: the primes of ctx and their indices are untouched.  Destroy
 * the table before its context. */
int hx_bgv_slots_create(hx_ctx* ctx, uint64_t p, hx_bgv_slots** out);
int hx_bgv_slots_destroy(hx_bgv_slots* t);
/* p, rho, and the hypercube of Z_m^*: ndims generators with their orders (at most 8 are written); any output may be
 * NULL. */
int hx_bgv_slots_info(const hx_bgv_slots* t, uint64_t* p, uint64_t* rho, int* ndims, uint64_t* gens, uint64_t* ords);
/* EncryptedArray::encode (src/EncryptedArray.cpp:438-447) of `batch` vectors of nslots <= phi(m) integers each
 * ([batch][nslots], host; missing slots are 0, any int64 is reduced mod p): `out` (batch elements on its own prime
 * set, a poly of the table's context) receives balanced(mul * H mod p) in evaluation form -- mul = 1 is the plain
 * encoding, mul = Q mod p the balanced_MulMod of PubKey::Encrypt (src/keys.cpp:358-488); coeffs_out (optional, host,
 * [batch][phi(m)]) receives that zzX, every coefficient in (-p/2, p/2). */
int hx_bgv_encode(const hx_bgv_slots* t, const int64_t* slots, int batch, int nslots, uint64_t mul, hx_poly* out,
                  int64_t* coeffs_out);
/* The decode behind SecKey::Decrypt (src/keys.cpp:1383-1405): acc = sum_parts part * s^r in evaluation form (at most
 * 64 primes; unchanged) -> slots_out[batch][phi(m)] (host) in [0, p): the centred CRT value reduced mod p (the
 * arithmetic of hx_poly_rem, kept on the device), times factor_inv mod p (the inverse of productOfPrimes * intFactor;
 * 1 if none), evaluated at the slots.  One download. */
int hx_bgv_decode(const hx_bgv_slots* t, const hx_poly* acc, uint64_t factor_inv, int64_t* slots_out);
/* EncryptedArray::decode of `batch` plaintext polynomials (host, [batch][phi(m)], any int64) -> slots_out as above. */
int hx_bgv_embed(const hx_bgv_slots* t, const int64_t* coeffs, int batch, int64_t* slots_out);
/* The constants of MatMul1DExec / MatMulFullExec (src/matmul.cpp:604-643, 2035-2075), read out of a matrix that lives
 * on the device.  hx_bgv_matrix_create uploads a_host ([rows][cols], any int64; entries count mod p) once.  dim = -1:
 * a full matrix, rows = cols = phi(m), indexed by slot; dim = i: a D x D matrix for dimension i of the hypercube,
 * D = ords[i], indexed by the coordinate in that dimension.  Any other shape or dim: HX_ERR_INVALID.  Destroy the
 * matrix before its table. */
typedef struct hx_bgv_matrix hx_bgv_matrix;
int hx_bgv_matrix_create(const hx_bgv_slots* t, const int64_t* a_host, int rows, int cols, int dim, hx_bgv_matrix** out);
int hx_bgv_matrix_destroy(hx_bgv_matrix* a);
/* One diagonal.  Slot s has the hypercube coordinates c (the last dimension fastest); s0 is s with c[rot_dim] replaced
 * by c[rot_dim] - rot_amt (plaintextAutomorph at d = 1, build_ConstMultiplier, src/matmul.cpp:375-389; rot_dim = -1:
 * no rotation).  The slot's value is
 *   full matrix       A[r, s0], r the slot with the coordinates c_i(s0) - off[i] in every dimension i
 *                     (MatMulFullHelper::processDiagonal over the accumulated rotate1D of the index vector, :1998-2024,
 *                     2060-2072)
 *   dimension dim     A[c_dim(s0) - off[dim], c_dim(s0)]   (processDiagonal1, :449-504)
 * every difference taken modulo the order of its dimension; off and rot_amt may be any int32. */
typedef struct hx_bgv_diag {
  int32_t off[8];
  int32_t rot_dim, rot_amt;
} hx_bgv_diag;
/* out (batch ndiag on its own prime set, as for hx_bgv_encode) receives the balanced encoding, in evaluation form, of
 * the ndiag diagonals d[] of a; coeffs_out (optional) their zzX as in hx_bgv_encode; nonzero_out[t] = 0 exactly when
 * every slot of diagonal t is 0 mod p (the reference keeps no multiplier for it, :369-372).  out = NULL (then
 * coeffs_out = NULL too) computes the flags alone: one pass over the matrix words, no transform.  Preconditions and
 * errors as for hx_bgv_encode; a matrix of another table and a rot_dim outside [-1, ndims) are HX_ERR_INVALID; a
 * refused call touches no output.  The scratch grows with ndiag * phi(m): callers pass the diagonals in chunks. */
int hx_bgv_encode_diagonals(const hx_bgv_slots* t, const hx_bgv_matrix* a, const hx_bgv_diag* d, int ndiag, hx_poly* out,
                            int64_t* coeffs_out, int* nonzero_out);

/* ---------------- BGV slots for any d = ord_m(p): integer slots mod p, or mod p^r (bgv_crt.hip) ----------------
 * The default-constructed EncryptedArray (G = X, include/helib/EncryptedArray.h): Phi_m mod p has nslots = phi(m) / d
 * factors of degree d and a slot holds an integer mod p.  Factor 0 is the smallest by poly_comp
 * (src/PAlgebra.cpp:67-81, 715-721), factor i the minimal polynomial of X^(1/t_i) mod F_0, t_i = ith_rep(i) of
 * Z_m^* / <p> in hypercube order (:726-733).  The maps are two nslots x phi(m) matrices modulo p, uint32 words on the
 * device: E, row i the idempotent of factor i (CRT_reconstruct of constants, :1007-1045, crtCoeffs :750-756), and R,
 * R[i][k] = the constant term of X^k mod F_i (CRT_decompose :885-936, decodePlaintext's degG == 1 branch :1243-1261).
 * Any ring the context itself supports; all calls synchronise the context's stream and fail with HX_ERR_INVALID
 * under an open graph capture. */
typedef struct hx_bgv_crt hx_bgv_crt; /* the tables of one (context, p) pair */
/* Replaces PAlgebraModDerived's constructor at r = 1 (src/PAlgebra.cpp:680-772; hx_bgv_crt_create_pr takes any r).  p not a prime, or p | m:
 * HX_ERR_INVALID.  A prime p >= 2^31 (the tables hold 32-bit words), a table above 1 GiB, m < 3: HX_ERR_UNSUPPORTED,
 * the message gives the figure.  Any d is accepted, d = 1 included.  Destroy the table before its context. */
int hx_bgv_crt_create(hx_ctx* ctx, uint64_t p, hx_bgv_crt** out);
/* The same constructor for the plaintext space p^r, r >= 1 (its r > 1 branch, src/PAlgebra.cpp:757-763 over
 * PAlgebraLift, :840-881): the factors are found and ordered modulo p as above and Hensel-lifted, E and R are the
 * same two matrices modulo p^r, and a slot holds an integer mod p^r.  hx_bgv_crt_encode, _decode and _embed then work
 * modulo p^r wherever their descriptions say p (mul and factor_inv are reduced mod p^r); at an even p^r a coefficient
 * equal to p^r / 2 is encoded as +p^r / 2 (the reference draws its sign at random, src/zzX.cpp:122-137).  The tables
 * reduced mod p^k, k < r, are the tables of p^k.  r = 1 is hx_bgv_crt_create, table for table.  r < 1: HX_ERR_INVALID;
 * p^r >= 2^31: HX_ERR_UNSUPPORTED with the figure; otherwise the errors of hx_bgv_crt_create. */
int hx_bgv_crt_create_pr(hx_ctx* ctx, uint64_t p, int r, hx_bgv_crt** out);
int hx_bgv_crt_destroy(hx_bgv_crt* t);
/* The exponent r and the modulus p^r of the table's maps (hx_bgv_crt_info gives p); either output may be NULL. */
int hx_bgv_crt_space(const hx_bgv_crt* t, int* r, uint64_t* modulus);
/* p, d, nslots, the hypercube of Z_m^* / <p> -- ndims generators with their orders, a non-native dimension's order
 * negated as Context::writeTo stores it (src/PAlgebra.cpp:470-507; at most 8 are written) -- and the bytes of E and
 * R together; any output may be NULL. */
int hx_bgv_crt_info(const hx_bgv_crt* t, uint64_t* p, int* d, int* nslots, int* ndims, uint64_t* gens, int64_t* ords,
                    uint64_t* table_bytes);
/* EncryptedArray::encode (src/EncryptedArray.cpp:438-447) of `batch` vectors of nslots integers ([batch][nslots],
 * host; any int64 is reduced mod p).  out, mul and coeffs_out as for hx_bgv_encode; for p = 2 a coefficient is 0 or 1
 * (the reference draws the sign of a 1 at random, src/zzX.cpp:139-154). */
int hx_bgv_crt_encode(const hx_bgv_crt* t, const int64_t* slots, int batch, uint64_t mul, hx_poly* out, int64_t* coeffs_out);
/* As hx_bgv_decode (src/keys.cpp:1383-1405, then EncryptedArray::decode): -> slots_out[batch][nslots] in [0, p). */
int hx_bgv_crt_decode(const hx_bgv_crt* t, const hx_poly* acc, uint64_t factor_inv, int64_t* slots_out);
/* EncryptedArray::decode (src/EncryptedArray.cpp:461-470) of `batch` plaintext polynomials (host, [batch][phi(m)], any
 * int64) -> slots_out[batch][nslots] in [0, p). */
int hx_bgv_crt_embed(const hx_bgv_crt* t, const int64_t* coeffs, int batch, int64_t* slots_out);

/* ---------------- BGV slots in GF(p^d) = Z_p[X] / G, G = F_0, d = ord_m(p), r = 1 (bgv_gf.hip) ----------------
 * EncryptedArray(context, G) with G the first factor of Phi_m mod p (the one hx_bgv_crt numbers 0): slot i holds a
 * polynomial alpha_i of degree < d over Z_p, d int64 words lowest coefficient first, read modulo G.  The plaintext is
 * H = sum_i alpha_i(X^(t_i)) E_i mod (Phi_m, p) (PAlgebraModDerived::embedInSlots and CRT_reconstruct with the
 * G = F_0 special case, src/PAlgebra.cpp:1064-1067, 1096-1100, 1168-1186, and matrix_maps), and slot i of a
 * plaintext w is (w mod F_i)(X^(1/t_i)) mod G (decodePlaintext, :1243-1278).  A slot (a, 0, ..., 0) is the integer a
 * of hx_bgv_crt, word for word; d = 1 is hx_bgv_crt.  The tables stay nslots x phi(m): E, the decode rows run d - 1
 * words further, two d x d maps per slot and d - 1 rows X^(phi(m) + u) mod Phi_m.  Calls synchronise the context's
 * stream and fail with HX_ERR_INVALID under an open graph capture. */
typedef struct hx_bgv_gf hx_bgv_gf; /* the tables of one (context, p) pair */
/* Replaces PAlgebraModDerived's constructor and mapToSlots at G = F_0 (src/PAlgebra.cpp:680-772, 1116-1186).  The
 * refusals of hx_bgv_crt_create, and d > 64: HX_ERR_UNSUPPORTED with the figures. */
int hx_bgv_gf_create(hx_ctx* ctx, uint64_t p, hx_bgv_gf** out);
/* The same tables for the plaintext space p^r, r >= 1: a slot is an element of the Galois ring Z_(p^r)[X] / G, G the
 * Hensel lift of F_0 (the EncryptedArray RecryptData::init builds over p^(e - e' + r), src/recryption.cpp:310-343).
 * Every table is the same formula modulo p^r over the lifted factors of hx_bgv_crt_create_pr -- the lift of a
 * factorisation is unique, so X -> X^(t_i) carries the lifted F_0 to the lifted F_i -- and the per-slot map is inverted
 * with pivots that are units.  hx_bgv_gf_encode, _decode and _embed then work modulo p^r wherever their descriptions
 * say p; hx_bgv_gf_info gives the prime and the lifted G; a slot (a, 0, ..., 0) is the integer a of
 * hx_bgv_crt_create_pr, word for word.  r = 1 is hx_bgv_gf_create, byte for byte.  r < 1: HX_ERR_INVALID; p^r >= 2^31:
 * HX_ERR_UNSUPPORTED with the figure; otherwise the errors of hx_bgv_gf_create.  hx_bgv_gf_matrix_create refuses a
 * table with r > 1; hx_bgv_gr_matrix_create takes it. */
int hx_bgv_gf_create_pr(hx_ctx* ctx, uint64_t p, int r, hx_bgv_gf** out);
/* hx_bgv_gf_create_pr over a hypercube the caller chooses: slot i belongs to t_i = prod_j gens[j]^(e_j), (e_0, ..)
 * the i-th exponent vector with the last generator's exponent fastest, 0 <= e_j < |ords[j]| -- what PAlgebra's
 * constructor does with ContextBuilder.gens().ords() (src/PAlgebra.cpp:476-509).  As there (:497-501) a supplied sign
 * is not trusted: the order is |ords[i]| and hx_bgv_gf_info reports it negated when gens[i]^|ords[i]| != 1 mod m.
 * EvalMap needs such a hypercube: dimension i generated by an element that is 1 modulo every factor of m but the i-th
 * (src/EvalMap.cpp:42-105).  ngens = 0 is hx_bgv_gf_create_pr, byte for byte.  Refused with HX_ERR_INVALID and the
 * figures, before any device allocation: more than 8 generators, a generator not coprime to m, orders that do not
 * multiply to phi(m) / d, exponent vectors that do not enumerate Z_m^* / <p> exactly once. */
int hx_bgv_gf_create_gens(hx_ctx* ctx, uint64_t p, int r, const uint64_t* gens, const int64_t* ords, int ngens, hx_bgv_gf** out);
/* The exponent r and the modulus p^r of the table's maps (hx_bgv_gf_info gives p); either output may be NULL. */
int hx_bgv_gf_space(const hx_bgv_gf* t, int* r, uint64_t* modulus);
int hx_bgv_gf_destroy(hx_bgv_gf* t);
/* As hx_bgv_crt_info; table_bytes counts every device table; G receives d + 1 words, the constant coefficient first
 * (PAlgebraMod::getFactors()[0], src/PAlgebra.cpp:715-721).  Any output may be NULL. */
int hx_bgv_gf_info(const hx_bgv_gf* t, uint64_t* p, int* d, int* nslots, int* ndims, uint64_t* gens, int64_t* ords,
                   uint64_t* table_bytes, uint64_t* G);
/* EncryptedArray::encode (src/EncryptedArray.cpp:438-447 over src/PAlgebra.cpp:1064-1100, 1007-1045) of `batch`
 * vectors of nslots slots ([batch][nslots][d], host; any int64 is reduced mod p).  out, mul and coeffs_out as for
 * hx_bgv_crt_encode. */
int hx_bgv_gf_encode(const hx_bgv_gf* t, const int64_t* slots, int batch, uint64_t mul, hx_poly* out, int64_t* coeffs_out);
/* As hx_bgv_crt_decode (src/keys.cpp:1383-1405, then EncryptedArray::decode over src/PAlgebra.cpp:1243-1278):
 * -> slots_out[batch][nslots][d] in [0, p). */
int hx_bgv_gf_decode(const hx_bgv_gf* t, const hx_poly* acc, uint64_t factor_inv, int64_t* slots_out);
/* EncryptedArray::decode (src/EncryptedArray.cpp:461-470 over src/PAlgebra.cpp:1243-1278) of `batch` plaintext
 * polynomials (host, [batch][phi(m)], any int64) -> slots_out[batch][nslots][d] in [0, p). */
int hx_bgv_gf_embed(const hx_bgv_gf* t, const int64_t* coeffs, int batch, int64_t* slots_out);

/* ---------------- linear maps on GF(p^d) slots: the constants of linearized polynomials (bgv_gf_linalg.hip) ------------
 * A Z_p-linear map of a slot is sum_k C[k] alpha^(p^k) (EncryptedArrayDerived::buildLinPolyCoeffs,
 * src/EncryptedArray.cpp:760-798).  The host tables: frob[e][l] = X^(l p^e) mod G ([d][d][d] words), K = the inverse of
 * M[i][j] = (X^j)^(p^i) over the field ([d][d] elements of d words: buildLinPolyMatrix + ppInvert,
 * src/NumbTh.cpp:1099-1111, src/EncryptedArray.cpp:783-787) and the flat table T[(j,b)][(k,c)] = [X^c](X^b K[j][k] mod G)
 * ([d^2][d^2] words) with C = E T for the map sending X^j to sum_b E[j][b] X^b.  Host only; any output may be NULL.
 * G: d + 1 words, monic.  d > 64 or p >= 2^31: HX_ERR_UNSUPPORTED. */
int hx_bgv_gf_linalg_tables(uint64_t p, int d, const uint64_t* G, uint32_t* frob_out, uint32_t* K_out, uint32_t* T_out);
typedef struct hx_bgv_gf_matrix hx_bgv_gf_matrix; /* a matrix of GF(p^d) entries or d x d blocks on the device */
/* The matrix of a MatMul1D with entries in GF(p^d) (block = 0: words[nb][D][D][d]) or of a BlockMatMul1D (block = 1:
 * words[nb][D][D][d][d], entry row j = the image of X^j), uint32 words below p on the host.  blk[s], col[s] (nslots
 * each) name the transform and the column slot s reads (PAlgebra::breakIndexByDim; the size-1 dimension of
 * BlockMatMul1DExec has blk[s] = s, col[s] = 0, D = 1).  For blocks every entry's linearized-polynomial coefficients
 * [d][d] are formed here, once, by one product [nb D D, d^2] x [d^2, d^2] modulo p on the device (replaces
 * buildLinPolyCoeffs per entry in processDiagonal1/2, src/matmul.cpp:1369-1373, 1452-1457).  Words not below p, blk or
 * col out of range: HX_ERR_INVALID.  Synchronises the context's stream.  Destroy the matrix before its context. */
int hx_bgv_gf_matrix_create(hx_ctx* ctx, const hx_bgv_gf* t, int block, int nb, int D, const uint32_t* words, const int32_t* blk,
                            const int32_t* col, hx_bgv_gf_matrix** out);
int hx_bgv_gf_matrix_destroy(hx_bgv_gf_matrix* a);
/* The words the gather reads: [nb D D][d][d] coefficients (row k = C[k]) for blocks, the entries themselves otherwise. */
int hx_bgv_gf_matrix_coeffs(const hx_bgv_gf_matrix* a, uint32_t* out);
/* One constant: slot s, with (src, e) = maps[map][s] (two int32 per slot), holds zero when src = -1 and otherwise
 * Frob^e of coefficient k (0 for GF entries) of the entry [(col[src] - diag) mod D, col[src]] of transform blk[src]. */
typedef struct hx_bgv_gf_desc {
  int32_t diag, k, map;
} hx_bgv_gf_desc;
/* slots_out[ndesc][nslots][d] (host, the layout hx_bgv_gf_encode reads) and nonzero_out[ndesc] (0 exactly when every
 * word of the constant is 0).  Replaces the slot-by-slot transposition and the poly-space plaintextAutomorph / mask
 * products of build_ConstMultiplier(poly, -1, -j), (poly, dim, -i), the masked halves and (poly1, dim, D)
 * (src/matmul.cpp:375-389, 1392-1400, 1467-1475, 1560-1651): a plaintext automorphism permutes slots and applies a
 * power of the Frobenius to each.  Anything out of range: HX_ERR_INVALID before the device is touched. */
int hx_bgv_gf_gather(const hx_bgv_gf_matrix* a, const hx_bgv_gf_desc* descs, int ndesc, const int32_t* maps, int nmaps,
                     int64_t* slots_out, int* nonzero_out);

/* ---------------- linear maps on Galois-ring slots modulo p^r (bgv_gf_linalg.hip) ----------------
 * Over Z_(p^r)[X] / G, G the Hensel lift of F_0, a Z_(p^r)-linear map of a slot is sum_k C[k] sigma^k(alpha) with
 * sigma: X -> X^p (EncryptedArrayDerived::buildLinPolyCoeffs with its ppsolve branch, src/EncryptedArray.cpp:740-798).
 * hx_bgv_gf_linalg_tables modulo P = p^r: frob[e][l] = X^(l p^e) mod G mod P, K = the inverse over the ring of the Moore
 * matrix M[i][j] = sigma^i(X^j) (buildLinPolyMatrix + ppInvert, src/NumbTh.cpp:1099-1111, src/EncryptedArray.cpp:783-787;
 * here through the Gram matrix of traces, inverted with pivots that are units) and the flat table T.  G: d + 1 words,
 * monic, the lifted F_0.  r = 1 gives hx_bgv_gf_linalg_tables byte for byte, and the tables reduced mod p are the r = 1
 * tables.  r < 1: HX_ERR_INVALID; d > 64 or p^r >= 2^31: HX_ERR_UNSUPPORTED. */
int hx_bgv_gr_linalg_tables(uint64_t p, int r, int d, const uint64_t* G, uint32_t* frob_out, uint32_t* K_out, uint32_t* T_out);
/* hx_bgv_gf_matrix_create over a table of any r >= 1 (hx_bgv_gf_create or hx_bgv_gf_create_pr): the same contract with
 * the modulus p^r where that one says p -- words below p^r, the coefficients of every block formed modulo p^r on the
 * device (replaces buildLinPolyCoeffs per entry in BlockMatMul1D_derived_impl::processDiagonal1/2 over p^r,
 * src/matmul.cpp:1369-1373, 1452-1457).  hx_bgv_gf_matrix_destroy, hx_bgv_gf_matrix_coeffs and hx_bgv_gf_gather work on
 * the handle unchanged.  hx_bgv_gf_matrix_create keeps refusing r > 1. */
int hx_bgv_gr_matrix_create(hx_ctx* ctx, const hx_bgv_gf* t, int block, int nb, int D, const uint32_t* words, const int32_t* blk,
                            const int32_t* col, hx_bgv_gf_matrix** out);
/* hx_bgv_gf_gather and hx_bgv_gf_encode in one call, the constants never leaving the device: for every descriptor the
 * CRT components the encode reads -- gather, sigma^e and the per-slot map in one kernel -- then the encode itself
 * (replaces build_ConstMultiplier's poly-space plaintextAutomorph / mask products and the encode of every constant of
 * BlockMatMul1DExec_construct / MatMul1DExec_construct, src/matmul.cpp:375-389, 626-688, 1537-1658).  out (batch ndesc on
 * its own prime set), mul and coeffs_out as for hx_bgv_gf_encode: the same words as hx_bgv_gf_encode of
 * hx_bgv_gf_gather's slots, a zero polynomial for a constant that is zero.  nonzero_out[ndesc] as for hx_bgv_gf_gather.
 * out = NULL (then coeffs_out = NULL too) computes the flags alone and writes no row.  The matrix must have been built
 * over t's context, modulus and geometry.  Null arguments, anything out of range, another context: HX_ERR_INVALID
 * before the device is touched; fails with HX_ERR_INVALID under an open graph capture. */
int hx_bgv_gf_encode_gathered(const hx_bgv_gf* t, const hx_bgv_gf_matrix* a, const hx_bgv_gf_desc* descs, int ndesc,
                              const int32_t* maps, int nmaps, uint64_t mul, hx_poly* out, int64_t* coeffs_out, int* nonzero_out);

/* ---------------- fused multiply-add of the matrix product (linalg.hip) ---------------- */
/* out0 (+)= sum_t c[t] * in0[t],  out1 (+)= sum_t c[t] * in1[t]   (t < n), row by row modulo each prime.
 * Replaces n x { tmp = b; tmp *= a; x += tmp }: MulAdd, src/matmul.cpp:391-408, and DoubleCRT::Mul with
 * matchIndexSets = false (the inner loop of MatMul1DExec::mul, src/matmul.cpp:973-1110, 1220-1322).
 * All operands are in evaluation form, words canonical in [0, q); the result equals, word for word, the
 * hx_mul / hx_add sequence.  in0[t], in1[t] have the batch and the prime set (same order) of out0, out1; in1 and
 * out1 may both be null (a one-part ciphertext).  c[t] has batch 1 (broadcast over the batch) or the outputs'
 * batch, and may live on more primes than the outputs: its rows are matched by prime index, a missing prime is
 * HX_ERR_INVALID.  accumulate = 0 overwrites the outputs.  n < 1, a null entry, mismatched shapes and an output that
 * is also an input are HX_ERR_INVALID.  The call is asynchronous on the context's stream.  It uploads a table of
 * operand pointers, so it cannot be recorded: under an open graph capture it returns HX_ERR_UNSUPPORTED before
 * touching the device. */
int hx_mul_add_many(hx_poly* out0, hx_poly* out1, const hx_poly* const* c, const hx_poly* const* in0,
                    const hx_poly* const* in1, int n, int accumulate);
/* The inner loop of unpack (src/intraSlot.cpp:108-115:
 *   unpacked[i] = frob[0];  unpacked[i].multByConstant(C[i]);
 *   for j = 1 .. d-1:  tmp = frob[j];  tmp.multByConstant(C[(i + j) mod d]);  unpacked[i] += tmp;)
 * on the parts of d ciphertexts, in one pass:
 *   out0[i] = sum_(j<d) c[(i + j) mod d] * in0[j],   out1[i] likewise,   0 <= i < nout <= d <= 64,
 * row by row modulo each prime; every word is canonical in [0, q) and equal to what the hx_poly_copy / hx_mul / hx_add
 * sequence leaves (an exact sum modulo q does not depend on the order of its terms).  All operands are in evaluation
 * form.  in0[j], in1[j] and the outputs share one batch and one prime set (same order); in1 and out1 are both null for
 * one-part operands.  c[t] has batch 1 (broadcast over the batch) or that batch, and may live on more primes than the
 * outputs: its rows are matched by prime index, a missing prime is HX_ERR_INVALID.  The outputs are overwritten, not
 * read.  Null arguments, nout < 1, nout > d, d < 1, a poly of another context, mismatched shapes, an output that is also
 * an input or appears twice are HX_ERR_INVALID; d > 64 and an odd phi(m) are HX_ERR_UNSUPPORTED; a refused call touches
 * no output.  Asynchronous on the context's stream.  It uploads a table of operand pointers through the staging ring of
 * hx_mul_add_many, so like that call it cannot be recorded: under an open graph capture it returns HX_ERR_UNSUPPORTED
 * before touching the device.  Per block of OB outputs (OB = 4 for nout <= 4, else 8) it reads the 2 d input rows and
 * d + OB - 1 constant rows once. */
int hx_mul_add_circulant(hx_poly* const* out0, hx_poly* const* out1, int nout, const hx_poly* const* c,
                         const hx_poly* const* in0, const hx_poly* const* in1, int d);
/* dst (batch 1, the prime set of src in the same order) <- batch element b of src: how a batch of encoded diagonals
 * becomes the batch-1 constants above.  Asynchronous on the context's stream; works under a graph capture. */
int hx_poly_extract(hx_poly* dst, const hx_poly* src, int b);
/* The mask split of the linear-array rotate / shift (src/EncryptedArray.cpp:270-274, 334-338:
 *   tmp = ctxt;  tmp.multByConstant(mask);  ctxt -= tmp;)
 * on the parts of one ciphertext, in one pass:  take = keep * mask,  keep = keep - take,  row by row modulo each
 * prime, every word canonical in [0, q) and equal to what hx_poly_copy(take, keep), hx_mul(take, mask),
 * hx_sub(keep, take) leave.  keep1 and take1 are both null for a one-part operand.  take0 / take1 are written, not
 * read; they have the batch and the prime set (same order) of keep0 / keep1.  mask is in evaluation form, with batch 1
 * (broadcast over the batch) or the batch of keep, and may live on more primes than keep: its rows are matched by
 * prime index, a missing prime is HX_ERR_PRIMESET (as hx_mul's).  Null arguments, an output that is also the mask,
 * keep and take (or the two parts) being one poly, a poly of another context and mismatched shapes are
 * HX_ERR_INVALID; an odd phi(m) is HX_ERR_UNSUPPORTED; a refused call touches no output.  Every pointer travels as a
 * kernel argument: the call is asynchronous on the context's stream and may be recorded in a graph capture.
 * HX_NO_MASK_SPLIT=1 runs the three calls per part instead. */
int hx_mask_split(hx_poly* keep0, hx_poly* keep1, hx_poly* take0, hx_poly* take1, const hx_poly* mask);
/* The tail of the non-native rotate1D (src/EncryptedArray.cpp:120-124:
 *   ctxt.multByConstant(m1);  ctxt += T;  T.multByConstant(m1);  ctxt -= T;)
 * on the parts of one ciphertext, in one pass:  c = c * mask + t - t * mask,  row by row modulo each prime, every word
 * canonical in [0, q) and equal to what hx_mul(c, mask), hx_add(c, t), hx_mul(t, mask), hx_sub(c, t) leave in c.  t is
 * read, not written: the four-call form ends with t = t * mask, a value every caller drops.  c1 and t1 are both null
 * for a one-part operand.  t0 / t1 have the batch and the prime set (same order) of c0 / c1; all are in evaluation form
 * (a poly does not record its form: that is the caller's to keep).  mask has batch 1 (broadcast over the batch) or the
 * batch of c, and may live on more primes than c: its rows are matched by prime index, a missing prime is
 * HX_ERR_PRIMESET (as hx_mul's).  Null arguments, c0 / c1 being the mask, c and t (or the two parts) being one poly, a
 * poly of another context and mismatched shapes are HX_ERR_INVALID; an odd phi(m) is HX_ERR_UNSUPPORTED; a refused
 * call touches no operand.  A c that still shares its rows with t (a lazy hx_poly_copy) takes its own copy first, and
 * the result is then c unchanged.  Every pointer travels as a kernel argument: the call is asynchronous on the
 * context's stream and may be recorded in a graph capture.  Per part, in passes over the part, the four calls read 6
 * and write 4 (and read the mask twice); this call reads 2 and writes 1 (and reads the mask once). */
int hx_mask_blend(hx_poly* c0, hx_poly* c1, const hx_poly* t0, const hx_poly* t1, const hx_poly* mask);
/* The mask stage of one layer of a permutation network (src/PermNetwork.cpp:239-242:
 *   tmp = c;  tmp.multByConstant(mask_k);   for each of the layer's K shift amounts)
 * on the parts of one ciphertext, in one pass:  out0[k] = c0 * masks[k],  out1[k] = c1 * masks[k]  for k < nout, row by
 * row modulo each prime, every word canonical in [0, q) and equal to what hx_poly_copy(out, c), hx_mul(out, masks[k])
 * leave.  out1 and c1 are both null for a one-part operand.  The outputs are written, not read; they have the batch and
 * the prime set (same order) of c0 / c1, are distinct polys, and none is c0, c1 or a mask.  An output that still shares
 * c's rows (a lazy hx_poly_copy) lets go of them first; c is left unchanged.  Each mask is in evaluation form, with
 * batch 1 (broadcast over the batch) or the batch of c, and may live on more primes than c, in any order: its rows are
 * matched by prime index, a missing prime is HX_ERR_PRIMESET (as hx_mul's).  Null arguments, nout < 1, aliased
 * outputs, a poly of another context and mismatched shapes are HX_ERR_INVALID; nout > 256 ("too many outputs"), more
 * rows than a launch addresses and an odd phi(m) are HX_ERR_UNSUPPORTED; a refused call touches no output.
 * Asynchronous on the context's stream.  The output and mask addresses travel in a table of nout (2 + rows) words: an
 * eager call uploads it through the staging ring of hx_mul_add_many; a call recorded in a graph capture takes a device
 * table of its own (kept until the context is destroyed) and writes it from kernel arguments, so it waits for nothing
 * and a replay reads no host memory.  Per part, in passes over the part, the K copies and K products read 2 K and
 * write 2 K; this call reads 1 and writes K (the masks are read once either way).  HX_NO_MASK_FAN=1 runs the copy and
 * the product per output and part instead. */
int hx_mask_fan(hx_poly* const* out0, hx_poly* const* out1, int nout, const hx_poly* c0, const hx_poly* c1,
                const hx_poly* const* masks);
/* The inner step of digit extraction (src/extractDigits.cpp:106-107:
 *   tmp -= digits[j];  tmp.divideByP();)
 * on the parts of one ciphertext, in one pass:  c = c * u[row] - t * v[row],  row by row modulo each prime.  After
 * Ctxt::addCtxt's intFactor harmonisation (src/Ctxt.cpp:1474-1536) the subtraction is e1 * tmp - e2 * digit and
 * Ctxt::divideByP (:2415-2435) multiplies by p^-1 mod Q, so the caller passes u = e1 * p^-1 and v = e2 * p^-1 modulo
 * each prime of c0, in the order of its rows.  Every word is canonical in [0, q) and equal to what
 * hx_mul_scalar(c, u), hx_poly_copy(t', t), hx_mul_scalar(t', v), hx_sub(c, t') leave in c.  t is read, not written.
 * c1 and t1 are both null for a one-part operand.  t0 / t1 have the batch and the prime set (same order) of c0 / c1.
 * Null arguments, c and t (or the two parts) being one poly, a poly of another context, mismatched shapes and a scalar
 * that is not below its row's prime are HX_ERR_INVALID; an odd phi(m) is HX_ERR_UNSUPPORTED; a refused call touches no
 * operand.  A c that still shares its rows with t (a lazy hx_poly_copy) takes its own copy first.  Pointers and
 * scalars travel as kernel arguments (one launch per 48 rows): the call is asynchronous on the context's stream and
 * may be recorded in a graph capture.  Per part, in passes over the part, the four calls read 5 and write 4; this call
 * reads 2 and writes 1. */
int hx_scaled_sub(hx_poly* c0, hx_poly* c1, const hx_poly* t0, const hx_poly* t1, const uint64_t* u_per_row,
                  const uint64_t* v_per_row);
/* The leaf of polyEval (src/polyEval.cpp:240-253:
 *   for each baby step  tmp = X^i;  tmp.multByConstant(f_i);  ret += tmp;   then  ret.addConstant(f_0);)
 * on the parts of n ciphertexts, in one pass:  for output row r (prime idx[r] of out0) and every word
 *   out0 = (sum_t w[t][r] * in0[t] + addend[r]) mod q,   out1 = (sum_t w[t][r] * in1[t]) mod q,
 * the sums over the terms t that have a row for that prime.  The powers of X sit on different prime sets: ret += tmp
 * mod-switches one side up (DoubleCRT::addPrimesAndScale, src/DoubleCRT.cpp:603-647: the old rows times the product of
 * the added primes, the new rows zero) and harmonises the intFactors (two products by a scalar), all of it exact
 * arithmetic modulo the row's prime.  The caller folds those integers into w, so a term's rows may be a subset of the
 * output's, in any order of its own, and a term without a row for a prime contributes nothing there; an output row that
 * no term covers is addend[r], or 0.  w is [n][rows(out0)], addend [rows(out0)] or null (zero); every entry is in
 * [0, q) of its row.  in1[t] has the batch and the prime set (same order) of in0[t]; out1 and in1 are both null for
 * one-part operands.  The outputs are overwritten, not read, and must not be among the inputs; every word written is
 * canonical in [0, q).  Null arguments, n < 1, a poly of another context, mismatched batches, an output among the
 * inputs and an entry of w or addend that is not below its row's prime are HX_ERR_INVALID; a term's prime that the
 * output lacks is HX_ERR_PRIMESET; n > 256 (the 128-bit accumulators take 256 products before they must be reduced),
 * more than 160 rows and an odd phi(m) are HX_ERR_UNSUPPORTED; a refused call touches no output.  The call uploads a
 * table of row addresses and weights, so it cannot be recorded: under an open graph capture it returns
 * HX_ERR_UNSUPPORTED before touching the device.  Asynchronous on the context's stream. */
int hx_lin_comb(hx_poly* out0, hx_poly* out1, const hx_poly* const* in0, const hx_poly* const* in1, int n,
                const uint64_t* w, const uint64_t* addend);
/* The loop of innerProduct before its one relinearisation (src/Ctxt.cpp:2885-2891:
 *   result = *v1[0];  result.multLowLvl(*v2[0]);
 *   for i = 1 .. n-1:  tmp = *v1[i];  tmp.multLowLvl(*v2[i]);  result += tmp;)
 * once the operands of every pair sit on one prime set: n x Ctxt::tensorProduct of two canonical ciphertexts
 * (src/Ctxt.cpp:1576-1597) and the part-wise sums of Ctxt::addCtxt (src/Ctxt.cpp:1538-1553), in one pass:
 *   o0 = sum_t a0[t] b0[t],   o1 = sum_t (a0[t] b1[t] + a1[t] b0[t]),   o2 = sum_t a1[t] b1[t],   t < n,
 * row by row modulo each prime.  (a0[t], a1[t]) and (b0[t], b1[t]) are the parts pointing at 1 and at s of the two
 * operands of pair t; o0, o1, o2 receive the parts pointing at 1, s and s^2.  All 4 n operands and the three outputs
 * share one batch and one prime set (same order), in evaluation form, words canonical in [0, q); every word written is
 * canonical and equal to what n x hx_tensor followed by hx_add of the products part by part leave (an exact sum of
 * products modulo q does not depend on the order of its terms).  Operands may repeat: a[t] and b[t] may be one poly (a
 * square) and a poly may appear in several terms.  The outputs are overwritten, not read; one that still shares its
 * rows with a lazy hx_poly_copy lets go of them first.  Null arguments, n < 1, two outputs that are one poly, an
 * output that is also an input, a poly of another context, a batch or prime set that differs from o0's and rows that
 * are not 16-byte aligned are HX_ERR_INVALID; an odd phi(m) is HX_ERR_UNSUPPORTED; a refused call touches no output.
 * Any n: the 128-bit accumulators are reduced every 128 terms (256 products in o1).  The call uploads a table of
 * operand pointers through the staging ring of hx_mul_add_many, so it cannot be recorded: under an open graph capture
 * it returns HX_ERR_UNSUPPORTED before touching the device.  Asynchronous on the context's stream.  In passes over a
 * row, the n tensors and 3 (n - 1) additions read and write 7 n + 9 (n - 1); this call reads 4 n and writes 3. */
int hx_tensor_sum(hx_poly* o0, hx_poly* o1, hx_poly* o2, const hx_poly* const* a0, const hx_poly* const* a1,
                  const hx_poly* const* b0, const hx_poly* const* b1, int n);
/* The last level of computeAllProducts and the weighted sum of tableLookup under one relinearisation
 * (src/tableLookup.cpp:261-267:  *products[ii] = products1[i];  products[ii]->multiplyBy(products2[j]);  ii = j k + i,
 *  and :94-103:  products[i].multByConstant(table[i]);  out += products[i];)
 * once the k + l operands sit on one prime set: relinearisation is linear, so the size tensor products weighted by the
 * table entries are summed first, in one pass:
 *   o0 = sum T[j k + i] a0[i] b0[j],   o1 = sum T[j k + i] (a0[i] b1[j] + a1[i] b0[j]),   o2 = sum T[j k + i] a1[i] b1[j]
 * over i < k, j < l with j k + i < size, row by row modulo each prime.  (a0[i], a1[i]) and (b0[j], b1[j]) are the parts
 * pointing at 1 and at s of products1[i] and products2[j]; o0, o1, o2 receive the parts pointing at 1, s and s^2.  The
 * 2 k + 2 l operands and the three outputs share one batch and one prime set (same order), in evaluation form, words
 * canonical in [0, q).  table is ONE poly whose batch axis is the table index: its batch equals size, entry e is T[e],
 * and every entry serves every batch element of the ciphertexts; it needs a row for every prime of o0 and may have
 * more, in another order.  1 <= k, l <= 256 and 1 <= size <= k l: the row of the grid that holds the last entry may be
 * ragged, and the rows after it hold nothing (their b[j] are checked like the others, and not read).
 * Every word written is canonical and equal to what, per j, one hx_mul_add_many of k terms (W_j = sum_i T[j k + i] a[i],
 * not accumulating) and then one hx_tensor_sum of the pairs (W_j, b[j]) leave: an exact sum of products modulo q does
 * not depend on the order of its terms.  The inner sums take k <= 256 products in 128 bits and one reduction; the outer
 * sums are reduced every 128 values of j (256 products in o1).  Operands may repeat (a[i] and b[j] may be one poly).
 * The outputs are overwritten, not read; one that still shares its rows with a lazy hx_poly_copy lets go of them
 * first.  Null arguments, k or l below 1, a size outside [1, k l], two outputs that are one poly, an output
 * that is also an input or the table, a poly of another context, a batch or prime set that differs from o0's, a table
 * whose batch is not size and rows that are not 16-byte aligned are HX_ERR_INVALID; a prime of o0 that the table lacks
 * is HX_ERR_PRIMESET; k or l above 256 and an odd phi(m) are HX_ERR_UNSUPPORTED; a refused call touches no operand.
 * The call uploads a table of operand pointers through the staging ring of hx_mul_add_many, so it cannot be recorded:
 * under an open graph capture it returns HX_ERR_UNSUPPORTED before touching the device.  Asynchronous on the context's
 * stream.  In passes over a row of one batch element, the l + 1 calls read (2 + 1/4) k l + 4 l and write 2 l + 3; this
 * call reads (1/2 + 1/2) k l + 2 l at batch > 1 and writes 3. */
int hx_table_tensor_sum(hx_poly* o0, hx_poly* o1, hx_poly* o2, const hx_poly* const* a0, const hx_poly* const* a1, int k,
                        const hx_poly* const* b0, const hx_poly* const* b1, int l, const hx_poly* table, int size);
/* The hoisted sum of traceMap (src/matmul.cpp:2878-2887 over BasicAutomorphPrecon, :48-184:
 *   BasicAutomorphPrecon precon(ctxt);  acc = ctxt;  for each t  acc += *precon.automorph(k[t]);)
 * in one pass: the ciphertext plus its images under the n automorphisms k[t], each key-switched by its own matrix W[t]
 * from the digits the ciphertext's s-part was broken into once.  digits: the block of hx_break_into_digits (ndig digits,
 * each on the primes of c0 followed by sp_idx); c0, c1: the parts pointing at 1 and at s, unscaled, on one prime set.
 * Per row, with Psp the product of the special primes modulo the row's prime and sigma_k the gather hx_automorph
 * performs on evaluation rows (out[j] = in[index of Z_m^*[j] k mod m]):
 *   ctxt rows:     out0 = Psp (c0 + sum_t sigma_k[t](c0)) + sum_t sum_j sigma_k[t](dig_j) b[t][j]
 *                  out1 = Psp c1                          + sum_t sum_j sigma_k[t](dig_j) a[t][j]
 *   special rows:  the two double sums alone
 * out0 / out1 end up on the primes of c0 followed by sp_idx, as in hx_relinearize; they are overwritten, not read, and
 * must not be among the inputs.  A W[t] made for a higher level is matched as hx_key_switch_digits matches it: its
 * leading ndig digits, its rows found by prime index.  Every word written is canonical in [0, q) and equals what the
 * loop leaves -- per term a copy and hx_automorph of the digit block and of c0, hx_add_primes_and_scale, a zero part,
 * hx_key_switch_digits and two hx_add -- since all of it is exact arithmetic modulo the row's prime, whatever the order
 * of the terms.  A word of out0 is one 128-bit sum of 1 + n + n ndig products of residues below 2^60, reduced once:
 * n (ndig + 1) + 1 <= 256 (the bound of hx_lin_comb: 256 (2^60 - 2)^2 + 2^60 < 2^128); beyond that, and past 160 rows,
 * HX_ERR_UNSUPPORTED.  Null arguments, n < 1, a k[t] outside Z_m^*, a poly or matrix of another context, mismatched
 * batches or prime sets (c1 against c0, the digit rows against c0's primes and sp_idx, an sp_idx entry that is no prime
 * of the context or already among c0's), an output among the inputs and a W[t] with fewer digits than the block are
 * HX_ERR_INVALID; a prime that a W[t] lacks is HX_ERR_PRIMESET; a refused call touches no output.  The call uploads a
 * table of key-row addresses, so it cannot be recorded: under an open graph capture it returns HX_ERR_UNSUPPORTED
 * before touching the device.  Asynchronous on the context's stream.  Per term the loop makes about 3 ndig + 14 passes
 * over a part in some ten launches; this call reads every digit word and key word once per term and writes the two
 * outputs once, in two launches. */
int hx_hoisted_automorph_sum(const hx_poly* digits, const hx_poly* c0, const hx_poly* c1, const uint64_t* k,
                             const hx_ksk* const* W, int n, const int* sp_idx, int nsp, hx_poly* out0, hx_poly* out1);

/* The hoisted, masked fan-out of replicateAll: an inner node of recursiveReplicateDim (src/replicate.cpp:432-483:
 *   masked = ctxt * M; left = masked + rotate(masked, +e); rest = ctxt - masked; right = rest + rotate(rest, -e))
 * and its leaf (:411-415), with both rotations taken from ONE digit decomposition of ctxt (BasicAutomorphPrecon,
 * src/matmul.cpp:48-184): since sigma_k(ctxt M) = sigma_k(ctxt) sigma_k(M), left = M ctxt + sigma_k+(M) rho^+e(ctxt) and
 * right = (1 - M) ctxt + sigma_k-(1 - M) rho^-e(ctxt).  digits, c0, c1, k, W, sp_idx are as in hx_hoisted_automorph_sum;
 * A[t], B[t] are masks in evaluation form, read at the word's own index (not gathered), of batch 1 (broadcast) or the
 * operands' batch, on any superset of the outputs' primes in any order (rows are matched by prime index); a null A[t] or
 * B[t], or a null array A or B, stands for the constant 1.  For every term t < n, per row, with Psp the product of the
 * special primes modulo the row's prime and sigma_t the gather of hx_automorph by k[t]:
 *   ctxt rows:     out0[t] = A_t (Psp c0) + B_t (Psp sigma_t(c0) + sum_d sigma_t(dig_d) b[t][d])
 *                  out1[t] = A_t (Psp c1) + B_t (                  sum_d sigma_t(dig_d) a[t][d])
 *   special rows:  out0[t] = B_t sum_d sigma_t(dig_d) b[t][d],  out1[t] likewise with a[t][d]
 * The 2 n outputs end up on the primes of c0 followed by sp_idx; they are overwritten, not read, pairwise distinct, and
 * none is an input or a mask; one that still shares rows with another poly (a lazy hx_poly_copy) lets go of them first.
 * Every word written is canonical in [0, q) and equals, word for word, what this sequence of calls leaves per term -- a
 * copy and hx_automorph of the digit block and of c0, hx_add_primes_and_scale, a zero part, hx_key_switch_digits, two
 * hx_mul by B_t, copies of c0 and c1 times A_t, hx_add_primes_and_scale, two hx_add -- since all of it is exact
 * arithmetic modulo the row's prime.  A word is two 128-bit sums: 1 + ndig <= 256 products of residues below 2^60,
 * reduced, then two products, reduced (256 (2^60 - 2)^2 + 2^60 < 2^128).  Null required arguments, n < 1, a k[t]
 * outside Z_m^*, a poly or matrix of another context, mismatched batches or prime sets (as hx_hoisted_automorph_sum
 * refuses them), a mask whose batch is neither 1 nor the operands', aliased outputs, an output among the inputs or
 * masks and a W[t] with fewer digits than the block are HX_ERR_INVALID; a prime that a W[t] or a mask lacks is
 * HX_ERR_PRIMESET; n > 256, more than 160 rows and an odd phi(m) are HX_ERR_UNSUPPORTED; every check comes before
 * anything is touched, so a refused call writes nothing.  The call uploads a table of key-row addresses, so it cannot be
 * recorded: under an open graph capture it returns HX_ERR_UNSUPPORTED before touching the device.  Asynchronous on the
 * context's stream.  Per term the sequence makes about 3 ndig + 24 passes over a part in some fifteen launches; this call
 * reads every digit word and key word once per term, c0 and c1 once for all terms (and c0 once more per term at the
 * gathered index), the masks once, and writes each output once, in two launches. */
int hx_hoisted_mask_fan(const hx_poly* digits, const hx_poly* c0, const hx_poly* c1, const uint64_t* k,
                        const hx_ksk* const* W, const hx_poly* const* A, const hx_poly* const* B, int n,
                        const int* sp_idx, int nsp, hx_poly* const* out0, hx_poly* const* out1);

/* The hoisted blend of MatMulFullExec::rec_mul along a non-native dimension (src/matmul.cpp:2174-2204:
 *   tmp = precon->automorph(i); tmp1 = precon1->automorph(i); tmp = tmp * m1 + tmp1 - tmp1 * m1)
 * over the two digit decompositions (BasicAutomorphPrecon, src/matmul.cpp:48-184) of ctxt = (a0, a1) with the digit block
 * digA and of ctxt1 = ctxt moved by g^(-ord) = (b0, b1) with digB, both as hx_break_into_digits leaves them on the
 * operands' primes followed by sp_idx.  k, W, sp_idx are as in hx_hoisted_automorph_sum; every M[t] is required, a mask in
 * evaluation form read at the word's own index (not gathered), of batch 1 (broadcast) or the operands' batch, on any
 * superset of the outputs' primes in any order (rows are matched by prime index).  For every term t < n, per row, with Psp
 * the product of the special primes modulo the row's prime and sigma_t the gather of hx_automorph by k[t]:
 *   X0 = Psp sigma_t(a0) + sum_d sigma_t(digA_d) b[t][d]      X1 = sum_d sigma_t(digA_d) a[t][d]
 *   Y0 = Psp sigma_t(b0) + sum_d sigma_t(digB_d) b[t][d]      Y1 = sum_d sigma_t(digB_d) a[t][d]
 *   out0[t] = M_t X0 + Y0 - M_t Y0                            out1[t] = M_t X1 + Y1 - M_t Y1
 * the Psp terms on the operands' own rows only.  a1 and b1 are held to the operands' shape and not read: the key switch
 * replaces the s-part.  The 2 n outputs end up on the primes of a0 followed by sp_idx; they are overwritten, not read,
 * pairwise distinct, and none is an input or a mask; one that still shares rows with another poly (a lazy hx_poly_copy)
 * lets go of them first.  Every word written is canonical in [0, q) and equals, word for word, what this sequence of calls
 * leaves per term -- for each operand a copy and hx_automorph of the digit block and of the 1-part,
 * hx_add_primes_and_scale, a zero part and hx_key_switch_digits, then hx_mask_blend -- since all of it is exact arithmetic
 * modulo the row's prime: the kernel blends the gathered operand words first (M x + y - M y, reduced) and multiplies the
 * blended word by the key word, one 128-bit sum of 1 + ndig <= 256 products of residues below 2^60 per output word.
 * Null arguments (a null M[t] included), n < 1, a k[t] outside Z_m^*, a poly or matrix of another context, mismatched
 * batches or prime sets (a1 against a0, the second operand against the first, the digit rows against a0's primes and
 * sp_idx, digit blocks of different length), a mask whose batch is neither 1 nor the operands', aliased outputs, an output
 * among the inputs or masks and a W[t] with fewer digits than the blocks are HX_ERR_INVALID; a prime that a W[t] or a mask
 * lacks is HX_ERR_PRIMESET; n > 256, more than 160 rows and an odd phi(m) are HX_ERR_UNSUPPORTED; every check comes
 * before anything is touched, so a refused call writes nothing.  The call uploads a table of key-row addresses, so it
 * cannot be recorded: under an open graph capture it returns HX_ERR_UNSUPPORTED before touching the device.  Asynchronous
 * on the context's stream.  Per term the sequence makes two full key-switch passes and a blend in some twenty launches;
 * this call reads every digit word of both blocks and every key word once per term, the mask once, and writes each output
 * once, in two launches. */
int hx_hoisted_blend(const hx_poly* digA, const hx_poly* a0, const hx_poly* a1, const hx_poly* digB, const hx_poly* b0,
                     const hx_poly* b1, const uint64_t* k, const hx_ksk* const* W, const hx_poly* const* M, int n,
                     const int* sp_idx, int nsp, hx_poly* const* out0, hx_poly* const* out1);

/* ---------------- HEXL-shim compatibility layer ---------------- */
/* Same signatures and semantics as namespace intel (src/intelExt.h:20-59):
 * host pointers, synchronous, in-place allowed.  FFTFwd / FFTRev1 are what
 * hexl::NTT(n, q).ComputeForward / ComputeInverse are (src/intelExt.cpp:76-98):
 *   - the root is the NTT object's own, MinimalPrimitiveRoot(2n, q), the smallest
 *     primitive 2n-th root of unity (no root crosses this seam);
 *   - FFTFwd returns BIT-REVERSED evaluation order, out[i] = f(psi^(2*brev(i)+1)),
 *     and FFTRev1 reads that order.  The reference's call sites depend on it:
 *     Cmodulus::FFT_aux runs BitReverseCopy after intel::FFTFwd
 *     (src/CModulus.cpp:385, :421-426) and Cmodulus::iFFT before intel::FFTRev1
 *     (:510-514), which makes the stored row the natural one, y[j] = f(psi^(2j+1)),
 *     that DoubleCRT::automorph (src/DoubleCRT.cpp:1160-1202) and the wire format
 *     index.  (hx_ntt_forward / hx_ntt_inverse work on natural rows directly.)
 * One PCIe round trip per call -- provided for link compatibility of a
 * USE_INTEL_HEXL-style build, not for speed. */
int hx_intel_FFTFwd(long* out, const long* in, long n, long q);
int hx_intel_FFTRev1(long* out, const long* in, long n, long q);
int hx_intel_EltwiseAddMod(long* r, const long* a, const long* b, long n, long q);
int hx_intel_EltwiseAddModScalar(long* r, const long* a, long scalar, long n, long q);
int hx_intel_EltwiseSubMod(long* r, const long* a, const long* b, long n, long q);
int hx_intel_EltwiseSubModScalar(long* r, const long* a, long scalar, long n, long q);
int hx_intel_EltwiseMultMod(long* r, const long* a, const long* b, long n, long q);
int hx_intel_EltwiseMultModScalar(long* r, const long* a, long scalar, long n, long q);

/* ---------------- measurement helpers ---------------- */
/* Runs `iters` back-to-back launches of the forward (dir=0) or inverse (dir=1)
 * NTT kernel on the first max_rows rows of p (0 = all rows) between two HIP
 * events recorded on the context's stream and returns the average kernel time
 * in milliseconds (bench.py roofline leg). */
int hx_time_ntt(hx_poly* p, int dir, int iters, int max_rows, float* avg_ms);
/* HIP events on the context's stream: begin records one, end records the second, waits for it
 * and returns the elapsed milliseconds of everything enqueued on the context in between. */
int hx_ctx_timer_begin(hx_ctx* ctx);
int hx_ctx_timer_end(hx_ctx* ctx, float* ms);
/* In-situ kernel timing (the reference's counterpart is its FHE timers printed by printAllTimers,
 * src/timing.cpp:87; here the unit is a device kernel).  Between begin and end every kernel the
 * library launches, on any context of the process, is bracketed by a pair of HIP events recorded on
 * the stream it is launched on, i.e. it is timed where it runs inside the real sequence.
 * hx_profile_end waits for the recorded launches and writes a NUL-terminated JSON summary
 *   {"launches": n, "dropped": d, "kernels": [{"kernel": name, "workgroups": g, "workgroup_size": t,
 *     "calls": k, "total_us": .., "avg_us": .., "min_us": .., "max_us": ..}, ... by total time]}
 * into json[0..cap).  With json == NULL it only reports the size in *needed (the summary is kept
 * for the next call).  Launches recorded into a HIP graph are not timed. */
int hx_profile_begin(void);
int hx_profile_end(char* json, size_t cap, size_t* needed);
/* The device-memory arena behind the context's DoubleCRT slabs (HElib leaves this to malloc through
 * NTL's vec_long, include/helib/DoubleCRT.h:87-95): out[0] = bytes reserved from hipMalloc, out[1] =
 * bytes handed out to polys, out[2] = hipMalloc calls made so far (a warm loop adds none, whatever it
 * keeps alive), out[3] = blocks parked because a live HIP graph may still point at them. */
int hx_ctx_arena_stats(hx_ctx* ctx, uint64_t out[4]);
/* Reserves at least `bytes` of device memory for the context's slabs now (one hipMalloc for what is missing), so
 * that a loop whose footprint is known -- a benchmark's batch, a pipeline's working set -- never reaches hipMalloc
 * while it runs: a multi-GiB hipMalloc takes tens of milliseconds and stalls the stream.  Sized for 288 GB parts:
 * reserve generously. */
int hx_ctx_reserve(hx_ctx* ctx, uint64_t bytes);

/* ---- HIP graphs: the launch-bound case -------------------------------------------------------
 * The reference's benchmark loop runs ONE ciphertext at a time (benchmarks/bgv_basic.cpp:158-164:
 * copy, multiplyBy); on the device that is ~40 kernels of a few microseconds each, bound by launch
 * latency.  hx_ctx_graph_begin starts recording everything enqueued on the context (the calls
 * return as usual but nothing runs), hx_ctx_graph_end closes the recording into a graph, and
 * hx_graph_launch replays it with one launch: the same kernels on the same buffers -- inputs are
 * whatever the input polys hold at launch time, results land in the polys the recorded calls
 * produced (keep them).  Run the sequence once eagerly first (plans, tables and kernel attributes
 * are set up on first use).  Calls that must wait for the device -- uploads, downloads, norm
 * read-backs (use the reference's noise bounds, not measured noise, in a captured sequence) --
 * cannot be recorded and make hx_ctx_graph_end fail.  While a graph is alive the context keeps
 * every buffer it may reference. */
typedef struct hx_graph hx_graph;
int hx_ctx_graph_begin(hx_ctx* ctx);
int hx_ctx_graph_end(hx_ctx* ctx, hx_graph** out);
int hx_graph_launch(hx_graph* g);
int hx_graph_destroy(hx_graph* g);

/* ---------------- the powerful basis (powerful.hip) ----------------
 * For m = m_1 ... m_k with pairwise coprime factors, Z_q[X] / Phi_m is isomorphic to
 * Z_q[X_1..X_k] / (Phi_m1(X_1), ..., Phi_mk(X_k)) by X^i -> prod_j X_j^(i_j), i = sum_j i_j (m / m_j) mod m.  An
 * element of the right-hand side is a cube of phi(m_1) x ... x phi(m_k) = phi(m) words, the last coordinate fastest:
 * PowerfulTranslationIndexes, PowerfulConversion and PowerfulDCRT (src/powerful.cpp:22-190, 199-244, 354-415).  EvalMap
 * consumes and produces it and recryption applies it to every ciphertext part after its raw mod-switch.  Both
 * directions take additions and subtractions only (Phi_n is a quotient of products of binomials), so a modulus is any
 * integer in [2, 2^62).  Calls synchronise the context's stream and fail with HX_ERR_INVALID under an open graph
 * capture. */
typedef struct hx_powerful hx_powerful; /* the tables of one (context, mvec) pair */
/* PowerfulTranslationIndexes(mvec) (src/powerful.cpp:152-190) on the device.  HX_ERR_INVALID with the figures: k not
 * in [1, 8], a factor below 2, factors that are not pairwise coprime, a product that is not the context's m.  Destroy
 * the tables before their context. */
int hx_powerful_create(hx_ctx* ctx, const uint64_t* mvec, int k, hx_powerful** out);
int hx_powerful_destroy(hx_powerful* t);
/* The per-prime step of PowerfulDCRT::dcrtToPowerful (src/powerful.cpp:354-383), in place: every coefficient row of a
 * (as hx_ntt_inverse leaves them: [batch][phi(m)] words below the row's prime) becomes its powerful cube modulo that
 * prime. */
int hx_poly_to_powerful(const hx_powerful* t, hx_poly* a);
/* The inverse (the per-prime step of PowerfulDCRT::powerfulToZZX, :385-415): cube rows back to coefficient rows. */
int hx_powerful_to_poly(const hx_powerful* t, hx_poly* a);
/* PowerfulConversion::polyToPowerful (to_powerful != 0) / powerfulToPoly (src/powerful.cpp:199-244) of host words
 * in[batch][phi(m)] (any int64, reduced into [0, q)) modulo any 2 <= q < 2^62 -> out[batch][phi(m)] in [0, q), by the
 * same kernel on one row. */
int hx_powerful_words(const hx_powerful* t, int to_powerful, uint64_t q, const int64_t* in, int batch, int64_t* out);

/* ---------------- recryption's pre-processing (recrypt.hip, recrypt_core.h) ----------------
 * The step of PubKey::reCrypt (src/recryption.cpp:367-545) between the switch to the recryption key and the product with
 * the encrypted key: Ctxt::rawModSwitch (src/Ctxt.cpp:2949-3049) from Q = prod S, S the part's primes, to q = p^e + 1,
 * then newMakeDivisible (src/recryption.cpp:73-136) and the division by p2ePrime = p^e' (:495-497) -- for one
 * ciphertext part, in one kernel, one thread per coefficient, with no big integers (the mixed-radix lift of
 * hx_poly_rem, and Q^-1 modulo 2^64 for the quotient; helib_amd/csrc/recrypt_core.h has the proof).
 *   in:  the part as coefficient rows, [k][batch][phi(m)] words below each row's prime: hx_ntt_inverse, then
 *        hx_poly_to_powerful.  A poly carries no mark of its form (no entry of this header can tell evaluation rows
 *        from coefficient rows), so this is the caller's to get right, as it is for hx_poly_to_powerful.
 *   out: another poly of the same context and batch on the primes T of the encrypted recryption key (its rows are
 *        overwritten): row t becomes w mod t in [0, t), in the same coefficient order as the input.
 * Per coefficient, as exact integers:
 *   1. c = the centred lift of the residues in [-Q/2, Q/2), as DoubleCRT::toPoly gives it.
 *   2. c q = Q X + Y by floor division; Y > floor(Q/2): Y -= Q, X += 1.
 *   3. delta = (Y mod p2r)(Q^-1 mod p2r) mod p2r >= 0; delta -= p2r if delta > floor(p2r/2), or p2r is even,
 *      delta = p2r/2 and (Y < 0, or Y = 0 and tie bit 0).
 *   4. x = X + delta; x -= q if x > floor(q/2), or q even, x = q/2 and tie bit 1; else x += q if x < -floor(q/2), or
 *      q even, x = -q/2 and tie bit 1.
 *   5. z = x mod p2ePrime in [0, p2ePrime); v = p2ePrime - z if z > floor(p2ePrime/2), or p = 2, z = p2ePrime/2 and tie
 *      bit 2; else v = -z; p2ePrime = 1: v = 0.  w = (x + q v) / p2ePrime, exactly.
 *   6. out row t = w mod t.
 * The reference goes powerful -> polynomial basis after 4 (powerfulToZZX, src/Ctxt.cpp:3041), back for 5
 * (ZZXtoPowerful, src/recryption.cpp:95) and to the polynomial basis again before it divides (:131, :495-497); both maps are integer-linear and inverse to each other on integers this small, and no
 * step looks at a coefficient's position, so the fused chain on the cube gives the cube of the reference's result.
 * Its ties are NTL::RandomBnd(2); here tie bit `which` of coefficient j of batch element b is bit 61 + which of
 * mix(mix(mix(mix(tie_seed) + part) + b) + j), mix the splitmix64 finaliser (recrypt_core.h): reproducible from the
 * seed, balanced.  x_host / v_host (either may be NULL): [batch][phi(m)] signed words, the x of step 4 and the v of
 * step 5, for tests.
 * HX_ERR_INVALID with the figures: gcd(q, p2r) != 1; q != 1 mod p2ePrime; gcd(Q mod q, q) != 1; q >= 2^30 (the
 * reference's e_bnd, src/recryption.cpp:211-217); p2r or p2ePrime not a power of p below 2^30; an output prime below
 * 2^31 (|w| < q is reduced without a division); out = in,
 * another context, another batch; an open graph capture.  HX_ERR_UNSUPPORTED: more than 16 input rows (three
 * ciphertext primes and the special primes are what reCrypt leaves), more than 64 output rows, a batch above 65535.  A refused call
 * touches no output.  Synchronous. */
int hx_recrypt_prep(const hx_poly* in, hx_poly* out, uint64_t q, uint64_t p, uint64_t p2r, uint64_t p2ePrime,
                    uint64_t tie_seed, int part, int64_t* x_host, int64_t* v_host);

#ifdef __cplusplus
}
#endif
#endif /* HELIB_AMD_H */
