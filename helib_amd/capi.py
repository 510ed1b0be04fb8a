"""ctypes binding of the C ABI (include/helib_amd.h) + a thin host-side mirror of
the reference's DoubleCRT interface for this path.

The HIP extension is the only compute path: importing works without a GPU (so
that the symbol table can be checked), but every compute call needs a gfx950
device and raises otherwise.  Nothing here imports oracle/.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# HX_LIB selects an alternative build of the same extension (kernel A/B experiments)
_SO = os.environ.get("HX_LIB") or os.path.join(_HERE, "lib", "libhelib_amd.so")
_lib = None

HX_OK = 0
HX_ERR_INVALID, HX_ERR_DEVICE, HX_ERR_PRIMESET = -1, -2, -3
HX_ERR_NOT_IN_ZMSTAR, HX_ERR_UNSUPPORTED, HX_ERR_NOMEM = -4, -5, -6


class HxError(RuntimeError):
    """helib::RuntimeError / LogicError analogue (include/helib/exceptions.h)."""

    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class InvalidArgument(HxError):
    pass


# every symbol include/helib_amd.h declares (checked by tests without a GPU)
SYMBOLS = [
    "hx_last_error", "hx_version", "hx_device_count",
    "hx_ctx_create", "hx_ctx_destroy", "hx_ctx_phim", "hx_ctx_set_stream", "hx_ctx_sync",
    "hx_ctx_add_prime", "hx_ctx_num_primes", "hx_ctx_prime",
    "hx_poly_create", "hx_poly_create_uninit", "hx_poly_wrap", "hx_poly_destroy", "hx_poly_shape", "hx_poly_primes",
    "hx_poly_device_ptr", "hx_poly_upload", "hx_poly_download", "hx_poly_copy",
    "hx_poly_set_zero", "hx_poly_remove_primes",
    "hx_ntt_forward", "hx_ntt_inverse",
    "hx_add", "hx_sub", "hx_mul", "hx_negate", "hx_add_scalar", "hx_sub_scalar", "hx_mul_scalar",
    "hx_set_scalar", "hx_exp",
    "hx_automorph", "hx_complex_conj",
    "hx_add_primes_and_scale", "hx_add_primes", "hx_poly_rem", "hx_scale_down", "hx_scale_down_multi",
    "hx_bring_to_set_multi", "hx_break_into_digits",
    "hx_ksk_create", "hx_ksk_destroy", "hx_ksk_shape", "hx_ksk_download", "hx_tensor", "hx_key_switch_digits", "hx_mul_relin",
    "hx_relinearize",
    "hx_ctx_defer_norms", "hx_norms_flush",
    "hx_embedding_norm", "hx_scale_down_multi_norms", "hx_bring_to_set_multi_norms",
    "hx_break_into_digits_norms", "hx_relinearize_norms",
    "hx_intel_FFTFwd", "hx_intel_FFTRev1", "hx_intel_EltwiseAddMod", "hx_intel_EltwiseAddModScalar",
    "hx_intel_EltwiseSubMod", "hx_intel_EltwiseSubModScalar", "hx_intel_EltwiseMultMod",
    "hx_intel_EltwiseMultModScalar",
    "hx_time_ntt", "hx_ctx_timer_begin", "hx_ctx_timer_end", "hx_randomize",
    "hx_ctx_graph_begin", "hx_ctx_graph_end", "hx_graph_launch", "hx_graph_destroy",
    "hx_profile_begin", "hx_profile_end", "hx_ctx_arena_stats", "hx_ctx_reserve",
    "hx_tensor_bring_to_set", "hx_tensor_bring_to_set_norms", "hx_mul_relin_norms",
    "hx_ckks_encode", "hx_ckks_embed", "hx_ckks_decode",
    "hx_mul_add_many", "hx_poly_extract", "hx_mask_split", "hx_mask_blend", "hx_scaled_sub",
    "hx_lin_comb", "hx_mul_add_circulant", "hx_hoisted_automorph_sum", "hx_mask_fan", "hx_tensor_sum",
    "hx_table_tensor_sum", "hx_hoisted_mask_fan", "hx_hoisted_blend",
    "hx_bgv_slots_create", "hx_bgv_slots_destroy", "hx_bgv_slots_info", "hx_bgv_encode", "hx_bgv_decode", "hx_bgv_embed",
    "hx_bgv_matrix_create", "hx_bgv_matrix_destroy", "hx_bgv_encode_diagonals",
    "hx_bgv_crt_create", "hx_bgv_crt_destroy", "hx_bgv_crt_info", "hx_bgv_crt_encode", "hx_bgv_crt_decode", "hx_bgv_crt_embed",
    "hx_bgv_crt_create_pr", "hx_bgv_crt_space",
    "hx_bgv_gf_create", "hx_bgv_gf_destroy", "hx_bgv_gf_info", "hx_bgv_gf_encode", "hx_bgv_gf_decode", "hx_bgv_gf_embed",
    "hx_bgv_gf_create_pr", "hx_bgv_gf_space",
    "hx_bgv_gf_linalg_tables", "hx_bgv_gf_matrix_create", "hx_bgv_gf_matrix_destroy", "hx_bgv_gf_matrix_coeffs", "hx_bgv_gf_gather",
    "hx_bgv_gr_linalg_tables", "hx_bgv_gr_matrix_create", "hx_bgv_gf_encode_gathered",
    "hx_bgv_gf_create_gens",
    "hx_powerful_create", "hx_powerful_destroy", "hx_poly_to_powerful", "hx_powerful_to_poly", "hx_powerful_words",
    "hx_recrypt_prep",
]


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so.7 and dlopens it by
    path; if this library (linked against /opt/rocm's copy of the same SONAME) was loaded first, the
    process ends up with two runtimes and the first one loses its devices (hipGetDeviceCount = 0).
    Loading torch's copy first -- without importing torch -- makes both resolve to one runtime
    whatever the import order.  No torch installed: nothing to do."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    """Load the HIP extension; fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise ImportError(
                f"{_SO} is missing: build it with `python -m helib_amd.build` "
                "(there is no CPU fallback)")
        _preload_hip_runtime()
        L = C.CDLL(_SO)
        L.hx_last_error.restype = C.c_char_p
        L.hx_version.restype = C.c_char_p
        L.hx_poly_device_ptr.restype = C.c_void_p
        L.hx_poly_device_ptr.argtypes = [C.c_void_p]
        vp, ip, u64 = C.c_void_p, C.c_int, C.c_uint64
        sig = {
            "hx_device_count": [vp],
            "hx_ctx_create": [vp, ip, u64], "hx_ctx_destroy": [vp], "hx_ctx_phim": [vp, vp],
            "hx_ctx_set_stream": [vp, vp], "hx_ctx_sync": [vp],
            "hx_ctx_add_prime": [vp, u64, u64, vp], "hx_ctx_num_primes": [vp, vp],
            "hx_ctx_prime": [vp, ip, vp, vp],
            "hx_poly_create": [vp, ip, vp, ip, vp], "hx_poly_create_uninit": [vp, ip, vp, ip, vp],
            "hx_poly_wrap": [vp, ip, vp, ip, vp, vp],
            "hx_poly_destroy": [vp], "hx_poly_shape": [vp, vp, vp, vp], "hx_poly_primes": [vp, vp],
            "hx_poly_upload": [vp, vp], "hx_poly_download": [vp, vp], "hx_poly_copy": [vp, vp],
            "hx_poly_set_zero": [vp], "hx_poly_remove_primes": [vp, vp, ip],
            "hx_ntt_forward": [vp], "hx_ntt_inverse": [vp],
            "hx_add": [vp, vp], "hx_sub": [vp, vp], "hx_mul": [vp, vp], "hx_negate": [vp],
            "hx_add_scalar": [vp, vp], "hx_sub_scalar": [vp, vp], "hx_mul_scalar": [vp, vp],
            "hx_set_scalar": [vp, vp], "hx_exp": [vp, u64],
            "hx_automorph": [vp, u64], "hx_complex_conj": [vp],
            "hx_add_primes_and_scale": [vp, vp, ip], "hx_add_primes": [vp, vp, ip],
            "hx_poly_rem": [vp, C.c_uint64, vp],
            "hx_scale_down": [vp, vp, ip, u64],
            "hx_scale_down_multi": [vp, ip, vp, ip, u64],
            "hx_bring_to_set_multi": [vp, ip, vp, ip, vp, ip, u64],
            "hx_break_into_digits": [vp, vp, vp, ip, vp, ip, vp],
            "hx_ksk_create": [vp, ip, vp, ip, vp, vp, vp], "hx_ksk_destroy": [vp],
            "hx_ksk_shape": [vp, vp, vp, vp], "hx_ksk_download": [vp, vp, vp],
            "hx_tensor": [vp] * 7, "hx_key_switch_digits": [vp] * 4,
            "hx_mul_relin": [vp, vp, vp, vp, vp, vp, vp, ip, vp, vp],
            "hx_relinearize": [vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, vp],
            "hx_ctx_defer_norms": [vp, ip], "hx_norms_flush": [vp],
            "hx_embedding_norm": [vp, vp, ip, vp],
            "hx_scale_down_multi_norms": [vp, ip, vp, ip, u64, vp, vp],
            "hx_bring_to_set_multi_norms": [vp, ip, vp, ip, vp, ip, u64, vp],
            "hx_break_into_digits_norms": [vp, vp, vp, ip, vp, ip, vp, vp],
            "hx_relinearize_norms": [vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, vp, vp],
            "hx_intel_FFTFwd": [vp, vp, C.c_long, C.c_long],
            "hx_intel_FFTRev1": [vp, vp, C.c_long, C.c_long],
            "hx_intel_EltwiseAddMod": [vp, vp, vp, C.c_long, C.c_long],
            "hx_intel_EltwiseSubMod": [vp, vp, vp, C.c_long, C.c_long],
            "hx_intel_EltwiseMultMod": [vp, vp, vp, C.c_long, C.c_long],
            "hx_intel_EltwiseAddModScalar": [vp, vp, C.c_long, C.c_long, C.c_long],
            "hx_intel_EltwiseSubModScalar": [vp, vp, C.c_long, C.c_long, C.c_long],
            "hx_intel_EltwiseMultModScalar": [vp, vp, C.c_long, C.c_long, C.c_long],
            "hx_time_ntt": [vp, ip, ip, ip, vp],
            "hx_ctx_timer_begin": [vp], "hx_ctx_timer_end": [vp, vp],
            "hx_randomize": [vp, C.c_char_p, C.c_uint64],
            "hx_ctx_graph_begin": [vp], "hx_ctx_graph_end": [vp, vp], "hx_graph_launch": [vp],
            "hx_graph_destroy": [vp],
            "hx_profile_begin": [], "hx_profile_end": [vp, C.c_size_t, vp],
            "hx_ctx_arena_stats": [vp, vp], "hx_ctx_reserve": [vp, C.c_uint64],
            "hx_mul_relin_norms": [vp, vp, vp, vp, vp, vp, vp, ip, vp, vp, vp],
            "hx_tensor_bring_to_set": [vp] * 8 + [ip, vp, ip, u64],
            "hx_tensor_bring_to_set_norms": [vp] * 8 + [ip, vp, ip, u64, vp],
            "hx_ckks_encode": [vp, vp, ip, ip, C.c_double, vp, vp],
            "hx_ckks_embed": [vp, vp, ip, vp],
            "hx_ckks_decode": [vp, C.c_double, vp],
            "hx_mul_add_many": [vp, vp, vp, vp, vp, ip, ip],
            "hx_poly_extract": [vp, vp, ip],
            "hx_mask_split": [vp, vp, vp, vp, vp],
            "hx_mask_blend": [vp, vp, vp, vp, vp],
            "hx_mask_fan": [vp, vp, C.c_int, vp, vp, vp],
            "hx_scaled_sub": [vp, vp, vp, vp, vp, vp],
            "hx_lin_comb": [vp, vp, vp, vp, ip, vp, vp],
            "hx_tensor_sum": [vp, vp, vp, vp, vp, vp, vp, ip],
            "hx_table_tensor_sum": [vp, vp, vp, vp, vp, ip, vp, vp, ip, vp, ip],
            "hx_mul_add_circulant": [vp, vp, ip, vp, vp, vp, ip],
            "hx_hoisted_automorph_sum": [vp, vp, vp, vp, vp, ip, vp, ip, vp, vp],
            "hx_hoisted_mask_fan": [vp, vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, vp],
            "hx_hoisted_blend": [vp, vp, vp, vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, vp],
            "hx_bgv_slots_create": [vp, u64, vp], "hx_bgv_slots_destroy": [vp],
            "hx_bgv_slots_info": [vp, vp, vp, vp, vp, vp],
            "hx_bgv_encode": [vp, vp, ip, ip, u64, vp, vp],
            "hx_bgv_decode": [vp, vp, u64, vp],
            "hx_bgv_embed": [vp, vp, ip, vp],
            "hx_bgv_matrix_create": [vp, vp, ip, ip, ip, vp], "hx_bgv_matrix_destroy": [vp],
            "hx_bgv_encode_diagonals": [vp, vp, vp, ip, vp, vp, vp],
            "hx_bgv_crt_create": [vp, u64, vp], "hx_bgv_crt_destroy": [vp],
            "hx_bgv_crt_create_pr": [vp, u64, ip, vp], "hx_bgv_crt_space": [vp, vp, vp],
            "hx_bgv_crt_info": [vp, vp, vp, vp, vp, vp, vp, vp],
            "hx_bgv_crt_encode": [vp, vp, ip, u64, vp, vp],
            "hx_bgv_crt_decode": [vp, vp, u64, vp],
            "hx_bgv_crt_embed": [vp, vp, ip, vp],
            "hx_bgv_gf_create": [vp, u64, vp], "hx_bgv_gf_destroy": [vp],
            "hx_bgv_gf_create_pr": [vp, u64, ip, vp], "hx_bgv_gf_space": [vp, vp, vp],
            "hx_bgv_gf_info": [vp, vp, vp, vp, vp, vp, vp, vp, vp],
            "hx_bgv_gf_encode": [vp, vp, ip, u64, vp, vp],
            "hx_bgv_gf_decode": [vp, vp, u64, vp],
            "hx_bgv_gf_embed": [vp, vp, ip, vp],
            "hx_bgv_gf_linalg_tables": [u64, ip, vp, vp, vp, vp],
            "hx_bgv_gf_matrix_create": [vp, vp, ip, ip, ip, vp, vp, vp, vp], "hx_bgv_gf_matrix_destroy": [vp],
            "hx_bgv_gf_matrix_coeffs": [vp, vp],
            "hx_bgv_gf_gather": [vp, vp, ip, vp, ip, vp, vp],
            "hx_bgv_gr_linalg_tables": [u64, ip, ip, vp, vp, vp, vp],
            "hx_bgv_gr_matrix_create": [vp, vp, ip, ip, ip, vp, vp, vp, vp],
            "hx_bgv_gf_encode_gathered": [vp, vp, vp, ip, vp, ip, u64, vp, vp, vp],
            "hx_bgv_gf_create_gens": [vp, u64, ip, vp, vp, ip, vp],
            "hx_powerful_create": [vp, vp, ip, vp], "hx_powerful_destroy": [vp],
            "hx_poly_to_powerful": [vp, vp], "hx_powerful_to_poly": [vp, vp],
            "hx_powerful_words": [vp, ip, u64, vp, ip, vp],
            "hx_recrypt_prep": [vp, vp, u64, u64, u64, u64, u64, ip, vp, vp],
        }
        for name, args in sig.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = C.c_int
        _lib = L
    return _lib


def _chk(rc):
    if rc != HX_OK:
        msg = lib().hx_last_error().decode()
        raise (InvalidArgument if rc == HX_ERR_INVALID else HxError)(rc, msg)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def device_count():
    n = C.c_int(0)
    rc = lib().hx_device_count(C.byref(n))
    return n.value if rc == HX_OK else 0


class Context:
    """Context::moduli + PAlgebra tables resident on one GPU."""

    def __init__(self, m, device=0):
        self.h = C.c_void_p()
        _chk(lib().hx_ctx_create(C.byref(self.h), device, m))
        self.m = m
        n = C.c_uint64()
        _chk(lib().hx_ctx_phim(self.h, C.byref(n)))
        self.phim = int(n.value)
        self.primes, self.roots = [], []

    def close(self):
        if self.h:
            lib().hx_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_prime(self, q, root=0):
        """Cmodulus(zms, q, root) -- returns the index in Context::moduli."""
        idx = C.c_int()
        _chk(lib().hx_ctx_add_prime(self.h, q, root, C.byref(idx)))
        qq, rr = C.c_uint64(), C.c_uint64()
        _chk(lib().hx_ctx_prime(self.h, idx.value, C.byref(qq), C.byref(rr)))
        self.primes.append(int(qq.value))
        self.roots.append(int(rr.value))
        return idx.value

    def ithPrime(self, i):
        return self.primes[i]

    def set_stream(self, stream_ptr):
        _chk(lib().hx_ctx_set_stream(self.h, C.c_void_p(stream_ptr)))

    def timerBegin(self):
        """HIP event on this context's stream (hx_ctx_timer_begin)."""
        _chk(lib().hx_ctx_timer_begin(self.h))

    def timerEnd(self):
        """Milliseconds of device time since timerBegin (waits for the closing event)."""
        ms = C.c_float()
        _chk(lib().hx_ctx_timer_end(self.h, C.byref(ms)))
        return ms.value

    def reserve(self, nbytes):
        """Reserve device memory for this context's slabs up front (hx_ctx_reserve)."""
        _chk(lib().hx_ctx_reserve(self.h, int(nbytes)))

    def arenaStats(self):
        """Device memory behind this context's DoubleCRT slabs (hx_ctx_arena_stats): bytes reserved from
        hipMalloc, bytes in use, number of hipMalloc calls so far, blocks parked for live HIP graphs."""
        v = (C.c_uint64 * 4)()
        _chk(lib().hx_ctx_arena_stats(self.h, v))
        return {"reserved": int(v[0]), "in_use": int(v[1]), "sys_calls": int(v[2]), "deferred": int(v[3])}

    def graphBegin(self):
        """Start recording everything enqueued on this context into a HIP graph (hx_ctx_graph_begin):
        the calls return as usual, nothing runs.  Run the sequence once eagerly first; no uploads,
        downloads or measured-noise read-backs inside."""
        _chk(lib().hx_ctx_graph_begin(self.h))

    def graphEnd(self):
        """Close the recording; returns a Graph whose launch() replays it with one launch."""
        g = C.c_void_p()
        _chk(lib().hx_ctx_graph_end(self.h, C.byref(g)))
        return Graph(self, g)

    def deferNorms(self, on):
        """Deferred read-back of the measured-noise norms (hx_ctx_defer_norms)."""
        if bool(on) != getattr(self, "_defer", False):
            _chk(lib().hx_ctx_defer_norms(self.h, 1 if on else 0))   # switching off flushes
            self._defer = bool(on)
            if not on:
                self._deferred = []

    def keepUntilFlush(self, out):
        """The library writes a deferred norm into the caller's array when the context is next
        flushed: the array must outlive that, whatever becomes of the ciphertext that asked for it
        (a result dropped without reading its noise estimate used to leave a dangling pointer)."""
        if getattr(self, "_defer", False):
            if not hasattr(self, "_deferred"):
                self._deferred = []
            self._deferred.append(out)
            if len(self._deferred) > 256:     # nobody is reading: complete them, keep the list short
                self.flushNorms()
        return out

    def flushNorms(self):
        _chk(lib().hx_norms_flush(self.h))
        self._deferred = []

    def sync(self):
        _chk(lib().hx_ctx_sync(self.h))


class Graph:
    """A captured sequence of engine calls (hx_graph): launch() re-executes the same kernels on the
    same buffers -- the inputs are whatever the input polys hold now, the results land in the polys
    the recorded calls produced."""

    def __init__(self, ctx, handle):
        self.context, self.h = ctx, handle

    def launch(self):
        _chk(lib().hx_graph_launch(self.h))
        return self

    def destroy(self):
        if self.h:
            lib().hx_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class DoubleCRT:
    """Batched DoubleCRT (include/helib/DoubleCRT.h:212-385 for the ops of this path).

    rows are numpy uint64 arrays of shape [nrows, batch, phim] on the host side."""

    def __init__(self, context, index_set, batch=1, data=None, zero=True):
        self.context = context
        idx = _i32(list(index_set))
        self.h = C.c_void_p()
        create = lib().hx_poly_create if (zero and data is None) else lib().hx_poly_create_uninit
        _chk(create(context.h, batch, _p(idx), len(idx), C.byref(self.h)))
        self.batch = batch
        if data is not None:
            self.upload(data)

    @classmethod
    def wrap(cls, context, index_set, batch, device_ptr):
        """hx_poly_wrap: a DoubleCRT over caller-owned device memory ([nrows][batch][phim] u64 at
        device_ptr, e.g. a torch tensor's data_ptr()); the rows never move out of that buffer and
        the caller keeps it alive.  Operations that need more rows than it holds fail."""
        self = cls.__new__(cls)
        self.context, self.batch = context, batch
        idx = _i32(list(index_set))
        self.h = C.c_void_p()
        _chk(lib().hx_poly_wrap(context.h, batch, _p(idx), len(idx), C.c_void_p(int(device_ptr)), C.byref(self.h)))
        return self

    def close(self):
        if self.h:
            lib().hx_poly_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- storage ---
    def getIndexSet(self):
        n = C.c_int()
        _chk(lib().hx_poly_shape(self.h, None, C.byref(n), None))
        out = np.zeros(max(n.value, 1), dtype=np.int32)
        _chk(lib().hx_poly_primes(self.h, _p(out)))
        return [int(x) for x in out[:n.value]]

    def upload(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        nrows = len(self.getIndexSet())
        assert rows.size == nrows * self.batch * self.context.phim, rows.shape
        _chk(lib().hx_poly_upload(self.h, _p(rows)))
        return self

    def download(self):
        nrows = len(self.getIndexSet())
        out = np.zeros((nrows, self.batch, self.context.phim), dtype=np.uint64)
        _chk(lib().hx_poly_download(self.h, _p(out)))
        return out

    def randomize(self, key32, stream):
        """DoubleCRT::randomize (src/DoubleCRT.cpp:1258-1378) on the device: uniform rows by the
        reference's rejection sampling from the ChaCha20 stream (key32, stream) -- hx_randomize."""
        key32 = bytes(key32)
        assert len(key32) == 32
        _chk(lib().hx_randomize(self.h, key32, int(stream)))
        return self

    def copy(self):
        # (a digit block lists its primes once per digit: hx_poly_copy resizes the destination and
        # takes over the source's row list, the destination only has to exist)
        o = DoubleCRT(self.context, list(dict.fromkeys(self.getIndexSet())), self.batch, zero=False)
        _chk(lib().hx_poly_copy(o.h, self.h))
        return o

    def device_ptr(self):
        return lib().hx_poly_device_ptr(self.h)

    # --- transforms (Cmodulus::FFT / iFFT over all rows) ---
    def FFT(self):
        _chk(lib().hx_ntt_forward(self.h))
        return self

    def iFFT(self):
        _chk(lib().hx_ntt_inverse(self.h))
        return self

    # --- ring ops ---
    def __iadd__(self, o):
        _chk(lib().hx_add(self.h, o.h))
        return self

    def __isub__(self, o):
        _chk(lib().hx_sub(self.h, o.h))
        return self

    def __imul__(self, o):
        _chk(lib().hx_mul(self.h, o.h))
        return self

    def Negate(self):
        _chk(lib().hx_negate(self.h))
        return self

    def _scalars(self, num):
        idx = self.getIndexSet()
        if np.isscalar(num) or isinstance(num, int):
            vals = [int(num) % self.context.primes[i] for i in idx]
        else:
            vals = [int(v) for v in num]
        return np.array(vals, dtype=np.uint64)

    def addConstant(self, num):
        s = self._scalars(num)
        _chk(lib().hx_add_scalar(self.h, _p(s)))
        return self

    def subConstant(self, num):
        s = self._scalars(num)
        _chk(lib().hx_sub_scalar(self.h, _p(s)))
        return self

    def mulConstant(self, num):
        s = self._scalars(num)
        _chk(lib().hx_mul_scalar(self.h, _p(s)))
        return self

    def setConstant(self, num):
        """DoubleCRT::operator=(ZZ): every entry becomes num mod q_i."""
        s = self._scalars(num)
        _chk(lib().hx_set_scalar(self.h, _p(s)))
        return self

    def Exp(self, e):
        """DoubleCRT::Exp: entry-wise PowerMod(x, e, q_i) for e >= 0."""
        if e < 0:
            raise ValueError("negative exponent")
        _chk(lib().hx_exp(self.h, int(e)))
        return self

    def automorph(self, k):
        _chk(lib().hx_automorph(self.h, k))
        return self

    def complexConj(self):
        _chk(lib().hx_complex_conj(self.h))
        return self

    # --- prime-set operations ---
    def removePrimes(self, s):
        s = _i32(list(s))
        _chk(lib().hx_poly_remove_primes(self.h, _p(s), len(s)))
        return self

    def addPrimesAndScale(self, s):
        s = _i32(list(s))
        _chk(lib().hx_add_primes_and_scale(self.h, _p(s), len(s)))
        return self

    def addPrimes(self, s):
        s = _i32(list(s))
        _chk(lib().hx_add_primes(self.h, _p(s), len(s)))
        return self

    def toPolyMod(self, t):
        """toPoly + PolyRed(t, abs=true) on the device: [batch, phim] residues in [0,t) of the
        centred coefficients (the tail of SecKey::Decrypt)."""
        out = np.zeros((self.batch, self.context.phim), dtype=np.uint64)
        _chk(lib().hx_poly_rem(self.h, int(t), _p(out)))
        return out

    def scaleDownToSet(self, keep_set, ptxtSpace, norms=False):
        """norms=True: returns embeddingLargestCoeff(delta/diffProd) per batch element instead of
        self (see scaleDownToSetMulti)."""
        if norms:
            return scaleDownToSetMulti([self], keep_set, ptxtSpace, norms=True)[0]
        drop = _i32([i for i in self.getIndexSet() if i not in set(keep_set)])
        _chk(lib().hx_scale_down(self.h, _p(drop), len(drop), ptxtSpace))
        return self

    def breakIntoDigits(self, digits, special, norms=False):
        dig_idx = _i32([p for d in digits for p in d])
        dig_off = _i32(np.concatenate([[0], np.cumsum([len(d) for d in digits])]))
        sp = _i32(list(special))
        out = DoubleCRT(self.context, self.getIndexSet(), self.batch, zero=False)
        if not norms:
            _chk(lib().hx_break_into_digits(self.h, _p(dig_idx), _p(dig_off), len(digits), _p(sp),
                                            len(sp), out.h))
            return out
        nrm = np.zeros((len(digits), self.batch), dtype=np.float64)
        self.context.deferNorms(False)
        _chk(lib().hx_break_into_digits_norms(self.h, _p(dig_idx), _p(dig_off), len(digits), _p(sp),
                                              len(sp), out.h, _p(nrm)))
        return out, nrm


class KeySwitch:
    """KeySwitch matrix W (include/helib/keySwitching.h:86-101) with explicit (b, a)."""

    def __init__(self, context, row_idx, b, a):
        b = np.ascontiguousarray(b, dtype=np.uint64)
        a = np.ascontiguousarray(a, dtype=np.uint64)
        idx = _i32(list(row_idx))
        self.ndig = b.shape[0]
        self.h = C.c_void_p()
        self.context = context
        self.row_idx = [int(i) for i in row_idx]
        _chk(lib().hx_ksk_create(context.h, self.ndig, _p(idx), len(idx), _p(b), _p(a),
                                 C.byref(self.h)))

    def download(self):
        """(b, a) back on the host, [ndig][nrows][phim] (hx_ksk_download)"""
        shape = (self.ndig, len(self.row_idx), self.context.phim)
        b, a = np.empty(shape, dtype=np.uint64), np.empty(shape, dtype=np.uint64)
        _chk(lib().hx_ksk_download(self.h, _p(b), _p(a)))
        return b, a

    def __del__(self):
        try:
            if self.h:
                lib().hx_ksk_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass


def tensorProduct(c0, c1, d0, d1):
    ctx = c0.context
    outs = [DoubleCRT(ctx, c0.getIndexSet(), c0.batch, zero=False) for _ in range(3)]
    _chk(lib().hx_tensor(c0.h, c1.h, d0.h, d1.h, outs[0].h, outs[1].h, outs[2].h))
    return outs


def keySwitchDigits(digits, W, out0, out1):
    """Ctxt::keySwitchDigits: out0 += sum_d digit_d*b_d, out1 += sum_d digit_d*a_d (out0/out1 on the
    ciphertext's primes followed by the special primes; digits as breakIntoDigits returns them)."""
    _chk(lib().hx_key_switch_digits(digits.h, W.h, out0.h, out1.h))


def breakIntoDigits(part, digits, special, norms=False):
    """DoubleCRT::breakIntoDigits as a backend entry point of helib_amd.ctxt (hoisting): the digit
    block (and, norms=True, embeddingLargestCoeff(digit)/P_d per digit and batch element)."""
    return part.breakIntoDigits(digits, special, norms)


def zerosLike(poly):
    return DoubleCRT(poly.context, poly.getIndexSet(), poly.batch)


def multiplyBy(c0, c1, d0, d1, W, digits, out0=None, out1=None):
    """Ctxt::multiplyBy data path at a fixed level (tensorProduct + reLinearize)."""
    ctx = c0.context
    dig_idx = _i32([p for d in digits for p in d])
    dig_off = _i32(np.concatenate([[0], np.cumsum([len(d) for d in digits])]))
    if out0 is None:
        out0 = DoubleCRT(ctx, c0.getIndexSet(), c0.batch, zero=False)
        out1 = DoubleCRT(ctx, c0.getIndexSet(), c0.batch, zero=False)
    _chk(lib().hx_mul_relin(c0.h, c1.h, d0.h, d1.h, W.h, _p(dig_idx), _p(dig_off), len(digits),
                            out0.h, out1.h))
    return out0, out1


def scaleDownToSetMulti(polys, keep_set, ptxtSpace, norms=False, fdelta=False, defer=False):
    """DoubleCRT::scaleDownToSet on several parts that share one prime set, batched into one
    pair of launches where possible.  norms=True additionally returns
    embeddingLargestCoeff(delta/diffProd) per (part, batch element) -- the measured mod-switch
    noise of Ctxt::modDownToSet (src/Ctxt.cpp:466-507) -- as an [nparts, batch] array
    (and the fdelta coefficients [nparts, batch, phi(m)] when fdelta=True)."""
    polys = list(polys)
    keep = set(keep_set)
    drop = _i32([i for i in polys[0].getIndexSet() if i not in keep])
    arr = (C.c_void_p * len(polys))(*[p.h for p in polys])
    if not norms:
        _chk(lib().hx_scale_down_multi(arr, len(polys), _p(drop), len(drop), ptxtSpace))
        return None
    out = np.zeros((len(polys), polys[0].batch), dtype=np.float64)
    fd = np.zeros((len(polys), polys[0].batch, polys[0].context.phim), dtype=np.float64) if fdelta else None
    polys[0].context.deferNorms(defer)   # defer=True: `out` is filled by normsFlush()
    polys[0].context.keepUntilFlush(out)
    _chk(lib().hx_scale_down_multi_norms(arr, len(polys), _p(drop), len(drop), ptxtSpace, _p(out),
                                         _p(fd) if fdelta else None))
    return (out, fd) if fdelta else out


def bringToSetMulti(polys, add_set, keep_set, ptxtSpace, norms=False, defer=False):
    """Ctxt::bringToSet on several parts sharing one prime set: mod-up by add_set, then mod-down
    to keep_set (fused into one pair of launches when a single prime is dropped).
    norms=True: also the measured mod-down noise, as in scaleDownToSetMulti."""
    polys = list(polys)
    add = _i32(list(add_set))
    keep = set(keep_set)
    cur = polys[0].getIndexSet() + [int(i) for i in add]
    drop = _i32([i for i in cur if i not in keep])
    arr = (C.c_void_p * len(polys))(*[p.h for p in polys])
    if not norms:
        _chk(lib().hx_bring_to_set_multi(arr, len(polys), _p(add), len(add), _p(drop), len(drop), ptxtSpace))
        return None
    out = np.zeros((len(polys), polys[0].batch), dtype=np.float64)
    polys[0].context.deferNorms(defer)
    polys[0].context.keepUntilFlush(out)
    _chk(lib().hx_bring_to_set_multi_norms(arr, len(polys), _p(add), len(add), _p(drop), len(drop),
                                           ptxtSpace, _p(out)))
    return out


def normsFlush(poly):
    """Complete every deferred norms read-back of poly's context (waits for the norm kernels
    only)."""
    poly.context.flushNorms()


def supportsNorms(m):
    """Measured (PGFFT-style) noise norms run on the device: power-of-two m (one N/2-point complex
    transform) and general m up to 131072 (complex-double Bluestein)."""
    return m >= 2 and ((m & (m - 1)) == 0 or m <= 131072)


def embeddingLargestCoeff(context, f):
    """embeddingLargestCoeff (src/norms.cpp:480-493) of real polynomials f[rows, phi(m)] on the
    device (m a power of two)."""
    f = np.ascontiguousarray(f, dtype=np.float64).reshape(-1, context.phim)
    out = np.zeros(f.shape[0], dtype=np.float64)
    _chk(lib().hx_embedding_norm(context.h, _p(f), f.shape[0], _p(out)))
    return out


def ckksEncode(context, slots, scaling, idx, coeffs=False):
    """CKKS_embedInSlots (src/norms.cpp:574-615) of slots[B, nslots] (complex, nslots <= m/4) scaled by `scaling`,
    rounded, on the device: a DoubleCRT over the prime indices `idx` in evaluation form (hx_ckks_encode).
    coeffs=True also returns the int64 coefficients [B, phi(m)] (the zzX)."""
    v = np.ascontiguousarray(np.atleast_2d(np.asarray(slots, dtype=np.complex128)))
    B, ns = v.shape
    out = DoubleCRT(context, list(idx), B, zero=False)
    cf = np.zeros((B, context.phim), dtype=np.int64) if coeffs else None
    _chk(lib().hx_ckks_encode(context.h, _p(v), B, ns, float(scaling), out.h, _p(cf) if coeffs else None))
    return (out, cf) if coeffs else out


def ckksEmbed(context, f):
    """CKKS_canonicalEmbedding (src/norms.cpp:495-519) of real polynomials f[B, phi(m)] on the device ->
    complex slots [B, m/4] (hx_ckks_embed)."""
    f = np.ascontiguousarray(np.atleast_2d(np.asarray(f, dtype=np.float64)))
    assert f.shape[1] == context.phim, f.shape
    out = np.zeros((f.shape[0], context.phim // 2), dtype=np.complex128)
    _chk(lib().hx_ckks_embed(context.h, _p(f), f.shape[0], _p(out)))
    return out


def ckksDecode(poly, ln_rat_factor):
    """rawDecrypt's decode (src/EaCx.cpp:62-86): poly = sum_parts part*s^r in evaluation form ->
    canonicalEmbedding(centred CRT value / ratFactor) as complex slots [B, m/4] (hx_ckks_decode)."""
    ctx = poly.context
    out = np.zeros((poly.batch, ctx.phim // 2), dtype=np.complex128)
    _chk(lib().hx_ckks_decode(poly.h, float(ln_rat_factor), _p(out)))
    return out


class BgvSlots:
    """The slot tables of one (Context, p) pair (hx_bgv_slots): EncryptedArray for d = ord_m(p) = 1.  HxError with
    HX_ERR_UNSUPPORTED when p is not 1 mod m."""

    def __init__(self, context, p):
        self.context, self.p = context, int(p)
        self.h = C.c_void_p()
        _chk(lib().hx_bgv_slots_create(context.h, self.p, C.byref(self.h)))
        rho, nd = C.c_uint64(), C.c_int()
        g, o = (C.c_uint64 * 8)(), (C.c_uint64 * 8)()
        _chk(lib().hx_bgv_slots_info(self.h, None, C.byref(rho), C.byref(nd), g, o))
        self.rho = int(rho.value)
        self.gens, self.ords = [int(x) for x in g[:nd.value]], [int(x) for x in o[:nd.value]]

    def close(self):
        if self.h:
            lib().hx_bgv_slots_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _slots_i64(v):
    """int64 [B, n]; python integers of any size are reduced by the caller (EncryptedArray._slots)"""
    return np.ascontiguousarray(np.atleast_2d(np.asarray(v, dtype=np.int64)))


def bgvEncode(table, slots, idx, mul=1, coeffs=False):
    """EncryptedArray::encode of slots[B, nslots] (integers, nslots <= phi(m)) on the device: a DoubleCRT over the
    prime indices `idx` holding balanced(mul * H mod p) in evaluation form (hx_bgv_encode).  coeffs=True also returns
    the int64 coefficients [B, phi(m)] (the zzX)."""
    v = _slots_i64(slots)
    B, ns = v.shape
    ctx = table.context
    out = DoubleCRT(ctx, list(idx), B, zero=False)
    cf = np.zeros((B, ctx.phim), dtype=np.int64) if coeffs else None
    _chk(lib().hx_bgv_encode(table.h, _p(v) if ns else None, B, ns, int(mul) % table.p, out.h, _p(cf) if coeffs else None))
    return (out, cf) if coeffs else out


def bgvDecode(table, poly, factor_inv=1):
    """SecKey::Decrypt's tail for slots: poly = sum_parts part*s^r in evaluation form -> int64 [B, phi(m)] in [0, p)
    (hx_bgv_decode)."""
    out = np.zeros((poly.batch, table.context.phim), dtype=np.int64)
    _chk(lib().hx_bgv_decode(table.h, poly.h, int(factor_inv) % table.p, _p(out)))
    return out


def bgvEmbed(table, f):
    """EncryptedArray::decode of plaintext polynomials f[B, phi(m)] (integers) -> int64 slots [B, phi(m)] in [0, p)
    (hx_bgv_embed)."""
    f = _slots_i64(f)
    assert f.shape[1] == table.context.phim, f.shape
    out = np.zeros_like(f)
    _chk(lib().hx_bgv_embed(table.h, _p(f), f.shape[0], _p(out)))
    return out


class BgvCrt:
    """The CRT tables of one (Context, p, r) triple (hx_bgv_crt): the default EncryptedArray for any d = ord_m(p), slots
    in Z_p or, with r > 1, Hensel-lifted in Z_(p^r) (hx_bgv_crt_create_pr).  d, nslots, gens, ords (signed: a non-native
    dimension's order negated), table_bytes; prime, r; p is the modulus p^r the maps work in."""

    def __init__(self, context, p, r=1):
        self.context, self.prime, self.r = context, int(p), int(r)
        self.h = C.c_void_p()
        if self.r == 1:
            _chk(lib().hx_bgv_crt_create(context.h, self.prime, C.byref(self.h)))
            self.p = self.prime
        else:
            _chk(lib().hx_bgv_crt_create_pr(context.h, self.prime, self.r, C.byref(self.h)))
            rr, mod = C.c_int(), C.c_uint64()
            _chk(lib().hx_bgv_crt_space(self.h, C.byref(rr), C.byref(mod)))
            assert rr.value == self.r and mod.value == self.prime ** self.r
            self.p = int(mod.value)
        d, ns, nd, tb = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
        g, o = (C.c_uint64 * 8)(), (C.c_int64 * 8)()
        _chk(lib().hx_bgv_crt_info(self.h, None, C.byref(d), C.byref(ns), C.byref(nd), g, o, C.byref(tb)))
        self.d, self.nslots, self.table_bytes = int(d.value), int(ns.value), int(tb.value)
        self.gens, self.ords = [int(x) for x in g[:nd.value]], [int(x) for x in o[:nd.value]]

    def close(self):
        if self.h:
            lib().hx_bgv_crt_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bgvCrtEncode(table, slots, idx, mul=1, coeffs=False):
    """EncryptedArray::encode of slots[B, <= nslots] (integers; missing slots are 0) through the CRT tables: a DoubleCRT
    over the prime indices `idx` holding balanced(mul * H mod p) in evaluation form (hx_bgv_crt_encode).  coeffs=True
    also returns the int64 coefficients [B, phi(m)] (the zzX)."""
    v = _slots_i64(slots)
    B, ns = v.shape
    if ns > table.nslots:
        raise InvalidArgument(HX_ERR_INVALID, "more values than slots")
    if ns < table.nslots:
        v = np.ascontiguousarray(np.pad(v, ((0, 0), (0, table.nslots - ns))))
    ctx = table.context
    out = DoubleCRT(ctx, list(idx), B, zero=False)
    cf = np.zeros((B, ctx.phim), dtype=np.int64) if coeffs else None
    _chk(lib().hx_bgv_crt_encode(table.h, _p(v), B, int(mul) % table.p, out.h, _p(cf) if coeffs else None))
    return (out, cf) if coeffs else out


def bgvCrtDecode(table, poly, factor_inv=1):
    """SecKey::Decrypt's tail for slots: poly = sum_parts part*s^r in evaluation form -> int64 [B, nslots] in [0, p)
    (hx_bgv_crt_decode)."""
    out = np.zeros((poly.batch, table.nslots), dtype=np.int64)
    _chk(lib().hx_bgv_crt_decode(table.h, poly.h, int(factor_inv) % table.p, _p(out)))
    return out


def bgvCrtEmbed(table, f):
    """EncryptedArray::decode of plaintext polynomials f[B, phi(m)] (integers) -> int64 slots [B, nslots] in [0, p)
    (hx_bgv_crt_embed)."""
    f = _slots_i64(f)
    assert f.shape[1] == table.context.phim, f.shape
    out = np.zeros((f.shape[0], table.nslots), dtype=np.int64)
    _chk(lib().hx_bgv_crt_embed(table.h, _p(f), f.shape[0], _p(out)))
    return out


class BgvGf:
    """The tables of one (Context, p, r) triple for slots in GF(p^d) = Z_p[X] / G, G = F_0 (hx_bgv_gf): EncryptedArray(context,
    G); with r > 1 slots in the Galois ring Z_(p^r)[X] / G, G the Hensel lift of F_0 (hx_bgv_gf_create_pr).  d, nslots,
    gens, ords (signed), table_bytes, G (d + 1 integers, the constant coefficient first); prime, r; p is the modulus p^r
    the maps work in.  gens / ords: the hypercube follows these generators (hx_bgv_gf_create_gens: the order is
    |ords[i]|, the sign recomputed); None is the library's own choice."""

    def __init__(self, context, p, r=1, gens=None, ords=None):
        self.context, self.prime, self.r = context, int(p), int(r)
        self.h = C.c_void_p()
        if (gens is None) != (ords is None):
            raise InvalidArgument(HX_ERR_INVALID, "gens and ords come together")
        if gens is not None and len(gens) > 0:
            if len(gens) != len(ords):
                raise InvalidArgument(HX_ERR_INVALID, "%d generators with %d orders" % (len(gens), len(ords)))
            g = np.array([int(x) for x in gens], dtype=np.uint64)
            o = np.array([int(x) for x in ords], dtype=np.int64)
            _chk(lib().hx_bgv_gf_create_gens(context.h, self.prime, self.r, _p(g), _p(o), len(g), C.byref(self.h)))
            rr, mod = C.c_int(), C.c_uint64()
            _chk(lib().hx_bgv_gf_space(self.h, C.byref(rr), C.byref(mod)))
            assert rr.value == self.r and mod.value == self.prime ** self.r
            self.p = int(mod.value)
        elif self.r == 1:
            _chk(lib().hx_bgv_gf_create(context.h, self.prime, C.byref(self.h)))
            self.p = self.prime
        else:
            _chk(lib().hx_bgv_gf_create_pr(context.h, self.prime, self.r, C.byref(self.h)))
            rr, mod = C.c_int(), C.c_uint64()
            _chk(lib().hx_bgv_gf_space(self.h, C.byref(rr), C.byref(mod)))
            assert rr.value == self.r and mod.value == self.prime ** self.r
            self.p = int(mod.value)
        d, ns, nd, tb = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
        g, o = (C.c_uint64 * 8)(), (C.c_int64 * 8)()
        _chk(lib().hx_bgv_gf_info(self.h, None, C.byref(d), C.byref(ns), C.byref(nd), g, o, C.byref(tb), None))
        self.d, self.nslots, self.table_bytes = int(d.value), int(ns.value), int(tb.value)
        self.gens, self.ords = [int(x) for x in g[:nd.value]], [int(x) for x in o[:nd.value]]
        G = (C.c_uint64 * (self.d + 1))()
        _chk(lib().hx_bgv_gf_info(self.h, None, None, None, None, None, None, None, G))
        self.G = [int(x) for x in G]

    def close(self):
        if self.h:
            lib().hx_bgv_gf_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _gf_slots(table, slots):
    """int64 [B, nslots, d] from [B, <= nslots] (constants in the slots) or [B, <= nslots, <= d]"""
    v = np.asarray(slots, dtype=np.int64)
    if v.ndim == 1:
        v = v[None, :]
    if v.ndim == 2:
        v = v[:, :, None]
    if v.ndim != 3 or v.shape[1] > table.nslots or v.shape[2] > table.d:
        raise InvalidArgument(HX_ERR_INVALID, "more values than slots, or more coefficients than d")
    out = np.zeros((v.shape[0], table.nslots, table.d), dtype=np.int64)
    out[:, :v.shape[1], :v.shape[2]] = v
    return out


def bgvGfEncode(table, slots, idx, mul=1, coeffs=False):
    """EncryptedArray::encode of GF(p^d) slots (see _gf_slots for the shapes) through the tables: a DoubleCRT over the
    prime indices `idx` holding balanced(mul * H mod p) in evaluation form (hx_bgv_gf_encode).  coeffs=True also returns
    the int64 coefficients [B, phi(m)] (the zzX)."""
    v = _gf_slots(table, slots)
    B = v.shape[0]
    ctx = table.context
    out = DoubleCRT(ctx, list(idx), B, zero=False)
    cf = np.zeros((B, ctx.phim), dtype=np.int64) if coeffs else None
    _chk(lib().hx_bgv_gf_encode(table.h, _p(v), B, int(mul) % table.p, out.h, _p(cf) if coeffs else None))
    return (out, cf) if coeffs else out


def bgvGfDecode(table, poly, factor_inv=1):
    """SecKey::Decrypt's tail for GF(p^d) slots: poly = sum_parts part*s^r in evaluation form -> int64
    [B, nslots, d] in [0, p) (hx_bgv_gf_decode)."""
    out = np.zeros((poly.batch, table.nslots, table.d), dtype=np.int64)
    _chk(lib().hx_bgv_gf_decode(table.h, poly.h, int(factor_inv) % table.p, _p(out)))
    return out


def bgvGfEmbed(table, f):
    """EncryptedArray::decode of plaintext polynomials f[B, phi(m)] (integers) -> int64 slots [B, nslots, d] in [0, p)
    (hx_bgv_gf_embed)."""
    f = _slots_i64(f)
    assert f.shape[1] == table.context.phim, f.shape
    out = np.zeros((f.shape[0], table.nslots, table.d), dtype=np.int64)
    _chk(lib().hx_bgv_gf_embed(table.h, _p(f), f.shape[0], _p(out)))
    return out


def bgvGfLinalgTables(p, d, G):
    """The host tables of linear maps on GF(p^d) slots (hx_bgv_gf_linalg_tables): frob [d, d, d] with frob[e][l] =
    X^(l p^e) mod G, K [d, d, d] with K[j][k] the entries of the inverse of M[i][j] = (X^j)^(p^i), and the flat table
    T [d^2, d^2] of buildLinPolyCoeffs; uint32."""
    return _linalgTables(lib().hx_bgv_gf_linalg_tables, (int(p),), d, G)


def bgvGrLinalgTables(p, r, d, G):
    """bgvGfLinalgTables modulo p^r over the lifted G (hx_bgv_gr_linalg_tables): frob, K and T over Z_(p^r); uint32."""
    return _linalgTables(lib().hx_bgv_gr_linalg_tables, (int(p), int(r)), d, G)


def _linalgTables(entry, ring, d, G):
    d = int(d)
    g = (C.c_uint64 * (d + 1))(*[int(x) for x in G])
    frob, K, T = (np.zeros(max(d, 1) ** e, dtype=np.uint32) for e in (3, 3, 4))
    _chk(entry(*ring, d, g, _p(frob), _p(K), _p(T)))
    return frob.reshape(d, d, d), K.reshape(d, d, d), T.reshape(d * d, d * d)


class BgvGfMatrix:
    """A matrix over GF(p^d) slots on the device (hx_bgv_gf_matrix): GF entries words[nb, D, D, d] or blocks
    words[nb, D, D, d, d] (integers in [0, p)); blk / col [nslots]: the transform and the column every slot reads.  For
    blocks the linearized-polynomial coefficients of every entry are formed on the device at creation.  ring=True builds
    over a table of any r (hx_bgv_gr_matrix_create: words in [0, p^r)); the default refuses r > 1."""

    def __init__(self, table, words, blk, col, ring=False):
        w = np.ascontiguousarray(np.asarray(words), dtype=np.uint32)
        if w.ndim not in (4, 5) or w.shape[1] != w.shape[2] or any(x != table.d for x in w.shape[3:]):
            raise InvalidArgument(HX_ERR_INVALID, "a GF matrix is [nb, D, D, d] or [nb, D, D, d, d]")
        self.table, self.block, self.nb, self.D = table, w.ndim == 5, w.shape[0], w.shape[1]
        blk, col = (np.ascontiguousarray(np.asarray(x), dtype=np.int32) for x in (blk, col))
        if blk.shape != (table.nslots,) or col.shape != (table.nslots,):
            raise InvalidArgument(HX_ERR_INVALID, "blk and col name one transform and one column per slot")
        self.h = C.c_void_p()
        create = lib().hx_bgv_gr_matrix_create if ring else lib().hx_bgv_gf_matrix_create
        _chk(create(table.context.h, table.h, 1 if self.block else 0, self.nb, self.D, _p(w), _p(blk), _p(col), C.byref(self.h)))

    def coeffs(self):
        """the words the gather reads: uint32 [nb, D, D, d, d] (row k = C[k] of the entry) or the entries [nb, D, D, d]"""
        d = self.table.d
        out = np.zeros((self.nb, self.D, self.D) + ((d, d) if self.block else (d,)), dtype=np.uint32)
        _chk(lib().hx_bgv_gf_matrix_coeffs(self.h, _p(out)))
        return out

    def close(self):
        if self.h:
            lib().hx_bgv_gf_matrix_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bgvGfGather(matrix, descs, maps):
    """descs int32 [n, 3] = (diagonal, coefficient index, map), maps int32 [nmaps, nslots, 2] = (source slot or -1,
    Frobenius exponent) -> (int64 slots [n, nslots, d] as bgvGfEncode reads them, bool non-zero flags [n])
    (hx_bgv_gf_gather)."""
    t = matrix.table
    ds = np.ascontiguousarray(descs, dtype=np.int32).reshape(-1, 3)
    mp = np.ascontiguousarray(maps, dtype=np.int32)
    if mp.ndim != 3 or mp.shape[1:] != (t.nslots, 2):
        raise InvalidArgument(HX_ERR_INVALID, "maps is [nmaps, nslots, 2]")
    n = ds.shape[0]
    out = np.zeros((n, t.nslots, t.d), dtype=np.int64)
    nz = np.zeros(max(n, 1), dtype=np.int32)
    _chk(lib().hx_bgv_gf_gather(matrix.h, _p(ds), n, _p(mp), mp.shape[0], _p(out), _p(nz)))
    return out, nz[:n] != 0


def bgvGfEncodeGathered(table, matrix, descs, maps, idx, mul=1, coeffs=False, flags_only=False):
    """bgvGfGather and bgvGfEncode in one call, the constants staying on the device (hx_bgv_gf_encode_gathered): ->
    (DoubleCRT of batch n over `idx`, [coefficients int64 [n, phi(m)],] bool non-zero flags [n]); flags_only=True ->
    the flags alone, no polynomial is made."""
    ds = np.ascontiguousarray(descs, dtype=np.int32).reshape(-1, 3)
    mp = np.ascontiguousarray(maps, dtype=np.int32)
    if mp.ndim != 3 or mp.shape[1:] != (table.nslots, 2):
        raise InvalidArgument(HX_ERR_INVALID, "maps is [nmaps, nslots, 2]")
    n = ds.shape[0]
    nz = np.zeros(max(n, 1), dtype=np.int32)
    ctx = table.context
    if flags_only:
        _chk(lib().hx_bgv_gf_encode_gathered(table.h, matrix.h, _p(ds), n, _p(mp), mp.shape[0], int(mul) % table.p, None, None, _p(nz)))
        return nz[:n] != 0
    out = DoubleCRT(ctx, list(idx), max(n, 1), zero=False)
    cf = np.zeros((n, ctx.phim), dtype=np.int64) if coeffs else None
    _chk(lib().hx_bgv_gf_encode_gathered(table.h, matrix.h, _p(ds), n, _p(mp), mp.shape[0], int(mul) % table.p, out.h,
                                         _p(cf) if coeffs else None, _p(nz)))
    return (out, cf, nz[:n] != 0) if coeffs else (out, nz[:n] != 0)


class BgvMatrix:
    """A plaintext matrix on the device (hx_bgv_matrix): a[phi(m), phi(m)] indexed by slot for dim = -1, a[D, D] indexed
    by the coordinate in dimension dim otherwise (D = ords[dim]).  Any int64; the entries count mod p."""

    def __init__(self, table, a, dim=-1):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.int64))
        if a.ndim != 2:
            raise InvalidArgument(HX_ERR_INVALID, "a matrix has two axes")
        self.table, self.dim, self.shape = table, int(dim), a.shape
        self.h = C.c_void_p()
        _chk(lib().hx_bgv_matrix_create(table.h, _p(a), a.shape[0], a.shape[1], self.dim, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().hx_bgv_matrix_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# hx_bgv_diag: off[8], rot_dim, rot_amt
BGV_DIAG_WORDS = 10


def bgvDiags(diags):
    """[(off, rot_dim, rot_amt)] -> the int32 [n, 10] array of hx_bgv_diag; off is a sequence of at most 8 offsets, one
    per dimension"""
    d = np.zeros((len(diags), BGV_DIAG_WORDS), dtype=np.int32)
    for k, (off, rot_dim, rot_amt) in enumerate(diags):
        d[k, :len(off)] = off
        d[k, 8], d[k, 9] = rot_dim, rot_amt
    return d


def bgvEncodeDiagonals(table, matrix, diags, idx=None, out=None, coeffs=False):
    """The diagonals `diags` ([(off, rot_dim, rot_amt)] or the array of bgvDiags) of a BgvMatrix, encoded on the device
    (hx_bgv_encode_diagonals): -> (DoubleCRT of batch len(diags) over the prime indices idx, int64 coefficients
    [n, phi(m)] or None, bool non-zero flags [n]).  idx = None: the flags alone, (None, None, flags).  out: a DoubleCRT
    to write into instead of a new one."""
    d = np.ascontiguousarray(diags, dtype=np.int32) if isinstance(diags, np.ndarray) else bgvDiags(diags)
    assert d.ndim == 2 and d.shape[1] == BGV_DIAG_WORDS, d.shape
    n, ctx = d.shape[0], table.context
    if out is None and idx is not None:
        out = DoubleCRT(ctx, list(idx), n, zero=False)
    cf = np.zeros((n, ctx.phim), dtype=np.int64) if coeffs else None
    nz = np.zeros(max(n, 1), dtype=np.int32)
    _chk(lib().hx_bgv_encode_diagonals(table.h, matrix.h, _p(d) if n else None, n, out.h if out is not None else None,
                                       _p(cf) if coeffs else None, _p(nz)))
    return out, cf, nz[:n] != 0


def mulAddMany(out0, out1, consts, in0, in1, accumulate=True):
    """out0 (+)= sum_t consts[t] * in0[t], out1 (+)= sum_t consts[t] * in1[t] in one pass (hx_mul_add_many): n x MulAdd
    (src/matmul.cpp:391-408).  out1 / in1 = None for a one-part ciphertext."""
    n = len(consts)
    assert len(in0) == n and (in1 is None or len(in1) == n)

    def arr(ps):
        return (C.c_void_p * max(n, 1))(*[p.h for p in ps])
    _chk(lib().hx_mul_add_many(out0.h, out1.h if out1 is not None else None, arr(consts), arr(in0),
                               arr(in1) if in1 is not None else None, n, 1 if accumulate else 0))


def mulAddCirculant(out0, out1, consts, in0, in1):
    """out0[i] = sum_j consts[(i + j) mod d] * in0[j], out1[i] likewise, for i < len(out0) <= d = len(consts) <= 64, in one
    pass (hx_mul_add_circulant): the inner loop of unpack (src/intraSlot.cpp:108-115).  out1 / in1 = None for one-part
    operands; the outputs are overwritten (make them with likeUninit) and must not be among the inputs."""
    d, nout = len(consts), len(out0)
    if len(in0) != d or (in1 is not None and len(in1) != d) or (out1 is None) != (in1 is None) or \
            (out1 is not None and len(out1) != nout):
        raise InvalidArgument(HX_ERR_INVALID, "mulAddCirculant: d constants, d inputs per part and as many outputs per part")

    def arr(ps):
        return (C.c_void_p * max(len(ps), 1))(*[p.h for p in ps])
    _chk(lib().hx_mul_add_circulant(arr(out0), arr(out1) if out1 is not None else None, nout, arr(consts), arr(in0),
                                    arr(in1) if in1 is not None else None, d))


def maskSplit(keep0, keep1, take0, take1, mask):
    """take = keep * mask, keep -= take on the one or two parts of a ciphertext in one pass (hx_mask_split): tmp = ctxt;
    tmp.multByConstant(mask); ctxt -= tmp (src/EncryptedArray.cpp:270-274).  keep1 / take1 = None for a one-part
    ciphertext; take* are overwritten (make them with likeUninit).  In a context created under HX_NO_MASK_SPLIT=1 the
    call issues hx_poly_copy, hx_mul and hx_sub per part instead; the words are the same."""
    if (keep1 is None) != (take1 is None):
        raise InvalidArgument(HX_ERR_INVALID, "keep1 and take1 go together (both None for a one-part ciphertext)")
    _chk(lib().hx_mask_split(keep0.h, keep1.h if keep1 is not None else None, take0.h,
                             take1.h if take1 is not None else None, mask.h))


def maskBlend(c0, c1, t0, t1, mask):
    """c = c * mask + t - t * mask on the one or two parts of a ciphertext in one pass (hx_mask_blend): the tail of the
    non-native rotate1D, ctxt.multByConstant(m1); ctxt += T; T.multByConstant(m1); ctxt -= T
    (src/EncryptedArray.cpp:120-124).  c1 / t1 = None for a one-part ciphertext; t* are read only."""
    if (c1 is None) != (t1 is None):
        raise InvalidArgument(HX_ERR_INVALID, "c1 and t1 go together (both None for a one-part ciphertext)")
    _chk(lib().hx_mask_blend(c0.h, c1.h if c1 is not None else None, t0.h, t1.h if t1 is not None else None, mask.h))


def maskFan(out0, out1, c0, c1, masks):
    """out0[k] = c0 * masks[k], out1[k] = c1 * masks[k] for k < len(masks) in one pass (hx_mask_fan): the mask stage of a
    permutation-network layer, tmp = c; tmp.multByConstant(mask_k) per shift amount (src/PermNetwork.cpp:239-242).
    out1 / c1 = None for a one-part operand; the outputs are overwritten (lazy copies of c, or likeUninit) and c is left
    as it is.  In a context created under HX_NO_MASK_FAN=1 the call issues hx_poly_copy and hx_mul per output and part
    instead; the words are the same."""
    nout = len(masks)
    if (out1 is None) != (c1 is None) or len(out0) != nout or (out1 is not None and len(out1) != nout):
        raise InvalidArgument(HX_ERR_INVALID, "maskFan: out1 and c1 go together, and one output per part for every mask")

    def arr(ps):
        return (C.c_void_p * max(len(ps), 1))(*[p.h for p in ps])
    _chk(lib().hx_mask_fan(arr(out0), arr(out1) if out1 is not None else None, nout, c0.h,
                           c1.h if c1 is not None else None, arr(masks)))


def scaledSub(c0, c1, t0, t1, u, v):
    """c = c * u[row] - t * v[row] on the one or two parts of a ciphertext in one pass (hx_scaled_sub): tmp -= digit;
    tmp.divideByP() (src/extractDigits.cpp:106-107) with u = e1 / p and v = e2 / p modulo each prime of c0, in the order
    of its rows (integers in [0, q)).  c1 / t1 = None for a one-part ciphertext; t* are read only."""
    if (c1 is None) != (t1 is None):
        raise InvalidArgument(HX_ERR_INVALID, "c1 and t1 go together (both None for a one-part ciphertext)")
    u = np.array([int(x) for x in u], dtype=np.uint64)
    v = np.array([int(x) for x in v], dtype=np.uint64)
    n = len(c0.getIndexSet())
    if len(u) != n or len(v) != n:
        raise InvalidArgument(HX_ERR_INVALID, "scaledSub takes one u and one v per prime row of c0")
    if n == 0:
        return
    _chk(lib().hx_scaled_sub(c0.h, c1.h if c1 is not None else None, t0.h, t1.h if t1 is not None else None, _p(u), _p(v)))


def linComb(in0, in1, idx, w, addend=None):
    """out = sum_t w[t][row] * in[t] + addend[row] on the one or two parts of n ciphertexts in one pass (hx_lin_comb):
    the loop of simplePolyEval (src/polyEval.cpp:240-253) with the integers of multByConstant, the mod-ups and the
    intFactor pairs folded into w.  in0 / in1: the n parts pointing at 1 and at s (in1 = None for one-part operands),
    each term on a subset of idx in its own order; idx: the prime indices of the output rows; w: n lists of one integer
    in [0, q) per output row; addend: one integer in [0, q) per output row, added to the first part, or None.
    -> (out0, out1), new DoubleCRTs (out1 = None with in1)."""
    if in0 is None or w is None or idx is None:
        raise InvalidArgument(HX_ERR_INVALID, "linComb: in0, idx and w are required")
    n, idx = len(in0), [int(i) for i in idx]
    if n < 1:
        raise InvalidArgument(HX_ERR_INVALID, "linComb needs at least one term")
    if in1 is not None and len(in1) != n:
        raise InvalidArgument(HX_ERR_INVALID, "linComb: in0 and in1 go together, term by term")
    if len(w) != n or any(len(row) != len(idx) for row in w) or (addend is not None and len(addend) != len(idx)):
        raise InvalidArgument(HX_ERR_INVALID, "linComb takes one weight per term and output row, and one addend per output row")
    wa = np.array([[int(x) for x in row] for row in w], dtype=np.uint64).reshape(n, len(idx))
    aa = np.array([int(x) for x in addend], dtype=np.uint64) if addend is not None else None
    ctx, batch = in0[0].context, in0[0].batch
    out0 = DoubleCRT(ctx, idx, batch, zero=False)
    out1 = DoubleCRT(ctx, idx, batch, zero=False) if in1 is not None else None

    def arr(ps):
        return (C.c_void_p * n)(*[p.h for p in ps])
    _chk(lib().hx_lin_comb(out0.h, out1.h if out1 is not None else None, arr(in0), arr(in1) if in1 is not None else None,
                           n, _p(wa), _p(aa) if aa is not None else None))
    return out0, out1


def tensorSum(a0, a1, b0, b1):
    """o0 = sum_t a0[t] b0[t], o1 = sum_t (a0[t] b1[t] + a1[t] b0[t]), o2 = sum_t a1[t] b1[t] in one pass
    (hx_tensor_sum): the tensor products of n pairs of canonical ciphertexts and their part-wise sums, the loop of
    innerProduct before its relinearisation (src/Ctxt.cpp:2885-2891).  a0 / a1 and b0 / b1: the parts pointing at 1 and
    at s of the two operands of every pair, all on one prime set and batch; operands may repeat.
    -> (o0, o1, o2), new DoubleCRTs on that prime set."""
    if a0 is None or a1 is None or b0 is None or b1 is None:
        raise InvalidArgument(HX_ERR_INVALID, "tensorSum: a0, a1, b0 and b1 are required")
    n = len(a0)
    if n < 1:
        raise InvalidArgument(HX_ERR_INVALID, "tensorSum needs at least one term")
    if len(a1) != n or len(b0) != n or len(b1) != n:
        raise InvalidArgument(HX_ERR_INVALID, "tensorSum: a0, a1, b0 and b1 go together, term by term")
    outs = [likeUninit(a0[0]) for _ in range(3)]

    def arr(ps):
        return (C.c_void_p * n)(*[p.h for p in ps])
    _chk(lib().hx_tensor_sum(outs[0].h, outs[1].h, outs[2].h, arr(a0), arr(a1), arr(b0), arr(b1), n))
    return tuple(outs)


def tableTensorSum(a0, a1, b0, b1, table, size=None):
    """o0 = sum T[j k + i] a0[i] b0[j], o1 = sum T[j k + i] (a0[i] b1[j] + a1[i] b0[j]), o2 = sum T[j k + i] a1[i] b1[j]
    over i < k = len(a0), j < l = len(b0), j k + i < size, in one pass (hx_table_tensor_sum): the last level of
    computeAllProducts and the weighted sum of tableLookup before ONE relinearisation (src/tableLookup.cpp:94-103,
    261-267).  a0 / a1 and b0 / b1: the parts pointing at 1 and at s of products1 and products2, all on one prime set and
    batch; table: one DoubleCRT whose batch axis is the table index (batch = size, default: the table's batch), with a row
    for every prime of a0[0].  -> (o0, o1, o2), new DoubleCRTs on the operands' prime set."""
    if a0 is None or a1 is None or b0 is None or b1 is None or table is None:
        raise InvalidArgument(HX_ERR_INVALID, "tableTensorSum: a0, a1, b0, b1 and the table are required")
    k, l = len(a0), len(b0)
    if k < 1 or l < 1:
        raise InvalidArgument(HX_ERR_INVALID, "tableTensorSum needs at least one a and one b")
    if len(a1) != k or len(b1) != l:
        raise InvalidArgument(HX_ERR_INVALID, "tableTensorSum: a0 and a1, and b0 and b1, go together entry by entry")
    size = table.batch if size is None else int(size)
    outs = [likeUninit(a0[0]) for _ in range(3)]

    def arr(ps):
        return (C.c_void_p * len(ps))(*[p.h for p in ps])
    _chk(lib().hx_table_tensor_sum(outs[0].h, outs[1].h, outs[2].h, arr(a0), arr(a1), k, arr(b0), arr(b1), l, table.h, size))
    return tuple(outs)


def hoistedAutomorphSum(digits, c0, c1, ks, Ws, special):
    """The ciphertext (c0, c1) plus its images under the automorphisms ks, each key-switched by its own matrix of Ws
    from the digit block of c1 (breakIntoDigits over `special`), in one pass (hx_hoisted_automorph_sum): the loop acc +=
    BasicAutomorphPrecon.automorph(k) of traceMap (src/matmul.cpp:2878-2887).  -> (out0, out1), new DoubleCRTs on the
    primes of c0 followed by special."""
    if digits is None or c0 is None or c1 is None or ks is None or Ws is None:
        raise InvalidArgument(HX_ERR_INVALID, "hoistedAutomorphSum: digits, c0, c1, ks and Ws are required")
    n = len(ks)
    if n < 1 or len(Ws) != n:
        raise InvalidArgument(HX_ERR_INVALID, "hoistedAutomorphSum takes at least one automorphism, and one matrix for each")
    ka = np.array([int(k) for k in ks], dtype=np.uint64)
    sp = _i32(list(special))
    idx = c0.getIndexSet() + [int(i) for i in sp]
    out0 = DoubleCRT(c0.context, idx, c0.batch, zero=False)
    out1 = DoubleCRT(c0.context, idx, c0.batch, zero=False)
    wa = (C.c_void_p * n)(*[W.h for W in Ws])
    _chk(lib().hx_hoisted_automorph_sum(digits.h, c0.h, c1.h, _p(ka), wa, n, _p(sp), len(sp), out0.h, out1.h))
    return out0, out1


hoistedSum = hoistedAutomorphSum    # the name helib_amd.ctxt looks for on a backend's ops


def hoistedMaskFan(digits, c0, c1, ks, Ws, A, B, special):
    """For every t: A[t] * (c0, c1) + B[t] * (the image of (c0, c1) under the automorphism ks[t], key-switched by Ws[t]
    from the digit block of c1), in one pass (hx_hoisted_mask_fan): an inner node of replicateAll's recursion
    (src/replicate.cpp:432-483) over one BasicAutomorphPrecon.  A, B: lists of DoubleCRT masks in evaluation form (batch 1
    or the operands'), None in a position -- or None for a whole list -- standing for the constant 1.
    -> (list of out0, list of out1), new DoubleCRTs on the primes of c0 followed by special."""
    if digits is None or c0 is None or c1 is None or ks is None or Ws is None:
        raise InvalidArgument(HX_ERR_INVALID, "hoistedMaskFan: digits, c0, c1, ks and Ws are required")
    n = len(ks)
    if n < 1 or len(Ws) != n:
        raise InvalidArgument(HX_ERR_INVALID, "hoistedMaskFan takes at least one automorphism, and one matrix for each")
    if (A is not None and len(A) != n) or (B is not None and len(B) != n):
        raise InvalidArgument(HX_ERR_INVALID, "hoistedMaskFan: A and B hold one mask (or None) per automorphism")
    ka = np.array([int(k) for k in ks], dtype=np.uint64)
    sp = _i32(list(special))
    idx = c0.getIndexSet() + [int(i) for i in sp]
    out0 = [DoubleCRT(c0.context, idx, c0.batch, zero=False) for _ in range(n)]
    out1 = [DoubleCRT(c0.context, idx, c0.batch, zero=False) for _ in range(n)]

    def arr(ps):
        return (C.c_void_p * n)(*[p.h if p is not None else None for p in ps]) if ps is not None else None
    _chk(lib().hx_hoisted_mask_fan(digits.h, c0.h, c1.h, _p(ka), arr(Ws), arr(A), arr(B), n, _p(sp), len(sp), arr(out0),
                                   arr(out1)))
    return out0, out1


def hoistedBlend(digA, a0, a1, digB, b0, b1, ks, Ws, masks, special):
    """For every t: M * X + Y - M * Y with X the image of (a0, a1) and Y the image of (b0, b1) under the automorphism
    ks[t], each key-switched by Ws[t] from its own digit block (digA of a1, digB of b1), M = masks[t], in one pass
    (hx_hoisted_blend): the inner step of MatMulFullExec::rec_mul along a non-native dimension (src/matmul.cpp:2174-2204)
    over two BasicAutomorphPrecon.  masks: one DoubleCRT in evaluation form per automorphism (batch 1 or the operands').
    -> (list of out0, list of out1), new DoubleCRTs on the primes of a0 followed by special."""
    if any(x is None for x in (digA, a0, a1, digB, b0, b1, ks, Ws, masks)):
        raise InvalidArgument(HX_ERR_INVALID, "hoistedBlend: both digit blocks, both part pairs, ks, Ws and masks are required")
    n = len(ks)
    if n < 1 or len(Ws) != n:
        raise InvalidArgument(HX_ERR_INVALID, "hoistedBlend takes at least one automorphism, and one matrix for each")
    if len(masks) != n or any(mk is None for mk in masks):
        raise InvalidArgument(HX_ERR_INVALID, "hoistedBlend: masks holds one mask per automorphism")
    ka = np.array([int(k) for k in ks], dtype=np.uint64)
    sp = _i32(list(special))
    idx = a0.getIndexSet() + [int(i) for i in sp]
    out0 = [DoubleCRT(a0.context, idx, a0.batch, zero=False) for _ in range(n)]
    out1 = [DoubleCRT(a0.context, idx, a0.batch, zero=False) for _ in range(n)]

    def arr(ps):
        return (C.c_void_p * n)(*[p.h for p in ps])
    _chk(lib().hx_hoisted_blend(digA.h, a0.h, a1.h, digB.h, b0.h, b1.h, _p(ka), arr(Ws), arr(masks), n, _p(sp), len(sp),
                                arr(out0), arr(out1)))
    return out0, out1


def constantLike(poly, idx, num):
    """DoubleCRT(num, context, primeSet): the constant polynomial num on the prime indices idx, with poly's batch"""
    return DoubleCRT(poly.context, list(idx), poly.batch, zero=False).setConstant(num)


def likeUninit(poly):
    """a DoubleCRT with poly's batch and prime set whose rows are about to be overwritten"""
    return DoubleCRT(poly.context, poly.getIndexSet(), poly.batch, zero=False)


def splitBatch(poly):
    """the batch elements of poly as batch-1 DoubleCRTs (hx_poly_extract)"""
    if poly.batch == 1:
        return [poly]
    idx, out = poly.getIndexSet(), []
    for b in range(poly.batch):
        d = DoubleCRT(poly.context, idx, 1, zero=False)
        _chk(lib().hx_poly_extract(d.h, poly.h, b))
        out.append(d)
    return out


def reLinearize(t0, t1, t2, W, digits, special, out0=None, out1=None, norms=False, defer=False):
    """Ctxt::reLinearize data path for a 3-part ciphertext (1, s, s^2), or with t1 = None for the
    (1, s(X^k)) ciphertext of Ctxt::smartAutomorph (t2 = the s(X^k) part).  norms=True also returns
    the [ndigits, batch] array embeddingLargestCoeff(digit)/P_digit (the pieces of
    breakIntoDigits' return value, src/DoubleCRT.cpp:538-545)."""
    ctx = t0.context
    dig_idx = _i32([p for d in digits for p in d])
    dig_off = _i32(np.concatenate([[0], np.cumsum([len(d) for d in digits])]))
    sp = _i32(list(special))
    if out0 is None:
        out0 = DoubleCRT(ctx, t0.getIndexSet(), t0.batch, zero=False)
        out1 = DoubleCRT(ctx, t0.getIndexSet(), t0.batch, zero=False)
    if not norms:
        _chk(lib().hx_relinearize(t0.h, t1.h if t1 is not None else None, t2.h, W.h, _p(dig_idx),
                                  _p(dig_off), len(digits), _p(sp), len(sp), out0.h, out1.h))
        return out0, out1
    nrm = np.zeros((len(digits), t0.batch), dtype=np.float64)
    ctx.deferNorms(defer)
    ctx.keepUntilFlush(nrm)
    _chk(lib().hx_relinearize_norms(t0.h, t1.h if t1 is not None else None, t2.h, W.h, _p(dig_idx),
                                    _p(dig_off), len(digits), _p(sp), len(sp), out0.h, out1.h, _p(nrm)))
    return out0, out1, nrm


def time_ntt(poly, inverse, iters, max_rows=0):
    ms = C.c_float()
    _chk(lib().hx_time_ntt(poly.h, 1 if inverse else 0, iters, max_rows, C.byref(ms)))
    return ms.value


def profileBegin():
    """Start timing every kernel the library launches with HIP events on its own stream (hx_profile_begin)."""
    _chk(lib().hx_profile_begin())


def profileEnd():
    """Wait for the launches recorded since profileBegin and return the per-kernel summary
    (hx_profile_end): {"launches", "dropped", "kernels": [{"kernel", "workgroups", "workgroup_size",
    "calls", "total_us", "avg_us", "min_us", "max_us"}, ...]} ordered by total time."""
    import json
    need = C.c_size_t()
    _chk(lib().hx_profile_end(None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value)
    _chk(lib().hx_profile_end(buf, need.value, None))
    return json.loads(buf.value.decode())


def tensorBringToSet(c0, c1, d0, d1, add_set, keep_set, ptxtSpace, norms=False, defer=False):
    """Ctxt::tensorProduct followed by Ctxt::bringToSet of the three product parts (hx_tensor_bring_to_set): the
    parts (1), (s), (s^2) on `keep_set` (= the operands' primes + add_set - what is dropped).  norms: also the
    embeddingLargestCoeff of the mod-switch deltas, [3][batch] (deferred read-back as in bringToSetMulti)."""
    ctx = c0.context
    cur = c0.getIndexSet()
    add = [i for i in add_set if i not in cur]
    drop = [i for i in cur + add if i not in set(keep_set)]
    outs = [DoubleCRT(ctx, cur, c0.batch, zero=False) for _ in range(3)]
    a, d = _i32(add), _i32(drop)
    if not norms:
        _chk(lib().hx_tensor_bring_to_set(c0.h, c1.h, d0.h, d1.h, outs[0].h, outs[1].h, outs[2].h, _p(a), len(add),
                                          _p(d), len(drop), int(ptxtSpace)))
        return outs
    nrm = np.zeros((3, c0.batch), dtype=np.float64)
    ctx.deferNorms(defer)
    ctx.keepUntilFlush(nrm)
    _chk(lib().hx_tensor_bring_to_set_norms(c0.h, c1.h, d0.h, d1.h, outs[0].h, outs[1].h, outs[2].h, _p(a), len(add),
                                            _p(d), len(drop), int(ptxtSpace), _p(nrm)))
    return outs, nrm


def mulRelin(c0, c1, d0, d1, W, digits, norms=False, defer=False):
    """Ctxt::tensorProduct + Ctxt::reLinearize at the full level of the matrix W with the product parts formed inside
    the key-switch kernels (hx_mul_relin[_norms]); the operands' primes must be W's leading rows.  norms=True also
    returns the [ndigits, batch] array of reLinearize (embeddingLargestCoeff(digit) / P_digit)."""
    ctx = c0.context
    dig_idx = _i32([p for d in digits for p in d])
    dig_off = _i32(np.concatenate([[0], np.cumsum([len(d) for d in digits])]))
    out0 = DoubleCRT(ctx, c0.getIndexSet(), c0.batch, zero=False)
    out1 = DoubleCRT(ctx, c0.getIndexSet(), c0.batch, zero=False)
    if not norms:
        _chk(lib().hx_mul_relin(c0.h, c1.h, d0.h, d1.h, W.h, _p(dig_idx), _p(dig_off), len(digits), out0.h, out1.h))
        return out0, out1
    nrm = np.zeros((len(digits), c0.batch), dtype=np.float64)
    ctx.deferNorms(defer)
    ctx.keepUntilFlush(nrm)
    _chk(lib().hx_mul_relin_norms(c0.h, c1.h, d0.h, d1.h, W.h, _p(dig_idx), _p(dig_off), len(digits), out0.h, out1.h,
                                  _p(nrm)))
    return out0, out1, nrm


class Powerful:
    """The powerful-basis tables of one (Context, mvec) pair (hx_powerful): m = prod mvec with pairwise coprime factors;
    Z_q[X] / Phi_m <-> the cube phi(m_1) x ... x phi(m_k), the last coordinate fastest (src/powerful.cpp:152-244)."""

    def __init__(self, context, mvec):
        self.context, self.mvec = context, [int(x) for x in mvec]
        self.h = C.c_void_p()
        mv = np.array(self.mvec, dtype=np.uint64)
        _chk(lib().hx_powerful_create(context.h, _p(mv), len(mv), C.byref(self.h)))

    def close(self):
        if self.h:
            lib().hx_powerful_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def polyToPowerful(table, poly):
    """every coefficient row of the DoubleCRT (after iFFT) -> its powerful cube modulo the row's prime, in place
    (hx_poly_to_powerful)"""
    _chk(lib().hx_poly_to_powerful(table.h, poly.h))
    return poly


def powerfulToPoly(table, poly):
    """the inverse of polyToPowerful, in place (hx_powerful_to_poly)"""
    _chk(lib().hx_powerful_to_poly(table.h, poly.h))
    return poly


def powerfulWords(table, words, q, to_powerful):
    """PowerfulConversion::polyToPowerful / powerfulToPoly of int64 words [B, phi(m)] modulo 2 <= q < 2^62 -> int64
    [B, phi(m)] in [0, q) (hx_powerful_words)"""
    w = np.ascontiguousarray(np.atleast_2d(np.asarray(words, dtype=np.int64)))
    if w.ndim != 2 or w.shape[1] != table.context.phim:
        raise InvalidArgument(HX_ERR_INVALID, "the words are not [B, phi(m)]")
    out = np.zeros_like(w)
    _chk(lib().hx_powerful_words(table.h, 1 if to_powerful else 0, int(q), _p(w), w.shape[0], _p(out)))
    return out


def recryptPrep(poly, out_set, q, p, p2r, p2ePrime, tie_seed, part, debug=False):
    """The pre-processing of reCrypt for one ciphertext part (hx_recrypt_prep): rawModSwitch to q = p^e + 1,
    newMakeDivisible and the division by p2ePrime = p^e', per coefficient, on the device.  poly: coefficient rows (after
    iFFT and polyToPowerful); -> a new DoubleCRT on the primes out_set whose row t is w mod t.  debug: also the host
    arrays x, v, int64 [batch, phi(m)]."""
    out = DoubleCRT(poly.context, list(out_set), poly.batch, zero=False)
    x = v = None
    if debug:
        x = np.zeros((poly.batch, poly.context.phim), dtype=np.int64)
        v = np.zeros_like(x)
    _chk(lib().hx_recrypt_prep(poly.h, out.h, int(q), int(p), int(p2r), int(p2ePrime),
                               int(tie_seed) & (2 ** 64 - 1), int(part), None if x is None else _p(x), None if v is None else _p(v)))
    return (out, x, v) if debug else out
