"""ctypes binding of libtinyntt.so (include/tinyntt.h) — the thin Python shim over the C ABI.

Host-side mirror of the reference's operator for the hot path:
`nwc_poly_mult(a, b, psi_2n) -> c` (new_reference/cg_ntt.py:78-92) and the
transforms around it, batched.  All compute happens in the HIP kernels behind
the C ABI; this module only marshals pointers.  There is no CPU fallback: if the
library is missing or no HIP device is visible, calls raise.

Buffers may be
  * numpy arrays (host)  -> the *_host entry points (H2D, kernel, D2H, sync), or
  * torch tensors on a CUDA/HIP device -> the *_dev entry points (enqueue on the
    plan's stream or on a given torch stream; no copies).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

from . import numtheory

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TINYNTT_LIB") or os.path.join(_HERE, "lib", "libtinyntt.so")   # env override: developer A/B builds

# tn_status (include/tinyntt.h)
TN_OK, TN_EBADLEN, TN_EBADPARAM, TN_ENODEVICE, TN_EHIP, TN_ENOMEM, TN_EINVAL, TN_EUNSUPPORTED = range(8)
# tn_variant
VARIANT_AUTO, VARIANT_FUSED, VARIANT_CG, VARIANT_CG8, VARIANT_CG8_PADDED = range(5)
VARIANTS = {"auto": VARIANT_AUTO, "fused": VARIANT_FUSED, "cg": VARIANT_CG, "cg8": VARIANT_CG8, "cg8_padded": VARIANT_CG8_PADDED,
            # lane-grouping x LDS-layout sweep of the constant-geometry kernel (BASELINE config 5)
            "cg_swizzled": 5, "cg8_swizzled": 6, "cg2": 7, "cg2_padded": 8, "cg2_swizzled": 9, "cg4": 10, "cg4_padded": 11, "cg4_swizzled": 12}
CG_VARIANTS = tuple(k for k in VARIANTS if k.startswith("cg"))
PLAN_FORCE_CANONICAL = 1
GALOIS_MAX = 16               # Galois elements per automorphism call: include/tinyntt.h TN_GALOIS_MAX
MONOMIAL_MINUS_ONE = 1        # (X^e - 1) * a instead of X^e * a: include/tinyntt.h TN_MONOMIAL_MINUS_ONE
GADGET_BALANCED = 1           # digits in [-B/2, B/2): include/tinyntt.h TN_GADGET_BALANCED
PLAN_CANONICAL_INPUTS = 2     # the caller promises inputs in [0, q): include/tinyntt.h TN_PLAN_CANONICAL_INPUTS

# Every symbol include/tinyntt.h declares (tests check the built library exports them all).
EXPORTED_SYMBOLS = (
    "tn_plan_create", "tn_plan_create_omega", "tn_plan_create_general", "tn_plan_is_general", "tn_plan_destroy", "tn_plan_n", "tn_plan_q", "tn_plan_psi", "tn_plan_omega",
    "tn_plan_elem_bytes", "tn_plan_device", "tn_plan_has_fused", "tn_plan_is_lazy",
    "tn_poly_mult_dev", "tn_poly_mult_host", "tn_plan_set_host_chunk_rows", "tn_cyclic_poly_mult_dev", "tn_pointwise_mul_dev", "tn_schoolbook_dev",
    "tn_prepare_dev", "tn_poly_mult_prepared_dev", "tn_poly_dot_prepared_dev", "tn_unprepare_dev", "tn_poly_dot_hat_dev",
    "tn_gadget_decompose_dev", "tn_poly_gadget_dot_prepared_dev", "tn_poly_gadget_multidot_prepared_dev",
    "tn_poly_external_product_prepared_dev",
    "tn_monomial_mul_dev", "tn_poly_cmux_rotate_prepared_dev", "tn_poly_blind_rotate_prepared_dev",
    "tn_automorphism_dev", "tn_automorphism_prepared_dev", "tn_poly_galois_keyswitch_prepared_dev", "tn_poly_pack_step_prepared_dev",
    "tn_lwe_modswitch_dev", "tn_sample_extract_dev", "tn_lwe_embed_dev", "tn_lwe_keyswitch_dev",
    "tn_lwe_ksk_prepared_bytes", "tn_lwe_ksk_prepare_dev", "tn_lwe_keyswitch_prepared_dev",
    "tn_plan_export_table", "tn_ntt_forward_dev", "tn_ntt_inverse_dev",
    "tn_ntt_forward_host", "tn_ntt_inverse_host", "tn_ntt_forward_trace_host", "tn_twisted_ntt_forward_dev",
    "tn_twisted_ntt_forward_host", "tn_schoolbook_host",
    "tn_fill_lcg_dev", "tn_checksum_rows_dev", "tn_plan_synchronize", "tn_time_poly_mult_dev",
    "tn_kernel_name", "tn_last_error", "tn_status_string", "tn_version", "tn_build_id",
    "tn_shard_rows", "tn_multi_create", "tn_multi_destroy", "tn_multi_size", "tn_multi_plan", "tn_multi_device",
    "tn_multi_poly_mult_host", "tn_multi_poly_mult_dev", "tn_multi_synchronize", "tn_multi_last_error",
)


class TinyNttError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libtinyntt: {message} (status {status})")
        self.status = status


_lib = None


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """Load libtinyntt.so (built in-tree by `make -C tiny_ntt_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"{p} not found: the HIP extension is not built. Run `make -C tiny_ntt_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback."
        )
    # PyTorch-ROCm bundles its own libamdhip64.so.7; two HIP runtimes in one process cannot both
    # own the GPU, so when torch is installed let it load first and bind libtinyntt to that copy.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = ctypes.CDLL(p)
    vp, u32, u64, sz, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
    lib.tn_plan_create.argtypes = [ctypes.POINTER(vp), u32, u64, u64, ci, u32]
    lib.tn_plan_create_omega.argtypes = [ctypes.POINTER(vp), u32, u64, u64, ci, u32]
    lib.tn_plan_create_general.argtypes = [ctypes.POINTER(vp), u32, u64, u64, ci, u32]
    lib.tn_plan_destroy.argtypes = [vp]
    for name, res in (("tn_plan_n", u32), ("tn_plan_q", u64), ("tn_plan_psi", u64), ("tn_plan_omega", u64),
                      ("tn_plan_elem_bytes", u32), ("tn_plan_device", ci), ("tn_plan_has_fused", ci), ("tn_plan_is_lazy", ci),
                      ("tn_plan_is_general", ci)):
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = res
    lib.tn_poly_mult_dev.argtypes = [vp, vp, vp, vp, sz, ci, vp]
    lib.tn_poly_mult_host.argtypes = [vp, vp, vp, vp, sz, ci]
    lib.tn_plan_set_host_chunk_rows.argtypes = [vp, sz]
    lib.tn_cyclic_poly_mult_dev.argtypes = [vp, vp, vp, vp, sz, ci, vp]
    lib.tn_pointwise_mul_dev.argtypes = [vp, vp, vp, vp, sz, vp]
    lib.tn_prepare_dev.argtypes = [vp, vp, vp, sz, vp]
    lib.tn_poly_mult_prepared_dev.argtypes = [vp, vp, vp, sz, vp, sz, vp]
    lib.tn_poly_dot_prepared_dev.argtypes = [vp, vp, vp, sz, vp, sz, sz, vp]
    lib.tn_unprepare_dev.argtypes = [vp, vp, vp, sz, vp]
    lib.tn_poly_dot_hat_dev.argtypes = [vp, vp, vp, sz, vp, sz, sz, ci, vp]
    lib.tn_gadget_decompose_dev.argtypes = [vp, vp, vp, sz, sz, u32, u32, vp]
    lib.tn_poly_gadget_dot_prepared_dev.argtypes = [vp, vp, vp, sz, vp, sz, sz, u32, u32, vp]
    lib.tn_poly_gadget_multidot_prepared_dev.argtypes = [vp, vp, vp, sz, vp, sz, sz, sz, u32, u32, vp]
    lib.tn_poly_external_product_prepared_dev.argtypes = [vp, vp, vp, sz, vp, sz, sz, sz, sz, u32, u32, vp]
    lib.tn_monomial_mul_dev.argtypes = [vp, vp, vp, vp, sz, sz, u32, vp]
    lib.tn_poly_cmux_rotate_prepared_dev.argtypes = [vp, vp, vp, vp, sz, vp, sz, sz, sz, u32, u32, vp]
    lib.tn_poly_blind_rotate_prepared_dev.argtypes = [vp, vp, vp, vp, vp, sz, sz, sz, sz, u32, u32, vp]
    lib.tn_automorphism_dev.argtypes = [vp, vp, vp, sz, ctypes.POINTER(u32), sz, vp]
    lib.tn_automorphism_prepared_dev.argtypes = [vp, vp, vp, sz, ctypes.POINTER(u32), sz, vp]
    lib.tn_poly_galois_keyswitch_prepared_dev.argtypes = [vp, vp, u32, vp, sz, vp, sz, sz, u32, u32, vp]
    lib.tn_poly_pack_step_prepared_dev.argtypes = [vp, vp, vp, u32, u32, vp, sz, vp, sz, sz, u32, u32, vp]
    lib.tn_lwe_embed_dev.argtypes = [vp, vp, vp, sz, u32, vp]
    lib.tn_lwe_modswitch_dev.argtypes = [vp, vp, vp, sz, sz, vp]
    lib.tn_sample_extract_dev.argtypes = [vp, vp, vp, sz, u32, vp]
    lib.tn_lwe_keyswitch_dev.argtypes = [vp, vp, vp, vp, sz, sz, sz, sz, u32, u32, vp]
    lib.tn_lwe_ksk_prepared_bytes.argtypes = [vp, sz, sz, sz, ctypes.POINTER(sz)]
    lib.tn_lwe_ksk_prepare_dev.argtypes = [vp, vp, vp, sz, sz, sz, vp]
    lib.tn_lwe_keyswitch_prepared_dev.argtypes = [vp, vp, vp, vp, sz, sz, sz, sz, u32, u32, vp]
    lib.tn_schoolbook_dev.argtypes = [vp, vp, vp, vp, sz, vp]
    lib.tn_plan_export_table.argtypes = [vp, ci, vp]
    for name in ("tn_ntt_forward_dev", "tn_ntt_inverse_dev", "tn_twisted_ntt_forward_dev"):
        getattr(lib, name).argtypes = [vp, vp, vp, sz, ci, vp]
    lib.tn_schoolbook_host.argtypes = [vp, vp, vp, vp, sz]
    for name in ("tn_ntt_forward_host", "tn_ntt_inverse_host", "tn_twisted_ntt_forward_host"):
        getattr(lib, name).argtypes = [vp, vp, vp, sz, ci]
    lib.tn_ntt_forward_trace_host.argtypes = [vp, vp, vp, vp, ci]
    lib.tn_fill_lcg_dev.argtypes = [vp, vp, sz, u64, u64, vp]
    lib.tn_checksum_rows_dev.argtypes = [vp, vp, vp, sz, vp]
    lib.tn_plan_synchronize.argtypes = [vp]
    lib.tn_time_poly_mult_dev.argtypes = [vp, vp, vp, vp, sz, ci, ci, ctypes.POINTER(ctypes.c_float)]
    lib.tn_kernel_name.argtypes = [vp, ci]
    lib.tn_kernel_name.restype = ctypes.c_char_p
    lib.tn_last_error.restype = ctypes.c_char_p
    lib.tn_status_string.argtypes = [ci]
    lib.tn_status_string.restype = ctypes.c_char_p
    lib.tn_version.restype = ci
    lib.tn_build_id.restype = ctypes.c_char_p
    lib.tn_shard_rows.argtypes = [sz, ci, ci, ctypes.POINTER(sz), ctypes.POINTER(sz)]
    lib.tn_multi_create.argtypes = [ctypes.POINTER(vp), u32, u64, u64, ctypes.POINTER(ci), ci, u32]
    lib.tn_multi_destroy.argtypes = [vp]
    lib.tn_multi_size.argtypes = [vp]
    lib.tn_multi_plan.argtypes = [vp, ci]; lib.tn_multi_plan.restype = vp
    lib.tn_multi_device.argtypes = [vp, ci]
    lib.tn_multi_poly_mult_host.argtypes = [vp, vp, vp, vp, sz, ci]
    lib.tn_multi_poly_mult_dev.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(sz), ci]
    lib.tn_multi_synchronize.argtypes = [vp]
    lib.tn_multi_last_error.restype = ctypes.c_char_p
    if path is None:
        _lib = lib
    return lib


def build_id() -> str:
    """sha256 prefix of the sources the loaded libtinyntt.so was compiled from (tn_build_id)."""
    return load_library().tn_build_id().decode()


def _check(lib, status: int, last_error=None):
    """Raise for a status other than TN_OK; last_error: the getter of the text (tn_multi_* keep their own)."""
    if status == TN_OK:
        return
    msg = (last_error or lib.tn_last_error)().decode() or lib.tn_status_string(status).decode()
    if status == TN_EBADLEN:
        raise ValueError(msg)          # the reference raises ValueError on a wrong length (cg_ntt.py:36-37,:79-80)
    raise TinyNttError(status, msg)


def _variant(v) -> int:
    if isinstance(v, str):
        return VARIANTS[v]
    return int(v)


def _is_torch(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


class PreparedOperand:
    """Second operand of the negacyclic product, transformed once (Plan.prepare) for any number of Plan.poly_mult_prepared
    calls.  Opaque device words (include/tinyntt.h: tn_prepare_dev), valid only with the plan that made them."""

    def __init__(self, plan, tensor, rows: int):
        self.plan, self.tensor, self.rows = plan, tensor, int(rows)


class PreparedLweKey:
    """An LWE key-switch key prepared once (Plan.lwe_ksk_prepare) for any number of Plan.lwe_keyswitch_prepared calls: opaque
    device bytes (include/tinyntt.h: tn_lwe_ksk_prepare_dev), valid only with the plan that made them."""

    def __init__(self, plan, tensor, n_in: int, n_out: int, terms: int):
        self.plan, self.tensor, self.n_in, self.n_out, self.terms = plan, tensor, int(n_in), int(n_out), int(terms)


class Plan:
    """Immutable (n, q, psi) plan on one HIP device: twiddle tables + stream.

    Replaces the reference's module constants N, Q (cg_ntt.py:5-6), the psi_2n
    argument (:78) and the constexpr tables of the C++ benchmark
    (benchmark_ntt_60bit.cpp:43-64).

    How coefficients are read (the reference takes Python ints and reduces them with %, cg_ntt.py:82-83):
      * HOST arrays / lists are VALUES: Python ints of any size and sign, and numpy signed integers, are taken mod q with
        Python's non-negative % (-1 -> q - 1); unsigned words wider than the plan's lanes are reduced, not truncated;
        floats raise TypeError.  So a numpy int64 array that was meant as a bag of 64-bit PATTERNS (words >= 2^63 showing as
        negatives, e.g. tensor.numpy() of a torch int64 tensor) must be passed as .view(np.uint64).
      * DEVICE tensors are BIT PATTERNS: torch has no unsigned 64-bit dtype, so torch.int64 / int32 storage is read as
        unsigned words (torch_dtype); the kernels take every word mod q.
    tests/test_host_logic.py::test_host_rows_take_integers_mod_q_and_refuse_floats and
    tests/test_gpu_parity.py::test_signed_host_values_and_device_bit_patterns pin both rules against the reference's %.
    """

    def __init__(self, n: int, q: int, psi: int, device: int = 0, flags: int = 0, omega: int = None, general: bool = False):
        """omega given (psi ignored): an OMEGA-ONLY plan (tn_plan_create_omega) — cg_ntt / cg_intt for any omega_n.
        general: tn_plan_create_general — nothing validated, nwc_poly_mult for ANY psi / modulus as cg_ntt.py:78-92 computes it."""
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        if not (0 <= int(n) < 2 ** 32):
            raise ValueError(f"Expected a power-of-two length >= 4, got {n}")
        if not (0 < int(q) < 2 ** 64):
            raise TinyNttError(TN_EBADPARAM, "q must be an odd prime below 2^62")
        self.omega_only = omega is not None
        self.general = bool(general) and not self.omega_only
        if self.general:
            _check(self._lib, self._lib.tn_plan_create_general(ctypes.byref(self._h), int(n), int(q), int(psi) % int(q), int(device), int(flags)))
        elif self.omega_only:
            _check(self._lib, self._lib.tn_plan_create_omega(ctypes.byref(self._h), int(n), int(q), int(omega) % int(q), int(device), int(flags)))
            psi = 0
        else:
            _check(self._lib, self._lib.tn_plan_create(ctypes.byref(self._h), int(n), int(q), int(psi) % int(q), int(device), int(flags)))
        self.n, self.q, self.psi = int(n), int(q), int(psi) % int(q)
        self.omega = int(self._lib.tn_plan_omega(self._h))
        self.elem_bytes = int(self._lib.tn_plan_elem_bytes(self._h))
        self.dtype = np.uint32 if self.elem_bytes == 4 else np.uint64
        self.device = int(device)
        self.has_fused = bool(self._lib.tn_plan_has_fused(self._h))
        self.is_lazy = bool(self._lib.tn_plan_is_lazy(self._h))
        self.logn = self.n.bit_length() - 1

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tn_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers -------------------------------------------------------------
    @property
    def torch_dtype(self):
        import torch
        return torch.int32 if self.elem_bytes == 4 else torch.int64   # DEVICE tensors: bit patterns, read as unsigned words (class docstring)

    def _host_rows(self, x, name):
        arr = np.asarray(x)
        if arr.dtype == object:                     # Python ints of any size / sign: taken mod q like the reference's % (cg_ntt.py:82-83)
            arr = np.array([int(v) % self.q for v in arr.ravel()], dtype=self.dtype).reshape(arr.shape)
        elif arr.dtype.kind == "i":                 # signed words: Python's % is non-negative
            arr = np.mod(arr.astype(np.int64), self.q).astype(self.dtype) if arr.size and arr.min() < 0 else arr
        elif arr.dtype.kind not in "u":
            raise TypeError(f"{name}: coefficients must be integers, got dtype {arr.dtype}")
        if arr.dtype.itemsize > self.elem_bytes and arr.size and int(arr.max()) >= 2 ** (8 * self.elem_bytes):
            arr = np.mod(arr, self.q)               # wider words than the plan's lanes: reduce instead of truncating
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        if arr.ndim == 1:
            arr = arr[None, :]
        if arr.ndim != 2 or arr.shape[1] != self.n:
            raise ValueError(f"Expected {self.n} coefficients, got {arr.shape[-1] if arr.ndim else 0}")
        return arr

    def _dev_rows(self, t, name):
        if not t.is_cuda:
            raise TinyNttError(TN_EINVAL, f"{name}: torch tensor must live on a HIP device")
        if t.element_size() != self.elem_bytes or not t.is_contiguous():
            raise TinyNttError(TN_EINVAL, f"{name}: need a contiguous tensor of {self.elem_bytes}-byte integers")
        if t.dim() == 1:
            rows, cols = 1, t.shape[0]
        elif t.dim() == 2:
            rows, cols = t.shape
        else:
            raise ValueError(f"Expected {self.n} coefficients")
        if cols != self.n:
            raise ValueError(f"Expected {self.n} coefficients, got {cols}")
        return rows

    def _stream_ptr(self, stream):
        """HIP stream handle for the *_dev entry points.

        None  -> torch's current stream on the plan's device, so results obey normal torch stream
                 semantics (torch's default stream has handle 0 = hipStreamLegacy, passed as
                 TN_STREAM_LEGACY because NULL means "the plan's own stream" in the C ABI);
        "plan" -> the plan's own non-blocking stream (call synchronize() before reading results);
        a torch.cuda.Stream or raw integer handle -> that stream.
        """
        if isinstance(stream, str) and stream == "plan":
            return None
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self.device)
        h = int(getattr(stream, "cuda_stream", stream))
        return ctypes.c_void_p(h if h else 1)

    def set_host_chunk_rows(self, rows: int):
        """Rows per chunk of the H2D -> kernel -> D2H pipeline behind the host-buffer entry points (0 = automatic)."""
        _check(self._lib, self._lib.tn_plan_set_host_chunk_rows(self._h, int(rows)))

    # ---- the operator ----------------------------------------------------------
    def poly_mult(self, a, b, variant="auto", out=None, stream=None):
        """c[r] = a[r] * b[r] in Z_q[x]/(x^n+1).  nwc_poly_mult (cg_ntt.py:78-92), batched."""
        v = _variant(variant)
        if _is_torch(a):
            import torch
            rows = self._dev_rows(a, "a")
            if self._dev_rows(b, "b") != rows:
                raise ValueError(f"Expected {self.n} coefficients")
            c = out if out is not None else torch.empty_like(a)
            self._dev_rows(c, "out")
            _check(self._lib, self._lib.tn_poly_mult_dev(self._h, a.data_ptr(), b.data_ptr(), c.data_ptr(), rows, v, self._stream_ptr(stream)))
            return c
        squeeze = np.ndim(a) == 1
        ha, hb = self._host_rows(a, "a"), self._host_rows(b, "b")
        if ha.shape != hb.shape:
            raise ValueError(f"Expected {self.n} coefficients")
        if out is not None:                  # caller-provided (e.g. pinned) result buffer
            if not (isinstance(out, np.ndarray) and out.dtype == self.dtype and out.flags.c_contiguous and out.size == ha.size):
                raise ValueError("out must be a C-contiguous array of the plan's dtype with the shape of a")
            hc = out.reshape(ha.shape)
        else:
            hc = np.empty_like(ha)
        _check(self._lib, self._lib.tn_poly_mult_host(self._h, ha.ctypes.data, hb.ctypes.data, hc.ctypes.data, ha.shape[0], v))
        return hc[0] if squeeze else hc

    def _binary_dev(self, fn, a, b, out, stream, *extra):
        """Shared marshalling of the device-only binary operators; numpy inputs are staged through torch."""
        import torch
        a, rows, host, one = self._rows_in(a)
        if host:
            b = self.to_device(b)
        if self._dev_rows(b, "b") != rows:
            raise ValueError(f"Expected {self.n} coefficients")
        c = out if out is not None else torch.empty_like(a)
        _check(self._lib, fn(self._h, a.data_ptr(), b.data_ptr(), c.data_ptr(), rows, *extra, self._stream_ptr(stream)))
        return self._result(c, host, host and one)

    # ---- the prepared family: one marshalling path --------------------------------
    def _rows_in(self, a):
        """a as a contiguous device tensor of rows -> (tensor, rows, came from the host, one polynomial)."""
        host = not _is_torch(a)
        one = (np.ndim(a) if host else a.dim()) == 1
        if host:
            a = self.to_device(a)
        return a, self._dev_rows(a, "a"), host, one

    def _own_prepared(self, prepared, fn, which):
        if not isinstance(prepared, PreparedOperand):
            raise TypeError(f"{fn}: the {which} must come from Plan.prepare (or Plan.poly_dot_hat with keep_prepared)")
        if prepared.plan is not self:
            raise TinyNttError(TN_EINVAL, f"{fn}: the prepared operand belongs to another plan")

    @staticmethod
    def _sets(prepared, batch, terms, which="prepared operand"):
        """bhat_sets of the C ABI: 1 when `prepared` holds one set of `terms` rows for every output row, batch when a set per row."""
        if prepared.rows not in (terms, batch * terms):
            raise ValueError(f"Expected a {which} of {terms} or {batch * terms} rows, got {prepared.rows}")
        return 1 if prepared.rows == terms else batch

    def _out_rows(self, out, batch, device):
        """out, or a new tensor on `device`: `batch` rows of the plan's words."""
        import torch
        c = out if out is not None else torch.empty((batch, self.n), dtype=self.torch_dtype, device=device)
        if self._dev_rows(c, "out") != batch:
            raise ValueError(f"Expected an output of {batch} rows of {self.n} coefficients")
        return c

    def _result(self, c, host, one, out=None):
        """Hand c back: a host array where the input came from the host; row 0 alone where one polynomial went in (and, on the
        device, the caller gave no `out`)."""
        if host:
            res = self.to_host(c)
            return res[0] if one else res
        return c[0] if one and out is None else c

    def prepare(self, b, out=None, stream=None) -> PreparedOperand:
        """Transform b once (tn_prepare_dev): b is one polynomial or [rows, n], host values (taken mod q) or a device tensor."""
        import torch
        if not _is_torch(b):
            b = self.to_device(b)
        rows = self._dev_rows(b, "b")
        t = out if out is not None else torch.empty((rows, self.n), dtype=self.torch_dtype, device=b.device)
        if self._dev_rows(t, "out") != rows:
            raise ValueError(f"Expected {rows} rows of {self.n} coefficients")
        _check(self._lib, self._lib.tn_prepare_dev(self._h, b.data_ptr(), t.data_ptr(), rows, self._stream_ptr(stream)))
        return PreparedOperand(self, t, rows)

    def poly_mult_prepared(self, a, prepared: PreparedOperand, out=None, stream=None):
        """c[r] = a[r] * b[r] in Z_q[x]/(x^n+1) with b given as Plan.prepare(b) (tn_poly_mult_prepared_dev): two transforms per
        row instead of three.  A prepared operand of ONE row is multiplied into every row of a."""
        import torch
        self._own_prepared(prepared, "poly_mult_prepared", "second operand")
        a, rows, host, one = self._rows_in(a)
        c = out if out is not None else torch.empty_like(a)
        self._dev_rows(c, "out")
        _check(self._lib, self._lib.tn_poly_mult_prepared_dev(self._h, a.data_ptr(), prepared.tensor.data_ptr(), prepared.rows, c.data_ptr(), rows,
                                                              self._stream_ptr(stream)))
        return self._result(c, host, host and one)

    def poly_dot_prepared(self, a, prepared: PreparedOperand, out=None, stream=None):
        """c[r] = sum_j a[r][j] * b[r][j] in Z_q[x]/(x^n+1) with b given as Plan.prepare(b) (tn_poly_dot_prepared_dev): one inverse
        transform per output row.  a is (batch, terms, n), or (terms, n) for one output polynomial; the prepared operand has
        batch * terms rows, or `terms` rows that every output row is multiplied by.  Returns (batch, n) or (n,)."""
        self._own_prepared(prepared, "poly_dot_prepared", "second operand")
        host = not _is_torch(a)
        if host:
            a = np.asarray(a)
        if a.ndim not in (2, 3) or a.shape[-1] != self.n or a.shape[-2] == 0:
            raise ValueError(f"Expected a of shape (batch, terms, {self.n}) or (terms, {self.n})")
        squeeze = a.ndim == 2
        terms = int(a.shape[-2])
        batch = 1 if squeeze else int(a.shape[0])
        if host:
            a = self.to_device(a.reshape(batch * terms, self.n))
        else:
            if not a.is_contiguous():
                raise TinyNttError(TN_EINVAL, f"a: need a contiguous tensor of {self.elem_bytes}-byte integers")
            self._dev_rows(a.reshape(batch * terms, self.n), "a")
        sets = self._sets(prepared, batch, terms)
        c = self._out_rows(out, batch, a.device)
        _check(self._lib, self._lib.tn_poly_dot_prepared_dev(self._h, a.data_ptr(), prepared.tensor.data_ptr(), sets, c.data_ptr(), batch, terms,
                                                             self._stream_ptr(stream)))
        return self._result(c, host, squeeze, out)

    def unprepare(self, prepared: PreparedOperand, out=None, stream=None):
        """The polynomials whose prepared form `prepared` holds (tn_unprepare_dev): a device tensor (rows, n) of canonical residues,
        the inverse of Plan.prepare."""
        self._own_prepared(prepared, "unprepare", "operand")
        rows = prepared.rows
        x = self._out_rows(out, rows, prepared.tensor.device)
        _check(self._lib, self._lib.tn_unprepare_dev(self._h, prepared.tensor.data_ptr(), x.data_ptr(), rows, self._stream_ptr(stream)))
        return x

    def poly_dot_hat(self, a_prepared: PreparedOperand, b_prepared: PreparedOperand, terms=1, out=None, stream=None, keep_prepared=False):
        """c[r] = sum_j a[r][j] * b[r][j] in Z_q[x]/(x^n+1) with BOTH operands prepared (tn_poly_dot_hat_dev).  a_prepared holds
        batch * terms rows (the terms of one output row are consecutive); b_prepared holds as many, or `terms` rows that every
        output row is multiplied by.  Returns a device tensor (batch, n) of coefficients, or, with keep_prepared, a
        PreparedOperand of batch rows (no transform runs; prepared rows of one plan add word-wise mod q)."""
        self._own_prepared(a_prepared, "poly_dot_hat", "first operand")
        self._own_prepared(b_prepared, "poly_dot_hat", "second operand")
        terms = int(terms)
        if terms < 1 or a_prepared.rows % terms:
            raise ValueError(f"Expected a first operand of batch * {terms} rows, got {a_prepared.rows}")
        batch = a_prepared.rows // terms
        sets = self._sets(b_prepared, batch, terms, "second operand")
        if isinstance(out, PreparedOperand):
            out = out.tensor
        c = self._out_rows(out, batch, a_prepared.tensor.device)
        _check(self._lib, self._lib.tn_poly_dot_hat_dev(self._h, a_prepared.tensor.data_ptr(), b_prepared.tensor.data_ptr(), sets, c.data_ptr(), batch,
                                                        terms, 1 if keep_prepared else 0, self._stream_ptr(stream)))
        return PreparedOperand(self, c, batch) if keep_prepared else c

    def gadget_decompose(self, a, terms, base_log, balanced=False, out=None, stream=None):
        """The base-2^base_log digits of every coefficient of a, taken mod q (tn_gadget_decompose_dev; include/tinyntt.h has the
        definition): a is (batch, n) or (n,), host values or a device tensor; returns (batch, terms, n) or (terms, n), canonical
        residues, digit polynomial j of row r at [r, j].  balanced: digits in [-B/2, B/2), negative ones stored as q + d.  Works
        on every plan."""
        import torch
        a, batch, host, one = self._rows_in(a)
        terms = int(terms)
        if terms < 1:
            raise ValueError(f"Expected terms >= 1, got {terms}")
        d = out if out is not None else torch.empty((batch, terms, self.n), dtype=self.torch_dtype, device=a.device)
        if not d.is_contiguous() or d.dtype != self.torch_dtype or d.numel() != batch * terms * self.n:
            raise ValueError(f"Expected an output of {batch} x {terms} rows of {self.n} coefficients")
        _check(self._lib, self._lib.tn_gadget_decompose_dev(self._h, a.data_ptr(), d.data_ptr(), batch, terms, int(base_log),
                                                            GADGET_BALANCED if balanced else 0, self._stream_ptr(stream)))
        return self._result(d.reshape(batch, terms, self.n) if host else d, host, one, out)

    def poly_gadget_dot_prepared(self, a, prepared: PreparedOperand, terms, base_log, balanced=False, out=None, stream=None):
        """c[r] = sum_j digit_j(a[r]) * b[r][j] in Z_q[x]/(x^n+1) with b given as Plan.prepare(b) (tn_poly_gadget_dot_prepared_dev):
        the digits of gadget_decompose are cut inside the kernel, so a is read once and they never reach memory.  a is (batch, n)
        or (n,); the prepared operand has batch * terms rows, or `terms` rows that every output row is multiplied by.  Returns
        (batch, n) or (n,), bit-identical to poly_dot_prepared(gadget_decompose(a, ...), prepared)."""
        self._own_prepared(prepared, "poly_gadget_dot_prepared", "second operand")
        a, batch, host, one = self._rows_in(a)
        terms = int(terms)
        if terms < 1:
            raise ValueError(f"Expected terms >= 1, got {terms}")
        sets = self._sets(prepared, batch, terms)
        c = self._out_rows(out, batch, a.device)
        _check(self._lib, self._lib.tn_poly_gadget_dot_prepared_dev(self._h, a.data_ptr(), prepared.tensor.data_ptr(), sets, c.data_ptr(), batch, terms,
                                                                    int(base_log), GADGET_BALANCED if balanced else 0, self._stream_ptr(stream)))
        return self._result(c, host, one, out)

    def poly_gadget_multidot_prepared(self, a, prepared: PreparedOperand, outs, terms, base_log, balanced=False, out=None, stream=None):
        """c[r][o] = sum_j digit_j(a[r]) * b[r][o][j] for o < outs (tn_poly_gadget_multidot_prepared_dev): the `outs` components of a
        key switch from ONE launch, the digits cut and transformed once for all of them.  a is (batch, n) or (n,); the prepared
        operand has batch * outs * terms rows ([batch][outs][terms]), or outs * terms rows that every output row is multiplied
        by.  outs is 1 or 2.  Returns (batch, outs, n) or (outs, n), bit-identical to poly_gadget_dot_prepared per component."""
        import torch
        self._own_prepared(prepared, "poly_gadget_multidot_prepared", "second operand")
        a, batch, host, one = self._rows_in(a)
        outs, terms = int(outs), int(terms)
        if terms < 1 or outs < 1:
            raise ValueError(f"Expected terms >= 1 and outs >= 1, got {terms} and {outs}")
        sets = self._sets(prepared, batch, outs * terms)
        c = out if out is not None else torch.empty((batch, outs, self.n), dtype=self.torch_dtype, device=a.device)
        if not _is_torch(c) or c.numel() != batch * outs * self.n or not c.is_contiguous():
            raise ValueError(f"Expected an output of {batch} x {outs} rows of {self.n} coefficients")
        self._dev_rows(c.reshape(batch * outs, self.n), "out")        # on the device, the plan's words: poly_gadget_dot_prepared's check
        _check(self._lib, self._lib.tn_poly_gadget_multidot_prepared_dev(self._h, a.data_ptr(), prepared.tensor.data_ptr(), sets, c.data_ptr(), batch,
                                                                         outs, terms, int(base_log), GADGET_BALANCED if balanced else 0,
                                                                         self._stream_ptr(stream)))
        return self._result(c.reshape(batch, outs, self.n) if host else c, host, one, out)

    def poly_external_product_prepared(self, a, prepared: PreparedOperand, outs, terms, base_log, balanced=False, out=None, stream=None):
        """c[r][o] = sum_i sum_j digit_j(a[r][i]) * b[r][o][i][j] for o < outs (tn_poly_external_product_prepared_dev): the external
        product RGSW x RLWE from ONE launch, the digits of every input polynomial cut and transformed once for both components.
        a is (batch, ins, n), or (ins, n) for one ciphertext, host values or a device tensor; the prepared operand has
        batch * outs * ins * terms rows ([batch][outs][ins][terms]), or outs * ins * terms rows that every output row is
        multiplied by.  ins >= 2 needs outs == 2; ins == 1 is poly_gadget_multidot_prepared.  Returns (batch, outs, n) or
        (outs, n), bit-identical per component to poly_dot_prepared on gadget_decompose of the (batch * ins, n) view of a."""
        import torch
        self._own_prepared(prepared, "poly_external_product_prepared", "second operand")
        host = not _is_torch(a)
        if host:
            a = np.asarray(a)
        if a.ndim not in (2, 3) or a.shape[-1] != self.n or a.shape[-2] == 0:
            raise ValueError(f"Expected a of shape (batch, ins, {self.n}) or (ins, {self.n})")
        one = a.ndim == 2
        ins = int(a.shape[-2])
        batch = 1 if one else int(a.shape[0])
        if host:
            a = self.to_device(a.reshape(batch * ins, self.n))
        else:
            if not a.is_contiguous():
                raise TinyNttError(TN_EINVAL, f"a: need a contiguous tensor of {self.elem_bytes}-byte integers")
            self._dev_rows(a.reshape(batch * ins, self.n), "a")
        outs, terms = int(outs), int(terms)
        if terms < 1 or outs < 1:
            raise ValueError(f"Expected terms >= 1 and outs >= 1, got {terms} and {outs}")
        sets = self._sets(prepared, batch, outs * ins * terms)
        c = out if out is not None else torch.empty((batch, outs, self.n), dtype=self.torch_dtype, device=a.device)
        if not _is_torch(c) or c.numel() != batch * outs * self.n or not c.is_contiguous():
            raise ValueError(f"Expected an output of {batch} x {outs} rows of {self.n} coefficients")
        self._dev_rows(c.reshape(batch * outs, self.n), "out")        # on the device, the plan's words: poly_gadget_dot_prepared's check
        _check(self._lib, self._lib.tn_poly_external_product_prepared_dev(self._h, a.data_ptr(), prepared.tensor.data_ptr(), sets, c.data_ptr(), batch,
                                                                          ins, outs, terms, int(base_log), GADGET_BALANCED if balanced else 0,
                                                                          self._stream_ptr(stream)))
        return self._result(c.reshape(batch, outs, self.n) if host else c, host, one, out)

    # ---- the CMux rotation step of a blind rotation ----------------------------------
    def _exps(self, exps, batch, device):
        """exps, a device tensor or host integers of `batch` entries -> a contiguous device tensor of 32-bit words (values are
        taken mod 2n by the kernels; host values are reduced here so that any Python integer fits the word)."""
        import torch
        if _is_torch(exps):
            if not exps.is_cuda:
                raise TinyNttError(TN_EINVAL, "exps: torch tensor must live on a HIP device")
            if exps.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not exps.is_contiguous():
                raise TinyNttError(TN_EINVAL, "exps: need a contiguous tensor of 32-bit integers")
            if exps.numel() != batch:
                raise ValueError(f"Expected {batch} exponents, got {exps.numel()}")
            return exps
        h = np.asarray(exps)
        if h.dtype == object or h.dtype.kind in "iu":
            h = np.array([int(v) % (2 * self.n) for v in h.ravel()], dtype=np.int64)
        else:
            raise TypeError(f"exps: exponents must be integers, got dtype {h.dtype}")
        if h.size != batch:
            raise ValueError(f"Expected {batch} exponents, got {h.size}")
        return torch.from_numpy(h.astype(np.int32)).to(device)

    def monomial_mul(self, a, exps, minus_one=False, out=None, stream=None):
        """X^e * a (or, with minus_one, (X^e - 1) * a) in Z_q[x]/(x^n + 1) with an exponent per batch item, any integer taken mod 2n
        (tn_monomial_mul_dev; include/tinyntt.h has the definition).  a is (batch, n) or (batch, group, n): exponent exps[r]
        applies to all `group` rows of item r; host values or a device tensor.  exps: a device tensor of 32-bit integers or host
        integers, `batch` entries.  Returns canonical residues in the shape of a; host arrays in give host arrays out.  Works
        on every plan."""
        import torch
        host = not _is_torch(a)
        if host:
            a = np.asarray(a)
        if a.ndim not in (2, 3) or a.shape[-1] != self.n or (a.ndim == 3 and a.shape[1] == 0):
            raise ValueError(f"Expected a of shape (batch, {self.n}) or (batch, group, {self.n})")
        shape = tuple(int(v) for v in a.shape)
        batch, group = shape[0], (shape[1] if len(shape) == 3 else 1)
        if host:
            a = self.to_device(a.reshape(batch * group, self.n))
        else:
            if not a.is_contiguous():
                raise TinyNttError(TN_EINVAL, f"a: need a contiguous tensor of {self.elem_bytes}-byte integers")
            self._dev_rows(a.reshape(batch * group, self.n), "a")
        e = self._exps(exps, batch, a.device)
        c = out if out is not None else torch.empty((batch * group, self.n), dtype=self.torch_dtype, device=a.device)
        if not _is_torch(c) or c.numel() != batch * group * self.n or not c.is_contiguous():
            raise ValueError(f"Expected an output of {batch} x {group} rows of {self.n} coefficients")
        self._dev_rows(c.reshape(batch * group, self.n), "out")
        _check(self._lib, self._lib.tn_monomial_mul_dev(self._h, a.data_ptr(), e.data_ptr(), c.data_ptr(), batch, group,
                                                        MONOMIAL_MINUS_ONE if minus_one else 0, self._stream_ptr(stream)))
        if host:
            return self.to_host(c).reshape(shape)
        return c if out is not None else c.reshape(shape)

    def poly_cmux_rotate_prepared(self, a, exps, prepared: PreparedOperand, terms, base_log, balanced=False, out=None, stream=None):
        """One step of a blind rotation from ONE launch (tn_poly_cmux_rotate_prepared_dev):
        c[r] = a[r] + RGSW [x] ((X^e_r - 1) * a[r]), that is c[r][o] = a[r][o] + sum_i sum_j digit_j((X^e_r - 1) a[r][i]) * b[r][o][i][j].
        a is (batch, 2, n), or (2, n) for one ciphertext, host values or a device tensor; exps as in monomial_mul; the prepared
        operand has batch * 4 * terms rows ([batch][2][2][terms]), or 4 * terms rows that every row is multiplied by.  Returns
        (batch, 2, n) or (2, n), bit-identical to monomial_mul(minus_one=True), poly_external_product_prepared and the addition
        mod q.  out must not be a: a blind rotation alternates two buffers (Plan.blind_rotate)."""
        import torch
        self._own_prepared(prepared, "poly_cmux_rotate_prepared", "key")
        host = not _is_torch(a)
        if host:
            a = np.asarray(a)
        if a.ndim not in (2, 3) or a.shape[-1] != self.n or a.shape[-2] == 0:
            raise ValueError(f"Expected a of shape (batch, comps, {self.n}) or (comps, {self.n})")
        one = a.ndim == 2
        comps = int(a.shape[-2])
        batch = 1 if one else int(a.shape[0])
        if host:
            a = self.to_device(a.reshape(batch * comps, self.n))
        else:
            if not a.is_contiguous():
                raise TinyNttError(TN_EINVAL, f"a: need a contiguous tensor of {self.elem_bytes}-byte integers")
            self._dev_rows(a.reshape(batch * comps, self.n), "a")
        terms = int(terms)
        if terms < 1:
            raise ValueError(f"Expected terms >= 1, got {terms}")
        sets = self._sets(prepared, batch, comps * comps * terms, "key")
        e = self._exps(exps, batch, a.device)
        c = out if out is not None else torch.empty((batch, comps, self.n), dtype=self.torch_dtype, device=a.device)
        if not _is_torch(c) or c.numel() != batch * comps * self.n or not c.is_contiguous():
            raise ValueError(f"Expected an output of {batch} x {comps} rows of {self.n} coefficients")
        self._dev_rows(c.reshape(batch * comps, self.n), "out")        # on the device, the plan's words: poly_gadget_dot_prepared's check
        _check(self._lib, self._lib.tn_poly_cmux_rotate_prepared_dev(self._h, a.data_ptr(), e.data_ptr(), prepared.tensor.data_ptr(), sets,
                                                                     c.data_ptr(), batch, comps, terms, int(base_log),
                                                                     GADGET_BALANCED if balanced else 0, self._stream_ptr(stream)))
        return self._result(c.reshape(batch, comps, self.n) if host else c, host, one, out)

    def poly_galois_keyswitch_prepared(self, a, galois, prepared: PreparedOperand, terms, base_log, balanced=False, out=None, stream=None):
        """The homomorphic automorphism of RLWE ciphertexts from ONE launch (tn_poly_galois_keyswitch_prepared_dev):
        c[r][0] = sigma_g(a[r][0]) + sum_j digit_j(sigma_g(a[r][1])) * b[r][0][j], c[r][1] = sum_j digit_j(sigma_g(a[r][1])) * b[r][1][j].
        a is (batch, 2, n), or (2, n) for one ciphertext, host values or a device tensor; galois is one odd integer below 2n; the
        prepared operand has batch * 2 * terms rows ([batch][2][terms]), or 2 * terms rows that every row is multiplied by (the
        layout of poly_gadget_multidot_prepared with outs = 2).  Returns (batch, 2, n) or (2, n), bit-identical to automorphism
        on both components, poly_gadget_multidot_prepared on the rotated second one and the addition mod q.  out must not be a."""
        import torch
        self._own_prepared(prepared, "poly_galois_keyswitch_prepared", "key")
        host = not _is_torch(a)
        if host:
            a = np.asarray(a)
        if a.ndim not in (2, 3) or a.shape[-1] != self.n or a.shape[-2] != 2:
            raise ValueError(f"Expected a of shape (batch, 2, {self.n}) or (2, {self.n})")
        one = a.ndim == 2
        batch = 1 if one else int(a.shape[0])
        if host:
            a = self.to_device(a.reshape(batch * 2, self.n))
        else:
            if not a.is_contiguous():
                raise TinyNttError(TN_EINVAL, f"a: need a contiguous tensor of {self.elem_bytes}-byte integers")
            self._dev_rows(a.reshape(batch * 2, self.n), "a")
        terms, g = int(terms), int(galois)
        if terms < 1:
            raise ValueError(f"Expected terms >= 1, got {terms}")
        if not 0 <= g < 2 ** 32:
            raise ValueError(f"Expected a Galois element below 2n = {2 * self.n}, got {g}")
        sets = self._sets(prepared, batch, 2 * terms, "key")
        c = out if out is not None else torch.empty((batch, 2, self.n), dtype=self.torch_dtype, device=a.device)
        if not _is_torch(c) or c.numel() != batch * 2 * self.n or not c.is_contiguous():
            raise ValueError(f"Expected an output of {batch} x 2 rows of {self.n} coefficients")
        self._dev_rows(c.reshape(batch * 2, self.n), "out")        # on the device, the plan's words: poly_gadget_dot_prepared's check
        _check(self._lib, self._lib.tn_poly_galois_keyswitch_prepared_dev(self._h, a.data_ptr(), g, prepared.tensor.data_ptr(), sets, c.data_ptr(),
                                                                          batch, terms, int(base_log), GADGET_BALANCED if balanced else 0,
                                                                          self._stream_ptr(stream)))
        return self._result(c.reshape(batch, 2, self.n) if host else c, host, one, out)

    def blind_rotate(self, acc, exps, prepared: PreparedOperand, terms, base_log, balanced=False, stream=None):
        """acc <- acc + RGSW_k [x] ((X^exps[k][r] - 1) * acc) for k = 0 .. steps - 1: poly_cmux_rotate_prepared step by step over two
        alternating buffers.  acc is a device tensor (batch, 2, n), left as it is; exps is (steps, batch), a device tensor of
        32-bit integers or host integers; prepared holds steps * 4 * terms rows, one shared key per step.  Returns the last
        buffer written (acc itself for no step)."""
        import torch
        self._own_prepared(prepared, "blind_rotate", "key")
        if not _is_torch(acc) or acc.dim() != 3:
            raise ValueError(f"Expected acc as a device tensor of shape (batch, 2, {self.n})")
        batch, steps, key = int(acc.shape[0]), len(exps), 4 * int(terms)
        if prepared.rows != steps * key:
            raise ValueError(f"Expected a key of {steps} x {key} rows, got {prepared.rows}")
        if not _is_torch(exps):
            exps = self._exps(np.asarray(exps).reshape(-1), steps * batch, acc.device).reshape(steps, batch)
        bufs = [torch.empty_like(acc), torch.empty_like(acc)]
        for k in range(steps):
            step_key = PreparedOperand(self, prepared.tensor[k * key:(k + 1) * key], key)
            acc = self.poly_cmux_rotate_prepared(acc, exps[k], step_key, terms, base_log, balanced, out=bufs[k & 1], stream=stream)
        return acc

    def poly_blind_rotate_prepared(self, acc, exps, prepared: PreparedOperand, terms, base_log, balanced=False, out=None, stream=None):
        """A blind rotation from ONE launch (tn_poly_blind_rotate_prepared_dev): the steps of blind_rotate with the accumulator
        kept on chip across them, bit-identical to that loop.  acc is a device tensor (batch, 2, n), left as it is unless out is
        acc; exps is (steps, batch), a device tensor of 32-bit integers or host integers; prepared holds steps * 4 * terms rows,
        one shared key per step.  out may be acc itself (in place) or another tensor of its shape that does not overlap it.
        Shapes whose accumulator does not fit a workgroup's LDS (n = 8192 with 64-bit words) raise TN_EUNSUPPORTED: use
        blind_rotate."""
        import torch
        self._own_prepared(prepared, "poly_blind_rotate_prepared", "key")
        if not _is_torch(acc) or acc.dim() != 3 or acc.shape[-1] != self.n or acc.shape[1] == 0:
            raise ValueError(f"Expected acc as a device tensor of shape (batch, 2, {self.n})")
        if not acc.is_contiguous():
            raise TinyNttError(TN_EINVAL, f"acc: need a contiguous tensor of {self.elem_bytes}-byte integers")
        batch, comps, terms = int(acc.shape[0]), int(acc.shape[1]), int(terms)
        self._dev_rows(acc.reshape(batch * comps, self.n), "acc")
        if terms < 1:
            raise ValueError(f"Expected terms >= 1, got {terms}")
        if _is_torch(exps):
            if exps.dim() != 2 or int(exps.shape[1]) != batch:
                raise ValueError(f"Expected exps of shape (steps, {batch})")
            steps = int(exps.shape[0])
            e = self._exps(exps, steps * batch, acc.device)
        else:
            h = np.asarray(exps)
            if h.ndim != 2 or h.shape[1] != batch:
                raise ValueError(f"Expected exps of shape (steps, {batch})")
            steps = int(h.shape[0])
            e = self._exps(h.reshape(-1), steps * batch, acc.device)
        key = comps * comps * terms
        if prepared.rows != steps * key:
            raise ValueError(f"Expected a key of {steps} x {key} rows, got {prepared.rows}")
        c = out if out is not None else torch.empty_like(acc)
        if not _is_torch(c) or c.numel() != batch * comps * self.n or not c.is_contiguous():
            raise ValueError(f"Expected an output of {batch} x {comps} rows of {self.n} coefficients")
        self._dev_rows(c.reshape(batch * comps, self.n), "out")
        _check(self._lib, self._lib.tn_poly_blind_rotate_prepared_dev(self._h, acc.data_ptr(), e.data_ptr(), prepared.tensor.data_ptr(), c.data_ptr(),
                                                                      batch, comps, steps, terms, int(base_log),
                                                                      GADGET_BALANCED if balanced else 0, self._stream_ptr(stream)))
        return c

    # ---- the LWE ends of a bootstrap ------------------------------------------------
    def _lwe_in(self, x, name, cols=None):
        """LWE rows (batch, d + 1), or (d + 1,) for one ciphertext, host values (taken mod q) or a device tensor of any words ->
        (contiguous device tensor (batch, d + 1), came from the host, one ciphertext).  cols: the row length expected."""
        import torch
        host = not _is_torch(x)
        if host:
            h = np.asarray(x)
            if h.dtype == object or h.dtype.kind == "i":
                h = np.array([int(v) % self.q for v in h.ravel()], dtype=self.dtype).reshape(h.shape)
            elif h.dtype.kind != "u":
                raise TypeError(f"{name}: words must be integers, got dtype {h.dtype}")
            elif h.dtype.itemsize > self.elem_bytes:
                h = np.mod(h, self.q)
            h = np.ascontiguousarray(h, dtype=self.dtype)
            x = torch.from_numpy(h.view(np.int32 if self.elem_bytes == 4 else np.int64)).to(f"cuda:{self.device}")
        elif not x.is_cuda or x.element_size() != self.elem_bytes or not x.is_contiguous():
            raise TinyNttError(TN_EINVAL, f"{name}: need a contiguous device tensor of {self.elem_bytes}-byte integers")
        one = x.dim() == 1
        if one:
            x = x[None, :]
        if x.dim() != 2 or x.shape[1] < 2 or (cols is not None and x.shape[1] != cols):
            raise ValueError(f"Expected {name} of shape (batch, {cols if cols is not None else 'dim + 1'})")
        return x, host, one

    def _lwe_out(self, out, shape, device, dtype=None):
        import torch
        dtype = dtype or self.torch_dtype
        c = out if out is not None else torch.empty(shape, dtype=dtype, device=device)
        if not _is_torch(c) or not c.is_cuda or c.numel() != int(np.prod(shape)) or not c.is_contiguous() or c.dtype != dtype:
            raise ValueError(f"Expected a contiguous device output of shape {tuple(shape)}")
        return c

    def lwe_modswitch(self, lwe, out=None, stream=None):
        """The modulus switch of LWE ciphertexts to 2n (tn_lwe_modswitch_dev): lwe is (batch, dim + 1) rows a_0 .. a_{dim-1}, b,
        host values or a device tensor of any words.  Returns the exponents TRANSPOSED, a 32-bit tensor (dim + 1, batch) with
        exps[i][r] = floor((2n x + floor(q / 2)) / q) mod 2n, x = lwe[r][i] mod q: exps[:dim] is the exps operand of
        poly_blind_rotate_prepared / blind_rotate, exps[dim] the body's exponent for monomial_mul.  Host rows in give a host
        array out.  Works on every plan."""
        import torch
        x, host, _ = self._lwe_in(lwe, "lwe")
        batch, dim = int(x.shape[0]), int(x.shape[1]) - 1
        e = self._lwe_out(out, (dim + 1, batch), x.device, torch.int32)
        _check(self._lib, self._lib.tn_lwe_modswitch_dev(self._h, x.data_ptr(), e.data_ptr(), batch, dim, self._stream_ptr(stream)))
        return e.cpu().numpy().view(np.uint32) if host else e

    def sample_extract(self, a, index=0, out=None, stream=None):
        """The LWE ciphertext of coefficient `index` of the phase of RLWE ciphertexts (tn_sample_extract_dev): a is (batch, 2, n),
        or (2, n) for one, phase c0 + c1 s; returns (batch, n + 1) rows (c1[index], c1[index - 1], .., c1[0], -c1[n - 1], ..,
        -c1[index + 1], c0[index]) mod q, whose phase b + <a, s> under the coefficients of s is that coefficient.  Host values or
        a device tensor in, the same kind out.  Works on every plan."""
        host = not _is_torch(a)
        if host:
            a = np.asarray(a)
        if a.ndim not in (2, 3) or a.shape[-1] != self.n or a.shape[-2] != 2:
            raise ValueError(f"Expected a of shape (batch, 2, {self.n}) or (2, {self.n})")
        one = a.ndim == 2
        batch = 1 if one else int(a.shape[0])
        if host:
            a = self.to_device(a.reshape(batch * 2, self.n))
        else:
            if not a.is_contiguous():
                raise TinyNttError(TN_EINVAL, f"a: need a contiguous tensor of {self.elem_bytes}-byte integers")
            self._dev_rows(a.reshape(batch * 2, self.n), "a")
        if not 0 <= int(index) < 2 ** 32:
            raise ValueError(f"Expected an index below n = {self.n}, got {index}")
        c = self._lwe_out(out, (batch, self.n + 1), a.device)
        _check(self._lib, self._lib.tn_sample_extract_dev(self._h, a.data_ptr(), c.data_ptr(), batch, int(index), self._stream_ptr(stream)))
        return self._result(c, host, one, out)

    def lwe_embed(self, lwe, index=0, out=None, stream=None):
        """The RLWE ciphertext whose phase has the phase of an LWE ciphertext at coefficient `index` (tn_lwe_embed_dev), the exact
        inverse of sample_extract at that index: lwe is (batch, n + 1), or (n + 1,) for one, under the coefficients of the ring key;
        returns (batch, 2, n), or (2, n), with c1[k] = lwe[index - k] for k <= index, -lwe[n + index - k] above it, and c0 the
        body at coefficient `index`, 0 elsewhere, all mod q.  The other coefficients of the phase are not zero: pack_lwes removes
        them.  Host values or a device tensor in, the same kind out.  Works on every plan."""
        x, host, one = self._lwe_in(lwe, "lwe", self.n + 1)
        batch = int(x.shape[0])
        if not 0 <= int(index) < 2 ** 32:
            raise ValueError(f"Expected an index below n = {self.n}, got {index}")
        c = self._lwe_out(out, (batch, 2, self.n), x.device)
        _check(self._lib, self._lib.tn_lwe_embed_dev(self._h, x.data_ptr(), c.data_ptr(), batch, int(index), self._stream_ptr(stream)))
        if host:
            res = self.to_host(c.reshape(batch * 2, self.n)).reshape(batch, 2, self.n)
            return res[0] if one else res
        return self._result(c, host, one, out)

    def poly_pack_step_prepared(self, ev, od, rot, galois, prepared: PreparedOperand, terms, base_log, balanced=False, out=None, stream=None):
        """One level of the LWE -> RLWE packing tree from ONE launch (tn_poly_pack_step_prepared_dev):
        c = (ev + X^rot od) + EvalAuto(ev - X^rot od, galois), that is, with t = X^rot od, s = ev + t, d = ev - t on both components,
        c[r][0] = s0 + sigma_g(d0) + sum_j digit_j(sigma_g(d1)) * b[r][0][j], c[r][1] = s1 + sum_j digit_j(sigma_g(d1)) * b[r][1][j].
        od=None is the trace step, c = ev + EvalAuto(ev, galois) (rot must be 0).  ev and od are (batch, 2, n), or (2, n) for one
        ciphertext, host values or device tensors (both of one kind); rot is an integer below 2n, galois one odd integer below 2n;
        the prepared operand is poly_galois_keyswitch_prepared's.  Returns (batch, 2, n) or (2, n), bit-identical to monomial_mul on
        od, the sum and the difference mod q, poly_galois_keyswitch_prepared on the difference and the addition of the sum.
        out must not overlap ev or od."""
        import torch
        self._own_prepared(prepared, "poly_pack_step_prepared", "key")
        host = not _is_torch(ev)
        if od is not None and _is_torch(od) == host:
            raise TypeError("poly_pack_step_prepared: ev and od must both be host values or both device tensors")

        def rows(x, name):
            if host:
                x = np.asarray(x)
            if x.ndim not in (2, 3) or x.shape[-1] != self.n or x.shape[-2] != 2:
                raise ValueError(f"Expected {name} of shape (batch, 2, {self.n}) or (2, {self.n})")
            one_, batch_ = x.ndim == 2, (1 if x.ndim == 2 else int(x.shape[0]))
            if host:
                x = self.to_device(x.reshape(batch_ * 2, self.n))
            else:
                if not x.is_contiguous():
                    raise TinyNttError(TN_EINVAL, f"{name}: need a contiguous tensor of {self.elem_bytes}-byte integers")
                self._dev_rows(x.reshape(batch_ * 2, self.n), name)
            return x, one_, batch_

        ev, one, batch = rows(ev, "ev")
        if od is not None:
            od, one_od, batch_od = rows(od, "od")
            if (one_od, batch_od) != (one, batch):
                raise ValueError("Expected od of the shape of ev")
        terms, g, rot = int(terms), int(galois), int(rot)
        if terms < 1:
            raise ValueError(f"Expected terms >= 1, got {terms}")
        if not 0 <= g < 2 ** 32:
            raise ValueError(f"Expected a Galois element below 2n = {2 * self.n}, got {g}")
        if not 0 <= rot < 2 ** 32:
            raise ValueError(f"Expected a rotation below 2n = {2 * self.n}, got {rot}")
        sets = self._sets(prepared, batch, 2 * terms, "key")
        c = out if out is not None else torch.empty((batch, 2, self.n), dtype=self.torch_dtype, device=ev.device)
        if not _is_torch(c) or c.numel() != batch * 2 * self.n or not c.is_contiguous():
            raise ValueError(f"Expected an output of {batch} x 2 rows of {self.n} coefficients")
        self._dev_rows(c.reshape(batch * 2, self.n), "out")
        _check(self._lib, self._lib.tn_poly_pack_step_prepared_dev(self._h, ev.data_ptr(), od.data_ptr() if od is not None else None, rot, g,
                                                                   prepared.tensor.data_ptr(), sets, c.data_ptr(), batch, terms, int(base_log),
                                                                   GADGET_BALANCED if balanced else 0, self._stream_ptr(stream)))
        return self._result(c.reshape(batch, 2, self.n) if host else c, host, one, out)

    def pack_lwes(self, lwe, keys: PreparedOperand, terms, base_log, balanced=False, stream=None):
        """LWE -> RLWE ring packing (PackLWEs and the field trace of Chen, Dai, Kim, Song, "Efficient Homomorphic Conversion Between
        (Ring) LWE Ciphertexts"): lwe is a device tensor (groups, count, n + 1), count a power of two <= n, LWE ciphertexts of
        dimension n under the coefficients of the ring key s.  Returns a device tensor (groups, 2, n): RLWE ciphertexts whose phase is
            n * sum_j mu_j X^(j n / count)   (plus noise),
        mu_j the phase of lwe[:, j].  THE FACTOR n IS NOT REMOVED: every automorphism step doubles the kept coefficients, log2 n
        steps in all.  A caller who wants sum_j mu_j X^(j n / count) scales the inputs (or the messages) by n^-1 mod q first, as the
        paper does; the library does not.
        keys: a PreparedOperand of log2(n) * 2 * terms rows; rows [(t - 1) * 2 * terms, t * 2 * terms), t = 1 .. log2 n, hold the
        key from sigma_g(s) to s for g = 2^t + 1 ([2][terms] prepared rows, poly_galois_keyswitch_prepared's layout), shared by every
        row.  All log2 n keys are needed for every count (numtheory.pack_elements lists k_t and g_t).
        The steps: the rows go slot-major (count, groups); lwe_embed at index 0; log2(count) poly_pack_step_prepared launches on
        halving batches (level t pairs the first half of the list with the second, rot = n / 2^t, g = 2^t + 1); then
        log2(n / count) trace launches (od=None).  Nothing synchronises; temporaries come from torch's allocator.
        stream: None (torch's current stream), a torch.cuda.Stream or a raw HIP stream handle; the library's launches are enqueued
        on it and the method's own torch work (the slot-major copy, every level's allocation and the release of the level before)
        runs under the same stream, so everything is ordered on it, as in Plan.bootstrap.  lwe and keys must be ready on that
        stream.  The plan's own stream ("plan") is refused: torch cannot run on it."""
        import torch
        if isinstance(stream, str):
            raise ValueError("pack_lwes: stream must be None, a torch.cuda.Stream or a raw stream handle (torch cannot run on the plan's own stream)")
        if stream is not None:
            ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=self.device)
            with torch.cuda.stream(ts):
                return self.pack_lwes(lwe, keys, terms, base_log, balanced, stream=None)
        self._own_prepared(keys, "pack_lwes", "key")
        if not _is_torch(lwe) or lwe.dim() != 3 or int(lwe.shape[2]) != self.n + 1:
            raise ValueError(f"Expected lwe as a device tensor of shape (groups, count, {self.n + 1})")
        groups, count, terms = int(lwe.shape[0]), int(lwe.shape[1]), int(terms)
        if count < 1 or count & (count - 1) or count > self.n or groups < 1:
            raise ValueError(f"Expected groups >= 1 and count a power of two between 1 and n = {self.n}, got {groups} and {count}")
        if terms < 1:
            raise ValueError(f"Expected terms >= 1, got {terms}")
        elements = numtheory.pack_elements(self.n)
        key = 2 * terms
        if keys.rows != len(elements) * key:
            raise ValueError(f"Expected keys of {len(elements)} x {key} rows, got {keys.rows}")
        slot_major = lwe.transpose(0, 1).contiguous().reshape(count * groups, self.n + 1)
        cur = self.lwe_embed(slot_major, 0, stream=stream)                    # (count * groups, 2, n): slot j at rows [j * groups, (j + 1) * groups)
        for t, (k, g) in enumerate(elements, start=1):
            level_key = PreparedOperand(self, keys.tensor[(t - 1) * key:t * key], key)
            rows = int(cur.shape[0])
            if rows > groups:                                                 # a pack level: the first half with the second
                half = rows // 2
                cur = self.poly_pack_step_prepared(cur[:half], cur[half:], k, g, level_key, terms, base_log, balanced, stream=stream)
            else:                                                             # a trace step
                cur = self.poly_pack_step_prepared(cur, None, 0, g, level_key, terms, base_log, balanced, stream=stream)
        return cur

    def lwe_keyswitch(self, lwe, ksk, n_out, terms, base_log, balanced=False, out=None, stream=None):
        """The LWE-to-LWE key switch (tn_lwe_keyswitch_dev): lwe is (batch, n_in + 1), ksk is (n_in, terms, n_out + 1) words of the
        plan's type, ksk[i][j] an LWE encryption of s_i 2^(j base_log) under the output key (a plain array, host values or a device
        tensor); returns (batch, n_out + 1) with out[r][k] = [k == n_out] b_r + sum_i sum_j digit_j(a_r[i]) ksk[i][j][k] mod q, the
        digits the gadget calls' (unsigned, or balanced).  n_in and n_out are independent of the plan's n.  Works on every plan."""
        x, host, one = self._lwe_in(lwe, "lwe")
        batch, n_in, n_out, terms = int(x.shape[0]), int(x.shape[1]) - 1, int(n_out), int(terms)
        if terms < 1 or n_out < 1:
            raise ValueError(f"Expected terms >= 1 and n_out >= 1, got {terms} and {n_out}")
        if _is_torch(ksk):
            k = ksk
            if not k.is_cuda or k.element_size() != self.elem_bytes or not k.is_contiguous():
                raise TinyNttError(TN_EINVAL, f"ksk: need a contiguous device tensor of {self.elem_bytes}-byte integers")
        else:
            k, _, _ = self._lwe_in(np.asarray(ksk).reshape(-1, n_out + 1), "ksk", n_out + 1)
        if k.numel() != n_in * terms * (n_out + 1):
            raise ValueError(f"Expected a key of shape ({n_in}, {terms}, {n_out + 1}), got {k.numel()} words")
        c = self._lwe_out(out, (batch, n_out + 1), x.device)
        _check(self._lib, self._lib.tn_lwe_keyswitch_dev(self._h, x.data_ptr(), k.data_ptr(), c.data_ptr(), batch, n_in, n_out, terms, int(base_log),
                                                         GADGET_BALANCED if balanced else 0, self._stream_ptr(stream)))
        return self._result(c, host, one, out)

    def lwe_ksk_prepared_bytes(self, n_in, n_out, terms):
        """The size in bytes of the prepared form of a key (n_in, terms, n_out + 1), padding included (tn_lwe_ksk_prepared_bytes)."""
        size = ctypes.c_size_t(0)
        _check(self._lib, self._lib.tn_lwe_ksk_prepared_bytes(self._h, int(n_in), int(n_out), int(terms), ctypes.byref(size)))
        return int(size.value)

    def lwe_ksk_prepare(self, ksk, terms, stream=None) -> PreparedLweKey:
        """Prepare an LWE key-switch key for the matrix cores (tn_lwe_ksk_prepare_dev): ksk is (n_in, terms, n_out + 1) words of
        the plan's type, host values or a device tensor of that shape (a plain key, as Plan.lwe_keyswitch takes it).  Returns a
        PreparedLweKey: signed-byte limbs of the centred residues in the matrix instruction's operand order, opaque, for
        Plan.lwe_keyswitch_prepared and Plan.bootstrap of THIS plan.  Works on every plan."""
        import torch
        terms = int(terms)
        shape = tuple(ksk.shape) if _is_torch(ksk) else np.shape(ksk)
        if len(shape) != 3 or shape[1] != terms or shape[2] < 2:
            raise ValueError(f"Expected a key of shape (n_in, {terms}, n_out + 1), got {tuple(shape)}")
        n_in, n_out = int(shape[0]), int(shape[2]) - 1
        if _is_torch(ksk):
            k = ksk
            if not k.is_cuda or k.element_size() != self.elem_bytes or not k.is_contiguous():
                raise TinyNttError(TN_EINVAL, f"ksk: need a contiguous device tensor of {self.elem_bytes}-byte integers")
        else:
            k, _, _ = self._lwe_in(np.asarray(ksk).reshape(-1, n_out + 1), "ksk", n_out + 1)
        prep = torch.empty(self.lwe_ksk_prepared_bytes(n_in, n_out, terms), dtype=torch.int8, device=k.device)
        _check(self._lib, self._lib.tn_lwe_ksk_prepare_dev(self._h, k.data_ptr(), prep.data_ptr(), n_in, n_out, terms, self._stream_ptr(stream)))
        return PreparedLweKey(self, prep, n_in, n_out, terms)

    def lwe_keyswitch_prepared(self, lwe, key: PreparedLweKey, base_log, balanced=False, out=None, stream=None):
        """Plan.lwe_keyswitch from a prepared key (tn_lwe_keyswitch_prepared_dev), bit for bit the same rows: lwe is
        (batch, key.n_in + 1), or one row, host values or a device tensor; returns (batch, key.n_out + 1).  Digits must fit a signed
        byte: base_log <= 7, or <= 8 with balanced digits; wider ones are Plan.lwe_keyswitch's.  Works on every plan."""
        if not isinstance(key, PreparedLweKey):
            raise TypeError("lwe_keyswitch_prepared: the key must come from Plan.lwe_ksk_prepare")
        if key.plan is not self:
            raise TinyNttError(TN_EINVAL, "lwe_keyswitch_prepared: the prepared key belongs to another plan")
        x, host, one = self._lwe_in(lwe, "lwe", key.n_in + 1)
        batch = int(x.shape[0])
        if key.tensor.numel() * key.tensor.element_size() < self.lwe_ksk_prepared_bytes(key.n_in, key.n_out, key.terms):
            raise TinyNttError(TN_EINVAL, "lwe_keyswitch_prepared: the prepared key is shorter than tn_lwe_ksk_prepared_bytes")
        c = self._lwe_out(out, (batch, key.n_out + 1), x.device)
        _check(self._lib, self._lib.tn_lwe_keyswitch_prepared_dev(self._h, x.data_ptr(), key.tensor.data_ptr(), c.data_ptr(), batch, key.n_in, key.n_out,
                                                                  key.terms, int(base_log), GADGET_BALANCED if balanced else 0,
                                                                  self._stream_ptr(stream)))
        return self._result(c, host, one, out)

    def bootstrap(self, lwe, bsk: PreparedOperand, test_vector, ksk, *, terms, base_log, ks_terms, ks_base_log, balanced=False, ks_balanced=False,
                  one_launch=False, stream=None):
        """A programmable bootstrap of LWE ciphertexts, LWE in and LWE under the same key out, from the library's calls alone:
          1. lwe_modswitch: exps (dim + 1, batch);
          2. the accumulator (X^exps[dim] * test_vector, 0) from monomial_mul;
          3. poly_blind_rotate_prepared when one_launch is set, else blind_rotate, over exps[:dim] with the bootstrap key bsk
             (dim * 4 * terms prepared rows: RGSW encryptions of the key bits, one per step);
          4. sample_extract at index 0: LWE of dimension n under the coefficients of the ring key;
          5. lwe_keyswitch with ksk (n, ks_terms, dim + 1) back to dimension dim; where ksk is a PreparedLweKey (lwe_ksk_prepare),
             lwe_keyswitch_prepared with it: the same rows from the matrix cores (ks_base_log within its byte-wide digits).
        lwe is (batch, dim + 1), host values or a device tensor; test_vector one polynomial of n words, host or device; ksk host
        or device words.  The two blind-rotation routes are bit-identical.  Which suits which batch (README, "Blind rotation"): one
        launch keeps the accumulator on chip and wins where the batch leaves workgroups to spare; the step-by-step loop reads
        each step's key once for the whole batch and is the route for large batches, and the only one where the accumulator does
        not fit a workgroup's LDS (n = 8192 with 64-bit words).  Nothing synchronises between the steps.  stream: None (torch's
        current stream), a torch.cuda.Stream or a raw HIP stream handle; the library's calls are enqueued on it and the method's
        own torch work (the intermediates' allocations, the zero fill of the accumulator, the copy of the test vector) runs under
        the same stream, so everything is ordered on it.  The plan's own stream ("plan") is refused: torch cannot run on it.
        Returns (batch, dim + 1), a host array where lwe came from the host."""
        import torch
        if isinstance(stream, str):
            raise ValueError("bootstrap: stream must be None, a torch.cuda.Stream or a raw stream handle (torch cannot run on the plan's own stream)")
        if stream is not None:
            ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream), device=self.device)
            with torch.cuda.stream(ts):
                return self.bootstrap(lwe, bsk, test_vector, ksk, terms=terms, base_log=base_log, ks_terms=ks_terms, ks_base_log=ks_base_log,
                                      balanced=balanced, ks_balanced=ks_balanced, one_launch=one_launch, stream=None)
        self._own_prepared(bsk, "bootstrap", "bootstrap key")
        x, host, one = self._lwe_in(lwe, "lwe")
        batch, dim = int(x.shape[0]), int(x.shape[1]) - 1
        if bsk.rows != dim * 4 * int(terms):
            raise ValueError(f"Expected a bootstrap key of {dim} x {4 * int(terms)} rows, got {bsk.rows}")
        tv = test_vector if _is_torch(test_vector) else self.to_device(np.asarray(test_vector).reshape(1, self.n))
        if self._dev_rows(tv.reshape(1, self.n) if tv.numel() == self.n else tv, "test_vector") != 1:
            raise ValueError(f"Expected a test vector of {self.n} coefficients")
        exps = self.lwe_modswitch(x, stream=stream)
        tvs = torch.zeros((batch, 2, self.n), dtype=self.torch_dtype, device=x.device)
        tvs[:, 0] = tv.reshape(self.n)
        acc = self.monomial_mul(tvs, exps[dim], stream=stream)
        if one_launch:
            acc = self.poly_blind_rotate_prepared(acc, exps[:dim], bsk, terms, base_log, balanced, out=acc, stream=stream)
        else:
            acc = self.blind_rotate(acc, exps[:dim], bsk, terms, base_log, balanced, stream=stream)
        big = self.sample_extract(acc, 0, stream=stream)
        if isinstance(ksk, PreparedLweKey):
            if (ksk.n_in, ksk.n_out, ksk.terms) != (self.n, dim, int(ks_terms)):
                raise ValueError(f"Expected a prepared key of shape ({self.n}, {int(ks_terms)}, {dim + 1}), got ({ksk.n_in}, {ksk.terms}, {ksk.n_out + 1})")
            c = self.lwe_keyswitch_prepared(big, ksk, ks_base_log, ks_balanced, stream=stream)
        else:
            c = self.lwe_keyswitch(big, ksk, dim, ks_terms, ks_base_log, ks_balanced, stream=stream)
        return self._result(c, host, one)

    # ---- ring automorphisms a(x) -> a(x^g) ----------------------------------------
    @staticmethod
    def _galois(galois):
        """galois, an int or a sequence of ints -> (ctypes uint32 array, count, one element was given).  Values the C ABI's
        uint32 cannot hold are refused here; evenness and the range [1, 2n) are the library's to check."""
        one = isinstance(galois, (int, np.integer))
        vals = [int(galois)] if one else [int(g) for g in galois]
        if any(g < 0 or g >= 2 ** 32 for g in vals):
            raise ValueError("Galois elements must be odd integers in [1, 2n)")
        return (ctypes.c_uint32 * max(len(vals), 1))(*vals), len(vals), one

    def _images(self, out, batch, count, device):
        """out, or a new tensor on `device`: batch x count rows of the plan's words, contiguous."""
        import torch
        c = out if out is not None else torch.empty((batch, count, self.n), dtype=self.torch_dtype, device=device)
        if not _is_torch(c) or c.numel() != batch * count * self.n or not c.is_contiguous() or c.shape[-1] != self.n:
            raise ValueError(f"Expected an output of {batch} x {count} rows of {self.n} coefficients")
        self._dev_rows(c.reshape(batch * count, self.n), "out")
        return c

    def automorphism(self, a, galois, out=None, stream=None):
        """sigma_g(a[r]) = a[r](x^g) mod (x^n + 1) for every Galois element g given (tn_automorphism_dev; include/tinyntt.h has
        the definition): a is (batch, n) or (n,), host values (taken mod q) or a device tensor of any words; galois is an odd
        int in [1, 2n) or a sequence of up to GALOIS_MAX of them.  Returns canonical residues, (batch, n) for an int and
        (batch, count, n) for a sequence, one read of a for all of them.  Works on every plan."""
        a, batch, host, one = self._rows_in(a)
        gl, count, single = self._galois(galois)
        c = self._images(out, batch, count, a.device)
        _check(self._lib, self._lib.tn_automorphism_dev(self._h, a.data_ptr(), c.data_ptr(), batch, gl, count, self._stream_ptr(stream)))
        if out is None:
            c = c.reshape(batch, self.n) if single else c.reshape(batch, count, self.n)
        return self._result(c, host, one, out)

    def automorphism_prepared(self, prepared: PreparedOperand, galois, out=None, stream=None) -> PreparedOperand:
        """The prepared form of sigma_g of the polynomials `prepared` holds (tn_automorphism_prepared_dev): a permutation of words
        in the transform domain, no transform runs.  Returns a PreparedOperand of rows * count rows, row r's image under element
        m at row r * count + m; word for word prepare(automorphism(unprepare(prepared), galois))."""
        self._own_prepared(prepared, "automorphism_prepared", "operand")
        gl, count, _ = self._galois(galois)
        rows = prepared.rows
        if isinstance(out, PreparedOperand):      # written in place of a new tensor: this plan's, rows * count rows
            self._own_prepared(out, "automorphism_prepared", "output")
            if out.rows != rows * count:
                raise ValueError(f"Expected an output of {rows} x {count} rows of {self.n} coefficients")
            out = out.tensor
        c = self._images(out, rows, count, prepared.tensor.device)
        _check(self._lib, self._lib.tn_automorphism_prepared_dev(self._h, prepared.tensor.data_ptr(), c.data_ptr(), rows, gl, count,
                                                                 self._stream_ptr(stream)))
        return PreparedOperand(self, c.reshape(rows * count, self.n), rows * count)

    def cyclic_poly_mult(self, a, b, variant="auto", out=None, stream=None):
        """Untwisted product forward->pointwise->inverse: python_poly_mult (test_ntt_poly_mult.py:38-43)."""
        return self._binary_dev(self._lib.tn_cyclic_poly_mult_dev, a, b, out, stream, _variant(variant))

    def pointwise_mul(self, a, b, out=None, stream=None):
        """c[i] = a[i]*b[i] mod q (cg_ntt.py:88; benchmark_ntt_60bit.cpp:142-146)."""
        return self._binary_dev(self._lib.tn_pointwise_mul_dev, a, b, out, stream)

    def schoolbook(self, a, b, out=None, stream=None):
        """O(n^2) direct negacyclic product on device (benchmark_ntt_60bit.cpp:167-180): independent checker."""
        return self._binary_dev(self._lib.tn_schoolbook_dev, a, b, out, stream)

    TABLES = {"psi_pow": 0, "psi_inv_ninv": 1, "omega_pow": 2, "omega_inv_pow": 3, "psi_brv": 4, "psi_inv_brv": 5, "psi_inv_pow": 6}

    def export_table(self, which) -> np.ndarray:
        """One of the plan's device tables as uint64 values (see tn_plan_export_table)."""
        w = self.TABLES[which] if isinstance(which, str) else int(which)
        out = np.empty(self.n // 2 if w in (2, 3) else self.n, dtype=np.uint64)
        _check(self._lib, self._lib.tn_plan_export_table(self._h, w, out.ctypes.data))
        return out

    def _ntt(self, fn_dev, fn_host, x, variant, out, stream):
        v = _variant(variant)
        if _is_torch(x):
            import torch
            rows = self._dev_rows(x, "in")
            y = out if out is not None else torch.empty_like(x)
            _check(self._lib, fn_dev(self._h, x.data_ptr(), y.data_ptr(), rows, v, self._stream_ptr(stream)))
            return y
        squeeze = np.ndim(x) == 1
        hx = self._host_rows(x, "in")
        hy = np.empty_like(hx)
        _check(self._lib, fn_host(self._h, hx.ctypes.data, hy.ctypes.data, hx.shape[0], v))
        return hy[0] if squeeze else hy

    def ntt_forward(self, x, variant="auto", out=None, stream=None):
        """cg_ntt(x, omega=psi^2) (cg_ntt.py:29-65): untwisted, natural order in and out.
        variant "auto"/"fused": register-tiled kernel; "cg"/"cg8"/"cg8_padded": the reference's stage sweep."""
        return self._ntt(self._lib.tn_ntt_forward_dev, self._lib.tn_ntt_forward_host, x, variant, out, stream)

    def ntt_inverse(self, x, variant="auto", out=None, stream=None):
        """cg_intt(x, omega=psi^2) (cg_ntt.py:68-75)."""
        return self._ntt(self._lib.tn_ntt_inverse_dev, self._lib.tn_ntt_inverse_host, x, variant, out, stream)

    def twisted_ntt_forward(self, x, variant="auto", out=None, stream=None):
        """twist + forward: forward_ntt_bench (benchmark_ntt_60bit.cpp:161-165).  Device tensors only."""
        if not _is_torch(x):
            import torch
            t = torch.from_numpy(self._host_rows(x, "in").view(np.int32 if self.elem_bytes == 4 else np.int64)).to(f"cuda:{self.device}")
            y = self._ntt(self._lib.tn_twisted_ntt_forward_dev, None, t, variant, None, None)
            self.synchronize()
            res = y.cpu().numpy().view(self.dtype)
            return res[0] if np.ndim(x) == 1 else res
        return self._ntt(self._lib.tn_twisted_ntt_forward_dev, None, x, variant, out, stream)

    def ntt_forward_trace(self, x, variant="cg"):
        """Forward transform of one polynomial plus every stage's output ([log2 n][n]),
        the lists cg_ntt(..., verbose=True) prints (cg_ntt.py:60-62)."""
        hx = self._host_rows(x, "in")
        if hx.shape[0] != 1:
            raise ValueError("ntt_forward_trace takes one polynomial")
        out = np.empty_like(hx)
        trace = np.empty((self.logn, self.n), dtype=self.dtype)
        _check(self._lib, self._lib.tn_ntt_forward_trace_host(self._h, hx.ctypes.data, out.ctypes.data, trace.ctypes.data, _variant(variant)))
        return out[0], trace

    # ---- synthetic data + digests (reference benchmark conventions) -------------
    def fill_lcg(self, batch: int, seed0: int = 1, seed_stride: int = 2, out=None, stream=None):
        """Device tensor whose row r is make_poly(seed0 + r*seed_stride) (benchmark_ntt_60bit.cpp:79-87)."""
        import torch
        t = out if out is not None else torch.empty((batch, self.n), dtype=self.torch_dtype, device=f"cuda:{self.device}")
        _check(self._lib, self._lib.tn_fill_lcg_dev(self._h, t.data_ptr(), batch, seed0 % 2 ** 64, seed_stride % 2 ** 64, self._stream_ptr(stream)))
        return t

    def checksum_rows(self, t, stream=None):
        """Per-row checksum (benchmark_ntt_60bit.cpp:182-188) as a numpy uint64 array."""
        import torch
        rows = self._dev_rows(t, "src")
        out = torch.empty((rows,), dtype=torch.int64, device=t.device)
        _check(self._lib, self._lib.tn_checksum_rows_dev(self._h, t.data_ptr(), out.data_ptr(), rows, self._stream_ptr(stream)))
        self.synchronize()
        return out.cpu().numpy().view(np.uint64)      # .cpu() waits on the current stream

    def time_poly_mult(self, a, b, c, iters: int, variant="auto") -> float:
        """Mean ms per launch over `iters` launches, HIP events on the plan's stream."""
        import torch
        rows = self._dev_rows(a, "a")
        torch.cuda.synchronize(self.device)            # inputs may have been produced on torch's stream
        ms = ctypes.c_float()
        _check(self._lib, self._lib.tn_time_poly_mult_dev(self._h, a.data_ptr(), b.data_ptr(), c.data_ptr(), rows, _variant(variant), iters, ctypes.byref(ms)))
        return float(ms.value)

    def kernel_name(self, variant="auto") -> str:
        return self._lib.tn_kernel_name(self._h, _variant(variant)).decode()

    def synchronize(self):
        _check(self._lib, self._lib.tn_plan_synchronize(self._h))

    def to_host(self, t) -> np.ndarray:
        """Device tensor -> numpy array of the plan's unsigned dtype."""
        self.synchronize()
        return t.cpu().numpy().view(self.dtype)       # .cpu() waits on the current stream

    def to_device(self, arr):
        import torch
        h = self._host_rows(arr, "arr")
        return torch.from_numpy(h.view(np.int32 if self.elem_bytes == 4 else np.int64)).to(f"cuda:{self.device}")


class MultiPlan:
    """tn_multi_*: one host call sharded over several devices in contiguous row blocks, each entry with its own plan and stream
    (no collective).  devices=None: every visible device; a device may be listed several times."""

    def __init__(self, n: int, q: int, psi: int, devices=None, flags: int = 0):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        arr = (ctypes.c_int * len(devices))(*devices) if devices is not None else None
        st = self._lib.tn_multi_create(ctypes.byref(self._h), int(n), int(q), int(psi) % int(q), arr, len(devices) if devices is not None else 0, int(flags))
        _check(self._lib, st, self._lib.tn_multi_last_error)
        self.n, self.q, self.psi = int(n), int(q), int(psi) % int(q)
        self.size = int(self._lib.tn_multi_size(self._h))
        self.devices = [int(self._lib.tn_multi_device(self._h, i)) for i in range(self.size)]
        self.elem_bytes = int(self._lib.tn_plan_elem_bytes(self._lib.tn_multi_plan(self._h, 0)))
        self.dtype = np.uint32 if self.elem_bytes == 4 else np.uint64

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.tn_multi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shard(self, batch: int, index: int):
        """(first_row, rows) of entry `index` (tn_shard_rows)."""
        f, r = ctypes.c_size_t(), ctypes.c_size_t()
        _check(self._lib, self._lib.tn_shard_rows(int(batch), self.size, int(index), ctypes.byref(f), ctypes.byref(r)))
        return int(f.value), int(r.value)

    def poly_mult(self, a, b, variant="auto"):
        """Host arrays [batch, n] -> [batch, n]: tn_multi_poly_mult_host."""
        ha = np.ascontiguousarray(a, dtype=self.dtype); hb = np.ascontiguousarray(b, dtype=self.dtype)
        if ha.ndim != 2 or ha.shape != hb.shape or ha.shape[1] != self.n:
            raise ValueError(f"Expected {self.n} coefficients")
        hc = np.empty_like(ha)
        st = self._lib.tn_multi_poly_mult_host(self._h, ha.ctypes.data, hb.ctypes.data, hc.ctypes.data, ha.shape[0], _variant(variant))
        _check(self._lib, st, self._lib.tn_multi_last_error)
        return hc


_plan_cache = {}


def _cached_plan(key, make) -> Plan:
    p = _plan_cache.get(key)
    if p is None:
        p = _plan_cache[key] = make()
    return p


def get_plan(n: int, q: int, psi: int, device: int = 0, flags: int = 0) -> Plan:
    key = (int(n), int(q), int(psi) % int(q), int(device), int(flags))
    return _cached_plan(key, lambda: Plan(*key))


def get_omega_plan(n: int, q: int, omega: int, device: int = 0) -> Plan:
    """Cached omega-only plan: the transforms cg_ntt(a, omega_n, modulus) / cg_intt for any omega_n (cg_ntt.py:29-75)."""
    key = ("omega", int(n), int(q), int(omega) % int(q), int(device))
    return _cached_plan(key, lambda: Plan(int(n), int(q), 0, int(device), 0, omega=int(omega)))


def get_general_plan(n: int, q: int, psi: int, device: int = 0) -> Plan:
    """Cached general plan (tn_plan_create_general): nwc_poly_mult for any psi_2n / modulus, as cg_ntt.py:78-92 computes it."""
    key = ("general", int(n), int(q), int(psi) % int(q), int(device))
    return _cached_plan(key, lambda: Plan(int(n), int(q), int(psi), int(device), 0, general=True))


def get_poly_plan(n: int, q: int, psi: int, device: int = 0) -> Plan:
    """The plan the reference-shaped entry points use: the validated one (throughput kernels) when (q, psi) admit it,
    else the general one — the reference validates neither (cg_ntt.py:78-92)."""
    try:
        return get_plan(n, q, psi, device)
    except TinyNttError as e:
        if e.status != TN_EBADPARAM:
            raise
    return get_general_plan(n, q, psi, device)


def clear_plan_cache():
    for p in _plan_cache.values():
        p.close()
    _plan_cache.clear()
