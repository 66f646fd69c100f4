"""ctypes binding of libswd_hip.so (C ABI: include/swd.h).

There is no CPU fallback: if the HIP library is missing or no MI355X is visible, construction of
any decoder raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported
from this package.)
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("SWD_LIB", "libswd_hip.so"))  # SWD_LIB: a development build next to it
_lib = None


class GraphDesc(C.Structure):
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("nnz", C.c_int32),
                ("row_ptr", C.c_void_p), ("col_idx", C.c_void_p), ("channel_probs", C.c_void_p)]


class WindowDesc(C.Structure):
    _fields_ = [("graph", GraphDesc), ("row0", C.c_int32), ("col0", C.c_int32), ("commit", C.c_int32),
                ("reserved", C.c_int32)]


class OsdwParams(C.Structure):
    _fields_ = [("pre_max_iter", C.c_int32), ("post_max_iter", C.c_int32),
                ("ms_scaling_factor", C.c_double), ("new_n", C.c_int32),
                ("osd_method", C.c_int32), ("osd_order", C.c_int32)]


class GdgParams(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("ms_scaling_factor", C.c_double), ("max_iter_per_step", C.c_int32),
                ("max_step", C.c_int32), ("max_tree_depth", C.c_int32), ("max_side_depth", C.c_int32),
                ("max_tree_branch_step", C.c_int32), ("max_side_branch_step", C.c_int32),
                ("gdg_factor", C.c_double), ("new_n", C.c_int32), ("low_error_mode", C.c_int32),
                ("mode", C.c_int32), ("multi_thread", C.c_int32)]


class Bp4Params(C.Structure):
    _fields_ = [("max_iter", C.c_int32), ("ms_scaling_factor", C.c_double), ("osd_method", C.c_int32),
                ("osd_order", C.c_int32)]


# every symbol include/swd.h declares: (name, restype, argtypes)
_vp, _i32, _i64, _dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
SYMBOLS = [
    ("swd_last_error", C.c_char_p, []),
    ("swd_last_error_class", C.c_int, []),
    ("swd_abi_version", C.c_int, []),
    ("swd_device_count", C.c_int, []),
    ("swd_osdw_create", _vp, [C.POINTER(GraphDesc), C.POINTER(OsdwParams), C.c_int]),
    ("swd_osdw_destroy", None, [_vp]),
    ("swd_osdw_info", C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    ("swd_osdw_decode_batch", C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    ("swd_osdw_decode_batch_dev", C.c_int, [_vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    ("swd_osdw_set_timing", C.c_int, [_vp, _i32]),
    ("swd_osdw_get_timing", C.c_int, [_vp, C.POINTER(_dbl), C.POINTER(_i64)]),
    ("swd_gdg_create", _vp, [C.POINTER(GraphDesc), C.POINTER(GdgParams), C.c_int]),
    ("swd_gdg_destroy", None, [_vp]),
    ("swd_gdg_decode_batch", C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32]),
    ("swd_gdg_decode_batch_dev", C.c_int, [_vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp]),
    ("swd_bp4_create", _vp, [C.POINTER(GraphDesc), C.POINTER(GraphDesc), _vp, _vp, _vp, C.POINTER(Bp4Params), C.c_int]),
    ("swd_bp4_create_ex", _vp, [C.POINTER(GraphDesc), C.POINTER(GraphDesc), _vp, _vp, _vp, C.POINTER(Bp4Params), C.c_int, _i32]),
    ("swd_bp4_is_general", C.c_int, [_vp]),
    ("swd_bp4_is_general_osd", C.c_int, [_vp]),
    ("swd_bp4_destroy", None, [_vp]),
    ("swd_bp4_info", C.c_int, [_vp] + [C.POINTER(_i32)] * 5),
    ("swd_bp4_heavy_info", C.c_int, [_vp] + [C.POINTER(_i32)] * 2),
    ("swd_bp4_last_form", C.c_int, [_vp] + [C.POINTER(_i32)] * 8),
    ("swd_bp4_decode_batch", C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("swd_bp4_decode_batch_dev", C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("swd_bp4_camel_decode_batch", C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    ("swd_bp4_camel_decode_batch_dev", C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("swd_pipeline_create_gdg", _vp, [_i32, _vp, C.POINTER(GraphDesc), C.POINTER(GdgParams), C.c_int]),
    ("swd_pipeline_create", _vp, [_i32, _vp, C.POINTER(GraphDesc), C.POINTER(OsdwParams), C.c_int]),
    ("swd_pipeline_destroy", None, [_vp]),
    ("swd_pipeline_info", C.c_int, [_vp] + [C.POINTER(_i32)] * 5),
    ("swd_pipeline_set_observables", C.c_int, [_vp, C.POINTER(GraphDesc)]),
    ("swd_pipeline_decode", C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    ("swd_pipeline_decode_dev", C.c_int, [_vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    ("swd_pipeline_decode_packed", C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    ("swd_pipeline_stream_create", _vp, [_vp, _i32, _i32]),
    ("swd_pipeline_stream_destroy", None, [_vp]),
    ("swd_pipeline_stream_push", C.c_int, [_vp, _i32, _vp]),
    ("swd_pipeline_stream_pop", C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("swd_pipeline_stream_pending", C.c_int, [_vp]),
    ("swd_pipeline_stream_push_dev", C.c_int, [_vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    ("swd_pipeline_stream_wait", C.c_int, [_vp, _vp]),
    ("swd_pipeline_stream_wait_last", C.c_int, [_vp, _vp]),
    ("swd_window_loop_create", _vp, [_i32, _vp, C.POINTER(GraphDesc), C.POINTER(GraphDesc), _i32, _vp, C.c_int]),
    ("swd_window_loop_destroy", None, [_vp]),
    ("swd_window_loop_info", C.c_int, [_vp] + [C.POINTER(_i32)] * 4 + [C.POINTER(_i64)]),
    ("swd_window_loop_decode_dev", C.c_int, [_vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    ("swd_window_loop_decode", C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    ("swd_pipeline_session_create", _vp, [_vp, _i32]),
    ("swd_pipeline_session_destroy", None, [_vp]),
    ("swd_pipeline_session_begin", C.c_int, [_vp, _i32]),
    ("swd_pipeline_session_push", C.c_int, [_vp, _i32, _vp, C.POINTER(_i32), C.POINTER(_i32)]),
    ("swd_pipeline_session_push_dev", C.c_int, [_vp, _i32, _vp, _i64, C.POINTER(_i32), C.POINTER(_i32), _vp]),
    ("swd_pipeline_session_window", C.c_int, [_vp, _i32, _vp, _vp, _vp]),
    ("swd_pipeline_session_finish", C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("swd_pipeline_session_buffers", C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i32)]),
    ("swd_pipeline_rolling_create", _vp, [_vp, _i32]),
    ("swd_pipeline_rolling_destroy", None, [_vp]),
    ("swd_pipeline_rolling_begin", C.c_int, [_vp, _i32]),
    ("swd_pipeline_rolling_push", C.c_int, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i32)]),
    ("swd_pipeline_rolling_push_dev", C.c_int, [_vp, _i32, _vp, _i64, _i32, _vp, _vp, _vp, C.POINTER(_i64), C.POINTER(_i32), _vp]),
    ("swd_pipeline_rolling_finish", C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    ("swd_pipeline_rolling_finish_dev", C.c_int, [_vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    ("swd_pipeline_rolling_state", C.c_int, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i64)]),
    ("swd_frontend_create", _vp, [C.POINTER(GraphDesc)] * 4 + [_i32, _i32, _i32, _i32, C.c_int]),
    ("swd_frontend_destroy", None, [_vp]),
    ("swd_frontend_begin", C.c_int, [_vp, _i32]),
    ("swd_frontend_state", C.c_int, [_vp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i32), C.POINTER(_i64)]),
    ("swd_frontend_push_dev", C.c_int, [_vp, _i32, _vp, _i64, _i32, _vp, _i64, C.POINTER(_i32), _vp]),
    ("swd_frontend_finish_dev", C.c_int, [_vp, _i32, _vp, _i64, _i32, _vp, _i64, C.POINTER(_i32), _vp, _vp]),
    ("swd_frontend_push", C.c_int, [_vp, _i32, _vp, _i32, _vp, C.POINTER(_i32)]),
    ("swd_frontend_finish", C.c_int, [_vp, _i32, _vp, _i32, _vp, C.POINTER(_i32), _vp]),
    ("swd_pipeline_status", C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    ("swd_pipeline_set_profiling", C.c_int, [_vp, _i32]),
    ("swd_pipeline_get_profile", C.c_int, [_vp, _i32, _vp]),
    ("swd_pipeline_set_timing", C.c_int, [_vp, _i32]),
    ("swd_pipeline_get_timing", C.c_int, [_vp, C.POINTER(_dbl), C.POINTER(_i64)]),
    ("swd_sampler_create", _vp, [C.POINTER(GraphDesc), C.POINTER(GraphDesc), C.c_int]),
    ("swd_sampler_destroy", None, [_vp]),
    ("swd_sampler_info", C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    ("swd_sampler_sample", C.c_int, [_vp, _i32, C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    ("swd_sampler_sample_dev", C.c_int, [_vp, _i32, C.c_uint64, C.c_uint64, _vp, _i64, _vp, _vp, _i64, _vp]),
    ("swd_rolling_sampler_create", _vp, [C.POINTER(GraphDesc), C.POINTER(GraphDesc), _i32, _i32, _i32, _vp, _i32, C.c_int]),
    ("swd_rolling_sampler_destroy", None, [_vp]),
    ("swd_rolling_sampler_info", C.c_int, [_vp, C.POINTER(_i32), _i32, _i32, _i32, C.POINTER(_i64), C.POINTER(_i64)]),
    ("swd_rolling_sampler_rows_dev", C.c_int, [_vp, _i32, C.c_uint64, C.c_uint64, _i32, _i32, _i32, _vp, _i64, _vp, _vp, _i64, _vp]),
    ("swd_rolling_sampler_rows", C.c_int, [_vp, _i32, C.c_uint64, C.c_uint64, _i32, _i32, _i32, _vp, _vp, _vp]),
    ("swd_circuit_sampler_create", _vp, [_i32] + [_vp] * 7 + [_i32, _i32, C.POINTER(GraphDesc), C.POINTER(GraphDesc), _i32, C.c_int]),
    ("swd_circuit_sampler_destroy", None, [_vp]),
    ("swd_circuit_sampler_info", C.c_int, [_vp, C.POINTER(_i64)]),
    ("swd_circuit_sampler_measure_dev", C.c_int, [_vp, _i32, C.c_uint64, C.c_uint64, _vp, _i64, _i32, _vp]),
    ("swd_circuit_sampler_sample_dev", C.c_int, [_vp, _i32, C.c_uint64, C.c_uint64, _vp, _i64, _vp, _vp, _i64, _vp]),
    ("swd_circuit_sampler_measure", C.c_int, [_vp, _i32, C.c_uint64, C.c_uint64, _vp, _i32]),
    ("swd_circuit_sampler_sample", C.c_int, [_vp, _i32, C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    ("swd_pauli_sampler_create", _vp, [C.POINTER(GraphDesc), C.POINTER(GraphDesc), _vp, _vp, _vp, C.c_int]),
    ("swd_pauli_sampler_destroy", None, [_vp]),
    ("swd_pauli_sampler_info", C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    ("swd_pauli_sampler_sample", C.c_int, [_vp, _i32, C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    ("swd_pauli_sampler_sample_dev", C.c_int, [_vp, _i32, C.c_uint64, C.c_uint64, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    ("swd_css_account_create", _vp, [C.POINTER(GraphDesc), _i32, C.POINTER(GraphDesc), _i32, C.c_int]),
    ("swd_css_account_destroy", None, [_vp]),
    ("swd_css_account_dev", C.c_int, [_vp, _i32, _vp, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _vp]),
    ("swd_shot_account_dev", C.c_int, [C.c_int, _i32, _i32, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _vp, _vp, _i32, _vp]),
    ("swd_group_account_dev", C.c_int, [C.c_int, _i32, _vp, _vp, _i32, _vp, _vp, _vp]),
    ("swd_diag_occupy",C.c_int, [C.c_int, _i32, _i32, _i32, _i32, _vp]),
    ("swd_diag_libm", C.c_int, [C.c_int, _i32, _i64, _vp, _vp, _vp, _vp]),
    ("swd_graph_layout", C.c_int, [C.POINTER(GraphDesc), _i32] + [_vp] * 9),
    ("swd_graph_node_depth", C.c_int, [C.POINTER(GraphDesc), _i32, _i32, _i32, _vp] + [_vp] * 6),
    ("swd_graph_cache_image", C.c_int, [C.POINTER(GraphDesc), _i32, _i32, _i32, _i32, _i32, _vp] + [_vp] * 7),
    ("swd_osdw_node_depth", C.c_int, [_vp]),
    ("swd_pipeline_node_depth", C.c_int, [_vp]),
    ("swd_window_forms", C.c_int, [_i32, _vp, _i32, C.POINTER(OsdwParams), C.POINTER(GdgParams), _vp, _vp]),
    ("swd_osdw_last_form", C.c_int, [_vp, _vp, _vp]),
    ("swd_gdg_last_form", C.c_int, [_vp, _vp, _vp]),
    ("swd_pipeline_last_form", C.c_int, [_vp, _vp, _vp]),
]
FORM_PLAN_WORDS = FORM_WINDOW_WORDS = 16  # include/swd.h: SWD_FORM_PLAN_WORDS, SWD_FORM_WINDOW_WORDS

STAT_WORDS = 8
WINDOW_COUNTER_WORDS = 10  # include/swd.h: SWD_WINDOW_COUNTER_WORDS
MAX_OBSERVABLE_GROUPS = 4  # include/swd.h: SWD_MAX_OBSERVABLE_GROUPS
FRONTEND_STAGE_BYTES = 32768  # include/swd.h, swd_frontend_create: what one launch of the front end stages
STREAM_PACKED,STREAM_NO_STATS = 1, 2
STREAM_NO_DEPENDENCY = C.c_void_p(-1).value  # include/swd.h: SWD_STREAM_NO_DEPENDENCY


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  Two HIP runtimes in
    one process do not share a device context (the second one to initialise sees 0 devices), so
    when torch is installed its copy is loaded first with RTLD_GLOBAL and libswd_hip.so binds to
    it by SONAME; torch tensors' data_ptr()s and streams are then valid in our launches."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    libdir = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def lib():
    """Load libswd_hip.so; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C slidingwindowdecoder_amd/csrc). "
                "This package has no CPU fallback.")
        _preload_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            f = getattr(L, name, None)
            if f is None:
                if os.environ.get("SWD_LIB"):  # a development / bisect build may predate a symbol
                    continue
                raise RuntimeError(f"{LIB_PATH} does not export {name}: rebuild it")
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    return (lib().swd_last_error() or b"").decode()


ERR_FAILED, ERR_VALUE, ERR_CAPACITY, ERR_DEVICE = range(4)  # include/swd.h: enum swd_error_class


def last_error_class() -> int:
    return lib().swd_last_error_class()


class CapacityError(ValueError, RuntimeError):
    """The input is valid but beyond a bound of the form that was asked (include/swd.h, SWD_ERR_CAPACITY): this build's graph
    tables, the kernel variants, a workgroup's LDS, a general form's own limit.  Both bases on purpose: such refusals used to
    arrive as ValueError from one constructor and as RuntimeError from another."""


def error(name, prefix_value=False):
    """The exception for the failure the calling thread's last library call reported -- the one place that turns the library's
    message and class into a Python exception.  ``name``: the entry point that failed.  SWD_ERR_VALUE: ValueError with the
    bare message (``prefix_value``: with the ``name failed:`` prefix too); SWD_ERR_CAPACITY: CapacityError; anything else:
    RuntimeError."""
    msg, cls = last_error(), last_error_class()
    if cls == ERR_VALUE and not prefix_value:
        return ValueError(msg)
    return {ERR_VALUE: ValueError, ERR_CAPACITY: CapacityError}.get(cls, RuntimeError)(f"{name} failed: {msg}")
