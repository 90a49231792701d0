"""ctypes binding of libsavad.so (C ABI: include/savad.h).  Fails loudly: there is no CPU
fallback in the product path -- if the HIP library is missing or stale, importing it raises."""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_long, c_size_t, c_void_p
from pathlib import Path

_PKG = Path(__file__).resolve().parent
import os

LIB_PATH = Path(os.environ.get("SAVAD_LIB", _PKG / "libsavad.so"))  # override only for kernel experiments


class SavadError(RuntimeError):
    pass


class savad_config(ctypes.Structure):
    _fields_ = [("feature_size", c_int32), ("num_layers", c_int32), ("d_model", c_int32)]


class savad_frontend_config(ctypes.Structure):
    _fields_ = [("transform", c_int32), ("n_fft", c_int32), ("hop", c_int32), ("win", c_int32), ("n_mels", c_int32),
                ("n_mfcc", c_int32), ("deltas", c_int32)]


class savad_live_config(ctypes.Structure):
    _fields_ = [("streams", c_int32), ("max_push_samples", c_int32), ("half", c_int32), ("jump", c_int32), ("chunk", c_int32)]


class savad_live_slot(ctypes.Structure):
    _fields_ = [("n_samples", c_int64), ("base", c_int64), ("open", c_int32), ("phase", c_int32)]


class savad_live_push(ctypes.Structure):
    _fields_ = [("slot", c_int32), ("n_samples", c_int32), ("dtype", c_int32), ("finish", c_int32), ("data", c_void_p)]


class savad_live_counts(ctypes.Structure):
    _fields_ = [("entries", c_int32), ("tiles", c_int32), ("items", c_int32), ("rows", c_int32), ("table_bytes", c_int32), ("W", c_int32)]


class savad_live_event(ctypes.Structure):
    _fields_ = [("sample", c_int64), ("slot", c_int32), ("kind", c_int32)]


class savad_live_post_config(ctypes.Structure):
    _fields_ = [("W", c_int32), ("threshold", c_float), ("min_vally", c_int32), ("min_hill", c_int32), ("hang_before", c_int32),
                ("hang_over", c_int32)]


# every symbol include/savad.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "savad_create": (c_int, [POINTER(savad_config), POINTER(c_void_p)]),
    "savad_destroy": (None, [c_void_p]),
    "savad_set_param": (c_int, [c_void_p, c_char_p, c_void_p, c_size_t, c_void_p]),
    "savad_num_params": (c_int, [c_void_p]),
    "savad_param_key": (c_char_p, [c_void_p, c_int]),
    "savad_param_numel": (c_size_t, [c_void_p, c_int]),
    "savad_reserve": (c_int, [c_void_p, c_int, c_void_p]),
    "savad_workspace_bytes": (c_int, [c_void_p, c_int, c_int, POINTER(c_size_t)]),
    "savad_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "savad_set_precision": (c_int, [c_void_p, c_int]),
    "savad_residual_saturations": (c_int, [c_void_p, POINTER(ctypes.c_ulonglong), c_void_p]),
    "savad_forward_ex": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "savad_forward_strided": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_long, c_void_p, c_void_p, c_size_t, c_void_p]),
    "savad_set_attention_splits": (c_int, [c_void_p, c_int]),
    "savad_set_row_mode": (c_int, [c_void_p, c_int]),
    "savad_set_batch_invariant": (c_int, [c_void_p, c_int]),
    "savad_set_profiling": (c_int, [c_void_p, c_int]),
    "savad_profiling_skip": (c_int, [c_void_p, c_int]),
    "savad_last_kernel_times": (c_int, [c_void_p, POINTER(c_char_p), POINTER(c_float), c_int]),
    "savad_window_offsets": (c_int, [c_int, c_int, POINTER(c_int32)]),
    "savad_gather_windows": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "savad_boost": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "savad_predict_workspace_bytes": (c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "savad_predict_probabilities": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "savad_gather_windows_batch": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                           c_void_p]),
    "savad_boost_batch": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "savad_predict_batch_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(c_size_t)]),
    "savad_predict_probabilities_batch": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                                  c_void_p, c_size_t, c_void_p]),
    "savad_stream_window_count": (c_int, [c_int, c_int, c_int]),
    "savad_pcm16_to_f32": (c_int, [c_void_p, ctypes.c_long, c_void_p, c_void_p]),
    "savad_gather_strided": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "savad_overlap_merge": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "savad_logmel_frames": (c_int, [c_int]),
    "savad_logmel_workspace_bytes": (c_size_t, [c_int]),
    "savad_logmel": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "savad_logmel_span_samples": (c_int, [c_long, c_int, c_int, POINTER(c_long), POINTER(c_long)]),
    "savad_logmel_span_workspace_bytes": (c_size_t, [c_int]),
    "savad_logmel_span": (c_int, [c_void_p, c_long, c_long, c_long, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "savad_logmel_set_algorithm": (c_int, [c_int]),
    "savad_logmel_table_floats": (c_int, [c_int]),
    "savad_logmel_tables_host": (c_int, [c_void_p, c_void_p, c_void_p]),
    "savad_frontend_shape": (c_int, [POINTER(savad_frontend_config), c_long, POINTER(c_int), POINTER(c_int)]),
    "savad_frontend_workspace_bytes": (c_int, [POINTER(savad_frontend_config), c_long, POINTER(c_size_t)]),
    "savad_frontend_prepare": (c_int, [POINTER(savad_frontend_config)]),
    "savad_frontend": (c_int, [POINTER(savad_frontend_config), c_void_p, c_long, c_void_p, c_void_p, c_void_p]),
    "savad_frontend_table_floats": (c_int, [POINTER(savad_frontend_config), c_int]),
    "savad_frontend_tables_host": (c_int, [POINTER(savad_frontend_config), c_int, c_void_p]),
    "savad_resample_length": (c_long, [c_long, c_int]),
    "savad_resample_set_window": (c_int, [c_void_p]),
    "savad_resample_prepare": (c_int, [c_int]),
    "savad_resample": (c_int, [c_void_p, c_long, c_int, c_void_p, c_void_p]),
    "savad_resample_span_samples": (c_int, [c_long, c_int, c_long, c_long, POINTER(c_long), POINTER(c_long)]),
    "savad_resample_span": (c_int, [c_void_p, c_long, c_long, c_long, c_int, c_long, c_long, c_void_p, c_void_p]),
    "savad_resample_table_host": (c_int, [c_int, c_void_p, c_void_p]),
    "savad_resample_segments_host": (c_int, [c_int, c_int, c_void_p, c_void_p, c_void_p, POINTER(c_long)]),
    "savad_resample_set_table_mode": (c_int, [c_int]),
    "savad_ingest_downmix": (c_int, [c_void_p, c_int, c_int, c_long, c_void_p, c_void_p]),
    "savad_trim_voice_activity": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "savad_frames_to_samples": (c_long, [c_void_p, c_int, c_int, c_double, c_double, c_void_p]),
    "savad_samples_to_segments": (c_int, [c_void_p, c_long, c_void_p, c_void_p, c_int]),
    "savad_optimal_split": (c_int, [c_void_p, c_void_p, c_long, c_long, c_void_p]),
    "savad_post_supported": (c_int, [c_int, c_int, c_double, c_double, c_int]),
    "savad_post_workspace_bytes": (c_int, [c_int, c_int, c_int, c_double, c_double, POINTER(c_size_t)]),
    "savad_post_frames": (c_int, [c_void_p, c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "savad_post_segments": (c_int, [c_void_p, c_void_p, c_int, c_int, c_double, c_double, c_long, c_void_p, c_void_p, c_int, c_void_p, c_size_t,
                                    c_void_p]),
    "savad_post_sample_probs": (c_int, [c_void_p, c_int, c_int, c_double, c_double, c_void_p, c_void_p]),
    "savad_post_frames_host": (c_int, [c_void_p, c_int, c_int, c_float, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "savad_post_sample_class_host": (c_int, [c_void_p, c_int, c_int, c_double, c_double, c_long, c_long, c_void_p]),
    "savad_post_set_block": (c_int, [c_int]),
    "savad_eval_supported": (c_int, [c_int, c_long, c_long]),
    "savad_eval_workspace_bytes": (c_int, [c_int, c_int, POINTER(c_size_t)]),
    "savad_eval_counts": (c_long, [c_void_p, c_int, c_int, c_void_p, c_long, c_float, c_int, c_void_p, c_void_p, c_long, c_void_p, c_size_t,
                                   c_void_p]),
    "savad_eval_sort": (c_int, [c_void_p, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "savad_eval_counts_host": (c_long, [c_void_p, c_int, c_int, c_void_p, c_long, c_float, c_int, c_void_p, c_void_p, c_long]),
    "savad_eval_set_block": (c_int, [c_int]),
    "savad_live_ready_frames": (c_long, [c_long]),
    "savad_live_final_rows": (c_long, [c_long, c_int]),
    "savad_live_state_bytes": (c_int, [c_void_p, POINTER(c_size_t)]),
    "savad_live_table_bytes": (c_int, [c_void_p, c_int, POINTER(c_size_t)]),
    "savad_live_max_rows": (c_int, [c_void_p, POINTER(c_int)]),
    "savad_live_workspace_bytes": (c_int, [c_void_p, c_void_p, c_int, POINTER(c_size_t)]),
    "savad_live_open": (c_int, [c_void_p, c_void_p, c_int]),
    "savad_live_plan": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p]),
    "savad_live_append": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "savad_live_logmel": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "savad_live_gather": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "savad_live_boost": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "savad_live_commit": (c_int, [c_void_p, c_void_p, c_void_p]),
    "savad_live_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "savad_live_post_state_bytes": (c_int, [c_void_p, c_int, POINTER(c_size_t)]),
    "savad_live_post_event_bytes": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_size_t), POINTER(c_size_t)]),
    "savad_live_post_workspace_bytes": (c_int, [c_void_p, c_void_p, c_void_p, POINTER(c_size_t)]),
    "savad_live_post": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p]),
    "savad_live_post_host": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_int, POINTER(c_int)]),
    "savad_last_error": (c_char_p, []),
    "savad_version": (c_char_p, []),
}

_lib = None


def load():
    """Load libsavad.so (once).  `import torch` first so that the HIP runtime already mapped by
    torch (same SONAME libamdhip64.so.7) is the one the library binds to."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (maps libamdhip64 before dlopen)

    if not LIB_PATH.exists():
        raise SavadError(
            f"{LIB_PATH} is missing: build it with `python -m voice_activity_detection_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for this path.")
    lib = ctypes.CDLL(str(LIB_PATH))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI drifted
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        raise SavadError(f"libsavad error {rc}: {load().savad_last_error().decode()}")
