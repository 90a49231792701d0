"""ctypes binding of libsavad.so (C ABI: include/savad.h).  Fails loudly: there is no CPU
fallback in the product path -- if the HIP library is missing or stale, importing it raises.
The symbol table states for every pointer of the ABI whether it is DEVICE memory, HOST memory or the stream, and its element type
(`dev`, `host`, `stream`): call sites hand over tensors, arrays and streams themselves, and a numpy array, a CPU tensor, a strided
view, a wrong dtype or a tensor of another GPU than the current one is an exception at the call, not a fault in a kernel.  Beside
the types: the one argument check of the public functions (`check_tensor`) and the one device guard (`on_device`)."""
from __future__ import annotations

import contextlib
import ctypes
import functools
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_long, c_size_t, c_ulonglong, c_void_p
from pathlib import Path

import numpy as np
import torch  # (before the library is loaded: the HIP runtime torch maps is the one libsavad.so binds to)

_PKG = Path(__file__).resolve().parent

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


class savad_audio_clip(ctypes.Structure):
    _fields_ = [("first", c_int64), ("count", c_int64)]


# ---- pointer argument types ---------------------------------------------------------------------------------------------------
f32, f64, bf16, i16, i32, i64, u8 = (torch.float32, torch.float64, torch.bfloat16, torch.int16, torch.int32, torch.int64, torch.uint8)
_NUMPY = {d: np.dtype(str(d)[6:]) for d in (f32, f64, i16, i32, i64, u8)}


class _Memory:
    """An `argtypes` entry for a pointer into memory on one of `sides` holding elements of `dtypes` (none = any).  A tensor or an array is
    checked and becomes its address; everything `c_void_p` takes -- None, an int, a c_void_p, byref(...), a ctypes array or
    structure -- passes through unchanged: the raw form of the C ABI, and the spelling of an offset address."""
    sides, dtypes, arrays = (), (), ()

    @classmethod
    def _check(cls, value, side, dtypes, contiguous):
        if side not in cls.sides:
            raise TypeError(f"{cls.__name__}: a {type(value).__name__} in {side} memory where {' or '.join(cls.sides)} memory is read")
        if cls.dtypes and value.dtype not in dtypes:
            raise ValueError(f"{cls.__name__}: {value.dtype} elements")
        if not contiguous:
            raise ValueError(f"{cls.__name__}: the {type(value).__name__} is not contiguous")

    @classmethod
    def from_param(cls, value):
        if isinstance(value, torch.Tensor):
            cls._check(value, "device" if value.is_cuda else "host", cls.dtypes, value.is_contiguous())
            if value.is_cuda and value.get_device() != torch.cuda.current_device():   # the library launches on the current device
                raise ValueError(f"{cls.__name__}: a tensor of {value.device} while cuda:{torch.cuda.current_device()} is current (see on_device)")
            value = value.data_ptr()
        elif isinstance(value, np.ndarray):
            cls._check(value, "host", cls.arrays, value.flags.c_contiguous)
            value = value.ctypes.data
        return c_void_p.from_param(value)


def _memory(sides: tuple, *dtypes, _types={}) -> type:
    if (sides, dtypes) not in _types:
        name = f"{' or '.join(sides)}({', '.join(str(d)[6:] for d in dtypes)})"
        _types[sides, dtypes] = type(name, (_Memory,), {"sides": sides, "dtypes": dtypes, "arrays": tuple(_NUMPY[d] for d in dtypes if d in _NUMPY)})
    return _types[sides, dtypes]


# dev(*dtypes): DEVICE memory, a contiguous tensor on the current HIP device; host(*dtypes): HOST memory, a C-contiguous numpy array or a
# contiguous CPU tensor, pinned or not; mem(*dtypes): either side (the library copies with hipMemcpyDefault)
dev, host, mem = (functools.partial(_memory, sides) for sides in (("device",), ("host",), ("host", "device")))


class stream:
    """the hipStream_t of a call: a torch.cuda.Stream (its handle), or what `c_void_p` takes (None = the default stream)"""

    @classmethod
    def from_param(cls, value):
        return c_void_p.from_param(value.cuda_stream if isinstance(value, torch.cuda.Stream) else value)


handle = c_void_p       # savad_handle: opaque
_cfg, _fe, _live, _post = POINTER(savad_config), POINTER(savad_frontend_config), POINTER(savad_live_config), POINTER(savad_live_post_config)
_slots, _size = POINTER(savad_live_slot), POINTER(c_size_t)
_ws, _table_host, _table_dev = dev(u8, f32), host(u8), dev(u8)   # a workspace, as the callers allocate them; a live tick's tables


class _AudioClips(POINTER(savad_audio_clip)):
    """An `argtypes` entry for a savad_audio_clip [C] table in `side` memory: an int64 [C, 2] array or tensor of (first, count) is
    checked as `_Memory` checks and becomes its address; None, an int, a c_void_p or a pointer pass through (the raw form of the C ABI).
    (A struct pointer of the header is a ctypes pointer type in this table, so the class derives from one.)"""
    _type_ = savad_audio_clip
    side = None

    @classmethod
    def from_param(cls, value):
        if isinstance(value, (torch.Tensor, np.ndarray)):
            if value.ndim != 2 or value.shape[1] != 2:
                raise ValueError(f"{cls.__name__}: an audio clip table is [C, 2] (first, count), not {tuple(value.shape)}")
            _memory((cls.side,), i64).from_param(value)   # (the side, dtype and contiguity checks)
            value = value.data_ptr() if isinstance(value, torch.Tensor) else value.ctypes.data
        if isinstance(value, (int, c_void_p)):
            value = ctypes.cast(value if isinstance(value, c_void_p) else c_void_p(value), POINTER(savad_audio_clip))
        return POINTER(savad_audio_clip).from_param(value)   # (ctypes' own check: None, a pointer, byref, an array of the struct)


def _audio_clips(side: str) -> type:
    return type(f"{side} audio clips", (_AudioClips,), {"side": side, "_type_": savad_audio_clip})


_clips_host, _clips_dev = _audio_clips("host"), _audio_clips("device")   # savad_audio_clip [C] on either side

# every symbol include/savad.h declares: name -> (restype, argtypes); pointer kinds and element types as the header states them
SYMBOLS = {
    "savad_create": (c_int, [_cfg, POINTER(handle)]),
    "savad_destroy": (None, [handle]),
    "savad_set_param": (c_int, [handle, c_char_p, mem(f32), c_size_t, stream]),
    "savad_num_params": (c_int, [handle]),
    "savad_param_key": (c_char_p, [handle, c_int]),
    "savad_param_numel": (c_size_t, [handle, c_int]),
    "savad_reserve": (c_int, [handle, c_int, stream]),
    "savad_workspace_bytes": (c_int, [handle, c_int, c_int, _size]),
    "savad_forward": (c_int, [handle, dev(f32), c_int, c_int, dev(f32), _ws, c_size_t, stream]),
    "savad_set_precision": (c_int, [handle, c_int]),
    "savad_residual_saturations": (c_int, [handle, POINTER(c_ulonglong), stream]),
    "savad_forward_ex": (c_int, [handle, dev(f32, bf16), c_int, c_int, c_int, dev(f32), _ws, c_size_t, stream]),
    "savad_forward_strided": (c_int, [handle, dev(f32, bf16), c_int, c_int, c_int, c_long, dev(f32), _ws, c_size_t, stream]),
    "savad_set_attention_splits": (c_int, [handle, c_int]),
    "savad_set_row_mode": (c_int, [handle, c_int]),
    "savad_set_batch_invariant": (c_int, [handle, c_int]),
    "savad_set_profiling": (c_int, [handle, c_int]),
    "savad_profiling_skip": (c_int, [handle, c_int]),
    "savad_last_kernel_times": (c_int, [handle, POINTER(c_char_p), POINTER(c_float), c_int]),
    "savad_window_offsets": (c_int, [c_int, c_int, POINTER(c_int32)]),
    "savad_gather_windows": (c_int, [dev(f32), c_int, c_int, c_int, c_int, c_int, c_int, dev(f32), dev(i64), stream]),
    "savad_boost": (c_int, [dev(f32), dev(i64), c_int, c_int, c_int, dev(f32), dev(f32), dev(f32), stream]),
    "savad_predict_workspace_bytes": (c_int, [handle, c_int, c_int, c_int, c_int, _size]),
    "savad_predict_probabilities": (c_int, [handle, dev(f32), c_int, c_int, c_int, c_int, dev(f32), dev(f32), _ws, c_size_t, stream]),
    "savad_gather_windows_batch": (c_int, [dev(f32), host(i32), dev(i32), c_int, c_int, c_int, c_int, c_int, c_int, dev(i32), dev(f32),
                                           dev(i64), stream]),
    "savad_boost_batch": (c_int, [dev(f32), host(i32), dev(i32), c_int, c_int, c_int, dev(i32), dev(f32), dev(f32), stream]),
    "savad_predict_batch_workspace_bytes": (c_int, [handle, host(i32), c_int, c_int, c_int, c_int, _size]),
    "savad_predict_probabilities_batch": (c_int, [handle, dev(f32), host(i32), dev(i32), c_int, c_int, c_int, c_int, dev(f32), dev(f32),
                                                  _ws, c_size_t, stream]),
    "savad_stream_window_count": (c_int, [c_int, c_int, c_int]),
    "savad_pcm16_to_f32": (c_int, [dev(i16), c_long, dev(f32), stream]),
    "savad_gather_strided": (c_int, [dev(f32), c_int, c_int, c_int, c_int, c_int, c_int, dev(f32), stream]),
    "savad_overlap_merge": (c_int, [dev(f32), c_int, c_int, c_int, c_int, dev(f32), stream]),
    "savad_logmel_frames": (c_int, [c_int]),
    "savad_logmel_workspace_bytes": (c_size_t, [c_int]),
    "savad_logmel": (c_int, [dev(f32), c_int, dev(f32), dev(f32), stream]),
    "savad_logmel_span_samples": (c_int, [c_long, c_int, c_int, POINTER(c_long), POINTER(c_long)]),
    "savad_logmel_span_workspace_bytes": (c_size_t, [c_int]),
    "savad_logmel_span": (c_int, [dev(f32), c_long, c_long, c_long, c_int, c_int, dev(f32), dev(f32), stream]),
    "savad_logmel_set_algorithm": (c_int, [c_int]),
    "savad_logmel_table_floats": (c_int, [c_int]),
    "savad_logmel_tables_host": (c_int, [host(f32), host(f32), host(f32)]),
    "savad_logmel_batch_shape": (c_int, [_clips_host, c_int, c_int64, POINTER(c_int64), POINTER(c_int64)]),
    "savad_logmel_batch_workspace_bytes": (c_int, [_clips_host, c_int, c_int64, _size]),
    "savad_logmel_batch": (c_int, [dev(f32), c_int64, _clips_host, _clips_dev, c_int, _ws, dev(f32), dev(i32), stream]),
    "savad_frontend_shape": (c_int, [_fe, c_long, POINTER(c_int), POINTER(c_int)]),
    "savad_frontend_workspace_bytes": (c_int, [_fe, c_long, _size]),
    "savad_frontend_prepare": (c_int, [_fe]),
    "savad_frontend": (c_int, [_fe, dev(f32), c_long, dev(f32), dev(f32), stream]),
    "savad_frontend_table_floats": (c_int, [_fe, c_int]),
    "savad_frontend_tables_host": (c_int, [_fe, c_int, host(f32)]),
    "savad_resample_length": (c_long, [c_long, c_int]),
    "savad_resample_set_window": (c_int, [host(f64)]),
    "savad_resample_prepare": (c_int, [c_int]),
    "savad_resample": (c_int, [dev(f32), c_long, c_int, dev(f32), stream]),
    "savad_resample_span_samples": (c_int, [c_long, c_int, c_long, c_long, POINTER(c_long), POINTER(c_long)]),
    "savad_resample_span": (c_int, [dev(f32), c_long, c_long, c_long, c_int, c_long, c_long, dev(f32), stream]),
    "savad_resample_table_host": (c_int, [c_int, host(f64), host(f64)]),
    "savad_resample_segments_host": (c_int, [c_int, c_int, host(i64), host(f64), host(f64), POINTER(c_long)]),
    "savad_resample_set_table_mode": (c_int, [c_int]),
    "savad_ingest_downmix": (c_int, [dev(i16, f32), c_int, c_int, c_long, dev(f32), stream]),
    "savad_trim_voice_activity": (c_int, [host(u8), c_int, c_int, c_int, c_int, c_int, host(u8)]),
    "savad_frames_to_samples": (c_long, [host(f64), c_int, c_int, c_double, c_double, host(f64)]),
    "savad_samples_to_segments": (c_int, [host(f64), c_long, host(i64), host(i64), c_int]),
    "savad_optimal_split": (c_int, [host(f64), host(f64), c_long, c_long, host(f64)]),
    "savad_post_supported": (c_int, [c_int, c_int, c_double, c_double, c_int]),
    "savad_post_workspace_bytes": (c_int, [c_int, c_int, c_int, c_double, c_double, _size]),
    "savad_post_frames": (c_int, [dev(f32), c_int, c_int, c_float, c_int, c_int, c_int, c_int, dev(f32), dev(u8), _ws, c_size_t, stream]),
    "savad_post_segments": (c_int, [dev(u8), dev(f32), c_int, c_int, c_double, c_double, c_long, host(i64), host(i64), c_int, _ws, c_size_t, stream]),
    "savad_post_sample_probs": (c_int, [dev(f32), c_int, c_int, c_double, c_double, dev(f64), stream]),
    "savad_post_frames_host": (c_int, [host(f32), c_int, c_int, c_float, c_int, c_int, c_int, c_int, host(f32), host(u8)]),
    "savad_post_sample_class_host": (c_int, [host(u8), c_int, c_int, c_double, c_double, c_long, c_long, host(u8)]),
    "savad_post_set_block": (c_int, [c_int]),
    "savad_post_batch_supported": (c_int, [host(i32), c_int, c_int, c_int, c_double, c_double]),
    "savad_post_batch_slot_table": (c_int, [host(i32), c_int, c_int, c_double, c_double, host(i64)]),
    "savad_post_batch_workspace_bytes": (c_int, [host(i32), c_int, c_int, c_int, c_double, c_double, _size]),
    "savad_post_batch_frames": (c_int, [dev(f32), host(i32), dev(i32), c_int, c_int, c_float, c_int, c_int, c_int, c_int, dev(f32), dev(u8), _ws,
                                        c_size_t, stream]),
    "savad_post_batch_segments": (c_int, [dev(u8), dev(f32), host(i32), dev(i32), c_int, c_int, c_double, c_double, c_long, host(i64), host(u8),
                                          host(i64), host(i64), c_int, _ws, c_size_t, stream]),
    "savad_post_batch_frames_host": (c_int, [host(f32), host(i32), c_int, c_int, c_float, c_int, c_int, c_int, c_int, host(f32), host(u8)]),
    "savad_post_batch_slot_class_host": (c_int, [host(u8), host(i32), c_int, c_int, c_double, c_double, host(u8)]),
    "savad_eval_supported": (c_int, [c_int, c_long, c_long]),
    "savad_eval_workspace_bytes": (c_int, [c_int, c_int, _size]),
    "savad_eval_counts": (c_long, [dev(f32), c_int, c_int, dev(u8), c_long, c_float, c_int, host(i64), host(u8), c_long, _ws, c_size_t, stream]),
    "savad_eval_sort": (c_int, [dev(f32), dev(u8), c_long, dev(f32), dev(u8), _ws, c_size_t, stream]),
    "savad_eval_counts_host": (c_long, [host(f32), c_int, c_int, host(u8), c_long, c_float, c_int, host(i64), host(u8), c_long]),
    "savad_eval_set_block": (c_int, [c_int]),
    "savad_eval_batch_supported": (c_int, [host(i32), host(i32), c_int, c_int]),
    "savad_eval_batch_workspace_bytes": (c_int, [host(i32), host(i32), c_int, c_int, _size]),
    "savad_eval_batch_counts": (c_long, [dev(f32), host(i32), dev(i32), dev(u8), host(i32), dev(i32), c_int, c_int, c_float, c_int, host(i64), host(u8),
                                         c_long, host(i64), _ws, c_size_t, stream]),
    "savad_eval_batch_counts_host": (c_long, [host(f32), host(i32), host(u8), host(i32), c_int, c_int, c_float, c_int, host(i64), host(u8), c_long,
                                              host(i64)]),
    "savad_live_ready_frames": (c_long, [c_long]),
    "savad_live_final_rows": (c_long, [c_long, c_int]),
    "savad_live_state_bytes": (c_int, [_live, _size]),
    "savad_live_table_bytes": (c_int, [_live, c_int, _size]),
    "savad_live_max_rows": (c_int, [_live, POINTER(c_int)]),
    "savad_live_workspace_bytes": (c_int, [handle, _live, c_int, _size]),
    "savad_live_open": (c_int, [_live, _slots, c_int]),
    "savad_live_plan": (c_int, [_live, _slots, POINTER(savad_live_push), c_int, dev(u8), _table_host, c_size_t, POINTER(savad_live_counts),
                                host(i64)]),
    "savad_live_append": (c_int, [_live, _table_host, _table_dev, stream]),
    "savad_live_logmel": (c_int, [_live, _table_host, _table_dev, stream]),
    "savad_live_gather": (c_int, [_live, _table_host, _table_dev, c_int, c_int, dev(f32), stream]),
    "savad_live_boost": (c_int, [_live, _table_host, _table_dev, dev(f32), dev(f32), dev(f32), stream]),
    "savad_live_commit": (c_int, [_live, _table_host, _slots]),
    "savad_live_step": (c_int, [handle, _live, _slots, _table_host, _table_dev, dev(f32), dev(f32), _ws, c_size_t, stream]),
    "savad_live_post_state_bytes": (c_int, [_post, c_int, _size]),
    "savad_live_post_event_bytes": (c_int, [_live, _post, _table_host, _size, _size]),
    "savad_live_post_workspace_bytes": (c_int, [_live, _post, _table_host, _size]),
    "savad_live_post": (c_int, [_live, _post, _table_host, _table_dev, dev(f32), dev(u8), dev(u8), c_size_t, _ws, c_size_t, stream]),
    "savad_live_post_host": (c_int, [_post, host(u8), c_int, c_int64, c_int, c_int, host(f32), POINTER(savad_live_event), c_int, POINTER(c_int)]),
    "savad_last_error": (c_char_p, []),
    "savad_version": (c_char_p, []),
}

_lib = None


def load():
    """Load libsavad.so (once)."""
    global _lib
    if _lib is not None:
        return _lib
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


# ---- the argument check and the device guard of the public functions -----------------------------------------------------------
def check_tensor(t, name: str, dtypes, ndim=None, shape=None, device=None, contiguous: bool = True) -> None:
    """`t` is a tensor on a HIP device (on `device`, when given) with one of `dtypes` and `ndim` dimensions or exactly `shape` (None =
    any size there), contiguous unless the caller makes it so: ValueError otherwise.  The argument types above are the backstop
    behind this check, not its replacement."""
    dtypes = dtypes if isinstance(dtypes, tuple) else (dtypes,)
    ok = isinstance(t, torch.Tensor) and t.dtype in dtypes and t.is_cuda and (t.is_contiguous() or not contiguous)
    if ok and shape is not None:
        ok = t.dim() == len(shape) and all(want is None or want == have for want, have in zip(shape, t.shape))
    if not (ok and (ndim is None or t.dim() == ndim) and (device is None or t.device == device)):
        form = "[" + ", ".join("N" if s is None else str(s) for s in shape) + "]" if shape is not None else f"{ndim}-D" if ndim is not None else "any-shape"
        raise ValueError(f"{name} must be a {'contiguous ' if contiguous else ''}{' or '.join(str(d)[6:] for d in dtypes)} {form} tensor on "
                         f"{'a HIP device' if device is None else device}")


_current = contextlib.nullcontext()   # shared: entering the device that is current already costs nothing


def on_device(device: torch.device):
    """The context every library call is made in: `device` is the current one inside it.  A no-op object when it is current
    already (torch.cuda.device costs ~10 us, and is only needed to switch)."""
    index = device.index
    if index is not None and index == torch.cuda.current_device():
        return _current
    if device.type != "cuda":
        raise SavadError(f"libsavad launches only on a HIP device, not on {device} (no CPU fallback)")
    return _current if index is None else torch.cuda.device(device)
