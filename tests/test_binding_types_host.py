"""The pointer argument types of the ctypes binding (_lib.dev / host / stream) on the CPU: what passes through as `c_void_p` takes
it, what a host array becomes, what is refused -- and the symbol table against include/savad.h, parameter by parameter.  No
library call is made: only `from_param` runs."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from voice_activity_detection_amd import _lib

REPO = Path(__file__).resolve().parents[1]
KINDS = [_lib.dev(_lib.f32), _lib.dev(), _lib.host(_lib.i32), _lib.host(), _lib.mem(_lib.f32), _lib.stream]


def address(param):
    """the address a from_param result puts on the stack"""
    return ctypes.cast(param, ctypes.c_void_p).value


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.__name__)
def test_raw_values_pass_as_c_void_p_takes_them(kind):
    scalar, array, struct = ctypes.c_int(7), (ctypes.c_float * 4)(), _lib.savad_live_counts()
    for value in (None, 0, 1 << 20, (1 << 47) + 16, ctypes.c_void_p(12345), ctypes.c_void_p(), ctypes.byref(scalar), array,
                  ctypes.byref(struct), ctypes.pointer(scalar)):
        assert address(kind.from_param(value)) == address(ctypes.c_void_p.from_param(value)), value
    assert address(kind.from_param(array)) == ctypes.addressof(array)
    assert address(kind.from_param(ctypes.byref(scalar))) == ctypes.addressof(scalar)
    with pytest.raises(TypeError):
        kind.from_param(1.5)   # (what c_void_p refuses stays refused)


def test_host_takes_arrays_and_cpu_tensors_to_their_data():
    kind = _lib.host(_lib.i32)
    a = np.arange(12, dtype=np.int32)
    assert address(kind.from_param(a)) == a.ctypes.data
    assert address(kind.from_param(a[3:])) == a.ctypes.data + 12          # a contiguous slice: its own first element
    assert address(kind.from_param(a.reshape(3, 4))) == a.ctypes.data
    t = torch.arange(12, dtype=torch.int32)
    assert address(kind.from_param(t)) == t.data_ptr()
    assert address(_lib.host().from_param(np.zeros(3, np.float64))) != 0   # no dtypes: any
    with pytest.raises(ValueError, match="int64"):
        kind.from_param(np.arange(12, dtype=np.int64))
    with pytest.raises(ValueError, match="int64"):
        kind.from_param(torch.arange(12))
    with pytest.raises(ValueError, match="contiguous"):
        kind.from_param(a[::2])
    with pytest.raises(ValueError, match="contiguous"):
        kind.from_param(t[::2])
    with pytest.raises(ValueError, match="contiguous"):
        kind.from_param(np.asfortranarray(a.reshape(3, 4)))
    two = _lib.host(_lib.i16, _lib.f32)
    assert address(two.from_param(np.zeros(4, np.int16))) and address(two.from_param(np.zeros(4, np.float32)))
    with pytest.raises(ValueError):
        two.from_param(np.zeros(4, np.float64))


def test_device_refuses_host_memory_by_name():
    for kind in (_lib.dev(_lib.f32), _lib.dev()):
        with pytest.raises(TypeError, match="device"):
            kind.from_param(torch.zeros(4))
        with pytest.raises(TypeError, match="device"):
            kind.from_param(np.zeros(4, np.float32))
    assert "device" in _lib.dev(_lib.f32).__name__ and "host" in _lib.host(_lib.i32).__name__
    # either side (savad_set_param's data: hipMemcpyDefault) takes host memory, with the dtype rule
    assert address(_lib.mem(_lib.f32).from_param(torch.zeros(4))) != 0
    with pytest.raises(ValueError):
        _lib.mem(_lib.f32).from_param(torch.zeros(4, dtype=torch.float64))


def test_same_kind_is_one_type():
    assert _lib.dev(_lib.f32) is _lib.dev(_lib.f32) and _lib.dev(_lib.f32) is not _lib.host(_lib.f32)
    assert _lib.dev(_lib.f32, _lib.bf16) is not _lib.dev(_lib.f32)


# ---- the table against the header ----------------------------------------------------------------------------------------------
OPAQUE = ("savad_handle",)   # the header's opaque handle: the only bare c_void_p of the table
SCALARS = {"float": (_lib.f32, ctypes.c_float), "double": (_lib.f64, ctypes.c_double), "int64_t": (_lib.i64, ctypes.c_int64),
           "long": (_lib.i64, ctypes.c_long), "int32_t": (_lib.i32, ctypes.c_int32), "int": (_lib.i32, ctypes.c_int),
           "short": (_lib.i16, ctypes.c_short), "uint8_t": (_lib.u8, ctypes.c_uint8), "size_t": (None, ctypes.c_size_t),
           "unsigned long long": (None, ctypes.c_ulonglong)}
VALUES = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
          "int64_t": ctypes.c_int64}


def header_functions():
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "savad.h").read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(savad_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = [] if params == ["void"] else [re.match(r"(?:const )?(.*?)\s*(\w+)$", p).groups() for p in params]
    return out


def test_every_pointer_of_the_header_has_a_kind():
    functions = header_functions()
    assert set(functions) == set(_lib.SYMBOLS)
    kinds = 0
    for name, params in functions.items():
        argtypes = _lib.SYMBOLS[name][1]
        assert len(argtypes) == len(params), name
        for (ctype, pname), arg in zip(params, argtypes):
            where = f"{name}({ctype} {pname})"
            if ctype in OPAQUE:
                assert arg is ctypes.c_void_p, where
                continue
            assert arg is not ctypes.c_void_p, f"{where}: a bare c_void_p"
            if not ctype.endswith("*"):
                assert arg is VALUES[ctype], where
            elif pname == "stream":
                assert ctype == "void*" and arg is _lib.stream, where
            elif ctype == "char*":
                assert arg is ctypes.c_char_p, where
            elif issubclass(arg, ctypes._Pointer):     # an out-parameter, a struct, an array of structs or of strings
                base = ctype[:-1].replace("const ", "").strip()
                want = (getattr(_lib, base, None) or {"savad_handle": ctypes.c_void_p, "char*": ctypes.c_char_p}.get(base)
                        or SCALARS[base][1])
                assert arg._type_ is want, where
            else:
                assert issubclass(arg, _lib._Memory) and arg.sides in (("device",), ("host",), ("host", "device")), where
                kinds += 1
                base = ctype[:-1].strip()
                if base != "void":                     # a typed pointer: the table's element type is the header's
                    assert arg.dtypes == (SCALARS[base][0],), where
    assert kinds > 100   # (this branch is not idle: the table has about 140 such pointers)


def test_kinds_the_header_spells_out():
    S = _lib.SYMBOLS
    dev, host, f32, i32, i64, i16, u8, bf16 = _lib.dev, _lib.host, _lib.f32, _lib.i32, _lib.i64, _lib.i16, _lib.u8, _lib.bf16
    assert S["savad_logmel"][1] == [dev(f32), ctypes.c_int, dev(f32), dev(f32), _lib.stream]
    assert S["savad_boost"][1][1] is dev(i64)
    batch = S["savad_predict_probabilities_batch"][1]
    assert batch[2] is host(i32) and batch[3] is dev(i32)                # clip_first_host (HOST), clip_first (DEVICE)
    assert S["savad_forward_ex"][1][1] is dev(f32, bf16) and S["savad_ingest_downmix"][1][0] is dev(i16, f32)
    assert S["savad_forward"][1][5] is dev(u8, f32)                      # a workspace, as the callers allocate them
    assert S["savad_set_param"][1][2] is _lib.mem(f32)                   # "a host or a device pointer"
    post = S["savad_post_segments"][1]
    assert post[0] is dev(u8) and post[1] is dev(f32) and post[7] is host(i64) and post[8] is host(i64)   # "starts, ends: HOST"
    counts = S["savad_eval_counts"][1]
    assert counts[3] is dev(u8) and counts[7] is host(i64) and counts[8] is host(u8)                      # "counters, seg: HOST"
    for name in ("savad_trim_voice_activity", "savad_frames_to_samples", "savad_samples_to_segments", "savad_optimal_split",
                 "savad_post_frames_host", "savad_post_sample_class_host", "savad_eval_counts_host", "savad_logmel_tables_host",
                 "savad_resample_table_host", "savad_resample_set_window"):
        assert all(a.sides == ("host",) for a in S[name][1] if isinstance(a, type) and issubclass(a, _lib._Memory)), name
    step = S["savad_live_step"][1]
    assert step[3] is host(u8) and step[4] is dev(u8)                    # table_host, table_dev


def test_check_tensor_and_guard_refuse_the_cpu():
    with pytest.raises(ValueError, match="pcm must be a contiguous int16 1-D tensor on a HIP device"):
        _lib.check_tensor(torch.zeros(4, dtype=torch.int16), "pcm", torch.int16, 1)
    with pytest.raises(ValueError, match=r"out must be a contiguous float32 \[3, 7, 2\] tensor"):
        _lib.check_tensor(np.zeros((3, 7, 2), np.float32), "out", torch.float32, shape=(3, 7, 2))
    with pytest.raises(_lib.SavadError, match="no CPU fallback"):
        _lib.on_device(torch.device("cpu"))
