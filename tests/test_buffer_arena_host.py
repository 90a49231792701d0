"""tests/buffer_arena.py on the CPU, with plain numpy "kernels": the helper accepts an exact kernel and catches each violation the GPU
cases (tests/test_gpu_caller_buffers.py) exist to find -- a one-byte overrun, a one-byte underrun, a write into an input, and a read of
one poisoned element that reaches the result.  Runs on any box."""
import numpy as np
import pytest
import torch

from tests.buffer_arena import GUARD, IN_FILL, OUT_FILL, BufferArena, same_bits

N = 61   # odd: 244 bytes of float32, 61 bytes of uint8


def _case(align_in=4, align_out=4):
    x = torch.from_numpy(np.random.default_rng(3).standard_normal(N).astype(np.float32))
    arena = BufferArena("cpu", 1 << 16)
    xin = arena.place_input(x, align_in, "x")
    out = arena.place_output(4 * N, align_out, torch.float32, "out")
    return arena, x, xin, out


def _raw(arena):
    return arena.buf.numpy()


def _extent(arena, name):
    for n, _, _, start, end, _, _ in arena.placed:
        if n == name:
            return start, end
    raise KeyError(name)


def test_exact_kernel_passes():
    arena, x, xin, out = _case()
    assert same_bits(xin, x) and (out.view(torch.uint8) == OUT_FILL).all()
    out.numpy()[:] = 2.0 * xin.numpy()
    arena.check()
    assert same_bits(out, 2.0 * x)


@pytest.mark.parametrize("align", [1, 2, 4, 8, 16])
def test_placement_has_the_alignment_and_no_more(align):
    arena = BufferArena("cpu", 1 << 16)
    a = arena.place_output(33, align, name="a")
    b = arena.place_input(torch.arange(7, dtype=torch.uint8), align, "b")
    for t in (a, b):
        assert t.data_ptr() % align == 0 and t.data_ptr() % (2 * align) != 0
    (sa, ea), (sb, eb) = _extent(arena, "a"), _extent(arena, "b")
    assert ea - sa == 33 and eb - sb == 7 and sa >= GUARD and sb - ea >= 2 * GUARD
    raw = _raw(arena)
    assert (raw[:sa] == OUT_FILL).all() and (raw[sa:ea + GUARD] == OUT_FILL).all()
    assert (raw[ea + GUARD:sb] == IN_FILL).all() and (raw[eb:eb + GUARD] == IN_FILL).all()
    arena.check()


def test_typed_views():
    arena = BufferArena("cpu", 1 << 16)
    pcm = arena.place_input(torch.tensor([-32768, -1, 0, 1, 32767], dtype=torch.int16), 2, "pcm")
    x = arena.place_input(torch.ones((3, 7, 13), dtype=torch.bfloat16), 16, "x")
    out = arena.place_output(8 * 5, 8, torch.float64, "out")
    assert pcm.dtype == torch.int16 and pcm.tolist() == [-32768, -1, 0, 1, 32767]
    assert x.shape == (3, 7, 13) and x.dtype == torch.bfloat16 and x.is_contiguous() and out.shape == (5,)
    arena.check()
    with pytest.raises(ValueError):
        arena.place_output(1 << 16, 4)
    with pytest.raises(ValueError):
        arena.place_output(4, 3)


def test_one_byte_overrun_is_caught():
    arena, x, xin, out = _case()
    out.numpy()[:] = xin.numpy()
    start, end = _extent(arena, "out")
    _raw(arena)[end] = 0   # a store one byte too wide
    found = arena.violations()
    assert len(found) == 1 and "out: 1 bytes of the back guard" in found[0] and "1 bytes past" in found[0]
    with pytest.raises(AssertionError, match="back guard"):
        arena.check()


def test_one_byte_underrun_is_caught():
    arena, x, xin, out = _case()
    out.numpy()[:] = xin.numpy()
    start, end = _extent(arena, "out")
    _raw(arena)[start - 1] = 0
    found = arena.violations()
    assert len(found) == 1 and "out: 1 bytes of the front guard" in found[0] and "1 bytes in front of" in found[0]
    with pytest.raises(AssertionError, match="front guard"):
        arena.check()


def test_far_end_of_a_guard_is_caught():
    arena, x, xin, out = _case()
    start, end = _extent(arena, "x")
    _raw(arena)[end + GUARD - 1] ^= 1
    assert any("x: 1 bytes of the back guard" in line for line in arena.violations())


def test_write_into_an_input_is_caught():
    arena, x, xin, out = _case()
    out.numpy()[:] = xin.numpy()
    xin.numpy()[N // 2] += 1.0   # an in-place "kernel"
    found = arena.violations()
    assert len(found) == 1 and found[0].startswith("x:") and "input itself changed" in found[0]
    with pytest.raises(AssertionError, match="input itself"):
        arena.check()


def test_poisoned_read_changes_the_result():
    """a moving sum that reads one element past the input: inside the arena that element is the poison, so the result differs from
    the clean call's, where an exact kernel's does not"""
    def exact(v, n):
        return np.array([v[i:min(i + 2, n)].sum() for i in range(n)], dtype=np.float32)

    def overreading(v, n):
        return np.array([v[i:i + 2].sum() for i in range(n)], dtype=np.float32)

    arena, x, xin, out = _case()
    start, end = _extent(arena, "x")
    wide = torch.from_numpy(_raw(arena)[start:end + 4]).view(torch.float32).numpy()   # what a kernel addressing past the end sees
    assert np.isnan(wide[N])
    clean = exact(x.numpy(), N)
    out.numpy()[:] = exact(wide, N)
    arena.check()
    assert same_bits(out, clean)
    out.numpy()[:] = overreading(wide, N)
    arena.check()                                    # nothing was written out of place ...
    assert not same_bits(out, clean)                 # ... the result gives the read away
    padded = np.concatenate([x.numpy(), np.zeros(1, np.float32)])
    assert same_bits(overreading(padded, N), clean)  # in allocator slack (zeros, say) the same kernel passes


def test_unwritten_output_element_differs_from_any_result():
    arena, x, xin, out = _case()
    out.numpy()[:N - 1] = xin.numpy()[:N - 1]
    arena.check()
    assert not same_bits(out, x) and same_bits(out[:N - 1], x[:N - 1])
    assert (out[N - 1:].view(torch.uint8) == OUT_FILL).all()


def test_poison_values():
    arena = BufferArena("cpu", 1 << 16)
    arena.place_input(torch.zeros(4), 4, "x")
    start, end = _extent(arena, "x")
    g = torch.from_numpy(_raw(arena)[end:end + 8].copy())
    assert torch.isnan(g.view(torch.float32)).all() and torch.isnan(g.view(torch.float16).float()).all()
    assert torch.isnan(g.view(torch.bfloat16).float()).all() and (g.view(torch.int16) == -1).all() and (g == 255).all()
