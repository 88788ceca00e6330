"""GPU tests of three small exported kernels of ast_amd/csrc/util.hip that the linear-projection encoder's backward and the weight-noise
path use: astk_colsum_add_f32 (the plainest handle on colreduce_block, which also carries the bias gradients and the BatchNorm
statistics), astk_add_f32 and astk_scale_f32.  Inputs are integer-valued float32 in -8..8, so every partial sum stays below 2^24
(20000 rows x 8 + 8 = 160008), any summation order is exact and the check is BIT EQUALITY with the float64 result: a dropped, doubled
or misplaced row or column always shows.  Pad columns and guard elements are NaN: readable, never to be emitted, never to be written."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_ops import dev, ok, stream, vp

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


def _ints(rng, *shape):
    return rng.integers(-8, 9, size=shape).astype(np.float32)


def _ptr(t, offset_floats=0):
    return C.c_void_p(t.data_ptr() + 4 * offset_floats)


# ------------------------------------------------------------------ astk_colsum_add_f32
ROWS = [1, 3, 63, 64, 65, 1000, 20000]       # below / at / above the 4 * NR rows of the unrolled path (NR = 16 .. 256 row lanes), several row slabs


@pytest.mark.parametrize("cols", [1, 3, 4, 5, 60, 64, 68, 1000])   # 1 .. 15 and 16 column lanes, ragged last quads, 1 .. 16 column slabs
def test_colsum_add_is_exact_on_integers(lib, cols):
    rng = np.random.default_rng(cols)
    for rows in ROWS:
        for lds in ((cols + 3) // 4 * 4, (cols + 3) // 4 * 4 + 8):
            src = np.full((rows, lds), NAN, np.float32)
            src[:, :cols] = _ints(rng, rows, cols)
            dst0 = _ints(rng, cols)
            want = dst0.astype(np.float64) + src[:, :cols].astype(np.float64).sum(0)
            assert np.abs(want).max() < 2 ** 24
            sd = dev(src)
            dd = torch.full((cols + 2,), NAN, device="cuda")                 # NaN guards on both sides of dst
            dd[1:cols + 1] = dev(dst0)
            ok(lib, lib.astk_colsum_add_f32(_ptr(dd, 1), vp(sd), lds, rows, cols, stream()))
            torch.cuda.synchronize()
            got = dd.cpu().numpy()
            assert np.isnan(got[0]) and np.isnan(got[cols + 1]), (rows, lds, "wrote beside dst")
            bad = np.flatnonzero(got[1:cols + 1].astype(np.float64) != want)
            assert bad.size == 0, (rows, lds, bad[:8], got[1:cols + 1][bad[:8]], want[bad[:8]])
            # the call ADDS: once more on the result
            ok(lib, lib.astk_colsum_add_f32(_ptr(dd, 1), vp(sd), lds, rows, cols, stream()))
            torch.cuda.synchronize()
            assert np.array_equal(dd.cpu().numpy()[1:cols + 1].astype(np.float64), 2 * want - dst0), (rows, lds, "second call")


def test_colsum_add_refuses_quads_it_cannot_load(lib):
    """The kernel loads 16-byte quads at src + r * lds + c: a leading dimension that is no multiple of 4 floats, or a src that is not
    16-byte aligned, is refused with the cause named -- and nothing is added.  (Buffers have slack behind them.)"""
    rows, cols = 70, 5
    rng = np.random.default_rng(0)
    sd = dev(_ints(rng, rows * 16 + 64))
    dst0 = _ints(rng, cols)
    dd = dev(dst0)
    for lds, off, says in [(5, 0, "multiple of 4"), (6, 0, "multiple of 4"), (7, 0, "multiple of 4"), (9, 0, "multiple of 4"),
                           (8, 1, "16-byte aligned"), (8, 2, "16-byte aligned"), (8, 3, "16-byte aligned"), (4, 0, "bad arguments")]:
        rc = lib.astk_colsum_add_f32(vp(dd), _ptr(sd, off), lds, rows, cols, stream())
        torch.cuda.synchronize()
        assert rc != 0, (lds, off)
        assert says in lib.astk_last_error().decode(), (lds, off, lib.astk_last_error().decode())
        assert np.array_equal(dd.cpu().numpy(), dst0), (lds, off, "dst was written")
    ok(lib, lib.astk_colsum_add_f32(vp(dd), _ptr(sd, 4), 8, rows, cols, stream()))      # one quad further: aligned again, accepted
    want = dst0 + sd.cpu().numpy()[4:4 + rows * 8].reshape(rows, 8)[:, :cols].astype(np.float64).sum(0)
    assert np.array_equal(dd.cpu().numpy().astype(np.float64), want)


# ------------------------------------------------------------------ astk_add_f32, astk_scale_f32
SIZES = [0, 1, 255, 256, 257, 10007, 1 << 20]     # nothing, below / at / above one block, an odd size, the grid-stride loop


def _guarded(values):
    t = torch.full((len(values) + 2,), NAN, device="cuda")
    t[1:-1] = dev(values)
    return t


def _unguard(t, what):
    got = t.cpu().numpy()
    assert np.isnan(got[0]) and np.isnan(got[-1]), f"{what}: wrote beside the vector"
    return got[1:-1]


@pytest.mark.parametrize("n", SIZES)
def test_add_is_exact_on_integers(lib, n):
    rng = np.random.default_rng(n)
    a, b = _ints(rng, n), _ints(rng, n)
    ad, bd = _guarded(a), _guarded(b)
    ok(lib, lib.astk_add_f32(_ptr(ad, 1), _ptr(bd, 1), n, stream()))
    torch.cuda.synchronize()
    assert np.array_equal(_unguard(ad, "add dst").astype(np.float64), a.astype(np.float64) + b)
    assert np.array_equal(_unguard(bd, "add src"), b)


@pytest.mark.parametrize("s", [0.5, -4.0])
@pytest.mark.parametrize("n", SIZES)
def test_scale_is_exact_on_integers(lib, n, s):
    rng = np.random.default_rng(n + 1)
    a = _ints(rng, n)
    ad = _guarded(a)
    ok(lib, lib.astk_scale_f32(_ptr(ad, 1), n, s, stream()))
    torch.cuda.synchronize()
    got = _unguard(ad, "scale")
    want = a.astype(np.float64) * s
    assert np.array_equal(got.astype(np.float64), want) and np.array_equal(np.signbit(got), np.signbit(want)), n


def test_add_and_scale_refuse_null_pointers(lib):
    x = torch.ones(8, device="cuda")
    assert lib.astk_scale_f32(None, 8, 2.0, stream()) != 0
    assert lib.astk_add_f32(None, vp(x), 8, stream()) != 0 and lib.astk_add_f32(vp(x), None, 8, stream()) != 0
    torch.cuda.synchronize()
    assert bool((x == 1).all())
