"""GPU tests of the train step's last stage, element by element against float64 models: the fused clip norm, the AMSGrad / Adam / SGD
update and the gradient-noise hook (tests/optimizer_model.py), and the counter-based dropout / normal fills (tests/rng_model.py) of
ast_amd/csrc/util.hip, through the C ABI and through ast_amd/optimizers.py.  The tolerances are optimizer_model.TOL, derived on the host
from the float32 evaluation of the same model (tests/test_optimizer_host.py); every buffer a kernel writes lies between sentinel bands.

Worst figures measured on an MI355X (relative to the reference tensor's maximum; the tolerance behind the slash):
norm 1.10e-7 / 1e-6, p 2.17e-7 / 1e-6, m 2.75e-7 / 2e-6, v 3.04e-7 / 2e-6, vhat 3.04e-7 / 2e-6, SGD p 1.21e-7 / 5e-7,
hook gradient 9.7e-8 / 5e-7 (what is left after the 1e-5 sigma allowance)."""
import ctypes as C

import numpy as np
import pytest
import torch

import optimizer_model as OM
import rng_model as RM
from conftest import tiny_cfg
from test_gpu_ops import dev, ok, stream, vp

pytestmark = pytest.mark.gpu

SENT_BITS = 0x5A5A5A5A
SENT = np.array([SENT_BITS], np.uint32).view(np.float32)[0]
WORST = {}


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


def note(q, e):
    WORST[q] = max(WORST.get(q, 0.0), float(e))
    return e


class Buf:
    """n float32 values between two sentinel bands of 64 + 4 floats; `shift` floats off a 16-byte boundary.  Everything outside the n
    values -- the bands, and so every element at index >= n -- must keep its bit pattern."""
    BAND = 64

    def __init__(self, values, shift=0):
        values = np.asarray(values, np.float32)
        self.n, self.lo = len(values), self.BAND + shift
        host = np.full(self.lo + self.n + self.BAND + 4, SENT, np.float32)
        host[self.lo:self.lo + self.n] = values
        self.t = dev(host)
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 4 * self.lo)

    def get(self):
        return self.t[self.lo:self.lo + self.n].cpu().numpy()

    def check(self, what=""):
        bits = self.t.view(torch.int32)
        bad = int((bits[:self.lo] != SENT_BITS).sum()) + int((bits[self.lo + self.n:] != SENT_BITS).sum())
        assert bad == 0, f"{what}: {bad} elements outside the {self.n} values were written"


class Sq:
    """The float64 norm slot between two bands of 64 doubles."""

    def __init__(self, value=-7.0):
        host = np.full(129, -7.0)
        host[64] = value
        self.t = dev(host, torch.float64)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 8 * 64)

    def value(self):
        return float(self.t[64].item())

    def check(self):
        assert int((self.t != -7.0).sum()) <= 1 and float(self.t[63]) == -7.0 and float(self.t[65]) == -7.0


def _norm(lib, p, g, gsc, l2, sq=None, n=None):
    sq = sq or Sq()
    n = p.n if n is None else n
    if gsc == 1.0:
        ok(lib, lib.astk_grad_sqnorm(g.ptr, p.ptr, l2, n, sq.ptr, stream()))
    else:
        ok(lib, lib.astk_grad_sqnorm_scaled(g.ptr, p.ptr, gsc, l2, n, sq.ptr, stream()))
    return sq


# ------------------------------------------------------------------ 1. the clip norm
@pytest.mark.parametrize("n", OM.SIZES)
def test_clip_norm_against_float64(lib, n):
    for l2, gsc in OM.NORM_PARAMS:
        p0, g0 = OM.norm_inputs(n, l2, gsc)
        want = OM.finished_gradient(p0, g0, gsc=gsc, l2=l2)[1]
        p, g = Buf(p0), Buf(g0)
        sq = _norm(lib, p, g, gsc, l2)
        got = np.sqrt(sq.value())
        e = note("norm", abs(got - want) / want)
        print(f"norm n={n} l2={l2} gsc={gsc:.3f}: rel err {e:.2e}")
        assert e <= OM.TOL["norm"], (n, l2, gsc, got, want)
        first = sq.value()
        _norm(lib, p, g, gsc, l2, sq)
        assert sq.value() == first, "the same input twice must give the same bits"
        if gsc != 1.0:          # the unscaled entry point on a pre-scaled buffer: the product rounds the same way
            sq1 = _norm(lib, p, Buf(g0 * np.float32(gsc)), 1.0, l2)
            assert sq1.value() == first
        sq.check(), p.check("p"), g.check("g")


def test_clip_norm_never_reads_partial_sums_of_an_earlier_larger_launch(lib):
    big = OM.SIZES[-1]
    order = [big, 5, big, 1, 10007]
    bufs = {n: (Buf(OM.norm_inputs(n, 1e-4, 1.0)[0]), Buf(OM.norm_inputs(n, 1e-4, 1.0)[1])) for n in set(order)}
    sqs = [_norm(lib, *bufs[n], 1.0, 1e-4) for n in order]            # back to back on one stream, read afterwards
    torch.cuda.synchronize()
    for n, sq in zip(order, sqs):
        want = OM.finished_gradient(*OM.norm_inputs(n, 1e-4, 1.0), l2=1e-4)[1]
        assert abs(np.sqrt(sq.value()) - want) <= OM.TOL["norm"] * want, (n, np.sqrt(sq.value()), want)


@pytest.mark.parametrize("n", [1, 5, 10007])
def test_clip_norm_of_a_zero_gradient_is_exactly_zero(lib, n):
    sq = _norm(lib, Buf(OM.weights(n, 1)), Buf(np.zeros(n)), 1.0, 0.0)
    assert sq.value() == 0.0
    sq.check()


def test_clip_norm_refuses_misaligned_buffers(lib):
    p, g = Buf(OM.weights(64, 1)), Buf(OM.weights(64, 2))
    for pa, ga in ((Buf(OM.weights(64, 1), shift=1), g), (p, Buf(OM.weights(64, 2), shift=1))):
        sq = Sq(3.25)
        rc = lib.astk_grad_sqnorm_scaled(ga.ptr, pa.ptr, 1.0, 1e-4, 64, sq.ptr, stream())
        torch.cuda.synchronize()
        assert rc != 0 and b"aligned" in lib.astk_last_error()
        assert sq.value() == 3.25


# ------------------------------------------------------------------ 2. Adam / AMSGrad
def _adam_run(lib, c, shifts=(0, 0, 0, 0, 0), vhat="given", check=True):
    """Runs case `c` through the two kernels; returns the (p, m, v, vhat) arrays after the last step.  shifts: floats off a 16-byte
    boundary for p, g, m, v, vhat (the norm needs aligned p and g: it runs on aligned copies)."""
    c.build()
    n = c.n
    zeros = np.zeros(n, np.float32)
    p, m, v = Buf(c.p0, shifts[0]), Buf(zeros, shifts[2]), Buf(zeros, shifts[3])
    vh = Buf(zeros if c.amsgrad else np.full(n, 7.0, np.float32), shifts[4])
    sq = Sq()
    for t, (g0, ref) in enumerate(zip(c.grads, c.ref), 1):
        g = Buf(g0, shifts[1])
        if shifts[0] or shifts[1]:
            _norm(lib, Buf(p.get()), Buf(g0), c.gsc, c.l2, sq)
        else:
            _norm(lib, p, g, c.gsc, c.l2, sq)
        args = (c.l2, c.clip, sq.ptr, OM.lr_t(c.lr, t), OM.B1, OM.B2, OM.EPS, 1 if c.amsgrad else 0, stream())
        vptr = None if vhat == "null" else vh.ptr
        if c.gsc == 1.0:
            ok(lib, lib.astk_decay_clip_amsgrad_step(p.ptr, g.ptr, m.ptr, v.ptr, vptr, n, *args))
        else:
            ok(lib, lib.astk_decay_clip_amsgrad_step_scaled(p.ptr, g.ptr, m.ptr, v.ptr, vptr, n, c.gsc, *args))
        g.check("g")
        assert np.array_equal(g.get(), g0), "the update must not write the gradient"
        if not check:
            continue
        if not c.zero:
            assert note("norm", abs(np.sqrt(sq.value()) - ref["norm"]) / ref["norm"]) <= OM.TOL["norm"], (c.name, t)
        for q, b in (("p", p), ("m", m), ("v", v)) + ((("vhat", vh),) if c.amsgrad else ()):
            e = note(q, OM.relerr(b.get(), ref[q]))
            assert e <= OM.TOL[q], f"{c.name}: {q} after step {t}: {e:.3e} of its maximum (tolerance {OM.TOL[q]:.0e})"
    for b in (p, m, v, vh):
        b.check(c.name)
    sq.check()
    return p.get(), m.get(), v.get(), vh.get()


@pytest.mark.parametrize("c", OM.adam_cases(), ids=lambda c: c.name)
def test_adam_step_against_float64_after_every_step(lib, c):
    """p, m, v and vhat after each of the 8 steps (zero case: 1): AMSGrad at every size, and at n = 5 / 10007 plain Adam, no clipping
    (clip = 3e38), grad_scale = float32(1/3) and a zero gradient."""
    p, m, v, vh = _adam_run(lib, c)
    print({q: f"{e:.2e}" for q, e in WORST.items()})
    if c.zero:
        assert np.array_equal(p.view(np.uint32), c.p0.view(np.uint32)) and not m.any() and not v.any() and not vh.any()
        assert np.isfinite(p).all()
    if not c.amsgrad:
        assert np.array_equal(vh.view(np.uint32), np.full(c.n, 7.0, np.float32).view(np.uint32)), "amsgrad = 0 must not touch vhat"
        pn, mn, vn, _ = _adam_run(lib, c, vhat="null", check=False)
        assert np.array_equal(pn, p) and np.array_equal(mn, m) and np.array_equal(vn, v)


@pytest.mark.parametrize("n", [5, 10007, 262147])
@pytest.mark.parametrize("shifts", [(1, 1, 1, 1, 1), (0, 1, 0, 0, 0)], ids=["all-offset", "g-offset"])
def test_adam_scalar_path_for_unaligned_pointers_gives_the_same_bits(lib, n, shifts):
    c = next(c for c in OM.adam_cases() if c.name == f"amsgrad-{n}")
    want = _adam_run(lib, c, check=False)
    got = _adam_run(lib, c, shifts=shifts, check=False)
    for q, a, b in zip(("p", "m", "v", "vhat"), got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{q}: {int((a != b).sum())} of {n} elements differ from the aligned run"


# ------------------------------------------------------------------ 3. SGD
@pytest.mark.parametrize("c", OM.sgd_cases(), ids=lambda c: c.name)
def test_sgd_step_against_float64(lib, c):
    c.build()
    p, sq = Buf(c.p0), Sq()
    for t, (g0, ref) in enumerate(zip(c.grads, c.ref), 1):
        g = Buf(g0)
        _norm(lib, p, g, c.gsc, c.l2, sq)
        if c.gsc == 1.0:
            ok(lib, lib.astk_decay_clip_sgd_step(p.ptr, g.ptr, c.n, c.l2, c.clip, sq.ptr, c.lr, stream()))
        else:
            ok(lib, lib.astk_decay_clip_sgd_step_scaled(p.ptr, g.ptr, c.n, c.gsc, c.l2, c.clip, sq.ptr, c.lr, stream()))
        assert note("norm", abs(np.sqrt(sq.value()) - ref["norm"]) / ref["norm"]) <= OM.TOL["norm"], (c.name, t)
        e = note("sgd_p", OM.relerr(p.get(), ref["p"]))
        assert e <= OM.TOL["sgd_p"], f"{c.name}: p after step {t}: {e:.3e} (tolerance {OM.TOL['sgd_p']:.0e})"
        g.check("g")
    p.check("p"), sq.check()
    print({q: f"{e:.2e}" for q, e in WORST.items()})


# ------------------------------------------------------------------ 4. the noise hook's kernel
@pytest.mark.parametrize("n", OM.HOOK_SIZES)
def test_noise_hook_kernel_against_float64(lib, n):
    p0, g0, l2, gsc, clip = OM.hook_inputs(n)
    p = Buf(p0)
    det, norm = OM.finished_gradient(p0, g0, gsc=gsc, l2=l2, clip=clip)
    assert not 0.67 * clip <= norm <= 1.5 * clip          # (clip active at every size but n = 1)
    sq = _norm(lib, p, Buf(g0), gsc, l2)
    for off in OM.HOOK_OFFSETS:
        for sigma in OM.HOOK_SIGMAS:
            g = Buf(g0)
            ok(lib, lib.astk_decay_clip_noise(g.ptr, p.ptr, n, gsc, l2, clip, sq.ptr, sigma, OM.NOISE_SEED, off, stream()))
            want = det + float(np.float32(sigma)) * RM.hook_noise(n, OM.NOISE_SEED, off)
            err = np.abs(g.get() - want).max()
            note("hook", max(0.0, err - 1e-5 * sigma) / np.abs(want).max())
            assert err <= OM.TOL["hook"] * np.abs(want).max() + 1e-5 * sigma, (n, off, sigma, err)
            g.check(f"hook n={n}")        # includes element n, one past the end of an odd n
    p.check("p")
    print({q: f"{e:.2e}" for q, e in WORST.items()})


# ------------------------------------------------------------------ 5. noise and freeze through ast_amd/optimizers.py
def _tiny_model():
    from oracle import ast_ref as R
    from schedule_helpers import gpu_model
    cfg = tiny_cfg()
    P = R.init_params(cfg, 26, 11, seed=0, dtype=np.float32)
    m = gpu_model(cfg, P, 26, 11)
    for link in OM.FREEZE:
        m[link].disable_update()
    return m


def test_enabled_ranges_cover_exactly_the_unfrozen_tensors():
    m = _tiny_model()
    a = m.arena
    offsets, sizes, total = OM.arena_layout(a.shapes)
    assert offsets == a.offsets and total == a.size
    ranges = m.enabled_ranges()
    assert ranges == OM.enabled_ranges(a.shapes, OM.FREEZE)
    assert all(r0[0] + r0[1] < r1[0] for r0, r1 in zip(ranges, ranges[1:])), "ranges are merged and ascending"
    covered = np.zeros(total, bool)
    for o, n in ranges:
        assert not covered[o:o + n].any()
        covered[o:o + n] = True
    for name in a.shapes:
        o, n = offsets[name], sizes[name]
        assert covered[o:o + (n + 3) // 4 * 4].all() == (name.split("/")[0] not in OM.FREEZE) and covered[o:o + n].any() == covered[o:o + n].all()


@pytest.mark.parametrize("eta", [0.0, OM.NOISE_ETA], ids=["plain", "noise"])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_python_layer_updates_with_frozen_links_against_float64(kind, eta):
    from ast_amd import optimizers as O
    m = _tiny_model()
    a = m.arena
    shapes = a.shapes
    offsets, sizes, total = OM.arena_layout(shapes)
    exact, enabled = np.zeros(total, bool), np.zeros(total, bool)
    for name in shapes:
        exact[offsets[name]:offsets[name] + sizes[name]] = True
        enabled[offsets[name]:offsets[name] + sizes[name]] = name.split("/")[0] not in OM.FREEZE
    p0 = a.data.cpu().numpy().copy()
    grads = OM.arena_gradients(shapes, OM.FREEZE, OM.ARENA_STEPS)
    ref = OM.arena_run(shapes, p0, OM.FREEZE, grads, kind, eta)
    opt = (O.Adam(alpha=1e-3, amsgrad=True) if kind == "adam" else O.SGD(lr=0.05)).setup(m)
    opt.add_hook(O.WeightDecay(OM.ARENA_HYPER["l2"]))
    opt.add_hook(O.GradientClipping(OM.ARENA_HYPER["clip"]))
    if eta:
        hook = O.GradientNoise(eta)
        assert hook.seed == OM.NOISE_SEED
        opt.add_hook(hook)
    frozen = exact & ~enabled
    for t, (g0, st) in enumerate(zip(grads, ref), 1):
        a.grad.copy_(torch.from_numpy(g0))
        opt.update()
        torch.cuda.synchronize()
        assert note("norm", abs(opt.last_grad_norm - st["norm"]) / st["norm"]) <= OM.TOL["norm"]
        data, grad = a.data.cpu().numpy(), a.grad.cpu().numpy()
        got = {"p": data}
        if kind == "adam":
            got.update(m=opt.m.cpu().numpy(), v=opt.v.cpu().numpy(), vhat=opt.vhat.cpu().numpy())
        for q, x in got.items():
            tq = "sgd_p" if kind == "sgd" else q
            e = note(tq, OM.relerr(x[enabled], st[q][enabled]))
            assert e <= OM.TOL[tq], f"{kind} eta={eta}: {q} after update {t}: {e:.3e} (tolerance {OM.TOL[tq]:.0e})"
            assert not x[~exact].any(), f"{q}: an alignment pad is no longer zero"
            if q != "p":
                assert not x[frozen].any(), f"{q}: a frozen tensor has a moment"
        assert np.array_equal(data[frozen].view(np.uint32), p0[frozen].view(np.uint32)), "a frozen tensor moved"
        assert np.array_equal(grad[frozen], g0[frozen]) and not grad[~exact].any()
        if eta:
            sigma = OM.noise_sigma(eta, t - 1)
            err = np.abs(grad[enabled] - st["grad"][enabled]).max()
            note("hook", max(0.0, err - 1e-5 * sigma) / np.abs(st["grad"][enabled]).max())
            assert err <= OM.TOL["hook"] * np.abs(st["grad"][enabled]).max() + 1e-5 * sigma, (t, err)
        else:
            assert np.array_equal(grad, g0), "without the noise hook the arena keeps the raw gradient"
    if eta:
        # no value of the noise repeats, across consecutive tensors and across steps: the counter ranges never overlap
        z = np.concatenate([st["noise"][enabled] for st in ref])
        assert len(np.unique(z)) == len(z) and hook.offset == sum((sizes[k] + 1) // 2 for k in shapes if k.split("/")[0] not in OM.FREEZE) * len(ref)
    print({q: f"{e:.2e}" for q, e in WORST.items()})


# ------------------------------------------------------------------ 7. the fills
@pytest.mark.parametrize("ratio", [0.0, 0.3, 0.5])
def test_dropout_mask_bit_equal_to_the_model(lib, ratio):
    for n, off in ((1, 0), (1, 1), (2, 1), (17, 3), (4096, 0), (100003, 2 ** 33 + 1)):
        out = Buf(np.full(n, 9.0))
        ok(lib, lib.astk_fill_dropout_mask(out.ptr, n, ratio, 0x5EED, off, stream()))
        want = RM.dropout_mask(n, ratio, 0x5EED, off)
        got = out.get()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, off, int((got != want).sum()))
        out.check(f"dropout n={n}")


def _normal_bound(mean, sigma):
    """1e-5 sigma (ten times the ~1e-6 of a unit normal the kernel documents for the hardware log2 / sin / cos) + one float32 ulp of the
    largest output magnitude, |mean| + 6 sigma."""
    return 1e-5 * sigma + float(np.spacing(np.float32(abs(mean) + 6 * sigma)))


@pytest.mark.parametrize("mean,sigma", [(0.0, 1.0), (1.0, 0.25)])
def test_normal_fill_against_the_model(lib, mean, sigma):
    """Measured maximum on an MI355X: 5.7e-7 (mean 0, sigma 1) and 1.4e-7 (mean 1, sigma 0.25), against bounds of 1.05e-5 and 2.7e-6."""
    worst = 0.0
    for n in (1, 2, 7, 100003):
        for off in (0, 2 ** 33 + 1):
            out = Buf(np.full(n, 9.0))
            ok(lib, lib.astk_fill_normal(out.ptr, n, mean, sigma, 99, off, stream()))
            err = np.abs(out.get() - RM.normal_fill(n, mean, sigma, 99, off)).max()
            worst = max(worst, err)
            out.check(f"normal n={n}")
            assert err <= _normal_bound(mean, sigma), (n, off, err, _normal_bound(mean, sigma))
    print(f"normal fill mean={mean} sigma={sigma}: max err {worst:.3e} (bound {_normal_bound(mean, sigma):.3e})")


@pytest.mark.parametrize("n_words", [0, 1, 256])
@pytest.mark.parametrize("n_segs", [0, 2])
def test_fused_fill_words_and_segments(lib, n_words, n_segs):
    from ast_amd._lib import RAND_DROPOUT, RAND_NORMAL, RAND_WORDS_MAX, RandSeg
    assert RAND_WORDS_MAX == 256
    spec = [(RAND_DROPOUT, 1001, 0.3, 0.0, 0x5EED, 2 ** 33 + 1), (RAND_NORMAL, 777, 1.0, 0.25, 99, 5)][:n_segs]
    segs = (RandSeg * max(1, n_segs))()
    outs = []
    for i, (kind, n, a, b, seed, off) in enumerate(spec):
        outs.append(Buf(np.full(n, 9.0)))
        segs[i].out, segs[i].n, segs[i].kind, segs[i].a, segs[i].b, segs[i].seed, segs[i].offset = outs[i].ptr.value, n, kind, a, b, seed, off
    words = np.random.default_rng(n_words).integers(-2 ** 31, 2 ** 31, max(n_words, 1)).astype(np.int32)
    dst = torch.full((64 + n_words + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    warr = (C.c_int32 * max(n_words, 1))(*words.tolist())
    ok(lib, lib.astk_fill_random_ex(segs, n_segs, warr, n_words, C.c_void_p(dst.data_ptr() + 4 * 64), stream()))
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    assert np.array_equal(d[64:64 + n_words], words[:n_words]) and (d[:64] == 0x5A5A5A5A).all() and (d[64 + n_words:] == 0x5A5A5A5A).all()
    if n_segs:
        assert np.array_equal(outs[0].get().view(np.uint32), RM.dropout_mask(1001, 0.3, 0x5EED, 2 ** 33 + 1).view(np.uint32))
        assert np.abs(outs[1].get() - RM.normal_fill(777, 1.0, 0.25, 99, 5)).max() <= _normal_bound(1.0, 0.25)
        outs[0].check("dropout segment"), outs[1].check("normal segment")


def test_fused_fill_refuses_too_many_words_or_segments(lib):
    from ast_amd._lib import RAND_NORMAL, RAND_SEG_MAX, RAND_WORDS_MAX, RandSeg
    dst = torch.full((RAND_WORDS_MAX + 64,), 7, dtype=torch.int32, device="cuda")
    warr = (C.c_int32 * (RAND_WORDS_MAX + 1))()
    assert lib.astk_fill_random_ex(None, 0, warr, RAND_WORDS_MAX + 1, vp(dst), stream()) != 0 and b"words" in lib.astk_last_error()
    out = Buf(np.full(16 * (RAND_SEG_MAX + 1), 9.0))
    segs = (RandSeg * (RAND_SEG_MAX + 1))()
    for i in range(RAND_SEG_MAX + 1):
        segs[i].out, segs[i].n, segs[i].kind, segs[i].a, segs[i].b, segs[i].seed, segs[i].offset = out.ptr.value + 64 * i, 16, RAND_NORMAL, 0.0, 1.0, 1, 16 * i
    assert lib.astk_fill_random_ex(segs, RAND_SEG_MAX + 1, None, 0, None, stream()) != 0 and b"segments" in lib.astk_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(out.get(), np.full(out.n, 9.0, np.float32)) and int((dst != 7).sum()) == 0
    ok(lib, lib.astk_fill_random_ex(segs, RAND_SEG_MAX, None, 0, None, stream()))          # the maximum itself is served
    torch.cuda.synchronize()
    assert (out.get()[:16 * RAND_SEG_MAX] != 9.0).all() and (out.get()[16 * RAND_SEG_MAX:] == 9.0).all()
    out.check("segments")
