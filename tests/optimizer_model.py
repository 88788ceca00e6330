"""The last stage of the train step restated over flat NumPy arrays: the fused clip norm, the AMSGrad / Adam / SGD update and the
gradient-noise hook of ast_amd/csrc/util.hip, as driven by ast_amd/optimizers.py.  A helper, not a test module:
tests/test_optimizer_host.py derives the GPU tolerances from it, tests/test_gpu_optimizer.py compares the kernels with it.

One update, on inputs rounded to float32 first (they are the kernel's inputs), evaluated in `dtype`:

    g' = round_f32(g * gsc) + l2 * p                 over the WHOLE arena (decay on every parameter with a gradient)
    sq = sum g'^2, norm = sqrt(sq)                   over the whole arena
    r  = clip / norm, g'' = g' * r  only when r < 1  (norm = 0: r = inf, no clip)
    g''' = g'' + noise                               (optional: the GradientNoise hook, an explicit vector)
    inside the enabled ranges only:
      Adam:  m += (1 - b1)(g''' - m);  v += (1 - b2)(g'''^2 - v);  vhat = max(vhat, v) (AMSGrad) or v;
             p -= lr_t * m / (sqrt(vhat) + eps)      lr_t = lr sqrt(1 - b2^t) / (1 - b1^t)
      SGD:   p -= lr * g'''

Hyper-parameters are kernel arguments too: gsc, l2, clip, lr_t (lr for SGD) and eps are rounded to float32, and the moment rates are
float32(1 - beta) with the subtraction in double -- what Chainer-on-NumPy multiplies its float32 arrays with.

dtype = float64 is the reference; dtype = float32 is the "plain float32" evaluation in the sense of tests/test_ranges_host.py: every
operation rounded to float32 (the norm's sum in float64, as the kernel and Chainer-on-NumPy's dot both accumulate wider than the data).

Tolerances (relative to the maximum of the checked tensor over the case; the norm relative to itself).  Each is the smallest value of
the form {1, 2, 5} x 10^k for which the float32 evaluation stays within a QUARTER of it on every case the GPU suite runs
(tests/test_optimizer_host.py asserts the quarter condition and that every mutant below misses at least one of them).  Measured float32
figures, worst over all cases:

    quantity      float32 model   tolerance
    norm          1.29e-7         1e-6
    p  (Adam)     2.17e-7         1e-6
    m             3.68e-7         2e-6
    v             3.14e-7         2e-6
    vhat          3.14e-7         2e-6
    p  (SGD)      1.21e-7         5e-7
    hook gradient 1.17e-7         5e-7
"""
import numpy as np

TOL = {"norm": 1e-6, "p": 1e-6, "m": 2e-6, "v": 2e-6, "vhat": 2e-6, "sgd_p": 5e-7, "hook": 5e-7}

B1, B2, EPS = 0.9, 0.999, 1e-8
NO_CLIP = 3.0e38                                  # what optimizers.py passes when no GradientClipping hook is installed
GSC3 = float(np.float32(1.0 / 3.0))               # a grad_scale whose product with a float32 rounds
SIZES = (1, 3, 4, 5, 1023, 10007, 262147, 2098355)      # the last: 2^21 + 1203, above every threshold of the kernels, 3-element tail
LADDER = (0.05, 0.001, 0.2, 50.0, 0.0003, 3.0, 0.01, 0.0001)      # gradient scales; begins with the old entry test's (0.05, 0.001, 0.2)
MAGS = (1e-3, 1.0, 30.0)                          # weight magnitudes, cycling element by element
MUTANTS = ("no_max", "eps_inside_sqrt", "clip_before_decay", "clip_always", "norm_without_decay", "norm_over_enabled_only",
           "sgd_without_decay", "scale_after_decay")


def f32(x, dt):
    """A hyper-parameter as the kernel receives it: rounded to float32, then carried in the evaluation's type."""
    return dt(np.float32(x))


def lr_t(lr, t):
    return lr * np.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)


def finished_gradient(p, g, *, gsc=1.0, l2=0.0, clip=NO_CLIP, ranges=None, dtype=np.float64, mutant=None):
    """(g'' , norm): the decayed, clipped gradient over the whole arena and the norm the clip compared with its threshold."""
    dt = np.dtype(dtype).type
    p32, g32 = np.asarray(p, np.float32), np.asarray(g, np.float32)
    if mutant == "scale_after_decay":
        gd = (g32.astype(dtype) + f32(l2, dt) * p32.astype(dtype)) * dt(np.float32(gsc))
    else:
        gd = (g32 * np.float32(gsc)).astype(dtype) + f32(l2, dt) * p32.astype(dtype)      # the product rounds to float32 in either dtype
    gn = (g32 * np.float32(gsc)).astype(dtype) if mutant in ("norm_without_decay", "clip_before_decay") else gd
    if mutant == "norm_over_enabled_only" and ranges is not None:
        gn = np.concatenate([gn[o:o + n] for o, n in ranges]) if ranges else gn[:0]
    sq = float(np.sum(gn.astype(np.float64) ** 2)) if dtype == np.float64 else float(np.sum((gn * gn).astype(np.float64)))
    norm = np.sqrt(sq)
    nd = dt(norm)
    with np.errstate(over="ignore"):              # NO_CLIP over a small float32 norm: inf, no clip
        r = f32(clip, dt) / nd if nd > 0 else dt(np.inf)
    if mutant == "clip_before_decay":
        gd = (gn * r if r < 1 else gn) + f32(l2, dt) * p32.astype(dtype)
    elif r < 1 or (mutant == "clip_always" and np.isfinite(r)):
        gd = gd * r
    return gd, norm


class State:
    """p, m, v, vhat of one arena, in `dtype`, starting from float32 weights and zero moments; t counts the updates."""

    def __init__(self, p0, dtype=np.float64):
        self.dtype = dtype
        self.p = np.asarray(p0, np.float32).astype(dtype)
        self.m, self.v, self.vhat = (np.zeros_like(self.p) for _ in range(3))
        self.t = 0
        self.norm = None
        self.grad = None            # the finished gradient of the last update (what the noise hook leaves in the arena)


def update(s, g, *, kind="adam", amsgrad=True, gsc=1.0, l2=0.0, clip=NO_CLIP, lr=1e-3, ranges=None, noise=None, mutant=None):
    """One update of State `s` with gradient `g` (float32 values).  `ranges`: [(offset, n)] enabled for the update rule (None: all).
    `noise`: vector added to the finished gradient inside the ranges' exact extents (zeros elsewhere).  The float32 evaluation feeds the
    rounded weights back in, as the kernel does."""
    dtype, dt = s.dtype, np.dtype(s.dtype).type
    p_in = s.p.astype(np.float32)
    gd, s.norm = finished_gradient(p_in, g, gsc=gsc, l2=l2, clip=clip, ranges=ranges, dtype=dtype, mutant=mutant)
    if mutant == "sgd_without_decay" and kind == "sgd":
        gd = gd - f32(l2, dt) * p_in.astype(dtype) * (f32(clip, dt) / dt(s.norm) if f32(clip, dt) / dt(s.norm) < 1 else dt(1))
    if noise is not None:
        gd = gd + np.asarray(noise).astype(dtype)
    s.grad = gd
    s.t += 1
    for o, n in ([(0, len(s.p))] if ranges is None else ranges):
        q = slice(o, o + n)
        gi = gd[q]
        if kind == "sgd":
            s.p[q] = s.p[q] - f32(lr, dt) * gi
            continue
        s.m[q] += f32(1 - B1, dt) * (gi - s.m[q])
        s.v[q] += f32(1 - B2, dt) * (gi * gi - s.v[q])
        s.vhat[q] = np.maximum(s.vhat[q], s.v[q]) if amsgrad and mutant != "no_max" else s.v[q]
        den = np.sqrt(s.vhat[q] + f32(EPS, dt)) if mutant == "eps_inside_sqrt" else np.sqrt(s.vhat[q]) + f32(EPS, dt)
        s.p[q] = s.p[q] - dt(np.float32(lr_t(lr, s.t))) * s.m[q] / den
    return s


# ------------------------------------------------------------------ the cases of tests/test_gpu_optimizer.py (and of the host test)
def weights(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.asarray(MAGS)[np.arange(n) % 3]).astype(np.float32)


def unit_gradients(n, steps, seed):
    rng = np.random.default_rng(seed + 1000)
    return [rng.standard_normal(n).astype(np.float32) for _ in range(steps)]


class Case:
    """One kernel-level case: weights, per-step gradients and hyper-parameters.  The gradient of step k is the unit draw times the first
    LADDER entry, cyclically from k, that leaves the float64 norm outside [0.5, 2] x clip -- so float32 and float64 (and the kernel) take
    the same side of the clip -- found by running the float64 reference alongside.  `ref` holds the reference after every step."""

    def __init__(self, name, n, *, kind="adam", steps=8, amsgrad=True, gsc=1.0, l2=1e-4, clip=2.0, lr=1e-3, zero=False, seed=0,
                 first=0):
        self.name, self.n, self.kind, self.steps, self.amsgrad = name, n, kind, steps, amsgrad
        self.gsc, self.l2, self.clip, self.lr, self.zero, self.seed, self.first = gsc, l2, clip, lr, zero, seed, first
        self._built = False

    @property
    def kw(self):
        return dict(kind=self.kind, amsgrad=self.amsgrad, gsc=self.gsc, l2=self.l2, clip=self.clip, lr=self.lr)

    def build(self):
        if self._built:
            return self
        self.p0 = weights(self.n, self.seed)
        self.grads, self.scales, self.ref = [], [], []
        s = State(self.p0)
        for k, z in enumerate(unit_gradients(self.n, self.steps, self.seed)):
            for j in range(len(LADDER)):
                sc = 0.0 if self.zero else LADDER[(self.first + k + j) % len(LADDER)]
                g = (z * np.float32(sc / self.gsc)).astype(np.float32)
                _, norm = finished_gradient(s.p, g, gsc=self.gsc, l2=self.l2, clip=self.clip)
                if self.zero or not 0.5 * self.clip <= norm <= 2.0 * self.clip:
                    break
            else:
                raise AssertionError(f"{self.name}: no ladder entry keeps step {k} clear of the clip threshold")
            self.grads.append(g)
            self.scales.append(sc)
            update(s, g, **self.kw)
            self.ref.append(dict(p=s.p.copy(), m=s.m.copy(), v=s.v.copy(), vhat=s.vhat.copy(), norm=s.norm))
        self._built = True
        return self

    def run(self, dtype=np.float64, mutant=None):
        """The trajectory under `dtype` / `mutant`: a list like `ref`."""
        self.build()
        s, out = State(self.p0, dtype), []
        for g in self.grads:
            update(s, g, mutant=mutant, **self.kw)
            out.append(dict(p=s.p.copy(), m=s.m.copy(), v=s.v.copy(), vhat=s.vhat.copy(), norm=s.norm))
        return out


def relerr(got, ref):
    """max |got - ref| relative to max |ref| (0 where the reference is identically 0 and so is `got`)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    if scale == 0.0:
        return 0.0 if err == 0.0 else np.inf
    return err / scale


_CASES = {}


def _reg(c):
    _CASES[c.name] = c
    return c


def adam_cases():
    """Every kernel-level Adam case of the GPU suite (built lazily, kept for the process)."""
    out = []
    for n in SIZES:
        out.append(_CASES.get(f"amsgrad-{n}") or _reg(Case(f"amsgrad-{n}", n, seed=n % 97)))
    for n in (5, 10007):
        for nm, kw in (("adam", dict(amsgrad=False)), ("noclip", dict(clip=NO_CLIP)), ("gsc", dict(gsc=GSC3)),
                       ("zero", dict(zero=True, l2=0.0, steps=1))):
            out.append(_CASES.get(f"{nm}-{n}") or _reg(Case(f"{nm}-{n}", n, seed=n % 89 + 1, first=3 if nm == "gsc" else 0, **kw)))
    return out


def sgd_cases():
    out = []
    for n in SIZES:
        for nm, kw in (("sgd", dict(first=0)), ("sgd-gsc", dict(first=3, gsc=GSC3))):
            out.append(_CASES.get(f"{nm}-{n}") or _reg(Case(f"{nm}-{n}", n, kind="sgd", steps=3, lr=0.05, seed=n % 83 + 2, **kw)))
    return out


def norm_inputs(n, l2, gsc, seed=5):
    """(p, g) of one clip-norm case."""
    rng = np.random.default_rng(seed + n % 101)
    return weights(n, seed + 7), (rng.standard_normal(n) * 0.01 / gsc).astype(np.float32)


NORM_PARAMS = [(l2, gsc) for l2 in (0.0, 1e-4) for gsc in (1.0, GSC3)]
HOOK_SIZES, HOOK_OFFSETS, HOOK_SIGMAS = (1, 2, 7, 10007), (0, 5, 2 ** 33 + 1), (0.0, 0.3)


def hook_inputs(n):
    """(p, g, l2, gsc, clip) of one noise-hook kernel case (the norm handed to the kernel is computed over these n: above the clip
    threshold at every size but n = 1)."""
    rng = np.random.default_rng(n + 11)
    return weights(n, n + 13), (rng.standard_normal(n) * 3.0 * 30.0).astype(np.float32), 1e-2, GSC3, 5.0


# ------------------------------------------------------------------ the arena of a model: offsets, ranges, the hook's noise
def arena_layout(shapes):
    """ast_amd.params.ParamArena's rule restated: every tensor starts on a multiple of 4 floats; (offsets, sizes, total)."""
    offsets, sizes, off = {}, {}, 0
    for name, shp in shapes.items():
        n = int(np.prod(shp))
        offsets[name], sizes[name] = off, n
        off += (n + 3) // 4 * 4
    return offsets, sizes, off


def enabled_ranges(shapes, frozen_links):
    """Merged contiguous (offset, padded n) ranges of the tensors whose link is not frozen."""
    offsets, sizes, _ = arena_layout(shapes)
    out = []
    for name in shapes:
        if name.split("/")[0] in frozen_links:
            continue
        o, n = offsets[name], (sizes[name] + 3) // 4 * 4
        if out and out[-1][0] + out[-1][1] == o:
            out[-1] = (out[-1][0], out[-1][1] + n)
        else:
            out.append((o, n))
    return out


def arena_noise(shapes, frozen_links, sigma, seed, offset):
    """(noise vector over the arena, next offset): optimizers.py's bookkeeping restated -- tensor by tensor over the exact extents, frozen
    links skipped (no draw, no counter consumed), pads zero, the pair counter advancing by (n + 1) // 2 per tensor."""
    from rng_model import hook_noise
    offsets, sizes, total = arena_layout(shapes)
    out = np.zeros(total, np.float64)
    for name in shapes:
        if name.split("/")[0] in frozen_links:
            continue
        n = sizes[name]
        out[offsets[name]:offsets[name] + n] = sigma * hook_noise(n, seed, offset)
        offset += (n + 1) // 2
    return out, offset


def noise_sigma(eta, t_before):
    """GradientNoise: sigma^2 = eta / (1 + t)^0.55 with the update count BEFORE the update."""
    return float(np.sqrt(eta / (1.0 + t_before) ** 0.55))


FREEZE = ("L0_enc", "out")


def arena_gradients(shapes, frozen_links, steps, seed=3):
    """Fixed random gradients over an arena, pads zero, the frozen links carrying most of the norm (scale 1 against 0.02)."""
    offsets, sizes, total = arena_layout(shapes)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        g = np.zeros(total, np.float32)
        for name in shapes:
            sc = 1.0 if name.split("/")[0] in frozen_links else 0.02
            g[offsets[name]:offsets[name] + sizes[name]] = rng.standard_normal(sizes[name]) * sc
        out.append(g)
    return out


def arena_vector(shapes, values):
    offsets, sizes, total = arena_layout(shapes)
    out = np.zeros(total, np.float32)
    for name in shapes:
        out[offsets[name]:offsets[name] + sizes[name]] = np.asarray(values[name], np.float32).ravel()
    return out


ARENA_HYPER = dict(l2=1e-4, clip=2.0)
ARENA_KINDS = {"adam": dict(kind="adam", amsgrad=True, lr=1e-3), "sgd": dict(kind="sgd", lr=0.05)}
NOISE_SEED, NOISE_ETA, ARENA_STEPS = 0x6E015E, 0.3, 4


def arena_run(shapes, p0, frozen_links, grads, kind, eta, dtype=np.float64, mutant=None):
    """The Python layer's updates (O.Adam / O.SGD with WeightDecay, GradientClipping and, for eta > 0, GradientNoise) over one arena:
    per step a dict of p, m, v, vhat, norm, grad (the finished gradient) and noise (the vector added; zeros without the hook)."""
    ranges = enabled_ranges(shapes, frozen_links)
    s, off, out = State(p0, dtype), 0, []
    for g in grads:
        noise = None
        if eta > 0:
            noise, off = arena_noise(shapes, frozen_links, noise_sigma(eta, s.t), NOISE_SEED, off)
        update(s, g, ranges=ranges, noise=noise, mutant=mutant, **ARENA_HYPER, **ARENA_KINDS[kind])
        out.append(dict(p=s.p.copy(), m=s.m.copy(), v=s.v.copy(), vhat=s.vhat.copy(), norm=s.norm, grad=s.grad.copy(),
                        noise=np.zeros(len(s.p)) if noise is None else noise))
    return out
