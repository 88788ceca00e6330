"""Float32-level accuracy gates for the direct layer-0 convolution k_conv0_fwd_x3 of ast_amd/csrc/conv.hip, shared by
tests/test_conv0_accuracy_host.py (CPU) and tests/test_gpu_conv0_accuracy.py (MI355X).  A helper, not a test module: nothing here touches a
GPU.  DESIGN.md section 40; the vocabulary is that of sections 38 and 39 (tests/gemm_accuracy_model.py).

The kernel, as conv.hip states it.  A workgroup owns a tile of TT = 80 output steps of one (b, f) and all channels; the noisy input
x * noise (a float32 product) of the tile lies in LDS as rows of JP = 20 columns (columns >= kf and rows outside [0, T) are zero), split
into three bf16 planes hi / mid / lo; output step t reads the 192 contiguous elements from 2 t * 20 on, so the product's k index is
k = i * 20 + j (time tap i, frequency tap j) and the weights are zero at j >= kf and i >= kt.  Six 32-k MFMA steps, per step six term
products (plane of W, plane of the window) in the order lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi.  The sequence is written out at
three code SITES: the even block of a pair of 16-step blocks (block index within the tile 0 or 2), the odd block (1 or 3) and the tail
block (4).  A wave holds 32 channels as two weight fragments wf[0] (the first 16) and wf[1] (the last 16): the channel HALVES.
model(): every term product of a 32-k step is summed exactly (float64) and the accumulator is rounded to float32 once per MFMA.

Y is reached without a hook: a one-layer stack with no_bn = 1 and a zero bias gives out = relu(Y), run with W and with -W, and
Y_hat = out(W) - out(-W) is every entry of Y (one of the two terms is an exact zero).

Gates:
 (a) selection identities, bit for bit.  Forward: full-mantissa window, weights with one +-2^e per channel at tap seq[(c + p) % (kt kf)]
     of pass p -- every output is 2^e times the selected noisy input element (selection_fwd()).  Window (XF): a bias that makes every unit
     active, an upstream gradient with one +-2^e per channel at one output position -- CNN_0/W's gradient is 2^e times that position's
     kt x kf patch, dbias the sum of the upstream gradient (selection_xf()).
 (b) error gate: N(0,1) window over four decades per frequency bin, N(0,1) weights; |Y_hat - ref| of every entry over its own
     sqrt(sum_k x^2 w^2) against TOL[kt] = 4 x the worst figure of model() over the cases of that kt (F32_MODEL_ERR).
 (c) projection gates: c = <got - ref, p> / <p, p> for p = exact(mutant) - ref must stay within C_GATE on every direction of directions().
 (d) the fused BatchNorm statistics (bn_decay = 0: avg_mean / avg_var are the batch statistics, undiluted) against the float64 statistics
     of the reference Y, on a benign and an offset draw, within STAT_TOL = 4 x the worst figure of stats_model(), the kernel's own
     summation in float32; on the benign draw the post-BatchNorm output, dW and dgamma / dbeta within BN_TOL (f32_bn_step()).
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import gemm_accuracy_model as G

JP, TT, NKS, KW = 20, 80, 6, 192
TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))        # (plane of W, plane of the window) per MFMA of a 32-k step
PLANES = ("hi", "mid", "lo")
SITE_OF_BLOCK = (0, 1, 0, 1, 2)                                  # 16-step block of a tile -> the code site that multiplies it
SITE_NAMES = ("even", "odd", "tail")
C_GATE, C_F32_MAX, C_MUTANT_MIN, COS_MAX = 0.25, 0.1, 0.8, 0.1
PREC_BF16X3 = 2                                                  # ASTK_PREC_BF16X3, through the descriptor's `precision`
DIRECT_MSG = "took the direct-convolution layer-0 path"

# name, layer-0 geometry, input shape, speech noise
Case = namedtuple("Case", "name C kt kf st sf pt B T D noise")
CASES = [
    # the base shape: B = 2, F' = 2, 167 output steps = three tiles per (b, f), the last with 7 steps; all four waves full
    Case("base-c128", 128, 9, 13, 2, 13, 4, 2, 333, 26, False),
    Case("c48-noise", 48, 9, 13, 2, 13, 4, 2, 333, 26, True),          # the second wave holds half its channels
    Case("kf14-sf7-pt0", 16, 9, 14, 2, 7, 0, 2, 341, 21, False),       # kf = the maximum (no pad column in XF), overlapping windows, no time pad
    Case("kt5-kf8-noise", 32, 5, 8, 2, 8, 4, 2, 333, 16, True),        # even kf, pt = kt - 1, 169 steps (last tile 9)
    Case("kf1", 16, 9, 1, 2, 1, 4, 2, 333, 2, False),                  # JG = 2; waves 1 to 3 hold no channel
    Case("kt2-pt0", 16, 2, 13, 2, 13, 0, 2, 334, 26, False),           # kt == st, no time pad
    Case("gaps-pt8-noise", 32, 9, 5, 2, 9, 8, 2, 333, 14, True),       # sf > kf: uncovered bins; pt = kt - 1, 171 steps (last tile 11)
    # 720 one-tile groups of 10 steps: more tiles than twice the CU count, so a workgroup runs a second and third tile
    Case("tile-loop", 16, 9, 1, 2, 1, 4, 9, 20, 80, False),
]
FWD_SELECTION_ROWS = ("base-c128", "c48-noise", "kf14-sf7-pt0", "kt5-kf8-noise", "kf1", "kt2-pt0", "tile-loop")
XF_SELECTION_ROWS = ("base-c128", "kf14-sf7-pt0", "kt2-pt0", "tile-loop")
STAT_ROWS = ("base-c128", "c48-noise", "kf14-sf7-pt0", "tile-loop")

# Worst |model - ref| / scale over the cases of a kt, printed by test_float32_model_error_is_what_the_tolerances_were_taken_from, and
# TOL = 4 x that (the standing margin of sections 23, 38 and 39: it covers another summation order inside an MFMA).  Measured on the CPU.
F32_MODEL_ERR = {9: 1.2e-6, 5: 4.9e-7, 2: 5.2e-7}
TOL = {k: 4.0 * v for k, v in F32_MODEL_ERR.items()}
# Gate (d), per row of STAT_ROWS (the rows differ in how many tiles and steps a sum runs over): the worst figure of stats_model() over both
# draws -- the mean over the channel's standard deviation, the variance relative -- and of f32_bn_step() on the benign draw, every entry
# over the largest of its tensor.  Tolerance = 4 x the figure, as above.
STAT_MODEL_ERR = {      # (the mean's figure is the float32 STORAGE of avg_mean on the offset draw: 6e-8 x 170 standard deviations)
    "base-c128": {"mean": 9.2e-6, "var": 6.5e-7}, "c48-noise": {"mean": 4.0e-6, "var": 4.2e-7},
    "kf14-sf7-pt0": {"mean": 2.8e-6, "var": 2.7e-7}, "tile-loop": {"mean": 2.2e-6, "var": 4.9e-6},
}
BN_MODEL_ERR = {
    "base-c128": {"out": 2.5e-7, "dW": 5.2e-7, "dparam": 8.2e-7}, "c48-noise": {"out": 1.8e-7, "dW": 6.4e-7, "dparam": 5.2e-7},
    "kf14-sf7-pt0": {"out": 1.7e-7, "dW": 4.2e-7, "dparam": 5.2e-7}, "tile-loop": {"out": 1.4e-6, "dW": 2.3e-6, "dparam": 1.7e-6},
}
STAT_TOL = {n: {k: 4.0 * v for k, v in row.items()} for n, row in STAT_MODEL_ERR.items()}
BN_TOL = {n: {k: 4.0 * v for k, v in row.items()} for n, row in BN_MODEL_ERR.items()}


def by_name(name):
    return next(c for c in CASES if c.name == name)


def direct_shape(c):
    """conv.hip's conv0_direct_shape restated.  The LDS window of an 80-step tile is st * 20 * 79 + 232 elements and has to fit 4096: with
    the even-stride rule st = 2 is the ONLY stride the kernel admits (st = 4: 6552)."""
    win = c.st * JP * (TT - 1) + 32 * NKS + 40
    return (win <= 512 * 8 and c.C * c.kt * c.kf * 4 <= 64 * 1024 and c.kt * JP <= 32 * NKS and c.kf <= 14 and c.st % 2 == 0 and c.C <= 128
            and c.C % 16 == 0)


def dims(c):
    """-> F', T', tiles per (b, f), tiles in all."""
    F = (c.D - c.kf) // c.sf + 1
    T1 = (c.T + 2 * c.pt - c.kt) // c.st + 1
    tiles_t = (T1 + TT - 1) // TT
    return F, T1, tiles_t, c.B * F * tiles_t


def layer(c):
    return [(c.C, c.kt, c.kf, c.st, c.sf, c.pt)]


def cfg_of(c, bn):
    import range_cases as RC
    cfg = RC.cnn_geometry_cfg(layer(c))
    cfg["cnn_config"]["bn"] = bool(bn)
    return cfg


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------ windows, weights in the kernel's k order
def noisy(X, noise):
    """The float32 product the kernel forms; every reference starts from it."""
    X = np.asarray(X, np.float32)
    return X if noise is None else (X * np.asarray(noise, np.float32)).astype(np.float32)


def windows(c, xn, rows_i=None):
    """xn (B, T, D) float32 -> (B, F', T', rows_i, kf): rows 2 t1 - pt + i of the time-padded input, bins f sf + j.  rows_i defaults to kt;
    the LDS image holds the rows behind a patch too (rows_i = 10 covers the 192 k of the MFMA steps)."""
    F, T1, _, _ = dims(c)
    n = c.kt if rows_i is None else rows_i
    xp = np.zeros((c.B, c.st * (T1 - 1) + n + 1, c.D), np.float32)
    hi = min(c.T, xp.shape[1] - c.pt)
    xp[:, c.pt:c.pt + hi] = xn[:, :hi]
    ti = c.st * np.arange(T1)[:, None] + np.arange(n)[None, :]                   # (T', n)
    fj = c.sf * np.arange(F)[:, None] + np.arange(c.kf)[None, :]                 # (F', kf)
    return xp[:, ti[None, :, :, None], fj[:, None, None, :]]                     # (B, F', T', n, kf)


def window_k(c, xn):
    """-> (B F' T', 192) float32: what output step (b, f, t1) multiplies, in the kernel's k order (zero pad columns)."""
    w = windows(c, xn, 10)
    out = np.zeros(w.shape[:3] + (10, JP), np.float32)
    out[..., :c.kf] = w
    return out.reshape(-1, 10 * JP)[:, :KW]


def weight_k(c, W):
    """W (C, kt, kf) -> (C, 192) float32 in the kernel's k order."""
    out = np.zeros((c.C, 10, JP), np.float32)
    out[:, :c.kt, :c.kf] = np.asarray(W, np.float32).reshape(c.C, c.kt, c.kf)
    return out.reshape(c.C, 10 * JP)[:, :KW]


def sites(c):
    """Per output row (b, f, t1): the code site that multiplies it."""
    F, T1, _, _ = dims(c)
    s = np.array(SITE_OF_BLOCK)[(np.arange(T1) % TT) // 16]
    return np.tile(s, c.B * F)


def halves(c):
    return (np.arange(c.C) % 32) // 16


def planes(x):
    return G.planes(x, "bf16x3")[0]


def reference(c, W, xn):
    """float64 on the float32 inputs -> (B F' T', C)."""
    w = windows(c, xn).astype(np.float64).reshape(-1, c.kt * c.kf)
    return w @ np.asarray(W, np.float64).reshape(c.C, -1).T


def entry_scale(c, W, xn):
    w = windows(c, xn).astype(np.float64).reshape(-1, c.kt * c.kf)
    s = np.sqrt((w ** 2) @ (np.asarray(W, np.float64).reshape(c.C, -1) ** 2).T)
    return np.where(s > 0, s, 1.0)


def to_rows(c, out):
    """The output's (T', B, C F') layout (feature index c F' + f) -> (B F' T', C)."""
    F, T1, _, _ = dims(c)
    return np.asarray(out).reshape(T1, c.B, c.C, F).transpose(1, 3, 0, 2).reshape(-1, c.C)


def from_rows(c, rows):
    F, T1, _, _ = dims(c)
    return np.asarray(rows).reshape(c.B, F, T1, c.C).transpose(2, 0, 3, 1).reshape(T1, c.B, c.C * F)


# ------------------------------------------------------------------ the float32 model and its mutants
# A mutant: ("drop", term, site | None, half | None)  the term product left out at a code site / in a channel half (None: everywhere)
#           ("zero", "w" | "x", plane, half | None)   a plane lost
#           ("shift-w",)                              the weight fragments' k order off by one pad column
#           ("x-lo-swap",)                            the window's lo plane read from the neighbouring 32-k step (ks ^ 1)
def mutant_name(m):
    if m[0] == "drop":
        a, b = TERMS[m[1]]
        return (f"w.{PLANES[a]} x x.{PLANES[b]} missing" + ("" if m[2] is None else f" in the {SITE_NAMES[m[2]]} block")
                + ("" if m[3] is None else f", wf[{m[3]}]"))
    if m[0] == "zero":
        return f"{m[1]}.{PLANES[m[2]]} lost" + ("" if m[3] is None else f" in wf[{m[3]}]")
    return m[0]


def model(c, Wk, Pk, mutant=None, f32=True):
    """Wk (C, 192), Pk (rows, 192) float32 -> (rows, C) float64.  f32: one rounding per MFMA; else the same terms summed exactly."""
    kind = mutant[0] if mutant else None
    if kind == "shift-w":
        Wk = np.roll(Wk, 1, axis=1)
    wp = [p.reshape(c.C, NKS, 32) for p in planes(Wk)]
    xp = [p.reshape(-1, NKS, 32) for p in planes(Pk)]
    st, hv = sites(c), halves(c)
    if kind == "zero":
        _, op, pl, half = mutant
        if op == "w":
            wp[pl] = wp[pl] * (np.zeros(c.C) if half is None else (hv != half))[:, None, None]
        else:
            xp[pl] = np.zeros_like(xp[pl])
    xlo = xp[2][:, [1, 0, 3, 2, 5, 4]] if kind == "x-lo-swap" else xp[2]
    rnd = _f32 if f32 else (lambda v: v)
    acc = np.zeros((Pk.shape[0], c.C))
    for ks in range((c.kt * JP + 31) // 32 if kind != "x-lo-swap" else NKS):      # (the steps behind kt * 20 multiply zero weights)
        for t, (a, b) in enumerate(TERMS):
            x = xlo if b == 2 else xp[b]
            T = x[:, ks] @ wp[a][:, ks].T
            if kind == "drop" and mutant[1] == t:
                keep = np.ones((Pk.shape[0], c.C), bool)
                rs = np.ones(Pk.shape[0], bool) if mutant[2] is None else st == mutant[2]
                cs = np.ones(c.C, bool) if mutant[3] is None else hv == mutant[3]
                keep[np.ix_(rs, cs)] = False
                T = T * keep
            acc = rnd(acc + T)
    return acc


def directions(c):
    """Gate (c).  Each of the three low terms missing at each code site the case's rows reach; w.lo x x.hi per channel half as well, so
    that the supports are disjoint.  MERGED: `the weights' lo plane lost in wf[h]` is the sum of the (w.lo x x.hi, site, wf[h]) directions
    over the sites and `the window's lo plane lost` the sum of the (w.hi x x.lo, site) directions -- their cosines with a site direction
    are 0.4 .. 0.6 at any shape, so they are not directions of their own; a kernel with such a defect has c = 1 on every component
    (shown by the host test)."""
    reach = sorted(set(sites(c).tolist()))
    hs = sorted(set(halves(c).tolist()))
    out = [("drop", 0, s, h) for s in reach for h in hs]
    out += [("drop", t, s, None) for t in (1, 2) for s in reach]
    return out


def components(c, m):
    """The directions on which a merged defect must show."""
    ds = directions(c)
    if m[0] == "zero" and m[1] == "w" and m[2] == 2:
        return [d for d in ds if d[1] == 0 and (m[3] is None or d[3] == m[3])]
    if m[0] == "zero" and m[1] == "x" and m[2] == 2:
        return [d for d in ds if d[1] == 1]
    raise AssertionError(m)


GATE_B_MUTANTS = [("zero", "w", 1, None), ("zero", "x", 1, None), ("drop", 3, None, None), ("shift-w",)]


def coefficient(got, ref, p, scale):
    return G.coefficient(got, ref, p, scale)


# ------------------------------------------------------------------ draws
@functools.lru_cache(maxsize=None)
def dense(name):
    """Gates (b), (c): -> W (C, kt, kf), X, noise (float32; noise None where the case has none)."""
    c = by_name(name)
    rng = np.random.default_rng(_seed("dense", name))
    X = (rng.standard_normal((c.B, c.T, c.D)) * 10.0 ** (-(np.arange(c.D) % 4))[None, None, :]).astype(np.float32)
    W = rng.standard_normal((c.C, c.kt, c.kf)).astype(np.float32)
    noise = rng.normal(1.0, 0.25, X.shape).astype(np.float32) if c.noise else None
    return W, X, noise


@functools.lru_cache(maxsize=None)
def dense_parts(name):
    """-> Wk, Pk, reference, scale of the dense draw (computed once, shared)."""
    c = by_name(name)
    W, X, noise = dense(name)
    xn = noisy(X, noise)
    return weight_k(c, W), window_k(c, xn), reference(c, W, xn), entry_scale(c, W, xn)


def tap_sequence(c):
    """The taps (i, j) of a case, those on both sides of every 32-k step boundary (k = i * 20 + j) first."""
    taps = [(i, j) for i in range(c.kt) for j in range(c.kf)]
    k = lambda t: t[0] * JP + t[1]
    first = []
    for b in range(32, c.kt * JP, 32):
        below = [t for t in taps if k(t) < b]
        above = [t for t in taps if k(t) >= b]
        first += ([max(below, key=k)] if below else []) + ([min(above, key=k)] if above else [])
    first = list(dict.fromkeys(first))
    return first + [t for t in taps if t not in first]


@functools.lru_cache(maxsize=None)
def heavy_input(name, what):
    """Full 24-bit mantissas, heavy-tailed like gemm_accuracy_model's; values whose three bf16 planes do not reconstruct them under
    every order of adding them are redrawn.  -> X, noise, xn (float32), the share of redrawn values.  With noise, X and the noise are
    powers of two times such values so that the float32 PRODUCT is the full-mantissa value the identities are about."""
    c = by_name(name)
    rng = np.random.default_rng(_seed("heavy", name, what))
    xn = G._heavy(rng, (c.B, c.T, c.D), "bf16x3")
    if what == "xf":                       # (the bias has to dominate Y: a narrower range)
        xn = np.clip(np.abs(xn), 2.0 ** -10, 2.0 ** 10).astype(np.float32) * np.sign(xn).astype(np.float32)
    redrawn = 0
    for _ in range(20):
        bad = ~G.exact_under_every_order(xn, "bf16x3")
        if not bad.any():
            break
        redrawn += int(bad.sum())
        v = G._heavy(rng, (int(bad.sum()),), "bf16x3")
        xn[bad] = np.clip(np.abs(v), 2.0 ** -10, 2.0 ** 10).astype(np.float32) * np.sign(v).astype(np.float32) if what == "xf" else v
    assert G.exact_under_every_order(xn, "bf16x3").all()
    if c.noise:
        noise = (2.0 ** rng.integers(-2, 3, size=xn.shape)).astype(np.float32)
        X = (xn / noise).astype(np.float32)
        assert np.array_equal(noisy(X, noise), xn)
    else:
        noise, X = None, xn
    return X, noise, xn, redrawn / xn.size


def selection_fwd(name, p):
    """Gate (a), forward, pass p of kt * kf: -> W (C, kt, kf) with one +-2^e per channel, the expected Y (B F' T', C) float32, exact."""
    c = by_name(name)
    _, _, xn, _ = heavy_input(name, "fwd")
    seq = tap_sequence(c)
    rng = np.random.default_rng(_seed("sel", name, p))
    val = (2.0 ** rng.integers(-3, 4, size=c.C) * rng.choice([-1.0, 1.0], size=c.C)).astype(np.float32)
    W = np.zeros((c.C, c.kt, c.kf), np.float32)
    taps = [seq[(ch + p) % len(seq)] for ch in range(c.C)]
    ii, jj = np.array([t[0] for t in taps]), np.array([t[1] for t in taps])
    W[np.arange(c.C), ii, jj] = val
    w = windows(c, xn)                                              # (B, F', T', kt, kf)
    expect = w[:, :, :, ii, jj].astype(np.float64) * val.astype(np.float64)
    assert (expect.astype(np.float32).astype(np.float64) == expect).all()
    return W, expect.astype(np.float32).reshape(-1, c.C)


def position_sequence(c):
    """Output rows (b, f, t1) as flat indices, the first and last step of every tile first."""
    F, T1, tiles_t, _ = dims(c)
    first = []
    for g in range(c.B * F):
        for t in range(tiles_t):
            first += [g * T1 + t * TT, g * T1 + min(T1, (t + 1) * TT) - 1]
    first = list(dict.fromkeys(first))
    seen = set(first)
    return first + [r for r in range(c.B * F * T1) if r not in seen]


def xf_passes(c):
    F, T1, _, _ = dims(c)
    return (c.B * F * T1 + c.C - 1) // c.C


@functools.lru_cache(maxsize=None)
def xf_setup(name):
    """Gate (a), window: -> W (small, dense), bias (one power of two for every channel, at least twice the largest |Y| of the reference:
    every unit is active), the reference Y."""
    c = by_name(name)
    _, _, xn, _ = heavy_input(name, "xf")
    rng = np.random.default_rng(_seed("xfw", name))
    W = (rng.standard_normal((c.C, c.kt, c.kf)) * 2.0 ** -6).astype(np.float32)
    Y = reference(c, W, xn)
    bias = np.full(c.C, 2.0 ** np.ceil(np.log2(2.0 * np.abs(Y).max() + 1.0)), np.float32)
    return W, bias, Y


def selection_xf(name, p):
    """Pass p: -> the upstream gradient (T', B, C F') float32 with one +-2^e per channel, the expected dW (C, kt, kf) and dbias (C,)."""
    c = by_name(name)
    _, _, xn, _ = heavy_input(name, "xf")
    seq = position_sequence(c)
    rng = np.random.default_rng(_seed("selxf", name, p))
    val = (2.0 ** rng.integers(-3, 4, size=c.C) * rng.choice([-1.0, 1.0], size=c.C)).astype(np.float32)
    rows = np.array([seq[(p * c.C + ch) % len(seq)] for ch in range(c.C)])
    g = np.zeros((len(seq), c.C), np.float32)
    g[rows, np.arange(c.C)] = val
    w = windows(c, xn).reshape(-1, c.kt, c.kf)
    dW = w[rows].astype(np.float64) * val.astype(np.float64)[:, None, None]
    assert (dW.astype(np.float32).astype(np.float64) == dW).all()
    return from_rows(c, g), dW.astype(np.float32), val, rows


# ------------------------------------------------------------------ gate (d): the fused statistics
def bn_draws(name, offset):
    """-> cfg, P (float64 values that are float32 numbers), X, noise (float32), the upstream-gradient generator.  benign: range_cases.cnn_draws
    as the operator tests draw it; offset: x_offset = 64, ramp = False, centre_taps = True -- channel means tens of standard deviations out.
    The offset draw has no speech noise on any row: a multiplicative N(1, 0.25) on an offset of 64 IS a spread of 16, and the channel
    means would lie 8 standard deviations out, not tens."""
    import range_cases as RC
    c = by_name(name)
    kw = dict(x_offset=64.0, ramp=False, centre_taps=True) if offset else {}
    cfg, P, X, noise, rng = RC.cnn_draws(c.B, c.T, c.D, None, None, c.noise and not offset, seed=_seed("bn", name) % 1000, layers=layer(c), **kw)
    P = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in P.items()}
    X = np.asarray(X, np.float32)
    noise = None if noise is None else np.asarray(noise, np.float32)
    return cfg, P, X, noise, rng


def stats_reference(Y):
    """Y (rows, C) float64 -> mean, unbiased variance (what avg_mean / avg_var hold under bn_decay = 0), m."""
    return Y.mean(axis=0), Y.var(axis=0, ddof=1), Y.shape[0]


def pivots(c, W, X, noise):
    """The kernel's pivot: the channel's tap sum times the mean of the input's first kf values, float32 sums in index order."""
    f = np.float32
    xs = f(0)
    x0, n0 = np.asarray(X, f).reshape(-1)[:c.kf], (None if noise is None else np.asarray(noise, f).reshape(-1)[:c.kf])
    for j in range(c.kf):
        xs = f(xs + (x0[j] if n0 is None else f(x0[j] * n0[j])))
    wsum = np.zeros(c.C, f)
    Wf = np.asarray(W, f).reshape(c.C, -1)
    for k in range(Wf.shape[1]):
        wsum = (wsum + Wf[:, k]).astype(f)
    return (wsum * f(xs / f(c.kf))).astype(f)


def stats_model(c, Y32, piv, mutant=None):
    """The kernel's own summation.  Y32 (B F' T', C): the float32 convolution output.  Per tile and channel, the lane of output-step
    residue r adds its steps' deviations d = y - pivot in float32 (sum d, and sum d^2 through an fma); the 16 lanes fold in a butterfly
    (xor 8, 4, 2, 1); one row per tile; k_colstats_tiles adds the rows in float32 in colreduce_block's order (one row slab at these
    sizes, asserted) and emits the raw sums in double: sum y = s + n p, sum y^2 = q + 2 p s + n p^2.  -> mean, variance (biased), float64.
    mutant "raw": one-pass float32 sums of y and y^2 (no pivot); "cum80": the last ragged tile counted as 80 steps in cum()."""
    f = np.float32
    F, T1, tiles_t, total = dims(c)
    Y = np.asarray(Y32, f).reshape(c.B * F, T1, c.C)
    p = np.zeros(c.C, f) if mutant == "raw" else np.asarray(piv, f)
    pad = np.zeros((c.B * F, tiles_t * TT, c.C), f)
    valid = np.zeros((c.B * F, tiles_t * TT, 1), bool)
    pad[:, :T1] = (Y - p[None, None, :]).astype(f)
    valid[:, :T1] = True
    d = pad.reshape(c.B * F * tiles_t, TT // 16, 16, c.C)                # (tile, block, lane r, channel)
    sa = np.zeros((d.shape[0], 16, c.C), f)
    qa = np.zeros_like(sa)
    for ti in range(TT // 16):                                           # (steps past T' add an exact zero)
        sa = (sa + d[:, ti]).astype(f)
        qa = (qa.astype(np.float64) + d[:, ti].astype(np.float64) ** 2).astype(f)
    for o in (8, 4, 2, 1):
        idx = np.arange(16) ^ o
        sa, qa = (sa + sa[:, idx]).astype(f), (qa + qa[:, idx]).astype(f)
    rows = np.stack([sa[:, 0], qa[:, 0]], axis=1)                        # (tiles, 2, C)
    # colreduce_block<2>: CL column lanes, NR row lanes; row lane rl adds rows rl, rl + NR, ... in order; then lane 0 adds the NR partials
    q4 = (c.C + 3) // 4
    CL = min(q4, 16)
    NR = 256 // CL
    assert (total + 16 * NR - 1) // (16 * NR) == 1, "more than one row slab: the model would need the launch's grid"
    part = np.zeros((NR, 2, c.C), f)
    for r in range(total):
        part[r % NR] = (part[r % NR] + rows[r]).astype(f)
    tot = part[0].copy()
    for k in range(1, NR):
        tot = (tot + part[k]).astype(f)
    n = float(c.B * F * (tiles_t * TT if mutant == "cum80" else T1))
    s, q, pe = tot[0].astype(np.float64), tot[1].astype(np.float64), p.astype(np.float64)
    s0, s1 = s + n * pe, q + 2.0 * pe * s + n * pe * pe
    m = float(c.B * F * T1)
    mu = s0 / m
    var = np.maximum(s1 / m - mu * mu, 0.0)
    # bn_finalize_channel with bn_decay = 0: what the call leaves in avg_mean / avg_var, float32 numbers
    return _f32(mu), _f32(var * (m / (m - 1.0))), mu, var


def stat_errors(mean, var, ref_mean, ref_var):
    """-> the worst mean error over the channel's standard deviation, the worst relative variance error."""
    return float((np.abs(mean - ref_mean) / np.sqrt(ref_var)).max()), float((np.abs(var - ref_var) / ref_var).max())


def bn_reference(c, cfg, P, X, noise):
    """float64 training-mode step on the float32 inputs -> out, upstream gradient (zero at the reference's near-kink units), dW, dgamma,
    dbeta -- oracle.ast_ref_torch.cnn_torch and autograd."""
    import torch
    import range_cases as RC
    from oracle.ast_ref_torch import cnn_torch
    Pt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=k.startswith("CNN") and "avg" not in k) for k, v in P.items()}
    xn64 = noisy(X, noise).astype(np.float64)                    # the float32 product: the reference starts from it
    near = RC.cnn_bn_inputs(cfg, P, xn64, None)[0][1].abs() < 2e-5
    out = cnn_torch(cfg, Pt, torch.tensor(xn64), None)
    gout = np.random.default_rng(_seed("gout", c.name)).standard_normal(tuple(out.shape))
    gout[RC.seq_layout(near).numpy()] = 0.0
    gout = gout.astype(np.float32)
    out.backward(torch.tensor(gout.astype(np.float64)))
    return (out.detach().numpy(), gout, Pt["CNN_0/W"].grad.numpy().reshape(c.C, c.kt, c.kf), Pt["CNN_0_bn/gamma"].grad.numpy(),
            Pt["CNN_0_bn/beta"].grad.numpy())


def f32_bn_step(c, P, Y32, mean, var, gout, xn, eps=2e-5):
    """A float32 evaluation of the step behind the convolution: scale / shift from the modelled statistics, relu(fma(y, scale, shift)),
    the ReLU + BatchNorm backward with float32 column sums, and the weight gradient as the library forms it -- a bf16x3 product of dY^T
    and the windows (gemm_accuracy_model.product, 128-tile kernel).  -> out (T', B, C F'), dW (C, kt, kf), dgamma, dbeta, as float64."""
    f = np.float32
    gamma, beta = P["CNN_0_bn/gamma"].astype(f), P["CNN_0_bn/beta"].astype(f)
    mu = mean.astype(f)
    inv = (1.0 / np.sqrt(var + float(f(eps)))).astype(f)
    sc = (gamma * inv).astype(f)
    sh = (beta - (mu * sc).astype(f)).astype(f)
    Y = np.asarray(Y32, f)
    z = (Y.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)).astype(f)
    out = np.maximum(z, f(0))
    g = (to_rows(c, gout).astype(f) * (z > 0)).astype(f)
    xh = ((Y - mu[None, :]).astype(f) * inv[None, :]).astype(f)
    m = f(Y.shape[0])
    dbeta = g.sum(axis=0, dtype=f)
    dgamma = (g * xh).astype(f).sum(axis=0, dtype=f)
    dy = (sc[None, :] * (g - ((dbeta[None, :] + (xh * dgamma[None, :]).astype(f)).astype(f) / m).astype(f)).astype(f)).astype(f)
    w = windows(c, xn).reshape(-1, c.kt * c.kf)
    dW = G.product(np.ascontiguousarray(dy.T), np.ascontiguousarray(w.T), "bf16x3", 128, 128)
    return from_rows(c, out).astype(np.float64), dW.reshape(c.C, c.kt, c.kf), dgamma.astype(np.float64), dbeta.astype(np.float64)


def tensor_error(got, ref):
    """Every entry over the largest of its tensor."""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(float(np.abs(ref).max()), 1e-30))
