"""The definition of astk_resample (include/astk.h) in NumPy float64, and the named cases of its tests.

Band-limited resampling by the rational ratio out_rate / in_rate = q / p with a Hann-windowed sinc.  Parity with sox / Kaldi is
unpinned (Kaldi perturbs speed with sox, which does not exist here); tests/test_resample_host.py pins this model independently,
against scipy.signal.upfirdn and against what a resampler must do to a sine and to a constant.

    c = rolloff * min(1, q / p),  K = ceil(Z / c)                        (p, q reduced by their gcd; Z = num_zeros)
    g(t) = c sinc(c t) cos^2(pi c t / (2 Z)) for |c t| < Z, else 0;  sinc(u) = sin(pi u) / (pi u)
    n_out = ceil(n_in q / p)
    y[m] = sum over k = -K+1 .. K of x[n0 + k] g(phi / q - k),  n0 = (m p) div q,  phi = (m p) mod q;  x = 0 outside [0, n_in)

The sum runs in ascending k in float64 and is rounded once to float32.  sin(pi u) is evaluated on u folded into [-1/2, 1/2] (exact
steps), so it is exactly 0 at the integers as the device's sinpi is: the ratio 1/1 with rolloff 1 is the identity bit for bit."""
import functools
import math
from fractions import Fraction

import numpy as np

TILE = 256                 # astk.h ASTK_RESAMPLE_TILE
MAX_PHASES, MAX_HALF_TAPS = 1024, 256


def reduced(p, q):
    g = math.gcd(int(p), int(q))
    return int(p) // g, int(q) // g


def constants(p, q, num_zeros=6, rolloff=0.99):
    """(P, Q, c, K) of a ratio."""
    P, Q = reduced(p, q)
    c = rolloff * (Q / P if Q < P else 1.0)
    return P, Q, c, int(math.ceil(num_zeros / c))


def speed_ratio(factor):
    """p / q of a speed factor: Fraction(str(factor))."""
    f = Fraction(str(factor))
    return f.numerator, f.denominator


def sinpi(u):
    """sin(pi u) with u folded into [-1/2, 1/2] first: u - 2 round(u / 2) lies in [-1, 1] and every step is exact."""
    u = np.asarray(u, np.float64)
    r = u - 2.0 * np.round(u / 2.0)
    r = np.where(r > 0.5, 1.0 - r, np.where(r < -0.5, -1.0 - r, r))
    return np.sin(np.pi * r)


def g(t, c, num_zeros):
    u = c * np.asarray(t, np.float64)
    safe = np.where(u == 0.0, 1.0, u)
    sinc = np.where(u == 0.0, 1.0, sinpi(u) / (np.pi * safe))
    cw = np.cos(np.pi * (u / (2.0 * num_zeros)))
    return np.where(np.abs(u) < num_zeros, c * sinc * (cw * cw), 0.0)


def table(p, q, num_zeros=6, rolloff=0.99):
    """(2K, Q): g(phi / Q - k) at [k + K - 1][phi]."""
    P, Q, c, K = constants(p, q, num_zeros, rolloff)
    k = np.arange(-K + 1, K + 1, dtype=np.float64)[:, None]
    phi = np.arange(Q, dtype=np.float64)[None, :]
    return g(phi / float(Q) - k, c, num_zeros)


def n_out(n_in, p, q):
    P, Q = reduced(p, q)
    return -((-int(n_in) * Q) // P)


def resample64(x, p, q, num_zeros=6, rolloff=0.99):
    """The float64 sums of one row (before the rounding to float32)."""
    x = np.asarray(x).astype(np.float64)
    P, Q, c, K = constants(p, q, num_zeros, rolloff)
    tab = table(p, q, num_zeros, rolloff)
    n, M = len(x), n_out(len(x), p, q)
    mp = np.arange(M, dtype=np.int64) * P
    n0, phi = mp // Q, mp % Q
    acc = np.zeros(M, np.float64)
    for j in range(2 * K):                                     # ascending k
        idx = n0 - K + 1 + j
        inside = (idx >= 0) & (idx < n)
        xv = np.where(inside, x[np.clip(idx, 0, max(n - 1, 0))] if n else 0.0, 0.0)
        acc = acc + xv * tab[j, phi]
    return acc


def resample(x, p, q, num_zeros=6, rolloff=0.99):
    return resample64(x, p, q, num_zeros, rolloff).astype(np.float32)


def batch_resample(c):
    """(out (B, Mmax) float32, n_out (B) int32, n_bad) of a case: what astk_resample must write."""
    B, Nmax = c["wave"].shape
    out = np.zeros((B, c["Mmax"]), np.float32)
    counts = np.full(B, -1, np.int32)
    for b, n in enumerate(c["n_samples"].tolist()):
        if n < 0 or n > Nmax or n_out(n, c["p"], c["q"]) > c["Mmax"]:
            continue
        y = resample(c["wave"][b, :n], c["p"], c["q"], c["num_zeros"], c["rolloff"])
        out[b, :len(y)] = y
        counts[b] = len(y)
    return out, counts, int((counts < 0).sum())


# ------------------------------------------------------------------ the named cases
def n_with_out(M, p, q):
    """An input length whose output count is exactly M."""
    P, Q = reduced(p, q)
    for n in range(max(0, M * P // Q - 2), M * P // Q + 3):
        if n_out(n, p, q) == M:
            return n
    raise ValueError(f"no input length gives {M} output samples at {p}/{q}")


def gauss(rng, n, sigma=3000.0):
    return np.clip(np.round(rng.standard_normal(n) * sigma), -32768, 32767)


def tone(n, freq, sr, amp=32767.0):
    return np.round(amp * np.sin(2.0 * np.pi * freq / sr * np.arange(n)))


def _case(rows, p, q, num_zeros=6, rolloff=0.99, dtype=np.int16, fill=0, extra=3, Mmax=None, n_samples=None):
    Nmax = max(1, max(len(r) for r in rows) + extra)
    wave = np.full((len(rows), Nmax), fill, dtype=dtype)
    for b, r in enumerate(rows):
        wave[b, :len(r)] = np.asarray(r).astype(dtype)
    n = np.asarray([len(r) for r in rows] if n_samples is None else n_samples, np.int32)
    good = [n_out(v, p, q) for v in n.tolist() if 0 <= v <= Nmax]
    return dict(wave=wave, n_samples=n, p=p, q=q, num_zeros=num_zeros, rolloff=rolloff, Mmax=Mmax or max(1, max(good) if good else 1))


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % (2 ** 31)
    return h


RATIO_CASES = {"r9-10": (9, 10), "r11-10": (11, 10), "r1-2": (1, 2), "r2-1": (2, 1), "r1-1": (1, 1), "r441-80": (441, 80), "r80-441": (80, 441),
               "r1023-1024": (1023, 1024), "unreduced-8000-16000": (8000, 16000),
               # steeper than a tile's span fits in LDS: the samples come from global memory; 211/13 with a table too large for LDS as well
               "steep-40-1": (40, 1), "steep-211-13": (211, 13)}


def _build(name):
    rng = np.random.default_rng(hash_name(name))
    if name == "counts-edge":                 # 0, 0, 1, 2 and K - 1 samples beside a row of 3 tiles plus 1
        K = constants(9, 10)[3]
        return _case([gauss(rng, n) for n in (0, 0, 1, 2, K - 1, n_with_out(3 * TILE + 1, 9, 10))], 9, 10)
    if name in ("tile-edge-up", "tile-edge-down"):        # n_out = TILE - 1, TILE, TILE + 1
        p, q = (9, 10) if name.endswith("up") else (11, 10)
        return _case([gauss(rng, n_with_out(M, p, q)) for M in (TILE - 1, TILE, TILE + 1)], p, q)
    if name == "mmax-above":                  # Mmax above every count; real samples lie behind every length
        rows = [gauss(rng, 900) for _ in range(3)]
        return _case(rows, 9, 10, n_samples=[700, 0, 231], Mmax=6 * TILE + 5)
    if name == "bad-rows":                    # lengths outside [0, Nmax] and an output count above Mmax, between good rows
        rows = [gauss(rng, 400) for _ in range(6)]
        return _case(rows, 9, 10, n_samples=[300, -1, 404, 301, 400, 0], Mmax=n_out(301, 9, 10), extra=3)
    if name in RATIO_CASES:
        p, q = RATIO_CASES[name]
        P, Q, _, K = constants(p, q)
        n_long = max(-((-(TILE + 44) * P) // Q), 2 * K + 5)          # more than one tile of output
        return _case([gauss(rng, n_long), gauss(rng, K + 1), gauss(rng, 1)], p, q)
    if name in ("zeros1", "zeros16"):         # num_zeros 1 and 16
        Z = int(name[5:])
        return _case([gauss(rng, 500), gauss(rng, 3)], 11, 10, num_zeros=Z)
    if name in ("rolloff1", "rolloff05"):
        return _case([gauss(rng, 500), gauss(rng, 3)], 9, 10, rolloff=1.0 if name == "rolloff1" else 0.5)
    if name == "int16-extremes":
        x = np.round(rng.uniform(-32768, 32767, 600))
        x[[0, 3, 250, 251, 599]] = -32768
        x[[1, 4, 300, 301, 598]] = 32767
        return _case([x, gauss(rng, 200, 20000.0)], 9, 10)
    if name == "float32-nan-behind":          # non-integer samples; NaN behind every row's length must not surface
        return _case([rng.standard_normal(n) * 3000.0 for n in (300, 1, 0, 520)], 11, 10, dtype=np.float32, fill=np.nan, extra=90)
    if name == "int16-max-behind":
        return _case([gauss(rng, n) for n in (300, 1, 0, 520)], 9, 10, fill=32767, extra=90)
    if name == "tone":                        # full scale
        return _case([tone(700, 1000.0, 8000.0)], 9, 10)
    if name == "impulse-first":
        x = np.zeros(300)
        x[0] = 32767
        return _case([x], 9, 10)
    if name == "impulse-last":
        x = np.zeros(300)
        x[-1] = -32768
        return _case([x], 11, 10)
    if name == "constant":
        return _case([np.full(600, 12345.0), gauss(rng, 30)], 9, 10)
    if name == "zeros":
        return _case([np.zeros(600), np.zeros(5)], 11, 10)
    raise KeyError(name)


ZERO_ROW_CASES = ("zeros",)
ALL_CASES = ("counts-edge", "tile-edge-up", "tile-edge-down", "mmax-above", "bad-rows") + tuple(RATIO_CASES) + (
    "zeros1", "zeros16", "rolloff1", "rolloff05", "int16-extremes", "float32-nan-behind", "int16-max-behind", "tone", "impulse-first",
    "impulse-last", "constant", "zeros")


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


@functools.lru_cache(maxsize=None)
def result(name):
    """(case, (out, n_out, n_bad)): computed once, shared, never written."""
    c = case(name)
    r = batch_resample(c)
    for a in (c["wave"], c["n_samples"], r[0], r[1]):
        a.setflags(write=False)
    return c, r
