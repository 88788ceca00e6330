"""The speech features and CMVN of include/astk.h (astk_speech_features, astk_cmvn_accumulate, astk_cmvn_apply)
restated in NumPy float64, and the named cases the host and GPU tests run.  A helper, not a test module.

This file IS the contract: it is written from Kaldi's documented algorithm and option names (compute-mfcc-feats / compute-fbank-feats,
snip-edges=true), but no Kaldi output exists to pin it to.  tests/test_speech_features_host.py pins it independently instead (a direct
DFT, Parseval, the shape of the filters, orthonormal DCT rows, a float32 restatement).

Two things are stated more narrowly than "float64" so that silence is reproducible bit for bit:
  * a floored energy's logarithm is the constant LOG_EPS, not a call of log;
  * lift_k dct[k][j] is built from det_cospi, a fixed sequence of IEEE operations, and the cepstra are summed over ascending j with
    every product and every sum rounded on its own.  The kernel repeats both, so its table equals this one bit for bit and the
    cepstra of a frame whose energies all sit on the floor (sums that cancel to rounding noise) equal the model's."""
import functools
import math

import numpy as np
import scipy.fft

import rng_model as RM

EPS = 2.0 ** -23
LOG_EPS = -15.942385152878742
assert LOG_EPS == math.log(EPS)
WINDOWS = ("povey", "hamming", "hanning", "rectangular")
DEFAULTS = dict(sample_frequency=8000.0, frame_length=25.0, frame_shift=10.0, num_mel_bins=23, num_ceps=13, low_freq=20.0, high_freq=0.0,
                preemphasis_coefficient=0.97, cepstral_lifter=22.0, window_type="povey", kind="mfcc", remove_dc_offset=True,
                use_energy=False, dither=0.0, frame_len=None, frame_shift_samples=None)


def config(**kw):
    """A configuration as a plain dict: Kaldi's option names; frame_len / frame_shift_samples (in samples) override the millisecond
    fields when given."""
    c = dict(DEFAULTS)
    assert set(kw) <= set(c), set(kw) - set(c)
    c.update(kw)
    if c["frame_len"] is None:
        c["frame_len"] = int(round(c["sample_frequency"] * c["frame_length"] / 1000.0))
    if c["frame_shift_samples"] is None:
        c["frame_shift_samples"] = int(round(c["sample_frequency"] * c["frame_shift"] / 1000.0))
    return c


def dim(cfg):
    return cfg["num_mel_bins"] if cfg["kind"] == "fbank" else cfg["num_ceps"]


def fft_size(cfg):
    n = 2
    while n < cfg["frame_len"]:
        n *= 2
    return n


def frames(n_samples, frame_len, frame_shift):
    return 0 if n_samples < frame_len else 1 + (n_samples - frame_len) // frame_shift


# ------------------------------------------------------------------ cos(pi t) in a fixed sequence of IEEE operations
_CC = [(-1.0) ** n / float(math.factorial(2 * n)) for n in range(11)]
_SC = [(-1.0) ** n / float(math.factorial(2 * n + 1)) for n in range(11)]


def _poly(c, x2):
    acc = np.full_like(x2, c[-1])
    for v in c[-2::-1]:
        acc = acc * x2 + v               # NumPy: one rounded product, one rounded sum
    return acc


def det_cospi(t):
    """cos(pi t) for t >= 0: fmod to [0, 2), fold to [0, 1/2] with the sign, then the Taylor series of cos below 1/4 and of sin(pi (1/2 - r))
    above.  Accurate to a few units of 2^-53; what matters is that every step is one correctly rounded operation."""
    t = np.asarray(t, np.float64)
    r = np.fmod(t, 2.0)
    r = np.where(r > 1.0, 2.0 - r, r)
    sign = np.where(r > 0.5, -1.0, 1.0)
    r = np.where(r > 0.5, 1.0 - r, r)
    xs = np.pi * (0.5 - r)
    xc = np.pi * r
    v = np.where(r > 0.25, xs * _poly(_SC, xs * xs), _poly(_CC, xc * xc))
    return sign * v


def det_sinpi(t):
    return det_cospi(np.abs(np.asarray(t, np.float64) - 0.5))


def dct_rows(cfg):
    """dct[k][j], k < num_ceps: orthonormal rows."""
    M, K = cfg["num_mel_bins"], cfg["num_ceps"]
    j = np.arange(M, dtype=np.float64)[None, :]
    k = np.arange(K, dtype=np.float64)[:, None]
    d = np.sqrt(2.0 / M) * det_cospi(((j + 0.5) * k) / M)
    d[0] = np.sqrt(1.0 / M)
    return d


def lifter(cfg):
    Q, K = float(cfg["cepstral_lifter"]), cfg["num_ceps"]
    if Q == 0.0:
        return np.ones(K)
    return 1.0 + (0.5 * Q) * det_sinpi(np.arange(K, dtype=np.float64) / Q)


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, np.float64) / 700.0)


def resolved_high(cfg):
    return cfg["high_freq"] if cfg["high_freq"] > 0 else 0.5 * cfg["sample_frequency"] + cfg["high_freq"]


def mel_banks(cfg):
    """(num_mel_bins, N / 2) weights of the FFT bins 0 .. N/2 - 1 (the Nyquist bin is not used)."""
    N, M = fft_size(cfg), cfg["num_mel_bins"]
    lo, hi = float(mel(cfg["low_freq"])), float(mel(resolved_high(cfg)))
    delta = (hi - lo) / (M + 1)
    m = mel(np.arange(N // 2, dtype=np.float64) * cfg["sample_frequency"] / N)
    W = np.zeros((M, N // 2))
    for j in range(M):
        left, center, right = lo + j * delta, lo + (j + 1) * delta, lo + (j + 2) * delta
        inside = (m > left) & (m < right)
        up = (m - left) / (center - left)
        down = (right - m) / (right - center)
        W[j] = np.where(inside, np.where(m <= center, up, down), 0.0)
    return W


def window(cfg):
    L = cfg["frame_len"]
    c = np.cos(2.0 * np.pi * np.arange(L, dtype=np.float64) / (L - 1))
    return {"povey": lambda: (0.5 - 0.5 * c) ** 0.85, "hamming": lambda: 0.54 - 0.46 * c, "hanning": lambda: 0.5 - 0.5 * c,
            "rectangular": lambda: np.ones(L)}[cfg["window_type"]]()


def dither_stream(seed, g0, n):
    """z(seed, g) for g = g0 .. g0 + n - 1: element g of rng_model.unit_normals(., seed, 0)."""
    return RM.unit_normals(n + (g0 & 1), seed, g0 >> 1)[(g0 & 1):]


def log_floor(e):
    e = np.asarray(e, np.float64)
    return np.where(e > EPS, np.log(np.where(e > EPS, e, 1.0)), LOG_EPS)


def windowed_frames(x, cfg, seed=0, offset=0):
    """(F, frame_len) float64 frames after dither, DC removal, pre-emphasis and the window; and the raw log energies (F)."""
    L, S = cfg["frame_len"], cfg["frame_shift_samples"]
    x = np.asarray(x).astype(np.float64)
    F = frames(len(x), L, S)
    if cfg["dither"] != 0.0 and len(x):
        x = x + cfg["dither"] * dither_stream(seed, int(offset), len(x))
    fr = x[np.arange(F)[:, None] * S + np.arange(L)[None, :]] if F else np.zeros((0, L))
    if cfg["remove_dc_offset"]:
        fr = fr - fr.mean(axis=1, keepdims=True)
    energy = log_floor((fr * fr).sum(axis=1))
    c = float(cfg["preemphasis_coefficient"])
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    return (fr - c * prev) * window(cfg)[None, :], energy


def power_spectrum(wf, cfg):
    """(F, N / 2 + 1) |X_k|^2 of the zero-padded frames."""
    N = fft_size(cfg)
    pad = np.zeros((wf.shape[0], N))
    pad[:, :wf.shape[1]] = wf
    S = scipy.fft.rfft(pad, axis=1)
    return S.real ** 2 + S.imag ** 2


def mel_energies(x, cfg, seed=0, offset=0):
    wf, energy = windowed_frames(x, cfg, seed, offset)
    P = power_spectrum(wf, cfg)
    return P[:, :-1] @ mel_banks(cfg).T, energy


def features(x, cfg, seed=0, offset=0):
    """(F, D) float64 features of one waveform."""
    E, energy = mel_energies(x, cfg, seed, offset)
    Lg = log_floor(E)
    if cfg["kind"] == "fbank":
        return Lg
    T = lifter(cfg)[:, None] * dct_rows(cfg)                 # (K, M)
    acc = np.zeros((Lg.shape[0], cfg["num_ceps"]))
    for j in range(cfg["num_mel_bins"]):
        acc = acc + T[None, :, j] * Lg[:, j, None]
    if cfg["use_energy"]:
        acc[:, 0] = energy
    return acc


def batch_features(case):
    """What astk_speech_features leaves for a case: feats (B, Fmax, D) float32 (the float64 values rounded once), n_frames, n_bad."""
    cfg = case["cfg"]
    B, Fmax, D = len(case["n_samples"]), case["Fmax"], dim(cfg)
    feats = np.zeros((B, Fmax, D), np.float32)
    n_frames = np.zeros(B, np.int32)
    for b, n in enumerate(case["n_samples"].tolist()):
        F = -1 if (n < 0 or n > case["wave"].shape[1]) else frames(n, cfg["frame_len"], cfg["frame_shift_samples"])
        if F > Fmax:
            F = -1
        n_frames[b] = F
        if F > 0:
            feats[b, :F] = features(case["wave"][b, :n], cfg, case["seed"], case["offsets"][b]).astype(np.float32)
    return feats, n_frames, int((n_frames < 0).sum())


# ------------------------------------------------------------------ CMVN
def cmvn_stats(X, n_frames, group, G, stats=None):
    """Adds to stats (G, 2, D + 1) float64 in Kaldi's layout; returns (stats, n_bad)."""
    B, Fmax, D = X.shape
    stats = np.zeros((G, 2, D + 1)) if stats is None else stats.copy()
    n_bad = 0
    for b in range(B):
        g, nf = int(group[b]), int(n_frames[b])
        if g < 0 or g >= G:
            n_bad += 1
            continue
        if nf < 0:
            continue
        x = X[b, :min(nf, Fmax)].astype(np.float64)
        stats[g, 0, :D] += x.sum(axis=0)
        stats[g, 1, :D] += (x * x).sum(axis=0)
        stats[g, 0, D] += x.shape[0]
    return stats, n_bad


def cmvn_apply(X, n_frames, group, stats, norm_vars):
    B, Fmax, D = X.shape
    G = stats.shape[0]
    Y = X.copy()
    for b in range(B):
        g, nf = int(group[b]), int(n_frames[b])
        if g < 0 or g >= G or nf < 0 or stats[g, 0, D] <= 0:
            continue
        count = stats[g, 0, D]
        mean = stats[g, 0, :D] / count
        scale = np.ones(D)
        if norm_vars:
            scale = 1.0 / np.sqrt(np.maximum(stats[g, 1, :D] / count - mean * mean, 1e-20))
        nf = min(nf, Fmax)
        Y[b, :nf] = ((X[b, :nf].astype(np.float64) - mean) * scale).astype(np.float32)
    return Y


# ------------------------------------------------------------------ the named cases
def n_for(F, cfg):
    """Samples of exactly F >= 1 frames."""
    return cfg["frame_len"] + (F - 1) * cfg["frame_shift_samples"]


def gauss(rng, n, sigma=3000.0):
    return np.clip(np.round(rng.standard_normal(n) * sigma), -32768, 32767)


def tone(n, freq=500.0, sr=8000.0, amp=32767.0):
    return np.round(amp * np.sin(2.0 * np.pi * freq / sr * np.arange(n)))


def _pack(rows, dtype, fill, extra=3):
    """Rows of different lengths -> (B, Nmax) with `fill` written behind every row's length (Nmax = the longest row + extra)."""
    Nmax = max(1, max(len(r) for r in rows) + extra)
    w = np.full((len(rows), Nmax), fill, dtype=dtype)
    for b, r in enumerate(rows):
        w[b, :len(r)] = np.asarray(r).astype(dtype)
    return w, np.asarray([len(r) for r in rows], np.int32)


def _case(rows, cfg=None, dtype=np.int16, fill=0, Fmax=None, seed=0, offsets=None, n_samples=None, extra=3):
    cfg = cfg or config()
    wave, n = _pack(rows, dtype, fill, extra)
    if n_samples is not None:
        n = np.asarray(n_samples, np.int32)
    good = [frames(int(v), cfg["frame_len"], cfg["frame_shift_samples"]) for v in n.tolist() if 0 <= v <= wave.shape[1]]
    Fmax = Fmax or max(1, max(good) if good else 1)
    return dict(cfg=cfg, wave=wave, n_samples=n, Fmax=Fmax, seed=seed,
                offsets=np.asarray(offsets if offsets is not None else [0] * len(rows), np.int64), with_offsets=offsets is not None)


def _build(name):
    rng = np.random.default_rng(abs(hash_name(name)))
    c8 = config()
    c16 = dict(sample_frequency=16000.0)
    g = lambda F, cfg=c8, sigma=3000.0: gauss(rng, n_for(F, cfg), sigma)        # noqa: E731
    if name == "counts-edge":                 # 0, 0, 1, 1, 2 frames beside a 9-frame row: zero-frame rows, zero fill behind F_b
        return _case([gauss(rng, n) for n in (0, 199, 200, 279, 280)] + [g(9)])
    if name == "counts-workgroup":            # 3, 4, 5, 9 frames and one row of 130
        return _case([g(3), g(4), g(5), g(9), g(130)])
    if name == "fmax-above":                  # Fmax above every count; 6 x 1700 items: real frames (row 5) behind the grid's first stride
        return _case([g(3), g(4), g(5), g(9), gauss(rng, 100), g(130)], Fmax=1700)
    if name == "bad-rows":                    # lengths outside [0, Nmax] and a row with more frames than Fmax, between good rows
        rows = [g(5), g(5), g(5), g(9), g(5), g(2)]
        return _case(rows, Fmax=5, n_samples=[n_for(5, c8), -1, n_for(9, c8) + 4, n_for(9, c8), n_for(4, c8) + 7, 0])
    if name == "int16-extremes":
        x = np.round(rng.uniform(-32768, 32767, n_for(6, c8)))
        x[[3, 250, 251]] = -32768
        x[[4, 300, 301]] = 32767
        return _case([x, gauss(rng, n_for(2, c8), 20000.0)])
    if name == "float32-nan-behind":          # non-integer samples; NaN behind every row's length must not surface
        return _case([rng.standard_normal(n_for(F, c8)) * 3000.0 for F in (4, 1, 7)] + [rng.standard_normal(150)], dtype=np.float32,
                     fill=np.nan, extra=90)
    if name == "int16-max-behind":
        return _case([g(4), g(1), g(7), gauss(rng, 150)], fill=32767, extra=90)
    if name == "gauss":
        return _case([g(9)])
    if name == "tone":                        # a clean full-scale 500 Hz tone: the case that separates float64 from float32 arithmetic
        return _case([tone(n_for(9, c8))])
    if name == "loud-quiet":
        n = n_for(9, c8)
        return _case([np.concatenate([gauss(rng, n // 2, 20000.0), np.round(rng.uniform(-2, 2, n - n // 2))])])
    if name == "impulse":                     # frames of exact zeros beside the frames that hold the impulse
        x = np.zeros(n_for(9, c8))
        x[300] = 32767
        return _case([x])
    if name == "constant":                    # exactly zero after the DC removal
        return _case([np.full(n_for(9, c8), 12345.0), g(3)])
    if name == "zeros":
        return _case([np.zeros(n_for(5, c8)), np.zeros(100)])
    if name == "16k-fbank80":                 # more filters than lanes
        cfg = config(num_mel_bins=80, kind="fbank", **c16)
        return _case([g(5, cfg), tone(n_for(3, cfg), sr=16000.0), np.round(rng.uniform(-1, 1, n_for(4, cfg)))], cfg)
    if name == "16k-mfcc40":
        cfg = config(num_mel_bins=40, num_ceps=40, **c16)
        return _case([g(5, cfg), g(2, cfg)], cfg)
    if name == "len256":                      # no padding at all
        cfg = config(frame_len=256)
        return _case([g(5, cfg), g(1, cfg)], cfg)
    if name == "len100":
        cfg = config(frame_len=100, frame_shift_samples=40)
        return _case([g(7, cfg), g(1, cfg)], cfg)
    if name == "len1200":                     # N = 2048, the largest transform
        cfg = config(frame_len=1200, frame_shift_samples=480)
        return _case([g(5, cfg), g(1, cfg)], cfg)
    if name == "len2":                        # N = 2, the smallest transform: one complex point, one usable bin
        cfg = config(frame_len=2, frame_shift_samples=1, low_freq=0.0, num_mel_bins=3, num_ceps=3, remove_dc_offset=False, preemphasis_coefficient=0.0)
        return _case([g(1, cfg) + 9000, g(70, cfg) + 9000], cfg)
    if name == "band":
        cfg = config(high_freq=-200.0, low_freq=0.0)
        return _case([g(5, cfg)], cfg)
    if name in ("hamming", "hanning", "rectangular"):
        cfg = config(window_type=name)
        return _case([g(5, cfg)], cfg)
    if name == "preemph0":
        cfg = config(preemphasis_coefficient=0.0)
        return _case([g(5, cfg)], cfg)
    if name == "no-dc":
        cfg = config(remove_dc_offset=False)
        return _case([g(5, cfg) + 700, np.full(n_for(2, cfg), 12345.0)], cfg)
    if name == "lifter0":
        cfg = config(cepstral_lifter=0.0)
        return _case([g(5, cfg)], cfg)
    if name == "energy":
        cfg = config(use_energy=True)
        return _case([g(5, cfg), np.zeros(n_for(2, cfg))], cfg)
    if name in ("dither-seed1", "dither-seed2"):      # the same samples under two seeds, non-zero offsets (odd and even)
        rng = np.random.default_rng(77)
        cfg = config(dither=1.0)
        rows = [gauss(rng, n_for(5, cfg)), np.zeros(n_for(3, cfg)), gauss(rng, n_for(2, cfg))]
        return _case(rows, cfg, seed=1 if name.endswith("1") else 2, offsets=[12345, 7, 0])
    raise KeyError(name)


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % (2 ** 31)
    return h


EXACT_ZERO_CASES = ("constant", "zeros", "impulse")          # cases with frames whose every energy is exactly 0
NOISE_LIKE_CASES = ("gauss", "counts-edge", "loud-quiet", "int16-extremes", "16k-mfcc40")
ALL_CASES = ("counts-edge", "counts-workgroup", "fmax-above", "bad-rows", "int16-extremes", "float32-nan-behind", "int16-max-behind", "gauss",
             "tone", "loud-quiet", "impulse", "constant", "zeros", "16k-fbank80", "16k-mfcc40", "len256", "len100", "len1200", "len2", "band",
             "hamming", "hanning", "rectangular", "preemph0", "no-dc", "lifter0", "energy", "dither-seed1", "dither-seed2")


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


@functools.lru_cache(maxsize=None)
def result(name):
    """(case, (feats, n_frames, n_bad)): computed once, shared, never written."""
    c = case(name)
    r = batch_features(c)
    for a in (c["wave"], c["n_samples"], c["offsets"], r[0], r[1]):
        a.setflags(write=False)
    return c, r


def _cmvn_build(name):
    rng = np.random.default_rng(hash_name(name))
    D = 13

    def rows(lens, Fmax=None):
        Fmax = Fmax or max(max(lens), 1)
        X = np.zeros((len(lens), Fmax, D), np.float32)
        for b, n in enumerate(lens):
            if n > 0:
                X[b, :n] = (rng.standard_normal((n, D)) * 4.0 + rng.standard_normal(D) * 10.0).astype(np.float32)
        return X, np.asarray(lens, np.int32)
    if name == "per-utterance":               # group[b] = b; a one-frame utterance (variance floor) and a constant-feature one
        X, nf = rows([9, 1, 70, 5, 0])
        X[3, :5] = np.float32(3.25) * np.arange(1, D + 1, dtype=np.float32)[None, :]
        return dict(X=X, n_frames=nf, group=np.arange(5, dtype=np.int32), G=5, norm_vars=True)
    if name == "two-speakers":                # five rows of different lengths over two speakers; group 2 has no frames at all
        X, nf = rows([9, 130, 3, 65, 17], Fmax=131)
        return dict(X=X, n_frames=nf, group=np.asarray([0, 1, 0, 1, 1], np.int32), G=3, norm_vars=True)
    if name == "empty-group":                 # a group whose only row has no frames, and a row the features marked bad
        X, nf = rows([6, 0, 4, 5])
        nf[3] = -1
        return dict(X=X, n_frames=nf, group=np.asarray([0, 1, 0, 2], np.int32), G=3, norm_vars=True)
    if name == "no-norm-vars":
        X, nf = rows([9, 4, 2])
        return dict(X=X, n_frames=nf, group=np.asarray([0, 0, 1], np.int32), G=2, norm_vars=False)
    if name == "bad-group":
        X, nf = rows([5, 6, 7, 8])
        return dict(X=X, n_frames=nf, group=np.asarray([0, -1, 2, 1], np.int32), G=2, norm_vars=True)
    if name == "wide":                        # 80 columns: more than one column block
        D = 80
        X, nf = rows([5, 66])
        return dict(X=X, n_frames=nf, group=np.asarray([0, 0], np.int32), G=1, norm_vars=True)
    raise KeyError(name)


CMVN_CASES = ("per-utterance", "two-speakers", "empty-group", "no-norm-vars", "bad-group", "wide")


@functools.lru_cache(maxsize=None)
def cmvn_case(name):
    c = _cmvn_build(name)
    for a in (c["X"], c["n_frames"], c["group"]):
        a.setflags(write=False)
    return c
