"""SpecAugment of the training loader (include/astk.h astk_spec_augment holds the draw contract): contiguous
frequency and time masks, drawn from a counter-based stream keyed by (seed, presentation counter of the utterance), filled with zero
or with the utterance's own per-bin mean.  Not in the reference: train_cfg.json `extras.spec_augment`, off by default.
  checked_spec_augment   the config dict, validated (what the library would refuse raises ValueError here, naming the key)
  spec_spans             the contract on Python integers
  apply_host             NumPy, one (len, D) utterance -- the CPU loader's path
  apply_device           astk_spec_augment on a padded device batch -- the GPU loader's path"""
import math
import numbers

import numpy as np

from .seq2seq import mix64

_M64 = (1 << 64) - 1
MAX_MASKS = 8           # astk.h ASTK_SPEC_MAX_MASKS
MAX_BINS = 1024         # astk.h ASTK_SPEC_MAX_BINS
FILLS = {"zero": 0, "mean": 1}      # astk.h ASTK_SPEC_FILL_*
DEFAULTS = {"freq_masks": 2, "freq_width": 15, "time_masks": 2, "time_width": 40, "time_ratio": 0.2, "fill": "zero", "seed": 2024}


def _int(cfg, key, what, lo, hi=None):
    v = cfg[key]
    if isinstance(v, bool) or not isinstance(v, (numbers.Integral, np.integer)):
        raise ValueError(f"{what}.{key} must be an integer, got {v!r}")
    v = int(v)
    if v < lo or (hi is not None and v > hi):
        raise ValueError(f"{what}.{key} must be {lo}..{hi}, got {v}" if hi is not None else f"{what}.{key} must be >= {lo}, got {v}")
    return v


def checked_spec_augment(cfg, what="extras.spec_augment"):
    """The config with every key present, or None for off (cfg None or {}).  Keys: freq_masks, time_masks (0..8), freq_width, time_width
    (>= 0, fitting int32), time_ratio (finite, 0..1), fill ("zero" | "mean"), seed (0 <= seed < 2^64); defaults: DEFAULTS."""
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError(f"{what} must be a dict or null, got {cfg!r}")
    if not cfg:
        return None
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"{what}: unknown key {unknown[0]!r} (known: {', '.join(DEFAULTS)})")
    c = dict(DEFAULTS, **cfg)
    out = {"freq_masks": _int(c, "freq_masks", what, 0, MAX_MASKS), "freq_width": _int(c, "freq_width", what, 0, 2**31 - 1),
           "time_masks": _int(c, "time_masks", what, 0, MAX_MASKS), "time_width": _int(c, "time_width", what, 0, 2**31 - 1)}
    p = c["time_ratio"]
    if isinstance(p, bool) or not isinstance(p, (numbers.Real, np.floating, np.integer)):
        raise ValueError(f"{what}.time_ratio must be a number in [0, 1], got {p!r}")
    p = float(p)
    if not math.isfinite(p) or p < 0.0 or p > 1.0:
        raise ValueError(f"{what}.time_ratio must be finite and in [0, 1], got {p!r}")
    out["time_ratio"] = p
    if c["fill"] not in FILLS:
        raise ValueError(f"{what}.fill must be 'zero' or 'mean', got {c['fill']!r}")
    out["fill"] = c["fill"]
    out["seed"] = _int(c, "seed", what, 0, _M64)
    return out


def _word(key, c, i, r):
    return mix64(key ^ ((c << 32) | (i << 1) | r)) >> 11


def spec_spans(seed, counter, D, length, cfg):
    """(frequency spans, time spans) of the utterance presented as number `counter`: lists of (start, width), masks in draw order.
    cfg: a checked_spec_augment dict.  length is the true frame count (already clamped to the batch's T)."""
    seed, counter, D, length = int(seed) & _M64, int(counter) & _M64, int(D), int(length)
    key = mix64(seed ^ mix64(counter))
    freq, time = [], []
    for i in range(cfg["freq_masks"]):
        cap = min(cfg["freq_width"], D)
        f = _word(key, 0, i, 0) % (cap + 1)
        freq.append((_word(key, 0, i, 1) % (D - f + 1), f))
    for i in range(cfg["time_masks"]):
        cap = min(cfg["time_width"], int(cfg["time_ratio"] * length))
        t = _word(key, 1, i, 0) % (cap + 1)
        time.append((_word(key, 1, i, 1) % (length - t + 1), t))
    return freq, time


def apply_host(x, counter, cfg):
    """A masked copy of one (len, D) float32 utterance.  The mean fill takes each bin's mean over the utterance as given, in float64,
    rounded to float32.  An empty utterance comes back as it is."""
    x = np.array(x, dtype=np.float32, copy=True)
    n, D = x.shape
    if n == 0:
        return x
    fill = x.mean(axis=0, dtype=np.float64).astype(np.float32) if cfg["fill"] == "mean" else np.zeros(D, np.float32)
    freq, time = spec_spans(cfg["seed"], counter, D, n, cfg)
    for f0, f in freq:
        x[:, f0:f0 + f] = fill[f0:f0 + f]
    for t0, t in time:
        x[t0:t0 + t, :] = fill
    return x


def apply_device(X, lens, counter0, stride, cfg, stream):
    """astk_spec_augment in place on the padded device batch X (B, T, D) float32; lens: (B,) int32 on the device; row b is presented
    as number counter0 + b * stride; stream: the raw stream handle the call is ordered on.  Allocates nothing, does not synchronise."""
    import ctypes as C
    from . import _lib
    assert X.is_cuda and X.is_contiguous() and X.dim() == 3 and X.dtype.is_floating_point and X.element_size() == 4
    assert lens.is_cuda and lens.is_contiguous() and lens.numel() == X.shape[0] and lens.element_size() == 4
    d = _lib.SpecAugmentDesc(cfg["freq_masks"], cfg["freq_width"], cfg["time_masks"], cfg["time_width"], cfg["time_ratio"], FILLS[cfg["fill"]])
    _lib.check(_lib.load().astk_spec_augment(C.c_void_p(X.data_ptr()), X.shape[0], X.shape[1], X.shape[2], C.c_void_p(lens.data_ptr()),
                                             C.byref(d), cfg["seed"], int(counter0) & _M64, int(stride) & _M64, C.c_void_p(stream)))
