"""An independent restatement of the SpecAugment draw contract (include/astk.h astk_spec_augment) and a float64
model of a masked batch.  Imports nothing from ast_amd.spec_augment: the tests compare that module, the library and the loaders
against this file.

  key(seed, n)      = mix64(seed ^ mix64(n))
  word(key,c,i,r)   = mix64(key ^ ((c << 32) | (i << 1) | r))
  frequency mask i  : cap = min(F, D);            f = (word(key,0,i,0) >> 11) % (cap + 1);  f0 = (word(key,0,i,1) >> 11) % (D - f + 1)
  time mask i       : cap = min(W, int(p * len)); t = (word(key,1,i,0) >> 11) % (cap + 1);  t0 = (word(key,1,i,1) >> 11) % (len - t + 1)
"""
import numpy as np

M = 0xFFFFFFFFFFFFFFFF

# the configuration of the known-answer table: two masks of each kind, F = 15, W = 40, p = 0.2
TABLE_CFG = {"freq_masks": 2, "freq_width": 15, "time_masks": 2, "time_width": 40, "time_ratio": 0.2, "fill": "zero", "seed": 2024}


def cfg(**kw):
    return dict(TABLE_CFG, **kw)


def splitmix(z):
    z = (z + 0x9E3779B97F4A7C15) & M
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def key(seed, n):
    return splitmix((seed & M) ^ splitmix(n & M))


def draw(k, kind, i, r):
    return splitmix(k ^ ((kind << 32) | (i << 1) | r)) >> 11


def spans(seed, n, D, length, c):
    """([(f0, f)], [(t0, t)]) of the utterance presented as number n."""
    k = key(seed, n)
    fs, ts = [], []
    for i in range(c["freq_masks"]):
        w = draw(k, 0, i, 0) % (min(c["freq_width"], D) + 1)
        fs.append((draw(k, 0, i, 1) % (D - w + 1), w))
    for i in range(c["time_masks"]):
        w = draw(k, 1, i, 0) % (min(c["time_width"], int(c["time_ratio"] * length)) + 1)
        ts.append((draw(k, 1, i, 1) % (length - w + 1), w))
    return fs, ts


def masked(X, lens, seed, counter0, stride, c):
    """The expected batch, float64, and the boolean mask of the cells the call writes.  X: (B, T, D); row b has lens[b] true frames
    (clamped to [0, T]) and is presented as number counter0 + b * stride.  Masked cells hold +0.0 (fill "zero") or the float64 mean
    of their bin over the row's true frames as X has them on entry (fill "mean").  Every other cell is X's, converted."""
    X = np.asarray(X)
    B, T, D = X.shape
    out = X.astype(np.float64)
    mask = np.zeros((B, T, D), dtype=bool)
    for b in range(B):
        n = min(max(int(lens[b]), 0), T)
        if n == 0:
            continue
        fs, ts = spans(seed, (counter0 + b * stride) & M, D, n, c)
        for f0, f in fs:
            mask[b, :n, f0:f0 + f] = True
        for t0, t in ts:
            mask[b, t0:t0 + t, :] = True
        assert not mask[b, n:].any()
        fill = X[b, :n].astype(np.float64).mean(axis=0) if c["fill"] == "mean" else np.zeros(D)
        out[b] = np.where(mask[b], fill[None, :], out[b])
    return out, mask


def mean_bound(X, lens):
    """(B, D): len * 2^-24 * mean_t |x[t, d]| -- the worst-case error of a float32 sum of len terms, divided by len."""
    X = np.asarray(X, dtype=np.float64)
    B, T, D = X.shape
    out = np.zeros((B, D))
    for b in range(B):
        n = min(max(int(lens[b]), 0), T)
        if n:
            out[b] = n * 2.0 ** -24 * np.abs(X[b, :n]).mean(axis=0)
    return out
