"""The contract of truncated sampling (include/astk.h, "truncated sampling on the device": top-k, then top-p among the survivors)
restated in NumPy float64 on top of sample_noise_model.noise, independently of the package's own pick function
(ast_amd.seq2seq.truncated_pick): what tests/test_truncate_host.py pins to known answers and what tests/test_gpu_truncate.py compares the
device loop and the per-step fallback with.  A helper, not a test module."""
import numpy as np

from sample_noise_model import noise


def scaled(lg, inv_temp):
    """Step 1: xs = x * inv_temp -- in float32 for float32 logits (the rank is taken on the float32 xs), in float64 for an oracle's."""
    lg = np.asarray(lg)
    if lg.dtype == np.float32:
        return (lg * np.float32(inv_temp)).astype(np.float64)
    return lg.astype(np.float64) * float(inv_temp)


def draw_from(xs, g, top_k, top_p):
    """Steps 2 to 5 for rows of scaled logits xs (B, V) float64 and their noise g (B, V) float64.  Returns per row the token, logp, the
    kept count m and the guard gap, the least of
      xs_{K-1} - xs_K                  (only where m = K and K < V: the k-th and the first excluded candidate),
      min_j |cum_j - top_p|            (only where top_p < 1: how close a prefix sum comes to the cut),
      the top-2 gap of z among the kept (only where m > 1)."""
    B, V = xs.shape
    K = int(top_k)
    assert 1 <= K <= V and 0.0 < top_p <= 1.0
    order = np.argsort(-xs, axis=1, kind="stable")           # higher values first, among equal values the lower id first
    rows = np.arange(B)[:, None]
    ids = order[:, :K]
    v = xs[rows, ids]
    q = np.exp(v - v[:, :1])
    q = q / q.sum(axis=1, keepdims=True)
    cum = np.cumsum(q, axis=1)
    if top_p == 1.0:
        m = np.full(B, K)
    else:
        reach = cum >= top_p
        m = np.where(reach.any(axis=1), reach.argmax(axis=1) + 1, K)
    tok, logp, gap = np.zeros(B, np.int32), np.zeros(B), np.full(B, np.inf)
    for b in range(B):
        mb = int(m[b])
        z = v[b, :mb] + g[b, ids[b, :mb]]
        best = np.flatnonzero(z == z.max())
        j = int(best[np.argmin(ids[b, best])])                # among equal z the lower token id
        tok[b] = ids[b, j]
        logp[b] = (v[b, j] - v[b, 0]) - np.log(np.exp(v[b, :mb] - v[b, 0]).sum())
        if mb == K and K < V:
            gap[b] = min(gap[b], v[b, K - 1] - xs[b, order[b, K]])
        if top_p < 1.0:
            gap[b] = min(gap[b], np.abs(cum[b] - top_p).min())
        if mb > 1:
            zs = np.sort(z)
            gap[b] = min(gap[b], zs[-1] - zs[-2])
    return tok, logp, m.astype(np.int32), gap


def draw(lg, keys, step, inv_temp, top_k, top_p):
    """One step's truncated draw from logits lg (B, V) for the row keys `keys` (B,) uint64: token, logp, m, guard gap."""
    xs = scaled(lg, inv_temp)
    g = noise(np.asarray(keys, dtype=np.uint64)[:, None], step, np.arange(xs.shape[1])[None, :])[2]
    return draw_from(xs, g, top_k, top_p)
