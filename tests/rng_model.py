"""The counter-based random fills of ast_amd/csrc/util.hip restated in NumPy: dropout keep-masks, Box-Muller normal fills and the
gradient-noise hook's normals, as functions of (seed, offset, index) alone.  "These bits are training behaviour" (util.hip): the masks
are pinned bit for bit, the normals to the accuracy of the device's log / sin / cos.  Built on the splitmix64 finaliser of
tests/sample_noise_model.py.  A helper, not a test module.

Uniforms: a 24-bit integer k from the hash gives u = (k + 1) * 2^-24 in (0, 1].  (The kernels write the factor as 1.0f / 16777217.0f:
the float32 literal 16777217 rounds to 2^24, so the factor IS 2^-24 and every u is an exactly representable float32 -- unlike the sampled
decoder's contract in sample_noise_model.noise, which uses the float32 next to 1 / 16777217.)"""
import numpy as np

from sample_noise_model import mix64, mix64_np

U24 = 2.0 ** -24


def _hash(seed, counters):
    return mix64_np(np.uint64(seed) ^ mix64_np(np.asarray(counters, dtype=np.uint64)))


def _halves(h):
    return h & np.uint64(0xFFFFFFFF), h >> np.uint64(32)


def _u_half(half):
    return ((half >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * U24


def dropout_uniforms(n, seed, offset):
    """u of elements offset .. offset + n - 1: global index g takes the low (g even) or high (g odd) half of mix64(seed ^ mix64(g >> 1))."""
    g = np.uint64(offset) + np.arange(n, dtype=np.uint64)
    lo, hi = _halves(_hash(seed, g >> np.uint64(1)))
    return _u_half(np.where((g & np.uint64(1)) == 0, lo, hi))


def dropout_mask(n, ratio, seed, offset):
    """float32 keep-mask: 1 / (1 - ratio) where float32(u) >= float32(ratio), else 0.  Bit-exact: every quantity is an integer or an
    exactly representable float32, and the kept value is ONE float32 division."""
    r = np.float32(ratio)
    u = dropout_uniforms(n, seed, offset).astype(np.float32)
    return np.where(u >= r, np.float32(1) / (np.float32(1) - r), np.float32(0)).astype(np.float32)


def _box_muller(u1, u2, n):
    r = np.sqrt(-2.0 * np.log(u1))
    out = np.empty(2 * len(u1), np.float64)
    out[0::2] = r * np.cos(2.0 * np.pi * u2)
    out[1::2] = r * np.sin(2.0 * np.pi * u2)
    return out[:n]


def unit_normals(n, seed, offset):
    """float64 unit normals of a normal fill: pair i uses b = mix64(seed ^ mix64(offset + i)), u1 from its low half, u2 from its high half;
    cosine to element 2i, sine to 2i + 1."""
    i = np.uint64(offset) + np.arange((n + 1) // 2, dtype=np.uint64)
    lo, hi = _halves(_hash(seed, i))
    return _box_muller(_u_half(lo), _u_half(hi), n)


def normal_fill(n, mean, sigma, seed, offset):
    return float(np.float32(mean)) + float(np.float32(sigma)) * unit_normals(n, seed, offset)


def hook_noise(n, seed, offset):
    """float64 unit normals of the gradient-noise hook: pair i uses b = mix64(seed ^ mix64(offset + i)), u1 from the top 24 bits of b, u2
    from the top 24 bits of mix64(b)."""
    b = _hash(seed, np.uint64(offset) + np.arange((n + 1) // 2, dtype=np.uint64))
    top = lambda w: ((w >> np.uint64(40)) + np.uint64(1)).astype(np.float64) * U24      # noqa: E731
    return _box_muller(top(b), top(mix64_np(b)), n)


def scalar_hash(seed, counter):
    """The same hash in plain Python integers (cross-check of the NumPy path)."""
    return mix64((seed ^ mix64(counter & ((1 << 64) - 1))) & ((1 << 64) - 1))
