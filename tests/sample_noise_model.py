"""The noise contract of sampled decoding (include/astk.h, "sampled decoding on the device") restated in NumPy and plain Python integers,
independently of the package's own mirror (ast_amd.seq2seq.sample_row_key / gumbel_noise): what tests/test_sample_host.py pins to the
contract's known answers and what tests/test_gpu_sample.py draws the oracle's samples with.  A helper, not a test module."""
import numpy as np

M64 = (1 << 64) - 1


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def row_key(seed, stream):
    return mix64((seed & M64) ^ mix64(stream & M64))


def mix64_np(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def noise(keys, s, n):
    """word >> 40, u (float32) and g (float64) for row keys `keys` (any shape), decoder step s and class ids n (broadcast)."""
    keys, n = np.asarray(keys, dtype=np.uint64), np.asarray(n, dtype=np.uint64)
    word = mix64_np(keys ^ ((np.uint64(s) << np.uint64(32)) | n))
    top = word >> np.uint64(40)
    u = (top + np.uint64(1)).astype(np.float32) * np.float32(1.0 / 16777217.0)
    assert u.dtype == np.float32
    return top, u, -np.log(-np.log(u.astype(np.float64)))
