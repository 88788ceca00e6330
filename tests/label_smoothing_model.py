"""Shared by the label-smoothing tests (tests/test_label_smoothing_host.py, tests/test_gpu_label_smoothing.py): the float64 model of the
smoothed training loss, the same as a minichainer Function, and a context manager that runs the float64 oracle
with it.  For a step's logits x (B, V), scored targets t (clamped to [0, V)), class weights w (None = 1) and count c:

    row_b  = w[t_b] / c ((1 - eps) (LSE_b - x_b[t_b]) + eps (LSE_b - mean_v x_b[v]))
    dx_b,v = w[t_b] / c (softmax(x_b)_v - (1 - eps) [v == t_b] - eps / V)

Smoothing is uniform over all V classes and the ROW carries the target's class weight -- not torch's cross_entropy(weight=,
label_smoothing=), which weights the uniform term per class.  Nothing under oracle/ changes: oracle/ast_ref.py looks
softmax_cross_entropy up through its module at call time, so swapping the module attribute is enough."""
import contextlib

import numpy as np

from oracle import minichainer as F


def _log_softmax(x):
    m = x.max(axis=1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True))


def _prep(x, t, w, dtype=np.float64):
    x = np.asarray(x, dtype)
    V = x.shape[1]
    t = np.clip(np.asarray(t).astype(np.int64), 0, V - 1)
    wt = np.ones(len(t), dtype) if w is None else np.asarray(w, dtype)[t]
    return x, t, wt, V


def smoothed_rows(x, t, w, eps, count):
    """Loss rows (B,) of the definition, float64."""
    x, t, wt, V = _prep(x, t, w)
    logp = _log_softmax(x)
    rows = np.arange(len(t))
    return wt / count * ((1.0 - eps) * -logp[rows, t] + eps * -logp.mean(axis=1))


def smoothed_grad(x, t, w, eps, count):
    """Gradient (B, V) of sum(smoothed_rows) with respect to x, float64."""
    x, t, wt, V = _prep(x, t, w)
    g = np.exp(_log_softmax(x)) - eps / V
    g[np.arange(len(t)), t] -= 1.0 - eps
    return g * (wt / count)[:, None]


class SmoothedSoftmaxCrossEntropy(F.Function):
    """oracle.minichainer._SoftmaxCrossEntropy (A6: class-weighted, normalised by the count of t != -1, == B here) with the uniform term.
    Computes in the dtype of x, like the Function it stands in for; with eps = 0 every operation returns that Function's bits
    ((1 - 0) a + 0 b = a, y - 0 = y)."""

    def __init__(self, t, class_weight, eps):
        self.t = np.asarray(t)
        self.w = class_weight
        self.eps = float(eps)

    def forward(self, xs):
        x = xs[0]
        eps = x.dtype.type(self.eps)
        logp = F.log_softmax_np(x)
        self.y = np.exp(logp)
        rows = np.arange(len(self.t))
        wt = self.w[self.t].astype(x.dtype) if self.w is not None else np.ones(len(self.t), x.dtype)
        self.wt = wt
        self.count = max(int((self.t != -1).sum()), 1)
        per_row = (1 - eps) * logp[rows, self.t] + eps * logp.mean(axis=1)
        return np.asarray(-(per_row * wt).sum() / self.count, dtype=x.dtype)

    def backward(self, gys):
        eps = self.y.dtype.type(self.eps)
        rows = np.arange(len(self.t))
        gx = (self.y - eps / self.y.shape[1]) * self.wt[:, None]
        gx[rows, self.t] -= (1 - eps) * self.wt
        return gx * (gys[0] / self.count)


@contextlib.contextmanager
def smoothed_oracle(eps):
    """Inside: oracle.minichainer.softmax_cross_entropy is the smoothed loss, so RefModel.forward_loss / train_step train on it."""
    orig = F.softmax_cross_entropy

    def smoothed(x, t, class_weight=None):
        t = t.data if isinstance(t, F.Variable) else t
        return SmoothedSoftmaxCrossEntropy(t, class_weight, eps)(x)
    F.softmax_cross_entropy = smoothed
    try:
        yield
    finally:
        F.softmax_cross_entropy = orig
