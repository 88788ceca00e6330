"""Shared by the row-weight tests (tests/test_row_weight_host.py, tests/test_gpu_row_weight.py, tests/test_risk_host.py): the float64
model of the training loss with one weight per batch row, the same as a minichainer Function, and a context
manager that runs the float64 oracle with it.  For a step's logits x (B, V), scored targets t (clamped to [0, V)), class weights w
(None = 1), row weights r (None = 1), smoothing eps and count c:

    row_b  = r_b w[t_b] / c ((1 - eps) (LSE_b - x_b[t_b]) + eps (LSE_b - mean_v x_b[v]))
    dx_b,v = r_b w[t_b] / c (softmax(x_b)_v - (1 - eps) [v == t_b] - eps / V)

r_b is any finite float: a negative weight turns the row's gradient round, 0 switches the row off.  The count stays the number of rows
(quirk Q6), whatever the weights.  Nothing under oracle/ changes: oracle/ast_ref.py looks softmax_cross_entropy up through its module
at call time, so swapping the module attribute is enough; the same (B,) vector applies to the rows of every step."""
import contextlib

import numpy as np

import label_smoothing_model as LS
from oracle import minichainer as F


def weighted_rows(x, t, w, r, eps, count):
    """Loss rows (B,) of the definition, float64."""
    rows = LS.smoothed_rows(x, t, w, eps, count)
    return rows if r is None else np.asarray(r, np.float64) * rows


def weighted_grad(x, t, w, r, eps, count):
    """Gradient (B, V) of sum(weighted_rows) with respect to x, float64."""
    g = LS.smoothed_grad(x, t, w, eps, count)
    return g if r is None else np.asarray(r, np.float64)[:, None] * g


class RowWeightedSoftmaxCrossEntropy(LS.SmoothedSoftmaxCrossEntropy):
    """label_smoothing_model.SmoothedSoftmaxCrossEntropy with the row weights folded into the rows' class weights.  Computes in the dtype
    of x; with all-ones weights and eps = 0 every operation returns the bits of oracle.minichainer._SoftmaxCrossEntropy (wt * 1 = wt)."""

    def __init__(self, t, class_weight, eps, row_weight):
        super().__init__(t, class_weight, eps)
        self.r = np.asarray(row_weight)

    def forward(self, xs):
        x = xs[0]
        eps = x.dtype.type(self.eps)
        logp = F.log_softmax_np(x)
        self.y = np.exp(logp)
        rows = np.arange(len(self.t))
        wt = self.w[self.t].astype(x.dtype) if self.w is not None else np.ones(len(self.t), x.dtype)
        assert self.r.shape == wt.shape, "one weight per row of the step"
        self.wt = wt * self.r.astype(x.dtype)
        self.count = max(int((self.t != -1).sum()), 1)
        per_row = (1 - eps) * logp[rows, self.t] + eps * logp.mean(axis=1)
        return np.asarray(-(per_row * self.wt).sum() / self.count, dtype=x.dtype)


@contextlib.contextmanager
def weighted_oracle(eps, row_weight, record=None):
    """Inside: oracle.minichainer.softmax_cross_entropy is the smoothed loss with the (B,) vector row_weight on every step's rows, so
    RefModel.forward_loss / train_step train on it.  record: a list that gets one (logits copy, targets copy) per call, in call order."""
    orig = F.softmax_cross_entropy
    r = np.asarray(row_weight, np.float64)

    def weighted(x, t, class_weight=None):
        t = t.data if isinstance(t, F.Variable) else t
        if record is not None:
            record.append((np.array(x.data if isinstance(x, F.Variable) else x), np.array(t)))
        return RowWeightedSoftmaxCrossEntropy(t, class_weight, eps, r)(x)
    F.softmax_cross_entropy = weighted
    try:
        yield
    finally:
        F.softmax_cross_entropy = orig
