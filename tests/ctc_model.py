"""Shared by the CTC tests (tests/test_ctc_host.py, tests/test_gpu_ctc.py): a NumPy model of the CTC loss of include/astk.h
astk_ctc_loss and of its gradient with respect to the LOGITS, runnable in float64 and float32, the input cases of
the operator tests, and a context manager that adds ctc_weight * mean_b nll_b over a `ctc_out` head to the float64 oracle's train step.

For a row with labels l_1 .. l_U the extended sequence z has S' = 2U + 1 states, blanks at the even positions.  With e[t][s] =
log softmax(logits[t])[z_s], in the log domain,

    alpha[0][0] = e[0][0], alpha[0][1] = e[0][1];  alpha[t][s] = e[t][s] + log(exp alpha[t-1][s] + exp alpha[t-1][s-1] + [skip] exp alpha[t-1][s-2])
    [skip]: z_s is a label and z_s != z_{s-2};     log p = log(exp alpha[n-1][S'-1] + exp alpha[n-1][S'-2]);   nll = -log p
    d nll / d logits[t][k] = softmax(logits[t])[k] - sum_{s: z_s = k} exp(alpha[t][s] + beta[t][s] - e[t][s] - log p)

over the n = input_len valid frames; frames behind n get gradient 0.  A row with n < U + (adjacent equal labels) has no path: nll = +inf,
gradient 0, not part of the sum.  Nothing under oracle/ changes: the wrapper swaps RefModel.forward_loss for the block."""
import contextlib

import numpy as np

from oracle import ast_ref as R
from oracle import minichainer as F

PAD_ID, UNK_ID = 0, 3          # the model's blank and first label (ast_amd/seq2seq.py)


def labels_of(yrow, first_label, V):
    """The labels of one target row: entries with id >= first_label, in order (ids >= V are read as V - 1, like the kernel)."""
    return [min(int(i), V - 1) for i in yrow if int(i) >= first_label]


def feasible(labels, n):
    return n >= len(labels) + sum(1 for a, b in zip(labels[:-1], labels[1:]) if a == b)


def ctc_row(x, labels, blank, dtype=np.float64):
    """(nll, d nll / d x) of one row: x (n, V) logits of the valid frames; every operation in `dtype`.  (inf, zeros) without a path."""
    x = np.asarray(x, dtype)
    n, V = x.shape
    if not feasible(labels, n):
        return dtype(np.inf), np.zeros_like(x)
    if n == 0:
        return dtype(0.0), np.zeros_like(x)
    U = len(labels)
    S = 2 * U + 1
    z = np.full(S, blank, np.int64)
    z[1::2] = labels
    skip = np.zeros(S, bool)
    skip[3::2] = z[3::2] != z[1:-2:2]
    m = x.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(axis=1, keepdims=True, dtype=dtype))
    logp = x - lse
    e = logp[:, z]                                                # (n, S)
    ninf = dtype(-np.inf)

    def shifted(a, k):                                            # a[s - k] (k > 0) or a[s + |k|], -inf outside
        out = np.full(S, ninf, dtype)
        if k > 0:
            out[k:] = a[:S - k]
        else:
            out[:S + k] = a[-k:]
        return out
    with np.errstate(invalid="ignore", over="ignore"):
        alpha = np.full((n, S), ninf, dtype)
        prev = np.full(S, ninf, dtype)
        prev[0] = 0
        for t in range(n):
            a2 = np.where(skip, shifted(prev, 2), ninf)
            prev = np.logaddexp(np.logaddexp(prev, shifted(prev, 1)), a2).astype(dtype) + e[t]
            alpha[t] = prev
        ll = np.logaddexp(alpha[-1, S - 1], alpha[-1, S - 2] if S >= 2 else ninf).astype(dtype)
        skip_b = np.zeros(S, bool)
        skip_b[:-2] = skip[2:]
        nxt = np.full(S, ninf, dtype)
        nxt[S - 1] = 0
        occ = np.zeros((n, V), dtype)
        for t in range(n - 1, -1, -1):
            b2 = np.where(skip_b, shifted(nxt, -2), ninf)
            nxt = np.logaddexp(np.logaddexp(nxt, shifted(nxt, -1)), b2).astype(dtype) + e[t]
            dead = np.isneginf(alpha[t]) | np.isneginf(nxt)
            g = np.where(dead, dtype(0), np.exp(np.where(dead, dtype(0), alpha[t] + nxt - e[t] - ll))).astype(dtype)
            np.add.at(occ[t], z, g)
    return dtype(-ll), (np.exp(logp) - occ).astype(dtype)


def ctc_loss_grad(logits, y, input_len=None, first_label=UNK_ID, blank=PAD_ID, scale=1.0, dtype=np.float64):
    """The contract of astk_ctc_loss on host arrays: dict(row_nll (B), dlogits (B, T, V) = scale * d(sum of feasible nll) / d logits,
    loss = scale * sum of the feasible rows' nll, n_infeasible)."""
    logits = np.asarray(logits)
    B, T, V = logits.shape
    lens = np.full(B, T, np.int64) if input_len is None else np.clip(np.asarray(input_len).astype(np.int64), 0, T)
    nll = np.zeros(B, dtype)
    g = np.zeros((B, T, V), dtype)
    bad = 0
    for b in range(B):
        n = int(lens[b])
        nll[b], gb = ctc_row(logits[b, :n], labels_of(y[b], first_label, V), blank, dtype)
        if np.isinf(nll[b]):
            bad += 1
        else:
            g[b, :n] = gb * dtype(scale)
    ok = ~np.isinf(nll)
    return dict(row_nll=nll, dlogits=g, loss=dtype(scale) * nll[ok].sum(dtype=dtype), n_infeasible=bad)


def collapse(best, blank=PAD_ID):
    """Greedy CTC decode of one row of per-frame classes: repeats collapsed, blanks dropped."""
    out, prev = [], None
    for c in best:
        c = int(c)
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


# ------------------------------------------------------------------ operator cases
def op_logits(kind, B, T, V, seed):
    """Logits of one value kind, float32: 'normal' N(0, 1); 'offset+' / 'offset-' the same shifted by +-30; 'peaked' N(0, 1) with one
    class per frame raised by 30 (tests/range_cases.py: offset and peaked inputs)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    if kind == "offset+":
        x += np.float32(30)
    elif kind == "offset-":
        x -= np.float32(30)
    elif kind == "peaked":
        k = rng.integers(0, V, size=(B, T))
        np.put_along_axis(x, k[..., None], np.take_along_axis(x, k[..., None], 2) + np.float32(30), 2)
    elif kind != "normal":
        raise KeyError(kind)
    return x


def _distinct(first, n):
    return list(range(first, first + n))


# name -> dict(kind, family, B, T, V, L, rows = per row a label count or an explicit label list, lens, ldv pad).  The smallest shapes at
# which the kernels can go wrong: V below / no multiple of / above a wavefront and of 4; one row, a few, more rows than a wave set; T = 1,
# 2; U = 0, 1; S' = 63, 65, 129, 511 around the wavefront boundaries; T = U + repeats (exactly one path); all labels equal; ragged
# lengths down to 1; an infeasible row between feasible ones (U = 255 in 64 frames); row lengths one short of, at and one past
# the step loop's block of 16 (ctc_rows.h CTC_PF).  `family` names the tolerance the case is held to.
OP_CASES = {
    "t1-v5": dict(kind="normal", family="short", B=3, T=1, V=5, L=4, rows=[0, [4], 0], lens=None),
    "t2-v5": dict(kind="normal", family="short", B=3, T=2, V=5, L=4, rows=[0, [3], [3, 4]], lens=[2, 1, 2]),
    "b33-ragged": dict(kind="normal", family="short", B=33, T=9, V=57, L=7, rows=[b % 5 for b in range(33)],
                       lens=[1 if b % 5 < 2 and b % 3 == 0 else 9 - (b % 3) for b in range(33)]),
    "v1098-one-path": dict(kind="normal", family="short", B=3, T=9, V=1098, L=12, rows=[2, _distinct(500, 9), 0], lens=None),
    "all-equal-one-path": dict(kind="normal", family="short", B=1, T=9, V=57, L=8, rows=[[7] * 5], lens=None),
    "all-equal": dict(kind="normal", family="short", B=3, T=9, V=57, L=8, rows=[[7] * 4, [9] * 2, [11]], lens=[9, 5, 9]),
    "offset+": dict(kind="offset+", family="offset", B=3, T=9, V=57, L=6, rows=[2, 3, 0], lens=None),
    "offset-": dict(kind="offset-", family="offset", B=3, T=9, V=57, L=6, rows=[2, 3, 0], lens=[9, 7, 2]),
    "peaked": dict(kind="peaked", family="peaked", B=3, T=9, V=57, L=6, rows=[2, 3, 0], lens=None),
    "u31-log-domain": dict(kind="normal", family="long", B=1, T=64, V=57, L=40, rows=[31], lens=None),
    "u32-ragged": dict(kind="normal", family="long", B=3, T=64, V=57, L=40, rows=[32, 31, 1], lens=[64, 40, 1]),
    "u64-one-path": dict(kind="normal", family="long", B=1, T=64, V=1098, L=70, rows=[_distinct(100, 64)], lens=None),
    "u255-infeasible-between": dict(kind="normal", family="long", B=3, T=64, V=57, L=255, rows=[5, 255, 64], lens=[64, 64, 64]),
    "u255-s511": dict(kind="normal", family="s511", B=1, T=300, V=57, L=255, rows=[255], lens=None),
    "ldv-pad": dict(kind="normal", family="long", B=3, T=64, V=57, L=40, rows=[32, 31, 1], lens=[64, 40, 1], ldv=64),
    "t17-blocks": dict(kind="normal", family="long", B=3, T=17, V=57, L=6, rows=[2, [5, 5, 9], 4], lens=[16, 17, 15]),
}


# Worst error of this model's gradient run in float32 against its float64 run over the cases of a family (gradients of magnitude <= 1,
# absolute; measured on the CPU and held by tests/test_ctc_host.py): the error grows with the size of the log-domain quantities, a
# float32 ulp at |alpha + beta| ~ nll (nll up to 66 in `short`, 268 in `peaked`, 478 in `long`, 1112 in `s511`).  The operator's dlogits
# bound is 4 x this figure (tests/test_gpu_ctc.py); the factor covers another summation order.
F32_MODEL_ERR = {"short": 7.8e-6, "offset": 7.7e-6, "peaked": 3.1e-5, "long": 9.2e-5, "s511": 3.1e-4}


def op_case(name):
    """(logits (B, T, V) float32, y (B, L) int32, lens or None) of one operator case; a pure function of the name."""
    c = OP_CASES[name]
    seed = sum(ord(ch) for ch in name)
    rng = np.random.default_rng(seed + 1)
    x = op_logits(c["kind"], c["B"], c["T"], c["V"], seed)
    y = rng.integers(0, UNK_ID, size=(c["B"], c["L"])).astype(np.int32)
    for b, r in enumerate(c["rows"]):
        labels = list(r) if isinstance(r, list) else [int(v) for v in rng.integers(UNK_ID, c["V"], size=int(r))]
        pos = np.sort(rng.choice(c["L"], size=len(labels), replace=False))
        y[b, pos] = labels
    lens = None if c["lens"] is None else np.asarray(c["lens"], np.int32)
    return x, y, lens


# ------------------------------------------------------------------ the oracle with the auxiliary loss
def head_params(H, V, seed=77, dtype=np.float32):
    """ctc_out/W (V, H) LeCun normal, ctc_out/b (V,) small and non-zero (so that a wrong bias gradient or a dropped bias shows)."""
    rng = np.random.default_rng(seed)
    return {"ctc_out/W": (rng.standard_normal((V, H)) / np.sqrt(H)).astype(dtype), "ctc_out/b": (0.1 * rng.standard_normal(V)).astype(dtype)}


def t2_lens(cnn_layers, x_lens):
    """Frames per row behind the CNN (the time formula of every layer, no pooling)."""
    out = []
    for n in x_lens:
        t = int(n)
        for l in cnn_layers:
            t = R.conv_out(t, l["ksize"][0], l["stride"][0], l["pad"][0])
        out.append(t)
    return np.asarray(out, np.int64)


class CTCHead(F.Function):
    """weight / B * sum_b nll_b over logits = enc W^T + b, computed in the dtype of enc; records row_nll and n_infeasible."""

    def __init__(self, y, lens, weight):
        self.y, self.lens, self.weight = np.asarray(y), lens, float(weight)

    def forward(self, xs):
        enc, W, b = xs
        dt = enc.dtype.type
        self.enc, self.W = enc, W
        logits = enc.dot(W.T) + b
        r = ctc_loss_grad(logits, self.y, self.lens, UNK_ID, PAD_ID, scale=self.weight / enc.shape[0], dtype=dt)
        self.row_nll, self.n_infeasible, self.g = r["row_nll"], r["n_infeasible"], r["dlogits"]
        return np.asarray(r["loss"], dtype=enc.dtype)

    def backward(self, gys):
        g = self.g * gys[0]
        return g.dot(self.W), np.einsum("btv,bth->vh", g, self.enc), g.sum(axis=(0, 1))


@contextlib.contextmanager
def ctc_oracle(weight, x_lens=None):
    """Inside: RefModel.forward_loss of a model that has ctc_out/W returns loss_attention + weight * mean_b nll_b (x_lens: frames per row
    in front of the CNN, None = all of them) and leaves the term, the rows and the count on the model (ctc_term, ctc_rows, ctc_infeasible)."""
    orig = R.RefModel.forward_loss

    def forward_loss(self, X, y, *a, **k):
        loss = orig(self, X, y, *a, **k)
        if "ctc_out/W" not in self.p or not weight:
            return loss
        lens = None if x_lens is None else t2_lens(self.cnn_layers, x_lens)
        yy = np.asarray(y.data if isinstance(y, F.Variable) else y)
        head = CTCHead(yy, lens, weight)
        term = head(self.enc_states, self.p["ctc_out/W"], self.p["ctc_out/b"])
        self.ctc_term, self.ctc_rows, self.ctc_infeasible = float(term.data), head.row_nll, head.n_infeasible
        return loss + term
    R.RefModel.forward_loss = forward_loss
    try:
        yield
    finally:
        R.RefModel.forward_loss = orig
