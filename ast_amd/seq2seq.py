"""Drop-in for the reference's model class (seq2seq.py:22-568): SpeechEncoderDecoder(gpuid, cfg) with the same
method names, argument meaning and state protocol, running on libastk.so (hand-written HIP for gfx950).

PyTorch is used only as the owner of device memory and streams; every arithmetic step of the hot path is a
C-ABI call (include/astk.h).  There is no CPU / eager-PyTorch fallback: without the HIP library and a GPU
the compute methods raise.
"""
import ctypes as C
import os
import random

import numpy as np
import torch

from . import _lib
from ._lib import (CnnDesc, CnnLayerGrads, CnnLayerParams, DecoderDesc, DecoderGrads, DecoderParams, LstmGrads,
                   LstmParams, LstmStackDesc, check)
from .params import ParamArena, init_values, param_shapes


class _Config:
    """Stand-in for chainer.config / chainer.using_config('train', flag) (nn.py:174, 216, 248)."""
    train = True


config = _Config()


class using_config:
    def __init__(self, name, value):
        assert name == "train"
        self.value = value

    def __enter__(self):
        self.old = config.train
        config.train = self.value

    def __exit__(self, *a):
        config.train = self.old


class Link:
    """What `model[name]` returns (nn.py:113-116 calls .disable_update(); copy_params.py reads child params)."""

    def __init__(self, model, name):
        self._model, self.name = model, name

    def disable_update(self):
        self._model._frozen.add(self.name)

    def enable_update(self):
        self._model._frozen.discard(self.name)

    def namedparams(self):
        a = self._model.arena
        return [(k, v) for k, v in a.views.items() if k.split("/")[0] == self.name]


def raise_if_aborted(status, where="train step"):
    """`status` = the persistent kernels' sticky status word as read back next to the loss (include/astk.h
    astk_persist_status_snapshot).  Non-zero: a bounded spin timed out (the grid was not fully resident: another tenant on the GPU,
    RCCL kernels holding CUs, a partitioned device), the kernels drained, and the step's loss and gradients are garbage."""
    mask = int(status)
    if mask:
        names = [n for b, n in ((1, "encoder forward"), (2, "encoder backward"), (4, "decoder forward"), (8, "decoder backward"),
                                (16, "reported by a peer rank of the data-parallel job")) if mask & b]
        _lib.load().astk_persist_status(None, 1)          # clear the sticky word: the caller may retry (e.g. with the *.persist knobs at 0)
        raise _lib.AstkError(f"{where}: persistent kernel(s) timed out waiting for a peer workgroup ({', '.join(names)}); the results "
                             "of this step are invalid.  The whole grid must be resident (one workgroup per CU); set "
                             "the tuning knobs lstm.persist / dec.persist to 0 (ast_amd._lib.set_tuning) to use the per-launch kernels on a shared device")


def draw_flags_and_targets(yh, teach_ratio, random_out, V, randint, rank=None, world=None, gather=None):
    """forward_loss's draws from the seeded Python `random` stream in the reference's order (seq2seq.py:431-436, 456-465): per decoder
    step one teacher-forcing coin (0 < i < L-2), then one draw per target >= 4 of THE BATCH -- above `random_out` the scored target is
    replaced by randint(4, V + 1), clamped to V - 1 (quirk Q8).  Returns (flags, scored targets of the local rows).
    Data parallelism: the stream also feeds next epoch's shuffles and must stay IDENTICAL on every rank, but the number of draws depends
    on the targets -- and the ranks hold different rows.  So every rank makes the draws of the WHOLE global batch, in the row order of
    the unsharded batch (the loader gives rank r rows r::world: global row b * world + r), and keeps the replacements of its own rows:
    the `y` of all ranks is gathered first (`gather(yh) -> [yh of rank 0, ..]`; default torch.distributed.all_gather_object)."""
    from . import dist as adist
    world = adist.world_size() if world is None else world
    rank = adist.rank() if rank is None else rank
    B, L = yh.shape
    S = L - 1
    tg = yh.copy()
    if world > 1:
        if gather is None:
            def gather(a):
                out = [None] * world
                td_ = __import__("torch.distributed", fromlist=["x"])
                td_.all_gather_object(out, np.ascontiguousarray(a))
                return out
        parts = gather(yh)
        assert len(parts) == world and all(p.shape == yh.shape for p in parts), "shards of one bucketed batch share (B, L) (dataloader.get_batch)"
        rows = [(parts[g % world], g // world, g % world == rank) for g in range(B * world)]
    else:
        rows = [(yh, b, True) for b in range(B)]
    flags = []
    for i in range(S):
        flags.append(int(random.random() < teach_ratio) if 0 < i < L - 2 else 1)
        for src, b, mine in rows:
            if int(src[b, i + 1]) >= 4 and random.random() > random_out:
                if mine:
                    tg[b, i + 1] = min(int(randint(4, V + 1)), V - 1)
    return flags, tg


def ctc_count_of(word):
    """The int32 that astk_ctc_loss wrote into a float slot of the loss buffer (read back as a Python float)."""
    return int(np.float32(word).view(np.int32))


class LossData:
    """`loss.data` (nn.py:189: `float(loss.data)`): the 0-d device scalar, read through the persistent kernels' status word.  float(),
    .item(), .tolist() and NumPy conversion all read the [loss, status] pair in ONE copy and raise AstkError when a kernel of the step
    timed out -- a drop-in caller that only ever touches `.data` cannot train on with garbage.  `.tensor` is the raw 0-d tensor (no
    check, no synchronisation) for callers that keep the value on the device."""

    def __init__(self, pair, quad=None, model=None):
        self._pair = pair
        self._quad, self._model = quad, model     # a step with the CTC branch: [loss, status, rows without a path (int32), attention loss]

    @property
    def tensor(self):
        return self._pair[0]

    def _checked(self):
        if self._quad is not None:
            v = self._quad.tolist()               # the same one copy, 16 bytes instead of 8
            self._model.ctc_infeasible = ctc_count_of(v[2])
        else:
            v = self._pair.tolist()
        raise_if_aborted(v[1])
        return v[0]

    def __float__(self):
        return self._checked()

    def item(self):
        return self._checked()

    def tolist(self):
        return self._checked()

    def __array__(self, dtype=None, copy=None):
        return np.asarray(self._checked(), dtype=dtype or np.float32)

    def __getattr__(self, name):              # shape / dtype / device / clone() ... of the 0-d tensor
        if name.startswith("_"):              # (copy / pickle probe dunder names before _pair exists: no recursion)
            raise AttributeError(name)
        return getattr(self._pair[0], name)


class Loss:
    """What forward_loss returns: `.data` (the 0-d loss, status-checked when it is read: LossData), float(), `.backward()`
    (nn.py:175-189).  `.pair` = [loss, status] on the device: the status word of the persistent kernels rides next to the scalar, so one
    read-back serves both."""

    def __init__(self, model, pair, quad=None):
        self._model = model
        self.pair = pair
        self.quad = quad          # None, or (a step with ctc_weight > 0) [loss, status, int32 count of rows without a CTC path, attention loss]
        self.data = LossData(pair, quad, model)

    def backward(self):
        self._model._backward()

    def __float__(self):
        return float(self.data)


class _Pending:
    """A decode on the device path: its words [.., status word (float), .., results] -- and the float words of a second buffer, forced
    alpha -- on their way into pinned memory.  result() waits for the copy, raises if the status word (at index `status_at`) reports a
    timed-out kernel, and returns parse(words, second buffer's words or None).  `keep` holds the launch's device inputs until then."""

    def __init__(self, host, host2, event, status_at, where, parse, keep=None):
        self.host, self.host2, self.event, self.status_at, self.where, self.parse, self.keep = host, host2, event, status_at, where, parse, keep

    def result(self):
        self.event.synchronize()
        self.keep = None
        v = self.host.numpy()
        raise_if_aborted(v[self.status_at:self.status_at + 1].view(np.float32)[0], self.where)
        return self.parse(v, None if self.host2 is None else self.host2.numpy())


class ScoredPrediction:
    """What predict_scored returns: `tokens` (B, n_steps) int32 exactly as predict() returns them, `logp` (B, n_steps) float32 the
    log-probability of each emitted token, `nll` (B, n_steps) float32 the class-weighted negative log-likelihood of the target of each
    step (0 where a step has no target; None without targets), `n_steps`, and the two reductions (float64, on the host):
      loss     = sum over the steps of the mean over the B rows of nll -- the free-running dev loss of the reference's older trainer
                 (enc_dec.py:372-429: rows that have emitted EOS keep contributing, PAD targets weigh 0); None without targets;
      score[b] = sum of logp[b, :k], k = the position of row b's first `end_token` plus one, or n_steps.
    `kept` (B, n_steps) int32: truncated sampling's kept count m of every draw (sample(top_k=, top_p=)); None on every other path."""

    def __init__(self, tokens, logp, nll, end_token, kept=None):
        self.tokens, self.logp, self.nll, self.kept = tokens, logp, nll, kept
        self.n_steps = int(tokens.shape[1])
        self.loss = None if nll is None else float(nll.astype(np.float64).sum(axis=0).sum() / max(tokens.shape[0], 1))
        is_end = tokens == end_token
        k = np.where(is_end.any(axis=1), is_end.argmax(axis=1) + 1, self.n_steps)
        keep = np.arange(self.n_steps)[None, :] < k[:, None]
        self.score = np.where(keep, logp.astype(np.float64), 0.0).sum(axis=1)


def scored_from_rows(words, n_steps, B, stop_limit, has_nll, end_token, has_kept=False):
    """The read-back words of a scored greedy decode -- step-major [tokens | logp | nll], each (stop_limit, B), the last two float32
    bit patterns -- cut to the first n_steps steps and reduced (ScoredPrediction).  has_kept: the third block is truncated sampling's
    int32 kept counts instead."""
    n, sb = int(n_steps), int(stop_limit) * B
    rows = lambda k: words[k * sb:k * sb + n * B].reshape(n, B).T.copy()
    return ScoredPrediction(rows(0), rows(1).view(np.float32), rows(2).view(np.float32) if has_nll else None, end_token,
                            rows(2) if has_kept else None)


# ---- sampled decoding: the noise contract of include/astk.h ("sampled decoding on the device"), restated on the host
_M64 = (1 << 64) - 1


def mix64(z):
    """The splitmix64 finaliser of csrc/common.h on Python integers."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample_row_key(seed, stream):
    """row_key(seed, stream) = mix64(seed ^ mix64(stream)): the key of one batch row of a sampled decode (astk_sample_row_key)."""
    return mix64((int(seed) & _M64) ^ mix64(int(stream) & _M64))


def gumbel_noise(row_key, step, V):
    """The host mirror of csrc/common.h sample_gumbel: (u, g) for the classes 0..V-1 of one row and decoder step -- u the float32 uniform
    of the contract, to the bit, g = -ln(-ln(u)) in float64 (the device's float32 g lies within 5e-6 of it)."""
    n = np.arange(V, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(row_key) ^ ((np.uint64(step) << np.uint64(32)) | n)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    u = ((z >> np.uint64(40)) + np.uint64(1)).astype(np.float32) * np.float32(1.0 / 16777217.0)
    return u, -np.log(-np.log(u.astype(np.float64)))


def checked_temperature(temperature):
    """1 / temperature as the float32 the library takes; ValueError unless temperature is finite and > 0 and its inverse is a finite
    positive float32."""
    t = float(temperature)
    if not (np.isfinite(t) and t > 0):
        raise ValueError(f"sample: temperature must be finite and > 0, got {temperature!r}")
    with np.errstate(over="ignore", under="ignore"):
        inv = float(np.float32(1.0 / t))
    if not (np.isfinite(inv) and inv > 0):
        raise ValueError(f"sample: 1 / temperature must be a finite positive float32, got temperature {temperature!r} (inverse {inv!r})")
    return inv


# ---- truncated sampling: the contract of include/astk.h ("truncated sampling on the device"), top-k and top-p / nucleus
SAMPLE_MAX_TOPK = 16      # ASTK_SAMPLE_MAX_TOPK


def checked_truncation(top_k, top_p, V=None):
    """(top_k, top_p) as the library takes them, or (None, 1.0) for the untruncated draw; ValueError unless top_p is a number in (0, 1],
    top_k is None or an integer in 1..16 (and at most V, when given), and top_p < 1 comes with a top_k."""
    try:
        p = float(top_p)
    except (TypeError, ValueError):
        p = float("nan")
    if not (np.isfinite(p) and 0.0 < p <= 1.0):
        raise ValueError(f"sample: top_p must be a number in (0, 1], got {top_p!r}")
    if top_k is None:
        if p < 1.0:
            raise ValueError(f"sample: top_p = {top_p!r} needs top_k: the nucleus is taken among top_k <= {SAMPLE_MAX_TOPK} candidates")
        return None, 1.0
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or not 1 <= int(top_k) <= SAMPLE_MAX_TOPK:
        raise ValueError(f"sample: top_k must be an integer in 1..{SAMPLE_MAX_TOPK}, got {top_k!r}")
    if V is not None and int(top_k) > int(V):
        raise ValueError(f"sample: top_k = {int(top_k)} is above the vocabulary size V = {int(V)}")
    return int(top_k), float(np.float32(p)) if p < 1.0 else 1.0


def truncated_pick(logits, g, inv_temp, top_k, top_p):
    """One step's truncated draw (include/astk.h, "truncated sampling on the device", steps 1 to 5) as a pure function of torch tensors,
    on any device: logits (B, V) float32, g (B, V) the noise of (row key, step, class id), inv_temp, top_k in 1..16, top_p in (0, 1].
      1. xs = logits * inv_temp in float32;
      2. the top_k largest xs are the candidates, by a stable descending sort of the float32 xs: higher values first, among equal
         values the lower token id first;
      3. q = exp(xs_j - LSE_K) over the candidates; m = the smallest count >= 1 whose prefix sum of q is >= top_p, K if none reaches it,
         and K exactly for top_p == 1 (prefix sums and LSE in float64);
      4. the token is the candidate j < m with the largest z_j = xs_j + g at its id (float32), among equal z the lower token id;
      5. logp = xs_tok - LSE over the m kept (float64): the log-probability under the distribution actually sampled, NOT the model's
         full-softmax log-probability (score() gives that).
    Returns (tokens (B,) int32, logp (B,) float64, kept (B,) int32)."""
    K = int(top_k)
    xs = logits.to(torch.float32) * float(inv_temp)
    vals, ids = torch.sort(xs, dim=1, descending=True, stable=True)
    vals, ids = vals[:, :K], ids[:, :K]
    e = torch.exp(vals.double() - vals[:, :1].double())
    if float(top_p) >= 1.0:
        m = torch.full((xs.shape[0],), K, dtype=torch.int64, device=xs.device)
    else:
        cum = torch.cumsum(e / e.sum(dim=1, keepdim=True), dim=1)
        m = ((cum < float(top_p)).sum(dim=1) + 1).clamp(max=K)
    kept = torch.arange(K, device=xs.device)[None, :] < m[:, None]
    z = torch.where(kept, vals + g.to(torch.float32).gather(1, ids), torch.full_like(vals, float("-inf")))
    best = z == z.max(dim=1, keepdim=True).values
    tok = torch.where(best, ids, torch.full_like(ids, xs.shape[1])).min(dim=1).values
    x_tok = xs.gather(1, tok[:, None])[:, 0].double()
    logp = (x_tok - vals[:, 0].double()) - torch.log(torch.where(kept, e, torch.zeros_like(e)).sum(dim=1))
    return tok.to(torch.int32), logp, m.to(torch.int32)


class ForcedScore:
    """What score() returns for targets y (B, L), S = L - 1 steps, step s fed y[:, s] and scored against y[:, s + 1]:
      logp (B, S) float32      log p(y[b, s + 1]), unweighted;   logp_max (B, S) the log-probability of the argmax;
      pred (B, S) int32        the argmax (first maximum);        weight (B, S) = mask_pad_id[y[:, 1:]] (0 at PAD targets);
      alpha (B, S, T'') float32 the attention rows, or None;
    and the reductions (float64, on the host):
      score[b]    = sum of logp[b] where weight is non-zero, n_tokens[b] = how many such positions;
      loss        = sum over the steps of the mean over the B rows of weight * (-logp): the value of eval-mode
                    forward_loss(X, y, teach_ratio=1) (PAD targets weigh 0, every step divides by B)."""

    def __init__(self, logp, logp_max, pred, weight, alpha=None):
        self.logp, self.logp_max, self.pred, self.alpha = logp, logp_max, pred, alpha
        self.weight = np.asarray(weight, dtype=np.float32)
        keep = self.weight != 0
        lp64 = logp.astype(np.float64)
        self.score = np.where(keep, lp64, 0.0).sum(axis=1)
        self.n_tokens = keep.sum(axis=1).astype(np.int64)
        self.loss = float((self.weight.astype(np.float64) * -lp64).sum(axis=0).sum() / max(logp.shape[0], 1))


def forced_from_rows(words, B, S, weight, alpha=None):
    """The read-back words of a forced decode -- step-major [logp | logp_max | pred], each (S, B), the first two float32 bit
    patterns -- as a ForcedScore; weight (B, S) as in ForcedScore."""
    sb = int(S) * int(B)
    rows = lambda k: words[k * sb:(k + 1) * sb].reshape(S, B).T.copy()
    return ForcedScore(rows(0).view(np.float32), rows(1).view(np.float32), rows(2), weight, alpha)


def checked_targets(y, V):
    """y as a (B, L >= 2) int32 host array; ValueError for another shape or an id outside [0, V)."""
    if isinstance(y, torch.Tensor):
        y = y.detach().cpu().numpy()
    y = np.ascontiguousarray(np.asarray(y))
    if y.ndim != 2 or y.shape[1] < 2:
        raise ValueError(f"score: y must be (B, L >= 2), got {tuple(y.shape)}")
    if not np.issubdtype(y.dtype, np.integer):
        raise ValueError(f"score: y must hold integer token ids, got {y.dtype}")
    if y.size and (int(y.min()) < 0 or int(y.max()) >= int(V)):
        raise ValueError(f"score: token ids must lie in [0, V = {int(V)}), got [{int(y.min())}, {int(y.max())}]")
    return y.astype(np.int32, copy=False)


def checked_label_smoothing(eps, what="label_smoothing"):
    """eps as a float; ValueError for anything but a finite number with 0 <= eps < 1 (a bool or a string is no number)."""
    import numbers
    if isinstance(eps, bool) or not isinstance(eps, (numbers.Real, np.floating, np.integer)):
        raise ValueError(f"{what} must be a number with 0 <= eps < 1, got {eps!r}")
    eps = float(eps)
    if not np.isfinite(eps) or eps < 0.0 or eps >= 1.0:
        raise ValueError(f"{what} must be finite with 0 <= eps < 1, got {eps!r}")
    return eps


def checked_ctc_weight(weight, has_head, what="ctc_weight"):
    """weight of the auxiliary CTC loss as a float; ValueError for anything but a finite number >= 0 (a bool or a string is no number),
    and for a positive weight on a model without the head (model_cfg.json: rnn_config.ctc)."""
    import numbers
    if isinstance(weight, bool) or not isinstance(weight, (numbers.Real, np.floating, np.integer)):
        raise ValueError(f"{what} must be a number >= 0, got {weight!r}")
    weight = float(weight)
    if not np.isfinite(weight) or weight < 0.0:
        raise ValueError(f"{what} must be finite and >= 0, got {weight!r}")
    if weight > 0.0 and not has_head:
        raise ValueError(f"{what} = {weight!r} needs the CTC head: set rnn_config.ctc = true in model_cfg.json")
    return weight


def checked_ctc_beam_width(N, C, V=None):
    """(N, C) of a CTC prefix beam search as ints within astk_ctc_beam's bounds: 1 <= N <= 16, 1 <= C <= min(16, V - UNK_ID)."""
    for name, v in (("N", N), ("C", C)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"ctc_beam: {name} must be an integer, got {v!r}")
    if not 1 <= N <= _lib.CTC_BEAM_MAX_N:
        raise ValueError(f"ctc_beam: the beam width N must lie in 1..{_lib.CTC_BEAM_MAX_N}, got {N}")
    top = _lib.CTC_BEAM_MAX_C if V is None else min(_lib.CTC_BEAM_MAX_C, int(V) - UNK_ID)
    if not 1 <= C <= top:
        raise ValueError(f"ctc_beam: C labels per frame must lie in 1..{top}, got {C}")
    return int(N), int(C)


def checked_x_lens(x_lens, B, T):
    """Frames per row in front of the CNN as a (B,) int64 host array; ValueError for another count, a non-integer dtype or a length
    outside 1..T.  A host array by contract: the lengths are mapped through the CNN's time formula on the host."""
    if isinstance(x_lens, torch.Tensor):
        if x_lens.device.type != "cpu":
            raise ValueError("x_lens must be a host array (the loader has the true lengths on the host)")
        x_lens = x_lens.numpy()
    x_lens = np.asarray(x_lens)
    if x_lens.ndim != 1 or x_lens.shape[0] != int(B):
        raise ValueError(f"x_lens must name B = {int(B)} rows, got shape {tuple(x_lens.shape)}")
    if not np.issubdtype(x_lens.dtype, np.integer):
        raise ValueError(f"x_lens must hold integers, got {x_lens.dtype}")
    if int(x_lens.min()) < 1 or int(x_lens.max()) > int(T):
        raise ValueError(f"x_lens must lie in 1..T = {int(T)}, got [{int(x_lens.min())}, {int(x_lens.max())}]")
    return x_lens.astype(np.int64)


PAD_ID, GO_ID, EOS_ID, UNK_ID = 0, 1, 2, 3      # the vocabulary's reserved ids (the CTC branch: blank = PAD_ID, labels from UNK_ID on)
ROWS_MAX = 32       # the device loop's batch (include/astk.h: B <= 32)


def checked_row_lens(lens, B, T):
    """lens as a (B,) int32 host array; ValueError for another count, a non-integer dtype or a length outside 1..T."""
    if isinstance(lens, torch.Tensor):
        lens = lens.detach().cpu().numpy()
    lens = np.asarray(lens)
    if lens.ndim != 1 or lens.shape[0] != int(B):
        raise ValueError(f"RowBatch: lens must name B = {int(B)} rows, got shape {tuple(lens.shape)}")
    if not np.issubdtype(lens.dtype, np.integer):
        raise ValueError(f"RowBatch: lens must hold integers, got {lens.dtype}")
    if int(lens.min()) < 1 or int(lens.max()) > int(T):
        raise ValueError(f"RowBatch: lengths must lie in 1..T''max = {int(T)}, got [{int(lens.min())}, {int(lens.max())}]")
    return np.ascontiguousarray(lens.astype(np.int32))


def cnn_out_lens(cnn_layers, n):
    """Output steps of every CNN layer for an utterance of n frames (the time formula of astk_conv_bn_relu_out_dims, no pooling):
    [T_0, .., T''].  ValueError where the library would refuse the utterance alone (a padded input shorter than the kernel)."""
    out, t = [], int(n)
    for i, l in enumerate(cnn_layers):
        kt, st, pt = int(l["ksize"][0]), int(l["stride"][0]), int(l["pad"][0])
        if t < 1 or t + 2 * pt < kt:
            raise ValueError(f"cnn_out_lens: {int(n)} frames are too short for layer {i} (kt = {kt}, pad = {pt}, input {t})")
        t = (t + 2 * pt - kt) // st + 1
        out.append(t)
    return out


def input_span(cnn_layers, start, end, x_len):
    """The input frames [lo, hi) behind the encoder frames [start, end): output step j of a layer with kernel kt, stride st and pad pt
    reads its input steps j * st - pt .. j * st - pt + kt - 1, so through the layers from the last to the first
        lo <- lo * st - pt   (from lo = start),      hi <- hi * st - pt + kt - 1   (from hi = end - 1),
    and the span is [lo, hi + 1) clipped to [0, x_len]: the receptive start of the first frame and the receptive end of the last.  Both
    ends are monotone in the frame, so ordered segments stay ordered; neighbours overlap by the receptive fields' overlap."""
    lo, hi = int(start), int(end) - 1
    for l in reversed(cnn_layers):
        kt, st, pt = int(l["ksize"][0]), int(l["stride"][0]), int(l["pad"][0])
        lo, hi = lo * st - pt, hi * st - pt + kt - 1
    return min(max(lo, 0), int(x_len)), min(max(hi + 1, 0), int(x_len))


def plan_encode_batches(lens, max_rows=ROWS_MAX):
    """Utterances -> encoder calls of at most max_rows rows: the indices ordered by length, longest first (ties in index order), cut
    into consecutive batches, so that a batch pads its rows to a length close to their own.  Host only."""
    max_rows = int(max_rows)
    if max_rows < 1:
        raise ValueError(f"plan_encode_batches: max_rows = {max_rows} must be at least 1")
    order = sorted(range(len(lens)), key=lambda u: (-int(lens[u]), u))
    return [order[i:i + max_rows] for i in range(0, len(order), max_rows)]


class RowBatch:
    """Rows of DIFFERENT utterances for the decode entry points (`rows=` of predict / predict_scored / sample / score): `enc`
    (B, T''max, H) the rows' encoder memories, each padded behind its own length, `lens` (B,) int32 on the host, 1 <= lens[b] <= T''max,
    and the decoder states `c0` / `h0` (n_layers, B, H).  Row b attends over enc[b, :lens[b]] only and decodes as it would alone (what
    lies behind a row's length is never read into a result).  SpeechEncoderDecoder.encode_rows builds one from utterances; built from
    tensors directly it takes any lengths.  At most 32 rows: the device loop's batch."""

    def __init__(self, enc, lens, c0, h0):
        enc, c0, h0 = (torch.as_tensor(t) for t in (enc, c0, h0))
        if enc.dim() != 3 or enc.shape[0] < 1 or enc.shape[1] < 1:
            raise ValueError(f"RowBatch: enc must be (B >= 1, T''max >= 1, H), got {tuple(enc.shape)}")
        B, T, H = (int(v) for v in enc.shape)
        if B > ROWS_MAX:
            raise ValueError(f"RowBatch: at most {ROWS_MAX} rows, got {B}")
        for name, t in (("c0", c0), ("h0", h0)):
            if t.dim() != 3 or int(t.shape[1]) != B or int(t.shape[2]) != H or t.shape != c0.shape:
                raise ValueError(f"RowBatch: {name} must be (n_layers, B = {B}, H = {H}), got {tuple(t.shape)}")
        self.lens = checked_row_lens(lens, B, T)
        self.enc, self.c0, self.h0 = enc, c0, h0

    @property
    def B(self):
        return int(self.enc.shape[0])

    @property
    def T(self):
        return int(self.enc.shape[1])

    def row(self, b):
        """Row b alone, its memory cut at its length."""
        n = int(self.lens[b])
        return RowBatch(self.enc[b:b + 1, :n], [n], self.c0[:, b:b + 1], self.h0[:, b:b + 1])


class _Ready:
    def __init__(self, value):
        self.value = value

    def result(self):
        return self.value


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_LAZY_CLEARGRADS = os.environ.get("ASTK_LAZY_CLEARGRADS", "1") != "0"      # (0: cleargrads() always fills at once -- A/B runs)


class SpeechEncoderDecoder:
    def __init__(self, gpuid, cfg):
        self.gpuid = gpuid
        self.cfg = cfg
        rc, cc = cfg["rnn_config"], cfg["cnn_config"]
        # Optional features of the reference's model (seq2seq.py:43-57, 81-121, 244-291, 369-394; none is set by a shipped config).
        # They run on per-launch kernels / layer-by-layer stacks instead of the persistent kernels of the default model: `paths()` says so.
        self.rnn_ln = bool(rc.get("ln", False))
        self.rnn_linear_proj = bool(rc.get("linear_proj", False))
        self.feed_attn = bool(rc.get("feed_attn", True))
        n_attn = int(rc.get("n_attn", 1))
        if not 1 <= n_attn <= _lib.MAX_ATTN:
            raise ValueError(f"rnn_config.n_attn = {n_attn}: 1..{_lib.MAX_ATTN} attention heads are supported")
        if not rc["bi_rnn"]:
            self.n_dirs = 1
        else:
            self.n_dirs = 2
        self.cnns = [f"CNN_{i}" for i in range(len(cc["cnn_layers"]))]
        self.cnn_bn = cc["bn"]
        self.rnn_enc = [f"L{i}_enc" for i in range(rc["enc_layers"])]
        self.rnn_rev_enc = [f"L{i}_rev_enc" for i in range(rc["enc_layers"])] if rc["bi_rnn"] else []
        self.rnn_dec = [f"L{i}_dec" for i in range(rc["dec_layers"])]
        self.bi_rnn = rc["bi_rnn"]
        self.n_attn = n_attn
        self.enc_variant = None         # ast_amd.enc_variants.LayerNormEncoder / LinearProjEncoder (set in materialize)
        self.proj_bn_N = [0] * max(0, rc["enc_layers"] - 1)     # BatchNormalization N of the enc_proj{i}_bn links (one call per time step)
        self.h = rc["hidden_units"] // 2 if rc["bi_rnn"] else rc["hidden_units"]
        self.H, self.E, self.A = rc["hidden_units"], rc["embedding_units"], rc["attn_units"]
        self.V = rc.get("dec_vocab_size")
        self.device = torch.device(f"cuda:{gpuid}") if gpuid is not None and gpuid >= 0 else torch.device("cpu")
        self.arena = None
        self.persist = {}
        self.in_dim = None
        self._frozen = set()
        self._ws = {}
        self._shape_cache = {}
        self._pools = {}                # grow-only device buffers shared by all batch shapes (_pool)
        self._bstate = {}               # small zero-initialised state tensors, per batch size
        self.inject = {}          # test hooks: enc_masks / emb_mask / rnn_masks / noise / use_truth
        self.rng_seed = 0x5EED
        self._rng_offset = 0
        self._predrawn = {}             # random tensors of the current train step drawn ahead in one launch (_predraw)
        self._pending_flags = None      # the step's teacher-forcing flags on their way to the device with that launch
        self.bn_N = 0                   # training-mode forward passes so far = Chainer's BatchNormalization persistent N (A10)
        self.enc_states = None
        self.loss = 0
        self._cur = None
        self._dec_c = self._dec_h = None
        self._rows_alone = False        # inside the per-step path of a RowBatch: its rows decode one by one, off the device loop
        self.grad_buckets = None        # ast_amd.dist.GradBuckets under data parallelism: ranges are all-reduced as they become final
        self.stat_exchange = None       # ast_amd.dist.StatExchange: BatchNorm statistics over the global batch (train mode only)
        # Work BESIDE the latency-bound encoder recurrences (round 6): an ORDINARY second stream carries (i) the decoder's parameter
        # gradients beside the encoder's backward recurrence and (ii) -- inside the library, astk_lstm_stack_desc.side_stream -- the
        # time-chunked layer-0 products beside both recurrences; every launch on it is capped at the CUs the recurrence grid leaves
        # free, so neither order of dispatch can keep that grid from becoming resident.  (Rounds 1-5 needed CU-masked streams for
        # this and kept it opt-in: uncapped stream-K grids that got the CUs first blocked the recurrence.)  ASTK_SIDE_STREAM=0: in line.
        self.side_stream_on = os.environ.get("ASTK_SIDE_STREAM", "1") != "0"
        self._side = None
        self._side_by_main = {}
        self.mask_pad_id = None
        self._pinned = {}               # pinned read-back buffers of the decode modes, per (mode, slot) (_readback)
        self.last_score_path = None     # "device" (astk_forced_score) | "steps": which path the last score() took
        self.last_beam_path = None      # "device" (astk_beam_decode) | "steps" (decode_beam_batch): which path the last decode_beam_device took
        self.last_beam_steps = []       # ... and, on the device path, the steps each of its launches ran (n_steps)
        self.last_predict_path = None   # "device" (astk_greedy_decode) | "steps" (the per-step loop): which path the last predict() took
        # Evaluation-mode encodings of several utterances (encode_rows, decode_beam_batch / _device): False = every utterance alone at
        # batch 1; True = the distinct utterances in padded batches with per-row lengths (astk_*_fwd_rows), each row what it gives alone.
        self.batch_encode = False
        self.last_encode_path = None    # "batched" | "alone": which of the two the last such encoding took
        # Arithmetic of the batched products, per model (-> the descriptors' `precision` / `gemm_operands` fields): None = the library's
        # process-wide default (bf16x3: exact f32 operands on the 16-bit matrix pipe); "bf16x3" | "f32" | "fp16x2" (narrower, opt-in);
        # gemm_operands "fp16" = single-term fp16 operands for the eligible products (BASELINE configs[4]; reduced precision).
        self.gemm_precision = None
        self.gemm_operands = None
        # Deterministic backward (-> the descriptors' `deterministic` field, astk.h): every accumulated sum of the backward pass in a fixed
        # order -- split tiles of the batched products through the fix-up workspace instead of float atomics, ordered column / embedding /
        # bias sums, no side-stream work.  A few per cent slower; two runs over the same batches are then bit-identical in EVERY gradient,
        # which is what lets a soak see a hand-off race in the backward half of the step (train_cfg.json: extras.deterministic).
        self.deterministic = False
        # Auxiliary CTC loss on the encoder states (extension): rnn_config.ctc adds the head ctc_out/W, ctc_out/b;
        # forward_loss(ctc_weight=) trains on loss_attention + ctc_weight * mean_b nll_b.  Off (no head, or weight 0): nothing is
        # allocated and nothing is launched.
        self.ctc_head = bool(rc.get("ctc", False))
        self.ctc_nll = None             # (B,) device tensor: the rows' -log p of the last step with ctc_weight > 0 (+inf: no path)
        self.ctc_infeasible = 0         # rows without a path in that step: read with the loss, in the same copy (LossData)

    # ------------------------------------------------------------------ parameters
    def materialize(self, in_dim, values=None, seed=0):
        """Allocates the (lazily shaped, seq2seq.py:52,83) parameters once the feature dim is known."""
        if self.V is None:
            raise ValueError("cfg['rnn_config']['dec_vocab_size'] must be set (config.py:24 injects it)")
        train, persist = param_shapes(self.cfg, in_dim, self.V)
        self.in_dim = in_dim
        self.arena = ParamArena(train, self.device)
        vals = values if values is not None else init_values(self.cfg, in_dim, self.V, seed)
        self.arena.load(vals)
        self.persist = {k: torch.as_tensor(np.asarray(vals[k], dtype=np.float32)).to(self.device).contiguous() for k in persist}
        w = torch.ones(self.V, dtype=torch.float32)
        w[0] = 0                                             # seq2seq.py:152-156
        self.mask_pad_id = w.to(self.device)
        self._shape_cache.clear()
        if self.rnn_linear_proj:                             # (seq2seq.py:311-314: linear_proj takes precedence; that path has no LayerNorm)
            from .enc_variants import LinearProjEncoder
            self.enc_variant = LinearProjEncoder(self)
        elif self.rnn_ln:
            from .enc_variants import LayerNormEncoder
            self.enc_variant = LayerNormEncoder(self)
        return self

    def add_weight_noise(self, mu, sigma):
        """The OLD path's Gaussian weight noise (enc_dec.py:587-624, driven per epoch by nmt_run.py:850-853): N(mu, sigma) added, in place, to
        every LSTM's upward W and b and lateral W (encoder, reverse encoder, decoder) and to the decoder embedding.  Drawn on the
        device (the reference's draw is the unseeded global RNG, quirk Q7); inject['weight_noise'] = {name: tensor} replays given draws."""
        lib = self._require_gpu()
        names = []
        for n in self.rnn_enc + self.rnn_rev_enc + self.rnn_dec:
            names += [n + "/upward/W", n + "/upward/b", n + "/lateral/W"]
        names.append("embed_dec/W")
        for name in names:
            w = self.arena.views[name]
            if "weight_noise" in self.inject:
                z = self.inject["weight_noise"][name].to(self.device, torch.float32).contiguous()
            else:
                z = self._pool("weight_noise", (w.numel() + (w.numel() & 1),))[:w.numel()]
                check(lib.astk_fill_normal(_vp(z), w.numel(), float(mu), float(sigma), self.rng_seed ^ 0x5EED0015E, self._rng(w.numel() + 1), self._stream()))
            check(lib.astk_add_f32(_vp(w), _vp(z), w.numel(), self._stream()))

    def paths(self):
        """Which kernels this model's train step takes (bench.py / logs): the optional features leave the persistent kernels."""
        opts = [n for n, on in (("ln", self.rnn_ln), ("linear_proj", self.rnn_linear_proj), (f"n_attn={self.n_attn}", self.n_attn > 1),
                                ("feed_attn=false", not self.feed_attn), ("cnn bn=false", not self.cnn_bn),
                                ("dropout.out", bool(self.cfg["dropout"].get("out", 0))),
                                ("cnn_pool (max-pool, old path)", "cnn_pool" in self.cfg["cnn_config"])) if on]
        return {"options": opts,
                "encoder": "layer-by-layer one-layer stacks + " + ("Linear/BatchNorm/ReLU projections" if self.rnn_linear_proj else "LayerNorm kernels")
                if self.enc_variant is not None else "one stack call (persistent wavefront kernels when the shape fits)",
                "decoder": "per-launch loop (optional features)" if (self.rnn_ln or self.n_attn > 1 or not self.feed_attn or self.cfg["dropout"].get("out", 0))
                else "persistent loop when the shape fits",
                "ctc": "head ctc_out: one product + astk_ctc_loss behind the decoder forward, astk_ctc_head_bwd in front of the encoder backward, "
                       "when forward_loss gets ctc_weight > 0; nothing is launched at 0" if self.ctc_head
                else "off (no rnn_config.ctc head): nothing is allocated, nothing is launched"}

    def to_gpu(self, gpuid=None):
        if gpuid is not None and gpuid != self.gpuid:
            assert self.arena is None, "move before materialize()"
            self.gpuid = gpuid
            self.device = torch.device(f"cuda:{gpuid}")
        return self

    def __getitem__(self, name):
        return Link(self, name)

    def namedparams(self):
        return list(self.arena.views.items())

    def params(self):
        return list(self.arena.views.values())

    def cleargrads(self):
        """Zero gradients (nn.py:180 calls it between forward_loss and backward).  Behind a forward_loss on the device the fill is DEFERRED to
        the backward pass, whose first fill launch takes the arena along (a launch less per step); anything that reads the gradients before
        that performs it first (ParamArena.flush_zero), so the deferral cannot be observed."""
        if self.arena is None:
            return
        st = self._cur
        if st and st.get("train_mode") and "dd" in st and st.get("pending_backward") and _LAZY_CLEARGRADS:
            self.arena.defer_zero()
        else:
            self.arena.grad.zero_()

    def enabled_ranges(self):
        """Contiguous [offset, n) slices of the arena whose links have updates enabled (nn.py:113-116)."""
        out = []
        for name in self.arena.shapes:
            if name.split("/")[0] in self._frozen:
                continue
            o, n = self.arena.range_of(name)
            if out and out[-1][0] + out[-1][1] == o:
                out[-1] = (out[-1][0], out[-1][1] + n)
            else:
                out.append((o, n))
        return out

    # ------------------------------------------------------------------ plumbing
    def _require_gpu(self):
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("ast_amd compute path needs an MI355X GPU and libastk.so (no CPU fallback)")
        return _lib.load()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, key, nbytes):
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes:
            t = torch.empty(int(nbytes * 1.0) + 256, dtype=torch.uint8, device=self.device)
            self._ws[key] = t
        return t

    def _pool(self, name, shape, dtype=torch.float32):
        """A view of a persistent, grow-only device buffer: real batches come in hundreds of (T, L) combinations (bucket width 80
        frames, 2..max_pred targets), and a fresh set of 80 MB activation tensors per combination costs 40 ms per step in
        allocations and never gives the memory back.  Only data that is fully rewritten by every step lives here."""
        n = 1
        for d_ in shape:
            n *= int(d_)
        buf = self._pools.get(name)
        if buf is None or buf.numel() < n or buf.dtype != dtype:
            buf = torch.empty(int(n * 1.25) + 64, dtype=dtype, device=self.device)
            self._pools[name] = buf
            self._shape_cache.clear()          # cached views would keep the outgrown storage alive
        return buf[:n].view(shape)

    def _shape_state(self, B, T, D, L):
        """The descriptors, parameter tables and buffers of one batch shape (cached); the arithmetic the model currently asks for
        (`gemm_precision`, `gemm_operands`) goes into the descriptors' per-call fields (include/astk.h: ASTK_PREC_* / ASTK_OPERANDS_*)."""
        st = self._shape_state_cached(B, T, D, L)
        prec, ops = _lib.PREC_BY_NAME[self.gemm_precision], _lib.OPERANDS_BY_NAME[self.gemm_operands]
        for k in ("cd", "ld", "dd"):
            st[k].precision, st[k].gemm_operands = prec, ops
            st[k].deterministic = 1 if self.deterministic else 0
        return st

    def _shape_state_cached(self, B, T, D, L):
        key = (B, T, D, L)
        st = self._shape_cache.get(key)
        if st is not None:
            return st
        lib = self._require_gpu()
        if self.arena is None:
            self.materialize(D)
        dev = self.device
        cc = self.cfg["cnn_config"]["cnn_layers"]
        cd = CnnDesc()
        cd.B, cd.T, cd.D, cd.n_layers = B, T, D, len(cc)
        for i, l in enumerate(cc):
            cd.C[i] = l["out_channels"]
            cd.kt[i], cd.kf[i] = l["ksize"]
            cd.st[i], cd.sf[i] = l["stride"]
            cd.pt[i] = l["pad"][0]
            if l["pad"][1] != 0 or l.get("dilate", 1) != 1:
                raise NotImplementedError("frequency padding / dilation are not used by the shipped configs")
        cd.bn_eps, cd.bn_decay = 2e-5, 0.9
        cd.no_bn = 0 if self.cnn_bn else 1
        for i, (kt, kf) in enumerate(self.cfg["cnn_config"].get("cnn_pool", [])):     # OLD-path extra (enc_dec.py:444-456), -1 = whole extent
            cd.pool_t[i], cd.pool_f[i] = int(kt), int(kf)
        t2, f2, feat = C.c_int(), C.c_int(), C.c_int()
        check(lib.astk_conv_bn_relu_out_dims(C.byref(cd), C.byref(t2), C.byref(f2), C.byref(feat)))
        T2, feat = t2.value, feat.value
        rnn_in = self.arena.shapes["L0_enc/upward/W"][1]
        if feat != rnn_in:
            raise ValueError(f"feature dim {D} gives {feat} LSTM inputs but the model was built for {rnn_in} "
                             f"(in_dim {self.in_dim}); the reference's lazily-shaped links fix this at the first batch")
        a = self.arena
        cp = (CnnLayerParams * len(cc))()
        cg = (CnnLayerGrads * len(cc))()
        for i in range(len(cc)):
            n = f"CNN_{i}"
            cp[i].W, cg[i].dW = a.p(n + "/W"), a.g(n + "/W")
            if self.cnn_bn:
                cp[i].gamma, cp[i].beta = a.p(n + "_bn/gamma"), a.p(n + "_bn/beta")
                cp[i].avg_mean = self.persist[n + "_bn/avg_mean"].data_ptr()
                cp[i].avg_var = self.persist[n + "_bn/avg_var"].data_ptr()
                cg[i].dgamma, cg[i].dbeta = a.g(n + "_bn/gamma"), a.g(n + "_bn/beta")
            else:                                            # Convolution2D with bias, no BatchNormalization (seq2seq.py:52-57)
                cp[i].bias, cg[i].dbias = a.p(n + "/b"), a.g(n + "/b")
        nl, nd, h, H = len(self.rnn_enc), self.n_dirs, self.h, self.H
        ld = LstmStackDesc(T2, B, feat, h, nl, nd)
        # hints that spare the GEMMs absolute-maximum passes (include/astk.h): the layer outputs are bounded by the dropout scale; the
        # frames' maximum is taken by the CNN kernel that writes them (set per call in encode(): it lives in the CNN workspace)
        ratio = float(self.cfg["dropout"]["rnn"])
        ld.out_bound = 1.0 / (1.0 - ratio) if 0 <= ratio < 1 else 0.0
        lp = (LstmParams * (nl * nd))()
        lg = (LstmGrads * (nl * nd))()
        for d_, names in enumerate([self.rnn_enc, self.rnn_rev_enc][:nd]):
            for l, n in enumerate(names):
                k = d_ * nl + l
                lp[k].Wu, lp[k].b, lp[k].Wl = a.p(n + "/upward/W"), a.p(n + "/upward/b"), a.p(n + "/lateral/W")
                lg[k].dWu, lg[k].db, lg[k].dWl = a.g(n + "/upward/W"), a.g(n + "/upward/b"), a.g(n + "/lateral/W")
        nld = len(self.rnn_dec)
        dd = self._decoder_desc(B, max(L, 2), T2)
        dp, dg = self._decoder_tables()
        S = max(L, 2) - 1
        f32 = dict(dtype=torch.float32, device=dev)
        # pooled first (growing a pool clears the shape cache), then the per-batch-size state, then the views of this shape
        big = dict(xlstm=self._pool("xlstm", (T2, B, feat)), d_xlstm=self._pool("d_xlstm", (T2, B, feat)),
                   enc_states=self._pool("enc_states", (B, T2, H)), d_enc=self._pool("d_enc", (B, T2, H)),
                   pred=self._pool("pred", (S, B), torch.int32), flags=self._pool("flags", (S,), torch.int32))
        bs = self._bstate.get(B)
        if bs is None:
            # zero-initialised and only partly written (encoder layers without a decoder counterpart keep their zero gradient)
            bs = dict(cT=torch.zeros(nd, nl, B, h, **f32), hT=torch.zeros(nd, nl, B, h, **f32),
                      d_cT=torch.zeros(nd, nl, B, h, **f32), d_hT=torch.zeros(nd, nl, B, h, **f32),
                      c0=torch.zeros(nld, B, H, **f32), h0=torch.zeros(nld, B, H, **f32),
                      d_c0=torch.zeros(nld, B, H, **f32), d_h0=torch.zeros(nld, B, H, **f32))
            # [loss, status word] is the pair every reader knows; behind it, in the same 16 bytes, the CTC branch's count of rows
            # without a path (an int32), so that ONE copy reads all three (LossData)
            bs["loss4"] = torch.zeros(4, **f32)
            bs["loss"] = bs["loss4"][:2]
            self._bstate[B] = bs
        st = dict(key=key, B=B, T=T, D=D, L=L, T2=T2, feat=feat, S=S, cd=cd, cp=cp, cg=cg, ld=ld, lp=lp, lg=lg, dd=dd, dp=dp, dg=dg,
                  ws_cnn=int(lib.astk_conv_bn_relu_workspace_bytes(C.byref(cd))),
                  ws_lstm=int(lib.astk_lstm_stack_workspace_bytes(C.byref(ld))),
                  ws_dec=int(lib.astk_decoder_workspace_bytes(C.byref(dd))))
        st.update(big)
        st.update(bs)
        # the persistent kernels' status word rides in loss[1]: written by the decoder forward (the kernel that writes the loss) and once
        # more by the CNN backward's last kernel -- include/astk.h status_dst, a launch less each than astk_persist_status_snapshot
        dd.status_dst = cd.status_dst = bs["loss"].data_ptr() + 4
        assert st["ws_cnn"] and st["ws_lstm"] and st["ws_dec"], lib.astk_last_error().decode()
        self._shape_cache[key] = st
        return st

    def _decoder_desc(self, B, L, T2):
        return DecoderDesc(B, L, T2, self.H, self.E, self.A, self.V, len(self.rnn_dec), self.n_attn, 0 if self.feed_attn else 1,
                           1 if self.rnn_ln else 0)

    def _decoder_tables(self):
        """The decoder's parameter and gradient tables (pointers into the arena)."""
        a = self.arena
        dp, dg = DecoderParams(), DecoderGrads()
        dp.embed, dg.d_embed = a.p("embed_dec/W"), a.g("embed_dec/W")
        for l, n in enumerate(self.rnn_dec):
            dp.lstm[l].Wu, dp.lstm[l].b, dp.lstm[l].Wl = a.p(n + "/upward/W"), a.p(n + "/upward/b"), a.p(n + "/lateral/W")
            dg.lstm[l].dWu, dg.lstm[l].db, dg.lstm[l].dWl = a.g(n + "/upward/W"), a.g(n + "/upward/b"), a.g(n + "/lateral/W")
            if self.rnn_ln:
                dp.ln_gamma[l], dp.ln_beta[l] = a.p(n + "_ln/gamma"), a.p(n + "_ln/beta")
                dg.d_ln_gamma[l], dg.d_ln_beta[l] = a.g(n + "_ln/gamma"), a.g(n + "_ln/beta")
        for k in range(1, self.n_attn):
            dp.Wa_x[k - 1], dp.ba_x[k - 1] = a.p(f"attn_Wa{k}/W"), a.p(f"attn_Wa{k}/b")
            dg.dWa_x[k - 1], dg.dba_x[k - 1] = a.g(f"attn_Wa{k}/W"), a.g(f"attn_Wa{k}/b")
        dp.Wa, dp.ba, dp.Wc, dp.bc = a.p("attn_Wa/W"), a.p("attn_Wa/b"), a.p("context/W"), a.p("context/b")
        dp.Wo, dp.bo, dp.class_weight = a.p("out/W"), a.p("out/b"), self.mask_pad_id.data_ptr()
        dg.dWa, dg.dba, dg.dWc, dg.dbc = a.g("attn_Wa/W"), a.g("attn_Wa/b"), a.g("context/W"), a.g("context/b")
        dg.dWo, dg.dbo = a.g("out/W"), a.g("out/b")
        return dp, dg

    def _rng(self, n):
        off = self._rng_offset
        self._rng_offset += n
        return off

    def _masks(self, name, shape, ratio):
        """Scaled keep-masks: injected (parity tests) or drawn on device; None when dropout is inactive."""
        if name in self.inject:
            m = self.inject[name]
            return None if m is None else m.to(self.device, torch.float32).contiguous()
        if not config.train or ratio <= 0:
            return None
        pre = self._predrawn.pop(name, None)
        if pre is not None and tuple(pre.shape) == tuple(shape):
            return pre
        t = self._pool("mask_" + name, shape)
        lib = _lib.load()
        check(lib.astk_fill_dropout_mask(_vp(t), t.numel(), float(ratio), self.rng_seed, self._rng(t.numel()), self._stream()))
        return t

    def _predraw(self, X_shape, add_noise, st, L, with_decoder):
        """All random tensors of a train step -- the speech noise and the four kinds of dropout masks -- in ONE launch (astk_fill_random)
        instead of up to five; the (seed, offset) counters are consumed in the order the separate draws used, so every value is the one
        they would have produced.  Injected tensors (parity tests) are left alone, as before."""
        self._predrawn = {}
        if not config.train and not (with_decoder and self._pending_flags is not None):
            return
        dr = self.cfg["dropout"]
        B, S = X_shape[0], L - 1
        want = []
        if config.train and add_noise > 0 and "noise" not in self.inject:
            want.append(("noise", tuple(X_shape), _lib.RAND_NORMAL, 1.0, float(add_noise), self.rng_seed ^ 0xABCDEF))
        masks = [("enc_masks", (self.n_dirs, len(self.rnn_enc), st["T2"], B, self.h), dr["rnn"])]
        if with_decoder:
            masks += [("emb_mask", (S, B, self.E), dr["embed"]), ("rnn_masks", (len(self.rnn_dec), S, B, self.H), dr["rnn"]),
                      ("out_mask", (S, B, self.V), dr.get("out", 0))]
        for name, shape, ratio in masks:
            if config.train and name not in self.inject and ratio and ratio > 0:
                want.append((name, shape, _lib.RAND_DROPOUT, float(ratio), 0.0, self.rng_seed))
        flags = self._pending_flags if with_decoder else None
        if len(want) > _lib.RAND_SEG_MAX or (len(want) < 2 and flags is None):
            return                                    # (a single draw keeps its own launch)
        segs = (_lib.RandSeg * max(1, len(want)))()
        for i, (name, shape, kind, a, b, seed) in enumerate(want):
            t = self._pool("noise" if name == "noise" else "mask_" + name, shape)
            segs[i].out, segs[i].n, segs[i].kind, segs[i].a, segs[i].b = t.data_ptr(), t.numel(), kind, a, b
            segs[i].seed, segs[i].offset = seed & 0xFFFFFFFFFFFFFFFF, self._rng(t.numel())
            self._predrawn[name] = t
        if flags is None:
            check(_lib.load().astk_fill_random(segs, len(want), self._stream()))
        else:
            words = (C.c_int32 * len(flags))(*flags)
            check(_lib.load().astk_fill_random_ex(segs, len(want), words, len(flags), _vp(st["flags"]), self._stream()))
            self._pending_flags = None

    # ------------------------------------------------------------------ encoder (seq2seq.py:293-314)
    def _as_input(self, X):
        if isinstance(X, np.ndarray):
            X = torch.from_numpy(X)
        if hasattr(X, "data") and not isinstance(X, torch.Tensor):
            X = X.data
        return X.to(self.device, torch.float32).contiguous()

    def encode(self, X, add_noise=0):
        lib = self._require_gpu()
        X = self._as_input(X)
        B, T, D = X.shape
        in_forward_loss = bool(self._cur and self._cur.get("pending_L"))
        L = self._cur["L"] if in_forward_loss else 2
        st = self._shape_state(B, T, D, L)
        self._cur = st
        st["X"] = X
        noise = None
        self._predraw(tuple(X.shape), add_noise, st, L, in_forward_loss)
        if add_noise > 0 and config.train:
            if "noise" in self.inject:
                noise = self.inject["noise"].to(self.device, torch.float32).contiguous()
            elif "noise" in self._predrawn:
                noise = self._predrawn.pop("noise")
            else:
                noise = self._pool("noise", tuple(X.shape))
                check(lib.astk_fill_normal(_vp(noise), noise.numel(), 1.0, float(add_noise), self.rng_seed ^ 0xABCDEF,
                                           self._rng(noise.numel()), self._stream()))
        st["noise"] = noise
        nl, nd = len(self.rnn_enc), self.n_dirs
        st["enc_masks"] = self._masks("enc_masks", (nd, nl, st["T2"], B, self.h), self.cfg["dropout"]["rnn"])
        st["train_mode"] = bool(config.train)
        s = self._stream()
        wc = self._workspace("cnn", st["ws_cnn"])
        sx = self.stat_exchange if config.train else None
        if sx is None:
            check(lib.astk_conv_bn_relu_fwd(C.byref(st["cd"]), st["cp"], _vp(X), _vp(noise), _vp(st["xlstm"]), _vp(wc), wc.numel(),
                                            1 if config.train else 0, s))
        else:
            rc = lib.astk_conv_bn_relu_fwd_sync(C.byref(st["cd"]), st["cp"], _vp(X), _vp(noise), _vp(st["xlstm"]), _vp(wc), wc.numel(), 1,
                                                C.cast(sx.bind(wc).callback, C.c_void_p), None, sx.world, s)
            if sx.error is not None:
                raise sx.error
            check(rc)
        st["bn_world"] = 1 if sx is None else sx.world
        if config.train:
            self.bn_N += 1
        st["ld"].x_amax = lib.astk_conv_out_amax(C.byref(st["cd"]), _vp(wc), wc.numel())      # (None for bad arguments: the GEMM measures x itself)
        if self.enc_variant is not None:                     # rnn_config.ln / linear_proj: layer-by-layer (ast_amd/enc_variants.py)
            if self.rnn_linear_proj:
                self.enc_variant.forward(st, bool(config.train))
            else:
                self.enc_variant.forward(st)
        else:
            wl = self._workspace("lstm", st["ws_lstm"])
            # work beside the recurrences: the library cuts the layer-0 products into time chunks on this stream (astk.h side_stream), and
            # sizes its recurrence workgroups (16 / 32 batch rows) by whether it has one -- the backward call sees the same descriptor
            side = self._side_stream()
            st["ld"].side_stream = side.cuda_stream if side is not None else None
            check(lib.astk_lstm_stack_fwd(C.byref(st["ld"]), st["lp"], _vp(st["xlstm"]), _vp(st["enc_masks"]), _vp(st["enc_states"]),
                                          _vp(st["cT"]), _vp(st["hT"]), _vp(wl), wl.numel(), s))
        self.enc_states = st["enc_states"]
        self.loss = 0

    def _bridge_states(self, st, dec_c, dec_h, enc_c, enc_h, to_decoder):
        """[fwd_k ; rev_k] of the encoder <-> decoder layer k, for both tensors and every bridged layer in ONE launch (the twelve strided
        torch copies of a 3-layer model were 58 us of a 7.2 ms step)."""
        n = min(len(self.rnn_enc), len(self.rnn_dec))
        if self.h % 4:                      # (the kernel moves 16-byte pieces)
            for k in range(n):
                for d_, e_ in ((dec_c, enc_c), (dec_h, enc_h)):
                    if to_decoder:
                        d_[k].view(-1, self.n_dirs, self.h).copy_(e_[:, k].permute(1, 0, 2))
                    else:
                        e_[:, k].copy_(d_[k].view(-1, self.n_dirs, self.h).permute(1, 0, 2))
            return
        check(_lib.load().astk_bridge_states(_vp(dec_c), _vp(dec_h), _vp(enc_c), _vp(enc_h), self.n_dirs, len(self.rnn_enc), n, st["B"], self.h,
                                             1 if to_decoder else 0, self._stream()))

    # ------------------------------------------------------------------ seq2seq.py:318-333
    def init_decoder_state(self):
        st = self._cur
        h, nd = self.h, self.n_dirs
        # decoder layer k starts from [fwd_k ; rev_k] of the encoder; layers without an encoder counterpart keep the zeros they
        # were allocated with (c0/h0 are only ever written here).  One strided copy per tensor and layer.
        self._bridge_states(st, st["c0"], st["h0"], st["cT"], st["hT"], True)
        if config.train:
            self._dec_c, self._dec_h = st["c0"], st["h0"]      # the step API (decode_step) clones before it advances them
        else:
            self._dec_c, self._dec_h = st["c0"].clone(), st["h0"].clone()

    # ------------------------------------------------------------------ seq2seq.py:399-473
    def _side_stream(self):
        """The model's second stream (ordinary, from torch's pool) for the stream the step is running on, or None: side-stream work off, the
        step on the legacy default stream (which synchronises implicitly with every other stream), or no stream found that really runs
        CONCURRENTLY with it.  HIP multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default) and two streams that
        share one execute in order whatever their events say -- the flag-gated hand-offs between the recurrence kernels and the chunked
        products beside them need true concurrency (in one queue the consumer would sit in front of its producer until its bounded spin
        times out), so every candidate is probed once (a 3 ms spin on one stream, a trivial kernel on the other)."""
        if not self.side_stream_on or self.enc_variant is not None:
            return None
        # (the process default counts like the model's own wish: deterministic split tiles share ONE fix-up workspace, astk.h side_wgs)
        if self.deterministic or _lib.get_tuning("gemm.deterministic") != 0:
            self._side = None
            return None
        main = torch.cuda.current_stream(self.device)
        if main.cuda_stream == 0:
            return None
        if main.cuda_stream not in self._side_by_main:
            chosen = None
            for _ in range(6):
                cand = torch.cuda.Stream(device=self.device)
                if self._concurrent(main, cand) and self._concurrent(cand, main):
                    chosen = cand
                    break
            self._side_by_main[main.cuda_stream] = chosen
        self._side = self._side_by_main[main.cuda_stream]
        return self._side

    def _concurrent(self, a, b):
        """True if a kernel on stream b runs while stream a is busy (one 3 ms spin on a, a trivial kernel on b)."""
        lib = _lib.load()
        probe = self._ws.get("probe")
        if probe is None:
            probe = self._ws["probe"] = torch.zeros(4, device=self.device)
            check(lib.astk_spin(10, None, C.c_void_p(a.cuda_stream)))              # (first launches load the code objects: not inside the probe)
            check(lib.astk_scale_f32(_vp(probe), 4, 1.0, C.c_void_p(a.cuda_stream)))
        torch.cuda.synchronize(self.device)
        check(lib.astk_spin(3000, None, C.c_void_p(a.cuda_stream)))
        ea, eb = torch.cuda.Event(), torch.cuda.Event()
        ea.record(a)
        check(lib.astk_scale_f32(_vp(probe), 4, 1.0, C.c_void_p(b.cuda_stream)))
        eb.record(b)
        eb.synchronize()
        overlapped = not ea.query()
        ea.synchronize()
        return overlapped

    def close(self):
        """Kept for callers of rounds 2-5 (the CU-masked streams it used to destroy are gone; torch owns the side streams)."""
        self._side = None
        self._side_by_main = {}

    def _upload_flags(self, dst, flags, ring="flag_ring"):
        """Host -> device copy of the teacher-forcing flags WITHOUT a host sync: a copy from pageable memory would make the host wait
        for the encoder of this step, and the GPU then idles while the host catches up at the start of the next one.  The flags
        go through a small ring of pinned buffers; a slot is reused only after the copy that read it has executed."""
        ring_key, ring = ring, self._ws.get(ring)           # (the CTC branch's row lengths travel the same way, through a ring of their own)
        if ring is None or ring["bufs"][0][0].numel() < len(flags):
            ring = {"i": 0, "bufs": [(torch.empty(max(64, len(flags)), dtype=torch.int32).pin_memory(), torch.cuda.Event()) for _ in range(8)]}
            self._ws[ring_key] = ring
        buf, ev = ring["bufs"][ring["i"]]
        ring["i"] = (ring["i"] + 1) % len(ring["bufs"])
        ev.synchronize()                       # returns at once unless the host is 8 steps ahead
        buf[:len(flags)] = torch.tensor(flags, dtype=torch.int32)
        # (round 5: a side stream for this copy, beside the encoder, was measured -- it trades the 4.5 us copy for a 6 us cross-queue wait on
        #  the compute stream: nothing, and one more stream per model next to RCCL's; the copy stays in stream order)
        dst.copy_(buf[:len(flags)], non_blocking=True)
        ev.record(torch.cuda.current_stream(self.device))

    def forward_loss(self, X, y, teach_ratio, random_out=0, add_noise=0, row_weight=None, y_global=None, label_smoothing=0.0, ctc_weight=0.0,
                     x_lens=None):
        """seq2seq.py:399-473.  ctc_weight (extension): weight of the auxiliary CTC loss of the `ctc_out` head on the
        encoder states, loss = loss_attention + ctc_weight * mean_b nll_b; needs rnn_config.ctc; 0 = the reference's loss, and nothing
        of the branch is launched.  The labels of a row are its targets from UNK_ID on (PAD, GO and EOS dropped), the blank is PAD_ID.
        x_lens: host array of the rows' true frame counts in front of the CNN (None: every row has all T frames); read with
        ctc_weight > 0 only.  The attention term, `pred` and every decoder gradient do not depend on either.  label_smoothing (extension): eps of the training loss, uniform over all classes and
        weighted by the target's class weight; 0 = the reference's loss.  Predictions and fed-back tokens do not depend on it.  y_global (data parallelism with random_out > 0 only): the targets of the WHOLE unsharded batch as a host
        array, global row b * world + r = row b of rank r -- the loader has them before it shards (`batch["y_global"]`); without it the
        ranks' targets are all-gathered, a host-blocking collective in front of every step.  row_weight (extension):
        None, or one finite float per batch row -- a (B,) float32 device tensor, or a host array that is uploaded -- that multiplies the
        row's loss and gradient at every step (astk_decoder_fwd_w); any sign, 0 switches a row off exactly.  Predictions and fed-back
        tokens do not depend on it.  Not with ctc_weight > 0: the CTC term has no row weights.  (It stands in front of the extension keywords, whose
        order their own tests pin; pass it by name.)"""
        label_smoothing = checked_label_smoothing(label_smoothing)
        ctc_weight = checked_ctc_weight(ctc_weight, self.ctc_head)
        if row_weight is not None and ctc_weight > 0:
            raise ValueError("forward_loss: row_weight with ctc_weight > 0 (the CTC term has no row weights)")
        lib = self._require_gpu()
        X = self._as_input(X)
        if ctc_weight > 0:
            if x_lens is not None:
                x_lens = checked_x_lens(x_lens, X.shape[0], X.shape[1])
        if isinstance(y, np.ndarray):
            y = torch.from_numpy(y)
        if hasattr(y, "data") and not isinstance(y, torch.Tensor):
            y = y.data
        y_host = y if (random_out and y.device.type == "cpu") else None
        y = y.to(self.device, torch.int32).contiguous()
        B, L = y.shape
        assert L >= 2, "targets need at least GO and EOS"
        if ctc_weight > 0 and L > _lib.CTC_MAX_LABELS:
            raise ValueError(f"ctc_weight > 0: targets of padded length {L} exceed ASTK_CTC_MAX_LABELS = {_lib.CTC_MAX_LABELS}")
        S = L - 1
        if row_weight is not None:
            if not isinstance(row_weight, torch.Tensor):
                row_weight = torch.from_numpy(np.ascontiguousarray(row_weight, dtype=np.float32))
            row_weight = row_weight.to(self.device, torch.float32).contiguous()
            if tuple(row_weight.shape) != (B,):
                raise ValueError(f"forward_loss: row_weight of shape {tuple(row_weight.shape)}, one weight per batch row ({B},) is needed")
        # quirk Q4: one Python-`random` coin per step for 0 < i < L-2, truth otherwise (seq2seq.py:431-436).  With random_out > 0
        # (seq2seq.py:456-465) the SAME stream also decides, behind each step's coin, which targets >= 4 are replaced (draw ABOVE
        # random_out) by a class id from xp.random.randint(4, dec_vocab_size + 1).  That range is inclusive of dec_vocab_size, one past the
        # last class (quirk Q8): Chainer's softmax_cross_entropy raises on it with NumPy and reads out of bounds with CuPy.  DEVIATION: the
        # drawn id is clamped to dec_vocab_size - 1.  Nothing in a decoder step consumes either stream, so all draws are made here, in
        # the reference's order, and the scored targets go to the device as a second (B, L) matrix.
        targets = None
        if "use_truth" in self.inject:
            flags = [int(bool(v)) for v in self.inject["use_truth"]]
            assert not random_out, "inject['use_truth'] bypasses the random stream random_out shares"
        elif random_out:
            yh = (y_host if y_host is not None else y.cpu()).numpy()
            randint = self.inject.get("randint", np.random.randint)      # the reference's draw is the unseeded global xp RNG (quirk Q7)
            gather = None
            if y_global is not None:
                from . import dist as adist
                yg, w_ = np.asarray(y_global), adist.world_size()
                if w_ > 1 and yg.shape == (yh.shape[0] * w_, yh.shape[1]):
                    gather = lambda a: [yg[r::w_] for r in range(w_)]          # noqa: E731  (no collective: every rank holds the same global rows)
            flags, tg = draw_flags_and_targets(yh, teach_ratio, random_out, self.V, randint, gather=gather)
            targets = torch.from_numpy(np.ascontiguousarray(tg, dtype=np.int32)).to(self.device)
        else:
            flags = [int(random.random() < teach_ratio) if 0 < i < L - 2 else 1 for i in range(S)]
        self.use_truth = flags
        # (the flags go to the device with the step's random tensors, in the kernel arguments of that one launch: _predraw)
        self._pending_flags = flags if len(flags) <= _lib.RAND_WORDS_MAX else None
        self._cur = {"L": L, "pending_L": True}
        self.encode(X, add_noise=add_noise)
        st = self._cur
        self.init_decoder_state()
        if self._pending_flags is not None or len(flags) > _lib.RAND_WORDS_MAX:      # (not taken by _predraw: a copy of their own)
            self._pending_flags = None
            self._upload_flags(st["flags"], flags)
        st["flags_host"] = (C.c_int32 * S)(*flags)          # the per-launch loop scores the teacher-forced steps behind the loop (astk.h)
        st["dd"].use_truth_host = C.cast(st["flags_host"], C.POINTER(C.c_int32))
        st["dd"].label_smoothing = label_smoothing          # read by the forward call only (include/astk.h)
        st["y"] = y
        st["targets"] = targets
        st["row_weight"] = row_weight
        dr = self.cfg["dropout"]
        st["emb_mask"] = self._masks("emb_mask", (S, B, self.E), dr["embed"])
        st["rnn_masks"] = self._masks("rnn_masks", (len(self.rnn_dec), S, B, self.H), dr["rnn"])
        st["out_mask"] = self._masks("out_mask", (S, B, self.V), dr.get("out", 0))       # dropout on the logits (seq2seq.py:394)
        wd = self._workspace("dec", st["ws_dec"])
        check(lib.astk_decoder_fwd_w(C.byref(st["dd"]), C.byref(st["dp"]), _vp(st["enc_states"]), _vp(st["c0"]), _vp(st["h0"]),
                                     _vp(y), _vp(st["flags"]), _vp(st["emb_mask"]), _vp(st["rnn_masks"]), _vp(st["out_mask"]), _vp(targets),
                                     _vp(row_weight), _vp(st["loss"]), _vp(st["pred"]), _vp(wd), wd.numel(), self._stream()))
        # (loss[1] = the persistent kernels' status word: written by the op itself, astk_decoder_desc.status_dst)
        st["ctc"] = self._ctc_forward(st, y, ctc_weight, x_lens) if ctc_weight > 0 else None
        st["pending_backward"] = True
        self.loss = Loss(self, st["loss"], st["loss4"] if st["ctc"] is not None else None)
        return self.loss

    # ------------------------------------------------------------------ auxiliary CTC loss on the encoder states
    def _t2_lens(self, st, x_lens):
        """Device (B,) int32 of the rows' frames behind the CNN (the host maps the true lengths through cnn_out_lens), or None."""
        if x_lens is None:
            return None
        cc = self.cfg["cnn_config"]["cnn_layers"]
        t2 = [min(cnn_out_lens(cc, int(n))[-1], st["T2"]) for n in x_lens]
        dst = self._pool("ctc_lens", (len(t2),), torch.int32)
        self._upload_flags(dst, t2, ring="ctc_len_ring")
        return dst

    def _ctc_logits(self, st, s):
        """logits (B T'', Vp) = enc_states W^T + b of the head, one product under the model's arithmetic, into a pooled buffer."""
        lib = _lib.load()
        rows, V, a = st["B"] * st["T2"], self.V, self.arena
        Vp = (V + 3) // 4 * 4
        logits = self._pool("ctc_logits", (rows, Vp))
        check(lib.astk_ctc_head_fwd(rows, V, self.H, _vp(st["enc_states"]), a.p("ctc_out/W"), a.p("ctc_out/b"), _vp(logits), Vp,
                                    _lib.PREC_BY_NAME[self.gemm_precision], s))
        return logits, Vp

    def _ctc_forward(self, st, y, weight, x_lens):
        """Behind the decoder forward, on its stream: the head's logits, then astk_ctc_loss, which adds weight / B * sum_b nll_b to the
        loss word the decoder wrote and leaves weight / B * d(sum nll) / d logits in place of the logits for _backward."""
        lib = _lib.load()
        s = self._stream()
        B, T2, L = st["B"], st["T2"], int(y.shape[1])
        lens = self._t2_lens(st, x_lens)
        logits, Vp = self._ctc_logits(st, s)
        cdesc = _lib.CtcDesc(B, T2, self.V, Vp, L, L, UNK_ID, PAD_ID)
        nbytes = int(lib.astk_ctc_workspace_bytes(C.byref(cdesc)))
        if not nbytes:
            raise _lib.AstkError(lib.astk_last_error().decode())
        ws = self._workspace("ctc", nbytes)
        self.ctc_nll = self._pool("ctc_nll", (B,))
        quad = st["loss4"]
        quad[3:4].copy_(quad[0:1])                          # the attention term alone, for the log (nn.py: the epoch's mean CTC term)
        check(lib.astk_ctc_loss(C.byref(cdesc), _vp(logits), _vp(y), _vp(lens), weight / B, _vp(self.ctc_nll), _vp(quad),
                                _vp(logits), C.c_void_p(quad.data_ptr() + 8), _vp(ws), ws.numel(), s))
        return dict(dlogits=logits, Vp=Vp)

    def _ctc_backward(self, st, s):
        """Between the decoder's chain phase (which wrote d_enc and performed the deferred zero fill of the gradient arena) and the
        encoder's backward: d_enc += dlogits W, ctc_out/W.grad += dlogits^T enc, ctc_out/b.grad += column sums; main stream."""
        c, a = st["ctc"], self.arena
        check(_lib.load().astk_ctc_head_bwd(st["B"] * st["T2"], self.V, self.H, _vp(c["dlogits"]), c["Vp"], a.p("ctc_out/W"),
                                            _vp(st["enc_states"]), _vp(st["d_enc"]), a.g("ctc_out/W"), a.g("ctc_out/b"),
                                            _lib.PREC_BY_NAME[self.gemm_precision], 1 if self.deterministic else 0, s))

    def _ctc_eval_logits(self, who, X, x_lens, refuse=None):
        """What the CTC head's eval-mode methods open with: the head check (`who` names the method in its message; refuse(), if
        given, then raises for the method's own arguments, before the library or the device is touched), the inputs on the device,
        the eval-mode encode, the rows' frames behind the CNN and the head's logits.  Returns the library, X and x_lens as checked,
        the shape state, the stream, the device lengths (or None), the logits and their leading dimension Vp."""
        if not self.ctc_head:
            raise ValueError(f"{who} needs the CTC head: set rnn_config.ctc = true in model_cfg.json")
        if refuse is not None:
            refuse()
        lib = self._require_gpu()
        X = self._as_input(X)
        if x_lens is not None:
            x_lens = checked_x_lens(x_lens, X.shape[0], X.shape[1])
        with using_config("train", False):
            self._cur = None
            self.encode(X)
        st, s = self._cur, self._stream()
        lens = self._t2_lens(st, x_lens)
        logits, Vp = self._ctc_logits(st, s)
        return lib, X, x_lens, st, s, lens, logits, Vp

    def _int32_parts(self, name, sizes):
        """One pooled int32 buffer of sum(sizes) 4-byte words for everything a call sends back to the host (a float64 part goes first:
        8-byte aligned).  Returns the pointer of every part and read(): ONE device-to-host copy, the parts as numpy int32 views."""
        cuts = np.cumsum([0] + list(sizes))
        out = self._pool(name, (int(cuts[-1]),), torch.int32)
        ptrs = [C.c_void_p(out.data_ptr() + 4 * int(c)) for c in cuts[:-1]]

        def read():
            host = out.cpu().numpy()
            return [host[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        return ptrs, read

    def ctc_predict(self, X, x_lens=None):
        """Greedy decode of the CTC head (eval mode): encode the batch, the head's logits, the per-frame argmax over each row's valid
        frames (astk_ctc_greedy), then on the host repeats collapsed and blanks dropped.  Returns a list of token lists."""
        lib, X, x_lens, st, s, lens, logits, Vp = self._ctc_eval_logits("ctc_predict", X, x_lens)
        B, T2 = st["B"], st["T2"]
        cdesc = _lib.CtcDesc(B, T2, self.V, Vp, 1, 1, UNK_ID, PAD_ID)
        best = self._pool("ctc_best", (B, T2), torch.int32)
        check(lib.astk_ctc_greedy(C.byref(cdesc), _vp(logits), _vp(lens), _vp(best), s))
        out = []
        for row in best.cpu().numpy():
            prev = np.concatenate(([-1], row[:-1]))
            out.append([int(c) for c in row[(row != prev) & (row != PAD_ID)]])
        return out

    def ctc_beam(self, X, x_lens=None, N=5, C=5, max_labels=None):
        """CTC prefix beam search of the head alone (eval mode): encode the batch, the head's logits, the N most
        probable label strings of every row over its valid frames with C labels proposed per frame (astk_ctc_beam); ONE device-to-host
        copy.  Returns per row a list in rank order of {"hyp": [GO] + labels + [EOS], "score", "labels"}; score = the pruned float64
        sum over the string's alignments, a lower bound of log p_ctc(labels).  max_labels (default min(T'', 255)) caps the strings."""
        import ctypes                                        # (the parameter C shadows the module's alias)

        def refuse():
            nonlocal N, C
            N, C = checked_ctc_beam_width(N, C, self.V)
            if max_labels is not None and not 1 <= int(max_labels) <= _lib.CTC_MAX_LABELS:
                raise ValueError(f"ctc_beam: max_labels must lie in 1..{_lib.CTC_MAX_LABELS}, got {max_labels!r}")
        lib, X, x_lens, st, s, lens, logits, Vp = self._ctc_eval_logits("ctc_beam", X, x_lens, refuse)
        B, T2 = st["B"], st["T2"]
        if T2 > _lib.CTC_BEAM_MAX_T:
            raise ValueError(f"ctc_beam: {T2} encoder frames exceed the {_lib.CTC_BEAM_MAX_T} a row is limited to")
        Lm = min(T2, _lib.CTC_MAX_LABELS) if max_labels is None else int(max_labels)
        bdesc = _lib.CtcBeamDesc(B, T2, self.V, Vp, N, C, Lm, UNK_ID, PAD_ID)
        nbytes = int(lib.astk_ctc_beam_workspace_bytes(ctypes.byref(bdesc)))
        if not nbytes:
            raise _lib.AstkError(lib.astk_last_error().decode())
        ws = self._workspace("ctc", nbytes)
        # everything that goes back to the host, in one buffer of 4-byte words: score (B, N) float64 first (8-byte aligned), then
        # n_labels (B, N) and tokens (B, N, Lm)
        p, read = self._int32_parts("ctc_beam_out", [2 * B * N, B * N, B * N * Lm])
        check(lib.astk_ctc_beam(ctypes.byref(bdesc), _vp(logits), _vp(lens), p[2], p[1], p[0], _vp(ws), ws.numel(), s))
        part = read()
        score, n_lab, tok = part[0].view(np.float64).reshape(B, N), part[1].reshape(B, N), part[2].reshape(B, N, Lm)
        rows = []
        for b in range(B):
            row = []
            for r in range(N):
                if n_lab[b, r] < 0:
                    continue
                labels = [int(c) for c in tok[b, r, :n_lab[b, r]]]
                row.append({"hyp": [GO_ID] + labels + [EOS_ID], "score": float(score[b, r]), "labels": labels})
            rows.append(row)
        return rows

    def ctc_align(self, X, y, x_lens=None):
        """Forced alignment of the targets y (B, L) through the CTC head (eval mode): encode the batch, the head's
        logits, the best monotonic path of every row's labels (ids >= UNK_ID of y[b], in order) over its valid frames
        (astk_ctc_align), then astk_ctc_loss on the same logits for the full-sum score; ONE device-to-host copy brings everything back.
        Returns one dict per row:
          labels (U,), frame_state / frame_class (T'',) as astk.h defines them (-1 / the blank behind the row's n_frames),
          segments (U, 2): the encoder frames [start, end) of every label,
          segments_input (U, 2): the same in input frames (input_span), clipped to [0, x_len],
          label_logp (U,), confidence (U,) = exp(label_logp / frames in the label), score = the best path's log-probability,
          total_logp = log p_ctc(labels), the sum over all paths (score <= total_logp; the difference says how peaked the alignment is).
        A row without a path (fewer frames than labels + adjacent repeats): score = total_logp = -inf, segments all -1."""
        def refuse():                                        # (the shapes alone, on the host: y moves to the device behind the checks)
            nonlocal y
            if isinstance(y, np.ndarray):
                y = torch.from_numpy(y)
            if y.dim() != 2 or y.shape[0] != X.shape[0]:
                raise ValueError(f"ctc_align: y must be (B = {X.shape[0]}, L), got {tuple(y.shape)}")
            if y.shape[1] < 1:
                raise ValueError("ctc_align: y holds no column")
            if y.shape[1] > _lib.CTC_MAX_LABELS:
                raise ValueError(f"ctc_align: targets of padded length {int(y.shape[1])} exceed ASTK_CTC_MAX_LABELS = {_lib.CTC_MAX_LABELS}")
        lib, X, x_lens, st, s, lens, logits, Vp = self._ctc_eval_logits("ctc_align", X, x_lens, refuse)
        y = y.to(self.device, torch.int32).contiguous()
        L = int(y.shape[1])
        B, T2 = st["B"], st["T2"]
        cdesc = _lib.CtcDesc(B, T2, self.V, Vp, L, L, UNK_ID, PAD_ID)
        need_a, need_l = int(lib.astk_ctc_align_workspace_bytes(C.byref(cdesc))), int(lib.astk_ctc_workspace_bytes(C.byref(cdesc)))
        if not need_a or not need_l:
            raise _lib.AstkError(lib.astk_last_error().decode())
        ws = self._workspace("ctc", max(need_a, need_l))
        # everything that goes back to the host, in one buffer of 4-byte words: frame_state, frame_class (B, T''); label_start,
        # label_end, label_logp (B, L); row_score, row_nll (B)
        p, read = self._int32_parts("ctc_align_out", [B * T2, B * T2, B * L, B * L, B * L, B, B])
        check(lib.astk_ctc_align(C.byref(cdesc), _vp(logits), _vp(y), _vp(lens), p[0], p[1], p[2], p[3], p[4], p[5], None, _vp(ws),
                                 ws.numel(), s))
        # the full-sum score behind the alignment: astk_ctc_loss as it is, which leaves its gradient in place of the logits
        check(lib.astk_ctc_loss(C.byref(cdesc), _vp(logits), _vp(y), _vp(lens), 1.0, p[6], None, _vp(logits), None, _vp(ws), ws.numel(), s))
        part = read()
        fs, fc = part[0].reshape(B, T2), part[1].reshape(B, T2)
        l0, l1, lp = part[2].reshape(B, L), part[3].reshape(B, L), part[4].view(np.float32).reshape(B, L)
        score, nll = part[5].view(np.float32), part[6].view(np.float32)
        cc = self.cfg["cnn_config"]["cnn_layers"]
        y_np = y.cpu().numpy()
        rows = []
        for b in range(B):
            labels = np.minimum(y_np[b][y_np[b] >= UNK_ID], self.V - 1).astype(np.int32)
            U = len(labels)
            x_len = int(X.shape[1] if x_lens is None else x_lens[b])
            seg = np.stack([l0[b, :U], l1[b, :U]], axis=1).astype(np.int32)
            ok = bool(np.isfinite(score[b]))
            seg_in = np.asarray([input_span(cc, a, e, x_len) for a, e in seg], np.int32).reshape(U, 2) if ok else np.full((U, 2), -1, np.int32)
            with np.errstate(divide="ignore", invalid="ignore"):
                conf = np.exp(lp[b, :U].astype(np.float64) / np.maximum(seg[:, 1] - seg[:, 0], 1)) if ok else np.zeros(U)
            rows.append(dict(labels=labels, frame_state=fs[b].copy(), frame_class=fc[b].copy(), n_frames=int((fs[b] >= 0).sum()),
                             segments=seg, segments_input=seg_in, label_logp=lp[b, :U].copy(), confidence=conf.astype(np.float32),
                             score=float(score[b]), total_logp=float(-nll[b])))
        return rows

    def _backward(self):
        lib = _lib.load()
        st = self._cur
        s = self._stream()
        wd = self._workspace("dec", st["ws_dec"])
        st["pending_backward"] = False
        # a cleargrads() deferred to this pass: the decoder backward zeroes the arena in front of everything it accumulates (astk.h zero_ptr)
        if self.arena.take_zero():
            st["dd"].zero_ptr, st["dd"].zero_bytes = self.arena._grad.data_ptr(), 4 * self.arena.size
        else:
            st["dd"].zero_ptr, st["dd"].zero_bytes = None, 0

        def dec_bwd(phase, stream):
            check(lib.astk_decoder_bwd_phase_ex(C.byref(st["dd"]), C.byref(st["dp"]), C.byref(st["dg"]), _vp(st["enc_states"]), _vp(st["c0"]),
                                                _vp(st["h0"]), _vp(st["y"]), _vp(st["emb_mask"]), _vp(st["rnn_masks"]), _vp(st["out_mask"]),
                                                _vp(st["d_enc"]), _vp(st["d_c0"]), _vp(st["d_h0"]), _vp(wd), wd.numel(), phase, stream))
        joined = None
        side = self._side_stream()
        free = lib.astk_lstm_stack_free_cus(C.byref(st["ld"])) if side is not None else 0
        if side is not None and free >= 16:
            # The encoder's backward recurrence (0.7 ms; one workgroup on each of 96-192 CUs, one wave per SIMD) leaves the rest of the
            # device idle and needs nothing from the decoder's parameter gradients (0.17 ms of GEMMs at full speed).  They run beside
            # it on the side stream, every grid capped at the free CUs, ordered after the chain phase by an event and joined before
            # anything reads the gradient arena or reuses the workspace.
            main = torch.cuda.current_stream(self.device)
            dec_bwd(1, s)                                    # ASTK_DEC_BWD_CHAIN
            fork = torch.cuda.Event()
            fork.record(main)
            st["dd"].side_wgs = free
            with torch.cuda.stream(side):
                side.wait_event(fork)
                dec_bwd(2, C.c_void_p(side.cuda_stream))     # ASTK_DEC_BWD_PARAMS
                joined = torch.cuda.Event()
                joined.record(side)
            st["dd"].side_wgs = 0
        else:
            dec_bwd(0, s)
        if st.get("ctc") is not None:
            self._ctc_backward(st, s)                        # behind the chain phase on the main stream: d_enc and the arena's zero fill are done
        # The decoder's gradient range is final here, but its all-reduce is NOT launched yet: an RCCL kernel holds its CUs until every
        # peer has arrived, and the encoder's backward recurrence (next) needs up to 192 CUs to itself to become resident -- a peer
        # that is late would turn into a time-out of the recurrence's bounded spins.  Both ranges go out behind the recurrence and
        # hide behind the encoder's batched weight-gradient products and the CNN backward instead.
        h, nd = self.h, self.n_dirs
        # encoder layers without a decoder counterpart keep the zero gradient they were allocated with
        self._bridge_states(st, st["d_c0"], st["d_h0"], st["d_cT"], st["d_hT"], False)
        if self.enc_variant is not None:
            self.enc_variant.backward(st, st["d_enc"], st["d_cT"], st["d_hT"], st["d_xlstm"])
        else:
            wl = self._workspace("lstm", st["ws_lstm"])
            check(lib.astk_lstm_stack_bwd(C.byref(st["ld"]), st["lp"], st["lg"], _vp(st["xlstm"]), _vp(st["enc_masks"]), _vp(st["d_enc"]),
                                          _vp(st["d_cT"]), _vp(st["d_hT"]), _vp(st["d_xlstm"]), _vp(wl), wl.numel(), s))
        if joined is not None:
            # from here on everything is on one stream again, and the gradient exchange is launched from it
            torch.cuda.current_stream(self.device).wait_event(joined)
        if self.grad_buckets is not None:
            self.grad_buckets.launch("dec")
            self.grad_buckets.launch("enc")
        wc = self._workspace("cnn", st["ws_cnn"])
        sx = self.stat_exchange if st.get("bn_world", 1) > 1 else None   # backward of the statistics the forward pass used
        if sx is None:
            check(lib.astk_conv_bn_relu_bwd(C.byref(st["cd"]), st["cp"], st["cg"], _vp(st["d_xlstm"]), _vp(wc), wc.numel(), s))
        else:
            rc = lib.astk_conv_bn_relu_bwd_sync(C.byref(st["cd"]), st["cp"], st["cg"], _vp(st["d_xlstm"]), _vp(wc), wc.numel(),
                                                C.cast(sx.bind(wc).callback, C.c_void_p), None, sx.world, s)
            if sx.error is not None:
                raise sx.error
            check(rc)
        if self.grad_buckets is not None:
            self.grad_buckets.launch("cnn")
        # (the status word once more, behind the backward recurrences: astk_cnn_desc.status_dst, written by the CNN backward's last kernel)
        if self.grad_buckets is not None:
            # ... and once more behind the gradient exchange, when the peers' words have been merged (GradBuckets.finish): every rank's
            # pair of THIS step then carries the merged word
            self.grad_buckets.status_dest = st["loss"][1:2]

    # ------------------------------------------------------------------ inference (seq2seq.py:361-396, 475-568)
    def decode_step(self, word, ht):
        """Eval-mode step for predict()/beam: returns (logits (B,V), ht (B,A), alphas (B,T'',1))."""
        lib = self._require_gpu()
        if config.train:
            raise NotImplementedError("decode_step outside forward_loss is provided for eval mode (predict / beam)")
        st = self._cur
        if isinstance(word, np.ndarray):
            word = torch.from_numpy(word)
        word = word.to(self.device, torch.int32).contiguous()
        B = word.shape[0]
        ht = ht.to(self.device, torch.float32).contiguous().clone()
        logits = torch.empty(B, self.V, dtype=torch.float32, device=self.device)
        alpha = torch.empty(B, st["T2"], dtype=torch.float32, device=self.device)
        wd = self._workspace("dec", st["ws_dec"])
        check(lib.astk_decoder_step_infer(C.byref(st["dd"]), C.byref(st["dp"]), _vp(st["enc_states"]), _vp(self._dec_c),
                                          _vp(self._dec_h), _vp(ht), _vp(word), _vp(logits), _vp(alpha), None, _vp(wd), wd.numel(),
                                          self._stream()))
        return logits, ht, alpha.unsqueeze(2)

    def predict(self, X, start_token, end_token, stop_limit, rows=None):
        return self.predict_async(X, start_token, end_token, stop_limit, rows=rows).result()

    # What the decode entry points share.  _begin_decode: the eval-mode encoding and decoder state of a batch.  _device_decode: a mode's
    # one persistent launch with its one-copy read-back, or None for shapes the library does not run on the device loop (it reports a
    # workspace of 0).  _device_or_steps: that handle, or else the mode's per-step loop, finished on return.
    def _begin_decode(self, X, rows=None):
        if rows is not None:
            if X is not None:
                raise ValueError("decode: give X or rows=, not both")
            return self._adopt_rows(rows)
        if X is None:
            raise ValueError("decode: give X or rows=")
        X = self._as_input(X)
        self._cur = None
        self.encode(X)
        self.init_decoder_state()
        return self._cur["B"]

    def _adopt_rows(self, rows):
        """A RowBatch in place of an encoded batch: a decoder state of its own (B rows, T = T''max, the lengths uploaded), which the
        decode entry points read exactly as they read the state _begin_decode leaves."""
        lib = self._require_gpu()
        if not isinstance(rows, RowBatch):
            raise ValueError(f"decode: rows must be a RowBatch, got {type(rows).__name__}")
        if self.arena is None:
            raise ValueError("decode: the model has no parameters yet (materialize it, or encode a batch, first)")
        nl = len(self.rnn_dec)
        if int(rows.enc.shape[2]) != self.H or int(rows.c0.shape[0]) != nl:
            raise ValueError(f"decode: rows hold H = {int(rows.enc.shape[2])} and {int(rows.c0.shape[0])} decoder layers, "
                             f"the model H = {self.H} and {nl}")
        B, T2 = rows.B, rows.T
        f32 = dict(device=self.device, dtype=torch.float32)
        dd = self._decoder_desc(B, 2, T2)
        dd.precision, dd.gemm_operands = _lib.PREC_BY_NAME[self.gemm_precision], _lib.OPERANDS_BY_NAME[self.gemm_operands]
        dd.deterministic = 1 if self.deterministic else 0
        dp, _ = self._decoder_tables()
        enc = rows.enc.to(**f32).contiguous()
        self._cur = dict(B=B, T2=T2, dd=dd, dp=dp, enc_states=enc, rows=rows, ws_dec=int(lib.astk_decoder_workspace_bytes(C.byref(dd))),
                         row_len=torch.from_numpy(rows.lens).to(self.device))
        self.enc_states = enc
        self._dec_c, self._dec_h = rows.c0.to(**f32).contiguous().clone(), rows.h0.to(**f32).contiguous().clone()
        return B

    def encode_rows(self, Xs, rows_of=None, batch_encode=None):
        """A RowBatch of utterances: every X of the list Xs ((1, T_u, D) or (T_u, D)) is encoded as it is ALONE, at batch 1 in eval mode
        -- the reference's encoder has no length masks, so this is the only encoding that does not depend on the batch around it, and
        the one beam search sees -- and seeds its rows' decoder state as init_decoder_state does.  rows_of[b] = the utterance of row b
        (default: one row per utterance, in order); at most 32 rows.
        batch_encode (default: the model's attribute, False): the distinct utterances of rows_of go through the encoder in padded
        batches of up to 32 with per-row lengths (_encode_batched) instead of one call each; last_encode_path says which ran."""
        rows_of = list(range(len(Xs))) if rows_of is None else [int(u) for u in rows_of]
        if not rows_of or len(rows_of) > ROWS_MAX:
            raise ValueError(f"encode_rows: 1..{ROWS_MAX} rows, got {len(rows_of)}")
        if min(rows_of) < 0 or max(rows_of) >= len(Xs):
            raise ValueError(f"encode_rows: rows_of names utterances outside 0..{len(Xs) - 1}")
        encs, c0s, h0s = self._encode_utts(Xs, batch_encode=batch_encode, only=sorted(set(rows_of)))
        lens = {u: int(encs[u].shape[0]) for u in set(rows_of)}
        f32 = dict(device=self.device, dtype=torch.float32)
        enc = torch.zeros(len(rows_of), max(lens[u] for u in rows_of), self.H, **f32)
        for b, u in enumerate(rows_of):
            enc[b, :lens[u]] = encs[u]
        return RowBatch(enc, [lens[u] for u in rows_of], torch.stack([c0s[u] for u in rows_of], 1), torch.stack([h0s[u] for u in rows_of], 1))

    def _encode_utts(self, Xs, seeds=None, batch_encode=None, only=None):
        """What encode_rows and the batched beam searches share: _encode_alone, or -- batch_encode, default the model's attribute -- the
        same lists from _encode_batched, which encodes the utterances `only` names (default all; the other entries are None).  Models
        the batched calls do not serve (an encoder variant, cnn_pool, a workspace query of 0) take _encode_alone silently."""
        on = self.batch_encode if batch_encode is None else bool(batch_encode)
        out = self._encode_batched(Xs, seeds, only) if on else None
        self.last_encode_path = "alone" if out is None else "batched"
        return self._encode_alone(Xs, seeds) if out is None else out

    def _batch_encode_served(self):
        return self.enc_variant is None and not self.cfg["cnn_config"].get("cnn_pool")

    def _encode_batched(self, Xs, seeds=None, only=None):
        """_encode_alone's lists from padded batches: the utterances, longest first, in batches of at most 32 (plan_encode_batches), each
        batch through _encode_batch.  None (nothing launched) when the model or a batch's shape is not served."""
        if not self._batch_encode_served():
            return None
        Xs = [self._as_input(X) for X in Xs]
        Xs = [X[0] if X.dim() == 3 else X for X in Xs]
        only = list(range(len(Xs))) if only is None else list(only)
        frames = [int(Xs[u].shape[0]) for u in only]
        if min(frames) < 1:
            raise ValueError("encode_rows: an utterance has no frames")
        batches = [[only[k] for k in batch] for batch in plan_encode_batches(frames)]
        encs, c0s, h0s = [None] * len(Xs), [None] * len(Xs), [None] * len(Xs)
        sd = [None] * len(Xs)
        with using_config("train", False):
            plans = [self._plan_encode_batch([Xs[u] for u in batch]) for batch in batches]
            if any(p is None for p in plans):
                return None
            for batch, plan in zip(batches, plans):
                e, c, h, s_ = self._encode_batch([Xs[u] for u in batch], plan)
                for k, u in enumerate(batch):
                    encs[u], c0s[u], h0s[u], sd[u] = e[k], c[k], h[k], s_[k]
        if seeds is not None:
            seeds.extend(sd)
        return encs, c0s, h0s

    def _plan_encode_batch(self, Xs):
        """Shape state and row lengths of one padded batch, or None when the library does not serve its LSTM shape with row lengths."""
        lib = self._require_gpu()
        B, T, D = len(Xs), max(int(X.shape[0]) for X in Xs), int(Xs[0].shape[1])
        st = self._shape_state(B, T, D, 2)
        if int(lib.astk_lstm_stack_rows_workspace_bytes(C.byref(st["ld"]))) == 0:
            return None
        lens = np.asarray([int(X.shape[0]) for X in Xs], dtype=np.int32)
        lens2 = np.asarray([cnn_out_lens(self.cfg["cnn_config"]["cnn_layers"], n)[-1] for n in lens], dtype=np.int32)
        return st, lens, lens2

    def _encode_batch(self, Xs, plan):
        """One padded batch (<= 32 utterances (T_u, D) on the device) through astk_conv_bn_relu_fwd_rows and astk_lstm_stack_fwd_rows and
        the bridge of init_decoder_state: per utterance its states (T''_u, H), decoder c and h (n_layers, H) and its
        get_encoder_states()."""
        lib = self._require_gpu()
        st, lens, lens2 = plan
        B, T = st["B"], st["T"]
        X = torch.zeros(B, T, st["D"], dtype=torch.float32, device=self.device)      # zeros behind every row's frames: the entry point's contract
        for b, Xu in enumerate(Xs):
            X[b, :int(lens[b])] = Xu
        row_len, row_len2 = torch.from_numpy(lens).to(self.device), torch.from_numpy(lens2).to(self.device)
        self._cur = st
        s = self._stream()
        wc = self._workspace("cnn", st["ws_cnn"])
        check(lib.astk_conv_bn_relu_fwd_rows(C.byref(st["cd"]), st["cp"], _vp(X), _vp(row_len), _vp(st["xlstm"]), None, _vp(wc), wc.numel(), s))
        st["ld"].x_amax = lib.astk_conv_out_amax(C.byref(st["cd"]), _vp(wc), wc.numel())
        wl = self._workspace("lstm", st["ws_lstm"])
        side = self._side_stream()
        st["ld"].side_stream = side.cuda_stream if side is not None else None
        check(lib.astk_lstm_stack_fwd_rows(C.byref(st["ld"]), st["lp"], _vp(st["xlstm"]), _vp(row_len2), _vp(st["enc_states"]),
                                           _vp(st["cT"]), _vp(st["hT"]), _vp(wl), wl.numel(), s))
        self.enc_states = st["enc_states"]
        self._bridge_states(st, st["c0"], st["h0"], st["cT"], st["hT"], True)
        nd = self.n_dirs
        encs = [st["enc_states"][b, :int(lens2[b])].clone() for b in range(B)]
        c0s, h0s = [st["c0"][:, b].clone() for b in range(B)], [st["h0"][:, b].clone() for b in range(B)]
        seeds = [{k: [torch.cat([st[k + "T"][d_, l, b:b + 1] for d_ in range(nd)], 1) for l in range(len(self.rnn_enc))] for k in ("c", "h")}
                 for b in range(B)]
        return encs, c0s, h0s, seeds

    def _encode_alone(self, Xs, seeds=None):
        """Every utterance of Xs encoded at its own length, copied out of the pooled buffers: its states (T''_u, H) and the decoder
        state (n_layers, H) of init_decoder_state, c and h.  seeds (a list): also collects get_encoder_states() of every utterance."""
        encs, c0s, h0s = [], [], []
        with using_config("train", False):
            for X in Xs:
                X = self._as_input(X)
                self.encode(X[None] if X.dim() == 2 else X)
                self.init_decoder_state()
                encs.append(self.enc_states[0].clone())
                c0s.append(self._dec_c[:, 0].clone())
                h0s.append(self._dec_h[:, 0].clone())
                if seeds is not None:
                    seeds.append(self.get_encoder_states())
        return encs, c0s, h0s

    def _readback(self, key, slot, n, dtype):
        """n words of the pooled device buffer of (key, slot) and of its pinned twin; both only ever grow."""
        host = self._pinned.get((key, slot))
        if host is None or host.numel() < n:
            host = self._pinned[(key, slot)] = torch.empty(n, dtype=dtype, pin_memory=True)
        return self._pool(f"{key}_out{slot}", (n,), dtype), host[:n]

    def _device_decode(self, key, slot, nbytes, n, call, args, n_alpha=0, takes_rows=False, **pending):
        """`call` = the mode's library entry point, `nbytes` its workspace query; the launch writes n int32 words (and n_alpha floats,
        forced alpha) that come back in one non-blocking copy each, followed by an event.  args(p, alpha) = the mode's own arguments
        between the decoder state and the workspace: p(k) is the address of byte k of the words, alpha the float buffer's or None.
        takes_rows: `call` itself ends with row_len (NULL allowed) and has no _rows twin.
        `pending`: the status word's index, `where`, parse and keep of the _Pending handle returned."""
        if nbytes == 0 or self._rows_alone:
            return None
        ws = self._workspace("decode", nbytes)
        out, host = self._readback(key, slot, n, torch.int32)
        alpha, host_alpha = self._readback(key + "_alpha", slot, n_alpha, torch.float32) if n_alpha else (None, None)
        st, base = self._cur, out.data_ptr()
        lens = st.get("row_len")              # a RowBatch: the mode's _rows entry point, the lengths behind the stream
        if lens is not None:
            call = call if takes_rows else getattr(_lib.load(), call.__name__ + "_rows")
            pending["keep"] = (pending.get("keep"), lens, st["enc_states"])
        check(call(C.byref(st["dd"]), C.byref(st["dp"]), _vp(st["enc_states"]), _vp(self._dec_c), _vp(self._dec_h),
                   *args(lambda k: C.c_void_p(base + k), _vp(alpha)), _vp(ws), ws.numel(), self._stream(),
                   *(() if lens is None and not takes_rows else (_vp(lens),))))
        host.copy_(out, non_blocking=True)
        if n_alpha:
            host_alpha.copy_(alpha, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return _Pending(host, host_alpha, ev, **pending)

    def _device_or_steps(self, path_attr, handle, steps, alone=None):
        """alone(b, rows_b, end, stop) = the same decode of row b of a RowBatch by itself (rows_b: its one-row batch), for the per-step
        path: the per-step loops have no lengths, so there every row runs ALONE at B = 1 and T = its length."""
        setattr(self, path_attr, "steps" if handle is None else "device")
        if handle is not None:
            return handle
        rows = self._cur.get("rows")
        if rows is None or (rows.B == 1 and int(rows.lens[0]) == rows.T):
            return _Ready(steps())
        prev, self._rows_alone = self._rows_alone, True
        try:
            return _Ready(alone(rows))
        finally:
            self._rows_alone = prev
            setattr(self, path_attr, "steps")

    def _free_rows_alone(self, rows, end_token, stop_limit, run):
        """The free-running modes row by row: run(b, rows_b, end, stop) decodes row b alone.  A batch stops when ALL its rows have
        emitted end_token and every row decodes until then, so a row that stops earlier alone is decoded again, without a stop, for
        the batch's step count.  Returns the rows' results, each of n_steps columns."""
        first = [run(b, rows.row(b), end_token, stop_limit) for b in range(rows.B)]
        width = lambda r: int((r.tokens if isinstance(r, ScoredPrediction) else r).shape[1])
        n = max(width(r) for r in first)
        return [r if width(r) == n else run(b, rows.row(b), -1, n) for b, r in enumerate(first)], n

    def predict_async(self, X, start_token, end_token, stop_limit, slot=0, rows=None):
        """predict() with the read-back left to the caller: returns a handle whose result() is predict()'s array.  On the device path
        (include/astk.h astk_greedy_decode: the whole decode in one persistent launch) the tokens, n_steps and the status word come back
        in ONE copy into pinned buffer `slot` (0 or 1), which result() waits for: a caller that enqueues the next batch before it reads this
        one keeps the device busy (NN.predict alternates the slots).  Shapes the library does not run on the device loop (it reports a
        workspace of 0) take the per-step loop, which finishes before this returns.  `last_predict_path` says which path ran.
        rows= (a RowBatch, with X = None) decodes rows of different utterances, each over its own length; so for the other modes."""
        lib = _lib.load()
        go, eos, stop = int(start_token), int(end_token), int(stop_limit)
        with using_config("train", False):
            B = self._begin_decode(X, rows)
            # [n_steps, status word (float), 2 pad words, tokens (stop_limit, B)]
            handle = self._device_decode(
                "greedy", slot, int(lib.astk_greedy_workspace_bytes(C.byref(self._cur["dd"]), stop)), 4 + stop * B, lib.astk_greedy_decode,
                lambda p, _: (go, eos, stop, p(16), p(0), p(4)),
                status_at=1, where="predict", parse=lambda v, _: v[4:4 + int(v[0]) * B].reshape(int(v[0]), B).T.copy())
            def alone(rb):
                out, _ = self._free_rows_alone(rb, end_token, stop_limit, lambda b, r1, end, lim: self.predict(None, start_token, end, lim, rows=r1))
                return np.concatenate(out, axis=0)
            return self._device_or_steps("last_predict_path", handle, lambda: self._free_steps(start_token, end_token, stop_limit)[0], alone)

    def predict_scored(self, X, start_token, end_token, stop_limit, y=None, rows=None):
        """predict() that also scores what it decodes: a ScoredPrediction (tokens as predict() returns them, the log-probability of each
        emitted token, and -- with targets y (B, L) -- the free-running cross-entropy of every step against y[:, s+1] and its sum, the
        dev loss).  The decode is predict()'s in every case (up to stop_limit steps, all-EOS early stop): steps past L - 1 have no
        target and add 0, so `loss` is the value of the reference's loop, which stops at L - 1 (enc_dec.py:384-385)."""
        return self.predict_scored_async(X, start_token, end_token, stop_limit, y, rows=rows).result()

    def predict_scored_async(self, X, start_token, end_token, stop_limit, y=None, slot=0, rows=None):
        """predict_scored with the read-back left to the caller, like predict_async: on the device path (astk_greedy_decode_scored) ONE
        copy of [n_steps, status, tokens, logp, nll] into pinned buffer `slot`; otherwise the per-step loop, finished on return."""
        lib = _lib.load()
        go, eos, stop = int(start_token), int(end_token), int(stop_limit)
        with using_config("train", False):
            if rows is not None and y is not None and (np.ndim(y) != 2 or int(np.shape(y)[0]) != rows.B):
                raise ValueError(f"predict_scored: y must be (B = {rows.B}, L >= 1), got {tuple(np.shape(y))}")
            B = self._begin_decode(X, rows)
            if y is not None:
                y = torch.as_tensor(y).to(self.device, torch.int32).contiguous()
                if y.dim() != 2 or y.shape[0] != B or y.shape[1] < 1:
                    raise ValueError(f"predict_scored: y must be (B = {B}, L >= 1), got {tuple(y.shape)}")
            # [n_steps, status word (float), 2 pad words, tokens | logp | nll, each (stop_limit, B)]
            sb = stop * B
            handle = self._device_decode(
                "greedy_scored", slot, int(lib.astk_greedy_scored_workspace_bytes(C.byref(self._cur["dd"]), stop)),
                4 + (3 if y is not None else 2) * sb, lib.astk_greedy_decode_scored,
                lambda p, _: (go, eos, stop, _vp(y), int(y.shape[1]) if y is not None else 0, _vp(self.mask_pad_id), p(16), p(16 + 4 * sb),
                              p(16 + 8 * sb) if y is not None else None, p(0), p(4)),
                status_at=1, where="predict_scored", keep=y,
                parse=lambda v, _: scored_from_rows(v[4:], int(v[0]), B, stop, y is not None, eos))

            def steps():
                """Each step's logits scored: a float64 log_softmax on the device, the token's and the target's entries."""
                w64 = self.mask_pad_id.double()

                def record(logits, word, s):
                    ls = torch.log_softmax(logits.double(), dim=1)
                    lp = ls.gather(1, word.long()[:, None])[:, 0]
                    if y is None:
                        return (lp,)
                    if s + 1 < y.shape[1]:
                        t = y[:, s + 1].long().clamp(0, self.V - 1)
                        return lp, -w64[t] * ls.gather(1, t[:, None])[:, 0]
                    return lp, torch.zeros(B, dtype=torch.float64, device=self.device)
                tokens, cols = self._free_steps(start_token, end_token, stop_limit, record=record)
                return ScoredPrediction(tokens, cols[0], cols[1] if y is not None else None, eos)

            def alone(rb):
                out, _ = self._free_rows_alone(rb, end_token, stop_limit, lambda b, r1, end, lim: self.predict_scored(
                    None, start_token, end, lim, None if y is None else y[b:b + 1], rows=r1))
                cat = lambda k: np.concatenate([getattr(r, k) for r in out], axis=0)
                return ScoredPrediction(cat("tokens"), cat("logp"), cat("nll") if y is not None else None, eos)
            return self._device_or_steps("last_predict_path", handle, steps, alone)

    def sample(self, X, start_token, end_token, stop_limit, seed, streams=None, temperature=1.0, rows=None, top_k=None, top_p=1.0):
        """Ancestral sampling: predict_scored() with every step's token drawn from softmax(logits / temperature) by the Gumbel-max
        noise of include/astk.h -- row b draws from (seed, streams[b]) alone (streams defaults to the rows' indices), whatever its
        position and whatever the batch around it.  Returns a ScoredPrediction: tokens (B, n_steps), logp the log-probability of each
        drawn token under the sampled distribution, score cut at the first `end_token`; nll and loss are None.  A row is finished once
        it has drawn `end_token`; the decode stops when every row has, or at stop_limit.
        top_k (1..16) / top_p in (0, 1]: truncated sampling, the contract of include/astk.h ("truncated sampling on the device") -- the
        top_k largest xs = logits * inv_temp are the candidates (higher values first, among equal values the lower token id first),
        cut to the smallest prefix whose renormalised mass reaches top_p (top_p == 1: no cut), and the token is drawn among the kept
        by the same noise.  logp is then the log-probability under the distribution actually sampled -- the renormalised kept set --
        NOT the model's full-softmax log-probability; score() gives that.  `kept` holds the kept count of every draw.  top_p < 1
        needs a top_k: the nucleus is taken among top_k <= 16 candidates.  top_k = None and top_p = 1 is the untruncated draw."""
        return self.sample_async(X, start_token, end_token, stop_limit, seed, streams, temperature, rows=rows, top_k=top_k, top_p=top_p).result()

    def sample_async(self, X, start_token, end_token, stop_limit, seed, streams=None, temperature=1.0, slot=0, rows=None, top_k=None,
                     top_p=1.0):
        """sample() with the read-back left to the caller, like predict_scored_async: on the device path (astk_sample_decode, one
        persistent launch) ONE copy of [n_steps, status, tokens, logp] into pinned buffer `slot`; otherwise the per-step loop,
        finished on return.  `last_predict_path` says which path ran.  With top_k / top_p (astk_sample_decode_topk) the copy is
        [n_steps, status, tokens, logp, kept]."""
        inv_temp = checked_temperature(temperature)
        top_k, top_p = checked_truncation(top_k, top_p, getattr(self, "V", None))
        lib = _lib.load()
        go, eos, stop = int(start_token), int(end_token), int(stop_limit)
        with using_config("train", False):
            if rows is not None and streams is not None and len(list(streams)) != rows.B:
                raise ValueError(f"sample: streams must name B = {rows.B} rows, got {len(list(streams))}")
            B = self._begin_decode(X, rows)
            streams = list(range(B)) if streams is None else [int(v) for v in streams]
            if len(streams) != B:
                raise ValueError(f"sample: streams must name B = {B} rows, got {len(streams)}")
            keys = np.array([sample_row_key(seed, v) for v in streams], dtype=np.uint64)
            keys = torch.from_numpy(keys.view(np.int64)).to(self.device)      # (the bit patterns: torch has no uint64 arithmetic to offer)
            # [n_steps, status word (float), 2 pad words, tokens | logp, each (stop_limit, B)]
            sb = stop * B
            if top_k is None:
                handle = self._device_decode(
                    "sample", slot, int(lib.astk_sample_workspace_bytes(C.byref(self._cur["dd"]), stop)), 4 + 2 * sb, lib.astk_sample_decode,
                    lambda p, _: (go, eos, stop, _vp(keys), inv_temp, p(16), p(16 + 4 * sb), p(0), p(4)),
                    status_at=1, where="sample", keep=keys, parse=lambda v, _: scored_from_rows(v[4:], int(v[0]), B, stop, False, eos))
            else:
                # [n_steps, status word (float), 2 pad words, tokens | logp | kept, each (stop_limit, B)]
                handle = self._device_decode(
                    "sample_topk", slot, int(lib.astk_sample_topk_workspace_bytes(C.byref(self._cur["dd"]), stop)), 4 + 3 * sb,
                    lib.astk_sample_decode_topk,
                    lambda p, _: (go, eos, stop, _vp(keys), inv_temp, top_k, top_p, p(16), p(16 + 4 * sb), p(16 + 8 * sb), p(0), p(4)),
                    takes_rows=True, status_at=1, where="sample", keep=keys,
                    parse=lambda v, _: scored_from_rows(v[4:], int(v[0]), B, stop, False, eos, has_kept=True))

            def steps():
                """Per step one astk_gumbel_rows fill, the argmax of logits * inv_temp + g in float32, and the drawn token's entry of a
                float64 log_softmax of logits * inv_temp."""
                g = torch.empty(B, self.V, dtype=torch.float32, device=self.device)

                drawn = {}

                def pick(logits, s):
                    check(lib.astk_gumbel_rows(_vp(keys), B, s, self.V, _vp(g), self._stream()))
                    if top_k is None:
                        return (logits * inv_temp + g).argmax(dim=1).to(torch.int32)
                    # truncated: the pure pick function on this step's logits and noise; its logp and kept count are this step's record
                    word, drawn["logp"], drawn["kept"] = truncated_pick(logits, g, inv_temp, top_k, top_p)
                    return word

                def record(logits, word, s):
                    if top_k is not None:
                        return drawn["logp"], drawn["kept"].double()
                    return (torch.log_softmax(logits.double() * inv_temp, dim=1).gather(1, word.long()[:, None])[:, 0],)
                tokens, cols = self._free_steps(start_token, end_token, stop_limit, pick, record)
                return ScoredPrediction(tokens, cols[0], None, eos, None if top_k is None else np.rint(cols[1]).astype(np.int32))

            def alone(rb):
                out, _ = self._free_rows_alone(rb, end_token, stop_limit, lambda b, r1, end, lim: self.sample(
                    None, start_token, end, lim, seed, [streams[b]], temperature, rows=r1, top_k=top_k, top_p=top_p))
                cat = lambda k: np.concatenate([getattr(r, k) for r in out], axis=0)
                return ScoredPrediction(cat("tokens"), cat("logp"), None, eos, None if top_k is None else cat("kept"))
            return self._device_or_steps("last_predict_path", handle, steps, alone)

    def _free_steps(self, start_token, end_token, stop_limit, pick=None, record=None):
        """The free-running per-step loop (seq2seq.py:475-527): one astk_decoder_step_infer, a pick and a host read per token, until
        every row has emitted `end_token` or at stop_limit.  pick(logits, s) = the int32 tokens of step s (default: the argmax);
        record(logits, tokens, s) = a tuple of (B,) columns kept beside them.  Returns (tokens (B, n_steps) int32, the recorded columns
        as (B, n_steps) float32 arrays), on the host."""
        with using_config("train", False):
            B = self._cur["B"]
            ht = torch.zeros(B, self.A, dtype=torch.float32, device=self.device)
            word = torch.full((B,), start_token, dtype=torch.int32, device=self.device)
            done = torch.zeros(B, dtype=torch.bool, device=self.device)
            rows, cols, npred = [], [], 0
            while npred < stop_limit:
                logits, ht, _ = self.decode_step(word, ht)
                word = logits.argmax(dim=1).to(torch.int32) if pick is None else pick(logits, len(rows))
                if record is not None:
                    cols.append(record(logits, word, len(rows)))
                rows.append(word)
                done |= word == end_token
                if bool(done.all()):
                    break
                npred += 1
            return torch.stack(rows, 0).T.cpu().numpy(), [torch.stack(c, 0).T.float().cpu().numpy() for c in zip(*cols)]

    def score(self, X, y, return_alpha=False, rows=None):
        """Forced decoding: the eval-mode model run along the given translations y (B, L) -- step s is fed y[:, s] and scored against
        y[:, s + 1] -- as a ForcedScore: per-token log-probabilities, the argmax and its log-probability, PAD weights, per-row scores,
        the teacher-forced loss and, with return_alpha, the attention rows (B, L - 1, T'').  `last_score_path` says which path ran."""
        return self.score_async(X, y, return_alpha, rows=rows).result()

    def score_async(self, X, y, return_alpha=False, slot=0, rows=None):
        """score() with the read-back left to the caller, like predict_scored_async: on the device path (astk_forced_score, one
        persistent launch) ONE copy of [status, logp, logp_max, pred] into pinned buffer `slot` (alpha, when asked for, is one more
        copy); shapes the library does not run on the device loop take the per-step loop, finished on return."""
        y_host = checked_targets(y, self.V)
        lib = _lib.load()
        with using_config("train", False):
            if rows is not None and y_host.shape[0] != rows.B:
                raise ValueError(f"score: y must have B = {rows.B} rows, got {tuple(y_host.shape)}")
            B = self._begin_decode(X, rows)
            if y_host.shape[0] != B:
                raise ValueError(f"score: y must have B = {B} rows, got {tuple(y_host.shape)}")
            weight = (y_host[:, 1:] != 0).astype(np.float32)         # mask_pad_id[y[:, 1:]]: 0 at PAD, else 1 (materialize)
            y_dev = torch.from_numpy(y_host).to(self.device)
            S, with_alpha = int(y_dev.shape[1]) - 1, bool(return_alpha)
            # [status word (float), 3 pad words, logp | logp_max | pred, each (S, B)]; alpha (S, B, T'') in a buffer of its own
            # (a workspace of 0 also for S > ASTK_GREEDY_MAX_STEPS: the per-step loop serves those)
            sb = S * B
            handle = self._device_decode(
                "forced", slot, int(lib.astk_forced_workspace_bytes(C.byref(self._cur["dd"]), S, int(with_alpha))), 4 + 3 * sb,
                lib.astk_forced_score, lambda p, alpha: (_vp(y_dev), S + 1, p(16), p(16 + 4 * sb), p(16 + 8 * sb), alpha, p(0)),
                n_alpha=sb * self._cur["T2"] if with_alpha else 0, status_at=0, where="score", keep=y_dev,
                parse=lambda v, al: forced_from_rows(v[4:], B, S, weight, None if al is None else al.reshape(S, B, -1).transpose(1, 0, 2).copy()))
            def alone(rb):
                out = [self.score(None, y_host[b:b + 1], with_alpha, rows=rb.row(b)) for b in range(rb.B)]
                cat = lambda k: np.concatenate([getattr(r, k) for r in out], axis=0)
                alpha = None
                if with_alpha:            # (B, S, T''max), zeros beyond each row's length
                    alpha = np.zeros((rb.B, S, rb.T), dtype=np.float32)
                    for b, r in enumerate(out):
                        alpha[b, :, :r.alpha.shape[2]] = r.alpha[0]
                return ForcedScore(cat("logp"), cat("logp_max"), cat("pred"), weight, alpha)
            return self._device_or_steps("last_score_path", handle, lambda: self._score_steps(y_dev, weight, with_alpha), alone)

    def _score_steps(self, y, weight, with_alpha):
        """The per-step forced loop: y[:, s] through decode_step, a float64 log_softmax of each step's logits on the device.  (Kept apart
        from _free_steps: a fixed number of steps, the given token fed, and the attention rows kept.)"""
        with using_config("train", False):
            B, S = self._cur["B"], int(y.shape[1]) - 1
            ht = torch.zeros(B, self.A, dtype=torch.float32, device=self.device)
            lps, lpm, preds, alphas = [], [], [], []
            for s in range(S):
                logits, ht, al = self.decode_step(y[:, s].contiguous(), ht)
                ls = torch.log_softmax(logits.double(), dim=1)
                t = y[:, s + 1].long().clamp(0, self.V - 1)
                lps.append(ls.gather(1, t[:, None])[:, 0])
                lpm.append(ls.max(dim=1).values)
                preds.append(logits.argmax(dim=1).to(torch.int32))
                if with_alpha:
                    alphas.append(al[:, :, 0])
            f32 = lambda r: torch.stack(r, 0).T.float().cpu().numpy()
            alpha = torch.stack(alphas, 1).cpu().numpy() if with_alpha else None
            return ForcedScore(f32(lps), f32(lpm), torch.stack(preds, 0).T.cpu().numpy(), weight, alpha)

    def get_encoder_states(self):
        st = self._cur
        h = self.h
        out = {"c": [], "h": []}
        for k in range(len(self.rnn_enc)):
            out["c"].append(torch.cat([st["cT"][d_, k] for d_ in range(self.n_dirs)], 1))
            out["h"].append(torch.cat([st["hT"][d_, k] for d_ in range(self.n_dirs)], 1))
        return out

    def get_decoder_states(self):
        return {"c": [self._dec_c[l].clone() for l in range(len(self.rnn_dec))],
                "h": [self._dec_h[l].clone() for l in range(len(self.rnn_dec))]}

    def set_decoder_states(self, rnn_states):
        n = len(self.rnn_dec)
        B = rnn_states["c"][0].shape[0]
        c = torch.zeros(n, B, self.H, dtype=torch.float32, device=self.device)
        hh = torch.zeros(n, B, self.H, dtype=torch.float32, device=self.device)
        for l in range(min(n, len(rnn_states["c"]))):
            c[l] = rnn_states["c"][l]
            hh[l] = rnn_states["h"][l]
        self._dec_c, self._dec_h = c, hh
