"""Minimum-risk training (MRT; MWER training in ASR) -- DESIGN.md section 37.  For the candidates {y_i} of one utterance with sequence
log-probabilities s_i and costs c_i (1 - sentence BLEU, or the edit distance per reference token),

    Q_i = exp(alpha s_i) / sum_j exp(alpha s_j),   R = sum_i Q_i c_i   (the expected cost),
    dR/dtheta = d/dtheta sum_i w_i NLL_i   with   w_i = alpha Q_i (R - c_i),   Q held fixed:

a cross-entropy gradient with one signed weight per batch row, which forward_loss(row_weight=) takes (astk_decoder_fwd_w).  One step
(mrt_step): sample N translations per utterance on the device (model.sample; the step's only host read-back), build the batch of
U (N + 1) rows -- each utterance's samples and its reference --, count edits / n-gram matches of every (sample, reference) pair in one
astk_pair_stats launch, turn counts and scores into weights in one astk_risk_weights launch, and run the weighted train step.

The objective is (1 - lam) mean_u R_u + lam mean_u NLL(ref_u).  The decoder divides by the row count B = U (N + 1) (quirk Q6), so
risk_scale = (1 - lam) B / U on the risk term and ref_weight = lam B / U on the reference rows.

Approximations, on purpose: Q uses the scores of the sampling pass, which runs in eval mode (running BatchNorm statistics, no dropout),
and is a constant of the step; the reference is not part of the candidate set (that needs a forced-scoring pass; the flags of
astk_risk_weights allow it later).  The encoder runs on all B rows: (N + 1) times the plain step's encoder cost.

The pieces are pure functions the CPU suite tests: checked_mrt, risk_weights_host (the float64 restatement of astk_risk_weights),
build_mrt_batch."""
import ctypes
import math
import numbers

import numpy as np

from . import _lib
from .eval import bleu_from_counts

PAD_ID, GO_ID, EOS_ID = 0, 1, 2
GREEDY_MAX_STEPS = 512      # astk.h ASTK_GREEDY_MAX_STEPS: the longest decode of the device loop
LIVE, REFERENCE = 1, 2      # the flag bits of astk_risk_weights
DEFAULTS = {"samples": 7, "alpha": 1.0, "cost": "bleu", "mle_weight": 0.0, "max_len": None, "temperature": 1.0, "top_k": None, "top_p": 1.0,
            "seed": 0, "start_epoch": 0}


def _number(c, key, what):
    v = c[key]
    if isinstance(v, bool) or not isinstance(v, (numbers.Real, np.floating, np.integer)) or not math.isfinite(float(v)):
        raise ValueError(f"{what}.{key} must be a finite number, got {v!r}")
    return float(v)


def _integer(c, key, what, lo, hi):
    v = c[key]
    if isinstance(v, bool) or not isinstance(v, (numbers.Integral, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what}.{key} must be an integer in {lo}..{hi}, got {v!r}")
    return int(v)


def checked_mrt(cfg, what="extras.mrt"):
    """The config with every key present, or None for off (cfg None).  Keys: samples (1..63: with the reference a list has at most
    ASTK_RISK_MAX_LIST rows), alpha (>= 0), cost ("bleu" | "edit"), mle_weight (in [0, 1]), max_len (None: the batch's L - 1 + 10, capped
    at ASTK_GREEDY_MAX_STEPS), temperature, top_k, top_p (SpeechEncoderDecoder.sample checks them), seed, start_epoch; defaults:
    DEFAULTS."""
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError(f"{what} must be a dict or null, got {cfg!r}")
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"{what}: unknown key {unknown[0]!r} (known: {', '.join(DEFAULTS)})")
    c = dict(DEFAULTS, **cfg)
    out = {"samples": _integer(c, "samples", what, 1, _lib.RISK_MAX_LIST - 1)}
    out["alpha"] = _number(c, "alpha", what)
    if out["alpha"] < 0:
        raise ValueError(f"{what}.alpha must be >= 0, got {c['alpha']!r}")
    if c["cost"] not in _lib.RISK_COSTS:
        raise ValueError(f"{what}.cost must be 'bleu' or 'edit', got {c['cost']!r}")
    out["cost"] = c["cost"]
    out["mle_weight"] = _number(c, "mle_weight", what)
    if not 0.0 <= out["mle_weight"] <= 1.0:
        raise ValueError(f"{what}.mle_weight must lie in [0, 1], got {c['mle_weight']!r}")
    out["max_len"] = None if c["max_len"] is None else _integer(c, "max_len", what, 1, GREEDY_MAX_STEPS)
    out["temperature"] = _number(c, "temperature", what)
    out["top_k"] = None if c["top_k"] is None else _integer(c, "top_k", what, 1, 16)
    out["top_p"] = _number(c, "top_p", what)
    out["seed"] = _integer(c, "seed", what, 0, (1 << 64) - 1)
    out["start_epoch"] = _integer(c, "start_epoch", what, 0, 2**31 - 1)
    return out


def checked_mrt_setup(mrt, ctc_weight, random_out, world, what="extras.mrt"):
    """What extras.mrt does not combine with, each refused with the key's name: the CTC term (no row weights there), random_out (the
    weighted step scores the rows it was given), data parallelism (out of scope for this version)."""
    if mrt is None:
        return
    if ctc_weight > 0:
        raise ValueError(f"{what} does not combine with extras.ctc_weight > 0 (the CTC term has no row weights)")
    if random_out and float(random_out) > 0:
        raise ValueError(f"{what} does not combine with extras.random_out > 0")
    if world > 1:
        raise ValueError(f"{what} runs on one device only (world size {world})")


# ---- the float64 restatement of astk_risk_weights (include/astk.h)


def _list_rows(first, u, R):
    """(good, lo, hi, zlo, zhi) of list u: the rule of csrc/risk.hip rk_list."""
    lo, hi = int(first[u]), int(first[u + 1])
    prev = int(first[u - 1]) if u > 0 else 0
    good = lo >= 0 and hi <= R and lo <= hi and prev <= lo and hi - lo <= _lib.RISK_MAX_LIST
    return good, lo, hi, max(lo, prev, 0), min(hi, R)


def risk_cost(stats_row, hyp_len, ref_len, cost):
    """c_i of one live row: 1 - sentence BLEU from the clipped matches (ast_amd.eval.bleu_from_counts), or dist / max(1, ref_len)."""
    if cost == "bleu":
        return 1.0 - bleu_from_counts([int(v) for v in stats_row[4:8]], int(hyp_len), int(ref_len))
    return int(stats_row[0]) / max(1, int(ref_len))


def risk_weights_host(first, score, stats, lens, pairs, flags, cost, alpha, risk_scale, ref_weight, fill=0.0):
    """astk_risk_weights on the host, in float64 with each output rounded once to float32: (weight (R,), risk (U,), cost (R,), n_bad).
    alpha, risk_scale and ref_weight are taken as the float32 values the descriptor holds.  Rows no list owns keep `fill`."""
    first, score, stats = np.asarray(first, np.int64), np.asarray(score, np.float32).astype(np.float64), np.asarray(stats, np.int64)
    lens, pairs, flags = np.asarray(lens, np.int64), np.asarray(pairs, np.int64).reshape(-1, 2), np.asarray(flags, np.int64)
    alpha, risk_scale, ref_weight = (float(np.float32(v)) for v in (alpha, risk_scale, ref_weight))
    U, R = len(first) - 1, len(score)
    weight, costs = np.full(R, fill, np.float32), np.full(R, fill, np.float32)
    risk, n_bad = np.zeros(U, np.float32), 0
    for u in range(U):
        good, lo, hi, zlo, zhi = _list_rows(first, u, R)
        if not good:
            n_bad += 1
            weight[zlo:max(zhi, zlo)] = 0.0
            costs[zlo:max(zhi, zlo)] = 0.0
            continue
        rows = range(lo, hi)
        live = [bool(flags[i] & LIVE) and stats[i, 0] >= 0 for i in rows]
        c = [risk_cost(stats[i], lens[pairs[i, 0]], lens[pairs[i, 1]], cost) if l else 0.0 for i, l in zip(rows, live)]
        q = [0.0] * len(c)
        if any(live):
            smax = max(score[i] for i, l in zip(rows, live) if l)
            e = [math.exp(alpha * (score[i] - smax)) if l else 0.0 for i, l in zip(rows, live)]
            tot = math.fsum(e)
            q = [v / tot for v in e]
        rbar = math.fsum(qi * ci for qi, ci in zip(q, c))
        for k, i in enumerate(rows):
            weight[i] = risk_scale * alpha * q[k] * (rbar - c[k]) + (ref_weight if flags[i] & REFERENCE else 0.0)
            costs[i] = c[k]
        risk[u] = rbar
    return weight, risk, costs, n_bad


def risk_weights(first, score, stats, lens, pairs, flags, cost, alpha, risk_scale, ref_weight, with_cost=False, n_bad=None):
    """One astk_risk_weights launch on device tensors (first (U+1,) int32, score (R,) float32, stats / lens / pairs as
    eval.pair_stats(return_device=True) returns them, flags (R,) int32): (weight (R,), risk (U,), cost (R,) or None) on the device,
    nothing read back.  n_bad: a one-element int32 device tensor that receives the count of bad lists, or None."""
    import torch
    lib = _lib.load()
    U, R = int(first.numel()) - 1, int(score.numel())
    assert first.dtype == torch.int32 and flags.dtype == torch.int32 and score.dtype == torch.float32 and stats.dtype == torch.int32
    assert int(stats.numel()) == 8 * R and int(pairs.numel()) == 2 * R and int(flags.numel()) == R, "one stats row, pair and flag per row"
    dev = score.device
    weight, risk = torch.empty(R, dtype=torch.float32, device=dev), torch.empty(U, dtype=torch.float32, device=dev)
    costs = torch.empty(R, dtype=torch.float32, device=dev) if with_cost else None
    desc = _lib.RiskDesc(U, R, _lib.RISK_COSTS[cost], alpha, risk_scale, ref_weight)
    _lib.check(lib.astk_risk_weights(ctypes.byref(desc), _lib.ptr(first), _lib.ptr(score), _lib.ptr(stats), _lib.ptr(lens), _lib.ptr(pairs),
                                     _lib.ptr(flags), _lib.ptr(weight), _lib.ptr(risk), None if costs is None else _lib.ptr(costs),
                                     None if n_bad is None else _lib.ptr(n_bad), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return weight, risk, costs


# ---- the batch of one step


def cut_behind_eos(tokens, eos=EOS_ID):
    """The tokens up to and including the first `eos`; all of them when there is none."""
    t = [int(v) for v in tokens]
    return t[:t.index(eos) + 1] if eos in t else t


def strip_symbols(tokens, symbols=(PAD_ID, GO_ID, EOS_ID)):
    return [int(v) for v in tokens if int(v) not in symbols]


def build_mrt_batch(samples, refs, go=GO_ID, eos=EOS_ID, pad=PAD_ID):
    """The weighted step's batch from samples[u] = the drawn token rows of utterance u (without GO, as sample() returns them) and refs[u] =
    its reference row [GO, .., EOS, PAD ..].  Rows: per utterance its samples in order, then its reference.  Returns a dict:
      y      (R, L) int32: [GO] + a sample cut behind its first EOS (kept whole without one), the reference as it is (trailing PAD
             dropped); padded with PAD to the common L (at least 2)
      flags  (R,) int32: LIVE for a sample unless an earlier sample of the same utterance has the same tokens; REFERENCE alone for the
             reference row (it is not part of the candidate set)
      first  (U + 1,) int32 row offsets of the utterances
      pool   the strings of the pair statistics -- the R rows, then the U references, each with GO, EOS and PAD stripped
      pairs  (R, 2) int32: row i against its utterance's reference, (i, R + u)
      utt    (R,) the utterance of each row"""
    assert len(samples) == len(refs) and len(refs) >= 1
    rows, flags, first, utt = [], [], [0], []
    for u, (cands, ref) in enumerate(zip(samples, refs)):
        seen = set()
        for s in cands:
            t = tuple(cut_behind_eos(s, eos))
            rows.append([go] + list(t))
            flags.append(0 if t in seen else LIVE)
            seen.add(t)
            utt.append(u)
        r = [int(v) for v in ref]
        while len(r) > 1 and r[-1] == pad:
            r.pop()
        rows.append(r)
        flags.append(REFERENCE)
        utt.append(u)
        first.append(len(rows))
    R, L = len(rows), max(2, max(len(r) for r in rows))
    y = np.full((R, L), pad, np.int32)
    for i, r in enumerate(rows):
        y[i, :len(r)] = r
    sym = (pad, go, eos)
    pool = [strip_symbols(r, sym) for r in rows] + [strip_symbols(ref, sym) for ref in refs]
    pairs = np.array([(i, R + u) for i, u in enumerate(utt)], np.int32)
    return {"y": y, "flags": np.asarray(flags, np.int32), "first": np.asarray(first, np.int32), "pool": pool, "pairs": pairs,
            "utt": np.asarray(utt, np.int64)}


def mrt_scales(lam, B, U):
    """(risk_scale, ref_weight) under which the decoder's sum / B is (1 - lam) mean_u R_u + lam mean_u NLL(ref_u)."""
    return (1.0 - lam) * B / U, lam * B / U


def mrt_max_len(cfg, L):
    return int(cfg["max_len"]) if cfg["max_len"] is not None else min(L - 1 + 10, GREEDY_MAX_STEPS)


class MrtStep:
    """What mrt_step returns: `loss` (forward_loss's Loss, backward done), `risk` (U,) float32 device tensor of the expected costs,
    `weight` (R,) device tensor, `batch` (build_mrt_batch's dict), `scores` (R,) host float32 (0 on reference rows), `streams` the
    sample streams the step drew from, `next_stream` the first stream no step has used."""

    def __init__(self, **k):
        self.__dict__.update(k)


def draw_samples(model, X, n, max_len, cfg, first_stream):
    """n samples for each row of the padded batch X (U, T, D): the rows repeated, calls of at most 32 rows, row j of the repeated batch
    drawing from stream first_stream + j of cfg["seed"].  Returns (samples[u] = list of n token rows, scores (U, n) float64, streams)."""
    U = int(X.shape[0])
    Xs = X.repeat_interleave(n, dim=0)
    streams = list(range(first_stream, first_stream + U * n))
    toks, score = [], []
    for lo in range(0, U * n, 32):
        hi = min(lo + 32, U * n)
        r = model.sample(Xs[lo:hi], GO_ID, EOS_ID, max_len, cfg["seed"], streams=streams[lo:hi], temperature=cfg["temperature"],
                         top_k=cfg["top_k"], top_p=cfg["top_p"])
        toks.extend(list(r.tokens))
        score.extend(r.score.tolist())
    samples = [toks[u * n:(u + 1) * n] for u in range(U)]
    return samples, np.asarray(score, np.float64).reshape(U, n), streams


def mrt_step(model, X, y, cfg, step, optimizer=None):
    """One MRT step on a loader batch X (U, T, D), y (U, L) under cfg (a checked_mrt dict).  `step` is the running sample counter: the
    step draws from the streams step .. step + U N - 1 of cfg["seed"] and returns next_stream = step + U N, so no stream is used twice.
    Forward and backward are done on return; with an optimizer its update() too.  After the samples' read-back nothing touches the
    host: `risk` stays on the device for the caller to read when it reads the loss."""
    import torch
    from .eval import pair_stats
    from .seq2seq import using_config
    X = model._as_input(X)
    y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).astype(np.int32)
    U, L = y.shape
    n = int(cfg["samples"])
    samples, scores, streams = draw_samples(model, X, n, mrt_max_len(cfg, L), cfg, int(step))
    b = build_mrt_batch(samples, y)
    R = len(b["flags"])
    s = np.zeros(R, np.float32)
    s[b["flags"] != REFERENCE] = scores.reshape(-1).astype(np.float32)
    dev = model.device
    stats, lens, pairs = pair_stats(b["pool"], b["pairs"], device=dev, return_device=True)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    risk_scale, ref_weight = mrt_scales(cfg["mle_weight"], R, U)
    weight, risk, _ = risk_weights(up(b["first"]), up(s), stats, lens, pairs, up(b["flags"]), cfg["cost"], cfg["alpha"], risk_scale, ref_weight)
    with using_config("train", True):
        loss = model.forward_loss(X=X.repeat_interleave(n + 1, dim=0), y=up(b["y"]), teach_ratio=1.0, random_out=0, label_smoothing=0.0,
                                  row_weight=weight)
        model.cleargrads()
        loss.backward()
        if optimizer is not None:
            optimizer.update()
    return MrtStep(loss=loss, risk=risk, weight=weight, batch=b, scores=s, streams=streams, next_stream=int(step) + U * n)
