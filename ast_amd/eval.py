"""Eval drop-in (eval.py:12-48 of the reference): corpus BLEU-4 of the dev hypotheses against `ref.en<i>` files.

The reference delegates to nltk (`corpus_bleu(..., smoothing_function=SmoothingFunction().method2)`), which is not
installed here; this module restates the published algorithm it calls (Papineni et al. 2002 corpus BLEU; Lin & Och 2004
"add one" smoothing = nltk's method2) so that `train.py`'s per-epoch dev score works offline:
  p_n   = sum over segments of clipped n-gram matches / sum of hypothesis n-gram counts   (micro-average),
  method2: (matches + 1) / (total + 1) for n >= 2,
  BP    = 1 if c > r else exp(1 - r / c), r = sum of the reference lengths closest to each hypothesis (ties: shorter),
  BLEU  = BP * exp(sum_n w_n log p_n); 0 when no unigram matches.

Beside it, not in the reference: the pair statistics of token strings -- edit distance with its substitution /
deletion / insertion counts and the clipped n-gram matches -- from one astk_pair_stats launch (pair_stats) or restated on the host
(edit_stats, clipped_matches), sentence BLEU from those counts (bleu_from_counts) and the word error rate (error_rate, Eval.calc_wer)."""
import math
import os
from collections import Counter

from ._lib import PAIR_MAX_LEN      # astk.h ASTK_PAIR_MAX_LEN: the longest string the device takes


def _ngrams(tokens, n):
    return Counter(tuple(tokens[i:i + n]) for i in range(len(tokens) - n + 1))


def corpus_bleu(list_of_references, hypotheses, weights=(0.25, 0.25, 0.25, 0.25), smooth=True):
    assert len(list_of_references) == len(hypotheses), "one set of references per hypothesis"
    num, den = Counter(), Counter()
    hyp_len = ref_len = 0
    for refs, hyp in zip(list_of_references, hypotheses):
        for n in range(1, len(weights) + 1):
            counts = _ngrams(hyp, n)
            best = Counter()
            for ref in refs:
                for g, c in _ngrams(ref, n).items():
                    if c > best[g]:
                        best[g] = c
            num[n] += sum(min(c, best[g]) for g, c in counts.items())
            den[n] += max(1, sum(counts.values()))
        hyp_len += len(hyp)
        ref_len += min((len(r) for r in refs), key=lambda rl: (abs(rl - len(hyp)), rl))
    if num[1] == 0:
        return 0.0
    logp = 0.0
    for n, w in enumerate(weights, start=1):
        a, b = num[n], den[n]
        if smooth and n > 1:
            a, b = a + 1, b + 1
        if a == 0:
            return 0.0
        logp += w * math.log(a / b)
    bp = 1.0 if hyp_len > ref_len else (0.0 if hyp_len == 0 else math.exp(1.0 - ref_len / hyp_len))
    return bp * math.exp(logp)


def bleu_from_counts(m, hyp_len, ref_len, weights=(0.25, 0.25, 0.25, 0.25), smooth=True):
    """corpus_bleu([[ref]], [hyp]) from the clipped matches m = (m1, .., m4) and the two lengths alone: the same operations in the
    same order (denominators max(1, hyp_len - n + 1), method-2 smoothing, brevity penalty), so the same float bit for bit.  The
    matches are what astk_pair_stats returns (or clipped_matches on the host)."""
    if m[0] == 0:
        return 0.0
    logp = 0.0
    for n, w in enumerate(weights, start=1):
        a, b = int(m[n - 1]), max(1, hyp_len - n + 1)
        if smooth and n > 1:
            a, b = a + 1, b + 1
        if a == 0:
            return 0.0
        logp += w * math.log(a / b)
    bp = 1.0 if hyp_len > ref_len else (0.0 if hyp_len == 0 else math.exp(1.0 - ref_len / hyp_len))
    return bp * math.exp(logp)


# ---- pair statistics (include/astk.h astk_pair_stats): the host restatement and the device call


def edit_stats(a, b):
    """(dist, sub, del, ins) of hypothesis a against reference b under astk_pair_stats' forward rule: the candidates of a cell are
    tried diagonal, deletion (a reference token unmatched), insertion, and a later one wins only if it is strictly cheaper."""
    prev = [(j, 0, j, 0) for j in range(len(b) + 1)]
    for i, x in enumerate(a, start=1):
        row = [(i, 0, 0, i)]
        for j, y in enumerate(b, start=1):
            c, s, d, n = prev[j - 1]
            best = (c, s, d, n) if x == y else (c + 1, s + 1, d, n)
            c, s, d, n = row[j - 1]
            if c + 1 < best[0]:
                best = (c + 1, s, d + 1, n)
            c, s, d, n = prev[j]
            if c + 1 < best[0]:
                best = (c + 1, s, d, n + 1)
            row.append(best)
        prev = row
    return prev[len(b)]


def clipped_matches(a, b):
    """(m1, .., m4): per order the n-grams a and b share, each counted min(count in a, count in b) times -- corpus_bleu's num[n]."""
    out = []
    for n in range(1, 5):
        ca, cb = _ngrams(a, n), _ngrams(b, n)
        out.append(sum(min(c, cb[g]) for g, c in ca.items()))
    return tuple(out)


def pair_stats_host(strings, pairs):
    """astk_pair_stats on the host: one [dist, sub, del, ins, m1, .., m4] per pair (a, b) of indices into strings."""
    return [list(edit_stats(strings[a], strings[b])) + list(clipped_matches(strings[a], strings[b])) for a, b in pairs]


def pair_stats(strings, pairs, device=None, return_device=False):
    """One astk_pair_stats launch over a pool of int token strings (each at most PAIR_MAX_LEN long) and the pairs (a, b) of indices
    into it: a (P, 8) int32 array [dist, sub, del, ins, m1, .., m4].  Needs the GPU: no host fallback behind this name.
    return_device: the device tensors (stats (P, 8), lens (S,), pairs (P, 2)) instead, with nothing read back and so no check of the
    bad-row count -- what astk_risk_weights reads; P must be at least 1."""
    import ctypes
    import numpy as np
    import torch
    from . import _lib
    S, P = len(strings), len(pairs)
    if P == 0:
        if return_device:
            raise ValueError("pair_stats: return_device needs at least one pair")
        return np.zeros((0, 8), np.int32)
    lens = np.asarray([len(s) for s in strings], np.int32)
    if lens.max() > PAIR_MAX_LEN:
        raise ValueError(f"pair_stats: a string of {int(lens.max())} tokens, the device takes at most {PAIR_MAX_LEN}")
    Lmax = max(1, int(lens.max()))
    tokens = np.zeros((S, Lmax), np.int32)
    for i, s in enumerate(strings):
        tokens[i, :len(s)] = s
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("pair_stats needs an MI355X GPU and libastk.so (the host restatement is pair_stats_host)")
    lib = _lib.load()
    with torch.cuda.device(dev):
        t, l = torch.from_numpy(tokens).to(dev), torch.from_numpy(lens).to(dev)
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(P, 2))).to(dev)
        out = torch.empty(P * 8 + 1, dtype=torch.int32, device=dev)            # the statistics, then the count of bad rows
        desc = _lib.PairStatsDesc(S, Lmax, P)
        _lib.check(lib.astk_pair_stats(ctypes.byref(desc), _lib.ptr(t), _lib.ptr(l), _lib.ptr(p), _lib.ptr(out),
                                       ctypes.c_void_p(out.data_ptr() + 4 * P * 8), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        if return_device:
            return out[:-1].view(P, 8), l, p
        host = out.cpu().numpy()
    if host[-1] != 0:
        raise _lib.AstkError(f"pair_stats: {int(host[-1])} of {P} pairs name a string outside the pool")
    return host[:-1].reshape(P, 8)


def dense_ids(sequences):
    """Words (or any hashable tokens) as dense int ids in order of first appearance, one map for all the sequences of a call:
    ([[id, ..], ..], {token: id}).  Equal tokens get equal ids and different tokens different ones, which is all edit distance asks."""
    ids, out = {}, []
    for seq in sequences:
        out.append([ids.setdefault(w, len(ids)) for w in seq])
    return out, ids


def error_rate(list_of_references, hypotheses, device=None):
    """Word (token) error rate of the hypotheses, one set of references per hypothesis: per segment the reference of least edit
    distance (ties: the first) gives S, D, I and its length; {"S", "D", "I", "N", "rate"} with the sums and rate = (S + D + I) / N
    (0.0 when N = 0).  One astk_pair_stats launch over all (hypothesis, reference) pairs on `device` (None: the GPU when there is
    one, else the host restatement edit_stats); a pair with a string longer than PAIR_MAX_LEN tokens goes through the host."""
    assert len(list_of_references) == len(hypotheses), "one set of references per hypothesis"
    if device is None:
        import torch
        use_gpu = torch.cuda.is_available()
    else:
        use_gpu = str(device) != "cpu"
    n_hyp = len(hypotheses)
    pool, _ = dense_ids(list(hypotheses) + [r for refs in list_of_references for r in refs])
    pairs, k = [], n_hyp
    for h, refs in enumerate(list_of_references):
        assert len(refs) >= 1, "a segment without references"
        for _ in refs:
            pairs.append((h, k))
            k += 1
    fits = [use_gpu and max(len(pool[a]), len(pool[b])) <= PAIR_MAX_LEN for a, b in pairs]
    short = [s if len(s) <= PAIR_MAX_LEN else [] for s in pool]              # (no device pair names a longer string)
    on_dev = iter(pair_stats(short, [pr for pr, f in zip(pairs, fits) if f], device)[:, :4].tolist())
    stats = [next(on_dev) if f else list(edit_stats(pool[a], pool[b])) for (a, b), f in zip(pairs, fits)]
    tot = {"S": 0, "D": 0, "I": 0, "N": 0}
    k = 0
    for refs in list_of_references:
        best = min(range(len(refs)), key=lambda r: (stats[k + r][0], r))
        _, s, d, i = stats[k + best]
        tot["S"] += s
        tot["D"] += d
        tot["I"] += i
        tot["N"] += len(refs[best])
        k += len(refs)
    tot["rate"] = (tot["S"] + tot["D"] + tot["I"]) / tot["N"] if tot["N"] else 0.0
    return tot


class Eval:
    def __init__(self, path, n_evals):
        with open(os.path.join(path, "eval.ids"), "r", encoding="utf-8") as f:
            self.ids = [line.strip() for line in f]
        refs = []
        for i in range(n_evals):
            with open(os.path.join(path, "ref.en{0:d}".format(i)), "r", encoding="utf-8") as f:
                refs.append([line.strip().split() for line in f])
        self.refs = list(zip(*refs))

    def calc_bleu(self, hyps):
        return corpus_bleu(self.refs, [hyps[u] for u in self.ids])

    def calc_wer(self, hyps, device=None):
        return error_rate(self.refs, [hyps[u] for u in self.ids], device=device)

    def write_to_file(self, hyps, fname):
        with open(fname, "w", encoding="utf-8") as f:
            for u in self.ids:
                f.write("{0:s}\n".format(" ".join(hyps[u])))
