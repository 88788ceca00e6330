"""Truncated sampling (top-k, then top-p among the survivors), host side: the pick function of the per-step fallback
(ast_amd.seq2seq.truncated_pick) and the NumPy restatement of the contract (tests/truncation_model.py) against known answers and against
each other, the distribution of the draws, the argument checks of sample(), sample.py's flags and the stream numbering.  No GPU.
Every test prints its figures before it asserts."""
import types

import numpy as np
import pytest
import torch

from sample_noise_model import noise as _noise, row_key as _row_key
from truncation_model import draw_from as _draw_from

# the 0.999 quantile of the chi-square law, by degrees of freedom (1..15)
CHI2_999 = [10.828, 13.816, 16.266, 18.467, 20.515, 22.458, 24.322, 26.124, 27.877, 29.588, 31.264, 32.909, 34.528, 36.123, 37.697]


def _pick(lg, g, inv_temp, top_k, top_p):
    from ast_amd.seq2seq import truncated_pick
    tok, logp, kept = truncated_pick(torch.from_numpy(np.asarray(lg, dtype=np.float32)), torch.from_numpy(np.asarray(g, dtype=np.float32)),
                                     inv_temp, top_k, top_p)
    assert tok.dtype == torch.int32 and logp.dtype == torch.float64 and kept.dtype == torch.int32
    return tok.numpy(), logp.numpy(), kept.numpy()


def _both(lg, g, top_k, top_p, inv_temp=1.0):
    """The package's pick function and the restatement on the same float32 logits and noise: they agree, and the answer is returned."""
    lg = np.asarray(lg, dtype=np.float32)
    g = np.asarray(g, dtype=np.float32)
    tok, logp, kept = _pick(lg, g, inv_temp, top_k, top_p)
    xs = (lg * np.float32(inv_temp)).astype(np.float64)
    rt, rl, rm, gap = _draw_from(xs, g.astype(np.float64), top_k, top_p)
    assert (tok == rt).all() and (kept == rm).all() and np.abs(logp - rl).max() <= 1e-12, (tok, rt, kept, rm, logp, rl)
    return tok, logp, kept, gap


def test_known_answers_of_the_pick_function():
    p = np.array([[0.5, 0.2, 0.15, 0.1, 0.05]])
    lg = np.log(p)
    zero = np.zeros_like(lg)
    # top_k = 4: the survivors renormalise to 0.526, 0.737, 0.895, 1 -- top_p = 0.8 keeps 3, top_p = 1 keeps 4
    cum = np.cumsum(p[0, :4] / p[0, :4].sum())
    print("renormalised prefix sums of the top 4:", np.round(cum, 3).tolist())
    assert np.round(cum[:3], 3).tolist() == [0.526, 0.737, 0.895]
    tok, logp, kept, _ = _both(lg, zero, 4, 0.8)
    print(f"top_k 4 top_p 0.8: kept {kept[0]}, token {tok[0]}, logp {logp[0]:.6f}")
    assert kept[0] == 3 and tok[0] == 0 and abs(logp[0] - np.log(0.5 / 0.85)) <= 1e-6
    tok, logp, kept, _ = _both(lg, zero, 4, 1.0)
    assert kept[0] == 4 and abs(logp[0] - np.log(0.5 / 0.95)) <= 1e-6
    # noise moves the draw inside the kept set only: +10 on class 3 wins among 4 kept, but not when the nucleus has cut it
    g = np.array([[0.0, 0.0, 0.0, 10.0, 10.0]])
    tok, logp, kept, _ = _both(lg, g, 4, 1.0)
    assert tok[0] == 3 and abs(logp[0] - np.log(0.1 / 0.95)) <= 1e-6
    tok, logp, kept, _ = _both(lg, g, 4, 0.8)
    assert tok[0] == 0 and kept[0] == 3
    # top_k = 1: the argmax whatever the noise, logp exactly 0
    for top_p in (1.0, 0.3):
        tok, logp, kept, _ = _both(lg, g, 1, top_p)
        print(f"top_k 1 top_p {top_p}: token {tok[0]}, logp {logp[0]!r}, kept {kept[0]}")
        assert tok[0] == 0 and logp[0] == 0.0 and kept[0] == 1
    # top_p just below / above a prefix sum moves m by one
    for j in range(3):
        lo = _both(lg, zero, 4, float(cum[j]) - 1e-6)[2][0]
        hi = _both(lg, zero, 4, float(cum[j]) + 1e-6)[2][0]
        print(f"top_p around prefix sum {j} ({cum[j]:.6f}): kept {lo} below, {hi} above")
        assert lo == j + 1 and hi == j + 2
    # the temperature scales the logits before everything else: at inv_temp = 2 the top 4 are 0.25, 0.04, 0.0225, 0.01 (renormalised)
    tok, logp, kept, _ = _both(lg, zero, 4, 0.8, inv_temp=2.0)
    assert kept[0] == 2 and abs(logp[0] - np.log(0.25 / 0.29)) <= 1e-6


def test_equal_logits_keep_the_lower_id():
    # across the k boundary: classes 1, 2, 3 tie for the places 2 and 3 of top_k = 3 -> ids 1 and 2 are candidates, 3 is not
    lg = np.array([[2.0, 1.0, 1.0, 1.0, 0.0]])
    g = np.array([[0.0, 0.0, 0.0, 50.0, 0.0]])
    tok, _, kept, gap = _both(lg, g, 3, 1.0)
    print(f"tie across the k boundary: token {tok[0]}, kept {kept[0]}, guard gap {gap[0]}")
    assert tok[0] == 0 and kept[0] == 3 and gap[0] == 0.0            # (the guard sees the tie)
    g = np.array([[0.0, 0.0, 50.0, 50.0, 0.0]])
    assert _both(lg, g, 3, 1.0)[0][0] == 2
    # across the nucleus boundary: p = (0.4, 0.2, 0.2, 0.2), top_p = 0.55 keeps 2 -> ids 0 and 1
    lg = np.log(np.array([[0.4, 0.2, 0.2, 0.2]]))
    g = np.array([[0.0, 0.0, 50.0, 50.0]])
    tok, _, kept, _ = _both(lg, g, 4, 0.55)
    print(f"tie across the nucleus boundary: token {tok[0]}, kept {kept[0]}")
    assert kept[0] == 2 and tok[0] == 0
    g = np.array([[0.0, 50.0, 50.0, 50.0]])
    assert _both(lg, g, 4, 0.55)[0][0] == 1
    # equal z among the kept: the lower token id wins, whatever the candidates' order
    lg = np.array([[1.0, 3.0, 2.0, 0.0]])
    g = np.array([[4.0, 2.0, 3.0, 0.0]])             # z = 5, 5, 5, 0 with candidates ordered 1, 2, 0
    assert _both(lg, g, 3, 1.0)[0][0] == 0


@pytest.mark.parametrize("top_p", [1.0, 0.6])
def test_truncated_draws_follow_the_renormalised_kept_distribution(top_p):
    """20000 streams' draws at one step on a fixed 57-class row with top_k = 8: chi-square against the renormalised kept distribution
    below the 0.999 quantile of its degrees of freedom, and no draw outside the kept set."""
    x = (np.random.default_rng(1).standard_normal(57) * 2).astype(np.float32)
    n_draws, K = 20000, 8
    keys = np.array([_row_key(2024, st) for st in range(n_draws)], dtype=np.uint64)
    g = _noise(keys[:, None], 3, np.arange(57)[None, :])[2]
    lg = np.broadcast_to(x, (n_draws, 57)).copy()
    tok, logp, kept = _pick(lg, g, 1.0, K, top_p)
    rt, rl, rm, gap = _draw_from(lg.astype(np.float64), g, K, top_p)
    clear = gap >= 1e-4
    print(f"\ntop_p {top_p}: package and restatement agree at {(tok == rt).mean():.5f} of the draws ({clear.mean():.5f} guarded at 1e-4)")
    assert (tok[clear] == rt[clear]).all() and (kept == rm).all() and np.abs(logp - rl)[clear].max() <= 1e-9
    order = np.argsort(-x.astype(np.float64), kind="stable")
    m = int(kept[0])
    assert (kept == m).all() and 1 <= m <= K
    ids = order[:m]
    p = np.exp(x[ids].astype(np.float64) - float(x[ids[0]]))
    p /= p.sum()
    counts = np.bincount(tok, minlength=57).astype(np.float64)
    outside = int(counts.sum() - counts[ids].sum())
    print(f"kept {m} of top_k {K}: ids {ids.tolist()}, renormalised p {np.round(p, 4).tolist()}, draws outside the kept set {outside}")
    assert outside == 0
    pos = {int(t): j for j, t in enumerate(ids)}
    assert np.abs(logp - np.log(p)[[pos[int(t)] for t in tok]]).max() <= 1e-6          # logp under the distribution actually sampled
    if top_p < 1.0:
        full = np.exp(x[order[:K]].astype(np.float64) - float(x[order[0]]))
        cum = np.cumsum(full / full.sum())
        assert cum[m - 1] >= top_p and (m == 1 or cum[m - 2] < top_p)
    expect = p * n_draws
    small = expect < 5
    obs, exp_ = counts[ids][~small], expect[~small]
    if small.any():
        obs, exp_ = np.append(obs, counts[ids][small].sum()), np.append(exp_, expect[small].sum())
    dof = len(exp_) - 1
    if dof == 0:
        return
    chi2 = float(((obs - exp_) ** 2 / exp_).sum())
    print(f"chi-square {chi2:.2f} with {dof} degrees of freedom ({int(small.sum())} classes pooled), 0.999 quantile {CHI2_999[dof - 1]}")
    assert chi2 < CHI2_999[dof - 1]


def test_argument_checks_fire_before_any_library_call(monkeypatch):
    from ast_amd import _lib, seq2seq
    from ast_amd.seq2seq import SpeechEncoderDecoder, checked_truncation

    def no_library(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(seq2seq._lib, "load", no_library)
    m = SpeechEncoderDecoder.__new__(SpeechEncoderDecoder)
    m.V = 57
    X = np.zeros((1, 8, 4), dtype=np.float32)
    bad = [(dict(top_p=0.9), "top_k <= 16"), (dict(top_k=0), "top_k"), (dict(top_k=17), "top_k"), (dict(top_k=-1), "top_k"),
           (dict(top_k=2.5), "top_k"), (dict(top_k=True), "top_k"), (dict(top_k=16, top_p=0.0), "top_p"), (dict(top_k=5, top_p=-0.1), "top_p"),
           (dict(top_k=5, top_p=1.5), "top_p"), (dict(top_k=5, top_p=float("nan")), "top_p"), (dict(top_k=5, top_p=float("inf")), "top_p"),
           (dict(top_k=5, top_p=None), "top_p")]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word) as e:
            m.sample(X, 1, 2, 10, 0, **kw)
        print(kw, "->", e.value)
    m.V = 7
    with pytest.raises(ValueError, match="above the vocabulary"):
        m.sample(X, 1, 2, 10, 0, top_k=8)
    with pytest.raises(ValueError, match="nucleus is taken among top_k <= 16"):
        m.sample_async(X, 1, 2, 10, 0, top_p=0.5)
    # what passes: the untruncated default, and values as the library takes them
    assert checked_truncation(None, 1.0) == (None, 1.0) and checked_truncation(None, 1) == (None, 1.0)
    assert checked_truncation(16, 1.0, 57) == (16, 1.0) and checked_truncation(np.int64(3), 0.6) == (3, float(np.float32(0.6)))
    # ... and a valid truncated call gets past the checks, to the library
    with pytest.raises(AssertionError, match="the library was reached"):
        m.sample(X, 1, 2, 10, 0, top_k=5, top_p=0.9)


def test_sample_py_parses_the_new_flags():
    import sample
    a = sample.build_parser().parse_args("-m cfg -s dev -n 6 -t 0.8 --top-k 5 --top-p 0.9".split())
    assert a.top_k == 5 and a.top_p == 0.9
    a = sample.build_parser().parse_args("-m cfg -s dev -n 6 -k 16 -p 0.25".split())
    assert a.top_k == 16 and a.top_p == 0.25
    a = sample.build_parser().parse_args("-m cfg -s dev -n 6".split())
    assert a.top_k is None and a.top_p == 1.0
    # the default name gains a suffix only when truncation is on
    assert sample.default_name("dev", 6, 0.8) == "dev_sample_N-6_T-0.80.p"
    assert sample.default_name("dev", 6, 0.8, 5, 0.9) == "dev_sample_N-6_T-0.80_K-5_P-0.90.p"
    assert sample.default_name("dev", 6, 1.0, 5, 1.0) == "dev_sample_N-6_T-1.00_K-5_P-1.00.p"


def test_stream_numbering_is_unchanged_by_truncation():
    """sample_hypotheses_packed / sample_hypotheses hand the same rows the same streams with and without truncation, and pass top_k /
    top_p through; plan_row_packs does not see them."""
    from ast_amd import nn as gnn
    from ast_amd.seq2seq import ScoredPrediction
    calls = []

    class Fake:
        def _as_input(self, X):
            return torch.as_tensor(X)

        def encode_rows(self, Xs, rows_of):
            return types.SimpleNamespace(B=len(rows_of))

        def sample(self, X, go, eos, stop, seed, streams=None, temperature=1.0, rows=None, top_k=None, top_p=1.0):
            streams = list(streams)
            calls.append((streams, top_k, top_p))
            B = len(streams)
            return ScoredPrediction(np.full((B, 2), 5, np.int32), np.zeros((B, 2), np.float32), None, eos)
    Xs = [np.zeros((1, 4, 3), np.float32)] * 4
    plan = gnn.plan_row_packs([12] * 4, 3)
    gnn.sample_hypotheses_packed(Fake(), Xs, 12, 5, 0, max_utts=3)
    plain, calls[:] = list(calls), []
    gnn.sample_hypotheses_packed(Fake(), Xs, 12, 5, 0, max_utts=3, top_k=5, top_p=0.9)
    print("calls:", [(len(s), s[0], s[-1], k, p) for s, k, p in calls])
    assert gnn.plan_row_packs([12] * 4, 3) == plan and len(calls) == len(plan)
    assert [c[0] for c in calls] == [c[0] for c in plain] and all(c[1:] == (None, 1.0) for c in plain) and all(c[1:] == (5, 0.9) for c in calls)
    assert sorted(s for c in calls for s in c[0]) == list(range(48))
    calls[:] = []
    gnn.sample_hypotheses(Fake(), Xs[0], 40, 5, 0, first_stream=7, top_k=3)
    assert [c[0] for c in calls] == [list(range(7, 39)), list(range(39, 47))] and all(c[1:] == (3, 1.0) for c in calls)
