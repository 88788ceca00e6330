"""CPU tests of minimum-risk training's pure pieces (ast_amd/mrt.py): risk_weights_host against a direct float64
evaluation, the sign and the factor alpha of the weights against finite differences of the expected cost on the float64 oracle,
build_mrt_batch, and every refusal of extras.mrt."""
import json
import random

import numpy as np
import pytest

import risk_model as RM
import row_weight_model as RW
from conftest import tiny_cfg
from oracle import ast_ref as R

CASES = RM.cases()


# ------------------------------------------------------------------ 1. the host model
@pytest.mark.parametrize("cost", RM.COSTS)
@pytest.mark.parametrize("name", list(CASES))
def test_host_model_against_the_direct_evaluation(name, cost):
    case = CASES[name]
    w, risk, c, n_bad = RM.host(case, cost)
    want = RM.direct(case, cost)
    assert n_bad == 0 and w.dtype == risk.dtype == c.dtype == np.float32
    for got, ref, bound, what in zip((w, risk, c), want, RM.bounds(case, want), ("weight", "risk", "cost")):
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= bound).all(), (name, cost, what, err.max())
    assert ((c >= 0) & (c <= (1.0 if cost == "bleu" else np.inf))).all()
    live = ((case["flags"] & 1) != 0) & (case["stats"][:, 0] >= 0)
    assert (c[~live] == 0).all(), "a dead row has cost_out 0"


def test_named_cases_hold_what_their_names_say():
    w, risk, c, _ = RM.host(CASES["far_scores"], "edit")
    assert np.count_nonzero(w) == 0 or np.abs(w).max() < 1e-30, "Q saturates to one row per list: Rbar = its cost, every weight vanishes"
    w, risk, c, _ = RM.host(CASES["alpha0"], "bleu")
    assert w.tolist() == [0, 0, 0, 0.75, 0, 0.75], "alpha 0: only the reference term"
    w, risk, c, _ = RM.host(CASES["no_live"], "bleu")
    assert risk[1] == 0 and w[3:7].tolist() == [0, 0, 0, 0.5]
    assert RM.host(CASES["zero_match"], "bleu")[2][2] == 1.0 and CASES["zero_match"]["stats"][2, 4] == 0
    case = CASES["hyp_len0"]
    assert case["lens"][case["pairs"][4, 0]] == 0 and RM.host(case, "bleu")[2][4] == 1.0 and RM.host(case, "edit")[2][4] == 1.0
    assert len(CASES["full64"]["flags"]) == 64 and np.diff(CASES["ragged"]["first"]).tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert (CASES["bad_stats"]["stats"][1] == -1).all()


@pytest.mark.parametrize("cost", RM.COSTS)
@pytest.mark.parametrize("name", ["two", "ragged", "dead_middle", "bad_stats", "equal_scores", "full64"])
def test_weights_of_a_list_sum_to_zero_without_the_reference_term(name, cost):
    case = dict(CASES[name], ref_weight=0.0)
    w64, _, c64 = RM.direct(case, cost)
    for u in range(len(case["first"]) - 1):
        lo, hi = case["first"][u], case["first"][u + 1]
        scale = abs(case["risk_scale"]) * case["alpha"] * max(c64[lo:hi].max(), 1e-300)
        assert abs(w64[lo:hi].sum()) <= 1e-12 * scale, (name, u, w64[lo:hi].sum())


def test_bad_lists_on_the_host():
    """A list of 65 rows and a descent in the offsets: counted, their rows 0, the neighbours as if they stood alone."""
    a, b, big = RM.make_case([3], seed=20, risk_scale=2.0), RM.make_case([4], seed=21, risk_scale=2.0), RM.make_case([65], seed=22)
    R = 3 + 65 + 4
    cat = lambda k: np.concatenate([a[k], big[k], b[k]])
    lens = cat("lens")
    pairs = np.concatenate([a["pairs"], big["pairs"] + len(a["lens"]), b["pairs"] + len(a["lens"]) + len(big["lens"])])
    first = np.array([0, 3, 68, 72], np.int32)
    w, risk, c, n_bad = R_host(first, cat("score"), cat("stats"), lens, pairs, cat("flags"), fill=9.0)
    assert n_bad == 1 and (w[3:68] == 0).all() and risk[1] == 0
    np.testing.assert_array_equal(w[:3], RM.host(a, "bleu")[0])
    np.testing.assert_array_equal(w[68:], RM.host(b, "bleu")[0])
    # a descent: [0, 3, 2, 72] -- list 1 is (3, 2), list 2 starts below the offset in front of it; both bad, rows 3.. zeroed by list 2
    w, risk, c, n_bad = R_host(np.array([0, 3, 2, R], np.int32), cat("score"), cat("stats"), lens, pairs, cat("flags"), fill=9.0)
    assert n_bad == 2 and (w[3:] == 0).all() and risk[1:].tolist() == [0, 0]
    np.testing.assert_array_equal(w[:3], RM.host(a, "bleu")[0])


def R_host(first, score, stats, lens, pairs, flags, fill):
    from ast_amd import mrt
    return mrt.risk_weights_host(first, score, stats, lens, pairs, flags, "bleu", 1.0, 2.0, 0.0, fill=fill)


# ------------------------------------------------------------------ 2. the sign and the factor alpha
def test_weighted_loss_has_the_gradient_of_the_expected_cost():
    """Three candidate target rows of ONE utterance as three batch rows of the float64 oracle (teacher forcing on every step), costs c and
    alpha = 0.7.  R(theta) = sum_i softmax(alpha s(theta))_i c_i with s_i = -NLL_i, the NLLs from the oracle's loss under the three unit
    weight vectors (times the count B = 3 the oracle divides by).  Its central difference along a direction equals B times the
    directional derivative of the oracle's weighted loss under w = alpha Q (R - c) with Q held fixed, within 1e-6 relative."""
    cfg = tiny_cfg(c1=8)
    D, V, B, L, T = 26, 11, 3, 6, 21
    P = R.init_params(cfg, D, V, seed=3, dtype=np.float64)
    X1, _ = R.synth_batch(1, T, D, L, V, seed=4, dtype=np.float64)
    X = np.repeat(X1, B, axis=0)
    y = np.array([[1, 5, 7, 4, 2, 0], [1, 5, 9, 9, 6, 2], [1, 8, 2, 0, 0, 0]], np.int32)
    c, alpha, h = np.array([0.2, 0.9, 0.5]), 0.7, 1e-5

    def loss(Pd, r):
        with RW.weighted_oracle(0.0, r):
            m = R.RefModel(cfg, {k: v.copy() for k, v in Pd.items()}, V)
            return m, m.forward_loss(X, y, 1.0, pyrandom=random.Random(1))

    def nll(Pd):
        return np.array([B * float(loss(Pd, np.eye(B)[i])[1].data) for i in range(B)])

    def softmax(z):
        e = np.exp(z - z.max())
        return e / e.sum()

    def risk(Pd):
        return float(softmax(-alpha * nll(Pd)) @ c)
    q = softmax(-alpha * nll(P))
    rbar = float(q @ c)
    w = alpha * q * (rbar - c)
    assert (w > 0).any() and (w < 0).any() and abs(w.sum()) < 1e-15
    m, lw = loss(P, w)
    m.cleargrads()
    lw.backward()
    grads = {k: p.grad.copy() for k, p in m.params()}
    rng = np.random.default_rng(5)
    for k in ("out/W", "L1_dec/lateral/W", "L0_enc/upward/W"):
        d = rng.standard_normal(P[k].shape)
        d = d / np.sqrt((d * d).sum()) + grads[k] / np.sqrt((grads[k] ** 2).sum())
        d /= np.sqrt((d * d).sum())
        Pp, Pm = dict(P), dict(P)
        Pp[k], Pm[k] = P[k] + h * d, P[k] - h * d
        num = (risk(Pp) - risk(Pm)) / (2 * h)
        ana = B * float((grads[k] * d).sum())
        print(k, num, ana, abs(num - ana) / abs(ana))
        assert num * ana > 0, "the sign"
        assert abs(num - ana) <= 1e-6 * abs(ana), (k, num, ana)
    # ... and the factor alpha is in the weights: without it the derivative is off by 1 / alpha
    assert abs(num - ana / alpha) > 0.1 * abs(num)


# ------------------------------------------------------------------ 3. build_mrt_batch
def test_build_mrt_batch():
    from ast_amd.mrt import LIVE, REFERENCE, build_mrt_batch
    samples = [[np.array([5, 6, 2, 9, 9]),          # cut behind the first EOS
                np.array([5, 6, 7, 8, 4]),          # no EOS: kept whole
                np.array([5, 6, 2, 2, 0]),          # the first again once cut: a duplicate
                np.array([2, 5, 5, 5, 5])],         # EOS at once: an empty string
               [np.array([4, 0, 6, 2, 0]), np.array([4, 0, 6, 2, 7])]]
    refs = np.array([[1, 5, 6, 2, 0, 0, 0], [1, 4, 6, 8, 9, 7, 2]], np.int32)
    b = build_mrt_batch(samples, refs)
    assert b["y"].dtype == np.int32 and b["y"].shape == (8, 7)
    assert b["y"].tolist() == [[1, 5, 6, 2, 0, 0, 0], [1, 5, 6, 7, 8, 4, 0], [1, 5, 6, 2, 0, 0, 0], [1, 2, 0, 0, 0, 0, 0], [1, 5, 6, 2, 0, 0, 0],
                               [1, 4, 0, 6, 2, 0, 0], [1, 4, 0, 6, 2, 0, 0], [1, 4, 6, 8, 9, 7, 2]]
    assert b["flags"].tolist() == [LIVE, LIVE, 0, LIVE, REFERENCE, LIVE, 0, REFERENCE]
    assert b["first"].tolist() == [0, 5, 8]
    assert b["pool"] == [[5, 6], [5, 6, 7, 8, 4], [5, 6], [], [5, 6], [4, 6], [4, 6], [4, 6, 8, 9, 7], [5, 6], [4, 6, 8, 9, 7]]
    assert b["pairs"].tolist() == [[0, 8], [1, 8], [2, 8], [3, 8], [4, 8], [5, 9], [6, 9], [7, 9]]
    # one short utterance: L is at least 2
    b = build_mrt_batch([[np.array([2])]], np.array([[1, 2]], np.int32))
    assert b["y"].tolist() == [[1, 2], [1, 2]] and b["flags"].tolist() == [LIVE, REFERENCE]


def test_mrt_scales_and_max_len():
    from ast_amd.mrt import checked_mrt, mrt_max_len, mrt_scales
    rs, rw = mrt_scales(0.25, 32, 4)
    assert (rs, rw) == (6.0, 2.0)                    # sum / B of (rs risk rows + rw ref rows) = 0.75 mean R + 0.25 mean NLL(ref)
    cfg = checked_mrt({"samples": 3})
    assert mrt_max_len(cfg, 9) == 18 and mrt_max_len(cfg, 600) == 512 and mrt_max_len(checked_mrt({"max_len": 7}), 9) == 7
    assert checked_mrt(None) is None


# ------------------------------------------------------------------ 4. refusals
def _nn_dir(tmp_path, mrt, extras=None, ctc=False):
    mcfg = tiny_cfg()
    del mcfg["rnn_config"]["dec_vocab_size"]
    if ctc:
        mcfg["rnn_config"]["ctc"] = True
    ex = {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0, "mrt": mrt}
    ex.update(extras or {})
    tcfg = {"seed": "s", "gpuid": 0, "batch_size": 4, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 1,
            "optimizer": {"type": 0, "lr": 1e-3, "l2": 0, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": ex,
            "data": {"dataloader": "synthetic", "vocab_size": 11, "feat_dim": 13, "n_utts": {"syn_train": 4, "syn_dev": 2},
                     "frames": [60, 100], "targets": [2, 5], "buckets_num": 2, "buckets_width": 80, "max_pred": 8,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w"}}
    json.dump(mcfg, open(tmp_path / "model_cfg.json", "w"))
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))
    return str(tmp_path)


@pytest.mark.parametrize("mrt, key", [({"samples": 0}, "samples"), ({"samples": 64}, "samples"), ({"samples": 2.5}, "samples"),
                                      ({"alpha": -0.1}, "alpha"), ({"alpha": float("nan")}, "alpha"), ({"mle_weight": 1.5}, "mle_weight"),
                                      ({"mle_weight": -0.01}, "mle_weight"), ({"cost": "ter"}, "cost"), ({"sample": 3}, "sample"),
                                      ([3], "extras.mrt")], ids=repr)
def test_nn_refuses_a_bad_extras_mrt(mrt, key, tmp_path):
    """extras.mrt is checked when the experiment directory is read, in front of the loader and the model."""
    from ast_amd.nn import NN
    with pytest.raises(ValueError, match="extras.mrt") as e:
        NN(_nn_dir(tmp_path, mrt))
    assert key in str(e.value)


def test_nn_refuses_mrt_with_ctc_random_out_and_data_parallelism(tmp_path, monkeypatch):
    from ast_amd import dist as adist
    from ast_amd.nn import NN
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir(), (tmp_path / "c").mkdir()
    with pytest.raises(ValueError, match="extras.mrt.*ctc_weight"):
        NN(_nn_dir(tmp_path / "a", {"samples": 3}, {"ctc_weight": 0.3}, ctc=True))
    with pytest.raises(ValueError, match="extras.mrt.*random_out"):
        NN(_nn_dir(tmp_path / "b", {"samples": 3}, {"random_out": 0.1}))
    monkeypatch.setattr(adist, "world_size", lambda: 2)
    with pytest.raises(ValueError, match="extras.mrt.*world size 2"):
        NN(_nn_dir(tmp_path / "c", {"samples": 3}))
