"""CPU tests that pin the oracle (it has no reference vectors to lean on -- 'parity unpinned'):
float64 finite differences, an independent torch-autograd restatement, and hand-derivable
known-answer checks for the Chainer semantics listed in SURVEY.md Appendix A / B."""
import random

import numpy as np
import pytest
import torch

from oracle import ast_ref as R
from oracle import minichainer as F
from oracle.ast_ref_torch import forward_loss_torch
from conftest import tiny_cfg


def _setup(dtype=np.float64, drop=0.0, enc_layers=2, dec_layers=2, B=3, T=21, D=26, L=6, V=11, seed=0):
    cfg = tiny_cfg(enc_layers=enc_layers, dec_layers=dec_layers, drop=drop, V=V)
    P = R.init_params(cfg, D, V, seed=seed, dtype=dtype)
    X, y = R.synth_batch(B, T, D, L, V, seed=seed + 1, dtype=dtype)
    return cfg, P, X, y, V


def _loss(cfg, P, X, y, V, teach=1.0, masks=None, noise=None):
    m = R.RefModel(cfg, {k: v.copy() for k, v in P.items()}, V)
    if masks is not None:
        m.masks = masks
    loss = m.forward_loss(X, y, teach, add_noise=0.25 if noise is not None else 0, noise=noise,
                          pyrandom=random.Random("seed-ast-20h"))
    return m, loss


def test_finite_differences_f64():
    cfg, P, X, y, V = _setup()
    m, loss = _loss(cfg, P, X, y, V)
    m.cleargrads()
    loss.backward()
    rng = np.random.default_rng(5)
    for k, p in m.params():
        g = p.grad
        assert g is not None, k
        for _ in range(2):
            idx = tuple(int(rng.integers(0, s)) for s in g.shape)
            eps = 1e-6
            Pp = {n: v.copy() for n, v in P.items()}
            Pm = {n: v.copy() for n, v in P.items()}
            Pp[k][idx] += eps
            Pm[k][idx] -= eps
            num = (float(_loss(cfg, Pp, X, y, V)[1].data) - float(_loss(cfg, Pm, X, y, V)[1].data)) / (2 * eps)
            assert abs(num - g[idx]) <= 1e-6 * max(1.0, abs(num)) + 2e-8, (k, idx, num, g[idx])


@pytest.mark.parametrize("drop,enc_layers,dec_layers,teach", [(0.0, 2, 2, 1.0), (0.3, 3, 1, 0.5), (0.3, 1, 2, 0.8)])
def test_against_independent_torch_restatement(drop, enc_layers, dec_layers, teach):
    cfg, P, X, y, V = _setup(drop=drop, enc_layers=enc_layers, dec_layers=dec_layers, L=7)
    masks = R.RecordingMasks(3) if drop > 0 else None
    noise = np.random.default_rng(9).normal(1.0, 0.25, X.shape) if drop > 0 else None
    m, loss = _loss(cfg, P, X, y, V, teach, masks, noise)
    m.cleargrads()
    loss.backward()
    Pt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=R.is_trainable(k)) for k, v in P.items()}
    lt, enc_t = forward_loss_torch(cfg, Pt, torch.tensor(X), y, m.use_truth, V,
                                   masks=masks.masks if masks else None,
                                   noise=torch.tensor(noise) if noise is not None else None)
    lt.backward()
    assert abs(float(lt.detach()) - float(loss.data)) < 1e-10 * max(1, abs(float(lt.detach())))
    np.testing.assert_allclose(m.enc_states.data, enc_t.detach().numpy(), rtol=1e-10, atol=1e-12)
    for k, p in m.params():
        np.testing.assert_allclose(p.grad, Pt[k].grad.numpy(), rtol=1e-8, atol=1e-11, err_msg=k)


def test_lstm_gate_interleave_A1():
    # unit j gate k lives in column 4j+k; a=tanh, i,f,o = sigmoid
    z = np.zeros((1, 8))
    z[0, 0:4] = [0.5, 100, -100, 100]      # unit 0: a=.5, i->1, f->0, o->1
    z[0, 4:8] = [100, -100, 100, 100]      # unit 1: i->0, f->1: c = c_prev
    c_prev = np.array([[3.0, 0.25]])
    c, h = F.lstm(F.Variable(c_prev), F.Variable(z))
    np.testing.assert_allclose(c.data, [[np.tanh(0.5), 0.25]], atol=1e-12)
    np.testing.assert_allclose(h.data, [[np.tanh(np.tanh(0.5)), np.tanh(0.25)]], atol=1e-12)


def test_softmax_ce_weight_and_denominator_A6():
    x = np.log(np.array([[0.5, 0.25, 0.25], [0.1, 0.2, 0.7], [0.3, 0.3, 0.4]]))
    t = np.array([1, 0, 2])                # middle row is PAD: weight 0 but counted in the denominator
    w = np.array([0.0, 1.0, 1.0])
    xv = F.Variable(x)
    loss = F.softmax_cross_entropy(xv, t, class_weight=w)
    assert abs(float(loss.data) - (-(np.log(0.25) + np.log(0.4)) / 3)) < 1e-12
    loss.backward()
    np.testing.assert_allclose(xv.grad[1], 0, atol=1e-15)
    np.testing.assert_allclose(xv.grad[0], (np.array([0.5, 0.25, 0.25]) - [0, 1, 0]) / 3, atol=1e-12)


def test_reverse_stack_order_Q1():
    """The reverse stack consumes frames 0, T''-1, ..., 1; row p of its half of enc_states is the state
    after frame p+1 (p <= T''-2) and the last row is the state after frame 0 only."""
    cfg, P, X, y, V = _setup(enc_layers=1, dec_layers=1)
    m = R.RefModel(cfg, P, V)
    feats = m.forward_cnn(F.Variable(X))
    m.forward_rnn_encode(feats)
    T2 = feats.shape[0]
    link = F.LSTMLink(*(F.Variable(P[f"L0_rev_enc/{n}"]) for n in ("upward/W", "upward/b", "lateral/W")))
    first = link(F.Variable(feats.data[0])).data
    Hh = cfg["rnn_config"]["hidden_units"] // 2
    np.testing.assert_allclose(m.enc_states.data[:, T2 - 1, Hh:], first, atol=1e-12)
    second = link(F.Variable(feats.data[T2 - 1])).data
    np.testing.assert_allclose(m.enc_states.data[:, T2 - 2, Hh:], second, atol=1e-12)


def test_teacher_forcing_flags_Q4():
    rnd = random.Random("seed-ast-20h")
    flags = R.teacher_flags(8, 0.8, rnd)
    assert len(flags) == 7 and flags[0] and flags[-1]
    rnd2 = random.Random("seed-ast-20h")
    draws = [rnd2.random() < 0.8 for _ in range(5)]
    assert flags[1:6] == draws
    # str seeding is sha512-based and stable across CPython 3.x: pin the first draws
    rnd3 = random.Random("seed-ast-20h")
    assert [rnd3.random() for _ in range(4)] == pytest.approx(
        [0.12586440007881605, 0.06907301332172022, 0.6615765874083718, 0.36126063757535964], abs=1e-15)


def test_hooks_and_amsgrad_A7_A8():
    class M:
        def __init__(self):
            self.p = {"a/W": F.Parameter(np.array([3.0, -4.0])), "b/W": F.Parameter(np.array([12.0]))}

        def params(self):
            return list(self.p.items())
    m = M()
    cfg = {"type": 0, "lr": 0.1, "l2": 0.5, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []}
    opt = R.RefOptimizer(m, cfg)
    m.p["a/W"].grad = np.array([1.5, 2.0])
    m.p["b/W"].grad = np.array([0.0])
    opt.update()
    # decay first: g = [3, 0], [6]; norm = sqrt(45); rate = 2/sqrt(45) < 1 -> clipped
    g = np.array([3.0, 0.0, 6.0]) * (2 / np.sqrt(45))
    assert abs(opt.last_grad_norm - np.sqrt(45)) < 1e-12
    m1, v1 = 0.1 * g, 0.001 * g * g
    lr1 = 0.1 * np.sqrt(1 - 0.999) / (1 - 0.9)
    exp = np.array([3.0, -4.0, 12.0]) - lr1 * m1 / (np.sqrt(v1) + 1e-8)
    np.testing.assert_allclose(np.concatenate([m.p["a/W"].data, m.p["b/W"].data]), exp, rtol=1e-12)
    # second step with a smaller gradient: vhat keeps the max
    m.p["a/W"].grad = np.array([0.0, 0.0])
    m.p["b/W"].grad = np.array([0.0])
    for p in m.p.values():
        p.data[...] = 0
    opt.update()
    st = opt.state["b/W"]
    assert st["vhat"][0] == pytest.approx(v1[2]) and st["v"][0] == pytest.approx(0.999 * v1[2])


@pytest.mark.parametrize("kind", [1, 0])
def test_frozen_parameters_still_count_in_decay_norm_and_clip_A7(kind):
    """Chainer's hooks iterate target.params() whether or not a link's update is enabled; disable_update() only stops the update rule.
    a = [3, 4] frozen, b = [1], gradients equal to the values, l2 = 0, clip = 2: the norm is sqrt(9 + 16 + 1) = sqrt(26) (not 1), the
    clip factor 2 / sqrt(26) = 0.392, and only b moves."""
    class M:
        def __init__(self):
            self.p = {"a/W": F.Parameter(np.array([3.0, 4.0])), "b/W": F.Parameter(np.array([1.0]))}

        def params(self):
            return list(self.p.items())
    m = M()
    opt = R.RefOptimizer(m, {"type": kind, "lr": 0.1, "l2": 0, "grad_clip": 2, "grad_noise_eta": 0, "freeze": ["a"]})
    m.p["a/W"].grad, m.p["b/W"].grad = np.array([3.0, 4.0]), np.array([1.0])
    opt.update()
    r = 2 / np.sqrt(26)
    assert abs(opt.last_grad_norm - np.sqrt(26)) < 1e-12
    assert list(m.p["a/W"].data) == [3.0, 4.0] and "a/W" not in opt.state
    np.testing.assert_allclose(m.p["a/W"].grad, np.array([3.0, 4.0]) * r, rtol=1e-15)      # the hooks did run over the frozen gradient
    if kind == 1:       # SGD: b = 1 - 0.1 * 0.392 = 0.9608
        assert m.p["b/W"].data[0] == pytest.approx(1 - 0.1 * r, abs=1e-15) and abs(m.p["b/W"].data[0] - 0.9608) < 5e-5
    else:               # Adam, first step: m = 0.1 g, v = 0.001 g^2, lr_1 = lr sqrt(0.001) / 0.1 -> a step of lr g / (|g| + eps sqrt(1000))
        g = r
        lr1 = 0.1 * np.sqrt(1 - 0.999) / (1 - 0.9)
        assert m.p["b/W"].data[0] == pytest.approx(1 - lr1 * 0.1 * g / (np.sqrt(0.001 * g * g) + 1e-8), abs=1e-14)
        assert opt.state["b/W"]["vhat"][0] == pytest.approx(0.001 * g * g, rel=1e-12)
    # with a decay: the frozen weights feed the norm through l2 * p as well
    m2 = M()
    opt2 = R.RefOptimizer(m2, {"type": kind, "lr": 0.1, "l2": 1.0, "grad_clip": 2, "grad_noise_eta": 0, "freeze": ["a"]})
    m2.p["a/W"].grad, m2.p["b/W"].grad = np.array([0.0, 0.0]), np.array([0.0])
    opt2.update()
    assert abs(opt2.last_grad_norm - np.sqrt(26)) < 1e-12


def test_batchnorm_train_and_running_stats_A4():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 3, 4, 5)) * 2 + 1
    bn = F.BatchNormState(F.Parameter(np.ones(3)), F.Parameter(np.zeros(3)), np.zeros(3), np.ones(3))
    y = bn(F.Variable(x), train=True)
    np.testing.assert_allclose(y.data.mean(axis=(0, 2, 3)), 0, atol=1e-12)
    m = 2 * 4 * 5
    np.testing.assert_allclose(bn.avg_var, 0.9 + 0.1 * x.var(axis=(0, 2, 3)) * m / (m - 1), rtol=1e-12)
    np.testing.assert_allclose(bn.avg_mean, 0.1 * x.mean(axis=(0, 2, 3)), rtol=1e-12)
    xt = torch.tensor(x)
    yt = torch.nn.functional.batch_norm(xt, None, None, torch.ones(3, dtype=torch.float64),
                                        torch.zeros(3, dtype=torch.float64), training=True, eps=2e-5)
    np.testing.assert_allclose(y.data, yt.numpy(), atol=1e-12)


def test_train_step_reports_loss_over_batch_Q5():
    cfg, P, X, y, V = _setup(dtype=np.float32)
    m = R.RefModel(cfg, {k: v.copy() for k, v in P.items()}, V)
    opt = R.RefOptimizer(m, {"type": 0, "lr": 1e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []})
    before = m.p["out/W"].data.copy()
    loss, rep = R.train_step(m, opt, X, y, 0.8, pyrandom=random.Random("seed-ast-20h"))
    assert rep == pytest.approx(loss / len(y))
    assert opt.last_grad_norm > 0 and not np.allclose(before, m.p["out/W"].data)
    assert m.p["out/W"].data.dtype == np.float32


# ----------------------------------------------------------------------------------------------------------------------------------
# Optional model features of the NEW path (seq2seq.py:43-57, 81-121, 244-291, 369-394, 456-465)
def _opt_cfg(**kw):
    """tiny_cfg with rnn_config / cnn_config / dropout options switched on."""
    cfg = tiny_cfg(enc_layers=kw.pop("enc_layers", 2), dec_layers=kw.pop("dec_layers", 2), drop=kw.pop("drop", 0.0), V=kw.pop("V", 11))
    for k in ("ln", "linear_proj", "n_attn", "feed_attn"):
        if k in kw:
            cfg["rnn_config"][k] = kw.pop(k)
    if "bn" in kw:
        cfg["cnn_config"]["bn"] = kw.pop("bn")
    if "out" in kw:
        cfg["dropout"]["out"] = kw.pop("out")
    assert not kw, kw
    return cfg


OPTION_SETS = {
    "ln": dict(ln=True),
    "ln-drop": dict(ln=True, drop=0.3, enc_layers=3, dec_layers=1),
    "n_attn3": dict(n_attn=3),
    "no-feed": dict(feed_attn=False),
    "no-bn": dict(bn=False),
    "out-drop": dict(out=0.4, drop=0.2),
    "proj": dict(linear_proj=True, enc_layers=3),
    "proj-drop": dict(linear_proj=True, enc_layers=2, drop=0.3),
    "all": dict(ln=True, n_attn=2, feed_attn=False, bn=False, out=0.3, drop=0.2, enc_layers=2, dec_layers=3),
}


@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_option_sets_pass_finite_differences_f64(name):
    """Every optional feature's backward in the define-by-run oracle against float64 central differences of its own forward pass
    (dropout masks replayed, teacher forcing mixed): two entries of every parameter."""
    cfg = _opt_cfg(**OPTION_SETS[name])
    V, D, B, T, L = 11, 26, 3, 21, 6
    P = R.init_params(cfg, D, V, seed=3, dtype=np.float64)
    rng = np.random.default_rng(11)
    for k in P:                                    # away from the initial gamma = 1 / beta = 0 / b = 0, which hide mistakes
        if k.endswith(("gamma", "beta", "/b")) and "upward" not in k:
            P[k] = P[k] + 0.3 * rng.standard_normal(P[k].shape)
    X, y = R.synth_batch(B, T, D, L, V, seed=4, dtype=np.float64)
    drop = max(cfg["dropout"].values()) > 0
    rec = R.RecordingMasks(5) if drop else None

    class Replay:
        def __call__(self, shape, ratio, tag):
            return rec.masks[tag]

    def run(Pv, masks):
        m = R.RefModel(cfg, {k: v.copy() for k, v in Pv.items()}, V)
        if masks is not None:
            m.masks = masks
        loss = m.forward_loss(X, y, 0.5, pyrandom=random.Random(2))
        return m, loss
    m, loss = run(P, rec)
    flags = list(m.use_truth)
    assert not all(flags), "the case should feed back its own argmax at some step"
    m.cleargrads()
    loss.backward()
    unreached = []
    for k, p in m.params():
        # (a parameter the loss does not depend on keeps grad None, like Chainer's; the optimizer treats it as zeros: with linear_proj the
        #  top encoder layer matters only through the final states that seed a decoder layer of the same index)
        g = p.grad if p.grad is not None else np.zeros_like(p.data)
        if p.grad is None:
            unreached.append(k)
        for _ in range(2):
            idx = tuple(int(rng.integers(0, s)) for s in g.shape)
            eps = 1e-6
            Pp = {n: v.copy() for n, v in P.items()}
            Pm = {n: v.copy() for n, v in P.items()}
            Pp[k][idx] += eps
            Pm[k][idx] -= eps
            num = (float(run(Pp, Replay() if drop else None)[1].data) - float(run(Pm, Replay() if drop else None)[1].data)) / (2 * eps)
            assert abs(num - g[idx]) <= 2e-6 * max(1.0, abs(num)) + 5e-8, (k, idx, num, g[idx])
    assert all(k.startswith(("L2_enc", "L2_rev_enc")) for k in unreached) and (name == "proj") == bool(unreached), unreached


def test_layer_normalization_known_answer():
    """L.LayerNormalization: per-ROW statistics over the units, biased variance, eps = 1e-6 inside the square root, then gamma / beta."""
    x = np.array([[1.0, 2.0, 3.0, 6.0], [0.0, 0.0, 0.0, 0.0]])
    g, b = np.array([1.0, 2.0, 0.5, -1.0]), np.array([0.1, 0.0, -0.2, 0.3])
    y = F.layer_normalization(F.Variable(x), F.Variable(g), F.Variable(b), 1e-6).data
    mu, var = 3.0, (4 + 1 + 0 + 9) / 4.0
    want0 = (x[0] - mu) / np.sqrt(var + 1e-6) * g + b
    np.testing.assert_allclose(y[0], want0, atol=1e-14)
    np.testing.assert_allclose(y[1], b, atol=1e-14)            # a constant row normalises to 0 (eps keeps it finite)


def test_layernorm_sits_behind_dropout_and_leaves_the_recurrent_state_raw():
    """seq2seq.py:198-202: hs = LN(dropout(LSTM(hs))); the link's own h (next step's lateral input, decoder seed) stays un-normalised."""
    cfg = _opt_cfg(ln=True, enc_layers=1, dec_layers=1)
    V, D = 11, 26
    P = R.init_params(cfg, D, V, seed=0, dtype=np.float64)
    P["L0_enc_ln/gamma"] = P["L0_enc_ln/gamma"] * 1.7
    P["L0_enc_ln/beta"] = P["L0_enc_ln/beta"] + 0.2
    X, _ = R.synth_batch(2, 21, D, 5, V, seed=1, dtype=np.float64)
    m = R.RefModel(cfg, P, V)
    m.encode(X)
    h_raw = m.enc[0].h.data                                     # state after the last frame
    Hh = cfg["rnn_config"]["hidden_units"] // 2
    mu = h_raw.mean(1, keepdims=True)
    want = (h_raw - mu) / np.sqrt(((h_raw - mu) ** 2).mean(1, keepdims=True) + 1e-6) * 1.7 + 0.2
    np.testing.assert_allclose(m.enc_states.data[:, -1, :Hh], want, atol=1e-12)
    assert abs(h_raw).max() < 1.0                               # raw LSTM output, |h| < 1


def test_linear_proj_encoder_quirks():
    """seq2seq.py:244-291 as written: (i) the reverse stack sees the LAST frame of its layer's input at every step; (ii) the attention
    memory is the last PROJECTION's output, not the top LSTM layer's; (iii) the projection's BatchNorm normalises each time step over
    its B rows and advances its running statistics and N once per step."""
    cfg = _opt_cfg(linear_proj=True, enc_layers=2, dec_layers=1)
    V, D, B = 11, 26, 3
    H = cfg["rnn_config"]["hidden_units"]
    P = R.init_params(cfg, D, V, seed=0, dtype=np.float64)
    assert P["L1_enc/upward/W"].shape == (4 * (H // 2), H) and P["enc_proj0/W"].shape == (H, H) and "enc_proj1/W" not in P
    X, _ = R.synth_batch(B, 21, D, 5, V, seed=1, dtype=np.float64)
    m = R.RefModel(cfg, {k: v.copy() for k, v in P.items()}, V)
    feats = m.forward_cnn(F.Variable(X))
    m.forward_rnn_encode_proj(feats)
    T2 = feats.shape[0]
    assert m.enc_states.shape == (B, T2, H)
    # (i) layer-0 reverse stack: T2 steps on the constant input feats[-1]
    link = F.LSTMLink(*(F.Variable(P[f"L0_rev_enc/{n}"]) for n in ("upward/W", "upward/b", "lateral/W")))
    outs = [link(F.Variable(feats.data[-1])).data for _ in range(T2)]
    fwd = F.LSTMLink(*(F.Variable(P[f"L0_enc/{n}"]) for n in ("upward/W", "upward/b", "lateral/W")))
    fo = [fwd(F.Variable(feats.data[i])).data for i in range(T2)]
    # (ii) + (iii): enc_states[:, i] = relu(BN_step(Linear([fwd_i ; rev_{T2-1-i}]))) with the statistics of that step's B rows
    for i in (0, 3, T2 - 1):
        z = np.concatenate([fo[i], outs[T2 - 1 - i]], 1) @ P["enc_proj0/W"].T + P["enc_proj0/b"]
        zn = (z - z.mean(0)) / np.sqrt(z.var(0) + 2e-5)
        np.testing.assert_allclose(m.enc_states.data[:, i], np.maximum(zn, 0), atol=1e-10)
    assert m.bn["enc_proj0_bn"].N == T2
    # running mean after T2 sequential updates of decay 0.9
    means = [(np.concatenate([fo[i], outs[T2 - 1 - i]], 1) @ P["enc_proj0/W"].T + P["enc_proj0/b"]).mean(0) for i in range(T2)]
    avg = np.zeros(H)
    for mu in means:
        avg = 0.9 * avg + 0.1 * mu
    np.testing.assert_allclose(m.p["enc_proj0_bn/avg_mean"], avg, atol=1e-12)
    # the top layer reaches the decoder through its final states only
    m.init_decoder_state()
    assert m.dec[0].h.shape == (B, H)


def test_multiple_attention_heads_share_h_and_widen_the_context_layer():
    cfg = _opt_cfg(n_attn=3, enc_layers=1, dec_layers=1)
    V, D = 11, 26
    H, A = cfg["rnn_config"]["hidden_units"], cfg["rnn_config"]["attn_units"]
    P = R.init_params(cfg, D, V, seed=0, dtype=np.float64)
    assert P["context/W"].shape == (A, 4 * H) and P["attn_Wa2/W"].shape == (H, H)
    X, y = R.synth_batch(2, 21, D, 5, V, seed=1, dtype=np.float64)
    m = R.RefModel(cfg, P, V)
    m.train = False
    m.encode(X)
    m.init_decoder_state()
    logits, ht, alphas = m.decode_step(np.array([1, 1], dtype=np.int32), F.Variable(np.zeros((2, A))))
    h = m.dec[0].h.data
    enc = m.enc_states.data
    cvs = []
    for name in ("attn_Wa", "attn_Wa1", "attn_Wa2"):
        q = h @ P[name + "/W"].T + P[name + "/b"]
        s = np.einsum("bth,bh->bt", enc, q)
        a = np.exp(s - s.max(1, keepdims=True))
        a /= a.sum(1, keepdims=True)
        cvs.append(np.einsum("bt,bth->bh", a, enc))
        if name == "attn_Wa":
            np.testing.assert_allclose(alphas.data[:, :, 0], a, atol=1e-12)       # the returned alphas are the FIRST head's
    want = np.tanh(np.concatenate(cvs + [h], 1) @ P["context/W"].T + P["context/b"])
    np.testing.assert_allclose(ht.data, want, atol=1e-12)


def test_random_out_draw_order_and_clamp_Q8():
    """seq2seq.py:456-465: per step, BEHIND the teacher-forcing coin of that step, one random.random() per target >= 4 (none for special
    symbols), replacement when the draw is ABOVE random_out, id from randint(4, V + 1) -- clamped here to V - 1 (the one deviation)."""
    cfg = _opt_cfg(enc_layers=1, dec_layers=1)
    V, D, B, L = 11, 26, 3, 6
    P = R.init_params(cfg, D, V, seed=0, dtype=np.float64)
    X, y = R.synth_batch(B, 21, D, L, V, seed=1, dtype=np.float64)
    draws = iter([V, 4, 7, V, 5, 6, 9, 8, 4, 4, 4, 4, 4, 4, 4])           # V is the out-of-range id the reference can draw
    m = R.RefModel(cfg, P, V)
    rnd = random.Random(7)
    m.forward_loss(X, y, 0.5, random_out=0.4, pyrandom=rnd, randint=lambda lo, hi: next(draws))
    # replay the stream by hand
    rnd2 = random.Random(7)
    drawn = iter([V, 4, 7, V, 5, 6, 9, 8, 4, 4, 4, 4, 4, 4, 4])
    for i in range(L - 1):
        if 0 < i < L - 2:
            rnd2.random()
        want = y[:, i + 1].copy()
        for b in range(B):
            if want[b] >= 4 and rnd2.random() > 0.4:
                want[b] = min(next(drawn), V - 1)
        np.testing.assert_array_equal(m.targets[i], want)
    assert max(int(t.max()) for t in m.targets) == V - 1
    assert rnd.random() == rnd2.random()                                   # same number of draws consumed


@pytest.mark.parametrize("shape,k", [((2, 3, 7, 6), (2, 2)), ((1, 2, 5, 3), (3, 2)), ((2, 2, 4, 1), (4, 1)), ((1, 1, 9, 6), (1, 6))])
def test_max_pooling_nd_cover_all_against_torch(shape, k):
    """The old path's F.max_pooling_nd(h, (time_pool, freq_pool)) (enc_dec.py:456): stride = window, cover_all -- out = ceil(in / k), ragged
    last windows; torch's max_pool2d(ceil_mode=True) is the same operator.  Forward, and the gradient's routing to the window's maximum."""
    rng = np.random.default_rng(4)
    x = rng.standard_normal(shape)
    v = F.Variable(x.copy())
    y = F.max_pooling_nd(v, k)
    xt = torch.tensor(x, requires_grad=True)
    yt = torch.nn.functional.max_pool2d(xt, k, stride=k, ceil_mode=True)
    assert y.shape == tuple(yt.shape) == (shape[0], shape[1], -(-shape[2] // k[0]), -(-shape[3] // k[1]))
    np.testing.assert_array_equal(y.data, yt.detach().numpy())
    gy = rng.standard_normal(y.shape)
    y.grad = gy
    y.backward()
    yt.backward(torch.tensor(gy))
    np.testing.assert_array_equal(v.grad, xt.grad.numpy())


def test_cnn_pool_changes_the_lstm_input_width_and_passes_finite_differences():
    """cnn_pool = [[time, freq], ...] per layer, -1 = the whole extent (enc_dec.py:444-451); the pooled frequency bins set the encoder
    LSTMs' input width (C_last * F'), and the whole model still passes float64 finite differences."""
    cfg = tiny_cfg(enc_layers=1, dec_layers=1, V=11)
    cfg["cnn_config"]["cnn_pool"] = [[2, 2], [1, -1]]
    D = 80                                            # 6 frequency bins behind layer 0 -> 3 behind its pool -> 1
    P = R.init_params(cfg, D, 11, seed=0, dtype=np.float64)
    c_last = cfg["cnn_config"]["cnn_layers"][-1]["out_channels"]
    assert P["L0_enc/upward/W"].shape[1] == c_last * 1
    X, y = R.synth_batch(2, 40, D, 5, 11, seed=1, dtype=np.float64)
    m, loss = _loss(cfg, P, X, y, 11)
    assert m.enc_states.shape[1] == 5                # 40 frames -> 20 (conv) -> 10 (pool 2) -> 5 (conv)
    m.cleargrads()
    loss.backward()
    rng = np.random.default_rng(0)
    for name in ("CNN_0/W", "CNN_1/W", "CNN_0_bn/gamma", "L0_enc/upward/W"):
        g = dict(m.params())[name].grad
        for _ in range(3):
            idx = tuple(rng.integers(0, s) for s in g.shape)
            eps = 1e-6
            Pp, Pm = {k: v.copy() for k, v in P.items()}, {k: v.copy() for k, v in P.items()}
            Pp[name][idx] += eps
            Pm[name][idx] -= eps
            fd = (float(_loss(cfg, Pp, X, y, 11)[1].data) - float(_loss(cfg, Pm, X, y, 11)[1].data)) / (2 * eps)
            assert abs(fd - g[idx]) <= 1e-5 * max(abs(fd), 1e-3), (name, idx, fd, g[idx])
