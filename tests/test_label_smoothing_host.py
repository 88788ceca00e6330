"""CPU tests of the label-smoothing feature: the float64 model of tests/label_smoothing_model.py against torch, the
float64 oracle with the model swapped in against finite differences, and the argument checks of the Python surface and the C ABI mirror."""
import ctypes as C
import json
import random

import numpy as np
import pytest
import torch

import label_smoothing_model as LS
from conftest import tiny_cfg
from oracle import ast_ref as R


# ------------------------------------------------------------------ 1. the model against torch
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("V", [1, 5, 257])
def test_model_is_the_weight_free_torch_loss_times_the_target_weight(V, eps):
    """rows = cross_entropy(reduction="none", label_smoothing=eps) * w[t] / B in float64, the gradient by autograd; row 0's target has
    class weight 0 (loss row and gradient row exactly 0) and row 1's target id is V (clamped to V - 1)."""
    rng = np.random.default_rng(V)
    B = 6
    x = rng.standard_normal((B, V)) * 4
    t = rng.integers(0, V, B)
    w = rng.random(V) + 0.5
    t[0], w[0] = 0, 0.0
    if V > 1:
        t[2:] = np.maximum(t[2:], 1)
    t[1] = V
    tc = np.minimum(t, V - 1)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    want = torch.nn.functional.cross_entropy(xt, torch.tensor(tc).long(), reduction="none", label_smoothing=eps) * torch.tensor(w[tc]) / B
    want.sum().backward()
    rows, grad = LS.smoothed_rows(x, t, w, eps, B), LS.smoothed_grad(x, t, w, eps, B)
    np.testing.assert_allclose(rows, want.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(grad, xt.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert rows[0] == 0.0 and np.abs(grad[0]).max() == 0.0
    if V > 1 and eps > 0:
        # ... and it is NOT torch's weighted form, which weights the uniform term per class
        other = torch.nn.functional.cross_entropy(xt.detach(), torch.tensor(tc).long(), weight=torch.tensor(w), reduction="none",
                                                  label_smoothing=eps) / B
        assert np.abs(other.numpy() - rows).max() > 1e-3
    # the minichainer Function: the same numbers, as one summed loss
    f = LS.SmoothedSoftmaxCrossEntropy(tc, w, eps)
    v = f(x)
    np.testing.assert_allclose(float(v.data), rows.sum(), rtol=1e-12)
    np.testing.assert_allclose(f.backward([np.float64(1.0)]), grad, rtol=1e-12, atol=1e-15)


# ------------------------------------------------------------------ 2. the patched oracle
def _setup(seed=0, B=3, T=21, D=26, L=6, V=11):
    cfg = tiny_cfg(c1=8)
    P = R.init_params(cfg, D, V, seed=seed, dtype=np.float64)
    X, y = R.synth_batch(B, T, D, L, V, seed=seed + 1, dtype=np.float64)
    return cfg, P, X, y, V


def _loss(cfg, P, X, y, V, teach=1.0):
    m = R.RefModel(cfg, {k: v.copy() for k, v in P.items()}, V)
    return m, m.forward_loss(X, y, teach, pyrandom=random.Random("seed-ast-20h"))


def test_patched_oracle_passes_directional_finite_differences():
    """forward_loss of the float64 oracle with the smoothed loss swapped in: central differences along a random direction of four decoder
    and encoder parameters against the backward pass, within 1e-6 relative."""
    cfg, P, X, y, V = _setup()
    eps, h = 0.1, 1e-5
    rng = np.random.default_rng(11)
    with LS.smoothed_oracle(eps):
        m, loss = _loss(cfg, P, X, y, V)
        m.cleargrads()
        loss.backward()
        grads = {k: p.grad.copy() for k, p in m.params()}
        for k in ("out/W", "L1_dec/lateral/W", "attn_Wa/W", "L0_enc/upward/W"):
            # the direction: a random unit tensor plus the unit gradient, normalised -- a purely random direction of a (H, H) matrix has
            # a derivative near 0, where the round-off of the difference quotient (1e-16 loss / h) is no longer 1e-6 of it
            d = rng.standard_normal(P[k].shape)
            d = d / np.sqrt((d * d).sum()) + grads[k] / np.sqrt((grads[k] ** 2).sum())
            d /= np.sqrt((d * d).sum())
            Pp, Pm = dict(P), dict(P)
            Pp[k], Pm[k] = P[k] + h * d, P[k] - h * d
            num = (float(_loss(cfg, Pp, X, y, V)[1].data) - float(_loss(cfg, Pm, X, y, V)[1].data)) / (2 * h)
            ana = float((grads[k] * d).sum())
            print(k, num, ana, abs(num - ana) / abs(ana))
            assert abs(num - ana) <= 1e-6 * abs(ana), (k, num, ana)
    # and the smoothed loss is another loss (outside the context the oracle is itself again)
    assert float(loss.data) != float(_loss(cfg, P, X, y, V)[1].data)


def test_patched_oracle_at_zero_is_the_oracle_bit_for_bit():
    cfg, P, X, y, V = _setup()
    for dt in (np.float64, np.float32):
        Pd, Xd = {k: v.astype(dt) for k, v in P.items()}, X.astype(dt)
        m0, l0 = _loss(cfg, Pd, Xd, y, V, teach=0.5)
        m0.cleargrads()
        l0.backward()
        with LS.smoothed_oracle(0.0):
            m1, l1 = _loss(cfg, Pd, Xd, y, V, teach=0.5)
            m1.cleargrads()
            l1.backward()
        assert np.asarray(l0.data).tobytes() == np.asarray(l1.data).tobytes()
        g0, g1 = dict(m0.params()), dict(m1.params())
        for k in g0:
            assert g0[k].grad.tobytes() == g1[k].grad.tobytes(), k
    from oracle import minichainer as F
    assert F.softmax_cross_entropy.__module__ == "oracle.minichainer"      # restored


# ------------------------------------------------------------------ 3. validation and the ABI mirror
BAD = [-0.1, 1.0, float("nan"), "0.1"]


@pytest.mark.parametrize("eps", BAD, ids=repr)
def test_forward_loss_refuses_a_bad_label_smoothing(eps, monkeypatch):
    from ast_amd import _lib
    from ast_amd.seq2seq import SpeechEncoderDecoder
    m = SpeechEncoderDecoder(None, tiny_cfg())

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(m, "encode", touched)
    X, y = np.zeros((1, 16, 8), np.float32), np.array([[1, 5, 2]], np.int32)
    with pytest.raises(ValueError, match="label_smoothing"):
        m.forward_loss(X, y, 1.0, label_smoothing=eps)


def test_forward_loss_takes_label_smoothing_after_y_global():
    import inspect
    from ast_amd.seq2seq import SpeechEncoderDecoder, checked_label_smoothing
    names = list(inspect.signature(SpeechEncoderDecoder.forward_loss).parameters)
    assert names[names.index("y_global") + 1] == "label_smoothing"
    assert inspect.signature(SpeechEncoderDecoder.forward_loss).parameters["label_smoothing"].default == 0.0
    assert checked_label_smoothing(0) == 0.0 and checked_label_smoothing(np.float32(0.5)) == 0.5 and checked_label_smoothing(0.999) == 0.999
    for bad in BAD + [float("inf"), None, True]:
        with pytest.raises(ValueError):
            checked_label_smoothing(bad)


@pytest.mark.parametrize("eps", BAD, ids=repr)
def test_nn_refuses_a_bad_extras_label_smoothing(eps, tmp_path):
    """extras.label_smoothing is checked when the experiment directory is read, in front of the loader and the model."""
    from ast_amd.nn import NN
    mcfg = tiny_cfg()
    del mcfg["rnn_config"]["dec_vocab_size"]
    tcfg = {"seed": "s", "gpuid": 0, "batch_size": 4, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 1,
            "optimizer": {"type": 0, "lr": 1e-3, "l2": 0, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0, "label_smoothing": eps},
            "data": {"dataloader": "synthetic", "vocab_size": 11, "feat_dim": 13, "n_utts": {"syn_train": 4, "syn_dev": 2},
                     "frames": [60, 100], "targets": [2, 5], "buckets_num": 2, "buckets_width": 80, "max_pred": 8,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w"}}
    json.dump(mcfg, open(tmp_path / "model_cfg.json", "w"))
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))          # (json writes nan as NaN and reads it back as nan)
    with pytest.raises(ValueError, match="extras.label_smoothing"):
        NN(str(tmp_path))


def test_decoder_descriptor_grew_by_its_last_field():
    from ast_amd import _lib
    names = [f[0] for f in _lib.DecoderDesc._fields_]
    assert names[-1] == "label_smoothing" and _lib.DecoderDesc._fields_[-1][1] is C.c_float

    class Before(C.Structure):
        _fields_ = _lib.DecoderDesc._fields_[:-1]
    assert C.sizeof(_lib.DecoderDesc) > C.sizeof(Before)
    d = _lib.DecoderDesc(4, 6, 20, 64, 16, 64, 57, 1)
    assert d.label_smoothing == 0.0 and d.struct_size == C.sizeof(_lib.DecoderDesc)
    assert "astk_softmax_ce_fwd_ex" in _lib.SIGNATURES
