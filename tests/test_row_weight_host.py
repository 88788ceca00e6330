"""CPU tests of the per-row loss weights: the float64 model of tests/row_weight_model.py against torch, the float64
oracle with the model swapped in against finite differences, and the Python surface and the C ABI mirror."""
import ctypes as C
import random
import re
import os

import numpy as np
import pytest
import torch

import row_weight_model as RW
from conftest import tiny_cfg
from oracle import ast_ref as R

WEIGHTS = np.array([1.5, -0.5, 0.0, 0.25, 1.0, 2.0])


# ------------------------------------------------------------------ 1. the model against torch
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("V", [1, 5, 257])
def test_model_is_the_torch_loss_times_the_weights(V, eps):
    """rows = r_b * cross_entropy(reduction="none", label_smoothing=eps) * w[t] / B in float64, the gradient by autograd; the weights
    hold a negative and a zero entry (that row: loss and gradient exactly 0)."""
    rng = np.random.default_rng(V)
    B = 6
    x = rng.standard_normal((B, V)) * 4
    t = rng.integers(0, V, B)
    w = rng.random(V) + 0.5
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    want = torch.nn.functional.cross_entropy(xt, torch.tensor(t).long(), reduction="none", label_smoothing=eps) \
        * torch.tensor(w[t]) * torch.tensor(WEIGHTS) / B
    want.sum().backward()
    rows, grad = RW.weighted_rows(x, t, w, WEIGHTS, eps, B), RW.weighted_grad(x, t, w, WEIGHTS, eps, B)
    np.testing.assert_allclose(rows, want.detach().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(grad, xt.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert rows[2] == 0.0 and np.abs(grad[2]).max() == 0.0
    if V > 1:
        assert rows[1] < 0.0      # (a negative weight: a negative row)
    # the minichainer Function: the same numbers, as one summed loss
    f = RW.RowWeightedSoftmaxCrossEntropy(t, w, eps, WEIGHTS)
    v = f(x)
    np.testing.assert_allclose(float(v.data), rows.sum(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(f.backward([np.float64(1.0)]), grad, rtol=1e-12, atol=1e-15)
    # None is all ones
    np.testing.assert_array_equal(RW.weighted_rows(x, t, w, None, eps, B), RW.weighted_rows(x, t, w, np.ones(B), eps, B))


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
    """forward_loss of the float64 oracle with the weighted loss swapped in (mixed signs, eps 0.1): central differences along a direction
    of four decoder and encoder parameters against the backward pass, within 1e-6 relative."""
    cfg, P, X, y, V = _setup()
    eps, h, r = 0.1, 1e-5, np.array([1.5, -0.5, 0.25])
    rng = np.random.default_rng(11)
    with RW.weighted_oracle(eps, r):
        m, loss = _loss(cfg, P, X, y, V)
        m.cleargrads()
        loss.backward()
        grads = {k: p.grad.copy() for k, p in m.params()}
        for k in ("out/W", "L1_dec/lateral/W", "attn_Wa/W", "L0_enc/upward/W"):
            # the direction: a random unit tensor plus the unit gradient, normalised (test_label_smoothing_host.py says why)
            d = rng.standard_normal(P[k].shape)
            d = d / np.sqrt((d * d).sum()) + grads[k] / np.sqrt((grads[k] ** 2).sum())
            d /= np.sqrt((d * d).sum())
            Pp, Pm = dict(P), dict(P)
            Pp[k], Pm[k] = P[k] + h * d, P[k] - h * d
            num = (float(_loss(cfg, Pp, X, y, V)[1].data) - float(_loss(cfg, Pm, X, y, V)[1].data)) / (2 * h)
            ana = float((grads[k] * d).sum())
            print(k, num, ana, abs(num - ana) / abs(ana))
            assert abs(num - ana) <= 1e-6 * abs(ana), (k, num, ana)
    # and the weighted loss is another loss (outside the context the oracle is itself again)
    assert float(loss.data) != float(_loss(cfg, P, X, y, V)[1].data)


def test_patched_oracle_is_linear_in_the_weights():
    """The loss under r is sum_b r_b (loss under the b-th unit vector): what makes the per-row NLLs available to the risk tests."""
    cfg, P, X, y, V = _setup()
    r = np.array([1.5, -0.5, 0.25])
    with RW.weighted_oracle(0.0, r):
        whole = float(_loss(cfg, P, X, y, V)[1].data)
    parts = []
    for b in range(3):
        with RW.weighted_oracle(0.0, np.eye(3)[b]):
            parts.append(float(_loss(cfg, P, X, y, V)[1].data))
    assert abs(whole - float(np.dot(r, parts))) <= 1e-12 * np.abs(np.asarray(parts) * r).sum()


def test_patched_oracle_at_ones_is_the_oracle_bit_for_bit():
    cfg, P, X, y, V = _setup()
    for dt in (np.float64, np.float32):
        Pd, Xd = {k: v.astype(dt) for k, v in P.items()}, X.astype(dt)
        m0, l0 = _loss(cfg, Pd, Xd, y, V, teach=0.5)
        m0.cleargrads()
        l0.backward()
        with RW.weighted_oracle(0.0, np.ones(3)):
            m1, l1 = _loss(cfg, Pd, Xd, y, V, teach=0.5)
            m1.cleargrads()
            l1.backward()
        assert np.asarray(l0.data).tobytes() == np.asarray(l1.data).tobytes()
        g0, g1 = dict(m0.params()), dict(m1.params())
        for k in g0:
            assert g0[k].grad.tobytes() == g1[k].grad.tobytes(), k
    from oracle import minichainer as F
    assert F.softmax_cross_entropy.__module__ == "oracle.minichainer"      # restored


# ------------------------------------------------------------------ 3. the Python surface and the ABI mirror
def test_signatures_and_risk_desc():
    from ast_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "astk.h")).read()
    sig = _lib.SIGNATURES
    for name, base in (("astk_decoder_fwd_w", "astk_decoder_fwd_ex"), ("astk_softmax_ce_fwd_w", "astk_softmax_ce_fwd_ex")):
        assert sig[name][0] is C.c_int and len(sig[name][1]) == len(sig[base][1]) + 1
        decl = re.search(r"int %s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(sig[name][1]) and "const float* row_weight" in decl
    decl = re.search(r"int astk_decoder_fwd_w\(([^;]*)\);", hdr).group(1).split(",")
    names = [a.split()[-1].lstrip("*") for a in decl]
    assert names[names.index("targets") + 1] == "row_weight"      # behind `targets`
    decl = re.search(r"int astk_risk_weights\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(sig["astk_risk_weights"][1]) == 12
    fields = re.search(r"typedef struct \{([^}]*)\} astk_risk_desc;", hdr).group(1)
    names = [re.sub(r"/\*.*?\*/", "", f).split()[-1] for f in fields.split(";") if re.sub(r"/\*.*?\*/", "", f).strip()]
    assert names == [f[0] for f in _lib.RiskDesc._fields_]
    d = _lib.RiskDesc(3, 12, 1, 0.5, 2.0, 0.25)
    assert d.struct_size == C.sizeof(_lib.RiskDesc) == 32 and (d.U, d.R, d.cost) == (3, 12, 1)
    assert (d.alpha, d.risk_scale, d.ref_weight) == (0.5, 2.0, 0.25)
    assert int(re.search(r"#define ASTK_RISK_MAX_LIST (\d+)", hdr).group(1)) == _lib.RISK_MAX_LIST
    assert _lib.RISK_COSTS == {"bleu": 0, "edit": 1}


def test_decoder_descriptor_did_not_grow():
    from ast_amd import _lib
    assert _lib.DecoderDesc._fields_[-1][0] == "label_smoothing"


def test_forward_loss_refuses_row_weight_with_ctc(monkeypatch):
    from ast_amd import _lib
    from ast_amd.seq2seq import SpeechEncoderDecoder
    cfg = tiny_cfg()
    cfg["rnn_config"]["ctc"] = True
    m = SpeechEncoderDecoder(None, cfg)

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(m, "encode", touched)
    X, y = np.zeros((1, 16, 8), np.float32), np.array([[1, 5, 2]], np.int32)
    with pytest.raises(ValueError, match="row_weight"):
        m.forward_loss(X, y, 1.0, ctc_weight=0.3, row_weight=np.ones(1, np.float32))


def test_forward_loss_takes_row_weight_behind_the_reference_arguments():
    """The keyword stands behind the reference's five arguments and in front of the extension keywords, whose order their own tests pin."""
    import inspect
    from ast_amd.seq2seq import SpeechEncoderDecoder
    p = inspect.signature(SpeechEncoderDecoder.forward_loss).parameters
    names = list(p)
    assert names[1:7] == ["X", "y", "teach_ratio", "random_out", "add_noise", "row_weight"] and p["row_weight"].default is None
