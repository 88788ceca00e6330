"""GPU tests of label smoothing in the training loss (include/astk.h astk_decoder_desc.label_smoothing,
astk_softmax_ce_fwd_ex): the operator on the value cases of tests/range_cases.py, one train step on every decoder route against the
float64 oracle with the smoothed loss swapped in (tests/label_smoothing_model.py), the invariants (predictions, the closed form of the
change in d(out/b)), eps = 0 as the loss it always was, reproducibility of the last-block loss sum, the argument checks, and train.py."""
import contextlib
import ctypes as C
import random

import numpy as np
import pytest
import torch

import label_smoothing_model as LS
import range_cases as RC
import schedule_helpers as SH
from conftest import tiny_cfg
from test_gpu_ops import GuardedWS, _dec_setup, close, dev, ok, stream, vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


# ------------------------------------------------------------------ 1. operator level
def _ce_run(lib, x, t, w, ld, eps, t_stride=1, t_col=0, ex=True):
    B, V = x.shape
    buf = torch.zeros(B, ld, device="cuda")
    buf[:, :V] = dev(x)
    tm = np.full((B, t_stride), -7, np.int32)                         # the targets in column t_col of a (B, t_stride) matrix
    tm[:, t_col] = t
    t_d, w_d = dev(tm, torch.int32), dev(w)
    rows_d = torch.zeros(B, device="cuda")
    am_d = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    tp = C.c_void_p(t_d.data_ptr() + 4 * t_col)
    if ex:
        ok(lib, lib.astk_softmax_ce_fwd_ex(B, V, ld, vp(buf), tp, t_stride, vp(w_d), 1.0 / B, eps, vp(rows_d), vp(am_d), stream()))
    else:
        ok(lib, lib.astk_softmax_ce_fwd(B, V, ld, vp(buf), tp, t_stride, vp(w_d), 1.0 / B, vp(rows_d), vp(am_d), stream()))
    torch.cuda.synchronize()
    return buf, rows_d, am_d


@pytest.mark.parametrize("eps", [0.1, 0.5])
@pytest.mark.parametrize("V", RC.CE_VOCABS + [8004])
@pytest.mark.parametrize("kind", RC.CE_KINDS)
def test_softmax_ce_ex_value_cases(lib, kind, V, eps):
    """astk_softmax_ce_fwd_ex on every softmax-CE value case (logits ~ N(0, 60^2), at +-1e4, target at the row's minimum / maximum, tied
    maxima, a clamped target id, a class-weight-0 target; vocabularies below, at and above a workgroup and 8004) against the weight-free
    float64 torch loss times w[t]: loss rows within range_cases.ce_row_bound, gradient within ce_grad_bound through close(), padding
    columns exactly 0, argmax the first maximum, row 0 (weight 0) exactly 0; directly and through a (B, 5) target matrix read at
    column 2.  The uniform term at +-1e4 is what a plain sum of the logits would lose."""
    x, t, w = RC.ce_case(kind, V)
    B, ld = x.shape[0], V + 3
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tc = np.minimum(t, V - 1)
    want = torch.nn.functional.cross_entropy(xt, torch.tensor(tc).long(), reduction="none", label_smoothing=eps) \
        * torch.tensor(w.astype(np.float64)[tc]) / B
    want.sum().backward()
    want, grad = want.detach().numpy(), xt.grad.numpy()
    np.testing.assert_allclose(want, LS.smoothed_rows(x, t, w, eps, B), rtol=1e-11, atol=1e-13)      # (the shared model says the same)
    for t_stride, t_col in ((1, 0), (5, 2)):
        buf, rows_d, am_d = _ce_run(lib, x, t, w, ld, eps, t_stride, t_col)
        got = rows_d.cpu().double().numpy()
        print(kind, V, eps, "row err", np.abs(got - want).max(), "bound", RC.ce_row_bound(x, want),
              "grad err", float((buf[:, :V].cpu().double() - xt.grad).abs().max()), "bound", RC.ce_grad_bound(x, grad))
        assert np.abs(got - want).max() <= RC.ce_row_bound(x, want), (got, want)
        close(buf[:, :V], xt.grad, atol=RC.ce_grad_bound(x, grad), msg="dlogits")
        assert float(buf[:, V:].abs().max()) == 0.0
        assert (am_d.cpu().numpy() == x.argmax(1)).all(), "argmax (first maximum)"
        if V > 1:                                                     # row 0's target has class weight 0
            assert float(rows_d[0]) == 0.0 and float(buf[0, :V].abs().max()) == 0.0


@pytest.mark.parametrize("V", RC.CE_VOCABS + [8004])
@pytest.mark.parametrize("kind", RC.CE_KINDS)
def test_softmax_ce_ex_at_zero_is_softmax_ce(lib, kind, V):
    """eps = 0: gradient buffer, loss rows and argmax are the bits of astk_softmax_ce_fwd."""
    x, t, w = RC.ce_case(kind, V)
    a = _ce_run(lib, x, t, w, V + 3, 0.0, 5, 2, ex=True)
    b = _ce_run(lib, x, t, w, V + 3, 0.0, 5, 2, ex=False)
    for u, v, what in zip(a, b, ("buffer", "rows", "argmax")):
        assert torch.equal(u, v), what


def test_softmax_ce_ex_refuses_a_bad_label_smoothing(lib):
    for bad in (1.0, -0.1, float("nan"), float("inf")):
        buf = torch.full((2, 8), 3.0, device="cuda")
        t_d = torch.zeros(2, dtype=torch.int32, device="cuda")
        assert lib.astk_softmax_ce_fwd_ex(2, 5, 8, vp(buf), vp(t_d), 1, None, 0.5, bad, None, None, stream()) != 0
        assert "label_smoothing" in lib.astk_last_error().decode()
        torch.cuda.synchronize()
        assert float((buf - 3.0).abs().max()) == 0.0


# ------------------------------------------------------------------ 2. one train step on every route against the patched float64 oracle
EPS, OUT_GAIN = 0.1, 4.0      # the first choice; a case whose loss smoothing moves by less than the validity condition raises them (below)


def _mid_cfg(drop):
    return tiny_cfg(enc_layers=3, dec_layers=2, H=64, E=16, A=64, c0=16, c1=32, V=57, drop=drop)


# name -> (cfg(drop), B, T, D, L, V, drop, teach, route, eps, gain of out/W).  At an initialisation the target's logit lies no further
# from the row's mean than any other, so the change of the loss, eps w c sum (x_t - mean x), nearly cancels over the rows of the larger
# batches: their eps and gain were raised until the float64 oracle showed the condition (2e-3 of the loss; measured 3.3e-3, 2.7e-3,
# 3.2e-3, 2.9e-3, 4.2e-3, 3.9e-3 in the order below).  Routes (astk_decoder_path): "per_launch" 0, "persist" bit 0, "split" bit 2 (two
# launches over halves of the rows), "wide" 16.
CASES = {
    # V no multiple of 4; teach 0.5: steps that feed their argmax back (the in-loop softmax-CE call)
    "tiny-ls": (lambda d: tiny_cfg(c1=8, drop=d), 3, 21, 26, 6, 11, 0.0, 0.5, "per_launch", EPS, OUT_GAIN),
    # Vp > V, S B = 32 blocks in k_decoder_post
    "mid-ls": (_mid_cfg, 4, 120, 80, 9, 57, 0.0, 0.8, "persist", EPS, OUT_GAIN),
    "mid-drop-ls": (_mid_cfg, 4, 120, 80, 9, 57, 0.3, 0.8, "persist", 0.2, OUT_GAIN),
    # three layers, two ragged batch tiles, S B = 126 blocks
    "persist-h64-ls": (lambda d: tiny_cfg(enc_layers=3, dec_layers=3, H=128, E=16, A=64, c0=8, c1=16, V=57, drop=d), 18, 70, 80, 8, 57, 0.0, 0.8,
                       "persist", 0.5, 8.0),
    # the mid shape at B 40, widened to H = 512: at H = 64 forty rows fit ONE persistent launch (astk_decoder_path 513); at the shipped
    # width the loop holds 32, so this runs as two launches over 32 + 8 rows (519)
    "split-ls": (lambda d: tiny_cfg(enc_layers=3, dec_layers=2, H=512, E=16, A=64, c0=16, c1=32, V=57, drop=d), 40, 120, 80, 9, 57, 0.0, 0.8,
                 "split", 0.9, 16.0),
    "wide-ls": (lambda d: tiny_cfg(enc_layers=1, dec_layers=1, H=1024, E=128, A=1024, c0=8, c1=16, V=57, drop=d), 4, 40, 80, 6, 57, 0.0, 0.8,
                "wide", 0.2, OUT_GAIN),
}
ROUTES5 = ["tiny-ls", "mid-ls", "persist-h64-ls", "split-ls", "wide-ls"]


@contextlib.contextmanager
def _out_gain(gain):
    """Inside: the parameters schedule_helpers.oracle_case draws have out/W times `gain` (wider logits: the uniform term weighs more)."""
    orig = SH.make_inputs

    def scaled(*a, **k):
        P, X, y = orig(*a, **k)
        P = dict(P)
        P["out/W"] = P["out/W"] * np.float32(gain)
        return P, X, y
    SH.make_inputs = scaled
    try:
        yield
    finally:
        SH.make_inputs = orig


def _oracle(name):
    """The float64 oracle's train step on the smoothed loss (the case's eps and gain of out/W), computed once per process and case (the cache
    key of schedule_helpers.oracle_case holds the name), plus the UNSMOOTHED float64 loss of the same inputs, flags, masks and noise."""
    cfgf, B, T, D, L, V, drop, teach, _, eps, gain = CASES[name]
    with LS.smoothed_oracle(eps), _out_gain(gain):
        o = SH.oracle_case(name, cfgf, B, T, D, L, V, drop, teach)
    if "loss_plain" not in o:
        from oracle import ast_ref as R
        m = R.RefModel(o["cfg"], {k: v.astype(np.float64) for k, v in o["P"].items()}, V)
        if drop > 0:
            m.masks = lambda shape, ratio, tag: o["rec"].masks[tag]
        lp = m.forward_loss(o["X"].astype(np.float64), o["y"], 0.5, add_noise=0.25 if drop > 0 else 0, noise=o["noise"],
                            pyrandom=SH._Fixed(o["flags"]))
        assert list(m.use_truth) == list(o["flags"])
        o["loss_plain"] = float(lp.data)
    return o


def _gpu_step(lib, name, eps, scheme="bf16x3", with_opt=False, deterministic=False, omit_keyword=False):
    """One train step (forward, backward, optionally the optimizer's clip norm) of a fresh model on the case's inputs, flags, masks."""
    from oracle.ast_ref_torch import masks_from_recording
    from ast_amd.seq2seq import using_config
    cfgf, B, T, D, L, V, drop, teach, route = CASES[name][:9]
    o = _oracle(name)
    g = SH.gpu_model(o["cfg"], o["P"], D, V)
    g.gemm_precision = scheme
    g.deterministic = deterministic
    if drop > 0:
        packed = masks_from_recording(o["cfg"], o["rec"].masks, o["enc"].shape[1], L - 1, B)
        g.inject = {k: torch.from_numpy(v) for k, v in packed.items()}
        g.inject["noise"] = torch.from_numpy(o["noise"])
    g.inject["use_truth"] = o["flags"]
    opt = SH.gpu_optimizer(g, SH.OPT) if with_opt else None
    kw = {} if omit_keyword else {"label_smoothing": eps}
    with using_config("train", True):
        loss = g.forward_loss(X=torch.from_numpy(o["X"]), y=torch.from_numpy(o["y"]), teach_ratio=teach, random_out=0,
                              add_noise=0.25 if drop > 0 else 0, **kw)
        assert g._cur["dd"].label_smoothing == np.float32(0.0 if omit_keyword else eps)
        g.cleargrads()
        loss.backward()
        grads = g.arena.to_numpy(grads=True)
        arena = g.arena._grad.clone()
        if opt is not None:
            opt.update()
    torch.cuda.synchronize()
    path = lib.astk_decoder_path(C.byref(g._cur["dd"]))
    want = {"per_launch": path == 0, "persist": bool(path & 1) and not path & 4, "split": bool(path & 4), "wide": path == 16}[route]
    assert want, f"{name}: astk_decoder_path = {path}, meant to run on the {route} route"
    assert SH.status_word() == 0
    return dict(loss=float(loss.data), bits=loss.pair[:1].clone().view(torch.int32).item(), grads=grads, arena=arena,
                gnorm=opt.last_grad_norm if opt is not None else None, enc=g.enc_states.cpu().numpy(), pred=g._cur["pred"].clone(), o=o)


@pytest.mark.parametrize("name", list(CASES))
def test_smoothed_train_step_against_the_patched_oracle(lib, name, gemm_scheme):
    """Forward, backward and clip norm at eps = 0.1 with out/W x 4 (more of both where the condition below asks for it) against the float64 oracle on the smoothed loss, within the project's
    bounds for a train step (schedule_helpers.assert_first_step_against_oracle: loss and clip norm 1e-4, every gradient 3e-4), on the
    per-launch loop, the persistent loop (two and three layers, with dropout), the row split and the wide loop -- each asserted through
    astk_decoder_path.  Validity, on the oracle alone: smoothing moves the case's loss by at least 20 x the loss bound."""
    o = _oracle(name)
    assert abs(o["loss"] - o["loss_plain"]) >= 2e-3 * abs(o["loss"]), (name, o["loss"], o["loss_plain"])
    if name == "tiny-ls":
        assert 0 in o["flags"], "the case should feed at least one argmax back"
    if name == "mid-ls":
        assert (o["y"][:, -1] == 0).any() and (o["y"][:, -1] != 0).any(), "PAD targets in some rows' last columns"
    r = _gpu_step(lib, name, CASES[name][9], scheme=gemm_scheme, with_opt=True)
    print(name, gemm_scheme, "loss", r["loss"], o["loss"], "plain", o["loss_plain"], "gnorm", r["gnorm"], o["gnorm"])
    SH.assert_first_step_against_oracle(name, o, r["loss"], r["gnorm"], r["enc"], r["grads"])


# ------------------------------------------------------------------ 3. invariants
@pytest.mark.parametrize("name", ROUTES5)
def test_predictions_do_not_move_and_out_bias_gradient_moves_by_the_closed_form(lib, name):
    """Same inputs and flags at eps = 0 and eps = 0.3: `pred` is equal (so every fed-back token and every logit is), and
    d(out/b)_eps - d(out/b)_0 = sum_{s,b} w[t] c eps (onehot(t) - 1/V), formed on the host from the targets alone, within 3e-4 of
    max |d(out/b)|."""
    eps = 0.3
    a, b = _gpu_step(lib, name, 0.0), _gpu_step(lib, name, eps)
    assert torch.equal(a["pred"], b["pred"])
    o = a["o"]
    y, V, B = o["y"], CASES[name][5], CASES[name][1]
    w = np.ones(V)
    w[0] = 0.0                                                   # mask_pad_id
    want = np.zeros(V)
    for s in range(1, y.shape[1]):
        for t in np.clip(y[:, s], 0, V - 1):
            oh = np.zeros(V)
            oh[t] = 1.0
            want += w[t] / B * eps * (oh - 1.0 / V)              # dx carries -(1 - eps) onehot - eps / V against -onehot
    got = b["grads"]["out/b"].astype(np.float64) - a["grads"]["out/b"].astype(np.float64)
    scale = max(np.abs(a["grads"]["out/b"]).max(), np.abs(b["grads"]["out/b"]).max())
    print(name, "identity err", np.abs(got - want).max(), "of", scale)
    assert np.abs(want).max() > 10 * 3e-4 * scale                # (the change is well above the bound it is checked to)
    assert np.abs(got - want).max() <= 3e-4 * scale
    assert b["loss"] != a["loss"]


# ------------------------------------------------------------------ 4. eps = 0 is the step it always was
@pytest.mark.parametrize("name", ["tiny-ls", "mid-ls", "persist-h64-ls"])
def test_zero_smoothing_is_the_call_without_the_keyword(lib, name):
    a = _gpu_step(lib, name, 0.0, deterministic=True, omit_keyword=True)
    b = _gpu_step(lib, name, 0.0, deterministic=True)
    assert a["bits"] == b["bits"] and torch.equal(a["arena"], b["arena"]) and torch.equal(a["pred"], b["pred"])
    # ... and that loss is the UNSMOOTHED oracle's (1e-4, the train step's bound)
    assert SH.rel(a["loss"], a["o"]["loss_plain"]) < 1e-4


# ------------------------------------------------------------------ 5. reproducibility of the last-block sum
def test_smoothed_persistent_step_is_reproducible(lib):
    """126 blocks of k_decoder_post rewrite their loss rows and the last to arrive sums them, in index order: the loss bits do not depend
    on which block that is; in deterministic mode the gradients are bit-equal too."""
    runs = [_gpu_step(lib, "persist-h64-ls", EPS, deterministic=True) for _ in range(2)]
    assert runs[0]["bits"] == runs[1]["bits"]
    assert torch.equal(runs[0]["arena"], runs[1]["arena"])
    assert np.isfinite(runs[0]["loss"]) and runs[0]["loss"] > 0


# ------------------------------------------------------------------ 6. bad arguments
def test_decoder_forward_refuses_a_bad_label_smoothing(lib):
    B, L, T, H, E, A, V, nl = 5, 9, 23, 64, 16, 32, 57, 1
    s = _dec_setup(lib, B, L, T, H, E, A, V, nl, False, seed=B + L + 3)
    d = s["d"]
    nbytes = lib.astk_decoder_workspace_bytes(C.byref(d))
    assert nbytes > 0
    ws = GuardedWS(nbytes)
    enc_d, c0_d, h0_d = dev(s["enc"]), dev(s["c0"]), dev(s["h0"])
    y_d, fl_d = dev(s["y"], torch.int32), dev(np.asarray(s["flags"]), torch.int32)
    loss_d, pred_d = torch.full((1,), -5.0, device="cuda"), torch.full((s["S"], B), -3, dtype=torch.int32, device="cuda")

    def fwd():
        return lib.astk_decoder_fwd_ex(C.byref(d), C.byref(s["dp"]), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), vp(fl_d), None, None, None, None,
                                       vp(loss_d), vp(pred_d), vp(ws), nbytes, stream())
    for bad in (1.0, -0.1, float("nan")):
        d.label_smoothing = bad
        assert fwd() < 0
        assert "label_smoothing" in lib.astk_last_error().decode()
        torch.cuda.synchronize()
        assert float(loss_d) == -5.0 and int((pred_d != -3).sum()) == 0 and int((ws.t != 0x5A).sum()) == 0, "the refused call launched something"
    d.label_smoothing = 0.1
    assert lib.astk_decoder_path(C.byref(d)) & 1
    ok(lib, fwd())
    torch.cuda.synchronize()
    ws.check("decoder fwd, eps = 0.1")
    smoothed = float(loss_d)
    d.label_smoothing = 0.0
    ok(lib, fwd())
    torch.cuda.synchronize()
    assert np.isfinite(smoothed) and smoothed > 0 and smoothed != float(loss_d)


# ------------------------------------------------------------------ 7. train.py
def test_train_py_reads_extras_label_smoothing(tmp_path):
    """Two epochs of `python train.py` on the synthetic set with extras.label_smoothing = 0.1 and without: the training losses differ,
    and the dev loss of predict_scored on the smoothed run's weights is the one an NN without the key computes on them (evaluation never
    smooths)."""
    import json, os, shutil, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mcfg = tiny_cfg(enc_layers=2, dec_layers=1, H=32, E=16, A=32, c0=8, c1=16, V=31, drop=0.0)
    del mcfg["rnn_config"]["dec_vocab_size"]
    tcfg = {"seed": "seed-ast-20h", "gpuid": 0, "batch_size": 8, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 2,
            "optimizer": {"type": 0, "lr": 2e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0},
            "data": {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 24, "syn_dev": 6},
                     "frames": [60, 300], "targets": [2, 9], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w"}}
    logs = {}
    for eps in (0.1, None):
        d = tmp_path / ("ls" if eps else "plain")
        os.makedirs(d)
        if eps:
            tcfg["extras"]["label_smoothing"] = eps
        else:
            tcfg["extras"].pop("label_smoothing", None)
        json.dump(mcfg, open(d / "model_cfg.json", "w"))
        json.dump(tcfg, open(d / "train_cfg.json", "w"))
        r = subprocess.run([sys.executable, os.path.join(root, "train.py"), "-m", str(d), "-e", "2"], cwd=root, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        logs[eps] = [float(l.split(",")[1]) for l in open(d / "train.log").read().split("\n") if l.strip()]
    print(logs)
    assert len(logs[0.1]) == 2 and len(logs[None]) == 2 and all(np.isfinite(logs[0.1]))
    assert all(abs(a - b) > 2e-4 for a, b in zip(logs[0.1], logs[None])), logs      # (the log keeps four decimals)
    # the same weights, evaluated by an NN that smooths its training loss and by one that does not
    from ast_amd.nn import NN
    nn = NN(str(tmp_path / "ls"))
    assert nn.label_smoothing == 0.1 and nn.max_epoch == 2
    _, dev_ls, _ = nn.predict_scored("syn_dev")
    del nn
    shutil.copy(tmp_path / "ls" / "seq2seq_2.model", tmp_path / "plain" / "seq2seq_2.model")
    nn = NN(str(tmp_path / "plain"))
    assert nn.label_smoothing == 0.0 and nn.max_epoch == 2
    _, dev_plain, _ = nn.predict_scored("syn_dev")
    assert np.isfinite(dev_ls) and dev_ls == dev_plain, (dev_ls, dev_plain)
