"""GPU tests of the auxiliary CTC loss on the encoder states (include/astk.h astk_ctc_loss, astk_ctc_greedy,
astk_ctc_head_fwd / _bwd): the operator on the cases of tests/ctc_model.py against the float64 model, its properties (gradient sums,
exact zeros, the count, run-to-run bits, the greedy argmax), one train step against the float64 oracle with the CTC term added
(ctc_model.ctc_oracle), the invariants (weight 0 is the step it always was, the decoder does not move, an infeasible row, save / load)
and the descriptor refusals."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_model as CM
import schedule_helpers as SH
from conftest import tiny_cfg
from test_gpu_ops import GuardedWS, dev, ok, stream, vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


# ------------------------------------------------------------------ 1. operator level
# dlogits bound per case family = 4 x the worst error of the NumPy model run in float32 against its float64 run on the family's cases:
# ctc_model.F32_MODEL_ERR = short 7.8e-6, offset 7.7e-6, peaked 3.1e-5, long 9.2e-5, s511 3.1e-4 (measured on the CPU;
# tests/test_ctc_host.py::test_float32_model_error_is_what_the_bounds_were_taken_from holds the model to these figures).  The error is
# absolute on gradients of magnitude <= 1 and grows with the size of the log-domain quantities; the factor 4 covers another summation order.
GRAD_BOUND = {k: 4.0 * v for k, v in CM.F32_MODEL_ERR.items()}
NLL_RTOL = 1e-5                    # one operator of the project's 1e-4 loss bound

_MODEL = {}


def _model(name):
    """The float64 model's result of one operator case, computed once and shared."""
    if name not in _MODEL:
        x, y, lens = CM.op_case(name)
        _MODEL[name] = (x, y, lens, CM.ctc_loss_grad(x.astype(np.float64), y, lens))
    return _MODEL[name]


def _run_op(lib, x, y, lens, ldv=None, alias=True, scale=1.0, acc0=0.25, first_label=CM.UNK_ID, blank=CM.PAD_ID):
    """astk_ctc_loss on host arrays; returns dict(row_nll, dlogits (B, T, ldv), loss_acc, n_infeasible) as device tensors / numbers."""
    from ast_amd import _lib
    B, T, V = x.shape
    ldv = ldv or V
    buf = torch.full((B, T, ldv), 7.0, device="cuda")
    buf[:, :, :V] = dev(x)
    out = buf if alias else torch.full((B, T, ldv), -3.0, device="cuda")
    y_d = dev(y, torch.int32)
    len_d = None if lens is None else dev(lens, torch.int32)
    d = _lib.CtcDesc(B, T, V, ldv, y.shape[1], y.shape[1], first_label, blank)
    nbytes = lib.astk_ctc_workspace_bytes(C.byref(d))
    assert nbytes > 0, lib.astk_last_error().decode()
    ws = GuardedWS(nbytes)
    nll = torch.full((B,), -1.0, device="cuda")
    acc = torch.full((1,), acc0, device="cuda")
    bad = torch.full((1,), -9, dtype=torch.int32, device="cuda")
    ok(lib, lib.astk_ctc_loss(C.byref(d), vp(buf), vp(y_d), vp(len_d), scale, vp(nll), vp(acc), vp(out), vp(bad), vp(ws), nbytes, stream()))
    ws.check("ctc_loss")
    return dict(row_nll=nll, dlogits=out, loss_acc=float(acc), n_infeasible=int(bad))


@pytest.mark.parametrize("name", list(CM.OP_CASES))
def test_ctc_loss_against_the_float64_model(lib, name):
    """row_nll within 1e-5 relative, dlogits within the family's bound, the gradient of every valid frame summing to 0 within the same
    bound, frames behind a row's length / infeasible rows / the columns V..ldv exactly 0, the count exact, loss_acc = what it held +
    scale * the feasible rows' sum; written in place of the logits (the `ldv-pad` case: into a second buffer)."""
    x, y, lens, m = _model(name)
    c = CM.OP_CASES[name]
    B, T, V = x.shape
    if name == "u31-log-domain":
        assert m["row_nll"][0] > 104, "the linear-domain likelihood must underflow float32"
    scale = 0.5
    r = _run_op(lib, x, y, lens, ldv=c.get("ldv"), alias="ldv" not in c, scale=scale)
    got_nll = r["row_nll"].cpu().double().numpy()
    g = r["dlogits"].cpu().double().numpy()
    want = m["row_nll"]
    finite = ~np.isinf(want)
    bound = GRAD_BOUND[c["family"]]
    err_g = np.abs(g[:, :, :V] / scale - m["dlogits"]).max()
    rel = np.abs(got_nll[finite] - want[finite]) / want[finite]
    sums = np.abs(g[:, :, :V].sum(-1) / scale).max()
    print(name, "nll rel", rel.max() if rel.size else 0.0, "grad err", err_g, "bound", bound, "frame sums", sums)
    assert (np.isinf(got_nll) & (got_nll > 0)).tolist() == (~finite).tolist()
    assert (rel <= NLL_RTOL).all(), (got_nll, want)
    assert err_g <= bound
    assert sums <= bound
    assert r["n_infeasible"] == m["n_infeasible"]
    assert abs(r["loss_acc"] - 0.25 - scale * want[finite].sum()) <= 1e-5 * max(1.0, scale * want[finite].sum())
    n = np.full(B, T) if lens is None else lens
    for b in range(B):
        assert np.abs(g[b, int(n[b]):]).max(initial=0.0) == 0.0, "frames behind the row's length"
        if not finite[b]:
            assert np.abs(g[b]).max() == 0.0, "an infeasible row"
    if g.shape[2] > V:
        assert np.abs(g[:, :, V:]).max() == 0.0


@pytest.mark.parametrize("name", ["b33-ragged", "u255-infeasible-between", "all-equal", "v1098-one-path"])
def test_ctc_loss_is_bit_identical_from_run_to_run(lib, name):
    x, y, lens, _ = _model(name)
    a, b = _run_op(lib, x, y, lens), _run_op(lib, x, y, lens)
    assert torch.equal(a["row_nll"].view(torch.int32), b["row_nll"].view(torch.int32))
    assert torch.equal(a["dlogits"].view(torch.int32), b["dlogits"].view(torch.int32))
    assert np.float32(a["loss_acc"]).view(np.int32) == np.float32(b["loss_acc"]).view(np.int32)


def test_ctc_loss_without_the_optional_outputs(lib):
    """loss_acc and n_infeasible NULL, input_len NULL, another blank / first label: row_nll and dlogits as the model has them."""
    from ast_amd import _lib
    x, y, _, _ = _model("all-equal")
    B, T, V = x.shape
    m = CM.ctc_loss_grad(x.astype(np.float64), y, None, first_label=5, blank=4)
    buf, y_d = dev(x), dev(y, torch.int32)
    d = _lib.CtcDesc(B, T, V, V, y.shape[1], y.shape[1], 5, 4)
    nbytes = lib.astk_ctc_workspace_bytes(C.byref(d))
    ws = GuardedWS(nbytes)
    nll = torch.zeros(B, device="cuda")
    ok(lib, lib.astk_ctc_loss(C.byref(d), vp(buf), vp(y_d), None, 1.0, vp(nll), None, vp(buf), None, vp(ws), nbytes, stream()))
    ws.check("ctc_loss")
    np.testing.assert_allclose(nll.cpu().double().numpy(), m["row_nll"], rtol=NLL_RTOL)
    assert np.abs(buf.cpu().double().numpy() - m["dlogits"]).max() <= GRAD_BOUND["short"]


def test_ctc_greedy_is_the_first_argmax_over_the_valid_frames(lib):
    """Planted ties (equal maxima at several classes, the whole frame equal), V not a multiple of 64, ragged lengths: NumPy's argmax
    (the first maximum) on the valid frames, the blank behind them."""
    from ast_amd import _lib
    rng = np.random.default_rng(5)
    for V, ldv in ((5, 8), (57, 57), (1098, 1100)):
        B, T = 3, 9
        x = rng.standard_normal((B, T, V)).astype(np.float32)
        x[0, 0, :] = 1.5                                           # a whole frame tied
        x[1, 2, [V - 1, V // 2, 1]] = 9.0                          # three tied maxima: the lowest index wins
        x[2, 3, [V - 1, V - 2]] = 9.0
        lens = np.asarray([9, 4, 1], np.int32)
        buf = torch.zeros(B, T, ldv, device="cuda")
        buf[:, :, :V] = dev(x)
        buf[:, :, V:] = 100.0                                      # (columns behind V are not classes)
        best = torch.full((B, T), -5, dtype=torch.int32, device="cuda")
        d = _lib.CtcDesc(B, T, V, ldv, 1, 1, 3, 0)
        ok(lib, lib.astk_ctc_greedy(C.byref(d), vp(buf), vp(dev(lens, torch.int32)), vp(best), stream()))
        torch.cuda.synchronize()
        want = x.argmax(-1)
        for b in range(B):
            want[b, lens[b]:] = 0
        assert (best.cpu().numpy() == want).all(), V
        ok(lib, lib.astk_ctc_greedy(C.byref(d), vp(buf), None, vp(best), stream()))
        torch.cuda.synchronize()
        assert (best.cpu().numpy() == x.argmax(-1)).all(), V


def test_ctc_entry_points_refuse_a_bad_descriptor_before_any_launch(lib):
    from ast_amd import _lib
    B, T, V, L = 2, 4, 7, 3
    buf = torch.full((B, T, V), 2.0, device="cuda")
    y_d = torch.full((B, L), 4, dtype=torch.int32, device="cuda")
    nll = torch.full((B,), -1.0, device="cuda")
    best = torch.full((B, T), -5, dtype=torch.int32, device="cuda")
    ws = GuardedWS(1 << 16)
    good = dict(B=B, T=T, V=V, ldv=V, L=L, ldy=L, first_label=3, blank=0)
    for field, value, word in (("V", 1, "V"), ("blank", V, "blank"), ("blank", -1, "blank"), ("first_label", 0, "first_label"), ("B", 0, "B"),
                               ("T", 0, "T"), ("L", 0, "L"), ("L", 256, "labels"), ("ldv", V - 1, "ldv"), ("struct_size", 8, "struct_size")):
        d = _lib.CtcDesc(**{**good, **({field: value} if field != "struct_size" else {})})
        if field == "struct_size":
            d.struct_size = value
        if field == "L":
            d.ldy = max(value, 1)
        assert lib.astk_ctc_workspace_bytes(C.byref(d)) == 0
        assert lib.astk_ctc_loss(C.byref(d), vp(buf), vp(y_d), None, 1.0, vp(nll), None, vp(buf), None, vp(ws), ws.nbytes, stream()) != 0
        assert word in lib.astk_last_error().decode(), (field, lib.astk_last_error().decode())
        assert lib.astk_ctc_greedy(C.byref(d), vp(buf), None, vp(best), stream()) != 0
        torch.cuda.synchronize()
        assert float((buf - 2.0).abs().max()) == 0.0 and float((nll + 1.0).abs().max()) == 0.0 and int((best != -5).sum()) == 0
        assert int((ws.t != 0x5A).sum()) == 0, "the refused call launched something"
    d = _lib.CtcDesc(**good)
    need = lib.astk_ctc_workspace_bytes(C.byref(d))
    assert lib.astk_ctc_loss(C.byref(d), vp(buf), vp(y_d), None, 1.0, vp(nll), None, vp(buf), None, vp(ws), need - 1, stream()) != 0
    assert "workspace" in lib.astk_last_error().decode()


# ------------------------------------------------------------------ 2. one train step against the oracle with the CTC term
WEIGHT = 0.3


def _with_head(cfgf, ln=False):
    def f(drop):
        c = cfgf(drop)
        c["rnn_config"]["ctc"] = True
        c["rnn_config"]["ln"] = ln
        return c
    return f


def _mid_cfg(drop):
    return tiny_cfg(enc_layers=3, dec_layers=2, H=64, E=16, A=64, c0=16, c1=32, V=57, drop=drop)


# name -> (cfg(drop), B, T, D, L, V, drop, teach, x_lens): the tiny, mid (with and without dropout) and three-layer persistent shapes of
# tests/test_gpu_label_smoothing.py, the head added; one case with ragged true lengths, one on the LayerNorm encoder variant.
CASES = {
    "tiny-ctc": (_with_head(lambda d: tiny_cfg(c1=8, drop=d)), 3, 21, 26, 6, 11, 0.0, 0.5, None),
    "tiny-ln-ctc": (_with_head(lambda d: tiny_cfg(c1=8, drop=d), ln=True), 3, 21, 26, 6, 11, 0.0, 0.5, None),
    "mid-ctc": (_with_head(_mid_cfg), 4, 120, 80, 9, 57, 0.0, 0.8, None),
    "mid-ragged-ctc": (_with_head(_mid_cfg), 4, 120, 80, 9, 57, 0.0, 0.8, [120, 101, 77, 64]),
    "mid-drop-ctc": (_with_head(_mid_cfg), 4, 120, 80, 9, 57, 0.3, 0.8, None),
    "persist-h64-ctc": (_with_head(lambda d: tiny_cfg(enc_layers=3, dec_layers=3, H=128, E=16, A=64, c0=8, c1=16, V=57, drop=d)), 18, 70, 80, 8,
                        57, 0.0, 0.8, None),
}


class _head_inputs:
    """Inside: the parameters schedule_helpers.oracle_case draws carry the head (ctc_model.head_params)."""

    def __enter__(self):
        self.orig = orig = SH.make_inputs

        def with_head(cfg, B, T, D, L, V, **k):
            P, X, y = orig(cfg, B, T, D, L, V, **k)
            P = dict(P)
            P.update(CM.head_params(cfg["rnn_config"]["hidden_units"], V))
            return P, X, y
        SH.make_inputs = with_head

    def __exit__(self, *exc):
        SH.make_inputs = self.orig
        return False


def _oracle(name):
    """The float64 oracle's train step on loss_attention + 0.3 mean nll, once per process and case, plus -- for the validity conditions --
    the CTC term, the rows' nll and the gradient of L0_enc/upward/W WITHOUT the term (same inputs, flags, masks, noise)."""
    cfgf, B, T, D, L, V, drop, teach, x_lens = CASES[name]
    from oracle import ast_ref as R

    def replay():
        m = R.RefModel(o["cfg"], {k: v.astype(np.float64) for k, v in o["P"].items()}, V)
        if drop > 0:
            m.masks = lambda shape, ratio, tag: o["rec"].masks[tag]
        loss = m.forward_loss(o["X"].astype(np.float64), o["y"], 0.5, add_noise=0.25 if drop > 0 else 0, noise=o["noise"],
                              pyrandom=SH._Fixed(o["flags"]))
        return m, loss
    with CM.ctc_oracle(WEIGHT, x_lens), _head_inputs():
        o = SH.oracle_case(name, cfgf, B, T, D, L, V, drop, teach)
        if "ctc_term" not in o:
            m, _ = replay()
            o["ctc_term"], o["ctc_rows"], o["ctc_infeasible"] = m.ctc_term, m.ctc_rows, m.ctc_infeasible
    if "loss_plain" not in o:                                     # (outside the block: the oracle as it is)
        m, loss = replay()
        m.cleargrads()
        loss.backward()
        o["loss_plain"] = float(loss.data)
        o["plain_grads"] = {k: p.grad.copy() for k, p in m.params() if p.grad is not None}
    return o


def _gpu_step(lib, name, weight, scheme="bf16x3", with_opt=False, deterministic=False, omit_keyword=False, y=None, model=None):
    """One train step (forward, backward, optionally the clip norm) of a fresh model on the case's inputs, flags, masks."""
    from oracle.ast_ref_torch import masks_from_recording
    from ast_amd.seq2seq import using_config
    cfgf, B, T, D, L, V, drop, teach, x_lens = CASES[name]
    o = _oracle(name)
    g = model if model is not None else SH.gpu_model(o["cfg"], o["P"], D, V)
    g.gemm_precision = scheme
    g.deterministic = deterministic
    if drop > 0:
        packed = masks_from_recording(o["cfg"], o["rec"].masks, o["enc"].shape[1], L - 1, B)
        g.inject = {k: torch.from_numpy(v) for k, v in packed.items()}
        g.inject["noise"] = torch.from_numpy(o["noise"])
    g.inject["use_truth"] = o["flags"]
    opt = SH.gpu_optimizer(g, SH.OPT) if with_opt else None
    kw = {} if omit_keyword else {"ctc_weight": weight, "x_lens": None if x_lens is None else np.asarray(x_lens, np.int32)}
    yy = o["y"] if y is None else y
    with using_config("train", True):
        loss = g.forward_loss(X=torch.from_numpy(o["X"]), y=torch.from_numpy(yy), teach_ratio=teach, random_out=0,
                              add_noise=0.25 if drop > 0 else 0, **kw)
        g.cleargrads()
        loss.backward()
        grads = g.arena.to_numpy(grads=True)
        arena = g.arena._grad.clone()
        if opt is not None:
            opt.update()
    torch.cuda.synchronize()
    lv = float(loss.data)
    assert SH.status_word() == 0
    return dict(loss=lv, bits=loss.pair[:1].clone().view(torch.int32).item(), grads=grads, arena=arena, model=g,
                gnorm=opt.last_grad_norm if opt is not None else None, enc=g.enc_states.cpu().numpy(), pred=g._cur["pred"].clone(), o=o,
                nll=None if g.ctc_nll is None or omit_keyword or not weight else g.ctc_nll.cpu().double().numpy(), bad=g.ctc_infeasible)


@pytest.mark.parametrize("name", list(CASES))
def test_ctc_train_step_against_the_wrapped_oracle(lib, name, gemm_scheme):
    """Forward, backward and clip norm at ctc_weight = 0.3 against the float64 oracle with the term added, within the project's bounds for
    a train step (schedule_helpers.assert_first_step_against_oracle: loss and clip norm 1e-4, every gradient -- ctc_out/* included --
    3e-4).  Validity, on the oracle alone: every row has a path, the CTC term is at least 2e-3 of the loss, and it moves the gradient
    of L0_enc/upward/W by more than 10 x that gradient's tolerance."""
    o = _oracle(name)
    assert o["ctc_infeasible"] == 0 and np.isfinite(o["ctc_rows"]).all()
    assert o["ctc_term"] >= 2e-3 * abs(o["loss"]), (o["ctc_term"], o["loss"])
    assert abs(o["loss"] - o["loss_plain"] - o["ctc_term"]) <= 1e-9 * abs(o["loss"])
    k = "L0_enc/upward/W"
    gmax = max(np.abs(g).max() for g in o["grads"].values())
    tol = 3e-4 * max(np.abs(o["grads"][k]).max(), 1e-3 * gmax)
    assert np.abs(o["grads"][k] - o["plain_grads"][k]).max() > 10 * tol
    assert "ctc_out/W" in o["grads"] and "ctc_out/b" in o["grads"]
    r = _gpu_step(lib, name, WEIGHT, scheme=gemm_scheme, with_opt=True)
    print(name, gemm_scheme, "loss", r["loss"], o["loss"], "ctc term", o["ctc_term"], "gnorm", r["gnorm"], o["gnorm"])
    SH.assert_first_step_against_oracle(name, o, r["loss"], r["gnorm"], r["enc"], r["grads"])
    np.testing.assert_allclose(r["nll"], o["ctc_rows"], rtol=1e-4)
    assert r["bad"] == 0


# ------------------------------------------------------------------ 3. invariants
@pytest.mark.parametrize("name", ["tiny-ctc", "mid-ctc", "persist-h64-ctc"])
def test_zero_weight_is_the_call_without_the_keyword(lib, name):
    """ctc_weight = 0 on a model with the head: the loss word and the whole gradient arena are the bits of the call without the
    keyword, in deterministic mode; the head's gradient is exactly 0."""
    a = _gpu_step(lib, name, 0.0, deterministic=True, omit_keyword=True)
    b = _gpu_step(lib, name, 0.0, deterministic=True)
    assert a["bits"] == b["bits"] and torch.equal(a["arena"], b["arena"]) and torch.equal(a["pred"], b["pred"])
    assert np.abs(b["grads"]["ctc_out/W"]).max() == 0.0 and np.abs(b["grads"]["ctc_out/b"]).max() == 0.0
    assert SH.rel(a["loss"], a["o"]["loss_plain"]) < 1e-4
    assert "nothing is launched at 0" in b["model"].paths()["ctc"]


@pytest.mark.parametrize("name", ["tiny-ctc", "mid-ragged-ctc", "persist-h64-ctc"])
def test_the_decoder_does_not_move_with_the_weight(lib, name):
    """ctc_weight = 0.3 against 0, deterministic mode: `pred` and every decoder-side parameter gradient are bit-identical; the encoder,
    CNN and head gradients move; the loss grows by the term; twice the same step gives the same bits."""
    a, b, b2 = (_gpu_step(lib, name, w, deterministic=True) for w in (0.0, WEIGHT, WEIGHT))
    assert torch.equal(a["pred"], b["pred"])
    for k in a["grads"]:
        link = k.split("/")[0]
        same = np.array_equal(a["grads"][k].view(np.uint32), b["grads"][k].view(np.uint32))
        if link.startswith("CNN_") or "_enc" in link or link.startswith("ctc_out") or link.startswith("enc_proj"):
            assert not same, f"{k} did not move"
        else:
            assert same, f"{k} moved"
    assert SH.rel(b["loss"] - a["loss"], a["o"]["ctc_term"]) < 1e-3
    assert b["bits"] == b2["bits"] and torch.equal(b["arena"], b2["arena"])
    assert np.array_equal(b["nll"], b2["nll"])


def test_a_batch_with_an_infeasible_row_trains_on_the_others(lib):
    """tiny shape, T'' = 6: row 1 gets four equal labels (needs 7 frames).  The step reports one row, its nll is +inf, the loss and every
    gradient are finite, and the loss is the attention term + 0.3 / B * the other rows' nll."""
    name = "tiny-ctc"
    o = _oracle(name)
    y = o["y"].copy()
    y[1] = [1, 5, 5, 5, 5, 2]
    r = _gpu_step(lib, name, WEIGHT, deterministic=True, y=y)
    plain = _gpu_step(lib, name, 0.0, deterministic=True, y=y)
    assert r["bad"] == 1
    assert np.isinf(r["nll"][1]) and np.isfinite(np.delete(r["nll"], 1)).all()
    assert np.isfinite(r["loss"]) and all(np.isfinite(g).all() for g in r["grads"].values())
    want = plain["loss"] + WEIGHT / len(y) * np.delete(r["nll"], 1).sum()
    assert SH.rel(r["loss"], want) < 1e-5
    assert np.abs(r["grads"]["ctc_out/b"]).max() > 0


def test_save_load_step_gives_the_same_loss_bits(lib, tmp_path):
    from ast_amd import serializers
    from ast_amd.seq2seq import SpeechEncoderDecoder
    name = "mid-ctc"
    a = _gpu_step(lib, name, WEIGHT, deterministic=True)
    o, D, V = a["o"], CASES[name][3], CASES[name][5]
    path = str(tmp_path / "m.npz")
    fresh = SH.gpu_model(o["cfg"], o["P"], D, V)
    serializers.save_npz(path, fresh)
    with np.load(path) as z:
        assert "ctc_out/W" in z.files and "ctc_out/b" in z.files
    cfg = copy.deepcopy(o["cfg"])
    cfg["rnn_config"]["dec_vocab_size"] = V
    m = SpeechEncoderDecoder(0, cfg).materialize(D, seed=123)
    serializers.load_npz(path, m)
    b = _gpu_step(lib, name, WEIGHT, deterministic=True, model=m)
    assert a["bits"] == b["bits"] and torch.equal(a["arena"], b["arena"])
    # a checkpoint WITHOUT the head into a model with it: the head keeps its initial values, everything else is loaded
    nocfg = copy.deepcopy(cfg)
    nocfg["rnn_config"]["ctc"] = False
    P0 = {k: v for k, v in o["P"].items() if not k.startswith("ctc_out/")}
    serializers.save_npz(path, SpeechEncoderDecoder(0, nocfg).materialize(D, values=P0))
    m2 = SpeechEncoderDecoder(0, cfg).materialize(D, seed=123)
    w0 = m2.arena.views["ctc_out/W"].clone()
    serializers.load_npz(path, m2)
    assert torch.equal(m2.arena.views["ctc_out/W"], w0)
    assert torch.equal(m2.arena.views["out/W"].cpu(), torch.from_numpy(o["P"]["out/W"]))


def test_ctc_predict_collapses_the_head_argmax(lib):
    """ctc_predict = repeats collapsed and blanks dropped of argmax(enc_states W^T + b) over each row's valid frames, against NumPy on the
    encoder states the model leaves."""
    name = "mid-ragged-ctc"
    cfgf, B, T, D, L, V, _, _, x_lens = CASES[name]
    o = _oracle(name)
    P = dict(o["P"])
    P["ctc_out/b"] = P["ctc_out/b"].copy()
    P["ctc_out/b"][0] += 0.3                                        # (some blanks among the argmaxes)
    g = SH.gpu_model(o["cfg"], P, D, V)
    hyp = g.ctc_predict(torch.from_numpy(o["X"]), x_lens=np.asarray(x_lens, np.int32))
    enc = g.enc_states.cpu().double().numpy()
    logits = enc @ P["ctc_out/W"].astype(np.float64).T + P["ctc_out/b"]
    lens = CM.t2_lens(o["cfg"]["cnn_config"]["cnn_layers"], x_lens)
    top2 = np.sort(logits, -1)[..., -2:]
    assert (top2[..., 1] - top2[..., 0]).min() > 1e-4, "an argmax within rounding of the runner-up: pick another seed"
    want = [CM.collapse(logits[b, :lens[b]].argmax(-1)) for b in range(B)]
    assert hyp == want and any(len(h) for h in hyp)
    with pytest.raises(ValueError):
        SH.gpu_model(tiny_cfg(), SH.make_inputs(tiny_cfg(), 2, 21, 26, 5, 11)[0], 26, 11).ctc_predict(torch.zeros(2, 21, 26))


# ------------------------------------------------------------------ 4. train.py
def test_train_py_reads_extras_ctc_weight(tmp_path):
    """One epoch of `python train.py` on the synthetic set with rnn_config.ctc and extras.ctc_weight = 0.3: the weight is announced, the
    epoch's mean CTC term and its count of rows without a path are printed, the term is positive and below the logged loss, and the
    checkpoint holds the head."""
    import json, os, re, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mcfg = tiny_cfg(enc_layers=2, dec_layers=1, H=32, E=16, A=32, c0=8, c1=16, V=31, drop=0.0)
    del mcfg["rnn_config"]["dec_vocab_size"]
    mcfg["rnn_config"]["ctc"] = True
    tcfg = {"seed": "seed-ast-20h", "gpuid": 0, "batch_size": 8, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 1,
            "optimizer": {"type": 0, "lr": 2e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0, "ctc_weight": WEIGHT},
            "data": {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 24, "syn_dev": 6},
                     "frames": [60, 300], "targets": [2, 9], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w"}}
    json.dump(mcfg, open(tmp_path / "model_cfg.json", "w"))
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))
    r = subprocess.run([sys.executable, os.path.join(root, "train.py"), "-m", str(tmp_path), "-e", "1"], cwd=root, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "CTC weight: 0.3" in r.stdout
    term, bad = re.search(r"CTC term = ([0-9.]+), rows without a CTC path = (\d+)", r.stdout).groups()
    logged = [float(l.split(",")[1]) for l in open(tmp_path / "train.log").read().split("\n") if l.strip()]
    print(r.stdout[-600:], logged)
    assert len(logged) == 1 and np.isfinite(logged[0]) and 0 < float(term) < logged[0] and int(bad) == 0
    with np.load(tmp_path / "seq2seq_1.model") as z:
        assert z["ctc_out/W"].shape == (31, 32) and z["ctc_out/b"].shape == (31,)
