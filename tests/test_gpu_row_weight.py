"""GPU tests of the per-row loss weights (include/astk.h astk_decoder_fwd_w, astk_softmax_ce_fwd_w): the operator
on the value cases of tests/range_cases.py, one train step on every decoder route against the float64 oracle with the weighted loss
swapped in (tests/row_weight_model.py), mixed signs, all-ones weights and no weights as the step it always was, the zero-weight row,
and reproducibility of the last-block loss sum."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import range_cases as RC
import row_weight_model as RW
import schedule_helpers as SH
from conftest import tiny_cfg
from test_gpu_ops import close, dev, ok, stream, vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


# ------------------------------------------------------------------ 1. operator level
OP_WEIGHTS = np.array([1.5, -0.5, 0.0, 0.25, 1.0], np.float32)


def _ce_run(lib, x, t, w, r, ld, eps, entry="w"):
    B, V = x.shape
    buf = torch.zeros(B, ld, device="cuda")
    buf[:, :V] = dev(x)
    t_d, w_d = dev(t, torch.int32), dev(w)
    r_d = None if r is None else dev(r)
    rows_d = torch.full((B,), 7.0, device="cuda")
    am_d = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    if entry == "w":
        ok(lib, lib.astk_softmax_ce_fwd_w(B, V, ld, vp(buf), vp(t_d), 1, vp(w_d), vp(r_d), 1.0 / B, eps, vp(rows_d), vp(am_d), stream()))
    else:
        assert r is None
        ok(lib, lib.astk_softmax_ce_fwd_ex(B, V, ld, vp(buf), vp(t_d), 1, vp(w_d), 1.0 / B, eps, vp(rows_d), vp(am_d), stream()))
    torch.cuda.synchronize()
    return buf, rows_d, am_d


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("V", RC.CE_VOCABS)
@pytest.mark.parametrize("kind", RC.CE_KINDS)
def test_softmax_ce_w_value_cases(lib, kind, V, eps):
    """astk_softmax_ce_fwd_w on every softmax-CE value case at B = 5 under the weights (1.5, -0.5, 0, 0.25, 1) against the float64
    model: row b within |r_b| x range_cases.ce_row_bound, its gradient within |r_b| x ce_grad_bound (the bounds of the unweighted
    rows), so the zero-weight row exactly 0 in both; padding columns exactly 0, argmax the first maximum whatever the weights; with
    NULL weights the bits of astk_softmax_ce_fwd_ex."""
    x, t, w = RC.ce_case(kind, V, B=5)
    B, ld, r = 5, V + 3, OP_WEIGHTS
    rows0, grad0 = RW.weighted_rows(x, t, w, None, eps, B), RW.weighted_grad(x, t, w, None, eps, B)
    want, grad = RW.weighted_rows(x, t, w, r, eps, B), RW.weighted_grad(x, t, w, r, eps, B)
    row_bound, grad_bound = RC.ce_row_bound(x, rows0), RC.ce_grad_bound(x, grad0)
    buf, rows_d, am_d = _ce_run(lib, x, t, w, r, ld, eps)
    got, gg = rows_d.cpu().double().numpy(), buf[:, :V].cpu().double().numpy()
    re_, ge = np.abs(got - want), np.abs(gg - grad).max(axis=1)
    print(kind, V, eps, "row err", re_, "bound", row_bound, "grad err", ge, "bound", grad_bound)
    assert (re_ <= np.abs(r) * row_bound).all(), (got, want)
    assert (ge <= np.abs(r) * grad_bound).all()
    assert float(rows_d[2]) == 0.0 and float(buf[2].abs().max()) == 0.0, "the zero-weight row"
    assert float(buf[:, V:].abs().max()) == 0.0
    assert (am_d.cpu().numpy() == x.argmax(1)).all(), "argmax (first maximum)"
    a = _ce_run(lib, x, t, w, None, ld, eps)
    b = _ce_run(lib, x, t, w, None, ld, eps, entry="ex")
    for u, v, what in zip(a, b, ("buffer", "rows", "argmax")):
        assert torch.equal(u, v), what
    # all-ones weights: the same bits again (w * 1 = w)
    c = _ce_run(lib, x, t, w, np.ones(B, np.float32), ld, eps)
    for u, v, what in zip(a, c, ("buffer", "rows", "argmax")):
        assert torch.equal(u, v), what


# ------------------------------------------------------------------ 2. one train step on every route against the patched float64 oracle
def _mid_cfg(drop):
    return tiny_cfg(enc_layers=3, dec_layers=2, H=64, E=16, A=64, c0=16, c1=32, V=57, drop=drop)


# name -> (cfg(drop), B, T, D, L, V, drop, teach, route, eps): the smallest shapes that reach each route (astk_decoder_path: "per_launch" 0,
# "persist" bit 0, "split" bit 2 -- two launches over halves of the rows --, "wide" 16).  eps > 0 on one persistent and on the wide case:
# k_decoder_post and k_softmax_ce carry the weights with and without the uniform term.
CASES = {
    # V no multiple of 4; teach 0.5: steps that feed their argmax back (the in-loop softmax-CE call)
    "tiny-rw": (lambda d: tiny_cfg(c1=8, drop=d), 3, 21, 26, 6, 11, 0.0, 0.5, "per_launch", 0.0),
    # Vp > V, S B = 32 blocks in k_decoder_post
    "mid-rw": (_mid_cfg, 4, 120, 80, 9, 57, 0.0, 0.8, "persist", 0.1),
    # three layers, two ragged batch tiles, S B = 126 blocks
    "persist-h64-rw": (lambda d: tiny_cfg(enc_layers=3, dec_layers=3, H=128, E=16, A=64, c0=8, c1=16, V=57, drop=d), 18, 70, 80, 8, 57, 0.0,
                       0.8, "persist", 0.0),
    # B 40 at the shipped width H = 512: two launches over 32 + 8 rows, each half reads its part of the weights
    "split-rw": (lambda d: tiny_cfg(enc_layers=3, dec_layers=2, H=512, E=16, A=64, c0=16, c1=32, V=57, drop=d), 40, 120, 80, 9, 57, 0.0, 0.8,
                 "split", 0.0),
    "wide-rw": (lambda d: tiny_cfg(enc_layers=1, dec_layers=1, H=1024, E=128, A=1024, c0=8, c1=16, V=57, drop=d), 4, 40, 80, 6, 57, 0.0, 0.8,
                "wide", 0.1),
}
ROUTES5 = list(CASES)
ZERO_ROW = 1      # the row whose weight is exactly 0 (both halves of the split keep rows with other weights)


def _weights(name, kind="pos"):
    B = CASES[name][1]
    if kind == "ones":
        return np.ones(B, np.float32)
    cyc = (0.25, 2.0, 1.0, 0.5) if kind == "pos" else (1.5, -0.5, 0.0, 0.75)
    r = np.array([cyc[b % 4] for b in range(B)], np.float32)
    if kind == "pos":
        r[ZERO_ROW] = 0.0
    return r


def _oracle(name):
    """The float64 oracle's train step on the weighted loss (the case's eps, the positive weights with one zero), computed once per process
    and case (the cache key of schedule_helpers.oracle_case holds the name), the logits and targets of its first forward pass, plus the
    UNWEIGHTED float64 loss of the same inputs and flags."""
    cfgf, B, T, D, L, V, drop, teach, _, eps = CASES[name]
    rec = []
    with RW.weighted_oracle(eps, _weights(name), record=rec):
        o = SH.oracle_case(name, cfgf, B, T, D, L, V, drop, teach)
    if "steps" not in o:
        o["steps"] = rec[:L - 1]      # (the float64 model's first forward pass comes first)
        o["loss_plain"] = _oracle_run(name, o, np.ones(B))["loss"]
    return o


def _oracle_run(name, o, r):
    """Forward and backward of the float64 oracle on the case's inputs and recorded flags under the weights r: loss and raw gradients;
    cached in o."""
    key = ("run", tuple(np.asarray(r, np.float64).tolist()))
    if key not in o:
        from oracle import ast_ref as R
        V, eps = CASES[name][5], CASES[name][9]
        m = R.RefModel(o["cfg"], {k: v.astype(np.float64) for k, v in o["P"].items()}, V)
        with RW.weighted_oracle(eps, r):
            lp = m.forward_loss(o["X"].astype(np.float64), o["y"], 0.5, pyrandom=SH._Fixed(o["flags"]))
            assert list(m.use_truth) == list(o["flags"])
            m.cleargrads()
            lp.backward()
        o[key] = dict(loss=float(lp.data), grads={k: p.grad.copy() for k, p in m.params()})
    return o[key]


_NO_KW = object()


def _gpu_step(lib, name, r, scheme="bf16x3", with_opt=False, deterministic=False):
    """One train step (forward, backward, optionally the optimizer's clip norm) of a fresh model on the case's inputs and flags under the
    row weights r (None; _NO_KW: the keyword omitted)."""
    from ast_amd.seq2seq import using_config
    cfgf, B, T, D, L, V, drop, teach, route, eps = CASES[name]
    o = _oracle(name)
    g = SH.gpu_model(o["cfg"], o["P"], D, V)
    g.gemm_precision = scheme
    g.deterministic = deterministic
    g.inject["use_truth"] = o["flags"]
    opt = SH.gpu_optimizer(g, SH.OPT) if with_opt else None
    kw = {} if r is _NO_KW else {"row_weight": None if r is None else torch.from_numpy(np.asarray(r, np.float32)).cuda()}
    with using_config("train", True):
        loss = g.forward_loss(X=torch.from_numpy(o["X"]), y=torch.from_numpy(o["y"]), teach_ratio=teach, random_out=0, label_smoothing=eps, **kw)
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


@pytest.mark.parametrize("name", ROUTES5)
def test_weighted_train_step_against_the_patched_oracle(lib, name, gemm_scheme):
    """Forward, backward and clip norm under positive weights cycling (0.25, 2, 1, 0.5) with one row at exactly 0 against the float64
    oracle on the weighted loss, within the project's bounds for a train step (schedule_helpers.assert_first_step_against_oracle: loss
    and clip norm 1e-4, every gradient 3e-4), on the per-launch loop, the persistent loop (two and three layers), the row split and the
    wide loop -- each asserted through astk_decoder_path.  Validity, on the oracle alone: the weights move the case's loss by at least
    20 x the loss bound."""
    o = _oracle(name)
    assert abs(o["loss"] - o["loss_plain"]) >= 2e-3 * abs(o["loss"]), (name, o["loss"], o["loss_plain"])
    if name == "tiny-rw":
        assert 0 in o["flags"], "the case should feed at least one argmax back"
    r = _gpu_step(lib, name, _weights(name), scheme=gemm_scheme, with_opt=True)
    print(name, gemm_scheme, "loss", r["loss"], o["loss"], "plain", o["loss_plain"], "gnorm", r["gnorm"], o["gnorm"])
    SH.assert_first_step_against_oracle(name, o, r["loss"], r["gnorm"], r["enc"], r["grads"])


# ------------------------------------------------------------------ 3. mixed signs
@pytest.mark.parametrize("name", ["mid-rw", "split-rw"])
def test_mixed_signs_within_the_bounds_of_the_magnitudes(lib, name):
    """Weights cycling (1.5, -0.5, 0, 0.75): the rows' errors add up with the magnitudes, not with the signed sum, so the loss is
    bounded by 1e-4 of the oracle's loss under |r| and each gradient tensor's error norm by 3e-4 of that tensor's norm under |r|."""
    r = _weights(name, "mixed")
    o = _oracle(name)
    want, mag = _oracle_run(name, o, r), _oracle_run(name, o, np.abs(r))
    got = _gpu_step(lib, name, r)
    print(name, "loss", got["loss"], want["loss"], "under |r|", mag["loss"])
    assert abs(got["loss"] - want["loss"]) <= 1e-4 * abs(mag["loss"])
    assert abs(want["loss"]) < 0.9 * abs(mag["loss"]), "the signs should cancel part of the loss"
    for k, g in want["grads"].items():
        err = np.sqrt(((got["grads"][k] - g) ** 2).sum())
        tol = 3e-4 * np.sqrt((mag["grads"][k] ** 2).sum())
        print(name, k, "err norm", err, "tol", tol)
        assert err <= tol, f"{name}: grad {k}: err norm {err:.3e} tol {tol:.3e}"


# ------------------------------------------------------------------ 4. all-ones weights and no weights are the step it always was
@pytest.mark.parametrize("name", ROUTES5)
def test_ones_none_and_the_omitted_keyword_are_one_step(lib, name):
    a = _gpu_step(lib, name, _NO_KW, deterministic=True)
    b = _gpu_step(lib, name, None, deterministic=True)
    c = _gpu_step(lib, name, _weights(name, "ones"), deterministic=True)
    assert a["bits"] == b["bits"] and torch.equal(a["arena"], b["arena"]) and torch.equal(a["pred"], b["pred"])
    assert a["bits"] == c["bits"] and torch.equal(a["pred"], c["pred"])
    assert torch.equal(a["arena"], c["arena"])
    # ... and that loss is the UNWEIGHTED oracle's (1e-4, the train step's bound)
    assert SH.rel(a["loss"], a["o"]["loss_plain"]) < 1e-4


# ------------------------------------------------------------------ 5. the zero-weight row
@pytest.mark.parametrize("name", ROUTES5)
def test_zero_weight_row_and_the_closed_form_of_the_out_bias_gradient(lib, name):
    """Under the weights of test 2 `pred` is the unweighted call's (so every fed-back token and every logit is), and d(out/b) =
    sum_{s,b} r_b w[t] c (softmax - (1 - eps) onehot - eps / V) formed in float64 from the oracle's logits, the zero row adding nothing,
    within 3e-4 of max |d(out/b)|."""
    B, V, eps = CASES[name][1], CASES[name][5], CASES[name][9]
    r = _weights(name)
    a, b = _gpu_step(lib, name, None), _gpu_step(lib, name, r)
    assert torch.equal(a["pred"], b["pred"])
    o = b["o"]
    w = np.ones(V)
    w[0] = 0.0                                                   # mask_pad_id
    want = np.zeros(V)
    for x, t in o["steps"]:
        g = RW.weighted_grad(x, t, w, r, eps, B)
        assert np.abs(g[ZERO_ROW]).max() == 0.0
        want += g.sum(axis=0)
    got = b["grads"]["out/b"].astype(np.float64)
    scale = np.abs(got).max()
    print(name, "closed form err", np.abs(got - want).max(), "of", scale)
    assert np.abs(got - want).max() <= 3e-4 * scale
    assert np.abs(got - a["grads"]["out/b"]).max() > 10 * 3e-4 * scale      # (the weights move it well above the bound)
    assert b["loss"] != a["loss"]


# ------------------------------------------------------------------ 6. reproducibility of the last-block sum
def test_weighted_persistent_step_is_reproducible(lib):
    """126 blocks of k_decoder_post rewrite their loss rows and the last to arrive sums them, in index order: the loss bits do not depend
    on which block that is; in deterministic mode the gradients are bit-equal too."""
    runs = [_gpu_step(lib, "persist-h64-rw", _weights("persist-h64-rw"), deterministic=True) for _ in range(2)]
    assert runs[0]["bits"] == runs[1]["bits"]
    assert torch.equal(runs[0]["arena"], runs[1]["arena"])
    assert np.isfinite(runs[0]["loss"]) and runs[0]["loss"] > 0
