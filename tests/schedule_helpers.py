"""Shared by the whole-step GPU tests (tests/test_gpu_model.py, tests/test_gpu_schedules.py): the train-step parity check against the
float64 oracle as a function of the SCHEDULE it runs under -- the stream the step is launched on and a dict of tuning knobs -- plus the
small helpers the schedule tests need: the side-stream plan query, the status word, the stream probe's skip."""
import contextlib
import copy
import ctypes as C
import random

import numpy as np
import pytest
import torch

OPT = {"type": 0, "lr": 1e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []}


def with_offset(X, x_offset):
    """X + x_offset (0.5 + d / D) per frequency bin d (float32): features that are not mean-normalised -- BatchNorm channels of layer 0
    whose mean lies far from 0 (tests/range_cases.py cnn_draws uses the same rule)."""
    if not x_offset:
        return X
    D = X.shape[-1]
    return (X + np.float32(x_offset) * (0.5 + np.arange(D, dtype=np.float32) / D)).astype(np.float32)


def make_inputs(cfg, B, T, D, L, V, seed=0, x_offset=0.0):
    from oracle import ast_ref as R
    P = R.init_params(cfg, D, V, seed=seed, dtype=np.float32)
    X, y = R.synth_batch(B, T, D, L, V, seed=seed + 1, dtype=np.float32)
    return P, with_offset(X, x_offset), y


def gpu_model(cfg, P, D, V):
    from ast_amd.seq2seq import SpeechEncoderDecoder
    c = copy.deepcopy(cfg)
    c["rnn_config"]["dec_vocab_size"] = V
    m = SpeechEncoderDecoder(0, c)
    m.materialize(D, values=P)
    return m


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-12)


class _Fixed:
    """Replays a recorded teacher-forcing flag sequence through the `random.random() < ratio` test (ratio 0.5)."""

    def __init__(s, flags): s.it = iter(flags[1:-1])
    def random(s): return 0.0 if next(s.it) else 1.0


_ORACLE = {}


def _opt_key(opt_cfg):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in opt_cfg.items()))


def oracle_case(name, cfgf, B, T, D, L, V, drop, teach, x_offset=0.0, opt_cfg=None):
    """The float64 (reference truth) and float32 (what Chainer-on-NumPy would compute) oracle results of one parity case: computed once per
    process and shared -- by the three arithmetic schemes and by every schedule the case runs under -- and never changed afterwards.
    `opt_cfg`: the optimizer section of the experiment config (None: OPT); part of the cache key."""
    opt_cfg = OPT if opt_cfg is None else opt_cfg
    key = (name, B, T, D, L, V, drop, teach, x_offset, _opt_key(opt_cfg))
    if key in _ORACLE:
        return _ORACLE[key]
    from oracle import ast_ref as R
    cfg = cfgf(drop)
    P, X, y = make_inputs(cfg, B, T, D, L, V, x_offset=x_offset)
    res = {}
    for dt in (np.float64, np.float32):
        m = R.RefModel(cfg, {k: v.astype(dt) for k, v in P.items()}, V)
        rec = R.RecordingMasks(3) if drop > 0 else None
        if rec:
            m.masks = rec
        noise = np.random.default_rng(9).normal(1.0, 0.25, X.shape).astype(np.float32) if drop > 0 else None
        opt = R.RefOptimizer(m, opt_cfg)
        rnd = random.Random("seed-ast-20h")
        loss, _ = R.train_step(m, opt, X.astype(dt), y, teach, add_noise=0.25 if drop > 0 else 0, noise=noise, pyrandom=rnd)
        res[dt] = dict(loss=loss, gnorm=opt.last_grad_norm, model=m, opt=opt, flags=list(m.use_truth), rec=rec, noise=noise,
                       enc=m.enc_states.data.copy())
    ref = res[np.float64]
    # note: after update() the oracle's grads include decay and clip; recompute raw grads for the per-tensor check
    m2 = R.RefModel(cfg, {k: v.astype(np.float64) for k, v in P.items()}, V)
    if drop > 0:
        m2.masks = lambda shape, ratio, tag: ref["rec"].masks[tag]
    l2 = m2.forward_loss(X.astype(np.float64), y, 0.5, add_noise=0.25 if drop > 0 else 0, noise=ref["noise"], pyrandom=_Fixed(ref["flags"]))
    m2.cleargrads()
    l2.backward()
    grads = {k: p.grad.copy() for k, p in m2.params()}
    # ---- two more steps (no dropout, all teacher-forced)
    mo = ref["model"]
    nodrop = copy.deepcopy(mo.cfg)
    nodrop["dropout"] = {"embed": 0.0, "rnn": 0.0, "out": 0}
    mo.cfg = nodrop
    more, later = [], []
    for step in range(2):
        X2, y2 = R.synth_batch(B, T, D, L, V, seed=100 + step, dtype=np.float32)
        X2 = with_offset(X2, x_offset)
        more.append((X2, y2))
        later.append(R.train_step(mo, ref["opt"], X2.astype(np.float64), y2, 1.0, pyrandom=random.Random(1))[0])
    out = dict(cfg=cfg, P=P, X=X, y=y, loss=ref["loss"], gnorm=ref["gnorm"], loss_f32=res[np.float32]["loss"], flags=ref["flags"],
               rec=ref["rec"], noise=ref["noise"], enc=ref["enc"], grads=grads, more=more, later=later,
               after={k: p.data.copy() for k, p in mo.params()},
               bn={f"CNN_{i}_bn/{s}": np.array(mo.p[f"CNN_{i}_bn/{s}"]) for i in range(len(cfg["cnn_config"]["cnn_layers"]))
                   for s in ("avg_mean", "avg_var")})
    _ORACLE[key] = out
    return out


def assert_first_step_against_oracle(name, o, lv, gnorm, enc, grads):
    """The project's bounds for one train step against the float64 oracle: encoder states 2e-4 of their maximum, loss and clip norm 1e-4,
    every gradient 3e-4 of max(tensor max, 1e-3 global max).  (gnorm None: the step ran without an optimizer.)"""
    np.testing.assert_allclose(enc, o["enc"], rtol=0, atol=2e-4 * np.abs(o["enc"]).max(), err_msg="enc_states")
    assert rel(lv, o["loss"]) < 1e-4, (name, lv, o["loss"])
    if gnorm is not None:
        assert rel(gnorm, o["gnorm"]) < 1e-4, (name, gnorm, o["gnorm"])
    # the f32 oracle itself sits this far from the f64 one (context for the tolerance)
    assert rel(o["loss_f32"], o["loss"]) < 1e-4
    gmax = max(np.abs(g).max() for g in o["grads"].values())
    for k, g in o["grads"].items():
        err = np.abs(grads[k] - g).max()
        tol = 3e-4 * max(np.abs(g).max(), 1e-3 * gmax)
        assert err <= tol, f"{name}: grad {k}: err {err:.3e} tol {tol:.3e}"


def gpu_optimizer(model, opt_cfg):
    """init_optimizer (nn.py:81-119) on the HIP path from the optimizer section of the experiment config: Adam (AMSGrad) for type 0, SGD
    otherwise; WeightDecay, GradientClipping, GradientNoise in the reference's order; disable_update() on the frozen links."""
    from ast_amd import optimizers as O
    opt = O.Adam(alpha=opt_cfg["lr"], beta1=0.9, beta2=0.999, eps=1e-8, amsgrad=True) if opt_cfg["type"] == 0 else O.SGD(lr=opt_cfg["lr"])
    opt.setup(model)
    if opt_cfg["l2"] > 0:
        opt.add_hook(O.WeightDecay(opt_cfg["l2"]))
    opt.add_hook(O.GradientClipping(opt_cfg["grad_clip"]))
    if opt_cfg.get("grad_noise_eta", 0) > 0:
        opt.add_hook(O.GradientNoise(opt_cfg["grad_noise_eta"]))
    for link in opt_cfg.get("freeze", []):
        model[link].disable_update()
    return opt


def train_step_parity(name, cfgf, B, T, D, L, V, drop, teach, gemm_scheme, stream=None, knobs=None, inspect=None, x_offset=0.0,
                      opt_cfg=None):
    """One train step of the HIP path against the float64 oracle, two more updates, the parameter deltas and the BatchNorm statistics.
    `stream`: the torch stream the model runs on (None: the current one -- the legacy default stream in the suite); `knobs`: tuning knobs
    in force for the GPU steps (astk_set_tuning; restored afterwards); `inspect(model)`: called behind the first step, inside the knobs;
    `x_offset`: a per-bin offset on the features (with_offset); `opt_cfg`: the optimizer section of the experiment config (None: OPT),
    for the oracle and for the HIP path alike -- frozen links must come out of the three updates bit for bit as they went in."""
    from oracle.ast_ref_torch import masks_from_recording
    from ast_amd import _lib
    from ast_amd.seq2seq import using_config
    opt_cfg = OPT if opt_cfg is None else opt_cfg
    assert opt_cfg.get("grad_noise_eta", 0) == 0, "the oracle's gradient noise is another random stream: no parity to check"
    o = oracle_case(name, cfgf, B, T, D, L, V, drop, teach, x_offset, opt_cfg)
    cfg, P, X, y = o["cfg"], o["P"], o["X"], o["y"]
    on_stream = torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()
    with _lib.tuning(knobs or {}), on_stream:
        # ---- HIP path
        g = gpu_model(cfg, P, D, V)
        g.gemm_precision = gemm_scheme
        T2 = o["enc"].shape[1]
        if drop > 0:
            packed = masks_from_recording(cfg, o["rec"].masks, T2, L - 1, B)
            g.inject = {k: torch.from_numpy(v) for k, v in packed.items()}
            g.inject["noise"] = torch.from_numpy(o["noise"])
        g.inject["use_truth"] = o["flags"]
        opt = gpu_optimizer(g, opt_cfg)
        with using_config("train", True):
            loss = g.forward_loss(X=torch.from_numpy(X), y=torch.from_numpy(y), teach_ratio=teach, random_out=0,
                                  add_noise=0.25 if drop > 0 else 0)
            g.cleargrads()
            loss.backward()
            grads = g.arena.to_numpy(grads=True)
            opt.update()
        torch.cuda.synchronize()
        lv = float(loss.data)
        if inspect is not None:
            inspect(g)
        assert_first_step_against_oracle(name, o, lv, opt.last_grad_norm, g.enc_states.cpu().numpy(), grads)
        # ---- two more steps (no dropout, all teacher-forced), then compare losses and the parameter deltas
        for step in range(2):
            X2, y2 = o["more"][step]
            g.inject = {"use_truth": [1] * (L - 1), "enc_masks": None, "emb_mask": None, "rnn_masks": None}
            with using_config("train", True):
                ls = g.forward_loss(X=torch.from_numpy(X2), y=torch.from_numpy(y2), teach_ratio=1.0)
                g.cleargrads()
                ls.backward()
                opt.update()
            lref = o["later"][step]
            assert rel(float(ls.data), lref) < 2e-3, (name, step, float(ls.data), lref)
        torch.cuda.synchronize()
        after = g.arena.to_numpy()
    num = den = 0.0
    for k, p in o["after"].items():
        if k.split("/")[0] in opt_cfg.get("freeze", []):
            assert np.array_equal(after[k].view(np.uint32), P[k].view(np.uint32)) and np.array_equal(p, P[k]), f"{name}: frozen {k} moved"
        num += float(((after[k].astype(np.float64) - p) ** 2).sum())
        den += float(((p - P[k]) ** 2).sum())
    # AMSGrad's first steps move every weight by ~lr*sign(g): elements whose gradient is below f32 noise may flip
    assert np.sqrt(num / den) < 5e-2, f"{name}: parameter delta after 3 updates off by {np.sqrt(num / den):.3e} (relative L2)"
    # BN running statistics follow Chainer-sem A4
    for k, v in o["bn"].items():
        np.testing.assert_allclose(g.persist[k].cpu().numpy(), v, rtol=2e-3, atol=1e-5)
    return g


# ------------------------------------------------------------------ the schedule tests' small helpers
def side_plan(ld):
    """(forward head steps, forward chunks, backward chunks) the library plans for this encoder-stack descriptor, under the knobs in force."""
    from ast_amd import _lib
    head, fc, bc = C.c_int(), C.c_int(), C.c_int()
    _lib.check(_lib.load().astk_lstm_stack_side_plan(C.byref(ld), C.byref(head), C.byref(fc), C.byref(bc)))
    return head.value, fc.value, bc.value


def require_side(m):
    """The model ran on a stream of its own with side-stream work allowed: it must have found its second stream -- unless the probe found no
    stream that executes concurrently with the compute stream on this device (then the schedule under test cannot run: skip)."""
    if m._side is None and m._side_by_main and all(v is None for v in m._side_by_main.values()):
        pytest.skip("no pair of concurrently executing streams on this device")
    assert m._side is not None, "the side stream was not used"


def status_word():
    """The sticky status word of the persistent kernels' bounded hand-offs (0 = no time-out anywhere), read and reset."""
    from ast_amd import _lib
    mask = C.c_uint(0)
    assert _lib.load().astk_persist_status(C.byref(mask), 1) == 0
    return mask.value
