"""Greedy decoding on the device (include/astk.h astk_greedy_decode: the persistent decoder loop in its greedy mode, one launch per
batch) against the float64 oracle's predict and against the per-step GPU loop (astk_decoder_step_infer): the stop rule, long runs over
streamed attention slices, state left behind, the shapes that fall back to the loop, argument checks and NN.predict end to end.

Token comparisons are exact, guarded by the argmax margin at every compared step: `Wo` is scaled (the goldens' out_scale 8) so that the
top-2 gap is far above float32 rounding, and the margin is asserted as a precondition, so a comparison can never pass vacuously."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from decode_helpers import CFG1, EOS, ES_EN, GO, MID, WIDE, setup as _setup

pytestmark = pytest.mark.gpu


def _loop(m, X, stop_limit, eos_dist=None):
    """The per-step GPU loop of predict() with its logits kept: tokens (B, n) and the top-2 gap of every (step, row); eos_dist (a list):
    receives the distance of every step's maximum to the EOS logit."""
    from ast_amd.seq2seq import using_config
    with using_config("train", False):
        m.encode(torch.from_numpy(X))
        m.init_decoder_state()
        B = X.shape[0]
        ht = torch.zeros(B, m.A, dtype=torch.float32, device=m.device)
        word = torch.full((B,), GO, dtype=torch.int32, device=m.device)
        done = torch.zeros(B, dtype=torch.bool, device=m.device)
        rows, gaps = [], []
        for _ in range(stop_limit):
            logits, ht, _ = m.decode_step(word, ht)
            top = torch.topk(logits, 2, dim=1).values
            gaps.append((top[:, 0] - top[:, 1]).cpu().numpy())
            if eos_dist is not None:
                eos_dist.append((top[:, 0] - logits[:, EOS]).cpu().numpy())
            word = logits.argmax(dim=1).to(torch.int32)
            rows.append(word)
            done |= word == EOS
            if bool(done.all()):
                break
    return torch.stack(rows, 0).T.cpu().numpy(), np.stack(gaps, 0)


def _device(m, X, stop_limit):
    got = m.predict(torch.from_numpy(X), GO, EOS, stop_limit)
    assert m.last_predict_path == "device"
    return got


def _compare_guarded(got, ref, gaps, thr, min_frac):
    """Row by row up to the first step whose top-2 gap is below thr: equal; at least min_frac of the positions compared."""
    n_cmp, n_all = 0, 0
    for b in range(ref.shape[0]):
        n_all += ref.shape[1]
        k = ref.shape[1]
        low = np.nonzero(gaps[:, b] < thr)[0]
        if len(low):
            k = int(low[0])
        assert (got[b, :k] == ref[b, :k]).all(), (b, got[b, :k], ref[b, :k])
        n_cmp += k
    assert n_cmp >= min_frac * n_all, f"only {n_cmp} of {n_all} positions have a top-2 gap >= {thr}"


# ---------------------------------------------------------------- oracle parity at full size
def _oracle_greedy(cfg, P, X, V, stop_limit):
    from oracle import ast_ref as R
    m = R.RefModel(cfg, {k: v.astype(np.float64) for k, v in P.items()}, V)
    m.train = False
    B = X.shape[0]
    m.encode(X.astype(np.float64))
    m.init_decoder_state()
    ht = R.Variable(np.zeros((B, cfg["rnn_config"]["attn_units"])))
    word = np.full((B,), GO, dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    rows, gaps = [], []
    for step in range(stop_limit):
        logits, ht, _ = m.decode_step(word, ht, step=step)
        lg = np.asarray(logits.data)
        srt = np.sort(lg, axis=1)
        gaps.append(srt[:, -1] - srt[:, -2])
        word = lg.argmax(axis=1).astype(np.int32)
        rows.append(word)
        done[word == EOS] = True
        if done.all():
            break
    return np.stack(rows, 0).T, np.stack(gaps, 0)


@pytest.mark.parametrize("shape", [CFG1, ES_EN], ids=["configs1", "es_en_20h"])
def test_greedy_matches_oracle_full_size(shape):
    """B = 32, 800 frames (T'' = 200: the slices stay resident in LDS), both decoder depths of the H = 512 attention phase."""
    cfg, P, X, m = _setup(shape, 32, 800, seed=3)
    ref, gaps = _oracle_greedy(cfg, P, X, shape["V"], 40)
    got = _device(m, X, 40)
    assert got.shape == ref.shape
    _compare_guarded(got, ref, gaps, 1e-3, 0.9)


# ---------------------------------------------------------------- the stop rule against the per-step loop
def _first_eos(tokens):
    return [int(np.nonzero(r == EOS)[0][0]) if (r == EOS).any() else -1 for r in tokens]


@pytest.mark.parametrize("B", [1, 7, 16, 17, 32])
def test_stop_rule_matches_step_loop(B, tune):
    stop = 24
    # every row at EOS on step 0: one column
    _, _, X, m = _setup(MID, B, 120, seed=5, eos_bias=1e4)
    got = _device(m, X, stop)
    assert got.shape == (B, 1) and (got == EOS).all()
    # no EOS ever: stop_limit columns; and stop_limit = 1
    _, _, X, m = _setup(MID, B, 120, seed=5, eos_bias=-1e4)
    dist = []
    ref, gaps = _loop(m, X, stop, dist)
    assert ref.shape == (B, stop) and gaps.min() > 1e-4
    assert (_device(m, X, stop) == ref).all()
    got1 = _device(m, X, 1)
    assert got1.shape == (B, 1) and (got1 == ref[:, :1]).all()
    # rows finishing at different steps: n < stop_limit, the early rows' post-EOS tokens equal too.  Until its first EOS a row follows
    # the run above, so an EOS offset just above max over rows of (min over the first steps of the distance of the maximum to the EOS
    # logit) makes every row finish, each at its own step
    d = np.stack(dist, 0)[: stop - 2] - 1e4
    best = None
    for cand in np.unique(np.round(d, 3)) + 0.25:
        below = d < cand
        if below.any(axis=0).all():
            fe_c = below.argmax(axis=0)
            score = len(set(fe_c.tolist()))
            if best is None or score > best[0]:
                best = (score, float(cand))
    assert best is not None and (B == 1 or best[0] > 1), best
    bias = best[1]
    _, _, X, m = _setup(MID, B, 120, seed=5, eos_bias=bias)
    ref, gaps = _loop(m, X, stop)
    fe = _first_eos(ref)
    assert ref.shape[1] < stop and min(fe) >= 0 and (B == 1 or len(set(fe)) > 1), fe
    assert gaps.min() > 1e-4, gaps.min()
    got = _device(m, X, stop)
    assert got.shape == ref.shape and (got == ref).all(), (got, ref)
    # the same through predict() on the loop (dec.persist = 0)
    tune("dec.persist", 0)
    assert (m.predict(torch.from_numpy(X), GO, EOS, stop) == ref).all() and m.last_predict_path == "steps"


# ---------------------------------------------------------------- long runs: resident and streamed attention slices
@pytest.mark.parametrize("shape,T2", [(ES_EN, 200), (ES_EN, 224), (ES_EN, 232), (ES_EN, 420), (CFG1, 232)],
                         ids=["es_en_20h-200", "es_en_20h-224", "es_en_20h-232", "es_en_20h-420", "configs1-232"])
def test_long_runs_match_step_loop(shape, T2):
    """At B = 32, T'' = 224 is the last length whose slices stay resident in LDS (chunk 28), 232 the first streamed one, 420 the loader's
    longest bucket (1680 frames)."""
    _, _, X, m = _setup(shape, 32, 4 * T2, seed=7, eos_bias=-1e4)
    got = _device(m, X, 175)
    assert m._cur["T2"] == T2
    ref, gaps = _loop(m, X, 175)
    assert got.shape == ref.shape == (32, 175)
    _compare_guarded(got, ref, gaps, 1e-5, 0.9)


# ---------------------------------------------------------------- state
def test_predict_is_repeatable_and_leaves_no_state():
    from ast_amd import _lib
    from ast_amd.seq2seq import using_config
    from oracle import ast_ref as R
    cfg, P, X, m = _setup(MID, 17, 120, seed=9, eos_bias=8.0)
    a = _device(m, X, 30)
    b = _device(m, X, 30)
    assert a.dtype == np.int32 and (a == b).all()
    mask = C.c_uint(7)
    assert _lib.load().astk_persist_status(C.byref(mask), 0) == 0 and mask.value == 0
    # a train step after predict gives the same bits as on a model that never predicted
    _, _, _, fresh = _setup(MID, 17, 120, seed=9, eos_bias=8.0)
    Xt, yt = R.synth_batch(17, 120, 80, 9, MID["V"], seed=21, dtype=np.float32)
    out = []
    for g in (m, fresh):
        g.deterministic = True                # (every gradient sum in a fixed order: two runs compare to the bit)
        g.inject = {"use_truth": [1] * 8, "enc_masks": None, "emb_mask": None, "rnn_masks": None}
        with using_config("train", True):
            loss = g.forward_loss(torch.from_numpy(Xt), torch.from_numpy(yt), 1.0)
            g.cleargrads()
            loss.backward()
        torch.cuda.synchronize()
        out.append((float(loss.data), g.arena.grad.clone()))
    assert out[0][0] == out[1][0]
    assert torch.equal(out[0][1], out[1][1])


# ---------------------------------------------------------------- fallbacks
@pytest.mark.parametrize("over,B", [({"ln": True}, 4), ({"n_attn": 2}, 4), ({"feed_attn": False}, 4), ({}, 48)],
                         ids=["ln", "n_attn2", "no_feed_attn", "B48"])
def test_fallback_shapes_take_the_step_loop(over, B):
    from ast_amd import _lib
    _, _, X, m = _setup(MID, B, 120, seed=11, **over)
    got = m.predict(torch.from_numpy(X), GO, EOS, 6)
    assert m.last_predict_path == "steps" and got.shape[0] == B
    assert _lib.load().astk_greedy_workspace_bytes(C.byref(m._cur["dd"]), 6) == 0


def test_wide_decoder_takes_the_step_loop():
    from ast_amd import _lib
    _, _, X, m = _setup(WIDE, 4, 120, seed=11)
    got = m.predict(torch.from_numpy(X), GO, EOS, 6)
    assert m.last_predict_path == "steps" and got.shape[0] == 4
    assert _lib.load().astk_greedy_workspace_bytes(C.byref(m._cur["dd"]), 6) == 0
    d = _lib.DecoderDesc(32, 2, 200, 1024, 128, 1024, 1098, 1, 1, 0, 0)
    assert _lib.load().astk_greedy_workspace_bytes(C.byref(d), 175) == 0
    d = _lib.DecoderDesc(32, 2, 200, 512, 128, 512, 1098, 3, 1, 0, 0)
    assert _lib.load().astk_greedy_workspace_bytes(C.byref(d), 175) > 0
    assert _lib.load().astk_greedy_workspace_bytes(C.byref(d), 513) == 0
    assert _lib.load().astk_greedy_workspace_bytes(C.byref(d), 0) == 0


# ---------------------------------------------------------------- bad arguments
def test_bad_arguments_fail_with_a_message():
    from ast_amd import _lib
    from ast_amd.seq2seq import using_config
    lib = _lib.load()
    _, _, X, m = _setup(MID, 4, 120, seed=13)
    with using_config("train", False):
        m.encode(torch.from_numpy(X))
        m.init_decoder_state()
    st = m._cur
    dd = _lib.DecoderDesc.from_buffer_copy(st["dd"])
    nbytes = lib.astk_greedy_workspace_bytes(C.byref(dd), 10)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=m.device)
    toks = torch.empty(10 * 4, dtype=torch.int32, device=m.device)
    nst = torch.zeros(4, dtype=torch.int32, device=m.device)

    def call(d=dd, go=GO, eos=EOS, stop=10, wsz=nbytes):
        return lib.astk_greedy_decode(C.byref(d), C.byref(st["dp"]), C.c_void_p(st["enc_states"].data_ptr()), C.c_void_p(m._dec_c.data_ptr()),
                                      C.c_void_p(m._dec_h.data_ptr()), go, eos, stop, C.c_void_p(toks.data_ptr()), C.c_void_p(nst.data_ptr()),
                                      None, C.c_void_p(ws.data_ptr()), wsz, None)
    bad = _lib.DecoderDesc.from_buffer_copy(dd)
    bad.struct_size -= 8
    wide = _lib.DecoderDesc.from_buffer_copy(dd)
    wide.ln = 1
    for kw, word in ((dict(d=bad), b"struct_size"), (dict(go=-1), b"go"), (dict(go=MID["V"]), b"go"), (dict(eos=MID["V"]), b"eos"),
                     (dict(stop=0), b"stop_limit"), (dict(d=wide), b"device loop"), (dict(wsz=nbytes - 1), b"workspace too small")):
        assert call(**kw) < 0, kw
        assert word in lib.astk_last_error(), (kw, lib.astk_last_error())
    torch.cuda.synchronize()
    assert call() == 0
    torch.cuda.synchronize()
    assert 1 <= int(nst[0]) <= 10


# ---------------------------------------------------------------- NN.predict end to end
def test_nn_predict_same_with_and_without_the_device_loop(tune):
    """NN.predict (two read-back buffers, a batch read one batch late) on a decoder of the shipped shape: the same predictions
    with dec.persist on (device loop) and off (per-step loop)."""
    from ast_amd import nn as gnn
    _, _, _, m = _setup(ES_EN, 8, 240, seed=15, eos_bias=3.0)
    rng = np.random.default_rng(0)
    batches = []
    for i, (B, T) in enumerate(((8, 240), (5, 320), (8, 200), (3, 400))):
        batches.append({"X": rng.standard_normal((B, T, 80)).astype(np.float32), "utts": [f"u{i}_{j}" for j in range(B)]})
    # precondition: the per-step loop's top-2 gap on every step of these batches is far above the rounding of either path
    for b in batches:
        _, gaps = _loop(m, b["X"], 30)
        assert gaps.min() > 1e-4, gaps.min()
    stub = types.SimpleNamespace(model=m, cfg=types.SimpleNamespace(train={"data": {"max_pred": 30}, "batch_size": 8}),
                                 data_loader=types.SimpleNamespace(n_utts={"dev": sum(len(b["utts"]) for b in batches)},
                                                                   get_batch=lambda *a, **k: iter(batches)))
    on = gnn.NN.predict(stub, "dev")
    assert m.last_predict_path == "device"
    tune("dec.persist", 0)
    off = gnn.NN.predict(stub, "dev")
    assert m.last_predict_path == "steps"
    assert [u for u, _ in on] == [u for u, _ in off]
    assert on == off
