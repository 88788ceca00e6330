"""Sampled decoding on the device (include/astk.h astk_sample_decode: the persistent decoder loop in its sampled mode, Gumbel-max draws;
SpeechEncoderDecoder.sample, ast_amd.nn.sample_hypotheses, sample.py) against the float64 oracle's decode_step in a sampled loop that
draws with the NumPy restatement of the noise (tests/sample_noise_model.py), against the per-step GPU loop, and against forced decoding;
what it must leave untouched; fallbacks and bad arguments.

The recipes are those of tests/test_gpu_greedy_scored.py, restated: token comparisons are exact and guarded by the top-2 gap of the
PERTURBED scores z = logits * inv_temp + g; log-probabilities are compared under tol(): max(2 * E_LOOP * max(1, 1 / temperature),
1e-4 * max(1, |value|)) -- logit errors scale with inv_temp.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import tiny_cfg
from decode_helpers import (CFG1, EOS, ES_EN, GO, MID, WIDE, guard as _guard, lse64 as _lse64, max_err as _max_err, setup as _setup,
                            tol)
from sample_noise_model import noise as _noise, row_key as _row_key

pytestmark = pytest.mark.gpu

SEED = 2024


def _keys(seed, streams):
    return np.array([_row_key(seed, int(s)) for s in streams], dtype=np.uint64)


def _inv(temperature):
    return float(np.float32(1.0 / temperature))


def _draw(lg, keys, step, inv_temp):
    """float64: one step's draw from logits lg (B, V) -- token, top-2 gap of the perturbed scores, log p(token), z."""
    xs = lg * inv_temp
    z = xs + _noise(keys[:, None], step, np.arange(lg.shape[1])[None, :])[2]
    srt = np.sort(z, axis=1)
    word = z.argmax(axis=1).astype(np.int32)
    return word, srt[:, -1] - srt[:, -2], xs[np.arange(lg.shape[0]), word] - _lse64(xs), z


def _oracle_sample(cfg, P, X, V, stop_limit, keys, temperature):
    """The oracle's decode_step in a sampled loop: each step feeds back argmax(lg * inv_temp + g), g from the restatement.  Returns
    tokens (B, n), the perturbed gaps and logp (n, B), and the oracle's plain argmax of every step (B, n)."""
    from oracle import ast_ref as R
    m = R.RefModel(cfg, {k: v.astype(np.float64) for k, v in P.items()}, V)
    m.train = False
    B = X.shape[0]
    m.encode(X.astype(np.float64))
    m.init_decoder_state()
    ht = R.Variable(np.zeros((B, cfg["rnn_config"]["attn_units"])))
    word = np.full((B,), GO, dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    rows, gaps, lps, greedy = [], [], [], []
    for step in range(stop_limit):
        logits, ht, _ = m.decode_step(word, ht, step=step)
        lg = np.asarray(logits.data)
        greedy.append(lg.argmax(axis=1))
        word, gap, lp, _ = _draw(lg, keys, step, _inv(temperature))
        rows.append(word)
        gaps.append(gap)
        lps.append(lp)
        done[word == EOS] = True
        if done.all():
            break
    return np.stack(rows, 0).T, np.stack(gaps, 0), np.stack(lps, 0), np.stack(greedy, 0).T


def _loop(m, X, stop_limit, keys, temperature, eos_dist=None):
    """The per-step GPU loop with its logits kept (float32 logits from decode_step, the draw in float64 on the host from the
    restatement's noise): tokens (B, n), the perturbed gaps and logp (n, B)."""
    from ast_amd.seq2seq import using_config
    with using_config("train", False):
        m.encode(torch.from_numpy(X))
        m.init_decoder_state()
        B = X.shape[0]
        ht = torch.zeros(B, m.A, dtype=torch.float32, device=m.device)
        word = torch.full((B,), GO, dtype=torch.int32, device=m.device)
        done = np.zeros(B, dtype=bool)
        rows, gaps, lps = [], [], []
        for step in range(stop_limit):
            logits, ht, _ = m.decode_step(word, ht)
            w, gap, lp, z = _draw(logits.double().cpu().numpy(), keys, step, _inv(temperature))
            if eos_dist is not None:
                eos_dist.append(z.max(axis=1) - z[:, EOS])
            rows.append(w)
            gaps.append(gap)
            lps.append(lp)
            word = torch.from_numpy(w).to(m.device)
            done |= w == EOS
            if done.all():
                break
    return np.stack(rows, 0).T, np.stack(gaps, 0), np.stack(lps, 0)


def _sample(m, X, stop_limit, streams=None, temperature=1.0, seed=SEED, path="device"):
    r = m.sample(torch.from_numpy(X), GO, EOS, stop_limit, seed, streams=streams, temperature=temperature)
    assert m.last_predict_path == path, m.last_predict_path
    assert r.nll is None and r.loss is None and r.tokens.dtype == np.int32 and r.logp.dtype == np.float32
    return r


def _status_is_clear():
    from ast_amd import _lib
    mask = C.c_uint(7)
    return _lib.load().astk_persist_status(C.byref(mask), 0) == 0 and mask.value == 0


def _first_eos_scores(tokens, lp):
    """float64 sum of lp (n, B) up to and including each row's first EOS."""
    B, n = tokens.shape
    return np.array([lp[:(int(np.nonzero(tokens[b] == EOS)[0][0]) + 1) if (tokens[b] == EOS).any() else n, b].sum() for b in range(B)])


# ---------------------------------------------------------------- 1. the noise fill
def test_gumbel_rows_match_the_restatement():
    from ast_amd import _lib
    from ast_amd.seq2seq import sample_row_key
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    streams = [(2024, 0), (2024, 31), (7, 3), ((1 << 64) - 1, 5), (0, 0), (123456789, 1 << 40)]
    keys = np.array([sample_row_key(a, b) for a, b in streams], dtype=np.uint64)
    assert [int(k) for k in keys] == [_row_key(a, b) for a, b in streams]
    assert all(int(lib.astk_sample_row_key(a, b)) == _row_key(a, b) for a, b in streams)
    kd = torch.from_numpy(keys.view(np.int64)).to(dev)
    worst = 0.0
    for V in (1098, 57):
        out = torch.full((len(keys), V), float("nan"), dtype=torch.float32, device=dev)
        for step in (0, 7, 511):
            assert lib.astk_gumbel_rows(C.c_void_p(kd.data_ptr()), len(keys), step, V, C.c_void_p(out.data_ptr()), None) == 0
            torch.cuda.synchronize()
            got = out.cpu().numpy().astype(np.float64)
            want = _noise(keys[:, None], step, np.arange(V)[None, :])[2]
            err = np.abs(got - want).max()
            worst = max(worst, err)
            print(f"V {V} step {step}: max abs err {err:.3e}, g range [{got.min():.3f}, {got.max():.3f}]")
            assert np.isfinite(got).all() and err <= 5e-6
    # the known answers of the contract, through the device function
    out = torch.empty(1, 1098, dtype=torch.float32, device=dev)
    k0 = torch.from_numpy(np.array([_row_key(2024, 0)], dtype=np.uint64).view(np.int64)).to(dev)
    assert lib.astk_gumbel_rows(C.c_void_p(k0.data_ptr()), 1, 7, 1098, C.c_void_p(out.data_ptr()), None) == 0
    v = float(out[0, 1097])
    print(f"g((2024, 0), 7, 1097) = {v:.9f} (0.279620615), largest error of the fill {worst:.3e}")
    assert abs(v - 0.279620615) <= 5e-6
    assert lib.astk_gumbel_rows(None, 1, 0, 57, C.c_void_p(out.data_ptr()), None) < 0 and b"null pointer" in lib.astk_last_error()


# ---------------------------------------------------------------- 2. oracle parity at full size
@pytest.mark.parametrize("shape,temperature", [(CFG1, 1.0), (CFG1, 0.5), (ES_EN, 1.0)], ids=["configs1-T1", "configs1-T0.5", "es_en_20h-T1"])
def test_sampled_matches_oracle_full_size(shape, temperature, tune):
    """The inputs of test_scored_matches_oracle_full_size, seed 2024, streams 0..31, 40 steps, EOS not forced.  The oracle alone gives a
    guarded share of 1.000 / 0.967 / 0.983 and differs from its own argmax at 0.89 / 0.49 / 0.96 of the positions.  Figures measured on
    one MI355X are in the result table of DESIGN.md section 14."""
    V = shape["V"]
    cfg, P, X, m = _setup(shape, 32, 800, seed=3)
    keys = _keys(SEED, range(32))
    ref, gaps, rlp, greedy = _oracle_sample(cfg, P, X, V, 40, keys, temperature)
    ok = _guard(ref, gaps, 1e-3)
    frac = ok.sum() / ok.size
    differ = float((ref != greedy).mean())
    print(f"\n{'es_en_20h' if shape is ES_EN else 'configs1'} T {temperature}: oracle n_steps {ref.shape[1]}, guarded {frac:.3f}, "
          f"min gap {gaps.min():.3e}, differs from argmax at {differ:.2f}")
    assert frac >= 0.9
    # the per-step fallback's own error against the oracle on the same positions: e_loop
    tune("dec.persist", 0)
    fb = _sample(m, X, 40, temperature=temperature, path="steps")
    tune("dec.persist", 1)
    n = min(fb.n_steps, ref.shape[1])
    okl = ok[:, :n]
    miss_l = int((fb.tokens[:, :n][okl] != ref[:, :n][okl]).sum())
    e1, _ = _max_err("per-step fallback logp vs oracle", fb.logp[:, :n], rlp[:n].T, okl, temperature)
    print(f"  e_loop = {e1:.3e}, per-step fallback token mismatches at guarded positions {miss_l}")
    got = _sample(m, X, 40, temperature=temperature)
    n = min(got.n_steps, ref.shape[1])
    okd = ok[:, :n]
    miss = int((got.tokens[:, :n][okd] != ref[:, :n][okd]).sum())
    _, r1 = _max_err("device logp vs oracle", got.logp[:, :n], rlp[:n].T, okd, temperature)
    dd = float((got.tokens[:, :n] != greedy[:, :n]).mean())
    distinct = len({tuple(r) for r in got.tokens.tolist()})
    print(f"  device n_steps {got.n_steps}, token mismatches at guarded positions {miss}, differs from the oracle's argmax at {dd:.2f}, "
          f"distinct rows {distinct}")
    assert miss_l == 0 and miss == 0
    assert r1 <= 1.0, r1
    assert dd > 0.3 and distinct == 32
    if ok.all():
        assert got.n_steps == ref.shape[1]
        want = _first_eos_scores(ref, rlp)
        print(f"  score: max abs err {np.abs(got.score - want).max():.3e}, max |value| {np.abs(want).max():.3f}")
        assert (np.abs(got.score - want) <= tol(want, temperature)).all()
    assert _status_is_clear()


# ---------------------------------------------------------------- 3. the device loop against the per-step fallback
def _compare_runs(tag, dev, fb, ok, temperature=1.0):
    """A device-loop sample against the fallback's under the guard `ok` (B, n of the fallback): tokens at guarded positions, n_steps
    when every position is guarded, logp at guarded positions and the scores of fully guarded rows within tol()."""
    n = min(dev.n_steps, fb.n_steps, ok.shape[1])
    okn = ok[:, :n]
    share = ok.sum() / ok.size
    print(f"  {tag}: n_steps {dev.n_steps} / {fb.n_steps}, guarded {share:.3f}")
    assert share >= 0.9, (tag, share)
    assert (dev.tokens[:, :n][okn] == fb.tokens[:, :n][okn]).all(), tag
    if ok.all():
        assert dev.n_steps == fb.n_steps == ok.shape[1] and (dev.tokens == fb.tokens).all(), tag
    _, worst = _max_err(f"{tag} logp", dev.logp[:, :n], fb.logp[:, :n].astype(np.float64), okn, temperature)
    assert worst <= 1.0, (tag, worst)
    full = ok.all(axis=1) if dev.n_steps == fb.n_steps == ok.shape[1] else np.zeros(ok.shape[0], dtype=bool)
    if full.any():
        err = np.abs(dev.score - fb.score)[full]
        print(f"  {tag} score: max abs err {err.max():.3e} over {int(full.sum())} fully guarded rows")
        assert (err <= tol(fb.score[full], temperature)).all(), tag


@pytest.mark.parametrize("B", [1, 5, 16, 17, 32])
def test_device_loop_matches_step_fallback(B, tune):
    stop = 24
    keys = _keys(SEED, range(B))
    # no EOS ever: the batch stops at stop_limit
    _, _, X, m = _setup(MID, B, 120, seed=5, eos_bias=-1e4)
    dist = []
    ref, gaps, _ = _loop(m, X, stop, keys, 1.0, eos_dist=dist)
    assert ref.shape == (B, stop)
    # ... and an EOS offset that lets every row draw EOS within the first steps, each at its own step: the smallest offsets at which the
    # perturbed EOS score passes the step's winner (the trajectory of a row is the same up to there)
    d = np.stack(dist, 0)[: stop - 2] - 1e4
    best = None
    for cand in np.unique(np.round(d, 3)) + 0.25:
        below = d < cand
        if below.any(axis=0).all():
            score = len(set(below.argmax(axis=0).tolist()))
            if best is None or score > best[0]:
                best = (score, float(cand))
    assert best is not None
    for case, bias in (("never", -1e4), ("early", best[1])):
        _, _, X, m = _setup(MID, B, 120, seed=5, eos_bias=bias)
        ref, gaps, _ = _loop(m, X, stop, keys, 1.0)
        n = ref.shape[1]
        assert n == stop if case == "never" else 1 <= n < stop, (case, n)
        print(f"\nB {B} {case}: n_steps {n}, min gap {gaps.min():.3e}")
        tune("dec.persist", 1)
        dev = _sample(m, X, stop)
        tune("dec.persist", 0)
        fb = _sample(m, X, stop, path="steps")
        tune("dec.persist", 1)
        ok = _guard(ref, gaps, 1e-4)
        nn_ = min(n, fb.n_steps)
        assert (fb.tokens[:, :nn_][ok[:, :nn_]] == ref[:, :nn_][ok[:, :nn_]]).all()
        if ok.all():
            assert fb.n_steps == n
        _compare_runs(f"B {B} {case}", dev, fb, ok)
        if case == "early" and ok.all():
            assert (dev.tokens == EOS).any(axis=1).all()       # every row has drawn EOS when the batch stops early
    assert _status_is_clear()


# ---------------------------------------------------------------- 4. one long run on the streamed slices
def test_long_run_on_streamed_slices_matches_step_fallback(tune):
    """T'' = 420 (the loader's longest bucket): the streamed-slice variant of the sampled kernel, 175 steps."""
    _, _, X, m = _setup(ES_EN, 32, 4 * 420, seed=7, eos_bias=-1e4)
    keys = _keys(SEED, range(32))
    dev = _sample(m, X, 175)
    assert m._cur["T2"] == 420
    ref, gaps, lp = _loop(m, X, 175, keys, 1.0)
    assert dev.tokens.shape == ref.shape == (32, 175)
    ok = _guard(ref, gaps, 1e-5)
    print(f"\nlong run: guarded {ok.sum() / ok.size:.3f}, min gap {gaps.min():.3e}")
    assert ok.sum() >= 0.9 * ok.size
    assert (dev.tokens[ok] == ref[ok]).all()
    _, r1 = _max_err("long logp", dev.logp, lp.T, ok)
    assert r1 <= 1.0
    tune("dec.persist", 0)
    fb = _sample(m, X, 175, path="steps")
    tune("dec.persist", 1)
    _compare_runs("long run against the fallback", dev, fb, ok)
    assert _status_is_clear()


# ---------------------------------------------------------------- 5. reproducibility and independence
def test_draws_depend_on_seed_and_stream_alone():
    _, _, X1, m = _setup(MID, 1, 120, seed=5, eos_bias=-1e4)
    X = np.repeat(X1, 32, axis=0)
    stop = 24
    a = _sample(m, X, stop)
    b = _sample(m, X, stop)
    assert a.n_steps == b.n_steps and (a.tokens == b.tokens).all() and (a.logp.view(np.uint32) == b.logp.view(np.uint32)).all()
    c = _sample(m, X, stop, seed=SEED + 1)
    changed = float((a.tokens != c.tokens).mean())
    distinct = len({tuple(r) for r in a.tokens.tolist()})
    print(f"\nsame seed twice: identical; another seed changes {changed:.2f} of the tokens; distinct rows of one utterance {distinct}")
    assert changed > 0 and distinct > 1
    # the guard of every stream, from the per-step loop on the base order
    ref, gaps, _ = _loop(m, X, stop, _keys(SEED, range(32)), 1.0)
    ok = _guard(ref, gaps, 1e-4)
    print(f"guarded {ok.sum() / ok.size:.3f}, min gap {gaps.min():.3e}")
    assert ok.sum() >= 0.9 * ok.size and (a.tokens[ok] == ref[ok]).all()
    rng = np.random.default_rng(11)
    perm = rng.permutation(32)
    rep = np.array([3, 3, 17, 0, 3, 17, 29, 29] * 4)
    for tag, streams in (("permuted", perm), ("repeated", rep)):
        r = _sample(m, X, stop, streams=streams.tolist())
        assert r.n_steps == a.n_steps
        okp = ok[streams]
        same = (r.tokens[okp] == a.tokens[streams][okp]).all()
        err = np.abs(r.logp.astype(np.float64) - a.logp[streams])[okp]
        bits = bool((r.logp.view(np.uint32) == a.logp[streams].view(np.uint32)).all())
        print(f"{tag} streams: tokens at guarded positions equal {bool(same)}, logp max abs err {err.max():.3e}, bit-identical {bits}")
        assert same and (err <= tol(a.logp[streams][okp])).all()
    assert _status_is_clear()


# ---------------------------------------------------------------- 6. consistency with forced decoding
def test_sampled_scores_are_forced_scores():
    from ast_amd import nn as gnn
    _, _, X, m = _setup(ES_EN, 1, 400, seed=15, eos_bias=3.0)
    n = 40                                                      # two calls: 32 rows and 8
    hyps = gnn.sample_hypotheses(m, torch.from_numpy(X), n, 12, SEED, temperature=1.0, first_stream=5)
    assert m.last_predict_path == "device" and len(hyps) == n
    assert all(h["hyp"][0] == GO and EOS not in h["hyp"][1:-1] and 2 <= len(h["hyp"]) <= 13 for h in hyps)
    print()
    worst, lens = 0.0, set()
    for lo in (0, 32):
        part = hyps[lo:lo + 32]
        scores, r = gnn.score_hypotheses(m, X, [h["hyp"] for h in part])
        assert m.last_score_path == "device"
        for k, (h, sc) in enumerate(zip(part, scores)):
            steps = len(h["hyp"]) - 1
            bound = float(tol(r.logp[k, :steps].astype(np.float64)).sum())
            err = abs(sc - h["score"])
            print(f"stream {5 + lo + k}: {steps} steps, sampled {h['score']:.6f}, forced {sc:.6f}, |diff| {err:.3e} (bound {bound:.3e})")
            worst = max(worst, err / bound)
            lens.add(steps)
    print(f"{n} hypotheses, lengths {sorted(lens)}: largest |diff| / bound {worst:.3f}")
    assert worst <= 1.0
    assert len({tuple(h["hyp"]) for h in hyps}) > 1
    assert _status_is_clear()


# ---------------------------------------------------------------- 7. nothing else moved
def test_predict_score_and_training_are_untouched_by_a_sampled_decode():
    from ast_amd.seq2seq import using_config
    from oracle import ast_ref as R
    cfg, P, X, m = _setup(MID, 17, 120, seed=9, eos_bias=8.0)
    rng = np.random.default_rng(3)
    y = rng.integers(1, MID["V"], size=(17, 12)).astype(np.int32)
    Xt = torch.from_numpy(X)
    a = m.predict(Xt, GO, EOS, 30)
    sa = m.predict_scored(Xt, GO, EOS, 30, y=torch.from_numpy(y))
    fa = m.score(Xt, y)
    assert m.last_predict_path == "device" and m.last_score_path == "device"
    r = _sample(m, X, 30)
    r2 = _sample(m, X, 30, temperature=0.7)
    print(f"\nsampled n_steps {r.n_steps} / {r2.n_steps}, greedy n_steps {a.shape[1]}")
    b = m.predict(Xt, GO, EOS, 30)
    sb = m.predict_scored(Xt, GO, EOS, 30, y=torch.from_numpy(y))
    fb = m.score(Xt, y)
    assert a.shape == b.shape and (a == b).all()
    assert (sa.tokens == sb.tokens).all() and (sa.logp.view(np.uint32) == sb.logp.view(np.uint32)).all()
    assert (sa.nll.view(np.uint32) == sb.nll.view(np.uint32)).all() and sa.loss == sb.loss
    assert (fa.logp.view(np.uint32) == fb.logp.view(np.uint32)).all() and (fa.pred == fb.pred).all() and fa.loss == fb.loss
    assert _status_is_clear()
    # a train step after the sampled decode gives the same bits as on a model that never decoded
    _, _, _, fresh = _setup(MID, 17, 120, seed=9, eos_bias=8.0)
    Xs, ys = R.synth_batch(17, 120, 80, 9, MID["V"], seed=21, dtype=np.float32)
    out = []
    for g in (m, fresh):
        g.deterministic = True
        g.inject = {"use_truth": [1] * 8, "enc_masks": None, "emb_mask": None, "rnn_masks": None}
        with using_config("train", True):
            loss = g.forward_loss(torch.from_numpy(Xs), torch.from_numpy(ys), 1.0)
            g.cleargrads()
            loss.backward()
        torch.cuda.synchronize()
        out.append((float(loss.data), g.arena.grad.clone()))
    assert out[0][0] == out[1][0]
    assert torch.equal(out[0][1], out[1][1])
    assert _status_is_clear()


# ---------------------------------------------------------------- 8. fallbacks
@pytest.mark.parametrize("shape,over,B", [(MID, {"ln": True}, 4), (MID, {"n_attn": 2}, 4), (MID, {"feed_attn": False}, 4), (MID, {}, 48),
                                          (WIDE, {}, 4)], ids=["ln", "n_attn2", "no_feed_attn", "B48", "wide"])
def test_fallback_shapes_sample_on_the_step_loop(shape, over, B):
    from ast_amd import _lib
    cfg, P, X, m = _setup(shape, B, 120, seed=11, **over)
    V = shape["V"]
    got = _sample(m, X, 8, path="steps")
    assert _lib.load().astk_sample_workspace_bytes(C.byref(m._cur["dd"]), 8) == 0
    ref, gaps, rlp, greedy = _oracle_sample(cfg, P, X, V, 8, _keys(SEED, range(B)), 1.0)
    ok = _guard(ref, gaps, 1e-3)
    n = min(got.n_steps, ref.shape[1])
    okn = ok[:, :n]
    print(f"\nfallback: guarded {ok.sum()} of {ref.size}, min gap {gaps.min():.3e}, differs from argmax at {(ref != greedy).mean():.2f}")
    assert ok.sum() >= 0.9 * ref.size
    assert (got.tokens[:, :n][okn] == ref[:, :n][okn]).all()
    _, r1 = _max_err("fallback logp vs oracle", got.logp[:, :n], rlp[:n].T, okn)
    assert r1 <= 1.0
    if ok.all():
        assert got.n_steps == ref.shape[1]
        want = _first_eos_scores(ref, rlp)
        assert (np.abs(got.score - want) <= tol(want)).all()
    again = _sample(m, X, 8, path="steps")
    assert (again.tokens == got.tokens).all() and (again.logp == got.logp).all()


# ---------------------------------------------------------------- 9. bad arguments
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
    nbytes = lib.astk_sample_workspace_bytes(C.byref(dd), 10)
    assert nbytes > 0 and nbytes == lib.astk_greedy_workspace_bytes(C.byref(dd), 10)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=m.device)
    toks = torch.empty(10 * 4, dtype=torch.int32, device=m.device)
    logp = torch.empty(10 * 4, dtype=torch.float32, device=m.device)
    nst = torch.zeros(4, dtype=torch.int32, device=m.device)
    keys = torch.from_numpy(_keys(SEED, range(4)).view(np.int64)).to(m.device)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(d=dd, go=GO, eos=EOS, stop=10, wsz=nbytes, keys=keys, inv=1.0, toks=toks, logp=logp, nst=nst, enc=st["enc_states"]):
        return lib.astk_sample_decode(C.byref(d), C.byref(st["dp"]), P(enc), P(m._dec_c), P(m._dec_h), go, eos, stop, P(keys), inv, P(toks),
                                      P(logp), P(nst), None, P(ws), wsz, None)
    bad = _lib.DecoderDesc.from_buffer_copy(dd)
    bad.struct_size -= 8
    off = _lib.DecoderDesc.from_buffer_copy(dd)
    off.ln = 1
    for kw, word in ((dict(d=bad), b"struct_size"), (dict(go=-1), b"go"), (dict(eos=MID["V"]), b"eos"), (dict(stop=0), b"stop_limit"),
                     (dict(stop=513), b"stop_limit"), (dict(d=off), b"device loop"), (dict(wsz=nbytes - 1), b"workspace too small"),
                     (dict(toks=None), b"null pointer"), (dict(nst=None), b"null pointer"), (dict(enc=None), b"null pointer"),
                     (dict(logp=None), b"logp"), (dict(keys=None), b"row_keys"), (dict(inv=0.0), b"inv_temp"), (dict(inv=-1.0), b"inv_temp"),
                     (dict(inv=float("inf")), b"inv_temp"), (dict(inv=float("nan")), b"inv_temp")):
        assert call(**kw) < 0, kw
        print(kw.keys(), lib.astk_last_error().decode())
        assert word in lib.astk_last_error(), (kw, lib.astk_last_error())
    torch.cuda.synchronize()
    assert _status_is_clear()
    assert call() == 0
    torch.cuda.synchronize()
    assert 1 <= int(nst[0]) <= 10
    assert _status_is_clear()
    for t in (0.0, -1.0, float("inf"), float("nan"), 1e-60, 1e60):
        with pytest.raises(ValueError, match="temperature"):
            m.sample(torch.from_numpy(X), GO, EOS, 10, SEED, temperature=t)
    with pytest.raises(ValueError, match="streams"):
        m.sample(torch.from_numpy(X), GO, EOS, 10, SEED, streams=[0, 1])
    assert _status_is_clear()


# ---------------------------------------------------------------- 10. sample.py
def test_sample_py_writes_an_nbest_pickle_that_score_py_reads(tmp_path):
    """sample.py on a tiny synthetic experiment, as a child process: its pickle goes through `score.py --nbest` unchanged and the model
    scores agree with the sampled ones; --mbr writes one hypothesis per utterance."""
    import json, os, pickle, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mcfg = tiny_cfg(enc_layers=2, dec_layers=1, H=32, E=16, A=32, c0=8, c1=16, V=31, drop=0.0)
    del mcfg["rnn_config"]["dec_vocab_size"]
    tcfg = {"seed": "seed-ast-20h", "gpuid": 0, "batch_size": 8, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 1,
            "optimizer": {"type": 0, "lr": 2e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0},
            "data": {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 16, "syn_dev": 7},
                     "frames": [60, 300], "targets": [2, 9], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w", "refs_path": str(tmp_path / "refs"), "n_evals": 1}}
    json.dump(mcfg, open(tmp_path / "model_cfg.json", "w"))
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))
    from ast_amd.nn import NN
    nn = NN(str(tmp_path))
    refs = tmp_path / "refs" / "syn_dev"
    os.makedirs(refs)
    utts = sorted(nn.data_loader.info["syn_dev"])
    truth = nn.data_loader.get_hyps([(u, list(nn.data_loader.ids["syn_dev"][u])) for u in utts])
    (refs / "eval.ids").write_text("".join(u + "\n" for u in utts))
    (refs / "ref.en0").write_text("".join(" ".join(truth[u]) + "\n" for u in utts))
    del nn
    torch.cuda.empty_cache()

    def run(script, *extra):
        r = subprocess.run([sys.executable, os.path.join(root, script), "-m", str(tmp_path)] + list(extra), cwd=root, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    out1 = run("train.py", "-e", "1")
    assert "Traceback" not in out1
    pk = str(tmp_path / "samples.p")
    out2 = run("sample.py", "-s", "syn_dev", "-n", "6", "-t", "0.8", "--seed", "11", "--mbr", "-w", pk)
    print("\n" + "\n".join(out2.strip().splitlines()[-4:]))
    samples = pickle.load(open(pk, "rb"))
    assert sorted(samples) == utts and all(len(v) == 6 for v in samples.values())
    for lst in samples.values():
        for hyp, score, hist in lst:
            assert hyp[0] == GO and 2 <= len(hyp) <= 13 and EOS not in hyp[1:-1] and score <= 0 and hist == []
    assert "MBR BLEU = " in out2
    lines = open(pk + ".mbr.en").read().split("\n")
    assert len(lines) == len(utts) + 1 and lines[-1] == ""
    # the same seed again gives the same pickle; the default name carries N and T
    run("sample.py", "-s", "syn_dev", "-n", "6", "-t", "0.8", "--seed", "11")
    again = pickle.load(open(tmp_path / "syn_dev_sample_N-6_T-0.80.p", "rb"))
    assert again == samples
    # score.py reads it as it reads beam.py's: at temperature 1 the sampled score is the model's score of the hypothesis
    run("sample.py", "-s", "syn_dev", "-n", "6", "--seed", "11", "-w", pk)
    samples = pickle.load(open(pk, "rb"))
    out3 = run("score.py", "-s", "syn_dev", "--nbest", pk)
    rows = [l.split() for l in open(pk + ".scores.txt").read().splitlines()]
    assert len(rows) == 6 * len(utts)
    worst = max(abs(float(r[2]) - float(r[3])) / (int(r[4]) * float(tol(float(r[2]))) + 1e-6) for r in rows)
    print(out3.strip().splitlines()[-2], f"(worst ratio {worst:.3f})")
    assert "largest |beam score - model score|" in out3 and worst <= 1.0
