"""Forced decoding on the device (include/astk.h astk_forced_score: the persistent decoder loop in its forced mode;
SpeechEncoderDecoder.score, NN.score_set, score.py, train.py --forced-dev-loss) against the float64 oracle's decode_step run along the
given tokens, against eval-mode forward_loss, the per-step loop and beam search's own scores; what it must leave untouched; the step
cap, fallbacks and bad arguments.

Bounds are the project's: log-probabilities under tol() of tests/test_gpu_greedy_scored.py, the loss at 1e-4 relative, attention rows
at 1e-5 absolute, the argmax exactly wherever the oracle's top-2 logit gap is at least 1e-3 (at least 0.98 of the positions of every
full-size case).  Every test prints its figures before it asserts."""
import copy
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from conftest import tiny_cfg
from decode_helpers import CFG1, EOS, ES_EN, GO, MID, OUT_SCALE, WIDE, lse64 as _lse64, setup as _setup, targets, tol

pytestmark = pytest.mark.gpu

GAP = 1e-3                  # tests/test_gpu_greedy.py: the argmax margin against the oracle
SHARE = 0.98
_targets = functools.partial(targets, go_first=True)


def _rows_of(lg, y_next):
    """float64, from one step's logits: log p(target), log p(argmax), the argmax (first maximum), the top-2 gap."""
    lse = _lse64(lg)
    srt = np.sort(lg, axis=1)
    return lg[np.arange(lg.shape[0]), y_next] - lse, srt[:, -1] - lse, lg.argmax(axis=1).astype(np.int32), srt[:, -1] - srt[:, -2]


def _pack(rows, alphas, y):
    """Step-major lists -> a namespace of (B, S) arrays (alpha (B, S, T'')) and the loss sum_s (1 / B) sum_b weight * (-logp)."""
    logp, lpmax, pred, gaps = (np.stack([r[k] for r in rows], 1) for k in range(4))
    w = (y[:, 1:] != 0).astype(np.float64)
    return types.SimpleNamespace(logp=logp, logp_max=lpmax, pred=pred, gaps=gaps, alpha=np.stack(alphas, 1) if alphas else None, weight=w,
                                 loss=float((w * -logp).sum() / y.shape[0]), score=(w * logp).sum(axis=1), n_tokens=(w != 0).sum(axis=1))


def _oracle_forced(cfg, P, X, V, y):
    """oracle.ast_ref.RefModel in eval mode, decode_step(y[:, s], ht, step=s) in a loop: float64 logits and alphas."""
    from oracle import ast_ref as R
    m = R.RefModel(cfg, {k: v.astype(np.float64) for k, v in P.items()}, V)
    m.train = False
    B = X.shape[0]
    m.encode(X.astype(np.float64))
    m.init_decoder_state()
    ht = R.Variable(np.zeros((B, cfg["rnn_config"]["attn_units"])))
    rows, alphas = [], []
    for s in range(y.shape[1] - 1):
        logits, ht, al = m.decode_step(y[:, s].astype(np.int32), ht, step=s)
        rows.append(_rows_of(np.asarray(logits.data, dtype=np.float64), y[:, s + 1]))
        alphas.append(np.asarray(al.data, dtype=np.float64).reshape(B, -1))
    return _pack(rows, alphas, y)


def _loop_forced(m, X, y):
    """The per-step GPU loop with its float32 logits kept: the same namespace, from a float64 LSE on the host."""
    from ast_amd.seq2seq import using_config
    with using_config("train", False):
        m.encode(torch.from_numpy(X))
        m.init_decoder_state()
        B = X.shape[0]
        ht = torch.zeros(B, m.A, dtype=torch.float32, device=m.device)
        yd = torch.from_numpy(y).to(m.device)
        rows, alphas = [], []
        for s in range(y.shape[1] - 1):
            logits, ht, al = m.decode_step(yd[:, s].contiguous(), ht)
            rows.append(_rows_of(logits.double().cpu().numpy(), y[:, s + 1]))
            alphas.append(al[:, :, 0].double().cpu().numpy())
    return _pack(rows, alphas, y)


def _max_err(name, got, ref, ok=None):
    ok = np.ones(ref.shape, dtype=bool) if ok is None else ok
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)[ok]
    rel = err / tol(ref[ok])
    print(f"  {name}: max abs err {err.max():.3e}, max err / tol {rel.max():.3f}, value range {ref[ok].min():.3f} .. {ref[ok].max():.3f}, n {ok.sum()}")
    return float(rel.max())


def _compare(tag, got, ref, guard_pred=True, alpha=True):
    """A ForcedScore against a reference namespace: every field under the module's bounds.  Returns the share of compared argmaxes."""
    assert got.logp.shape == got.logp_max.shape == got.pred.shape == got.weight.shape == ref.logp.shape
    assert got.logp.dtype == np.float32 and got.logp_max.dtype == np.float32 and got.pred.dtype == np.int32
    ok = ref.gaps >= GAP if guard_pred else np.ones(ref.gaps.shape, dtype=bool)
    share = ok.sum() / ok.size
    print(f"\n{tag}: S {ref.logp.shape[1]}, share of positions with gap >= {GAP:g}: {share:.4f}, smallest gap {ref.gaps.min():.2e}")
    r1 = _max_err("logp", got.logp, ref.logp)
    r2 = _max_err("logp_max", got.logp_max, ref.logp_max)
    wrong = int((got.pred[ok] != ref.pred[ok]).sum())
    rl = abs(got.loss - ref.loss) / abs(ref.loss)
    print(f"  pred: {wrong} of {ok.sum()} compared positions differ; loss {got.loss:.6f} (reference {ref.loss:.6f}, rel {rl:.3e})")
    es = np.abs(got.score - ref.score)
    print(f"  score: max abs err {es.max():.3e}, max |value| {np.abs(ref.score).max():.3f}")
    if alpha:
        ea = np.abs(got.alpha.astype(np.float64) - ref.alpha).max()
        rs = np.abs(got.alpha.astype(np.float64).sum(axis=2) - 1).max()
        print(f"  alpha: max abs err {ea:.3e}, max |row sum - 1| {rs:.3e}, shape {got.alpha.shape}")
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)
    assert wrong == 0
    assert rl <= 1e-4, (got.loss, ref.loss)
    assert (got.weight == ref.weight).all() and (got.n_tokens == ref.n_tokens).all()
    assert (es <= np.maximum(tol(ref.score), (ref.weight * tol(ref.logp)).sum(axis=1))).all()
    if alpha:
        assert got.alpha.shape == ref.alpha.shape and got.alpha.dtype == np.float32
        assert ea <= 1e-5 and rs <= 1e-5, (ea, rs)
    return share


# ---------------------------------------------------------------- 1. oracle parity at full size
@functools.lru_cache(maxsize=None)
def _case(name, L):
    shape = {"configs1": CFG1, "es_en_20h": ES_EN}[name]
    cfg, P, X, m = _setup(shape, 32, 800, seed=0)
    y = _targets(32, L, shape["V"], seed=2)
    return cfg, P, X, m, y, _oracle_forced(cfg, P, X, shape["V"], y)


@pytest.mark.parametrize("L", [40, 176])
@pytest.mark.parametrize("name", ["configs1", "es_en_20h"])
def test_forced_matches_oracle_full_size(name, L):
    """Figures measured on one MI355X are in the result table of DESIGN.md section 13."""
    cfg, P, X, m, y, ref = _case(name, L)
    got = m.score(torch.from_numpy(X), y, return_alpha=True)
    assert m.last_score_path == "device"
    share = _compare(f"{name} L {L} device vs oracle", got, ref)
    assert share >= SHARE, share
    assert got.alpha.shape == (32, L - 1, m._cur["T2"])
    # without the alpha output: the same numbers to the bit, no alpha
    plain = m.score(torch.from_numpy(X), y)
    assert m.last_score_path == "device" and plain.alpha is None
    assert (plain.logp == got.logp).all() and (plain.logp_max == got.logp_max).all() and (plain.pred == got.pred).all()
    assert plain.loss == got.loss


# ---------------------------------------------------------------- 2. the project's other routes to the same numbers
@pytest.mark.parametrize("L", [40, 176])
@pytest.mark.parametrize("name", ["configs1", "es_en_20h"])
def test_loss_matches_eval_mode_forward_loss(name, L):
    from ast_amd.seq2seq import using_config
    cfg, P, X, m, y, ref = _case(name, L)
    got = m.score(torch.from_numpy(X), y)
    with using_config("train", False):
        fl = float(m.forward_loss(torch.from_numpy(X), torch.from_numpy(y), 1))
    print(f"\n{name} L {L}: score().loss {got.loss:.6f}, eval-mode forward_loss {fl:.6f} (rel {abs(got.loss - fl) / abs(fl):.3e}), "
          f"oracle {ref.loss:.6f}")
    assert abs(got.loss - fl) <= 1e-4 * abs(fl), (got.loss, fl, ref.loss)


@pytest.mark.parametrize("name", ["configs1", "es_en_20h"])
def test_device_loop_matches_step_fallback(name, tune):
    cfg, P, X, m, y, ref = _case(name, 40)
    dev = m.score(torch.from_numpy(X), y, return_alpha=True)
    assert m.last_score_path == "device"
    tune("dec.persist", 0)
    stp = m.score(torch.from_numpy(X), y, return_alpha=True)
    assert m.last_score_path == "steps"
    tune("dec.persist", 1)
    assert type(stp) is type(dev)
    _compare(f"{name} L 40 step fallback vs oracle", stp, ref)
    side = types.SimpleNamespace(logp=stp.logp.astype(np.float64), logp_max=stp.logp_max.astype(np.float64), pred=stp.pred, gaps=ref.gaps,
                                 alpha=stp.alpha.astype(np.float64), weight=stp.weight, loss=stp.loss, score=stp.score, n_tokens=stp.n_tokens)
    _compare(f"{name} L 40 device vs step fallback", dev, side)


@pytest.mark.parametrize("shape,over,B", [(MID, {"ln": True}, 4), (MID, {"n_attn": 2}, 4), (MID, {"feed_attn": False}, 4), (MID, {}, 48),
                                          (WIDE, {}, 4)], ids=["ln", "n_attn2", "no_feed_attn", "B48", "wide"])
def test_fallback_shapes_score_on_the_step_loop(shape, over, B):
    from ast_amd import _lib
    from ast_amd.seq2seq import ForcedScore
    cfg, P, X, m = _setup(shape, B, 120, seed=11, **over)
    V = shape["V"]
    y = _targets(B, 9, V, seed=2)
    got = m.score(torch.from_numpy(X), y, return_alpha=True)
    assert m.last_score_path == "steps" and isinstance(got, ForcedScore)
    assert _lib.load().astk_forced_workspace_bytes(C.byref(m._cur["dd"]), 8, 1) == 0
    share = _compare("fallback vs oracle", got, _oracle_forced(cfg, P, X, V, y))
    assert share >= 0.9, share
    assert m.score(torch.from_numpy(X), y).alpha is None


def test_streamed_slices_match_the_step_loop():
    """T'' = 420 (the loader's longest bucket): the streamed-slice variant of the forced kernel, 59 steps."""
    _, _, X, m = _setup(ES_EN, 32, 4 * 420, seed=7)
    y = _targets(32, 60, ES_EN["V"], seed=9)
    dev = m.score(torch.from_numpy(X), y, return_alpha=True)
    assert m.last_score_path == "device" and m._cur["T2"] == 420 and dev.alpha.shape == (32, 59, 420)
    share = _compare("streamed slices, device vs per-step loop", dev, _loop_forced(m, X, y))
    assert share >= 0.9, share


# ---------------------------------------------------------------- 3. beam search's scores are forced scores
def test_beam_scores_are_forced_scores():
    from oracle import ast_ref as R
    from ast_amd import nn as gnn
    from ast_amd.seq2seq import SpeechEncoderDecoder
    cfg = tiny_cfg(**MID)
    V, D, N = MID["V"], 80, 5
    P = R.init_params(cfg, D, V, seed=21, dtype=np.float32)
    P["out/W"] = (P["out/W"] * OUT_SCALE).astype(np.float32)
    P["out/b"] = P["out/b"].copy()
    P["out/b"][EOS] += 2.0                      # some hypotheses finish early: lengths differ inside an n-best list
    m = SpeechEncoderDecoder(0, copy.deepcopy(cfg)).materialize(D, values=P)
    Xs = [R.synth_batch(1, T, D, 4, V, seed=30 + i, dtype=np.float32)[0] for i, T in enumerate((90, 71, 120, 150))]
    lists = gnn.decode_beam_batch(m, [torch.from_numpy(X) for X in Xs], 12, N, N)
    worst, worst_a, n_hyp, lens = 0.0, 0.0, 0, set()
    for u, (X, lst) in enumerate(zip(Xs, lists)):
        hyps = [e["hyp"] for e in lst]
        scores, r = gnn.score_hypotheses(m, X, hyps, return_alpha=True)
        assert m.last_score_path == "device" and r.logp.shape[0] == len(hyps)
        for k, (e, sc) in enumerate(zip(lst, scores)):
            n = len(e["hyp"]) - 1
            bound = float(tol(r.logp[k, :n].astype(np.float64)).sum())
            err = abs(sc - e["score"])
            ah = np.stack(e["attn_history"], 0)
            ea = float(np.abs(r.alpha[k, :n] - ah).max())
            print(f"utt {u} hyp {k}: {n} steps, beam {e['score']:.6f}, forced {sc:.6f}, |diff| {err:.3e} (bound {bound:.3e}), alpha max err {ea:.3e}")
            worst, worst_a, n_hyp = max(worst, err / bound), max(worst_a, ea), n_hyp + 1
            lens.add(n)
            assert ah.shape == (n, r.alpha.shape[2])
    print(f"{n_hyp} hypotheses, lengths {sorted(lens)}: largest |diff| / bound {worst:.3f}, largest alpha error {worst_a:.3e}")
    assert n_hyp >= 4 * 2 and len(lens) > 1
    assert worst <= 1.0 and worst_a <= 1e-5


# ---------------------------------------------------------------- 4. the step cap
def test_long_cap_runs_on_the_device(tune):
    """ldy = 513 (512 steps, the cap of the greedy modes) runs on the device; ldy = 514 takes the per-step loop.  The training path's
    L <= 192 does not apply."""
    from ast_amd import _lib
    _, _, X, m = _setup(MID, 5, 120, seed=5)
    y = _targets(5, 514, MID["V"], seed=4)
    dev = m.score(torch.from_numpy(X), y[:, :513], return_alpha=True)
    assert m.last_score_path == "device" and dev.logp.shape == (5, 512)
    ref = _loop_forced(m, X, y[:, :513])
    share = _compare("ldy 513, device vs per-step loop", dev, ref)
    assert share >= 0.9, share
    d = m._cur["dd"]
    lib = _lib.load()
    assert lib.astk_forced_workspace_bytes(C.byref(d), 512, 0) > 0 and lib.astk_forced_workspace_bytes(C.byref(d), 513, 0) == 0
    over = m.score(torch.from_numpy(X), y)
    assert m.last_score_path == "steps" and over.logp.shape == (5, 513)
    r = float((np.abs(over.logp[:, :512].astype(np.float64) - ref.logp) / tol(ref.logp)).max())
    print(f"  ldy 514 on the per-step loop: first 512 steps against the loop above, max err / tol {r:.3f}")
    assert r <= 1.0


# ---------------------------------------------------------------- 5. nothing else moved
def test_predict_and_training_are_untouched_by_a_score_call():
    """predict and predict_scored give the same bits before and after score calls (one of them enqueued while a scored decode of the same
    slot is still pending: the workspaces and pinned buffers do not alias), and a train step behind them gives the bits it gives on a
    model that never scored."""
    from ast_amd import _lib
    from ast_amd.seq2seq import using_config
    from oracle import ast_ref as R
    cfg, P, X, m = _setup(MID, 17, 120, seed=9, eos_bias=3.0)
    y = _targets(17, 12, MID["V"], seed=3)
    a = m.predict(torch.from_numpy(X), GO, EOS, 30)
    sa = m.predict_scored(torch.from_numpy(X), GO, EOS, 30, y=torch.from_numpy(y))
    assert m.last_predict_path == "device"
    pend = m.predict_scored_async(torch.from_numpy(X), GO, EOS, 30, torch.from_numpy(y), slot=0)
    r = m.score_async(torch.from_numpy(X), y, return_alpha=True, slot=0).result()
    sb0 = pend.result()
    r2 = m.score(torch.from_numpy(X), y, return_alpha=True)
    assert m.last_score_path == "device"
    b = m.predict(torch.from_numpy(X), GO, EOS, 30)
    sb = m.predict_scored(torch.from_numpy(X), GO, EOS, 30, y=torch.from_numpy(y))
    print(f"\npredict {a.shape}, scored n_steps {sa.n_steps}, loss {sa.loss:.6f}; forced loss {r.loss:.6f}")
    assert a.dtype == np.int32 and a.shape == b.shape and (a == b).all()
    for s in (sb0, sb):
        assert (s.tokens == sa.tokens).all() and (s.logp == sa.logp).all() and (s.nll == sa.nll).all() and s.loss == sa.loss
    assert (r.logp == r2.logp).all() and (r.pred == r2.pred).all() and (r.alpha == r2.alpha).all() and r.loss == r2.loss
    mask = C.c_uint(7)
    assert _lib.load().astk_persist_status(C.byref(mask), 0) == 0 and mask.value == 0
    # a train step after the score calls gives the same bits as on a model that never scored
    _, _, _, fresh = _setup(MID, 17, 120, seed=9, eos_bias=3.0)
    Xt, yt = R.synth_batch(17, 120, 80, 9, MID["V"], seed=21, dtype=np.float32)
    out = []
    for g in (m, fresh):
        g.deterministic = True
        g.inject = {"use_truth": [1] * 8, "enc_masks": None, "emb_mask": None, "rnn_masks": None}
        with using_config("train", True):
            loss = g.forward_loss(torch.from_numpy(Xt), torch.from_numpy(yt), 1.0)
            g.cleargrads()
            loss.backward()
        torch.cuda.synchronize()
        out.append((float(loss.data), g.arena.grad.clone()))
    print(f"  train loss after score calls {out[0][0]!r}, on a fresh model {out[1][0]!r}")
    assert out[0][0] == out[1][0]
    assert torch.equal(out[0][1], out[1][1])


def test_nn_score_set_and_score_hypotheses(tune):
    from ast_amd import nn as gnn
    _, _, _, m = _setup(ES_EN, 8, 240, seed=15)
    rng = np.random.default_rng(0)
    batches = []
    for i, (B, T, L) in enumerate(((8, 240, 9), (5, 320, 14), (8, 200, 40), (3, 400, 5))):
        batches.append({"X": rng.standard_normal((B, T, 80)).astype(np.float32), "utts": [f"u{i}_{j}" for j in range(B)],
                        "y": torch.from_numpy(_targets(B, L, ES_EN["V"], seed=40 + i))})
    asked = []

    def get_batch(batch_size, set_key, train, labels=False):
        asked.append((train, labels))
        return iter(batches)
    stub = types.SimpleNamespace(model=m, cfg=types.SimpleNamespace(train={"data": {"max_pred": 30}, "batch_size": 8}),
                                 data_loader=types.SimpleNamespace(n_utts={"dev": sum(len(b["utts"]) for b in batches)}, get_batch=get_batch))
    scores, dev_loss, ppl = gnn.NN.score_set(stub, "dev")
    assert m.last_score_path == "device" and asked == [(False, True)]
    each = [m.score(b["X"], b["y"]) for b in batches]
    want_loss = np.mean([r.loss / b["y"].shape[1] for r, b in zip(each, batches)])
    lp, nt = np.concatenate([r.score for r in each]), np.concatenate([r.n_tokens for r in each])
    print(f"\nscore_set: dev loss {dev_loss:.6f} (batch by batch {want_loss:.6f}), perplexity {ppl:.4f}, {len(scores)} utterances")
    assert [u for u, _, _ in scores] == [u for b in batches for u in b["utts"]]
    assert [s for _, s, _ in scores] == lp.tolist() and [n for _, _, n in scores] == nt.tolist()
    assert abs(dev_loss - want_loss) <= 1e-12 * abs(want_loss)
    assert abs(ppl - np.exp(-lp.sum() / nt.sum())) <= 1e-12 * ppl and ppl > 1
    tune("dec.persist", 0)
    s_off, loss_off, ppl_off = gnn.NN.score_set(stub, "dev")
    tune("dec.persist", 1)
    assert m.last_score_path == "steps"
    # every token's error is within tol(its log-probability) <= tol(the utterance's score): an utterance's is within n_tokens times that
    per_utt = tol(lp) * np.maximum(nt, 1)
    assert (np.abs(np.array([s for _, s, _ in s_off]) - lp) <= per_utt).all()
    assert abs(loss_off - dev_loss) <= tol(dev_loss) and abs(np.log(ppl_off) - np.log(ppl)) <= per_utt.sum() / nt.sum()


def test_train_py_forced_dev_loss_columns_and_score_py(tmp_path):
    """Without --forced-dev-loss the dev log lines are what they were; with it two more columns, NN.score_set's dev loss and perplexity.
    score.py scores the references and a beam.py-style pickle of the same experiment."""
    import json, os, pickle, re, subprocess, sys
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
    assert "forced dev loss" not in out1 and "perplexity" not in out1
    out2 = run("train.py", "-e", "1", "--forced-dev-loss")
    out3 = run("train.py", "-e", "1", "--dev-loss", "--forced-dev-loss")
    lines = open(tmp_path / "dev.log").read().split("\n")
    print("\ndev.log:", lines)
    assert len(lines) == 4 and lines[3] == "" and re.fullmatch(r"1, \d+\.\d\d", lines[0])
    assert re.fullmatch(r"2, \d+\.\d\d, \d+\.\d{4}, \d+\.\d{4}", lines[1]) and re.fullmatch(r"3, \d+\.\d\d, \d+\.\d{4}, \d+\.\d{4}, \d+\.\d{4}", lines[2])
    nn = NN(str(tmp_path))
    assert nn.max_epoch == 3
    scores, dev_loss, ppl = nn.score_set("syn_dev")
    col = [float(v) for v in lines[2].split(", ")]
    assert abs(col[3] - dev_loss) <= 0.0000501 and abs(col[4] - ppl) <= 0.0000501 + 1e-6 * ppl, (lines[2], dev_loss, ppl)
    assert "forced dev loss = {0:.4f}, perplexity = {1:.4f}".format(col[3], col[4]) in out3 and "forced dev loss" in out2
    assert len(scores) == 7 and dev_loss > 0 and ppl > 1
    # score.py on the references: the same figures and one line per utterance
    by_utt = {u: (s, n) for u, s, n in scores}
    out4 = run("score.py", "-s", "syn_dev", "--alignments", str(tmp_path / "align.npz"))
    assert "forced dev loss = {0:.4f}".format(dev_loss) in out4
    rows = [l.split() for l in open(tmp_path / "syn_dev_scores.txt").read().splitlines()]
    assert sorted(r[0] for r in rows) == utts
    for u, s, n in rows:
        assert abs(float(s) - by_utt[u][0]) <= 1e-4 * max(1.0, abs(by_utt[u][0])) and int(n) == by_utt[u][1]
    al = np.load(tmp_path / "align.npz")
    assert sorted(al.files) == utts and all(abs(al[u].sum(axis=1) - 1).max() <= 1e-5 for u in utts)
    # ... and on an n-best pickle in beam.py's format
    beam = {}
    for utt in nn.data_loader.get_batch(1, "syn_dev", train=False, labels=False):
        beam[utt["utts"][0]] = [(e["hyp"], e["score"], e["attn_history"]) for e in nn.decode_beam(utt["X"], stop_limit=8, N=3, K=3)]
    pickle.dump(beam, open(tmp_path / "nbest.p", "wb"))
    del nn
    torch.cuda.empty_cache()
    out5 = run("score.py", "-s", "syn_dev", "--nbest", str(tmp_path / "nbest.p"))
    rows = [l.split() for l in open(str(tmp_path / "nbest.p") + ".scores.txt").read().splitlines()]
    assert len(rows) == sum(len(v) for v in beam.values())
    # (each step's log-probability is within tol() of itself, at most tol(the whole score); both columns are printed to 1e-6)
    worst = max(abs(float(r[2]) - float(r[3])) / (int(r[4]) * float(tol(float(r[2]))) + 1e-6) for r in rows)
    print(out5.strip().splitlines()[-2], f"(worst ratio {worst:.3f})")
    assert "largest |beam score - model score|" in out5 and worst <= 1.0


# ---------------------------------------------------------------- 6. bad arguments through the C ABI
def test_bad_arguments_fail_with_a_message_and_write_nothing():
    from ast_amd import _lib
    from ast_amd.seq2seq import using_config
    lib = _lib.load()
    _, _, X, m = _setup(MID, 4, 120, seed=13)
    with using_config("train", False):
        m.encode(torch.from_numpy(X))
        m.init_decoder_state()
    st = m._cur
    dd = _lib.DecoderDesc.from_buffer_copy(st["dd"])
    B, S, T2 = 4, 5, st["T2"]
    nbytes = lib.astk_forced_workspace_bytes(C.byref(dd), S, 1)
    assert nbytes > lib.astk_forced_workspace_bytes(C.byref(dd), S, 0) > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=m.device)
    SENT = -12345.0
    logp = torch.full((600 * B,), SENT, dtype=torch.float32, device=m.device)
    lpm, alpha, status = logp.clone(), torch.full((S * B * T2,), SENT, dtype=torch.float32, device=m.device), logp[:4].clone()
    pred = torch.full((600 * B,), -777, dtype=torch.int32, device=m.device)
    y = torch.from_numpy(_targets(B, 600, MID["V"], seed=1)).to(m.device)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(d=dd, prm=st["dp"], enc=st["enc_states"], c0=m._dec_c, h0=m._dec_h, y=y, ldy=S + 1, logp=logp, lpm=lpm, pred=pred, alpha=alpha,
             wsz=nbytes, ws=ws):
        return lib.astk_forced_score(C.byref(d), None if prm is None else C.byref(prm), P(enc), P(c0), P(h0), P(y), ldy, P(logp), P(lpm),
                                     P(pred), P(alpha), P(status), P(ws), wsz, None)
    bad = _lib.DecoderDesc.from_buffer_copy(dd)
    bad.struct_size -= 8
    off = _lib.DecoderDesc.from_buffer_copy(dd)
    off.ln = 1
    big = _lib.DecoderDesc.from_buffer_copy(dd)
    big.B = 48
    for kw, word in ((dict(d=bad), b"struct_size"), (dict(ldy=1), b"ldy"), (dict(ldy=0), b"ldy"), (dict(ldy=514), b"ldy"),
                     (dict(d=off), b"device loop"), (dict(d=big), b"device loop"), (dict(wsz=nbytes - 1), b"workspace too small"),
                     (dict(ws=None), b"workspace too small"), (dict(y=None), b"null pointer"), (dict(logp=None), b"null pointer"),
                     (dict(enc=None), b"null pointer"), (dict(c0=None), b"null pointer"), (dict(h0=None), b"null pointer"),
                     (dict(prm=None), b"null pointer")):
        assert call(**kw) < 0, kw
        print(f"  {kw if 'd' not in kw else 'descriptor'}: {lib.astk_last_error().decode()[:90]}")
        assert word in lib.astk_last_error(), (kw, lib.astk_last_error())
    torch.cuda.synchronize()
    for t, v in ((logp, SENT), (lpm, SENT), (alpha, SENT), (status, SENT), (pred, -777)):
        assert bool((t == v).all())
    mask = C.c_uint(7)
    assert lib.astk_persist_status(C.byref(mask), 0) == 0 and mask.value == 0
    # the same call with good arguments runs, with and without the optional outputs
    assert call() == 0
    torch.cuda.synchronize()
    assert float(status[0]) == 0.0 and bool((status[1:] == SENT).all())
    n = S * B
    assert bool((logp[:n] <= 0).all()) and bool((logp[n:] == SENT).all()) and bool((lpm[:n] <= 0).all()) and bool((lpm[:n] >= logp[:n]).all())
    assert bool(((pred[:n] >= 0) & (pred[:n] < MID["V"])).all()) and bool((pred[n:] == -777).all())
    assert bool(((alpha.view(n, T2).sum(dim=1) - 1).abs() <= 1e-5).all())
    first = logp[:n].clone()
    logp.fill_(SENT)
    assert call(lpm=None, pred=None, alpha=None, wsz=lib.astk_forced_workspace_bytes(C.byref(dd), S, 0)) == 0
    torch.cuda.synchronize()
    assert torch.equal(logp[:n], first)
    assert lib.astk_persist_status(C.byref(mask), 0) == 0 and mask.value == 0
