"""Scored greedy decoding on the device (include/astk.h astk_greedy_decode_scored: the persistent decoder loop in its scored greedy mode;
SpeechEncoderDecoder.predict_scored, NN.predict_scored, train.py --dev-loss) against the float64 oracle's greedy loop with
oracle.minichainer.softmax_cross_entropy, and against the per-step GPU loop; what it must leave untouched; fallbacks and bad arguments.

Token comparisons are exact and guarded by the argmax margin as in test_gpu_greedy.py.  Log-probabilities and loss terms are compared
under tol(): max(2 * E_LOOP, 1e-4 * max(1, |value|)), see E_LOOP in tests/decode_helpers.py.  Every test prints its figures before it asserts."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from conftest import tiny_cfg
from decode_helpers import (CFG1, EOS, ES_EN, GO, MID, WIDE, guard as _guard, lse64 as _lse64, max_err as _max_err, setup as _setup,
                            targets as _targets, tol)

pytestmark = pytest.mark.gpu


def _score_rows(lg, word, y, step, V):
    """float64: log p(word) and the weighted -log p(target of this step) (0 without one) from one step's logits."""
    lse = _lse64(lg)
    rows = np.arange(lg.shape[0])
    logp = lg[rows, word] - lse
    nll = np.zeros(lg.shape[0])
    if y is not None and step + 1 < y.shape[1]:
        t = y[:, step + 1]
        nll = np.where(t == 0, 0.0, lse - lg[rows, t])
    return logp, nll


def _loop(m, X, stop_limit, y=None, eos_dist=None):
    """The per-step GPU loop of predict() with its logits kept: tokens (B, n), the top-2 gap of every (step, row), and logp / nll (n, B)
    from a float64 LSE of the float32 logits on the host."""
    from ast_amd.seq2seq import using_config
    with using_config("train", False):
        m.encode(torch.from_numpy(X))
        m.init_decoder_state()
        B = X.shape[0]
        ht = torch.zeros(B, m.A, dtype=torch.float32, device=m.device)
        word = torch.full((B,), GO, dtype=torch.int32, device=m.device)
        done = torch.zeros(B, dtype=torch.bool, device=m.device)
        rows, gaps, lps, nlls = [], [], [], []
        for step in range(stop_limit):
            logits, ht, _ = m.decode_step(word, ht)
            top = torch.topk(logits, 2, dim=1).values
            gaps.append((top[:, 0] - top[:, 1]).cpu().numpy())
            if eos_dist is not None:
                eos_dist.append((top[:, 0] - logits[:, EOS]).cpu().numpy())
            word = logits.argmax(dim=1).to(torch.int32)
            lp, nl = _score_rows(logits.double().cpu().numpy(), word.cpu().numpy(), y, step, m.V)
            lps.append(lp)
            nlls.append(nl)
            rows.append(word)
            done |= word == EOS
            if bool(done.all()):
                break
    return torch.stack(rows, 0).T.cpu().numpy(), np.stack(gaps, 0), np.stack(lps, 0), np.stack(nlls, 0)


def _oracle_greedy(cfg, P, X, V, stop_limit, y=None):
    """The oracle's decode_step in a greedy loop; with targets, softmax_cross_entropy(logits, y[:, s+1], class_weight = w), w[0] = 0,
    summed until the all-EOS break (added before the break).  Returns tokens (B, n), gaps, logp, nll (n, B) and the loss."""
    from oracle import ast_ref as R
    from oracle import minichainer as F
    m = R.RefModel(cfg, {k: v.astype(np.float64) for k, v in P.items()}, V)
    m.train = False
    B = X.shape[0]
    m.encode(X.astype(np.float64))
    m.init_decoder_state()
    ht = R.Variable(np.zeros((B, cfg["rnn_config"]["attn_units"])))
    word = np.full((B,), GO, dtype=np.int32)
    done = np.zeros(B, dtype=bool)
    w = np.ones(V)
    w[0] = 0
    rows, gaps, lps, nlls, loss = [], [], [], [], 0.0
    for step in range(stop_limit):
        logits, ht, _ = m.decode_step(word, ht, step=step)
        lg = np.asarray(logits.data)
        srt = np.sort(lg, axis=1)
        gaps.append(srt[:, -1] - srt[:, -2])
        word = lg.argmax(axis=1).astype(np.int32)
        lp, nl = _score_rows(lg, word, y, step, V)
        if y is not None and step + 1 < y.shape[1]:
            ce = float(F.softmax_cross_entropy(logits, y[:, step + 1], class_weight=w).data)
            assert abs(ce - nl.sum() / B) < 1e-9 * max(1.0, abs(ce))       # (the per-element restatement is the oracle's value)
            loss += ce
        lps.append(lp)
        nlls.append(nl)
        rows.append(word)
        done[word == EOS] = True
        if done.all():
            break
    return np.stack(rows, 0).T, np.stack(gaps, 0), np.stack(lps, 0), np.stack(nlls, 0), loss


def _scored(m, X, stop_limit, y=None, path="device"):
    r = m.predict_scored(torch.from_numpy(X), GO, EOS, stop_limit, y=None if y is None else torch.from_numpy(y))
    assert m.last_predict_path == path, m.last_predict_path
    return r


# ---------------------------------------------------------------- oracle parity at full size
@pytest.mark.parametrize("shape", [CFG1, ES_EN], ids=["configs1", "es_en_20h"])
def test_scored_matches_oracle_full_size(shape):
    """The inputs of test_greedy_matches_oracle_full_size with targets synth_batch(32, 8, 80, 41, V, seed=5)[1].  Figures measured on
    one MI355X are in the result table of DESIGN.md section 12."""
    from oracle import ast_ref as R
    V = shape["V"]
    cfg, P, X, m = _setup(shape, 32, 800, seed=3)
    y = R.synth_batch(32, 8, 80, 41, V, seed=5)[1]
    ref, gaps, rlp, rnl, rloss = _oracle_greedy(cfg, P, X, V, 40, y)
    ok = _guard(ref, gaps, 1e-3)
    frac = ok.sum() / ok.size
    print(f"\n{'es_en_20h' if shape is ES_EN else 'configs1'}: oracle n_steps {ref.shape[1]}, guarded {frac:.3f}, min gap {gaps.min():.3e}, "
          f"loss {rloss:.6f}")
    assert frac >= 0.9
    # the per-step loop's own error against the oracle on the same positions: e_loop
    ltok, _, llp, lnl = _loop(m, X, 40, y)
    n = min(ltok.shape[1], ref.shape[1])
    okl = ok[:, :n]
    assert (ltok[:, :n][okl] == ref[:, :n][okl]).all()
    e1, _ = _max_err("per-step loop logp vs oracle", llp[:n].T, rlp[:n].T, okl)
    e2, _ = _max_err("per-step loop nll  vs oracle", lnl[:n].T, rnl[:n].T, okl)
    print(f"  e_loop = {max(e1, e2):.3e}")
    got = _scored(m, X, 40, y)
    print(f"  device n_steps {got.n_steps}, loss {got.loss:.6f} (oracle {rloss:.6f}, rel {abs(got.loss - rloss) / abs(rloss):.3e})")
    n = min(got.n_steps, ref.shape[1])
    okd = ok[:, :n]
    assert (got.tokens[:, :n][okd] == ref[:, :n][okd]).all()
    _, r1 = _max_err("device logp vs oracle", got.logp[:, :n], rlp[:n].T, okd)
    _, r2 = _max_err("device nll  vs oracle", got.nll[:, :n], rnl[:n].T, okd)
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)
    if shape is ES_EN:      # every position is guarded there
        assert ok.all()
        assert got.n_steps == ref.shape[1] and got.tokens.shape == ref.shape
        assert abs(got.loss - rloss) <= 1e-4 * abs(rloss), (got.loss, rloss)
        assert abs(rloss - 249.0655) < 1e-3
        # the per-hypothesis score: the oracle's log-probabilities up to the first EOS
        want = np.array([rlp[:(int(np.nonzero(ref[b] == EOS)[0][0]) + 1) if (ref[b] == EOS).any() else ref.shape[1], b].sum() for b in range(32)])
        print(f"  score: max abs err {np.abs(got.score - want).max():.3e}, max |value| {np.abs(want).max():.3f}")
        assert (np.abs(got.score - want) <= tol(want)).all(), np.abs(got.score - want).max()


# ---------------------------------------------------------------- the device loop against the per-step loop
def _compare_runs(tag, dev, ref):
    """A device-loop ScoredPrediction against the per-step loop's: tokens and n_steps equal, the rest within tol()."""
    assert dev.n_steps == ref.n_steps and (dev.tokens == ref.tokens).all(), (tag, dev.tokens, ref.tokens)
    allpos = np.ones(ref.tokens.shape, dtype=bool)
    worst = _max_err(f"{tag} logp", dev.logp, ref.logp.astype(np.float64), allpos)[1]
    if ref.nll is None:
        assert dev.nll is None and dev.loss is None
    else:
        worst = max(worst, _max_err(f"{tag} nll", dev.nll, ref.nll.astype(np.float64), allpos)[1])
        print(f"  {tag} loss {dev.loss:.6f} / {ref.loss:.6f}")
        assert abs(dev.loss - ref.loss) <= tol(ref.loss), (tag, dev.loss, ref.loss)
    assert worst <= 1.0, (tag, worst)
    assert (np.abs(dev.score - ref.score) <= tol(ref.score)).all(), (tag, dev.score, ref.score)


@pytest.mark.parametrize("B", [1, 5, 16, 17, 32])
def test_device_loop_matches_step_loop(B, tune):
    stop, V = 24, MID["V"]
    # no EOS ever: the batch stops at stop_limit
    _, _, X, m = _setup(MID, B, 120, seed=5, eos_bias=-1e4)
    dist = []
    ref, gaps, _, _ = _loop(m, X, stop, eos_dist=dist)
    assert ref.shape == (B, stop) and gaps.min() > 1e-4
    # ... and an EOS offset that lets every row finish within the first steps, each at its own step (as test_stop_rule_matches_step_loop)
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
        ref, gaps, _, _ = _loop(m, X, stop)
        n = ref.shape[1]
        assert gaps.min() > 1e-4, gaps.min()
        assert n == stop if case == "never" else 1 <= n < stop, (case, n)
        print(f"\nB {B} {case}: n_steps {n}")
        # targets whose L - 1 lies below, at and above the step count at which the batch stops; and none
        for L in sorted({max(n - 3, 1), n, n + 1, n + 5}) + [None]:
            y = None if L is None else _targets(B, L, V, seed=100 + L)
            tune("dec.persist", 1)
            dev = _scored(m, X, stop, y)
            tune("dec.persist", 0)
            loop = _scored(m, X, stop, y, path="steps")
            assert (loop.tokens == ref).all()
            _compare_runs(f"B {B} {case} L {L}", dev, loop)
            if y is not None and L - 1 < n:
                assert (dev.nll[:, L - 1:] == 0).all()           # steps past L - 1 have no target
        tune("dec.persist", 1)


def test_long_run_on_streamed_slices_matches_step_loop(tune):
    """T'' = 420 (the loader's longest bucket): the streamed-slice variant of the scored kernel, 175 steps, targets for the first 59."""
    _, _, X, m = _setup(ES_EN, 32, 4 * 420, seed=7, eos_bias=-1e4)
    y = _targets(32, 60, ES_EN["V"], seed=9)
    dev = _scored(m, X, 175, y)
    assert m._cur["T2"] == 420
    ref, gaps, lp, nl = _loop(m, X, 175, y)
    assert dev.tokens.shape == ref.shape == (32, 175)
    ok = _guard(ref, gaps, 1e-5)
    print(f"\nlong run: guarded {ok.sum() / ok.size:.3f}, min gap {gaps.min():.3e}")
    assert ok.sum() >= 0.9 * ok.size
    assert (dev.tokens[ok] == ref[ok]).all()
    _, r1 = _max_err("long logp", dev.logp, lp.T, ok)
    _, r2 = _max_err("long nll", dev.nll, nl.T, ok)
    assert r1 <= 1.0 and r2 <= 1.0
    assert (dev.nll[:, 59:] == 0).all()
    if ok[:, :59].all():
        want = nl[:59].sum() / 32
        print(f"  loss {dev.loss:.6f} / {want:.6f}")
        assert abs(dev.loss - want) <= tol(want)


# ---------------------------------------------------------------- nothing else moved
def test_predict_and_training_are_untouched_by_a_scored_decode():
    from ast_amd import _lib
    from ast_amd.seq2seq import using_config
    from oracle import ast_ref as R
    cfg, P, X, m = _setup(MID, 17, 120, seed=9, eos_bias=8.0)
    y = _targets(17, 12, MID["V"], seed=3)
    a = m.predict(torch.from_numpy(X), GO, EOS, 30)
    path_a = m.last_predict_path
    r = _scored(m, X, 30, y)
    r2 = _scored(m, X, 30, y)
    b = m.predict(torch.from_numpy(X), GO, EOS, 30)
    assert path_a == m.last_predict_path == "device"
    assert a.dtype == np.int32 and a.shape == b.shape and (a == b).all()
    assert (r.tokens == a).all() and r.tokens.dtype == np.int32
    assert (r.tokens == r2.tokens).all() and (r.logp == r2.logp).all() and (r.nll == r2.nll).all() and r.loss == r2.loss
    mask = C.c_uint(7)
    assert _lib.load().astk_persist_status(C.byref(mask), 0) == 0 and mask.value == 0
    # a train step after the scored decode gives the same bits as on a model that never decoded
    _, _, _, fresh = _setup(MID, 17, 120, seed=9, eos_bias=8.0)
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
    assert out[0][0] == out[1][0]
    assert torch.equal(out[0][1], out[1][1])


def test_nn_predict_scored_returns_nn_predicts_preds(tune):
    from ast_amd import nn as gnn
    _, _, _, m = _setup(ES_EN, 8, 240, seed=15, eos_bias=3.0)
    rng = np.random.default_rng(0)
    batches = []
    for i, (B, T, L) in enumerate(((8, 240, 9), (5, 320, 14), (8, 200, 40), (3, 400, 5))):
        batches.append({"X": rng.standard_normal((B, T, 80)).astype(np.float32), "utts": [f"u{i}_{j}" for j in range(B)],
                        "y": torch.from_numpy(_targets(B, L, ES_EN["V"], seed=40 + i))})
    for b in batches:
        _, gaps, _, _ = _loop(m, b["X"], 30)
        assert gaps.min() > 1e-4, gaps.min()
    asked = []

    def get_batch(batch_size, set_key, train, labels=False):
        asked.append((train, labels))
        return iter(batches)
    stub = types.SimpleNamespace(model=m, cfg=types.SimpleNamespace(train={"data": {"max_pred": 30}, "batch_size": 8}),
                                 data_loader=types.SimpleNamespace(n_utts={"dev": sum(len(b["utts"]) for b in batches)}, get_batch=get_batch))
    plain = gnn.NN.predict(stub, "dev")
    preds, dev_loss, scores = gnn.NN.predict_scored(stub, "dev")
    assert m.last_predict_path == "device"
    assert asked == [(False, False), (False, True)]
    assert preds == plain
    assert [u for u, _ in scores] == [u for u, _ in preds] and all(s <= 0 for _, s in scores)
    # the figure: mean over the batches of loss / padded target length, from predict_scored batch by batch
    want = np.mean([m.predict_scored(torch.from_numpy(b["X"]), GO, EOS, 30, y=b["y"]).loss / b["y"].shape[1] for b in batches])
    assert abs(dev_loss - want) <= 1e-12 * abs(want), (dev_loss, want)
    tune("dec.persist", 0)
    preds_off, loss_off, scores_off = gnn.NN.predict_scored(stub, "dev")
    assert m.last_predict_path == "steps"
    assert preds_off == preds
    assert abs(loss_off - dev_loss) <= tol(dev_loss), (loss_off, dev_loss)
    assert (np.abs(np.array([s for _, s in scores_off]) - np.array([s for _, s in scores])) <= tol(np.array([s for _, s in scores]))).all()


def test_train_py_dev_log_with_and_without_dev_loss(tmp_path):
    """Without --dev-loss the dev log line is `epoch, BLEU` as before; with it a third column that is NN.predict_scored's figure."""
    import json, os, re, subprocess, sys
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

    def run(*extra):
        r = subprocess.run([sys.executable, os.path.join(root, "train.py"), "-m", str(tmp_path), "-e", "1"] + list(extra), cwd=root,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    out1 = run()
    assert "dev loss" not in out1
    lines = open(tmp_path / "dev.log").read().split("\n")
    assert len(lines) == 2 and lines[1] == "" and re.fullmatch(r"1, \d+\.\d\d", lines[0]), lines
    # ... whose figure is the BLEU of NN.predict on epoch 1's checkpoint, as it always was
    from ast_amd.eval import Eval
    nn = NN(str(tmp_path))
    assert nn.max_epoch == 1
    bleu1 = Eval(str(refs), 1).calc_bleu(nn.data_loader.get_hyps(nn.predict("syn_dev"))) * 100
    assert abs(float(lines[0].split(", ")[1]) - bleu1) <= 0.00501, (lines[0], bleu1)
    del nn
    torch.cuda.empty_cache()
    out2 = run("--dev-loss")
    lines = open(tmp_path / "dev.log").read().split("\n")
    assert len(lines) == 3 and re.fullmatch(r"1, \d+\.\d\d", lines[0]) and re.fullmatch(r"2, \d+\.\d\d, \d+\.\d{4}", lines[1]), lines
    # the resumed model (epoch 2's checkpoint) gives the same figures in-process
    nn = NN(str(tmp_path))
    assert nn.max_epoch == 2
    preds, dev_loss, scores = nn.predict_scored("syn_dev")
    assert sorted(preds) == sorted(nn.predict("syn_dev"))             # (the loader shuffles the order of the dev batches)
    bleu = Eval(str(refs), 1).calc_bleu(nn.data_loader.get_hyps(preds)) * 100
    # equal at the printed precision (half a unit of the last place, and the rounding of a mean taken in another batch order)
    col = [float(v) for v in lines[1].split(", ")]
    assert abs(col[1] - bleu) <= 0.00501 and abs(col[2] - dev_loss) <= 0.0000501, (lines[1], bleu, dev_loss)
    assert "dev loss = {0:.4f}".format(col[2]) in out2
    assert len(scores) == 7 and dev_loss > 0


# ---------------------------------------------------------------- fallbacks
@pytest.mark.parametrize("shape,over,B", [(MID, {"ln": True}, 4), (MID, {"n_attn": 2}, 4), (MID, {"feed_attn": False}, 4), (MID, {}, 48),
                                          (WIDE, {}, 4)], ids=["ln", "n_attn2", "no_feed_attn", "B48", "wide"])
def test_fallback_shapes_score_on_the_step_loop(shape, over, B):
    from ast_amd import _lib
    cfg, P, X, m = _setup(shape, B, 120, seed=11, **over)
    V = shape["V"]
    y = _targets(B, 5, V, seed=2)
    got = _scored(m, X, 8, y, path="steps")
    assert _lib.load().astk_greedy_scored_workspace_bytes(C.byref(m._cur["dd"]), 8) == 0
    plain = m.predict(torch.from_numpy(X), GO, EOS, 8)
    assert m.last_predict_path == "steps" and (plain == got.tokens).all()
    ref, gaps, rlp, rnl, rloss = _oracle_greedy(cfg, P, X, V, 8, y)
    ok = _guard(ref, gaps, 1e-3)
    n = min(got.n_steps, ref.shape[1])
    ok = ok[:, :n]
    print(f"\nfallback: guarded {ok.sum()} of {ref.size}, loss {got.loss:.6f} / oracle {rloss:.6f}")
    assert ok.sum() >= 0.9 * ref.size
    assert (got.tokens[:, :n][ok] == ref[:, :n][ok]).all()
    _, r1 = _max_err("fallback logp vs oracle", got.logp[:, :n], rlp[:n].T, ok)
    _, r2 = _max_err("fallback nll  vs oracle", got.nll[:, :n], rnl[:n].T, ok)
    assert r1 <= 1.0 and r2 <= 1.0
    assert (got.nll[:, 4:] == 0).all()
    if ok.all() and got.n_steps == ref.shape[1]:
        assert abs(got.loss - rloss) <= 1e-4 * abs(rloss)
    none = _scored(m, X, 8, None, path="steps")
    assert none.nll is None and none.loss is None and (none.tokens == got.tokens).all() and (none.logp == got.logp).all()


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
    nbytes = lib.astk_greedy_scored_workspace_bytes(C.byref(dd), 10)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=m.device)
    toks = torch.empty(10 * 4, dtype=torch.int32, device=m.device)
    logp = torch.empty(10 * 4, dtype=torch.float32, device=m.device)
    nll = torch.empty(10 * 4, dtype=torch.float32, device=m.device)
    nst = torch.zeros(4, dtype=torch.int32, device=m.device)
    y = torch.from_numpy(_targets(4, 6, MID["V"], seed=1)).to(m.device)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(d=dd, go=GO, eos=EOS, stop=10, wsz=nbytes, y=y, ldy=6, toks=toks, logp=logp, nll=nll, nst=nst, enc=st["enc_states"]):
        return lib.astk_greedy_decode_scored(C.byref(d), C.byref(st["dp"]), P(enc), P(m._dec_c), P(m._dec_h), go, eos, stop, P(y), ldy,
                                             P(m.mask_pad_id), P(toks), P(logp), P(nll), P(nst), None, P(ws), wsz, None)
    bad = _lib.DecoderDesc.from_buffer_copy(dd)
    bad.struct_size -= 8
    off = _lib.DecoderDesc.from_buffer_copy(dd)
    off.ln = 1
    for kw, word in ((dict(d=bad), b"struct_size"), (dict(go=-1), b"go"), (dict(eos=MID["V"]), b"eos"), (dict(stop=0), b"stop_limit"),
                     (dict(stop=513), b"stop_limit"), (dict(d=off), b"device loop"), (dict(wsz=nbytes - 1), b"workspace too small"),
                     (dict(toks=None), b"null pointer"), (dict(nst=None), b"null pointer"), (dict(enc=None), b"null pointer"),
                     (dict(logp=None), b"null pointer"), (dict(nll=None), b"nll goes with y"), (dict(y=None), b"nll goes with y"),
                     (dict(ldy=0), b"ldy")):
        assert call(**kw) < 0, kw
        assert word in lib.astk_last_error(), (kw, lib.astk_last_error())
    torch.cuda.synchronize()
    mask = C.c_uint(7)
    assert lib.astk_persist_status(C.byref(mask), 0) == 0 and mask.value == 0
    assert call() == 0
    assert call(y=None, nll=None, ldy=0) == 0                  # without targets ldy is not looked at
    torch.cuda.synchronize()
    assert 1 <= int(nst[0]) <= 10
    assert lib.astk_persist_status(C.byref(mask), 0) == 0 and mask.value == 0
