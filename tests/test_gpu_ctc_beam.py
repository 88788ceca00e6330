"""GPU tests of the CTC prefix beam search (include/astk.h astk_ctc_beam): the operator through the C ABI on the
named cases of tests/ctc_beam_model.py -- tokens, label counts and rank order EQUAL to the float64 host model's for every row and slot
(tests/test_ctc_beam_host.py holds every case to a smallest non-zero gap of 1e-7, so nothing is excluded), scores within
1e-10 * max(1, |score|), run-to-run bits, untouched logits, the guarded workspace, the refusals -- then SpeechEncoderDecoder.ctc_beam,
rescore_ctc_nbest and ctc_decode.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_beam_model as BM
import ctc_model as CM
import schedule_helpers as SH
from conftest import tiny_cfg
from test_ctc_beam_host import GOOD, REFUSALS
from test_gpu_ops import GuardedWS, dev, ok, stream, vp

pytestmark = pytest.mark.gpu

# Section 30's derived bound: a few ulp (1.1e-16 relative) per frame over at most 2048 frames is below 1e-12; two orders of magnitude
# on top for another summation order in the log-sum-exp.
SCORE_TOL = 1e-10


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


def _run_op(lib, c):
    """astk_ctc_beam on one case's host arrays; the outputs as host arrays and the logits buffer before and after."""
    from ast_amd import _lib
    x, lens, N, Cc, Lm = c["logits"], c["lens"], c["N"], c["C"], c["max_labels"]
    B, T, V = x.shape
    ldv = c.get("ldv") or V
    buf = torch.full((B, T, ldv), 7.0, device="cuda")
    buf[:, :, :V] = dev(x)
    before = buf.clone()
    len_d = None if lens is None else dev(lens, torch.int32)
    d = _lib.CtcBeamDesc(B, T, V, ldv, N, Cc, Lm, BM.UNK_ID, BM.PAD_ID)
    nbytes = lib.astk_ctc_beam_workspace_bytes(C.byref(d))
    assert nbytes > 0, lib.astk_last_error().decode()
    ws = GuardedWS(nbytes)
    tokens = torch.full((B, N, Lm), -7, dtype=torch.int32, device="cuda")
    n_labels = torch.full((B, N), -7, dtype=torch.int32, device="cuda")
    score = torch.full((B, N), 5.0, dtype=torch.float64, device="cuda")
    ok(lib, lib.astk_ctc_beam(C.byref(d), vp(buf), vp(len_d), vp(tokens), vp(n_labels), vp(score), vp(ws), ws.nbytes, stream()))
    ws.check("ctc_beam")
    return dict(tokens=tokens.cpu().numpy(), n_labels=n_labels.cpu().numpy(), score=score.cpu().numpy(), logits_before=before, logits_after=buf)


def _assert_equal_to_model(got, want, what):
    """Every row and slot: the same strings in the same order; scores within the bound, -inf and the unused slots exactly."""
    assert np.array_equal(got["n_labels"], want["n_labels"]), (what, got["n_labels"], want["n_labels"])
    assert np.array_equal(got["tokens"], want["tokens"]), what
    inf = np.isinf(want["score"])
    assert np.array_equal(np.isinf(got["score"]), inf) and (got["score"][inf] == want["score"][inf]).all(), what
    err = np.abs(got["score"][~inf] - want["score"][~inf]) / np.maximum(1.0, np.abs(want["score"][~inf]))
    print(what, "largest score error / max(1, |score|)", err.max(initial=0.0), "bound", SCORE_TOL)
    assert (err <= SCORE_TOL).all(), (what, err.max())


@pytest.mark.parametrize("name", BM.ALL_CASES)
def test_ctc_beam_equals_the_float64_model(lib, name):
    c, m = BM.result(name)
    r = _run_op(lib, c)
    assert torch.equal(r["logits_before"].view(torch.int32), r["logits_after"].view(torch.int32)), "the logits were written"
    _assert_equal_to_model(r, m, name)
    if c["lens"] is not None:
        for b in np.flatnonzero(np.asarray(c["lens"]) == 0):                  # n = 0: the empty string with score 0 in slot 0
            assert r["n_labels"][b].tolist() == [0] + [-1] * (c["N"] - 1) and r["score"][b, 0] == 0.0
            assert (r["score"][b, 1:] == -np.inf).all() and (r["tokens"][b] == BM.PAD_ID).all()


@pytest.mark.parametrize("name", ["small-v", "long", "twin-columns", "ldv"])
def test_ctc_beam_is_bit_identical_from_run_to_run(lib, name):
    c, _ = BM.result(name)
    a, b = _run_op(lib, c), _run_op(lib, c)
    assert np.array_equal(a["tokens"], b["tokens"]) and np.array_equal(a["n_labels"], b["n_labels"])
    assert np.array_equal(a["score"].view(np.int64), b["score"].view(np.int64))


def test_ctc_beam_with_another_blank_and_first_label(lib):
    """blank = 1, first_label = 4 and input_len NULL: the model under the same ids."""
    from ast_amd import _lib
    x = BM.case("random-2")["logits"]
    B, T, V = x.shape
    m = BM.search(x, None, 3, 2, 9, first_label=4, blank=1)
    assert min(st["min_gap"] for st in m["stats"]) >= 1e-7
    d = _lib.CtcBeamDesc(B, T, V, V, 3, 2, 9, 4, 1)
    ws = GuardedWS(lib.astk_ctc_beam_workspace_bytes(C.byref(d)))
    tokens = torch.full((B, 3, 9), -7, dtype=torch.int32, device="cuda")
    n_labels = torch.full((B, 3), -7, dtype=torch.int32, device="cuda")
    score = torch.full((B, 3), 5.0, dtype=torch.float64, device="cuda")
    ok(lib, lib.astk_ctc_beam(C.byref(d), vp(dev(x)), None, vp(tokens), vp(n_labels), vp(score), vp(ws), ws.nbytes, stream()))
    ws.check("ctc_beam")
    got = dict(tokens=tokens.cpu().numpy(), n_labels=n_labels.cpu().numpy(), score=score.cpu().numpy())
    want = dict(m, tokens=np.where(np.arange(9) < m["n_labels"][:, :, None], m["tokens"], 1))
    _assert_equal_to_model(got, want, "blank 1, first label 4")
    assert (got["n_labels"] == 9).any()                                       # (and max_labels below T caps the strings)


def test_ctc_beam_refuses_bad_arguments_before_any_launch(lib):
    from ast_amd import _lib
    g = GOOD
    buf = torch.full((g["B"], g["T"], g["ldv"]), 2.0, device="cuda")
    tokens = torch.full((g["B"], g["N"], g["max_labels"]), -5, dtype=torch.int32, device="cuda")
    n_labels = torch.full((g["B"], g["N"]), -5, dtype=torch.int32, device="cuda")
    score = torch.full((g["B"], g["N"]), -1.0, dtype=torch.float64, device="cuda")
    ws = GuardedWS(1 << 16)

    def call(d, logits=buf, tok=tokens, nl=n_labels, sc=score, w=ws, nbytes=None):
        return lib.astk_ctc_beam(C.byref(d), vp(logits), None, vp(tok), vp(nl), vp(sc), vp(w), ws.nbytes if nbytes is None else nbytes, stream())

    def untouched():
        torch.cuda.synchronize()
        assert float((buf - 2.0).abs().max()) == 0.0 and float((score + 1.0).abs().max()) == 0.0
        assert int((tokens != -5).sum()) == 0 and int((n_labels != -5).sum()) == 0
        assert int((ws.t != 0x5A).sum()) == 0, "the refused call launched something"
    for field, value, word in REFUSALS + (("struct_size", 8, "struct_size"),):
        d = _lib.CtcBeamDesc(**{**g, **({field: value} if field != "struct_size" else {})})
        if field == "struct_size":
            d.struct_size = value
        if field == "V":
            d.ldv = value
        assert lib.astk_ctc_beam_workspace_bytes(C.byref(d)) == 0
        assert call(d) < 0
        assert word in lib.astk_last_error().decode(), (field, lib.astk_last_error().decode())
        untouched()
    d = _lib.CtcBeamDesc(**g)
    need = lib.astk_ctc_beam_workspace_bytes(C.byref(d))
    assert 0 < need <= ws.nbytes
    assert call(d, nbytes=need - 1) < 0 and "workspace" in lib.astk_last_error().decode()
    untouched()
    for kw in (dict(logits=None), dict(tok=None), dict(nl=None), dict(sc=None), dict(w=None)):
        assert call(d, **kw) < 0 and "null" in lib.astk_last_error().decode(), kw
        untouched()
    assert call(d, nbytes=need) == 0                                          # (and the good call goes through)
    torch.cuda.synchronize()
    assert int((tokens == -5).sum()) == 0 and int((n_labels == -5).sum()) == 0


# ------------------------------------------------------------------ 2. model level
def _head_model():
    """A model with the head on the small golden shape (B = 2, T = 37), a bias on the blank so that the strings stay short."""
    cfg = tiny_cfg(c1=8)
    cfg["rnn_config"]["ctc"] = True
    B, T, D, L, V = 2, 37, 26, 6, 11
    P, X, y = SH.make_inputs(cfg, B, T, D, L, V)
    P = dict(P)
    P.update(CM.head_params(cfg["rnn_config"]["hidden_units"], V))
    P["ctc_out/b"] = P["ctc_out/b"].copy()
    P["ctc_out/b"][0] += 0.3
    return cfg, SH.gpu_model(cfg, P, D, V), X, V


def test_seq2seq_ctc_beam_and_the_second_pass(lib):
    """Ragged x_lens: every row's list equals the host model run on the head's logits read back from the device; hyp = [GO] + labels
    + [EOS]; every score <= total_logp of ctc_align on the same labels within that test's float32 tolerance; ctc_predict returns what
    it returned before; rescore_ctc_nbest reproduces (1 - w) A + w C with A from score_hypotheses, one utterance at a time."""
    from ast_amd.nn import rescore_ctc_nbest, score_hypotheses
    from ast_amd.seq2seq import cnn_out_lens, using_config
    cfg, g, X, V = _head_model()
    Xt = torch.from_numpy(X)
    x_lens = np.asarray([37, 29], np.int32)
    greedy = g.ctc_predict(Xt, x_lens=x_lens)
    rows = g.ctc_beam(Xt, x_lens=x_lens, N=4, C=3)
    logits, Vp = g._ctc_logits(g._cur, g._stream())
    T2 = g._cur["T2"]
    lg = logits.view(len(X), T2, Vp)[:, :, :V].cpu().numpy()
    lens = np.asarray([cnn_out_lens(cfg["cnn_config"]["cnn_layers"], int(n))[-1] for n in x_lens], np.int32)
    m = BM.search(lg, lens, 4, 3, min(T2, 255))
    print("smallest non-zero gap on the head's logits", min(st["min_gap"] for st in m["stats"]))
    assert min(st["min_gap"] for st in m["stats"]) >= 1e-7 and (lens < T2).any()
    assert g.ctc_predict(Xt, x_lens=x_lens) == greedy
    assert greedy == [list(CM.collapse(lg[b, :lens[b]].argmax(axis=1))) for b in range(len(X))]
    for b, row in enumerate(rows):
        k = int((m["n_labels"][b] >= 0).sum())
        assert len(row) == k >= 1
        for r, e in enumerate(row):
            want = m["tokens"][b, r, :m["n_labels"][b, r]].tolist()
            assert e["labels"] == want and e["hyp"] == [BM.GO_ID] + want + [BM.EOS_ID]
            assert abs(e["score"] - m["score"][b, r]) <= SCORE_TOL * max(1.0, abs(m["score"][b, r]))
        # the full sums of the row's strings, from the alignment's float32 loss pass
        y = np.zeros((k, max(max(len(e["labels"]) for e in row), 1)), np.int32)
        for r, e in enumerate(row):
            y[r, :len(e["labels"])] = e["labels"]
        al = g.ctc_align(Xt[b:b + 1].expand(k, -1, -1), y, x_lens=np.full(k, x_lens[b], np.int32))
        for e, a in zip(row, al):
            print("row", b, e["labels"], "score", e["score"], "total_logp", a["total_logp"])
            assert e["score"] <= a["total_logp"] + 1e-4 * abs(a["total_logp"])
    one = g.ctc_beam(Xt, N=1, C=1, max_labels=2)
    assert all(len(r) == 1 and len(r[0]["labels"]) <= 2 for r in one)
    # ---- the second pass
    w = 0.3
    Xs = [Xt[b:b + 1, :int(x_lens[b])] for b in range(len(X))]
    with using_config("train", False):
        first = [g.ctc_beam(x, N=4, C=3)[0] for x in Xs]
        att = [score_hypotheses(g, x, [e["hyp"] for e in lst])[0] for x, lst in zip(Xs, first)]
    second = rescore_ctc_nbest(g, Xs, first, w, max_utts=2)
    for lst, A, out in zip(first, att, second):
        want = sorted(((1 - w) * a + w * e["score"], e["hyp"], a, e["score"]) for e, a in zip(lst, A))[::-1]
        assert [e["hyp"] for e in out] == [h for _, h, _, _ in want]
        for e, (s, _, a, c) in zip(out, want):
            assert e["ctc_score"] == c and abs(e["att_score"] - a) <= 1e-5 * abs(a) and abs(e["score"] - ((1 - w) * e["att_score"] + w * c)) <= 1e-12
    with pytest.raises(ValueError, match="rnn_config.ctc"):
        SH.gpu_model(tiny_cfg(), SH.make_inputs(tiny_cfg(), 2, 21, 26, 5, 11)[0], 26, 11).ctc_beam(torch.zeros(2, 21, 26))


def test_ctc_decode_py_writes_a_pickle_score_py_reads(tmp_path):
    """`python ctc_decode.py` on the synthetic corpus, then `python score.py --nbest` on its pickle; the pickle is what NN.ctc_beam_set
    returns, in sample_set's layout; the second pass of the command line appends the two terms."""
    import importlib.util, json, os, pickle, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mcfg = tiny_cfg(enc_layers=2, dec_layers=1, H=32, E=16, A=32, c0=8, c1=16, V=31, drop=0.0)
    del mcfg["rnn_config"]["dec_vocab_size"]
    mcfg["rnn_config"]["ctc"] = True
    tcfg = {"seed": "seed-ast-20h", "gpuid": 0, "batch_size": 4, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 1,
            "optimizer": {"type": 0, "lr": 2e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0},
            "data": {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 8, "syn_dev": 6},
                     "frames": [60, 300], "targets": [2, 9], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w"}}
    json.dump(mcfg, open(tmp_path / "model_cfg.json", "w"))
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))
    out = str(tmp_path / "nbest.p")
    r = subprocess.run([sys.executable, os.path.join(root, "ctc_decode.py"), "-m", str(tmp_path), "-s", "syn_dev", "-n", "3", "-c", "4", "-w", out],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Hypotheses written to: {0:s} (utterances: 6".format(out) in r.stdout
    nbest = pickle.load(open(out, "rb"))
    r = subprocess.run([sys.executable, os.path.join(root, "score.py"), "-m", str(tmp_path), "-s", "syn_dev", "--nbest", out, "-b", "4"], cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    n_hyps = sum(len(v) for v in nbest.values())
    assert "hypotheses scored = {0:d}".format(n_hyps) in r.stdout
    from ast_amd import nn as N
    nn = N.NN(str(tmp_path))
    assert sorted(nbest) == sorted(nn.data_loader.info["syn_dev"]) and nn.ctc_beam_set("syn_dev", 3, 4) == nbest
    for lst in nbest.values():
        assert 1 <= len(lst) <= 3 and [s for _, s, _ in lst] == sorted((s for _, s, _ in lst), reverse=True)
        for hyp, s, hist in lst:
            assert hyp[0] == BM.GO_ID and hyp[-1] == BM.EOS_ID and all(t >= BM.UNK_ID for t in hyp[1:-1]) and hist == [] and s <= 0.0
    spec = importlib.util.spec_from_file_location("ctc_decode_cli", os.path.join(root, "ctc_decode.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    both = cli.rescore_set(nn, "syn_dev", nbest, 0.25, 4)
    assert sorted(both) == sorted(nbest)
    for u, lst in both.items():
        assert sorted(tuple(h) for h, *_ in lst) == sorted(tuple(h) for h, _, _ in nbest[u])
        ctc = {tuple(h): s for h, s, _ in nbest[u]}
        for hyp, s, hist, a, c in lst:
            assert c == ctc[tuple(hyp)] and abs(s - (0.75 * a + 0.25 * c)) <= 1e-12 and hist == []
        assert [e[1] for e in lst] == sorted((e[1] for e in lst), reverse=True)
