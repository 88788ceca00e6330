"""Batched beam search (ast_amd.nn.decode_beam_batch, csrc/beam.hip): the per-row attention scan, the select / gather kernel against a
NumPy restatement of the reference's candidate and selection rule, and whole searches against the float64 oracle's decode_beam and
the per-utterance GPU path, utterance by utterance; beam.py -b end to end; argument checks of the C ABI."""
import copy
import ctypes as C
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import tiny_cfg

pytestmark = pytest.mark.gpu

GO, EOS = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- NumPy restatement of one step (nn.py:235-322 per utterance)
def np_select(logits, score, status, tokens, N, K, eos):
    """-> per new slot (parent, token, carried, score, status), slot by slot in the reference's candidate order, stable top-N."""
    R, V = logits.shape
    out = []
    for u in range(R // N):
        cands = []
        for j in range(N):
            r = u * N + j
            if status[r] == 0:
                continue
            if status[r] == 2:
                cands.append((float(score[r]), j, int(tokens[r]), 1))
                continue
            x = logits[r].astype(np.float64)
            lp = x - (np.log(np.exp(x - x.max()).sum()) + x.max())
            order = np.lexsort((np.arange(V), -lp))[:K]          # higher logp first, equal ones lower token id first
            cands += [(float(score[r]) + float(lp[v]), j, int(v), 0) for v in order]
        best = sorted(cands, key=lambda t: -t[0])[:N]            # stable: equal scores keep the earlier candidate
        for i in range(N):
            if i < len(best):
                s, p, t, car = best[i]
                out.append((p, t, car, s, 2 if (car or t == eos) else 1))
            else:
                out.append((-1, 0, 0, 0.0, 0))
    return out


def _lib():
    from ast_amd import _lib as L
    return L, L.load()


def _state(U, N, S, T, nl, H, A, dev="cuda"):
    R = U * N
    i32 = dict(dtype=torch.int32, device=dev)
    st = dict(row_utt=torch.arange(R, **i32) // N, row_len=torch.full((R,), T, **i32),
              c=torch.randn(nl, R, H, device=dev), h=torch.randn(nl, R, H, device=dev), ht=torch.randn(R, A, device=dev),
              tokens=torch.zeros(R, **i32), score=torch.zeros(R, dtype=torch.float64, device=dev), status=torch.zeros(R, **i32),
              frozen=torch.zeros(U, **i32), n_frozen=torch.zeros(1, **i32), hist=torch.zeros(S, R, 4, **i32),
              hist_alpha=torch.zeros(S, R, T, device=dev))
    return st


def _descs(L, U, N, K, S, T, V, st, lens=None):
    lens = np.asarray(lens if lens is not None else [T] * U, dtype=np.int32)
    bd = L.BeamDesc(U, N, K, S, T, V, EOS, lens.ctypes.data_as(C.POINTER(C.c_int32)))
    keys = ("row_utt", "row_len", "c", "h", "ht", "tokens", "score", "status", "frozen", "n_frozen", "hist", "hist_alpha")
    bs = L.BeamState(*[st[k].data_ptr() for k in keys])
    return bd, bs, lens


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------- op level: attention over per-row encoder slices
def test_attention_rows_cover_their_own_utterance_slice():
    L, lib = _lib()
    torch.manual_seed(0)
    H, lens, per = 128, [37, 50, 23, 8], 3
    U, T = len(lens), max(lens)
    enc = torch.randn(U, T, H, device="cuda")
    row_utt = torch.tensor([u for u in range(U) for _ in range(per)], dtype=torch.int32, device="cuda")
    row_len = torch.tensor([lens[u] for u in range(U) for _ in range(per)], dtype=torch.int32, device="cuda")
    R = row_utt.numel()
    q = torch.randn(R, H, device="cuda") * 0.3
    Tp = (T + 3) // 4 * 4
    alpha = torch.full((R, Tp), 7.0, device="cuda")
    cv = torch.zeros(R, H, device="cuda")
    nb = int(lib.astk_attn_workspace_bytes(R, T, H))
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    L.check(lib.astk_attn_step_fwd_rows(R, T, H, C.c_void_p(enc.data_ptr()), C.c_void_p(row_utt.data_ptr()), C.c_void_p(row_len.data_ptr()),
                                        C.c_void_p(q.data_ptr()), C.c_void_p(alpha.data_ptr()), C.c_void_p(cv.data_ptr()), C.c_void_p(ws.data_ptr()),
                                        nb, _stream()))
    torch.cuda.synchronize()
    e64, q64 = enc.double().cpu(), q.double().cpu()
    a, c = alpha.cpu(), cv.double().cpu()
    for r in range(R):
        u, n = int(row_utt[r]), int(row_len[r])
        s = e64[u, :n] @ q64[r]
        w = torch.softmax(s, 0)
        assert (a[r, n:] == 0).all(), r
        np.testing.assert_allclose(a[r, :n].numpy(), w.numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(c[r].numpy(), (w @ e64[u, :n]).numpy(), rtol=0, atol=1e-5)


# ---------------------------------------------------------------- op level: selection and gather
def _run_select(L, lib, logits, score, status, tokens, N, K, step=0, nl=2, H=16, A=8):
    R, V = logits.shape
    U, S, T = R // N, step + 1, 6
    st = _state(U, N, S, T, nl, H, A)
    st["score"].copy_(torch.from_numpy(score))
    st["status"].copy_(torch.from_numpy(status))
    st["tokens"].copy_(torch.from_numpy(tokens))
    old = {k: st[k].clone() for k in ("c", "h", "ht")}
    new = dict(c=torch.randn(nl, R, H, device="cuda"), h=torch.randn(nl, R, H, device="cuda"), ht=torch.randn(R, A, device="cuda"))
    alpha = torch.randn(R, T, device="cuda")
    lg = torch.from_numpy(logits).cuda()
    bd, bs, _ = _descs(L, U, N, K, S, T, V, st)
    L.check(lib.astk_beam_select(C.byref(bd), nl, H, A, C.c_void_p(lg.data_ptr()), C.c_void_p(alpha.data_ptr()), T,
                                 C.c_void_p(new["c"].data_ptr()), C.c_void_p(new["h"].data_ptr()), C.c_void_p(new["ht"].data_ptr()),
                                 C.byref(bs), step, _stream()))
    torch.cuda.synchronize()
    return st, old, new, alpha


def _check_select(st, want, step, N):
    hist = st["hist"][step].cpu().numpy()
    sc, stt = st["score"].cpu().numpy(), st["status"].cpu().numpy()
    for r, (p, t, car, s, status) in enumerate(want):
        assert stt[r] == status, (r, stt[r], status)
        if status == 0:
            assert hist[r, 0] == -1
            continue
        assert (hist[r, 0], hist[r, 1], hist[r, 2]) == (p, t, car), (r, hist[r], (p, t, car))
        assert abs(sc[r] - s) <= 1e-12 * max(1.0, abs(s)), (r, sc[r], s)


@pytest.mark.parametrize("case", ["ties", "k_eq_v", "v8004"])
def test_select_matches_the_reference_rule(case):
    L, lib = _lib()
    rng = np.random.default_rng(3)
    if case == "ties":
        N, K, V = 4, 3, 9
        logits = rng.integers(-3, 3, size=(3 * N, V)).astype(np.float32)      # many exact ties inside rows
        logits[1] = logits[0]                                                  # ... and between slots of equal score
        score = np.array([-1.0, -1.0, -2.5, -4.0, 0.0, -3.0, -3.0, 0, -0.5, -0.7, -9, -9], dtype=np.float64)
        status = np.array([1, 1, 2, 1, 1, 2, 0, 0, 2, 2, 2, 0], dtype=np.int32)   # live, finished (carried) and empty slots; a frozen utterance
        tokens = np.array([5, 6, EOS, 4, 1, EOS, 0, 0, EOS, EOS, EOS, 0], dtype=np.int32)
    elif case == "k_eq_v":
        N, K, V = 5, 5, 5
        logits = rng.normal(size=(2 * N, V)).astype(np.float32)
        score = np.array([0, -1, -1, -2, -8, -0.3, 0, 0, 0, 0], dtype=np.float64)
        status = np.array([1, 2, 1, 1, 2, 1, 0, 0, 0, 0], dtype=np.int32)
        tokens = np.array([3, EOS, 4, 1, EOS, GO, GO, GO, GO, GO], dtype=np.int32)
    else:
        N, K, V = 5, 5, 8004
        logits = (rng.normal(size=(2 * N, V)) * 3).astype(np.float32)
        logits[0, 100:110] = logits[0].max() + 1.0                             # a tie across the top of a row
        score = np.array([-1, -1.5, -2, -2, -7, 0, 0, 0, 0, 0], dtype=np.float64)
        status = np.array([1, 1, 2, 1, 1, 1, 0, 0, 0, 0], dtype=np.int32)
        tokens = np.array([9, 8, EOS, 7, 6, GO, GO, GO, GO, GO], dtype=np.int32)
    st, old, new, alpha = _run_select(L, lib, logits, score, status, tokens, N, K, step=1)
    want = np_select(logits, score, status, tokens, N, K, EOS)
    _check_select(st, want, 1, N)
    # frozen flags: an utterance whose non-empty slots have all finished
    U = logits.shape[0] // N
    fro = [all(w[4] != 1 for w in want[u * N:(u + 1) * N]) for u in range(U)]
    assert st["frozen"].cpu().tolist() == [int(f) for f in fro] and int(st["n_frozen"][0]) == sum(fro)
    # the gather and the alpha history
    ha = st["hist_alpha"][1].cpu()
    for r, (p, t, car, s, status) in enumerate(want):
        u = r // N
        for k in ("c", "h", "ht"):
            got = st[k][..., r, :].cpu()
            if status == 0:
                ref = old[k][..., r, :].cpu()
            else:
                ref = (old if car else new)[k][..., u * N + p, :].cpu()
            assert torch.equal(got, ref), (case, k, r, p, car)
        if status != 0 and not car:
            assert torch.equal(ha[r], alpha[u * N + p].cpu())


def test_select_gather_keeps_a_carried_row_while_neighbours_move():
    """Slot 1 (finished, best score) moves to slot 0 and keeps its own old state; the live slot 0's expansions take its new state."""
    L, lib = _lib()
    N, K, V = 3, 2, 6
    logits = np.array([[0, 5, 4, 0, 0, 0], [0] * 6, [0] * 6], dtype=np.float32)
    score = np.array([-1.0, -0.5, 0.0])
    status = np.array([1, 2, 0], dtype=np.int32)
    tokens = np.array([4, EOS, 0], dtype=np.int32)
    st, old, new, _ = _run_select(L, lib, logits, score, status, tokens, N, K)
    hist = st["hist"][0].cpu().numpy()
    assert [tuple(hist[i, :3]) for i in range(3)] == [(1, EOS, 1), (0, 1, 0), (0, 2, 0)]
    for k in ("c", "h", "ht"):
        assert torch.equal(st[k][..., 0, :], old[k][..., 1, :])
        assert torch.equal(st[k][..., 1, :], new[k][..., 0, :]) and torch.equal(st[k][..., 2, :], new[k][..., 0, :])


# ---------------------------------------------------------------- whole search against the float64 oracle
def _cfg_opt(**rc):
    cfg = tiny_cfg(enc_layers=3, dec_layers=3, H=64, E=16, A=32, c0=8, c1=16, V=41)
    bn = rc.pop("bn", True)
    cfg["cnn_config"]["bn"] = bn
    cfg["rnn_config"].update(rc)
    return cfg


CONFIGS = {
    "tiny-3x3": lambda: tiny_cfg(enc_layers=3, dec_layers=3, H=64, E=16, A=64, c0=8, c1=16, V=57),
    "dec-1-layer": lambda: tiny_cfg(enc_layers=2, dec_layers=1, H=64, E=16, A=32, c0=8, c1=16, V=45),
    "all": lambda: _cfg_opt(ln=True, n_attn=2, feed_attn=False, bn=False),
}


def _gpu_model(cfg, P, D):
    from ast_amd.seq2seq import SpeechEncoderDecoder
    return SpeechEncoderDecoder(0, copy.deepcopy(cfg)).materialize(D, values=P)


@pytest.mark.parametrize("N,K", [(3, 4), (4, 2), (1, 3)])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_batched_search_matches_oracle_per_utterance(name, N, K):
    from oracle import ast_ref as R
    from ast_amd import nn as gnn
    cfg = CONFIGS[name]()
    V, D, stop = cfg["rnn_config"]["dec_vocab_size"], 80, 7
    P = R.init_params(cfg, D, V, seed=21, dtype=np.float32)
    P["out/b"] = P["out/b"].copy()
    P["out/b"][EOS] += 2.0                      # some hypotheses finish before stop_limit: the carry path runs
    Xs = [R.synth_batch(1, T, D, 4, V, seed=30 + i, dtype=np.float32)[0] for i, T in enumerate((90, 71, 120))]
    ref = R.RefModel(cfg, {k: v.astype(np.float64) for k, v in P.items()}, V)
    g = _gpu_model(cfg, P, D)
    got = gnn.decode_beam_batch(g, [torch.from_numpy(X) for X in Xs], stop, N, K)
    finished_early = False
    for X, lst in zip(Xs, got):
        want = R.decode_beam(ref, X.astype(np.float64), stop_limit=stop, N=N, K=K)
        assert [e["hyp"] for e in lst] == [e["hyp"] for e in want], (name, [e["hyp"] for e in lst], [e["hyp"] for e in want])
        for a, b in zip(lst, want):
            assert isinstance(a["score"], float) and all(isinstance(t, int) for t in a["hyp"])
            assert abs(a["score"] - b["score"]) <= 1e-4 * max(1.0, abs(b["score"])), (a["score"], b["score"])
            assert len(a["attn_history"]) == len(b["attn_history"]) == len(a["hyp"]) - 1
            assert a["attn_history"][-1].shape == np.squeeze(b["attn_history"][-1]).shape
            np.testing.assert_allclose(a["attn_history"][-1], np.squeeze(b["attn_history"][-1]), rtol=0, atol=1e-5)
            finished_early |= a["hyp"][-1] == EOS and len(a["hyp"]) <= stop
    assert finished_early, "no hypothesis finished before stop_limit: the carry path was not exercised"


# ---------------------------------------------------------------- against the per-utterance GPU path at a realistic size
def _mid():
    from oracle import ast_ref as R
    cfg = tiny_cfg(enc_layers=2, dec_layers=2, H=512, E=64, A=256, c0=8, c1=16, V=1001)
    D, V = 80, 1001
    P = R.init_params(cfg, D, V, seed=5, dtype=np.float32)
    P["out/W"] = (P["out/W"] * 3).astype(np.float32)
    rng = np.random.default_rng(11)
    Xs = [torch.from_numpy(R.synth_batch(1, int(T), D, 4, V, seed=50 + i, dtype=np.float32)[0]) for i, T in enumerate(rng.integers(60, 240, 16))]
    return cfg, P, D, Xs


def test_batched_search_matches_per_utterance_gpu_path_mid_size():
    from ast_amd import nn as gnn
    cfg, P, D, Xs = _mid()
    g = _gpu_model(cfg, P, D)
    got = gnn.decode_beam_batch(g, Xs, 30, 5, 5)
    for X, lst in zip(Xs, got):
        want = gnn.decode_beam(g, X, 30, 5, 5)
        ws = [e["score"] for e in want]
        tight = any(abs(ws[i] - ws[j]) <= 1e-5 for i in range(len(ws)) for j in range(i))
        if not tight:
            assert [e["hyp"] for e in lst] == [e["hyp"] for e in want]
        if lst[0]["hyp"] == want[0]["hyp"]:
            assert abs(lst[0]["score"] - want[0]["score"]) <= 1e-5 * max(1.0, abs(want[0]["score"]))
            np.testing.assert_allclose(lst[0]["attn_v"].cpu().numpy(), want[0]["attn_v"].cpu().numpy(), rtol=0, atol=1e-5)


def test_batch_composition_does_not_matter():
    from ast_amd import nn as gnn
    cfg, P, D, Xs = _mid()
    g = _gpu_model(cfg, P, D)
    alone = gnn.decode_beam_batch(g, [Xs[3]], 30, 5, 5)[0]
    inside = gnn.decode_beam_batch(g, Xs[:8], 30, 5, 5)[3]
    assert [e["hyp"] for e in alone] == [e["hyp"] for e in inside]
    for a, b in zip(alone, inside):
        assert abs(a["score"] - b["score"]) <= 1e-6 * max(1.0, abs(b["score"]))


# ---------------------------------------------------------------- beam.py -b
def test_beam_py_batch_flag_writes_the_same_hypotheses(tmp_path):
    mcfg = tiny_cfg(enc_layers=2, dec_layers=1, H=32, E=16, A=32, c0=8, c1=16, V=31, drop=0.0)
    del mcfg["rnn_config"]["dec_vocab_size"]
    tcfg = {"seed": "seed-ast-20h", "gpuid": 0, "batch_size": 8, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 1,
            "optimizer": {"type": 0, "lr": 2e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0},
            "data": {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 16, "syn_dev": 7},
                     "frames": [60, 300], "targets": [2, 9], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w"}}
    json.dump(mcfg, open(tmp_path / "model_cfg.json", "w"))
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-m", str(tmp_path), "-e", "2"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    from ast_amd.nn import NN
    nn = NN(str(tmp_path))
    refs = tmp_path / "refs" / "syn_dev"
    os.makedirs(refs)
    utts = sorted(nn.data_loader.info["syn_dev"])
    truth = nn.data_loader.get_hyps([(u, list(nn.data_loader.ids["syn_dev"][u])) for u in utts])
    (refs / "eval.ids").write_text("".join(u + "\n" for u in utts))
    (refs / "ref.en0").write_text("".join(" ".join(truth[u]) + "\n" for u in utts))
    tcfg["data"].update(refs_path=str(tmp_path / "refs"), n_evals=1)
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))
    del nn
    torch.cuda.empty_cache()
    out = {}
    for extra in ([], ["-b", "4"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "beam.py"), "-m", str(tmp_path), "-n", "3", "-k", "4", "-s", "syn_dev", "-w", "0.6"]
                           + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "BLEU = " in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        with open(tmp_path / "syn_dev_beam_N-3_K-4.p", "rb") as f:
            beam = pickle.load(f)
        out[len(extra)] = ({u: [h for h, _, _ in v] for u, v in beam.items()}, open(tmp_path / "syn_dev_beam_N-3_K-4_W-0.60.en").read(),
                           {u: [s for _, s, _ in v] for u, v in beam.items()})
    assert len(out[0][0]) == 7 and out[0][0] == out[2][0]
    assert out[0][1] == out[2][1]
    for u in out[0][2]:
        np.testing.assert_allclose(out[2][2][u], out[0][2][u], rtol=1e-5)


# ---------------------------------------------------------------- argument checks of the C ABI
def test_bad_arguments_fail_with_a_message():
    L, lib = _lib()
    U, N, K, V, T, S, nl, H, A = 2, 3, 2, 7, 5, 2, 1, 16, 8
    st = _state(U, N, S, T, nl, H, A)
    R = U * N
    lg, al = torch.zeros(R, V, device="cuda"), torch.zeros(R, T, device="cuda")
    cn, ht = torch.zeros(nl, R, H, device="cuda"), torch.zeros(R, A, device="cuda")

    def sel(bd, bs):
        return lib.astk_beam_select(C.byref(bd), nl, H, A, C.c_void_p(lg.data_ptr()), C.c_void_p(al.data_ptr()), T, C.c_void_p(cn.data_ptr()),
                                    C.c_void_p(cn.data_ptr()), C.c_void_p(ht.data_ptr()), C.byref(bs), 0, _stream())
    bd, bs, keep = _descs(L, U, N, V + 1, S, T, V, st)
    assert sel(bd, bs) != 0 and b"larger than the vocabulary" in lib.astk_last_error()
    bd, bs, keep = _descs(L, U, L.BEAM_MAX_N + 1, K, S, T, V, st)
    assert sel(bd, bs) != 0 and b"N = 17" in lib.astk_last_error()
    bd, bs, keep = _descs(L, U, N, L.BEAM_MAX_K + 1, S, T, 40, st)
    assert sel(bd, bs) != 0 and b"K = 17" in lib.astk_last_error()
    bd, bs, keep = _descs(L, U, N, K, S, T, V, st, lens=[T, T + 1])
    assert sel(bd, bs) != 0 and b"outside 1..5" in lib.astk_last_error()
    # a short workspace for a whole step
    bd, bs, keep = _descs(L, U, N, K, S, T, V, st)
    dd = L.DecoderDesc(R, 2, T, H, 4, A, V, nl, 0, 0, 0)
    need = int(lib.astk_beam_workspace_bytes(C.byref(bd), C.byref(dd)))
    assert need > 0
    ws = torch.zeros(256, dtype=torch.uint8, device="cuda")
    rc = lib.astk_beam_step(C.byref(bd), C.byref(dd), C.byref(L.DecoderParams()), C.c_void_p(lg.data_ptr()), C.byref(bs), 0,
                            C.c_void_p(ws.data_ptr()), 256, _stream())
    assert rc != 0 and b"workspace too small" in lib.astk_last_error()
    # ... and the Python entry point refuses N / K above the kernel's limit before it touches the device
    from ast_amd import nn as gnn
    with pytest.raises(ValueError):
        gnn.decode_beam_batch(None, [], 5, L.BEAM_MAX_N + 1, 2)
    torch.cuda.synchronize()
