"""Beam search on the device loop (ast_amd.nn.decode_beam_device, include/astk.h astk_beam_decode): whole searches against the float64
oracle's decode_beam behind a near-tie guard, forced rescoring of every returned hypothesis at full size, N = 1 against the greedy
modes, exact ties, pack composition, the per-step batched search, the fallbacks and refusals, and beam.py --device end to end."""
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
from decode_helpers import CFG1, EOS, ES_EN, GO, MID, WIDE, setup, tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {
    "one": dict(enc_layers=2, dec_layers=1, H=64, E=16, A=32, c0=8, c1=16, V=45),
    "mid": MID,
    "three": dict(enc_layers=3, dec_layers=3, H=64, E=16, A=64, c0=8, c1=16, V=57),
}
FRAMES = (90, 71, 120, 64, 150, 101)
STOP, GAP = 12, 1e-4        # (1e-4: the guard value of test_gpu_sample.py)


def _utts(V, frames=FRAMES, D=80):
    from oracle import ast_ref as R
    return [R.synth_batch(1, T, D, 4, V, seed=30 + i, dtype=np.float32)[0] for i, T in enumerate(frames)]


def _tensors(Xs):
    return [torch.from_numpy(X) for X in Xs]


# ---------------------------------------------------------------- the oracle's search restated, with the smallest gap of any decision
def oracle_search_with_gaps(ref, X, stop_limit, N, K):
    """oracle.ast_ref.decode_beam, recording the smallest gap of any decision a float32 search could take the other way: consecutive
    sorted log-probabilities among ranks 1..K+1 of a live row, and consecutive scores among the first N+1 candidates of a step.  Also
    says whether a finished hypothesis was carried while another was live.  Returns (n_best, smallest gap, carried)."""
    from oracle import ast_ref as R
    was, ref.train = ref.train, False
    gap, carried = np.inf, False
    try:
        ref.encode(X)
        A = ref.cfg["rnn_config"]["attn_units"]
        n_best = [{"hyp": [R.GO_ID], "score": 0, "dec_state": ref.get_encoder_states(),
                   "attn_v": R.Variable(np.zeros((1, A), dtype=ref.dtype)), "attn_history": []}]
        for _ in range(stop_limit):
            done = [e["hyp"][-1] == R.EOS_ID for e in n_best]
            if all(done):
                break
            carried |= any(done)
            cur = []
            for e in n_best:
                if e["hyp"][-1] == R.EOS_ID:
                    cur.append(e)
                    continue
                ref.set_decoder_states(e["dec_state"])
                logits, ht, alphas = ref.decode_step(np.full((1,), e["hyp"][-1], dtype=np.int32), e["attn_v"])
                x = np.asarray(logits.data[0], dtype=np.float64)
                logp = x - (np.log(np.exp(x - x.max()).sum()) + x.max())
                top = np.argsort(logp)[-K:]
                ranked = np.sort(logp)[::-1][:K + 1]
                if len(ranked) > 1:
                    gap = min(gap, float(np.min(ranked[:-1] - ranked[1:])))
                state = ref.get_decoder_states()
                for pi in top[::-1]:
                    cur.append({"hyp": e["hyp"] + [int(pi)], "score": e["score"] + float(logp[pi]), "dec_state": state, "attn_v": ht,
                                "attn_history": e["attn_history"] + [np.squeeze(alphas.data)]})
            order = sorted(cur, reverse=True, key=lambda t: t["score"])
            sc = np.array([t["score"] for t in order[:N + 1]], dtype=np.float64)
            if len(sc) > 1:
                gap = min(gap, float(np.min(sc[:-1] - sc[1:])))
            n_best = order[:N]
        return n_best, gap, carried
    finally:
        ref.train = was


_ORACLE = {}


def _oracle_case(shape_name, N, K):
    """The six utterances' oracle lists, gaps and carry flags of a case, computed once."""
    key = (shape_name, N, K)
    if key not in _ORACLE:
        from oracle import ast_ref as R
        cfg, P, _, _ = _SETUP(shape_name)
        V = SHAPES[shape_name]["V"]
        ref = R.RefModel(cfg, {k: v.astype(np.float64) for k, v in P.items()}, V)
        rows = []
        for X in _utts(V):
            want, gap, carried = oracle_search_with_gaps(ref, X.astype(np.float64), STOP, N, K)
            plain = R.decode_beam(ref, X.astype(np.float64), stop_limit=STOP, N=N, K=K)
            assert [e["hyp"] for e in want] == [e["hyp"] for e in plain] and [e["score"] for e in want] == [e["score"] for e in plain]
            rows.append((want, gap, carried))
        _ORACLE[key] = rows
    return _ORACLE[key]


_MODELS = {}


def _SETUP(shape_name):
    """(cfg, P, X, model) of a small shape: init_params(seed = 21), out/W x 8, out/b[EOS] += 2."""
    if shape_name not in _MODELS:
        _MODELS[shape_name] = setup(SHAPES[shape_name], 1, 90, seed=21, eos_bias=2.0)
    return _MODELS[shape_name]


# ---------------------------------------------------------------- 1. against the float64 oracle
@pytest.mark.parametrize("N,K", [(5, 5), (3, 4), (1, 3), (16, 2)])
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_device_search_matches_oracle(shape_name, N, K):
    from ast_amd import nn as gnn
    cfg, P, _, m = _SETUP(shape_name)
    Xs = _utts(SHAPES[shape_name]["V"])
    ref_rows = _oracle_case(shape_name, N, K)
    got = gnn.decode_beam_device(m, _tensors(Xs), STOP, N, K)
    assert m.last_beam_path == "device"
    left_out = [i for i, (_, gap, _) in enumerate(ref_rows) if gap < GAP]
    print(f"\n{shape_name} N {N} K {K}: gaps {[f'{g:.2e}' for _, g, _ in ref_rows]}, left out {left_out}, n_steps {m.last_beam_steps}")
    assert len(left_out) <= 2, left_out
    finished_early, carried = False, False
    for i, (lst, (want, gap, car)) in enumerate(zip(got, ref_rows)):
        if i in left_out:
            continue
        carried |= car
        assert [e["hyp"] for e in lst] == [e["hyp"] for e in want], (shape_name, i, [e["hyp"] for e in lst], [e["hyp"] for e in want])
        for a, b in zip(lst, want):
            assert isinstance(a["score"], float) and all(isinstance(t, int) for t in a["hyp"])
            print(f"  utt {i}: score {a['score']:.6f} oracle {b['score']:.6f}")
            assert abs(a["score"] - b["score"]) <= 1e-4 * max(1.0, abs(b["score"])), (a["score"], b["score"])
            assert len(a["attn_history"]) == len(b["attn_history"]) == len(a["hyp"]) - 1
            for x, y in zip(a["attn_history"], b["attn_history"]):
                assert x.shape == np.squeeze(y).shape
                np.testing.assert_allclose(x, np.squeeze(y), rtol=0, atol=1e-5)
            finished_early |= a["hyp"][-1] == EOS and len(a["hyp"]) <= STOP
    # what the inputs cover (the oracle, on the CPU): with N > 1 every case carries a finished hypothesis while another is live; "three"
    # freezes every utterance before the stop limit unless N = 16 (its longest hypothesis then has 12 tokens)
    if N > 1:
        assert carried and finished_early, "no finished hypothesis was carried while another was live: the carry path was not exercised"
    if shape_name == "three" and N < 16:
        assert all(n < STOP for n in m.last_beam_steps), m.last_beam_steps


# ---------------------------------------------------------------- 2. forced rescoring at full size, no guard
@pytest.mark.parametrize("shape_name", ["es_en", "cfg1"])
def test_every_hypothesis_rescored_by_forced_decoding_full_size(shape_name):
    """A wrong gather of c, h or ht at any layer changes the state a hypothesis continues from: its score then differs from the
    forced score of its own tokens."""
    from ast_amd import nn as gnn
    shape = dict(es_en=ES_EN, cfg1=CFG1)[shape_name]
    _, _, _, m = setup(shape, 1, 200, seed=21, eos_bias=2.0)
    Xs = _tensors(_utts(shape["V"], frames=(200, 480, 333, 256, 410, 290)))
    got = gnn.decode_beam_device(m, Xs, STOP, 5, 5)
    assert m.last_beam_path == "device"
    worst = 0.0
    for X, lst in zip(Xs, got):
        assert len(lst) == 5
        scores, r = gnn.score_hypotheses(m, X, [e["hyp"] for e in lst])
        for i, (e, s) in enumerate(zip(lst, scores)):
            bound = float(np.sum(tol(r.logp[i, :len(e["hyp"]) - 1].astype(np.float64))))
            worst = max(worst, abs(e["score"] - s) / bound)
            assert abs(e["score"] - s) <= bound, (shape_name, i, e["hyp"], e["score"], s, bound)
    print(f"\n{shape_name}: largest |beam score - forced score| / bound {worst:.3f}, n_steps {m.last_beam_steps}")


# ---------------------------------------------------------------- 3. N = 1 is the greedy decode
@pytest.mark.parametrize("shape_name", ["mid", "three"])
def test_one_hypothesis_is_the_greedy_decode(shape_name):
    from ast_amd import nn as gnn
    _, _, _, m = _SETUP(shape_name)       # (equal encoder and decoder depths: encode_rows seeds the rows as the search seeds slot 0)
    Xs = _tensors(_utts(SHAPES[shape_name]["V"]))
    got = gnn.decode_beam_device(m, Xs, STOP, 1, 3)
    assert m.last_beam_path == "device"
    rows = m.encode_rows(Xs)
    tokens = m.predict(None, GO, EOS, STOP, rows=rows)
    scored = m.predict_scored(None, GO, EOS, STOP, rows=rows)
    assert m.last_predict_path == "device"
    for b, lst in enumerate(got):
        toks = [int(t) for t in tokens[b]]
        n = toks.index(EOS) + 1 if EOS in toks else len(toks)
        assert len(lst) == 1 and lst[0]["hyp"] == [GO] + toks[:n], (b, lst[0]["hyp"], toks)
        want = float(scored.logp[b, :n].astype(np.float64).sum())
        assert abs(lst[0]["score"] - want) <= float(np.sum(tol(scored.logp[b, :n].astype(np.float64)))), (b, lst[0]["score"], want)


# ---------------------------------------------------------------- 4. exact ties
def test_exact_ties_rank_the_lower_id_first_and_both_survive():
    from ast_amd import nn as gnn
    from oracle import ast_ref as R
    shape = SHAPES["mid"]
    cfg = tiny_cfg(**shape)
    P = R.init_params(cfg, 80, shape["V"], seed=21, dtype=np.float32)
    P["out/W"] = (P["out/W"] * 8).astype(np.float32)
    P["out/b"] = P["out/b"].copy()
    lo, hi = 11, 40
    P["out/W"][hi] = P["out/W"][lo]
    P["out/b"][lo] = P["out/b"][hi] = P["out/b"].max() + 30.0          # the two classes lead every row, exactly tied
    c = copy.deepcopy(cfg)
    c["rnn_config"]["dec_vocab_size"] = shape["V"]
    from ast_amd.seq2seq import SpeechEncoderDecoder
    m = SpeechEncoderDecoder(0, c).materialize(80, values=P)
    Xs = _tensors(_utts(shape["V"])[:3])
    one = gnn.decode_beam_device(m, Xs, 1, 3, 4)
    assert m.last_beam_path == "device"
    for lst in one:
        assert [e["hyp"] for e in lst[:2]] == [[GO, lo], [GO, hi]] and lst[0]["score"] == lst[1]["score"]
    want = gnn.decode_beam_batch(m, Xs, 1, 3, 4)
    for a, b in zip(one, want):
        assert [e["hyp"] for e in a] == [e["hyp"] for e in b]
    # a second step: the two expansions of one parent by the tied classes are neighbours, lower id first, with equal scores (which parent's
    # pair leads is a near-tie of ~1e-12 that float32 and float64 may order differently: not compared)
    two = gnn.decode_beam_device(m, Xs, 2, 4, 2)
    for lst in two:
        assert sorted(e["hyp"] for e in lst) == [[GO, a, b] for a in (lo, hi) for b in (lo, hi)]
        for a, b in zip(lst[0::2], lst[1::2]):
            assert a["hyp"][:2] == b["hyp"][:2] and (a["hyp"][2], b["hyp"][2]) == (lo, hi) and a["score"] == b["score"]


# ---------------------------------------------------------------- 5. composition
def test_pack_composition_does_not_matter():
    """Alone and inside a full pack of 6: the same hypotheses, the same score bits, the same alpha bits -- for every utterance, the
    longest and the shorter ones (whose launch has another row count and another T either way)."""
    from ast_amd import nn as gnn
    _, _, _, m = _SETUP("three")
    Xs = _tensors(_utts(SHAPES["three"]["V"]))
    pack = gnn.decode_beam_device(m, Xs, STOP, 5, 5)
    assert m.last_beam_path == "device"
    for u in range(len(Xs)):
        alone = gnn.decode_beam_device(m, [Xs[u]], STOP, 5, 5)[0]
        assert m.last_beam_path == "device"
        assert [e["hyp"] for e in alone] == [e["hyp"] for e in pack[u]]
        for a, b in zip(alone, pack[u]):
            assert a["score"] == b["score"], (u, a["score"], b["score"])
            for x, y in zip(a["attn_history"], b["attn_history"]):
                assert (x.view(np.uint32) == y.view(np.uint32)).all(), u
    # ... and a pack of two tiles' worth against a pack of other neighbours
    other = gnn.decode_beam_device(m, [Xs[2], Xs[0], Xs[5]], STOP, 5, 5)
    for got, u in zip(other, (2, 0, 5)):
        assert [e["hyp"] for e in got] == [e["hyp"] for e in pack[u]] and [e["score"] for e in got] == [e["score"] for e in pack[u]]


# ---------------------------------------------------------------- 6. against the per-step batched search
def test_device_search_matches_the_per_step_batched_search_mid_size():
    from ast_amd import nn as gnn
    from test_gpu_beam import _gpu_model, _mid
    cfg, P, D, Xs = _mid()
    Xs = Xs[:12]
    g = _gpu_model(cfg, P, D)
    got = gnn.decode_beam_device(g, Xs, 30, 5, 5)
    assert g.last_beam_path == "device"
    ref = gnn.decode_beam_batch(g, Xs, 30, 5, 5)
    for lst, want in zip(got, ref):
        ws = [e["score"] for e in want]
        tight = any(abs(ws[i] - ws[j]) <= 1e-5 for i in range(len(ws)) for j in range(i))
        if not tight:
            assert [e["hyp"] for e in lst] == [e["hyp"] for e in want]
        if lst[0]["hyp"] == want[0]["hyp"]:
            assert abs(lst[0]["score"] - want[0]["score"]) <= 1e-5 * max(1.0, abs(want[0]["score"]))
            np.testing.assert_allclose(lst[0]["attn_v"].cpu().numpy(), want[0]["attn_v"].cpu().numpy(), rtol=0, atol=1e-5)
            for k in ("c", "h"):
                for a, b in zip(lst[0]["dec_state"][k], want[0]["dec_state"][k]):
                    assert a.shape == b.shape and a.device == b.device
                    np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=0, atol=1e-4)
        assert list(lst[0]) == list(want[0])


# ---------------------------------------------------------------- 7. fallbacks and refusals
@pytest.mark.parametrize("case", ["n_attn", "wide"])
def test_shapes_off_the_device_loop_take_the_per_step_search(case):
    from ast_amd import nn as gnn
    if case == "n_attn":
        _, _, _, m = setup(SHAPES["mid"], 1, 90, seed=21, eos_bias=2.0, n_attn=2)
    else:
        _, _, _, m = setup(WIDE, 1, 90, seed=21, eos_bias=2.0)
    V = (SHAPES["mid"] if case == "n_attn" else WIDE)["V"]
    Xs = _tensors(_utts(V)[:2])
    got = gnn.decode_beam_device(m, Xs, 5, 3, 3)
    assert m.last_beam_path == "steps"
    want = gnn.decode_beam_batch(m, Xs, 5, 3, 3)
    for a, b in zip(got, want):
        assert [e["hyp"] for e in a] == [e["hyp"] for e in b] and [e["score"] for e in a] == [e["score"] for e in b]


def test_refusals_have_a_message():
    from ast_amd import _lib as L
    from ast_amd import nn as gnn
    with pytest.raises(ValueError, match="N = 17"):
        gnn.decode_beam_device(None, [], 5, 17, 2)
    lib = L.load()
    _, _, _, m = _SETUP("mid")
    m.predict(torch.from_numpy(_utts(SHAPES["mid"]["V"])[0]), GO, EOS, 3)          # (a decoder descriptor of the model)
    dd = L.DecoderDesc.from_buffer_copy(m._cur["dd"])
    q = lambda B, N, K, stop=12: (setattr(dd, "B", B), int(lib.astk_beam_decode_workspace_bytes(C.byref(dd), N, K, stop, 1)))[1]
    assert q(31, 5, 5) > 0 and q(10, 5, 5) > 0 and q(32, 16, 2) > 0
    assert q(31, 17, 5) == 0 and q(31, 5, 17) == 0 and q(31, 0, 5) == 0 and q(31, 5, 0) == 0      # N, K outside 1..16
    assert q(16, 5, 5) == 0 and q(12, 5, 5) == 0          # row 15 is padding at N = 5; 12 rows end inside an utterance
    assert q(33, 1, 1) == 0 and q(31, 5, 5, stop=0) == 0
    dd.B = 16
    z = C.c_void_p(0)
    rc = lib.astk_beam_decode(C.byref(dd), C.byref(m._cur["dp"]), z, z, z, z, 5, 5, GO, EOS, 12, z, z, z, z, z, z, z, z, z, z, 0, z)
    assert rc != 0 and b"do not end with the last" in lib.astk_last_error()


# ---------------------------------------------------------------- 8. beam.py --device
def test_beam_py_device_flag_writes_the_same_files(tmp_path):
    """The experiment of test_beam_py_batch_flag_writes_the_same_hypotheses with H = 64 in place of 32: the device loop runs hidden sizes
    that are multiples of 64 (beam.py prints which path searched)."""
    mcfg = tiny_cfg(enc_layers=2, dec_layers=1, H=64, E=16, A=32, c0=8, c1=16, V=31, drop=0.0)
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
    for name, extra in (("batch", ["-b", "4"]), ("device", ["--device", "-b", "4"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "beam.py"), "-m", str(tmp_path), "-n", "3", "-k", "4", "-s", "syn_dev", "-w", "0.6"]
                           + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "BLEU = " in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("search path: device" in r.stdout) == (name == "device"), r.stdout[-2000:]
        with open(tmp_path / "syn_dev_beam_N-3_K-4.p", "rb") as f:
            beam = pickle.load(f)
        out[name] = ({u: [h for h, _, _ in v] for u, v in beam.items()}, open(tmp_path / "syn_dev_beam_N-3_K-4_W-0.60.en").read(),
                     {u: [s for _, s, _ in v] for u, v in beam.items()}, {u: [a for _, _, a in v] for u, v in beam.items()})
    assert len(out["batch"][0]) == 7 and out["batch"][0] == out["device"][0]
    assert out["batch"][1] == out["device"][1]
    for u in out["batch"][2]:
        np.testing.assert_allclose(out["device"][2][u], out["batch"][2][u], rtol=1e-5)
        # the attention rows in the pickle: one per token of every hypothesis, the values of the per-step search (float32 either way)
        for ha, hb in zip(out["device"][3][u], out["batch"][3][u]):
            assert len(ha) == len(hb)
            for x, y in zip(ha, hb):
                assert x.shape == y.shape and x.dtype == y.dtype
                np.testing.assert_allclose(x, y, rtol=0, atol=1e-5)
