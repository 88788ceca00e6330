"""GPU tests of minimum-risk training (ast_amd/mrt.py, NN's extras.mrt): one mrt_step against the same step
composed by hand from the public pieces, its status and reporting, NN.train_epoch with extras.mrt (sample streams, start_epoch), and
train.py in a child process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import risk_model as RM
import schedule_helpers as SH
from conftest import tiny_cfg

pytestmark = pytest.mark.gpu
GO, EOS = 1, 2


def _mid():
    """The `mid` shape of the persistent route at U 2, N 3: 8 rows."""
    cfg = tiny_cfg(enc_layers=3, dec_layers=2, H=64, E=16, A=64, c0=16, c1=32, V=57, drop=0.0)
    P, X, y = SH.make_inputs(cfg, 2, 120, 80, 9, 57)
    return cfg, P, X, y


def _fresh(cfg, P):
    g = SH.gpu_model(cfg, P, 80, 57)
    g.deterministic = True
    return g


def _bits(loss):
    return loss.pair[:1].clone().view(torch.int32).item()


@pytest.mark.parametrize("cost", ["bleu", "edit"])
def test_mrt_step_is_the_step_composed_by_hand(cost):
    from ast_amd import _lib, mrt
    from ast_amd.eval import pair_stats_host
    from ast_amd.seq2seq import using_config
    lib = _lib.load()
    cfg, P, X, y = _mid()
    mc = mrt.checked_mrt({"samples": 3, "alpha": 0.5, "cost": cost, "mle_weight": 0.25, "seed": 11, "temperature": 1.5})
    U, N, first_stream = 2, 3, 100
    g = _fresh(cfg, P)
    st = mrt.mrt_step(g, torch.from_numpy(X), y, mc, first_stream)
    torch.cuda.synchronize()
    path = lib.astk_decoder_path(C.byref(g._cur["dd"]))
    assert path & 1 and not path & 4, f"astk_decoder_path = {path}, meant to run on the persistent route"
    assert SH.status_word() == 0
    assert st.streams == list(range(100, 106)) and st.next_stream == 106
    arena, bits = g.arena._grad.clone(), _bits(st.loss)
    risk, w_dev = st.risk.cpu().numpy(), st.weight.cpu().numpy()
    # ---- by hand, on a fresh model
    h = _fresh(cfg, P)
    max_len = 9 - 1 + 10
    r = h.sample(torch.from_numpy(X).repeat_interleave(N, dim=0), GO, EOS, max_len, 11, streams=range(100, 106), temperature=1.5)
    samples = [list(r.tokens[u * N:(u + 1) * N]) for u in range(U)]
    b = mrt.build_mrt_batch(samples, y)
    R = U * (N + 1)
    assert b["y"].shape[0] == R and b["flags"].tolist().count(mrt.REFERENCE) == U
    np.testing.assert_array_equal(b["y"], st.batch["y"])
    score = np.zeros(R, np.float32)
    score[b["flags"] != mrt.REFERENCE] = r.score.astype(np.float32)
    np.testing.assert_array_equal(score, st.scores)
    stats = pair_stats_host(b["pool"], [tuple(p) for p in b["pairs"]])
    rs, rw = mrt.mrt_scales(0.25, R, U)
    lens = [len(s) for s in b["pool"]]
    hw, hr, hc, n_bad = mrt.risk_weights_host(b["first"], score, stats, lens, b["pairs"], b["flags"], cost, 0.5, rs, rw)
    case = dict(alpha=0.5, risk_scale=rs, ref_weight=rw)
    bw, br, _ = RM.bounds(case, (hw, hr, hc))
    print(cost, "weights", w_dev, hw, "risk", risk, hr, "bit-equal", bool((w_dev == hw).all()))
    assert n_bad == 0 and (np.abs(w_dev.astype(np.float64) - hw) <= bw).all() and (np.abs(risk.astype(np.float64) - hr) <= br).all()
    assert np.isfinite(risk).all() and (risk >= 0).all() and (cost == "edit" or (risk <= 1).all())
    assert (hw[b["flags"] == mrt.REFERENCE] == np.float32(rw)).all(), "the reference rows carry ref_weight alone"
    assert (hw[b["flags"] == mrt.LIVE] != 0).any(), "the candidates differ in cost: the risk term is there"
    w = hw if (w_dev == hw).all() else w_dev      # (the comparison below tests the orchestration, not the ulp)
    with using_config("train", True):
        loss = h.forward_loss(X=torch.from_numpy(X).repeat_interleave(N + 1, dim=0), y=b["y"], teach_ratio=1.0, random_out=0,
                              label_smoothing=0.0, row_weight=w)
        h.cleargrads()
        loss.backward()
    torch.cuda.synchronize()
    assert SH.status_word() == 0
    assert _bits(loss) == bits, (float(loss.data), float(st.loss.data))
    assert torch.equal(h.arena._grad, arena)
    assert float(arena.abs().max()) > 0 and np.isfinite(float(st.loss.data))


def _exp_dir(d, mrt):
    mcfg = tiny_cfg(enc_layers=2, dec_layers=1, H=32, E=16, A=32, c0=8, c1=16, V=31, drop=0.0)
    del mcfg["rnn_config"]["dec_vocab_size"]
    ex = {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0, "deterministic": True}
    if mrt is not None:
        ex["mrt"] = mrt
    tcfg = {"seed": "seed-ast-20h", "gpuid": 0, "batch_size": 4, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 2,
            "optimizer": {"type": 0, "lr": 2e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": ex,
            "data": {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 8, "syn_dev": 4},
                     "frames": [60, 300], "targets": [2, 9], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w"}}
    os.makedirs(d)
    json.dump(mcfg, open(os.path.join(d, "model_cfg.json"), "w"))
    json.dump(tcfg, open(os.path.join(d, "train_cfg.json"), "w"))
    return str(d)


MRT = {"samples": 3, "alpha": 1.0, "cost": "bleu", "mle_weight": 0.5, "seed": 5}


def test_train_epoch_runs_mrt_steps_on_fresh_streams(tmp_path, monkeypatch):
    from ast_amd import mrt
    from ast_amd.nn import NN
    calls = []
    orig = mrt.mrt_step

    def spy(*a, **k):
        st = orig(*a, **k)
        calls.append(st)
        return st
    monkeypatch.setattr(mrt, "mrt_step", spy)
    nn = NN(_exp_dir(tmp_path / "mrt", MRT))
    assert nn.mrt["samples"] == 3 and nn.mrt_epoch is None
    losses = [nn.train_epoch("syn_train") for _ in range(2)]
    assert len(calls) >= 3, "at least three MRT steps"
    assert all(np.isfinite(losses)) and nn.mrt_epoch is not None and 0.0 <= nn.mrt_epoch <= 1.0
    used = [s for st in calls for s in st.streams]
    assert len(set(used)) == len(used), "no sample stream is drawn from twice"
    assert calls[1].streams[0] == calls[0].next_stream and nn.mrt_stream == calls[-1].next_stream
    assert SH.status_word() == 0
    risks = [float(st.risk.mean()) for st in calls[-(len(calls) // 2):]]
    assert abs(nn.mrt_epoch - np.mean(risks)) < 1e-6      # the last epoch's mean over its steps


def test_start_epoch_leaves_the_epochs_before_it_alone(tmp_path):
    from ast_amd.nn import NN
    plain = NN(_exp_dir(tmp_path / "plain", None))
    first_plain = plain.train_epoch("syn_train")
    assert plain.mrt is None and plain.mrt_epoch is None
    del plain
    late = NN(_exp_dir(tmp_path / "late", dict(MRT, start_epoch=1)))
    first_late = late.train_epoch("syn_train")
    assert late.mrt_epoch is None and first_late == first_plain, (first_late, first_plain)
    second = late.train_epoch("syn_train")
    assert late.mrt_epoch is not None and np.isfinite(second)


def test_train_py_reads_extras_mrt(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(d):
        return subprocess.run([sys.executable, os.path.join(root, "train.py"), "-m", d, "-e", "1"], cwd=root, capture_output=True, text=True,
                              timeout=600)
    r = run(_exp_dir(tmp_path / "ok", MRT))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "MRT expected cost" in r.stdout
    r = run(_exp_dir(tmp_path / "bad", dict(MRT, samples=64)))
    assert r.returncode != 0 and "ValueError" in r.stderr and "extras.mrt.samples" in r.stderr
