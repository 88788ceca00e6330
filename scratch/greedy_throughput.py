"""Greedy decoding throughput (predict, seq2seq.py:475-527): the device loop (astk_greedy_decode, one persistent launch per batch) against
the per-step loop (dec.persist = 0), in the same process, alternating, after a warm-up, each timed to a device synchronise.

    python scratch/greedy_throughput.py                                   # both shapes, both cases
    python scratch/greedy_throughput.py --scored                          # the device loop unscored / scored without targets / scored
                                                                          # with targets (predict_scored)
    python scratch/greedy_throughput.py --only device --shape es_en_20h --case no_eos --batches 1   # for a rocprofv3 --kernel-trace
                                                                          # --stats pass of its own (launches per batch: two such runs,
                                                                          # --batches 1 and 3, differenced)

Models: BASELINE configs[1] (1-layer decoder) and es_en_20h (3 layers), both H 512, V 1098, random weights (seed 0), `Wo` x 8.  Batches: the
fisher_dev frame counts (tests/golden/fisher_20h_frames.json) in the loader's length buckets (width 80, 20 buckets), 32 utterances per
batch, each batch padded to its longest utterance (at most 1680 frames) -- the shapes NN.predict sees; `--batches K` times K batches spread
evenly over that plan (sorted by length) and projects the whole dev pass as their mean times the number of batches.  Features N(0, 1).
Cases: EOS never wins (every batch runs all 175 steps) and an early stop (the EOS bias searched in both directions until the first timed
batch stops between steps 35 and 45).  Each predict call is also checked for the path it took (last_predict_path), and the encoder pass of
every batch (encode + init_decoder_state) is timed on its own, so that the decoder's share of both columns is known."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ast_amd import _lib  # noqa: E402
from ast_amd.seq2seq import SpeechEncoderDecoder, using_config  # noqa: E402
from conftest import tiny_cfg  # noqa: E402
from oracle import ast_ref as R  # noqa: E402

SHAPES = {"configs1": dict(enc_layers=3, dec_layers=1, H=512, E=128, A=512, c0=128, c1=512, V=1098),
          "es_en_20h": dict(enc_layers=3, dec_layers=3, H=512, E=128, A=512, c0=128, c1=512, V=1098)}
GO, EOS, EPOCH_S, MAX_FRAMES, WIDTH, NUM_B = 1, 2, 2.39, 1680, 80, 20


def dev_plan(seed=0):
    """(rows, frames) of every fisher_dev batch: length buckets of the loader, 32 rows, padded to the longest row."""
    fr = json.load(open(os.path.join(ROOT, "tests", "golden", "fisher_20h_frames.json")))["frames"]["fisher_dev"]
    buckets = [[] for _ in range(NUM_B)]
    for f in fr:
        buckets[min(int(f) // WIDTH, NUM_B - 1)].append(min(int(f), MAX_FRAMES))
    rng = np.random.default_rng(seed)
    plan = []
    for b in buckets:
        rng.shuffle(b)
        for i in range(0, len(b), 32):
            plan.append((len(b[i:i + 32]), max(b[i:i + 32])))
    return sorted(plan, key=lambda p: p[1])


def model(shape, eos_bias):
    cfg = tiny_cfg(**shape)
    cfg["rnn_config"]["dec_vocab_size"] = shape["V"]
    P = R.init_params(cfg, 80, shape["V"], seed=0, dtype=np.float32)
    P["out/W"] = (P["out/W"] * 8).astype(np.float32)
    P["out/b"] = P["out/b"].copy()
    P["out/b"][EOS] += eos_bias
    return SpeechEncoderDecoder(0, cfg).materialize(80, values=P)


def set_eos_bias(m, bias):
    with torch.no_grad():
        m.arena.views["out/b"][EOS] = float(bias)


def timed_predict(m, X, stop, persist):
    with _lib.tuning({"dec.persist": persist}):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = m.predict(X, GO, EOS, stop)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
    want = "device" if persist else "steps"
    assert m.last_predict_path == want, (m.last_predict_path, want)
    return dt, out


def timed_scored(m, X, stop, y):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = m.predict_scored(X, GO, EOS, stop, y=y)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    assert m.last_predict_path == "device", m.last_predict_path
    return dt, out


def run_scored(m, name, case, Xs, ys, stop, reps, n_plan):
    """The device loop three ways on the same batches, alternating within every repetition; per batch the median over the repetitions."""
    for X, y in zip(Xs, ys):                                         # warm-up of every shape of all three
        timed_predict(m, X, stop, 1)
        timed_scored(m, X, stop, None)
        timed_scored(m, X, stop, y)
    t = {k: [[] for _ in Xs] for k in ("unscored", "scored", "scored_y")}
    te, steps = [[] for _ in Xs], [0] * len(Xs)
    for _ in range(reps):
        for i, (X, y) in enumerate(zip(Xs, ys)):
            dt, out = timed_predict(m, X, stop, 1)
            t["unscored"][i].append(dt)
            dt, r0 = timed_scored(m, X, stop, None)
            t["scored"][i].append(dt)
            dt, r1 = timed_scored(m, X, stop, y)
            t["scored_y"][i].append(dt)
            te[i].append(timed_encode(m, X))
            assert (r0.tokens == out).all() and (r1.tokens == out).all()
            steps[i] = out.shape[1]
    enc = np.array([np.median(v) for v in te])
    res = dict(shape=name, case=case, reps=reps, frames=[int(X.shape[1]) for X in Xs], steps=steps, ms_encode=round(1e3 * float(enc.mean()), 3))
    for k, v in t.items():
        med = np.array([np.median(b) for b in v])
        res["ms_" + k] = round(1e3 * float(med.mean()), 3)
        res["us_per_step_" + k] = round(1e6 * float(((med - enc) / np.array(steps)).mean()), 2)
        res["spread_" + k] = round(float(np.mean([(max(b) - min(b)) / np.median(b) for b in v])), 3)
        res["dev_pass_s_" + k] = round(n_plan * float(med.mean()), 3)
    res["ratio_per_step_scored"] = round(res["us_per_step_scored"] / res["us_per_step_unscored"], 3)
    res["ratio_per_step_scored_y"] = round(res["us_per_step_scored_y"] / res["us_per_step_unscored"], 3)
    print(json.dumps(res), flush=True)


def timed_encode(m, X):
    with using_config("train", False):
        torch.cuda.synchronize()
        t = time.perf_counter()
        m._cur = None
        m.encode(X)
        m.init_decoder_state()
        torch.cuda.synchronize()
        return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--stop", type=int, default=175)
    ap.add_argument("--only", default="", choices=["", "device"])
    ap.add_argument("--shape", default="", choices=[""] + list(SHAPES))
    ap.add_argument("--case", default="", choices=["", "no_eos", "early"])
    ap.add_argument("--scored", action="store_true", help="time the device loop unscored, scored without targets and scored with targets")
    ap.add_argument("--reps", type=int, default=7, help="--scored: repetitions of every batch (the median is reported)")
    a = ap.parse_args()
    plan = dev_plan()
    idx = np.linspace(0, len(plan) - 1, a.batches).round().astype(int) if a.batches > 1 else [len(plan) // 2]
    rng = np.random.default_rng(1)
    Xs = [torch.from_numpy(rng.standard_normal((plan[i][0], plan[i][1], 80)).astype(np.float32)).cuda() for i in idx]
    for name, shape in SHAPES.items():
        if a.shape and name != a.shape:
            continue
        m = model(shape, 0.0)
        for case in ("no_eos", "early"):
            if a.case and case != a.case:
                continue
            if case == "no_eos":
                set_eos_bias(m, -1e4)
            else:                   # bisection on the EOS bias: the number of steps falls as the bias rises
                lo, hi = -60.0, 60.0
                for _ in range(20):
                    mid = 0.5 * (lo + hi)
                    set_eos_bias(m, mid)
                    n = timed_predict(m, Xs[0], a.stop, 1)[1].shape[1]
                    if n > 45:
                        lo = mid
                    elif n < 35:
                        hi = mid
                    else:
                        break
            if a.scored:
                # targets of the longest padded length the loader makes (max_pred 175), a quarter of them PAD
                ys = []
                for X in Xs:
                    y = rng.integers(1, shape["V"], size=(X.shape[0], a.stop)).astype(np.int32)
                    y[rng.random(y.shape) < 0.25] = 0
                    ys.append(torch.from_numpy(y).cuda())
                run_scored(m, name, case, Xs, ys, a.stop, a.reps, len(plan))
                continue
            timed_predict(m, Xs[0], a.stop, 1)                       # warm-up of both paths
            if a.only != "device":
                timed_predict(m, Xs[0], a.stop, 0)
            td, ts, te, steps = [], [], [], []
            for X in Xs:
                t, out = timed_predict(m, X, a.stop, 1)
                td.append(t)
                steps.append(out.shape[1])
                if a.only != "device":
                    ts_, out_s = timed_predict(m, X, a.stop, 0)
                    ts.append(ts_)
                    te.append(timed_encode(m, X))
            if a.only == "device":
                print(json.dumps(dict(shape=name, case=case, batches=len(Xs), steps=steps, ms_device=1e3 * float(np.mean(td)))), flush=True)
                continue
            ms_d, ms_s, ms_e = 1e3 * np.mean(td), 1e3 * np.mean(ts), 1e3 * np.mean(te)
            tok = float(np.mean([s * X.shape[0] for s, X in zip(steps, Xs)]))
            nb = len(plan)
            print(json.dumps(dict(shape=name, case=case, batches_timed=len(Xs), frames=[int(X.shape[1]) for X in Xs], steps=steps,
                                  ms_device=round(ms_d, 2), ms_steps=round(ms_s, 2), ms_encode=round(ms_e, 2),
                                  ms_device_decoder=round(ms_d - ms_e, 2), ms_steps_decoder=round(ms_s - ms_e, 2),
                                  speedup=round(ms_s / ms_d, 2), speedup_decoder=round((ms_s - ms_e) / (ms_d - ms_e), 2),
                                  tok_s_device=round(tok / (ms_d / 1e3)), tok_s_steps=round(tok / (ms_s / 1e3)), dev_batches=nb,
                                  dev_pass_device_s=round(nb * ms_d / 1e3, 2), dev_pass_steps_s=round(nb * ms_s / 1e3, 2),
                                  epoch_s=EPOCH_S)), flush=True)


if __name__ == "__main__":
    main()
