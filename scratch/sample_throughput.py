"""Sampled decoding throughput (SpeechEncoderDecoder.sample): the persistent loop's sampled mode against its
scored greedy mode, in the same process, alternating, and n-best lists from sampling beside batched beam search.

    python scratch/sample_throughput.py                      # the per-step cost on both shapes, then the hypotheses per second
    python scratch/sample_throughput.py --part step          # only the per-step cost (scored greedy / sampled, alternating)
    python scratch/sample_throughput.py --part nbest         # only hypotheses per second (sample_hypotheses n = 32 / decode_beam_batch)
    python scratch/sample_throughput.py --part step --top-k 1,5,16 [--top-p 0.9]
                                                             # the truncated loop beside the untruncated one

Per-step cost: the models and the four loader-bucketed fisher_dev batches of scratch/greedy_throughput.py --scored (32 rows, EOS never
wins: both modes run all --stop steps), a warm-up of every shape, then --reps repetitions alternating predict_scored (no targets) and
sample, each call timed to a device synchronise; per batch the median; per decoder step = (batch time - the batch's encoder pass) /
steps.  The yardstick is scored greedy re-measured in this call.  --top-k K[,K..] adds one truncated sampled loop per K (with --top-p)
to the alternation: the same batches, the same repetitions, their per-step cost beside the untruncated sampled loop's of the same run.
Hypotheses per second: the es_en_20h model and the 64 utterances of scratch/beam_throughput.py, stop_limit 175, EOS not forced:
sample_hypotheses(n = 32) utterance by utterance against decode_beam_batch(N = K = 5, U = 32), both timed to a device synchronise
after a warm-up.  The two searches do different things; the figure records what an n-best list costs either way."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import beam_throughput as bt  # noqa: E402
import greedy_throughput as gt  # noqa: E402
from ast_amd import nn as gnn  # noqa: E402
from ast_amd.seq2seq import SpeechEncoderDecoder  # noqa: E402

GO, EOS = gt.GO, gt.EOS


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def run_step_cost(name, shape, Xs, stop, reps, temperature, top_ks=(), top_p=1.0):
    m = gt.model(shape, 0.0)
    gt.set_eos_bias(m, -1e4)
    scored = lambda X: m.predict_scored(X, GO, EOS, stop)
    sampled = lambda X: m.sample(X, GO, EOS, stop, 2024, temperature=temperature)
    trunc = {f"topk{k}": (lambda X, k=k: m.sample(X, GO, EOS, stop, 2024, temperature=temperature, top_k=k, top_p=top_p)) for k in top_ks}
    for X in Xs:
        scored(X)
        sampled(X)
        for fn in trunc.values():
            fn(X)
    t = {"scored": [[] for _ in Xs], "sampled": [[] for _ in Xs], **{k: [[] for _ in Xs] for k in trunc}}
    te = [[] for _ in Xs]
    for _ in range(reps):
        for i, X in enumerate(Xs):
            dt, r0 = timed(lambda: scored(X))
            assert m.last_predict_path == "device" and r0.n_steps == stop
            t["scored"][i].append(dt)
            dt, r1 = timed(lambda: sampled(X))
            assert m.last_predict_path == "device" and r1.n_steps == stop
            t["sampled"][i].append(dt)
            for k, fn in trunc.items():
                dt, r2 = timed(lambda: fn(X))
                assert m.last_predict_path == "device" and r2.n_steps == stop
                t[k][i].append(dt)
            te[i].append(gt.timed_encode(m, X))
    enc = np.array([np.median(v) for v in te])
    res = dict(part="step", shape=name, reps=reps, temperature=temperature, frames=[int(X.shape[1]) for X in Xs], steps=stop,
               ms_encode=round(1e3 * float(enc.mean()), 3), differs_from_greedy=round(float((r0.tokens != r1.tokens).mean()), 3))
    for k, v in t.items():
        med = np.array([np.median(b) for b in v])
        res["ms_" + k] = round(1e3 * float(med.mean()), 3)
        res["us_per_step_" + k] = round(1e6 * float(((med - enc) / stop).mean()), 2)
        res["us_per_step_by_batch_" + k] = [round(1e6 * float(x), 2) for x in (med - enc) / stop]
        res["spread_" + k] = round(float(np.mean([(max(b) - min(b)) / np.median(b) for b in v])), 3)
    res["ratio_per_step"] = round(res["us_per_step_sampled"] / res["us_per_step_scored"], 3)
    if trunc:
        res["top_p"] = top_p
    for k in trunc:
        res["ratio_per_step_" + k] = round(res["us_per_step_" + k] / res["us_per_step_sampled"], 3)
    print(json.dumps(res), flush=True)


def run_nbest(utts, stop, n):
    D, N, K = 80, 5, 5
    frames = json.load(open(os.path.join(ROOT, "tests", "golden", "fisher_20h_frames.json")))["frames"]
    pool = np.concatenate([np.asarray(v) for v in frames.values()])
    rng = np.random.default_rng(0)
    lens = rng.choice(pool, utts)
    Xs = [torch.from_numpy(rng.standard_normal((1, int(T), D)).astype(np.float32)).cuda() for T in lens]
    m = SpeechEncoderDecoder(0, copy.deepcopy(bt.CFG)).materialize(D, seed=0)
    gnn.decode_beam_batch(m, Xs[:2], 3, N, K)
    gnn.sample_hypotheses(m, Xs[0], n, 3, 2024)
    dt_s, out_s = timed(lambda: [gnn.sample_hypotheses(m, X, n, stop, 2024, first_stream=i * n) for i, X in enumerate(Xs)])
    assert m.last_predict_path == "device"
    dt_b, out_b = timed(lambda: [l for lo in range(0, utts, 32) for l in gnn.decode_beam_batch(m, Xs[lo:lo + 32], stop, N, K)])
    hs, hb = sum(len(l) for l in out_s), sum(len(l) for l in out_b)
    print(json.dumps(dict(part="nbest", utts=utts, frames_mean=float(lens.mean()), frames_max=int(lens.max()), stop_limit=stop,
                          sample=dict(n=n, s=round(dt_s, 4), hyps=hs, hyp_per_s=round(hs / dt_s, 1), utt_per_s=round(utts / dt_s, 2),
                                      mean_hyp_len=float(np.mean([len(h["hyp"]) for l in out_s for h in l])),
                                      distinct_per_utt=float(np.mean([len({tuple(h["hyp"]) for h in l}) for l in out_s]))),
                          beam=dict(N=N, K=K, U=32, s=round(dt_b, 4), hyps=hb, hyp_per_s=round(hb / dt_b, 1), utt_per_s=round(utts / dt_b, 2),
                                    mean_hyp_len=float(np.mean([len(h["hyp"]) for l in out_b for h in l]))))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="", choices=["", "step", "nbest"])
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--stop", type=int, default=175)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", default="", help="comma-separated top_k values: also time the truncated sampled loop at each")
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("-n", type=int, default=32)
    a = ap.parse_args()
    if a.part in ("", "step"):
        plan = gt.dev_plan()
        idx = np.linspace(0, len(plan) - 1, a.batches).round().astype(int) if a.batches > 1 else [len(plan) // 2]
        rng = np.random.default_rng(1)
        Xs = [torch.from_numpy(rng.standard_normal((plan[i][0], plan[i][1], 80)).astype(np.float32)).cuda() for i in idx]
        for name, shape in gt.SHAPES.items():
            run_step_cost(name, shape, Xs, a.stop, a.reps, a.temperature, [int(k) for k in a.top_k.split(",") if k], a.top_p)
        del Xs
    if a.part in ("", "nbest"):
        run_nbest(a.utts, a.stop, a.n)


if __name__ == "__main__":
    main()
