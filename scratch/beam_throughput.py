"""Beam-search throughput: decode_beam (one utterance, one hypothesis at a time) against decode_beam_batch (U utterances per step).

    python scratch/beam_throughput.py                   # sequential path on --seq-utts utterances, then U = 8, 32, 64
    python scratch/beam_throughput.py --only 32         # one batched run (for a rocprofv3 --kernel-trace --stats pass of its own)

Model: the es_en_20h shape as bench.py --model es_en_20h builds it (3-layer encoder and decoder, hidden 512, V = 1098), random weights
(seed 0).  64 synthetic utterances (features N(0, 1), 80 dims) with frame counts drawn from tests/golden/fisher_20h_frames.json.
N = K = 5, stop_limit 175, EOS not forced: with random weights nearly every hypothesis runs to the limit, the worst case.  Every figure
is timed to a device synchronise after a warm-up.  The sequential path runs a subset of the utterances (it takes ~1 s per utterance
and step budget); utterances/s are per utterance either way."""
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

from ast_amd import nn as gnn  # noqa: E402
from ast_amd.seq2seq import SpeechEncoderDecoder  # noqa: E402

CFG = {"dropout": {"embed": 0.3, "rnn": 0.3, "out": 0},
       "rnn_config": {"bi_rnn": True, "enc_layers": 3, "dec_layers": 3, "hidden_units": 512, "embedding_units": 128,
                      "attn_units": 512, "n_attn": 1, "feed_attn": True, "ln": False, "dec_vocab_size": 1098},
       "cnn_config": {"bn": True, "cnn_layers": [
           {"in_channels": None, "out_channels": 128, "ksize": [9, 13], "stride": [2, 13], "pad": [4, 0]},
           {"in_channels": None, "out_channels": 512, "ksize": [9, 1], "stride": [2, 1], "pad": [4, 0]}]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--seq-utts", type=int, default=4)
    ap.add_argument("--stop", type=int, default=175)
    ap.add_argument("--only", type=int, default=0, help="run one batched search of this many utterances and nothing else")
    a = ap.parse_args()
    D, N, K = 80, 5, 5
    frames = json.load(open(os.path.join(ROOT, "tests", "golden", "fisher_20h_frames.json")))["frames"]
    pool = np.concatenate([np.asarray(v) for v in frames.values()])
    rng = np.random.default_rng(0)
    lens = rng.choice(pool, a.utts)
    Xs = [torch.from_numpy(rng.standard_normal((1, int(T), D)).astype(np.float32)).cuda() for T in lens]
    m = SpeechEncoderDecoder(0, copy.deepcopy(CFG)).materialize(D, seed=0)
    # warm-up: both paths, short
    gnn.decode_beam_batch(m, Xs[:2], 3, N, K)
    gnn.decode_beam(m, Xs[0], 3, N, K)
    torch.cuda.synchronize()
    res = {"frames_mean": float(lens.mean()), "frames_max": int(lens.max()), "N": N, "K": K, "stop_limit": a.stop}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    if a.only:
        dt, out = timed(lambda: gnn.decode_beam_batch(m, Xs[:a.only], a.stop, N, K))
        res[f"batch_U{a.only}"] = {"s": dt, "utt_per_s": a.only / dt, "mean_hyp_len": float(np.mean([len(l[0]["hyp"]) for l in out]))}
        print(json.dumps(res))
        return
    dt, out = timed(lambda: [gnn.decode_beam(m, X, a.stop, N, K) for X in Xs[:a.seq_utts]])
    res["sequential"] = {"utts": a.seq_utts, "s": dt, "utt_per_s": a.seq_utts / dt, "mean_hyp_len": float(np.mean([len(l[0]["hyp"]) for l in out]))}
    for U in (8, 32, 64):
        if U > a.utts:
            continue
        dt, out = timed(lambda: gnn.decode_beam_batch(m, Xs[:U], a.stop, N, K))
        res[f"batch_U{U}"] = {"s": dt, "utt_per_s": U / dt, "speedup": (U / dt) / res["sequential"]["utt_per_s"],
                              "mean_hyp_len": float(np.mean([len(l[0]["hyp"]) for l in out]))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
