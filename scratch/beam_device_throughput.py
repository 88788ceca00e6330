"""Beam-search throughput: decode_beam_batch (one astk_beam_step per decoder step) at U = 1, 6 and 32 utterances per search against
decode_beam_device (the whole search of up to 6 utterances in one persistent launch), same process, alternating.

    python scratch/beam_device_throughput.py [--utts 32] [--reps 3]

Workload: DESIGN.md section 10's (scratch/beam_throughput.py) -- the es_en_20h shape with random weights (seed 0), synthetic utterances
with frame counts drawn from tests/golden/fisher_20h_frames.json, N = K = 5, stop_limit 175, EOS not forced (nearly every hypothesis
runs to the limit).  Every figure is timed to a device synchronise after a warm-up, the median of --reps repetitions; encoding is
included on both sides (every utterance is encoded alone either way).  us per step = wall time / (searches or launches x steps run)."""
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
from beam_throughput import CFG  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--stop", type=int, default=175)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    D, N, K = 80, 5, 5
    frames = json.load(open(os.path.join(ROOT, "tests", "golden", "fisher_20h_frames.json")))["frames"]
    pool = np.concatenate([np.asarray(v) for v in frames.values()])
    rng = np.random.default_rng(0)
    lens = rng.choice(pool, a.utts)
    Xs = [torch.from_numpy(rng.standard_normal((1, int(T), D)).astype(np.float32)).cuda() for T in lens]
    m = SpeechEncoderDecoder(0, copy.deepcopy(CFG)).materialize(D, seed=0)
    gnn.decode_beam_batch(m, Xs[:2], 3, N, K)
    gnn.decode_beam_device(m, Xs[:2], 3, N, K)
    assert m.last_beam_path == "device"
    torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def steps_of(lists):          # the steps a search ran: its longest hypothesis without GO (at most the limit)
        return min(a.stop, max(len(e["hyp"]) - 1 for lst in lists for e in lst))
    res = {"frames_mean": float(lens.mean()), "frames_max": int(lens.max()), "N": N, "K": K, "stop_limit": a.stop, "utts": a.utts}
    for U in (1, 6, 32):
        n = min(a.utts, max(U, 6))           # utterances of this comparison
        groups = [Xs[i:i + U] for i in range(0, n, U)]
        t_steps, t_dev, steps_b, steps_d = [], [], 0, 0
        for _ in range(a.reps):
            dt, outs = timed(lambda: [gnn.decode_beam_batch(m, g, a.stop, N, K) for g in groups])
            t_steps.append(dt)
            steps_b = sum(steps_of(o) for o in outs)
            dt, outs = timed(lambda: [gnn.decode_beam_device(m, g, a.stop, N, K) for g in groups])
            assert m.last_beam_path == "device"
            t_dev.append(dt)
            steps_d = 0
            for g in groups:          # (launches of 6 utterances; steps per launch from the stop word)
                gnn.decode_beam_device(m, g, a.stop, N, K)
                steps_d += sum(m.last_beam_steps)
        tb, td = float(np.median(t_steps)), float(np.median(t_dev))
        res[f"U{U}"] = {"utts": n, "batch_s": tb, "device_s": td, "batch_utt_per_s": n / tb, "device_utt_per_s": n / td,
                        "batch_us_per_step": 1e6 * tb / steps_b, "device_us_per_step": 1e6 * td / steps_d,
                        "steps_batch": steps_b, "steps_device": steps_d, "per_utt_gain": tb / td,
                        "per_step_gain": (tb / steps_b) / (td / steps_d)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
