"""Per-row source lengths in the decode loops: what they cost where they are not used, and what packing buys.

    python scratch/rows_throughput.py --abi --parent-lib DIR/libastk.so      # (a)
    python scratch/rows_throughput.py --packed                               # (b)

(a) The existing entry points (NULL lengths) of this tree's libastk.so against another build of the library -- the parent commit's,
built into a side directory -- each loaded in a child process of its own (ASTK_LIB_PATH).  Both children hold the same models and the
same four fisher_dev batches (scratch/greedy_throughput.py's plan), warm every route up, and then run ONE repetition at a time when this
process tells them to, alternating between the two libraries, so that drift of the clocks hits both alike.  A route is
astk_greedy_decode (EOS never wins: 175 steps) or astk_forced_score (L = 176, no alpha) alone, on buffers allocated beforehand, timed
to a device synchronise, the encoder pass not included.  Reported: us per decoder step (the median over the repetitions per batch, the
mean over the batches), the run-to-run spread (max - min) / median as sections 12-14 report it, and the difference between the two
libraries beside that spread.

(b) Utterances per second of n-best rescoring (5 hypotheses per utterance, 41 tokens each) and of n = 4 sampling (stop limit 40, EOS
never drawn early) on the es_en_20h shape over the 64 utterances of scratch/beam_throughput.py: one utterance per call (-b 1: X
repeated over its rows, today's path) against 6 (rescoring: 30 rows) and 8 (sampling: 32 rows) utterances per call.  The encoder pass
per utterance is the same either way and is timed on its own, so the decoder's share -- the bound of the gain -- is in the table."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROWS_SYMBOLS = ("astk_greedy_decode_rows", "astk_greedy_decode_scored_rows", "astk_sample_decode_rows", "astk_forced_score_rows")
STEPS = 175


def sync_time(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


# ---------------------------------------------------------------------------------------------------- (a)
def abi_child(no_rows):
    from ast_amd import _lib
    if no_rows:                          # the other build does not export them
        for k in ROWS_SYMBOLS:
            _lib.SIGNATURES.pop(k)
    from greedy_throughput import EOS, GO, SHAPES, dev_plan, model, set_eos_bias
    from ast_amd.seq2seq import using_config
    lib = _lib.load()
    plan = dev_plan()
    idx = np.linspace(0, len(plan) - 1, 4).round().astype(int)
    rng = np.random.default_rng(1)
    Xs = [torch.from_numpy(rng.standard_normal((plan[i][0], plan[i][1], 80)).astype(np.float32)).cuda() for i in idx]
    P = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + off)
    cases = []
    for name, shape in SHAPES.items():
        m = model(shape, 0.0)
        set_eos_bias(m, -1e4)
        for X in Xs:
            B = int(X.shape[0])
            y = rng.integers(1, shape["V"], size=(B, STEPS + 1)).astype(np.int32)
            y[:, 0] = GO
            cases.append((name, m, X, torch.from_numpy(y).cuda(), torch.empty(4 + 3 * STEPS * B, dtype=torch.int32, device="cuda")))

    def run(mode, m, X, yd, out):
        with using_config("train", False):
            m._cur = None
            m.encode(X)
            m.init_decoder_state()
        st = m._cur
        B = st["B"]
        query = lib.astk_greedy_workspace_bytes if mode == "greedy" else lib.astk_forced_workspace_bytes
        ws = m._workspace("decode", int(query(C.byref(st["dd"]), STEPS, *(() if mode == "greedy" else (0,)))))
        head = (C.byref(st["dd"]), C.byref(st["dp"]), P(st["enc_states"]), P(m._dec_c), P(m._dec_h))
        if mode == "greedy":
            call = lambda: lib.astk_greedy_decode(*head, GO, EOS, STEPS, P(out, 16), P(out), P(out, 4), P(ws), ws.numel(), m._stream())
        else:
            call = lambda: lib.astk_forced_score(*head, P(yd), STEPS + 1, P(out, 16), P(out, 16 + 4 * STEPS * B), P(out, 16 + 8 * STEPS * B), None,
                                                 P(out), P(ws), ws.numel(), m._stream())
        dt, rc = sync_time(call)
        head4 = out[:4].cpu()
        assert rc == 0 and (int(head4[0]) == STEPS and float(head4[1:2].view(torch.float32)) == 0 if mode == "greedy" else int(head4[0]) == 0)
        return dt
    rep = lambda: [dict(shape=name, mode=mode, frames=int(X.shape[1]), s=run(mode, m, X, yd, out)) for name, m, X, yd, out in cases
                   for mode in ("greedy", "forced")]
    rep()
    rep()                                # warm-up of every route on every shape
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "rep":
            break
        print(json.dumps(rep()), flush=True)


def abi(parent_lib, reps):
    def child(lib_path, no_rows):
        env = dict(os.environ)
        if lib_path:
            env["ASTK_LIB_PATH"] = os.path.abspath(lib_path)
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--abi-child"] + (["--no-rows"] if no_rows else []), env=env,
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert p.stdout.readline().strip() == "ready", "the child did not come up"
        return p
    kids = {"this": child(None, False), "parent": child(parent_lib, True)}
    t = {}
    for r in range(reps):
        for k in (("this", "parent") if r % 2 == 0 else ("parent", "this")):        # alternating, and the order alternates too
            kids[k].stdin.write("rep\n")
            kids[k].stdin.flush()
            for e in json.loads(kids[k].stdout.readline()):
                t.setdefault((e["shape"], e["mode"], k), {}).setdefault(e["frames"], []).append(e["s"])
    for p in kids.values():
        p.stdin.write("quit\n")
        p.stdin.close()
        p.wait(timeout=60)
    for (shape, mode) in sorted({k[:2] for k in t}):
        res = dict(shape=shape, mode=mode, steps=STEPS, reps=reps)
        for k in ("this", "parent"):
            per = t[shape, mode, k]
            med = np.array([np.median(v) for v in per.values()])
            res["us_per_step_" + k] = round(1e6 * float((med / STEPS).mean()), 3)
            res["spread_" + k] = round(float(np.mean([(max(v) - min(v)) / np.median(v) for v in per.values()])), 4)
        res["this_over_parent"] = round(res["us_per_step_this"] / res["us_per_step_parent"], 4)
        print(json.dumps(res), flush=True)


# ---------------------------------------------------------------------------------------------------- (b)
def packed(n_utts, reps):
    import copy
    from beam_throughput import CFG
    from greedy_throughput import EOS, GO, set_eos_bias, timed_encode
    from ast_amd import nn as gnn
    from ast_amd.seq2seq import SpeechEncoderDecoder
    D, V, L, n_hyp, n_smp, stop = 80, 1098, 41, 5, 4, 40
    frames = json.load(open(os.path.join(ROOT, "tests", "golden", "fisher_20h_frames.json")))["frames"]
    pool = np.concatenate([np.asarray(v) for v in frames.values()])
    rng = np.random.default_rng(0)
    lens = rng.choice(pool, n_utts)
    Xs = [torch.from_numpy(rng.standard_normal((1, int(T), D)).astype(np.float32)).cuda() for T in lens]
    m = SpeechEncoderDecoder(0, copy.deepcopy(CFG)).materialize(D, seed=0)
    set_eos_bias(m, -1e4)
    hyps = [[[GO] + rng.integers(3, V, size=L - 1).tolist() for _ in range(n_hyp)] for _ in Xs]

    def group(U, fn):
        return [fn(Xs[i:i + U], i) for i in range(0, len(Xs), U)]
    routes = {
        "rescore_b1": lambda: [gnn.score_hypotheses(m, X, h) for X, h in zip(Xs, hyps)],
        "rescore_b6": lambda: group(6, lambda xs, i: gnn.score_hypotheses_packed(m, xs, hyps[i:i + len(xs)], max_utts=6)),
        "sample_b1": lambda: [gnn.sample_hypotheses(m, X, n_smp, stop, 7, first_stream=k * n_smp) for k, X in enumerate(Xs)],
        "sample_b8": lambda: group(8, lambda xs, i: gnn.sample_hypotheses_packed(m, xs, n_smp, stop, 7, first_streams=[(i + j) * n_smp for j in range(len(xs))],
                                                                              max_utts=8)),
    }
    for fn in routes.values():
        fn()                             # warm-up of every route on every shape
    assert m.last_predict_path == "device" and m.last_score_path == "device"
    t = {k: [] for k in routes}
    te = []
    for _ in range(reps):
        for k, fn in routes.items():     # alternating
            t[k].append(sync_time(fn)[0])
        te.append(sum(timed_encode(m, X) for X in Xs))
    enc = float(np.median(te))
    res = dict(utts=n_utts, reps=reps, frames_mean=float(lens.mean()), frames_max=int(lens.max()), s_encode_all=round(enc, 4))
    for k, v in t.items():
        med = float(np.median(v))
        res["utts_per_s_" + k] = round(n_utts / med, 2)
        res["spread_" + k] = round((max(v) - min(v)) / med, 3)
        res["decoder_share_" + k] = round(1 - enc / med, 3)
    res["gain_rescore"] = round(res["utts_per_s_rescore_b6"] / res["utts_per_s_rescore_b1"], 3)
    res["gain_sample"] = round(res["utts_per_s_sample_b8"] / res["utts_per_s_sample_b1"], 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--abi", action="store_true")
    ap.add_argument("--parent-lib", default="", help="(a): the other build of libastk.so")
    ap.add_argument("--abi-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-rows", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.abi_child:
        abi_child(a.no_rows)
    if a.abi:
        assert a.parent_lib, "--abi needs --parent-lib"
        abi(a.parent_lib, a.reps)
    if a.packed:
        packed(a.utts, a.reps)


if __name__ == "__main__":
    main()
