"""Per-row source lengths in the encoder: what one batched encoder pass buys, and what the untouched entry
points cost beside the parent commit's.

    python scratch/encode_rows_throughput.py --encode --packed                       # (a), (b)
    python scratch/encode_rows_throughput.py --abi --parent-lib DIR/libastk.so       # (c)

Set-up of scratch/rows_throughput.py (b): the es_en_20h model and 64 utterances drawn from the fisher_dev frame counts (mean 353, max
1169 frames).  One process, every route warmed up first, then 7 repetitions with the routes alternating inside a repetition, each timed
to a device synchronise; reported are the median and the spread (max - min) / median.
(a) The encoder pass of all 64 utterances: every utterance alone (encode + init_decoder_state at batch 1: today's path) against the
    batched path in calls of U = 8 and U = 32 consecutive utterances (what `-b U` hands to encode_rows), and all 64 in one call of the
    helper (two batches of 32, ordered by length).
(b) The two packed passes of section 15 -- score_hypotheses_packed at 6 utterances per call (5 hypotheses of 41 tokens each),
    sample_hypotheses_packed at 8 (n = 4, stop limit 40) -- with model.batch_encode off and on.
(c) astk_conv_bn_relu_fwd (train = 0) and astk_lstm_stack_fwd (no masks) of this tree's libastk.so against another build -- the parent
    commit's, built into a side directory -- each in a child process of its own (ASTK_LIB_PATH), alternating one repetition at a time, on
    three shapes: one utterance of 353 and of 1169 frames, and a batch of 32 x 800."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("astk_conv_bn_relu_fwd_rows", "astk_lstm_stack_rows_workspace_bytes", "astk_lstm_stack_fwd_rows")
ABI_SHAPES = ((1, 353), (1, 1169), (32, 800))


def stats(v):
    med = float(np.median(v))
    return dict(ms=round(1e3 * med, 3), spread=round((max(v) - min(v)) / med, 3))


def setup(n_utts):
    import copy
    from beam_throughput import CFG
    from greedy_throughput import set_eos_bias
    from ast_amd.seq2seq import SpeechEncoderDecoder
    frames = json.load(open(os.path.join(ROOT, "tests", "golden", "fisher_20h_frames.json")))["frames"]
    pool = np.concatenate([np.asarray(v) for v in frames.values()])
    rng = np.random.default_rng(0)
    lens = rng.choice(pool, n_utts)
    Xs = [torch.from_numpy(rng.standard_normal((1, int(T), 80)).astype(np.float32)).cuda() for T in lens]
    m = SpeechEncoderDecoder(0, copy.deepcopy(CFG)).materialize(80, seed=0)
    set_eos_bias(m, -1e4)
    return m, Xs, lens, rng


def timed_routes(routes, reps):
    from rows_throughput import sync_time
    for fn in routes.values():
        fn()
        fn()                             # warm-up of every route on every shape
    t = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():     # alternating
            t[k].append(sync_time(fn)[0])
    return t


def encode(m, Xs, lens, reps):
    def batched(U):
        def run():
            for i in range(0, len(Xs), U):
                m._encode_utts(Xs[i:i + U], batch_encode=True)
                assert m.last_encode_path == "batched"
        return run
    routes = {"alone": lambda: m._encode_utts(Xs, batch_encode=False), "batched_u8": batched(8), "batched_u32": batched(32),
              "batched_all_sorted": batched(len(Xs))}
    t = timed_routes(routes, reps)
    res = dict(what="encoder pass", utts=len(Xs), reps=reps, frames_mean=float(lens.mean()), frames_max=int(lens.max()))
    for k, v in t.items():
        res[k] = stats(v)
        res[k]["ms_per_utt"] = round(res[k]["ms"] / len(Xs), 4)
        res[k]["alone_over_this"] = round(float(np.median(t["alone"]) / np.median(v)), 3)
    print(json.dumps(res), flush=True)


def packed(m, Xs, lens, rng, reps):
    from greedy_throughput import GO
    from ast_amd import nn as gnn
    V, L, n_hyp, n_smp, stop = 1098, 41, 5, 4, 40
    hyps = [[[GO] + rng.integers(3, V, size=L - 1).tolist() for _ in range(n_hyp)] for _ in Xs]

    def group(U, fn):
        return [fn(Xs[i:i + U], i) for i in range(0, len(Xs), U)]

    def route(kind, on):
        def run():
            m.batch_encode = on
            try:
                if kind == "rescore":
                    group(6, lambda xs, i: gnn.score_hypotheses_packed(m, xs, hyps[i:i + len(xs)], max_utts=6))
                else:
                    group(8, lambda xs, i: gnn.sample_hypotheses_packed(m, xs, n_smp, stop, 7, first_streams=[(i + j) * n_smp for j in range(len(xs))],
                                                                        max_utts=8))
                assert m.last_encode_path == ("batched" if on else "alone")
            finally:
                m.batch_encode = False
        return run
    routes = {f"{kind}_{tag}": route(kind.split("_")[0], on) for kind in ("rescore_b6", "sample_b8") for tag, on in (("alone", False), ("batched", True))}
    t = timed_routes(routes, reps)
    assert m.last_predict_path == "device" and m.last_score_path == "device"
    res = dict(what="packed passes", utts=len(Xs), reps=reps)
    for k, v in t.items():
        res[k] = stats(v)
        res[k]["utts_per_s"] = round(len(Xs) / float(np.median(v)), 2)
    for kind in ("rescore_b6", "sample_b8"):
        res["gain_" + kind] = round(float(np.median(t[kind + "_alone"]) / np.median(t[kind + "_batched"])), 3)
    print(json.dumps(res), flush=True)


# ---------------------------------------------------------------------------------------------------- (c)
def abi_child(no_new):
    from ast_amd import _lib
    if no_new:                           # the other build does not export them
        for k in NEW_SYMBOLS:
            _lib.SIGNATURES.pop(k)
    from rows_throughput import sync_time
    from ast_amd.seq2seq import _vp, using_config
    m, _, _, rng = setup(1)
    lib = _lib.load()
    cases = []
    for B, T in ABI_SHAPES:
        X = torch.from_numpy(rng.standard_normal((B, T, 80)).astype(np.float32)).cuda()
        with using_config("train", False):
            m._cur = None
            m.encode(X)                  # the shape's descriptors, buffers and workspaces; the side stream as the model sets it
        cases.append((B, T, X, m._cur))

    def rep():
        out = []
        for B, T, X, st in cases:
            wc, wl, s = m._workspace("cnn", st["ws_cnn"]), m._workspace("lstm", st["ws_lstm"]), m._stream()
            conv = lambda: [lib.astk_conv_bn_relu_fwd(C.byref(st["cd"]), st["cp"], _vp(X), None, _vp(st["xlstm"]), _vp(wc), wc.numel(), 0, s)
                            for _ in range(5)]
            lstm = lambda: [lib.astk_lstm_stack_fwd(C.byref(st["ld"]), st["lp"], _vp(st["xlstm"]), None, _vp(st["enc_states"]), _vp(st["cT"]),
                                                    _vp(st["hT"]), _vp(wl), wl.numel(), s) for _ in range(5)]
            for name, fn in (("conv", conv), ("lstm", lstm)):
                dt, rcs = sync_time(fn)
                assert not any(rcs)
                out.append(dict(op=name, B=B, T=T, s=dt / 5))
        return out
    rep()
    rep()
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "rep":
            break
        print(json.dumps(rep()), flush=True)


def abi(parent_lib, reps):
    def child(lib_path, no_new):
        env = dict(os.environ)
        if lib_path:
            env["ASTK_LIB_PATH"] = os.path.abspath(lib_path)
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--abi-child"] + (["--no-new"] if no_new else []), env=env,
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert p.stdout.readline().strip() == "ready", "the child did not come up"
        return p
    kids = {"this": child(None, False), "parent": child(parent_lib, True)}
    t = {}
    try:
        for r in range(reps):
            for k in (("this", "parent") if r % 2 == 0 else ("parent", "this")):        # alternating, and the order alternates too
                kids[k].stdin.write("rep\n")
                kids[k].stdin.flush()
                for e in json.loads(kids[k].stdout.readline()):
                    t.setdefault((e["op"], e["B"], e["T"]), {}).setdefault(k, []).append(e["s"])
    finally:
        for p in kids.values():
            p.stdin.write("quit\n")
            p.stdin.close()
            p.wait(timeout=60)
    for (op, B, T), per in sorted(t.items()):
        res = dict(what="untouched entry point", op=op, B=B, T=T, reps=reps, this=stats(per["this"]), parent=stats(per["parent"]))
        res["this_over_parent"] = round(float(np.median(per["this"]) / np.median(per["parent"])), 4)
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encode", action="store_true")
    ap.add_argument("--packed", action="store_true")
    ap.add_argument("--abi", action="store_true")
    ap.add_argument("--parent-lib", default="", help="(c): the other build of libastk.so")
    ap.add_argument("--abi-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-new", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.abi_child:
        abi_child(a.no_new)
        return
    if a.encode or a.packed:
        m, Xs, lens, rng = setup(a.utts)
        if a.encode:
            encode(m, Xs, lens, a.reps)
        if a.packed:
            packed(m, Xs, lens, rng, a.reps)
    if a.abi:
        assert a.parent_lib, "--abi needs --parent-lib"
        abi(a.parent_lib, a.reps)


if __name__ == "__main__":
    main()
