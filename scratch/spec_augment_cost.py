"""What SpecAugment costs per train step, on bench.py's two workloads (configs[1] and the shipped es_en_20h
model: the same configs, batch, optimizer and step as bench.py builds them).

    python scratch/spec_augment_cost.py --parent-lib DIR/ast_amd/libastk.so

One child process holds both models on this tree's library and, after a warm-up, runs blocks of 50 steps ALTERNATING between three
variants: the call absent ("off"), and every step preceded by the one astk_spec_augment call on its batch, as the loader issues it, with
the zero fill and with the mean fill (two masks of each kind, F = 15, W = 40, p = 0.2).  The presentation counter moves on by B per
BLOCK, not per step: the steps of a block write the same spans into their copy of the batch, so the batch keeps four fifths of its
values (with a counter per step the masks pile up, the zero fill's batch drifts towards all zeros, and its steps ran 0.4 % FASTER than
the unmasked ones -- the clocks, not the kernel).
A second child runs the plain step on another build of the library -- the parent commit's, built in a checkout of its own (DIR) and
driven by that checkout's Python package.  The two children take turns block by block, so that drift of the clocks hits both alike.
Reported per workload and variant: the median ms/step over the blocks and the blocks' spread (max - min) / median.  The call's own time
comes from HIP events around 200 back-to-back calls on the 32 x 800 x 80 batch, priced against the bytes it moves: the masked share of
the batch written (the host model's count for the very counters used), plus the whole batch read once under the mean fill."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 50
SPEC = {"freq_masks": 2, "freq_width": 15, "time_masks": 2, "time_width": 40, "time_ratio": 0.2, "seed": 2024}


def child(tree, variants):
    sys.path.insert(0, tree)
    sys.path.append(ROOT)                                       # bench.py's configs (the same in both trees)
    import copy
    import numpy as np
    import torch
    import bench
    from ast_amd import optimizers as O
    from ast_amd.seq2seq import SpeechEncoderDecoder, using_config
    compute = torch.cuda.Stream()
    loads = {}
    for name in ("cfg1", "es_en_20h"):
        cfg = copy.deepcopy(bench.MODEL_CFG)
        if name == "es_en_20h":
            cfg["rnn_config"]["dec_layers"] = 3
        m = SpeechEncoderDecoder(0, cfg).materialize(80, seed=0)
        o = O.Adam(alpha=bench.TRAIN["lr"], beta1=0.9, beta2=0.999, eps=1e-8, amsgrad=True).setup(m)
        o.add_hook(O.WeightDecay(bench.TRAIN["l2"]))
        o.add_hook(O.GradientClipping(bench.TRAIN["grad_clip"]))
        Xh, yh = bench.synth_batch(32, 800, 80, 40, cfg["rnn_config"]["dec_vocab_size"], 20)
        loads[name] = (m, o, m.arena.data.clone(), torch.from_numpy(Xh).cuda(), torch.from_numpy(yh).cuda())
    lens = torch.full((32,), 800, dtype=torch.int32, device="cuda")
    counter = [0]
    if variants != ["off"]:
        from ast_amd import spec_augment as SA
        specs = {v: SA.checked_spec_augment(dict(SPEC, fill=v)) for v in variants if v != "off"}

    def mask(X, v, advance=True):
        SA.apply_device(X, lens, counter[0], 1, specs[v], torch.cuda.current_stream().cuda_stream)
        if advance:
            counter[0] += X.shape[0]

    def block(name, v, n):
        m, o, start, X, y = loads[name]
        Xs = X.clone() if v != "off" else X       # the masks go into a copy of the batch: one set of spans per block
        counter[0] += X.shape[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            with torch.cuda.stream(compute), using_config("train", True):
                if v != "off":
                    mask(Xs, v, advance=False)
                m.arena.data.copy_(start)
                loss = m.forward_loss(X=Xs, y=y, teach_ratio=bench.TRAIN["teach_ratio"], random_out=0, add_noise=bench.TRAIN["speech_noise"])
                m.cleargrads()
                loss.backward()
                o.update()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def call_alone(v, reps=200):
        """HIP-event time of `reps` back-to-back calls on fresh copies of the batch's values (the data does not matter to either fill's
        traffic: the zero fill reads nothing, the mean fill reads all of it), and the bytes the host model counts for those counters."""
        X = loads["cfg1"][3].clone()
        for _ in range(20):
            mask(X, v)
        first = counter[0]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            mask(X, v)
        e1.record()
        torch.cuda.synchronize()
        cells = 0
        for n in range(first, first + 32 * reps, 97):              # every 97th utterance: the mean masked share of an 800 x 80 utterance
            fs, ts = SA.spec_spans(SPEC["seed"], n, 80, 800, specs[v])
            mk = np.zeros((800, 80), bool)
            for f0, f in fs:
                mk[:, f0:f0 + f] = True
            for t0, t in ts:
                mk[t0:t0 + t] = True
            cells += int(mk.sum())
        share = cells / (len(range(first, first + 32 * reps, 97)) * 800 * 80)
        batch_bytes = X.numel() * 4
        return {"us": e0.elapsed_time(e1) / reps * 1e3, "masked_share": share, "bytes": batch_bytes * (share + (1.0 if v == "mean" else 0.0))}
    random.seed("seed-ast-20h")
    for name in loads:
        for v in variants:
            block(name, v, 10)
    alone = {v: call_alone(v) for v in variants if v != "off"}
    print("ready " + json.dumps(alone), flush=True)
    for line in sys.stdin:
        if line.strip() != "rep":
            break
        out = []
        for name in loads:
            for v in variants:
                out.append({"load": name, "variant": v, "ms": block(name, v, STEPS)})
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="the parent commit's libastk.so, in a checkout of that commit (DIR/ast_amd/libastk.so)")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--variants", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.variants.split(","))
    assert a.blocks >= 5

    def spawn(tree, variants, lib=None):
        env = dict(os.environ)
        if lib:
            env["ASTK_LIB_PATH"] = lib
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", tree, "--variants", variants], env=env, stdin=subprocess.PIPE,
                             stdout=subprocess.PIPE, text=True)
        line = p.stdout.readline()
        while line and not line.startswith("ready"):
            line = p.stdout.readline()
        assert line, "the child did not come up"
        return p, json.loads(line[len("ready"):])
    kids = {}
    kids["this"], alone = spawn(ROOT, "off,zero,mean")
    if a.parent_lib:
        lib = os.path.abspath(a.parent_lib)
        tree = os.path.dirname(os.path.dirname(lib))
        assert os.path.isdir(os.path.join(tree, "ast_amd")), "--parent-lib: expected DIR/ast_amd/libastk.so in a checkout of the parent commit"
        kids["parent"], _ = spawn(tree, "off", lib)
    t = {}
    for r in range(a.blocks):
        order = list(kids) if r % 2 == 0 else list(kids)[::-1]
        for k in order:
            kids[k].stdin.write("rep\n")
            kids[k].stdin.flush()
            for e in json.loads(kids[k].stdout.readline()):
                t.setdefault((e["load"], k, e["variant"]), []).append(e["ms"])
    for p in kids.values():
        p.stdin.write("quit\n")
        p.stdin.close()
        p.wait(timeout=60)
    for (load, k, v), ms in sorted(t.items()):
        ms = sorted(ms)
        med = ms[len(ms) // 2]
        print(f"{load:10s} {k:6s} {v:5s} median {med:7.3f} ms/step  spread {(ms[-1] - ms[0]) / med * 100:5.2f} %  blocks {[round(x, 3) for x in ms]}")
    for v, r in alone.items():
        print(f"astk_spec_augment alone, fill {v:5s}: {r['us']:7.2f} us per call on 32 x 800 x 80  masked share {r['masked_share']:.3f}  "
              f"{r['bytes'] / 1e6:5.2f} MB  {r['bytes'] / r['us'] / 1e3:7.1f} GB/s")


if __name__ == "__main__":
    main()
