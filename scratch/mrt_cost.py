"""What the per-row loss weights and a minimum-risk training step cost, on bench.py's two workloads (configs[1]
and the shipped es_en_20h model: the same configs, batch, optimizer and step as bench.py builds them).

    python scratch/mrt_cost.py --parent-lib DIR/ast_amd/libastk.so

(a), (b): one child process holds both models on this tree's library and, after a warm-up, runs blocks of 50 steps ALTERNATING between
row_weight=None and a weight vector (cycling 0.25, 2, 1, 0.5); a second child runs the plain step on another build of the library --
the parent commit's, built in a checkout of its own (DIR), driven by the parent's Python package beside it.  The two children take
turns block by block, so that drift of the clocks hits both alike.  Reported per workload and variant: the median ms/step over the
blocks and the blocks' spread (max - min) / median.  The comparison is only ever between the figures of ONE call of this script.
(c): one MRT step of the es_en_20h model at U 4, N 7 (32 rows; X 4 x 800 frames, references of 40 tokens), split by synchronising into
sampling, batch building on the host, pair statistics + astk_risk_weights, and the weighted train step; and astk_risk_weights alone
(100 launches between two synchronisations) beside its byte floor at 8 TB/s.  The plain step of the same 4 utterances is timed beside
it: the weighted step runs encoder and decoder on N + 1 = 8 times the rows."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 50
HBM_BYTES_PER_S = 8e12


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
        rw = torch.tensor([(0.25, 2.0, 1.0, 0.5)[b % 4] for b in range(32)], dtype=torch.float32, device="cuda")
        loads[name] = (m, o, m.arena.data.clone(), torch.from_numpy(Xh).cuda(), torch.from_numpy(yh).cuda(), rw)

    def block(name, variant, n):
        m, o, start, X, y, rw = loads[name]
        kw = {"row_weight": rw} if variant == "weighted" else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            with torch.cuda.stream(compute), using_config("train", True):
                m.arena.data.copy_(start)
                loss = m.forward_loss(X=X, y=y, teach_ratio=bench.TRAIN["teach_ratio"], random_out=0, add_noise=bench.TRAIN["speech_noise"], **kw)
                m.cleargrads()
                loss.backward()
                o.update()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt / n * 1e3, float(loss)
    random.seed("seed-ast-20h")
    for name in loads:
        for v in variants:
            block(name, v, 10)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "rep":
            break
        out = []
        for name in loads:
            for v in variants:
                ms, lv = block(name, v, STEPS)
                out.append({"load": name, "variant": v, "ms": ms, "loss": lv})
        print(json.dumps(out), flush=True)
    if line.strip() == "mrt":
        print(json.dumps(mrt_parts(loads["es_en_20h"])), flush=True)


def mrt_parts(load, U=4, N=7, reps=7):
    """(c): the parts of one MRT step, medians over `reps` steps that all start from the same parameters."""
    import numpy as np
    import torch
    from ast_amd import mrt
    from ast_amd.eval import pair_stats
    from ast_amd.seq2seq import using_config
    m, o, start, X, y, _ = load
    X, yh = X[:U].contiguous(), y[:U].cpu().numpy()
    cfg = mrt.checked_mrt({"samples": N, "alpha": 1.0, "cost": "bleu", "mle_weight": 0.5, "seed": 3})
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t = {k: [] for k in ("sample", "build", "stats+weights", "weighted step", "plain step U rows", "risk_weights alone us")}

    def clock(key, f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        t[key].append((time.perf_counter() - t0) * 1e3)
        return r
    for rep in range(reps + 1):
        m.arena.data.copy_(start)
        samples, scores, _ = clock("sample", lambda: mrt.draw_samples(m, X, N, mrt.mrt_max_len(cfg, yh.shape[1]), cfg, rep * U * N))
        b = clock("build", lambda: mrt.build_mrt_batch(samples, yh))
        R = len(b["flags"])
        s = np.zeros(R, np.float32)
        s[b["flags"] != mrt.REFERENCE] = scores.reshape(-1)
        rs, rw = mrt.mrt_scales(cfg["mle_weight"], R, U)

        def weights():
            stats, lens, pairs = pair_stats(b["pool"], b["pairs"], return_device=True)
            dev = (up(b["first"]), up(s), stats, lens, pairs, up(b["flags"]))
            return dev, mrt.risk_weights(*dev, "bleu", 1.0, rs, rw)[0]
        dev, w = clock("stats+weights", weights)

        def step(Xs, ys, **kw):
            with using_config("train", True):
                loss = m.forward_loss(X=Xs, y=ys, teach_ratio=1.0, random_out=0, **kw)
                m.cleargrads()
                loss.backward()
                o.update()
        clock("weighted step", lambda: step(X.repeat_interleave(N + 1, dim=0), up(b["y"]), row_weight=w))
        m.arena.data.copy_(start)
        clock("plain step U rows", lambda: step(X, y[:U]))
        clock("risk_weights alone us", lambda: [mrt.risk_weights(*dev, "bleu", 1.0, rs, rw) for _ in range(100)])
        t["risk_weights alone us"][-1] *= 10.0                  # ms per 100 launches -> us per launch
    out = {k: sorted(v[1:])[len(v[1:]) // 2] for k, v in t.items()}      # (the first repetition warms up)
    nbytes = 4 * (U + 1) + R * (4 + 32 + 8 + 4 + 4) + 2 * R * 4 + 4 * U
    out["risk_weights bytes"] = nbytes
    out["risk_weights byte floor us"] = nbytes / HBM_BYTES_PER_S * 1e6
    out["rows"] = R
    return out


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
        while line and line.strip() != "ready":
            line = p.stdout.readline()
        assert line, "the child did not come up"
        return p
    kids = {"this": spawn(ROOT, "plain,weighted")}
    if a.parent_lib:
        lib = os.path.abspath(a.parent_lib)
        tree = os.path.dirname(os.path.dirname(lib))
        assert os.path.isdir(os.path.join(tree, "ast_amd")), "--parent-lib: expected DIR/ast_amd/libastk.so in a checkout of the parent commit"
        kids["parent"] = spawn(tree, "plain", lib)
    t, losses = {}, {}
    for r in range(a.blocks):
        order = list(kids) if r % 2 == 0 else list(kids)[::-1]
        for k in order:
            kids[k].stdin.write("rep\n")
            kids[k].stdin.flush()
            for e in json.loads(kids[k].stdout.readline()):
                t.setdefault((e["load"], k, e["variant"]), []).append(e["ms"])
                losses.setdefault((e["load"], k, e["variant"]), set()).add(e["loss"])
    kids["this"].stdin.write("mrt\n")
    kids["this"].stdin.flush()
    parts = json.loads(kids["this"].stdout.readline())
    for k, p in kids.items():
        if k != "this":
            p.stdin.write("quit\n")
        p.stdin.close()
        p.wait(timeout=60)
    for (load, k, v), ms in sorted(t.items()):
        ms = sorted(ms)
        med = ms[len(ms) // 2]
        print(f"{load:10s} {k:6s} {v:8s} median {med:7.3f} ms/step  spread {(ms[-1] - ms[0]) / med * 100:5.2f} %  blocks {[round(x, 3) for x in ms]}  "
              f"last-step losses {min(losses[(load, k, v)]):.4f} .. {max(losses[(load, k, v)]):.4f}")
    print("one MRT step, es_en_20h, U 4, N 7 (medians, ms unless named):")
    for k, v in parts.items():
        print(f"  {k:28s} {v:10.3f}")


if __name__ == "__main__":
    main()
