"""What label smoothing costs per train step, on bench.py's two workloads (configs[1] and the shipped es_en_20h
model: the same configs, batch, optimizer and step as bench.py builds them).

    python scratch/label_smoothing_cost.py --parent-lib DIR/ast_amd/libastk.so

One child process holds both models on this tree's library and, after a warm-up, runs blocks of 50 steps ALTERNATING between eps = 0 and
eps = 0.1; a second child does the same at eps = 0 on another build of the library -- the parent commit's, built in a checkout of its
own (DIR).  The decoder descriptor grew by the new field, so the parent's library is driven by the parent's Python package beside it
(DIR/ast_amd), not by this tree's.  The two children take turns block by block, so that drift of the clocks hits both alike.  Reported
per workload and variant: the median ms/step over the blocks, the blocks' spread (max - min) / median, and the losses of the blocks' last steps (every step
starts from the same parameters, but the teacher-forcing coins and the dropout draws move on from block to block: a sanity figure, no
comparison)."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 50


def child(tree, eps_list):
    sys.path.insert(0, tree)
    sys.path.append(ROOT)                                       # bench.py's configs (the same in both trees)
    import copy
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

    def block(name, eps, n):
        m, o, start, X, y = loads[name]
        kw = {"label_smoothing": eps} if eps else {}
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
        for eps in eps_list:
            block(name, eps, 10)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "rep":
            break
        out = []
        for name in loads:
            for eps in eps_list:
                ms, lv = block(name, eps, STEPS)
                out.append({"load": name, "eps": eps, "ms": ms, "loss": lv})
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="the parent commit's libastk.so, in a checkout of that commit (DIR/ast_amd/libastk.so)")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--eps", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, [float(e) for e in a.eps.split(",")])
    assert a.blocks >= 5

    def spawn(tree, eps, lib=None):
        env = dict(os.environ)
        if lib:
            env["ASTK_LIB_PATH"] = lib
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", tree, "--eps", eps], env=env, stdin=subprocess.PIPE,
                             stdout=subprocess.PIPE, text=True)
        line = p.stdout.readline()
        while line and line.strip() != "ready":
            line = p.stdout.readline()
        assert line, "the child did not come up"
        return p
    kids = {"this": spawn(ROOT, "0,0.1")}
    if a.parent_lib:
        lib = os.path.abspath(a.parent_lib)
        tree = os.path.dirname(os.path.dirname(lib))
        assert os.path.isdir(os.path.join(tree, "ast_amd")), "--parent-lib: expected DIR/ast_amd/libastk.so in a checkout of the parent commit"
        kids["parent"] = spawn(tree, "0", lib)
    t, losses = {}, {}
    for r in range(a.blocks):
        order = list(kids) if r % 2 == 0 else list(kids)[::-1]
        for k in order:
            kids[k].stdin.write("rep\n")
            kids[k].stdin.flush()
            for e in json.loads(kids[k].stdout.readline()):
                t.setdefault((e["load"], k, e["eps"]), []).append(e["ms"])
                losses.setdefault((e["load"], k, e["eps"]), set()).add(e["loss"])
    for p in kids.values():
        p.stdin.write("quit\n")
        p.stdin.close()
        p.wait(timeout=60)
    for (load, k, eps), v in sorted(t.items()):
        v = sorted(v)
        med = v[len(v) // 2]
        print(f"{load:10s} {k:6s} eps {eps:<4} median {med:7.3f} ms/step  spread {(v[-1] - v[0]) / med * 100:5.2f} %  blocks {[round(x, 3) for x in v]}  "
              f"last-step losses {min(losses[(load, k, eps)]):.4f} .. {max(losses[(load, k, eps)]):.4f}")


if __name__ == "__main__":
    main()
