"""What the auxiliary CTC loss costs per train step, on bench.py's two workloads (configs[1] and the shipped
es_en_20h model: the same configs, batch, optimizer and step as bench.py builds them).

    python scratch/ctc_cost.py --parent-lib DIR/ast_amd/libastk.so

One child process holds, per workload, a model without the head (the feature off: the step every model ran before) and one with
rnn_config.ctc, on this tree's library, and after a warm-up runs blocks of 50 steps ALTERNATING between the two (the second at
ctc_weight = 0.3); a second child runs the model without the head on another build of the library -- the parent commit's, built in a
checkout of its own (DIR) and driven by the parent's Python package beside it (DIR/ast_amd).  The children take turns block by block, so
that drift of the clocks hits both alike.  Reported per workload and variant: the median ms/step over the blocks, the blocks' spread
(max - min) / median, and the losses of the blocks' last steps (a sanity figure, no comparison).

The first child also times the CTC launches alone at each workload's shape with device events (200 calls behind a warm-up): the four
launches of astk_ctc_loss, and the head's product + astk_ctc_loss, against their byte floors -- the logits read once and dlogits written
once (2 B T'' V floats) for the operator, the logits written once more for the pair (3 B T'' V floats) -- at the HBM rate quoted in
the line.  The recursion itself is latency-bound: T'' serial steps of one workgroup per row."""
import argparse
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 50
WEIGHT = 0.3
HBM_TBS = 6.3          # achievable streaming rate the floors are quoted against (TB/s)


def child(tree, variants):
    sys.path.insert(0, tree)
    sys.path.append(ROOT)                                       # bench.py's configs (the same in both trees)
    import copy
    import ctypes as C
    import torch
    import bench
    from ast_amd import optimizers as O
    from ast_amd.seq2seq import SpeechEncoderDecoder, using_config
    compute = torch.cuda.Stream()
    loads = {}
    for name in ("cfg1", "es_en_20h"):
        for var in variants:
            cfg = copy.deepcopy(bench.MODEL_CFG)
            if name == "es_en_20h":
                cfg["rnn_config"]["dec_layers"] = 3
            if var == "on":
                cfg["rnn_config"]["ctc"] = True
            m = SpeechEncoderDecoder(0, cfg).materialize(80, seed=0)
            o = O.Adam(alpha=bench.TRAIN["lr"], beta1=0.9, beta2=0.999, eps=1e-8, amsgrad=True).setup(m)
            o.add_hook(O.WeightDecay(bench.TRAIN["l2"]))
            o.add_hook(O.GradientClipping(bench.TRAIN["grad_clip"]))
            Xh, yh = bench.synth_batch(32, 800, 80, 40, cfg["rnn_config"]["dec_vocab_size"], 20)
            loads[(name, var)] = (m, o, m.arena.data.clone(), torch.from_numpy(Xh).cuda(), torch.from_numpy(yh).cuda())

    def block(key, n):
        m, o, start, X, y = loads[key]
        kw = {"ctc_weight": WEIGHT} if key[1] == "on" else {}
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

    def launches_alone(key):
        """us per call of astk_ctc_loss, and of the head's product + astk_ctc_loss, at the workload's shape (device events)."""
        from ast_amd import _lib
        lib = _lib.load()
        m, _, _, X, y = loads[key]
        st = m._cur
        B, T2, V, L = st["B"], st["T2"], m.V, int(y.shape[1])
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        logits, Vp = m._ctc_logits(st, s)
        keep = logits.clone()
        d = _lib.CtcDesc(B, T2, V, Vp, L, L, 3, 0)
        ws = torch.empty(int(lib.astk_ctc_workspace_bytes(C.byref(d))), dtype=torch.uint8, device="cuda")
        nll, acc = torch.zeros(B, device="cuda"), torch.zeros(4, device="cuda")
        yd = y.to(torch.int32).contiguous()

        def op():
            _lib.check(lib.astk_ctc_loss(C.byref(d), logits.data_ptr(), yd.data_ptr(), None, WEIGHT / B, nll.data_ptr(), acc.data_ptr(),
                                         logits.data_ptr(), acc.data_ptr() + 8, ws.data_ptr(), ws.numel(), s))

        def timed(f, n=200):
            for _ in range(20):
                f()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                f()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / n * 1e3

        def op_fresh():                                         # (on logits, not on the gradient the call before left in their place)
            logits.copy_(keep)
            op()
        t_copy = timed(lambda: logits.copy_(keep))
        t_op = timed(op_fresh) - t_copy
        t_pair = timed(lambda: (m._ctc_logits(st, s), op()))
        fl = B * T2 * V * 4
        return {"load": key[0], "B": B, "T2": T2, "V": V, "L": L, "op_us": t_op, "op_floor_us": 2 * fl / (HBM_TBS * 1e12) * 1e6,
                "pair_us": t_pair, "pair_floor_us": 3 * fl / (HBM_TBS * 1e12) * 1e6}
    random.seed("seed-ast-20h")
    for key in loads:
        block(key, 10)
    alone = [launches_alone(k) for k in loads if k[1] == "on"]
    print("ready " + json.dumps(alone), flush=True)
    for line in sys.stdin:
        if line.strip() != "rep":
            break
        out = []
        for key in loads:
            ms, lv = block(key, STEPS)
            out.append({"load": key[0], "var": key[1], "ms": ms, "loss": lv})
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
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", tree, "--variants", variants], env=env,
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        line = p.stdout.readline()
        while line and not line.startswith("ready"):
            line = p.stdout.readline()
        assert line, "the child did not come up"
        return p, json.loads(line[len("ready"):])
    kids = {}
    kids["this"], alone = spawn(ROOT, "off,on")
    if a.parent_lib:
        lib = os.path.abspath(a.parent_lib)
        tree = os.path.dirname(os.path.dirname(lib))
        assert os.path.isdir(os.path.join(tree, "ast_amd")), "--parent-lib: expected DIR/ast_amd/libastk.so in a checkout of the parent commit"
        kids["parent"], _ = spawn(tree, "off", lib)
    t, losses = {}, {}
    for r in range(a.blocks):
        order = list(kids) if r % 2 == 0 else list(kids)[::-1]
        for k in order:
            kids[k].stdin.write("rep\n")
            kids[k].stdin.flush()
            for e in json.loads(kids[k].stdout.readline()):
                t.setdefault((e["load"], k, e["var"]), []).append(e["ms"])
                losses.setdefault((e["load"], k, e["var"]), set()).add(e["loss"])
    for p in kids.values():
        p.stdin.write("quit\n")
        p.stdin.close()
        p.wait(timeout=60)
    med = {}
    for (load, k, var), v in sorted(t.items()):
        v = sorted(v)
        med[(load, k, var)] = v[len(v) // 2]
        print(f"{load:10s} {k:6s} ctc {var:3s} median {med[(load, k, var)]:7.3f} ms/step  spread {(v[-1] - v[0]) / v[len(v) // 2] * 100:5.2f} %  "
              f"blocks {[round(x, 3) for x in v]}  last-step losses {min(losses[(load, k, var)]):.4f} .. {max(losses[(load, k, var)]):.4f}")
    for load in ("cfg1", "es_en_20h"):
        print(f"{load:10s} added by ctc_weight = {WEIGHT}: {med[(load, 'this', 'on')] - med[(load, 'this', 'off')]:+.3f} ms/step")
    for e in alone:
        print(f"{e['load']:10s} B {e['B']} T'' {e['T2']} V {e['V']} L {e['L']}: astk_ctc_loss {e['op_us']:.1f} us (floor {e['op_floor_us']:.2f} us at "
              f"{HBM_TBS} TB/s), head product + astk_ctc_loss {e['pair_us']:.1f} us (floor {e['pair_floor_us']:.2f} us)")


if __name__ == "__main__":
    main()
