"""What joint CTC-attention decoding costs in the batched beam search, on configs[1] with the CTC head:
U = 32 utterances of T = 800 frames, N = K = 5, stop_limit = 40.

    python scratch/joint_beam_throughput.py --parent-lib DIR/ast_amd/libastk.so

One child process holds the model on this tree's library and, after a warm-up, runs blocks of decode_beam_batch calls ALTERNATING
between ctc_weight = 0 (the search every model ran before: the same code path as the parent's) and ctc_weight = 0.3; a second child
runs the plain search on another build of the library -- the parent commit's, built in a checkout of its own (DIR) and driven by the
parent's Python package beside it (DIR/ast_amd).  The children take turns block by block, so that drift of the clocks hits both alike.
Reported per variant: the median utterances/s over the blocks and the blocks' spread (max - min) / median.

The first child also times, with device events at the search's shape (R = 160 rows of prefixes of 10 labels, K = 5, T'' = 200,
V = 1098): the prefix-score launch of a step in its shipped form (a wavefront per candidate) beside the plain serial form (a thread
per candidate; libastk_test.so) and the shipped kernel reading its emission columns strided from the head's (U, T'', ldv) logits
instead of the init's (U, V, T'') copy, in the same call, against the bytes the scores must move -- the slots' states read once, the
candidates' states written K-fold and gathered for the N kept slots, the emission columns gathered -- at the HBM rate quoted in the
line; and the three init launches of a search."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = 3
WEIGHT = 0.3
U, N, K, T, STOP = 32, 5, 5, 800, 40
HBM_TBS = 6.3          # achievable streaming rate the floor is quoted against (TB/s)


def child(tree, variants):
    sys.path.insert(0, tree)
    sys.path.append(ROOT)                                       # bench.py's configs (the same in both trees)
    import copy
    import ctypes as C
    import numpy as np
    import torch
    import bench
    from ast_amd import nn as gnn
    from ast_amd.seq2seq import SpeechEncoderDecoder
    cfg = copy.deepcopy(bench.MODEL_CFG)
    cfg["rnn_config"]["ctc"] = True
    V = cfg["rnn_config"]["dec_vocab_size"]
    m = SpeechEncoderDecoder(0, cfg).materialize(80, seed=0)
    Xh, _ = bench.synth_batch(U, T, 80, 40, V, 20)
    Xs = [torch.from_numpy(Xh[u:u + 1]).cuda() for u in range(U)]

    def block(var, n):
        kw = {"ctc_weight": WEIGHT} if var == "w03" else ({"ctc_weight": 0.0} if var == "w0" else {})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out = gnn.decode_beam_batch(m, Xs, STOP, N, K, **kw)
        torch.cuda.synchronize()
        return U * n / (time.perf_counter() - t0), out[0][0]["score"]

    def timed(f, n):
        for _ in range(5):
            f()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n * 1e3

    def launches_alone():
        from ast_amd import _lib as L
        R, T2 = U * N, 200
        rng = np.random.default_rng(0)
        dev = "cuda"
        i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
        lens = np.full(U, T2, np.int32)
        st = dict(row_utt=torch.arange(R, **i32) // N, row_len=torch.full((R,), T2, **i32), c=torch.zeros(1, R, 8, device=dev),
                  h=torch.zeros(1, R, 8, device=dev), ht=torch.zeros(R, 8, device=dev), tokens=torch.full((R,), 1, **i32),
                  score=torch.zeros(R, **f64), status=torch.ones(R, **i32), frozen=torch.zeros(U, **i32), n_frozen=torch.zeros(1, **i32),
                  hist=torch.zeros(1, R, 4, **i32), hist_alpha=torch.zeros(1, R, T2, device=dev))
        bd = L.BeamDesc(U, N, K, 1, T2, V, 2, lens.ctypes.data_as(C.POINTER(C.c_int32)))
        bs = L.BeamState(*[st[k].data_ptr() for k in ("row_utt", "row_len", "c", "h", "ht", "tokens", "score", "status", "frozen", "n_frozen",
                                                      "hist", "hist_alpha")])
        Vp = (V + 3) // 4 * 4
        logits = torch.randn(U, T2, Vp, device=dev)
        state, att, psi, nlab = torch.zeros(R, T2, 2, **f64), torch.zeros(R, **f64), torch.zeros(R, **f64), torch.zeros(R, **i32)
        bc = L.BeamCtc(WEIGHT, 0, 3, logits.data_ptr(), Vp, state.data_ptr(), att.data_ptr(), psi.data_ptr(), nlab.data_ptr(), None, 0)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        with L.load_test_hooks() as lib:
            ws = torch.zeros(int(lib.astk_beam_ctc_workspace_bytes(C.byref(bd), C.byref(bc))), dtype=torch.uint8, device=dev)
            bc.ws, bc.ws_bytes = ws.data_ptr(), ws.numel()
            t_init = timed(lambda: L.check(lib.astk_beam_ctc_init(C.byref(bd), C.byref(bs), C.byref(bc), s)), 20)
            state[:] = state[::N].repeat_interleave(N, 0)          # every slot: the empty prefix, then 10 labels through the scorer itself
            out_psi, out_state = torch.zeros(R, K, **f64), torch.zeros(R, K, T2, 2, **f64)
            for _ in range(10):
                cand = torch.from_numpy(rng.integers(3, V, size=(R, K)).astype(np.int32)).cuda()
                L.check(lib.astk_debug_ctc_prefix(C.byref(bd), C.byref(bs), C.byref(bc), cand.data_ptr(), 0, out_psi.data_ptr(),
                                                  out_state.data_ptr(), s))
                state.copy_(out_state[:, 0])
                st["tokens"].copy_(cand[:, 0])
                nlab += 1
            t = [timed(lambda f=form: L.check(lib.astk_debug_ctc_prefix(C.byref(bd), C.byref(bs), C.byref(bc), cand.data_ptr(), f,
                                                                         out_psi.data_ptr(), out_state.data_ptr(), s)), 100) for form in (0, 1, 2)]
        moved = R * T2 * 16 + R * K * T2 * 16 + 2 * R * T2 * 16 + R * K * T2 * 4
        return {"R": R, "K": K, "T2": T2, "V": V, "wave_us": t[0], "serial_us": t[1], "strided_us": t[2], "bytes": moved,
                "floor_us": moved / (HBM_TBS * 1e12) * 1e6, "init_us": t_init, "psi_finite": bool(torch.isfinite(out_psi).all())}
    for var in variants:
        block(var, 1)
    alone = launches_alone() if "w03" in variants else {}
    for var in variants:                                        # (a full block of each behind the launch timings: the first one runs slow)
        block(var, CALLS)
    print("ready " + json.dumps(alone), flush=True)
    for line in sys.stdin:
        if line.strip() != "rep":
            break
        out = []
        for var in variants:
            ups, sc = block(var, CALLS)
            out.append({"var": var, "ups": ups, "score": sc})
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
    kids["this"], alone = spawn(ROOT, "w0,w03")
    if a.parent_lib:
        lib = os.path.abspath(a.parent_lib)
        tree = os.path.dirname(os.path.dirname(lib))
        assert os.path.isdir(os.path.join(tree, "ast_amd")), "--parent-lib: expected DIR/ast_amd/libastk.so in a checkout of the parent commit"
        kids["parent"], _ = spawn(tree, "plain", lib)
    t, scores = {}, {}
    for r in range(a.blocks):
        order = list(kids) if r % 2 == 0 else list(kids)[::-1]
        for k in order:
            kids[k].stdin.write("rep\n")
            kids[k].stdin.flush()
            for e in json.loads(kids[k].stdout.readline()):
                t.setdefault((k, e["var"]), []).append(e["ups"])
                scores.setdefault((k, e["var"]), set()).add(e["score"])
    for p in kids.values():
        p.stdin.write("quit\n")
        p.stdin.close()
        p.wait(timeout=60)
    for (k, var), v in sorted(t.items()):
        v = sorted(v)
        print(f"{k:6s} {var:5s} median {v[len(v) // 2]:8.2f} utt/s  spread {(v[-1] - v[0]) / v[len(v) // 2] * 100:5.2f} %  "
              f"blocks {[round(x, 2) for x in v]}  best scores {sorted(scores[(k, var)])}")
    e = alone
    print(f"prefix scores of a step, R {e['R']} K {e['K']} T'' {e['T2']} V {e['V']}: wavefront per candidate {e['wave_us']:.1f} us, thread per "
          f"candidate {e['serial_us']:.1f} us, wavefront per candidate with the emissions read strided from the head's layout {e['strided_us']:.1f} us; {e['bytes'] / 1e6:.2f} MB to move = {e['floor_us']:.2f} us at {HBM_TBS} TB/s; "
          f"init (3 launches, once per search) {e['init_us']:.1f} us; all psi finite: {e['psi_finite']}")


if __name__ == "__main__":
    main()
