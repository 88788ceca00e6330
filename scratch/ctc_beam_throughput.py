"""What the CTC prefix beam search costs, in one process:

    python scratch/ctc_beam_throughput.py

(a) The operator alone with device events at B = 32, T'' = 200, V = 1098: astk_ctc_beam at (N, C) = (5, 5), (16, 16) and (1, 1) -- the
    last one is the scan's fixed cost per frame: four barriers, the stay emission's read, the trie's probe -- beside astk_ctc_greedy on
    the same logits, ALTERNATING block by block (10 blocks of 20 calls each behind 20 warm-up calls each), so that drift of the clocks
    hits all alike.  Reported: the median over the blocks of the us per call, the blocks' spread (max - min) / median, and the byte
    floor at the HBM rate quoted in the line: the logits read once.
(b) Utterances/s on configs[1] with the CTC head, U = 32 utterances of T = 800 frames: the two-pass path -- ctc_beam (N = C = 5,
    max_labels = stop_limit - 1, so that no hypothesis is longer than the attention search's) on the padded batch, then
    rescore_ctc_nbest over the 160 hypotheses in packed calls of 32 rows -- against decode_beam_batch (N = K = 5, stop_limit 40),
    alternating block by block; the first pass alone is timed in blocks of its own."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T2, V = 32, 200, 1098
WIDTHS = [(5, 5), (16, 16), (1, 1)]
BLOCKS, CALLS, WARMUP = 10, 20, 20
U, N, K, T, STOP, WEIGHT = 32, 5, 5, 800, 40, 0.3
PATH_BLOCKS, PATH_CALLS = 7, 3
HBM_TBS = 6.3          # achievable streaming rate the floor is quoted against (TB/s)


def report(tag, v, unit):
    v = sorted(v)
    med = v[len(v) // 2]
    print(f"{tag:34s} median {med:9.1f} {unit}  spread {(v[-1] - v[0]) / med * 100:5.1f} %  blocks {[round(x, 1) for x in v]}")
    return med


def operator_alone():
    import numpy as np
    import torch
    from ast_amd import _lib
    lib = _lib.load()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Vp = (V + 3) // 4 * 4
    logits = torch.from_numpy(np.random.default_rng(0).standard_normal((B, T2, Vp)).astype(np.float32)).cuda()
    ops = {}
    keep = []
    for n, c in WIDTHS:
        d = _lib.CtcBeamDesc(B, T2, V, Vp, n, c, T2, 3, 0)
        need = int(lib.astk_ctc_beam_workspace_bytes(C.byref(d)))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        tok = torch.empty(B, n, T2, dtype=torch.int32, device="cuda")
        nl = torch.empty(B, n, dtype=torch.int32, device="cuda")
        sc = torch.empty(B, n, dtype=torch.float64, device="cuda")
        keep.append((d, ws, tok, nl, sc))
        ops[f"astk_ctc_beam N {n} C {c}"] = lambda d=d, ws=ws, tok=tok, nl=nl, sc=sc, need=need: _lib.check(lib.astk_ctc_beam(
            C.byref(d), logits.data_ptr(), None, tok.data_ptr(), nl.data_ptr(), sc.data_ptr(), ws.data_ptr(), need, s))
    gd = _lib.CtcDesc(B, T2, V, Vp, 1, 1, 3, 0)
    best = torch.empty(B, T2, dtype=torch.int32, device="cuda")
    ops["astk_ctc_greedy"] = lambda: _lib.check(lib.astk_ctc_greedy(C.byref(gd), logits.data_ptr(), None, best.data_ptr(), s))
    for f in ops.values():
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in ops}
    for r in range(BLOCKS):
        for k in (list(ops) if r % 2 == 0 else list(ops)[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                ops[k]()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) / CALLS * 1e3)
    for _, _, tok, nl, sc in keep:
        assert bool((nl[:, 0] > 0).all()) and bool(torch.isfinite(sc[:, 0]).all())
    print(f"(a) B {B} T'' {T2} V {V}: labels of the best string, per width: {[int(k[3][:, 0].float().mean()) for k in keep]} (mean over the rows)")
    for k, v in us.items():
        report(k, v, "us/call")
    print(f"byte floor (the logits read once, {B * T2 * V * 4 / 1e6:.1f} MB): {B * T2 * V * 4 / (HBM_TBS * 1e12) * 1e6:.2f} us at {HBM_TBS} TB/s")


def two_pass_against_the_attention_search():
    import copy
    import torch
    import bench
    from ast_amd import nn as gnn
    from ast_amd.seq2seq import SpeechEncoderDecoder
    cfg = copy.deepcopy(bench.MODEL_CFG)
    cfg["rnn_config"]["ctc"] = True
    Vm = cfg["rnn_config"]["dec_vocab_size"]
    m = SpeechEncoderDecoder(0, cfg).materialize(80, seed=0)
    Xh, _ = bench.synth_batch(U, T, 80, 40, Vm, 20)
    X = torch.from_numpy(Xh).cuda()
    Xs = [X[u:u + 1] for u in range(U)]
    lens = {}

    def first():
        return m.ctc_beam(X, N=N, C=N, max_labels=STOP - 1)

    def two_pass():
        nbest = first()
        out = gnn.rescore_ctc_nbest(m, Xs, nbest, WEIGHT, max_utts=U)
        lens["two"] = sum(len(e["hyp"]) for lst in out for e in lst) / sum(len(lst) for lst in out)
        return out

    def attention():
        out = gnn.decode_beam_batch(m, Xs, STOP, N, K)
        lens["att"] = sum(len(e["hyp"]) for lst in out for e in lst) / sum(len(lst) for lst in out)
        return out
    paths = {"ctc_beam alone": first, "ctc_beam + rescore_ctc_nbest": two_pass, "decode_beam_batch": attention}

    def block(f, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            f()
        torch.cuda.synchronize()
        return U * n / (time.perf_counter() - t0)
    for f in paths.values():
        block(f, 2)
    ups = {k: [] for k in paths}
    for r in range(PATH_BLOCKS):
        for k in (list(paths) if r % 2 == 0 else list(paths)[::-1]):
            ups[k].append(block(paths[k], PATH_CALLS))
    print(f"(b) U {U} T {T} N {N} C = K {K} stop_limit {STOP}, weight {WEIGHT}; mean hypothesis length: two-pass {lens['two']:.1f}, attention search {lens['att']:.1f} tokens")
    med = {k: report(k, v, "utt/s  ") for k, v in ups.items()}
    print(f"two-pass / attention search = {med['ctc_beam + rescore_ctc_nbest'] / med['decode_beam_batch']:.2f} x; ms per {U} utterances: "
          + ", ".join(f"{k} {U / v * 1e3:.2f}" for k, v in med.items()))


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "a timing needs the GPU"
    operator_alone()
    two_pass_against_the_attention_search()
