"""Forced decoding throughput (SpeechEncoderDecoder.score): the device loop (astk_forced_score, one persistent launch
per batch) without and with the alpha output, against the scored greedy loop with EOS never winning (the same loop with one more
dependency per step), eval-mode forward_loss (teach_ratio 1) and the per-step fallback (dec.persist = 0) -- one process, after a
warm-up, alternating within every repetition, each call timed to a device synchronise, the median of --reps per batch.

    python scratch/forced_throughput.py                       # both shapes, L = 40 and L = 176
    python scratch/forced_throughput.py --shape es_en_20h --L 176 --only alpha --batches 1 --reps 1    # for a rocprofv3 --kernel-trace pass

Models and batches are scratch/greedy_throughput.py's: BASELINE configs[1] and es_en_20h with random weights, the fisher_dev frame counts
in the loader's length buckets, --batches of them spread evenly over the plan; the dev pass is projected as their mean times the number of
batches.  Targets: ids in [1, V), a quarter of the positions PAD, column 0 = GO.

The routes above go through the Python wrappers: their per-step figure (batch time - the encoder pass) carries the host check and upload
of y, the read-back copies and -- with alpha -- the host-side transpose of S * B * T'' floats.  The routes `abi` and `abi_alpha` time
astk_forced_score alone (fill launch, encA product, the loop and, with alpha, k_alpha_normalise) on buffers allocated beforehand, to a
device synchronise, with no copy: that pair answers what the alpha output costs on the device."""
import argparse
import ctypes as C
import json
import time

import numpy as np
import torch

from greedy_throughput import EOS, GO, SHAPES, dev_plan, model, set_eos_bias, timed_encode
from ast_amd import _lib
from ast_amd.seq2seq import using_config


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def routes(m, only):
    def forced(alpha, persist):
        def go(X, y):
            with _lib.tuning({"dec.persist": persist}):
                r = m.score(X, y, return_alpha=alpha)
            assert m.last_score_path == ("device" if persist else "steps"), m.last_score_path
            return r.loss
        return go

    def greedy(X, y):
        r = m.predict_scored(X, GO, EOS, y.shape[1] - 1, y=y)
        assert m.last_predict_path == "device" and r.n_steps == y.shape[1] - 1
        return r.loss

    def fwd_loss(X, y):
        with using_config("train", False):
            return float(m.forward_loss(X, y, 1))

    def abi(alpha):
        def go(X, y):
            """encode and upload untimed; returns the seconds of the library call alone"""
            lib = _lib.load()
            with using_config("train", False):
                m._cur = None
                m.encode(X)
                m.init_decoder_state()
            st = m._cur
            B, S, T2 = st["B"], y.shape[1] - 1, st["T2"]
            yd = y.to(m.device, torch.int32).contiguous()
            out = torch.empty(4 + 3 * S * B, dtype=torch.int32, device=m.device)
            al = torch.empty(S * B * T2, dtype=torch.float32, device=m.device) if alpha else None
            ws = torch.empty(int(lib.astk_forced_workspace_bytes(C.byref(st["dd"]), S, int(alpha))), dtype=torch.uint8, device=m.device)
            assert ws.numel() > 0
            P = lambda t, off=0: None if t is None else C.c_void_p(t.data_ptr() + off)
            torch.cuda.synchronize()
            t = time.perf_counter()
            rc = lib.astk_forced_score(C.byref(st["dd"]), C.byref(st["dp"]), P(st["enc_states"]), P(m._dec_c), P(m._dec_h), P(yd), S + 1,
                                       P(out, 16), P(out, 16 + 4 * S * B), P(out, 16 + 8 * S * B), P(al), P(out), P(ws), ws.numel(), m._stream())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            assert rc == 0 and int(out[0]) == 0
            return dt
        return go
    all_ = {"abi": abi(False), "abi_alpha": abi(True), "forced": forced(False, 1), "alpha": forced(True, 1), "greedy_scored": greedy,
            "forward_loss": fwd_loss, "steps": forced(False, 0)}
    return {k: v for k, v in all_.items() if not only or k == only}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shape", default="", choices=[""] + list(SHAPES))
    ap.add_argument("--L", type=int, default=0, help="target length (default: 40 and 176)")
    ap.add_argument("--only", default="", choices=["", "abi", "abi_alpha", "forced", "alpha", "greedy_scored", "forward_loss", "steps"])
    a = ap.parse_args()
    plan = dev_plan()
    idx = np.linspace(0, len(plan) - 1, a.batches).round().astype(int) if a.batches > 1 else [len(plan) // 2]
    rng = np.random.default_rng(1)
    Xs = [torch.from_numpy(rng.standard_normal((plan[i][0], plan[i][1], 80)).astype(np.float32)).cuda() for i in idx]
    for name, shape in SHAPES.items():
        if a.shape and name != a.shape:
            continue
        m = model(shape, 0.0)
        set_eos_bias(m, -1e4)                        # the scored greedy loop runs every step
        run = routes(m, a.only)
        for L in ([a.L] if a.L else [40, 176]):
            ys = []
            for X in Xs:
                y = rng.integers(1, shape["V"], size=(X.shape[0], L)).astype(np.int32)
                y[rng.random(y.shape) < 0.25] = 0
                y[:, 0] = GO
                ys.append(torch.from_numpy(y))
            for X, y in zip(Xs, ys):                 # warm-up of every route on every shape
                for fn in run.values():
                    fn(X, y)
            t = {k: [[] for _ in Xs] for k in run}
            te, loss = [[] for _ in Xs], {}
            for _ in range(a.reps):
                for i, (X, y) in enumerate(zip(Xs, ys)):
                    for k, fn in run.items():
                        if k.startswith("abi"):
                            dt = fn(X, y)
                        else:
                            dt, loss[k, i] = timed(lambda: fn(X, y))
                        t[k][i].append(dt)
                    te[i].append(timed_encode(m, X))
            enc = np.array([np.median(v) for v in te])
            S = L - 1
            res = dict(shape=name, L=L, steps=S, reps=a.reps, frames=[int(X.shape[1]) for X in Xs], ms_encode=round(1e3 * float(enc.mean()), 3))
            for k, v in t.items():
                med = np.array([np.median(b) for b in v])
                res["ms_" + k] = round(1e3 * float(med.mean()), 3)
                res["us_per_step_" + k] = round(1e6 * float(((med if k.startswith("abi") else med - enc) / S).mean()), 2)
                res["spread_" + k] = round(float(np.mean([(max(b) - min(b)) / np.median(b) for b in v])), 3)
                res["pass_s_" + k] = round(len(plan) * float(med.mean()), 3)
            if "abi" in t and "abi_alpha" in t:
                res["ratio_abi_alpha_over_abi"] = round(res["us_per_step_abi_alpha"] / res["us_per_step_abi"], 3)
            if "forced" in t:
                for k in t:
                    if k != "forced" and not k.startswith("abi"):
                        res["ratio_per_step_" + k] = round(res["us_per_step_" + k] / res["us_per_step_forced"], 3)
            if "forced" in t and "forward_loss" in t:   # the forced loss of the last batch beside forward_loss's: the same number
                res["loss_forced"], res["loss_forward_loss"] = loss["forced", len(Xs) - 1], loss["forward_loss", len(Xs) - 1]
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
