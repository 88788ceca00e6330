"""Every host-side branch of conv.hip on ONE library (chosen by ASTK_LIB_PATH), results to an .npz.

    ASTK_LIB_PATH=<parent's libastk.so> python3 scratch/cnn_paths_dump.py parent.npz
    ASTK_LIB_PATH=<parent's libastk.so> python3 scratch/cnn_paths_dump.py parent_again.npz
    ASTK_LIB_PATH=<result's libastk.so> python3 scratch/cnn_paths_dump.py result.npz
    python3 scratch/cnn_paths_dump.py --compare parent.npz result.npz [parent_again.npz]
    python3 scratch/cnn_paths_dump.py --compare-traces PARENT_TRACE_DIR RESULT_TRACE_DIR

Each case draws its inputs with tests/range_cases.py cnn_draws and runs, on a fresh workspace: the training forward, the backward with
`deterministic` = 1 (options below add to that), then the evaluation forward; it saves both outputs, the running statistics of every layer
and every dW / dgamma / dbeta / dbias.  --compare with the parent's second run: an array the parent reproduces bit for bit between its
own two runs must be bit-equal in the result; one it does not reproduce (the training statistics end in double atomics) must lie within
the parent's own two-run difference -- both numbers are printed.  Without the third file every array must be bit-equal.  The same job under
`rocprofv3 --kernel-trace` (program behind `--`, no counters) gives the launch lists: --compare-traces wants the ordered
(kernel, grid, block) lists equal.  Everything runs on one stream."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHIPPED = (2, 170, 26, [(16, 9, 13, 2, 13, 4), (8, 9, 1, 2, 1, 4)])
C64 = (2, 50, 80, [(64, 9, 13, 2, 13, 4)])
# name: ((B, T, D, layers), tuning knobs, options).  Options: "f32" / "fp16x2" = the descriptor's precision (fp16x2 with the scaled terms on
# every size: the operand-maximum slots are read); ("pool", windows); "no_bn"; "sync" = the _sync entry points with world = 2 and an
# exchange that doubles the sums in place on the stream; "eval_only"; ("rows", frame counts) = astk_conv_bn_relu_fwd_rows; "bwd_twice" = a
# second backward call on the one forward (the fill in the place of the clean mark); "noise".
CASES = {
    "shipped_direct": (SHIPPED, {}, ("noise",)),
    "shipped_direct0_off": (SHIPPED, {"conv.direct0": 0}, ("noise",)),
    "shipped_f32": (SHIPPED, {}, ("f32",)),
    "shipped_fp16x2": (SHIPPED, {}, ("fp16x2",)),
    "c64_tiled_seq": (C64, {}, ()),
    "c64_seq_fwd_off": (C64, {"conv.seq_fwd": 0}, ()),
    "c64_seq_bwd_off": (C64, {"conv.seq_bwd": 0}, ()),
    "c64_both_off": (C64, {"conv.seq_fwd": 0, "conv.seq_bwd": 0}, ()),
    "f10_c64_last": ((2, 45, 80, [(16, 5, 8, 2, 8, 2), (64, 3, 1, 1, 1, 1)]), {}, ()),
    "f20_kf4_untiled_by_shape": ((2, 30, 80, [(16, 5, 4, 2, 4, 2), (8, 3, 1, 2, 1, 1)]), {}, ()),
    "thirteen_phases_flush": ((2, 60, 20, [(4, 4, 5, 1, 3, 0), (4, 13, 1, 13, 1, 0)]), {}, ()),
    "four_layers": ((2, 120, 26, [(16, 9, 13, 2, 13, 4), (8, 9, 1, 2, 1, 4), (8, 4, 1, 3, 1, 0), (4, 5, 1, 2, 1, 2)]), {}, ()),
    "pooled_layer0": ((3, 42, 80, [(16, 9, 13, 2, 13, 4), (8, 9, 1, 2, 1, 4)]), {}, (("pool", [[2, 1], [1, 1]]),)),
    "pooled_layer1": ((2, 76, 80, [(16, 9, 13, 2, 13, 4), (8, 9, 1, 2, 1, 4)]), {}, (("pool", [[1, 1], [3, 2]]),)),
    "pooled_last_c64": ((2, 76, 80, [(16, 9, 13, 2, 13, 4), (64, 9, 1, 2, 1, 4)]), {}, (("pool", [[1, 1], [2, 1]]),)),
    "no_bn_biases": (SHIPPED, {}, ("no_bn",)),
    "no_bn_im2col": (SHIPPED, {"conv.direct0": 0}, ("no_bn",)),
    "sync_world2_direct": (SHIPPED, {}, ("sync",)),
    "sync_world2_im2col_c64": (C64, {"conv.direct0": 0}, ("sync",)),
    "sync_world2_no_bn": (SHIPPED, {}, ("sync", "no_bn")),
    "eval_alone_direct": (SHIPPED, {}, ("eval_only",)),
    "eval_alone_im2col": (SHIPPED, {}, ("eval_only", "f32")),
    "rows_ragged": ((3, 170, 26, SHIPPED[3]), {}, (("rows", [170, 93, 41]),)),
    "rows_ragged_c64": ((3, 50, 80, C64[3]), {}, (("rows", [17, 50, 9]),)),
    "bwd_twice": (SHIPPED, {}, ("bwd_twice",)),
    "bwd_twice_c64": (C64, {}, ("bwd_twice",)),
}


def run_case(lib, G, torch, shape, opts):
    import range_cases
    from ast_amd import _lib
    from ast_amd._lib import CnnLayerGrads, CnnLayerParams
    B, T, D, layers = shape
    opt = {(o if isinstance(o, str) else o[0]): (True if isinstance(o, str) else o[1]) for o in opts}
    cfg, P, X, noise, rng = range_cases.cnn_draws(B, T, D, None, None, "noise" in opt, layers=layers, pool=opt.get("pool"))
    n = len(layers)
    cd = G._cnn_desc(cfg, B, T, D)
    cd.deterministic = 1
    cd.no_bn = 1 if "no_bn" in opt else 0
    cd.precision = _lib.PREC_F32 if "f32" in opt else _lib.PREC_FP16X2 if "fp16x2" in opt else _lib.PREC_DEFAULT
    for i, (wt, wf) in enumerate(opt.get("pool", [])):
        cd.pool_t[i], cd.pool_f[i] = wt, wf
    t2, f2, feat = C.c_int(), C.c_int(), C.c_int()
    G.ok(lib, lib.astk_conv_bn_relu_out_dims(C.byref(cd), C.byref(t2), C.byref(f2), C.byref(feat)))
    dev, vp, st = G.dev, G.vp, G.stream()
    names = [f"CNN_{i}" for i in range(n)]
    prm = {k + s: dev(P[k + s]) for k in names for s in ("/W", "_bn/gamma", "_bn/beta", "_bn/avg_mean", "_bn/avg_var")}
    prm.update({k + "/b": dev(0.3 * rng.standard_normal(P[k + "_bn/beta"].shape)) for k in names})
    grd = {k: torch.zeros_like(v) for k, v in prm.items() if "avg" not in k}
    cp, cg = (CnnLayerParams * n)(), (CnnLayerGrads * n)()
    for i, k in enumerate(names):
        cp[i].W, cp[i].gamma, cp[i].beta, cp[i].bias = (prm[k + s].data_ptr() for s in ("/W", "_bn/gamma", "_bn/beta", "/b"))
        cp[i].avg_mean, cp[i].avg_var = prm[k + "_bn/avg_mean"].data_ptr(), prm[k + "_bn/avg_var"].data_ptr()
        cg[i].dW, cg[i].dgamma, cg[i].dbeta, cg[i].dbias = (grd[k + s].data_ptr() for s in ("/W", "_bn/gamma", "_bn/beta", "/b"))
    nbytes = lib.astk_conv_bn_relu_workspace_bytes(C.byref(cd))
    ws = G.GuardedWS(nbytes)
    out = torch.zeros(t2.value, B, feat.value, device="cuda")
    xd, nd = dev(X), (dev(noise) if noise is not None else None)
    g = dev(rng.standard_normal(out.shape))
    res = {"workspace_bytes": np.int64(nbytes)}
    calls = [0]

    def exchange(user, stat, cnt, stream):          # in place, on the stream the library launches on (the current one)
        off = int(stat) - ws.t.data_ptr()
        assert 0 <= off and off + 8 * cnt <= nbytes and int(stream or 0) == int(st.value or 0)
        ws.t[off:off + 8 * cnt].view(torch.float64).mul_(2.0)
        calls[0] += 1
        return 0
    cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)(exchange)

    def fwd(train):
        if "sync" in opt:
            G.ok(lib, lib.astk_conv_bn_relu_fwd_sync(C.byref(cd), cp, vp(xd), vp(nd), vp(out), vp(ws), nbytes, train, cb, None, 2, st))
        else:
            G.ok(lib, lib.astk_conv_bn_relu_fwd(C.byref(cd), cp, vp(xd), vp(nd), vp(out), vp(ws), nbytes, train, st))
        ws.check("cnn_paths_dump fwd")
        return out.cpu().numpy()

    def bwd(tag):
        for v in grd.values():
            v.zero_()
        if "sync" in opt:
            G.ok(lib, lib.astk_conv_bn_relu_bwd_sync(C.byref(cd), cp, cg, vp(g), vp(ws), nbytes, cb, None, 2, st))
        else:
            G.ok(lib, lib.astk_conv_bn_relu_bwd(C.byref(cd), cp, cg, vp(g), vp(ws), nbytes, st))
        ws.check("cnn_paths_dump bwd")
        res.update({f"{tag} {k}": v.cpu().numpy() for k, v in grd.items()})

    if "rows" in opt:
        Xp = X.copy()
        for b, m in enumerate(opt["rows"]):
            Xp[b, m:] = 0.0
        xd, rl = dev(Xp), torch.tensor(opt["rows"], dtype=torch.int32, device="cuda")
        out_len = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        G.ok(lib, lib.astk_conv_bn_relu_fwd_rows(C.byref(cd), cp, vp(xd), vp(rl), vp(out), vp(out_len), vp(ws), nbytes, st))
        ws.check("cnn_paths_dump rows")
        res.update({"out rows": out.cpu().numpy(), "out_len": out_len.cpu().numpy()})
        return res
    if "eval_only" not in opt:
        res["out train"] = fwd(1)
        res.update({"after train " + k: v.cpu().numpy() for k, v in prm.items() if "avg" in k})
        bwd("grad")
        if "bwd_twice" in opt:
            bwd("grad again")
    res["out eval"] = fwd(0)
    res["exchange_calls"] = np.int64(calls[0])
    return res


def compare(a_path, b_path, a2_path=None):
    a, b = np.load(a_path), np.load(b_path)
    a2 = np.load(a2_path) if a2_path else None
    diff = lambda x, y: float(np.abs(x.astype(np.float64) - y).max()) if x.size else 0.0      # noqa: E731
    bad = sorted(set(a.files) ^ set(b.files))
    n_exact = 0
    for k in a.files:
        if k not in b.files:
            continue
        if a2 is None or np.array_equal(a[k], a2[k]):
            n_exact += 1
            if not np.array_equal(a[k], b[k]):
                bad.append(k)
                print(f"  DIFFERS {k}: parent against result {diff(a[k], b[k]):.3e} (the parent reproduces it bit for bit)")
        else:
            own, res = diff(a[k], a2[k]), diff(a[k], b[k])
            print(f"  not reproduced by the parent: {k}: parent against itself {own:.3e}, parent against result {res:.3e}")
            if res > own:
                bad.append(k)
    print(f"{len(a.files)} arrays in {a_path}, {len(b.files)} in {b_path}: {n_exact} to compare bit for bit, {len(a.files) - n_exact} within the "
          f"parent's own difference: " + ("all as wanted" if not bad else f"{len(bad)} NOT: {bad}"))
    return 1 if bad else 0


def compare_traces(a_dir, b_dir):
    """The ordered (kernel name, grid, block) lists of two `rocprofv3 --kernel-trace --output-format csv -d DIR` runs of this job."""
    import csv
    import glob

    def launches(d):
        rows = [r for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(p))]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        dims = [k for k in rows[0] if k.startswith(("Grid_Size", "Workgroup_Size"))]
        return [(r["Kernel_Name"],) + tuple(r[k] for k in dims) for r in rows]
    x, y = launches(a_dir), launches(b_dir)
    first = next((j for j, (p, q) in enumerate(zip(x, y)) if p != q), None if len(x) == len(y) else min(len(x), len(y)))
    print(f"{len(x)} launches in {a_dir}, {len(y)} in {b_dir}: " + ("equal line for line" if first is None else
                                                                    f"DIFFER from launch {first}: {x[first:first + 3]} / {y[first:first + 3]}"))
    return 0 if first is None else 1


def main():
    if len(sys.argv) in (4, 5) and sys.argv[1] == "--compare":
        return compare(*sys.argv[2:])
    if len(sys.argv) == 4 and sys.argv[1] == "--compare-traces":
        return compare_traces(sys.argv[2], sys.argv[3])
    import torch
    import test_gpu_ops as G
    from ast_amd import _lib
    lib = _lib.load()
    print("library:", _lib.LIB_PATH)
    out = {}
    for name, (shape, knobs, opts) in CASES.items():
        prev = {}
        for k, v in knobs.items():
            prev[k] = C.c_double()
            assert lib.astk_get_tuning(k.encode(), C.byref(prev[k])) == 0 and lib.astk_set_tuning(k.encode(), float(v)) == 0, k
        below = lib.astk_set_gemm_bf16_split_below(C.c_double(0.0 if "fp16x2" in opts else 3e9))
        try:
            res = run_case(lib, G, torch, shape, opts)
        finally:
            lib.astk_set_gemm_bf16_split_below(C.c_double(below))
            for k, v in prev.items():
                lib.astk_set_tuning(k.encode(), v.value)
        status = C.c_uint(0)
        assert lib.astk_persist_status(C.byref(status), 1) == 0 and status.value == 0, status.value
        key = next(k for k in ("out train", "out eval", "out rows") if k in res)
        print(f"{name}: {len(res)} arrays, |{key}| {float(np.abs(res[key]).sum()):.6f}", flush=True)
        out.update({f"{name}/{k}": v for k, v in res.items()})
    np.savez(sys.argv[1], **out)
    print(f"wrote {len(out)} arrays to {sys.argv[1]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
