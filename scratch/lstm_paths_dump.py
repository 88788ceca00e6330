"""Every host-side branch of lstm.hip on ONE library (chosen by ASTK_LIB_PATH), results to an .npz.

    ASTK_LIB_PATH=<parent's libastk.so> python3 scratch/lstm_paths_dump.py parent.npz
    ASTK_LIB_PATH=<result's libastk.so> python3 scratch/lstm_paths_dump.py result.npz
    python3 scratch/lstm_paths_dump.py --compare parent.npz result.npz
    python3 scratch/lstm_paths_dump.py --compare-traces PARENT_TRACE_DIR RESULT_TRACE_DIR

Each case runs astk_lstm_stack_fwd and astk_lstm_stack_bwd (or _bwd_on) and saves the path, the side plan, enc_states, cT, hT, dx and every
gradient tensor.  The forward is bit-reproducible by design and `deterministic` = 1 makes the backward so: two libraries that issue the same
launches with the same arguments write equal files, and --compare wants every array of every case bit-equal (numpy.array_equal).  The
side-stream cases cannot be deterministic -- the mode keeps everything in line -- so their backward arrays (split tiles added in any
order) are saved under "unordered/" names, for which --compare prints the largest difference and asks nothing; they are compared by the bits
of the forward and by the launch lists.  The same job under `rocprofv3 --kernel-trace` (program behind `--`, no counters) gives those
lists: --compare-traces wants the ordered (kernel, grid, block) list of every stream equal, the streams taken in order of first use."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SIDE = (70, 33, 16, 64, 3, True)
# name: ((T, B, in_dim, h, nl, masks), tuning knobs, options)
CASES = {
    "per_step": ((9, 5, 24, 20, 3, True), {}, ()),
    "per_step_persist_off": ((5, 17, 16, 64, 2, True), {"lstm.persist": 0}, ()),
    "persist_one_group": ((12, 5, 24, 64, 3, True), {}, ()),
    "persist_groups_2_1": ((5, 200, 16, 64, 3, False), {}, ()),
    "persist_groups_2_2_2": ((4, 20, 24, 512, 6, False), {}, ()),
    "hoisted": ((9, 19, 24, 1024, 3, True), {}, ()),
    "rows32_1": ((23, 33, 16, 64, 3, False), {"lstm.rows32": 1}, ()),
    "rows32_2": ((23, 33, 16, 64, 3, False), {"lstm.rows32": 2}, ()),
    "side_fwd_chunks": (SIDE, {"lstm.overlap_chunk": 4}, ("side",)),
    "side_bwd_every_chunk": (SIDE, {"lstm.overlap_chunk": 4, "lstm.side_bwd": -1}, ("side",)),
    "side_bwd_two_chunks": (SIDE, {"lstm.overlap_chunk": 4, "lstm.side_bwd": 2}, ("side",)),
    "one_direction": ((7, 33, 16, 128, 2, True), {}, ("one_dir",)),
    "one_direction_per_step": ((7, 5, 12, 20, 2, True), {}, ("one_dir",)),
    "one_step": ((1, 3, 8, 64, 2, True), {}, ()),
    "no_dx": ((12, 5, 24, 64, 3, True), {}, ("no_dx",)),
    "no_dx_per_step": ((9, 5, 24, 20, 3, True), {}, ("no_dx",)),
    "own_recurrence_stream": ((12, 5, 24, 64, 3, True), {}, ("bwd_on",)),
    "own_recurrence_stream_hoisted": ((3, 4, 16, 1024, 2, False), {}, ("bwd_on",)),
}


def run_case(lib, G, torch, shape, opts):
    import range_cases
    from ast_amd._lib import LstmGrads, LstmParams, LstmStackDesc
    T, B, in_dim, h, nl, masks = shape
    nd = 1 if "one_dir" in opts else 2
    c = range_cases.lstm_draws(T, B, in_dim, h, nl, masks)
    names = c["names"][:nd * nl]
    d = LstmStackDesc(T, B, in_dim, h, nl, nd)
    d.deterministic = 0 if "side" in opts else 1
    main = torch.cuda.Stream()
    keep = [main]
    if "side" in opts:
        keep.append(G._concurrent_stream(lib, main))
        d.side_stream = keep[-1].cuda_stream
    st = C.c_void_p(main.cuda_stream)
    dev, vp = G.dev, G.vp
    prm = {k: dev(v) for k, v in c["P"].items() if k.split("/")[0] in names}
    grd = {k: torch.zeros_like(v) for k, v in prm.items()}
    lp, lg = (LstmParams * (nd * nl))(), (LstmGrads * (nd * nl))()
    for i, n in enumerate(names):
        lp[i].Wu, lp[i].b, lp[i].Wl = (prm[n + s].data_ptr() for s in ("/upward/W", "/upward/b", "/lateral/W"))
        lg[i].dWu, lg[i].db, lg[i].dWl = (grd[n + s].data_ptr() for s in ("/upward/W", "/upward/b", "/lateral/W"))
    nbytes = lib.astk_lstm_stack_workspace_bytes(C.byref(d))
    ws = G.GuardedWS(nbytes)
    xd, md = dev(c["x"]), (dev(c["mk"][:nd]) if masks else None)
    enc = torch.zeros(B, T, nd * h, device="cuda")
    cT, hT = torch.zeros(nd, nl, B, h, device="cuda"), torch.zeros(nd, nl, B, h, device="cuda")
    dx = None if "no_dx" in opts else torch.zeros(T, B, in_dim, device="cuda")
    ge, gc, gh = dev(c["g_enc"][:, :, :nd * h]), dev(c["g_c"][:nd]), dev(c["g_h"][:nd])
    plan = [C.c_int(), C.c_int(), C.c_int()]
    G.ok(lib, lib.astk_lstm_stack_side_plan(C.byref(d), *[C.byref(p) for p in plan]))
    torch.cuda.synchronize()
    G.ok(lib, lib.astk_lstm_stack_fwd(C.byref(d), lp, vp(xd), vp(md), vp(enc), vp(cT), vp(hT), vp(ws), nbytes, st))
    if "bwd_on" in opts:
        keep.append(torch.cuda.Stream())
        G.ok(lib, lib.astk_lstm_stack_bwd_on(C.byref(d), lp, lg, vp(xd), vp(md), vp(ge), vp(gc), vp(gh), vp(dx), vp(ws), nbytes, st,
                                             C.c_void_p(keep[-1].cuda_stream)))
    else:
        G.ok(lib, lib.astk_lstm_stack_bwd(C.byref(d), lp, lg, vp(xd), vp(md), vp(ge), vp(gc), vp(gh), vp(dx), vp(ws), nbytes, st))
    torch.cuda.synchronize()
    ws.check("lstm_paths_dump")
    status = C.c_uint(0)
    assert lib.astk_persist_status(C.byref(status), 1) == 0 and status.value == 0, status.value
    out = {"path": np.int64(lib.astk_lstm_stack_path(C.byref(d))), "side_plan": np.array([p.value for p in plan]),
           "free_cus": np.int64(lib.astk_lstm_stack_free_cus(C.byref(d))), "workspace_bytes": np.int64(nbytes), "enc_states": enc, "cT": cT, "hT": hT}
    back = {"grad " + k: v for k, v in grd.items()}
    if dx is not None:
        back["dx"] = dx
    out.update({("unordered/" if "side" in opts else "") + k: v for k, v in back.items()})
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    exact = lambda k: "/unordered/" not in k                            # noqa: E731
    bad = sorted(set(a.files) ^ set(b.files)) + [k for k in a.files if k in b.files and exact(k) and not np.array_equal(a[k], b[k])]
    loose = [float(np.abs(a[k].astype(np.float64) - b[k]).max() / max(np.abs(a[k]).max(), 1e-30)) for k in a.files if k in b.files and not exact(k)]
    print(f"{len(a.files)} arrays in {a_path}, {len(b.files)} in {b_path}: {len(a.files) - len(loose)} to compare bit for bit: "
          + ("all bit-equal" if not bad else f"{len(bad)} DIFFER: {bad}")
          + (f"; {len(loose)} unordered sums (side-stream backward), largest difference {max(loose):.2e} of the array's maximum" if loose else ""))
    return 1 if bad else 0


def compare_traces(a_dir, b_dir):
    """The ordered (kernel name, grid, block) lists of two `rocprofv3 --kernel-trace --output-format csv -d DIR` runs of this job, stream by
    stream: the launches of two streams that run beside each other start in an order that differs from run to run."""
    import csv
    import glob

    def launches(d):
        rows = [r for p in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True) for r in csv.DictReader(open(p))]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        dims = [k for k in rows[0] if k.startswith(("Grid_Size", "Workgroup_Size"))]
        streams = {}                                                     # in order of first use
        for r in rows:
            streams.setdefault(r.get("Stream_Id", "0"), []).append((r["Kernel_Name"],) + tuple(r[k] for k in dims))
        return list(streams.values())
    a, b = launches(a_dir), launches(b_dir)
    bad = len(a) != len(b)
    print(f"{len(a)} streams with {sum(map(len, a))} launches in {a_dir}, {len(b)} with {sum(map(len, b))} in {b_dir}")
    for i, (x, y) in enumerate(zip(a, b)):
        first = next((j for j, (p, q) in enumerate(zip(x, y)) if p != q), None if len(x) == len(y) else min(len(x), len(y)))
        print(f"  stream {i}: {len(x)} / {len(y)} launches: " + ("equal line for line" if first is None else f"DIFFER from launch {first}: "
                                                                 f"{x[first:first + 3]} / {y[first:first + 3]}"))
        bad = bad or first is not None
    return 1 if bad else 0


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3])
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
        res = run_case(lib, G, torch, shape, opts)
        for k, v in prev.items():
            lib.astk_set_tuning(k.encode(), v.value)
        print(f"{name}: path {int(res['path'])}, side plan {res['side_plan'].tolist()}, |enc| {float(np.abs(res['enc_states']).sum()):.6f}", flush=True)
        out.update({f"{name}/{k}": v for k, v in res.items()})
    np.savez(sys.argv[1], **out)
    print(f"wrote {len(out)} arrays to {sys.argv[1]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
