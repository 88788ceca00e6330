"""Every host-side branch of decoder.hip on ONE library (chosen by ASTK_LIB_PATH), results to an .npz.

    ASTK_LIB_PATH=<parent's libastk.so> python3 scratch/decoder_paths_dump.py parent.npz
    ASTK_LIB_PATH=<result's libastk.so> python3 scratch/decoder_paths_dump.py result.npz
    python3 scratch/decoder_paths_dump.py --compare parent.npz result.npz
    python3 scratch/decoder_paths_dump.py --compare-traces PARENT_TRACE_DIR RESULT_TRACE_DIR

Each case runs astk_decoder_fwd_ex and astk_decoder_bwd with `deterministic` = 1 and saves loss, pred, d_enc, d_c0, d_h0 and every gradient
tensor.  The forward is bit-reproducible by design and `deterministic` makes the backward so: two libraries that issue the same launches
with the same arguments write equal files, and --compare wants every array of every case bit-equal (numpy.array_equal).  The same job under
`rocprofv3 --kernel-trace` (program behind `--`, no counters) gives the ordered launch lists to compare."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SMALL, EXTRA = (5, 9, 23, 64, 16, 32, 57, 1, False), (4, 6, 12, 64, 16, 64, 57, 2, True)
# name: ((B, L, T, H, E, A, V, nl, masks), tuning knobs, options)
CASES = {
    "persist_1layer": (SMALL, {}, ()),
    "persist_3layers": ((19, 8, 37, 128, 32, 64, 130, 3, True), {}, ()),
    "persist_b6_split_0": ((17, 5, 60, 256, 64, 128, 300, 1, False), {"dec.b6_split": 0}, ()),
    "persist_b6_fused_0": ((17, 5, 60, 256, 64, 128, 300, 1, False), {"dec.b6_fused": 0}, ()),
    "row_split": ((37, 5, 50, 512, 128, 512, 300, 1, False), {}, ()),
    "wide": ((9, 6, 30, 1024, 128, 1024, 300, 1, False), {}, ()),
    "steps_device_flags": ((5, 9, 23, 32, 12, 24, 57, 3, True), {}, ()),
    "steps_host_flags": ((5, 9, 23, 32, 12, 24, 57, 3, True), {}, ("host_flags",)),
    "steps_persist_off_host_flags": (SMALL, {"dec.persist": 0}, ("host_flags",)),
    "steps_ln": (EXTRA, {}, ("ln",)),
    "steps_two_heads": (EXTRA, {}, ("n_attn2",)),
    "steps_no_feed_attn": (EXTRA, {}, ("no_feed",)),
    "steps_out_mask": (EXTRA, {}, ("out_mask",)),
    "phases_chain_then_params": (SMALL, {}, ("phases",)),
}


def run_case(lib, G, torch, shape, opts):
    B, L, T, H, E, A, V, nl, masks = shape
    s = G._dec_setup(lib, B, L, T, H, E, A, V, nl, masks, seed=B + L)
    d, dp, dg, S = s["d"], s["dp"], s["dg"], s["S"]
    gen = torch.Generator(device="cpu").manual_seed(B * L + T)
    extra = {}                                          # parameters the optional features add, and their gradients

    def param(name, *shape_, scale=0.1, shift=0.0):
        extra[name] = (torch.randn(*shape_, generator=gen) * scale + shift).cuda()
        extra["d_" + name] = torch.zeros_like(extra[name])
        return extra[name].data_ptr(), extra["d_" + name].data_ptr()
    if "ln" in opts:
        d.ln = 1
        for l in range(nl):
            dp.ln_gamma[l], dg.d_ln_gamma[l] = param(f"ln_gamma{l}", H, shift=1.0)
            dp.ln_beta[l], dg.d_ln_beta[l] = param(f"ln_beta{l}", H)
    if "n_attn2" in opts:
        d.n_attn = 2
        dp.Wa_x[0], dg.dWa_x[0] = param("Wa1", H, H)
        dp.ba_x[0], dg.dba_x[0] = param("ba1", H)
        dp.Wc, dg.dWc = param("Wc3", A, 3 * H)         # context/W over [cv_0; cv_1; h]
    if "no_feed" in opts:
        d.no_feed_attn = 1                              # (layer 0 reads the first 4H * E floats of its (4H, E + A) weight as (4H, E))
    d.deterministic = 1
    host = (C.c_int32 * S)(*[int(f) for f in s["flags"]])
    if "host_flags" in opts:
        d.use_truth_host = C.cast(host, C.POINTER(C.c_int32))
    om = (torch.rand(S, B, V, generator=gen) < 0.8).float().cuda() * 1.25 if "out_mask" in opts else None
    nbytes = lib.astk_decoder_workspace_bytes(C.byref(d))
    ws = G.GuardedWS(nbytes)
    dev, vp, st = G.dev, G.vp, G.stream
    enc_d, c0_d, h0_d = dev(s["enc"]), dev(s["c0"]), dev(s["h0"])
    y_d, fl_d = dev(s["y"], torch.int32), dev(np.asarray(s["flags"]), torch.int32)
    em_d, rm_d = (dev(s["em"]) if masks else None), (dev(s["rm"]) if masks else None)
    loss_d, pred_d = torch.zeros(1, device="cuda"), torch.zeros(S, B, dtype=torch.int32, device="cuda")
    d_enc = torch.zeros(B, T, H, device="cuda")
    d_c0, d_h0 = torch.zeros(nl, B, H, device="cuda"), torch.zeros(nl, B, H, device="cuda")
    G.ok(lib, lib.astk_decoder_fwd_ex(C.byref(d), C.byref(dp), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), vp(fl_d), vp(em_d), vp(rm_d), vp(om), None,
                                      vp(loss_d), vp(pred_d), vp(ws), nbytes, st()))
    for phase in ((1, 2) if "phases" in opts else (0,)):   # ASTK_DEC_BWD_CHAIN, then ASTK_DEC_BWD_PARAMS; or ASTK_DEC_BWD_ALL
        G.ok(lib, lib.astk_decoder_bwd_phase_ex(C.byref(d), C.byref(dp), C.byref(dg), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), vp(em_d), vp(rm_d),
                                                vp(om), vp(d_enc), vp(d_c0), vp(d_h0), vp(ws), nbytes, phase, st()))
    ws.check("decoder_paths_dump")
    out = {"path": np.int64(lib.astk_decoder_path(C.byref(d))), "loss": loss_d, "pred": pred_d, "d_enc": d_enc, "d_c0": d_c0, "d_h0": d_h0}
    out.update({"grad " + k: v for k, v in s["grd"].items()})
    out.update({k: v for k, v in extra.items() if k.startswith("d_")})
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def run_step_infer(lib, G, torch):
    B, L, T, H, E, A, V, nl = 4, 5, 12, 16, 8, 16, 23, 2
    s = G._dec_setup(lib, B, L, T, H, E, A, V, nl, False, seed=5)
    nbytes = lib.astk_decoder_workspace_bytes(C.byref(s["d"]))
    ws = G.GuardedWS(nbytes)
    dev, vp = G.dev, G.vp
    enc_d, c, h = dev(s["enc"]), dev(s["c0"]), dev(s["h0"])
    ht, tok = torch.zeros(B, A, device="cuda"), dev(s["y"][:, 0], torch.int32)
    logits, alpha = torch.zeros(B, V, device="cuda"), torch.zeros(B, T, device="cuda")
    am = torch.zeros(B, dtype=torch.int32, device="cuda")
    G.ok(lib, lib.astk_decoder_step_infer(C.byref(s["d"]), C.byref(s["dp"]), vp(enc_d), vp(c), vp(h), vp(ht), vp(tok), vp(logits), vp(alpha),
                                          vp(am), vp(ws), nbytes, G.stream()))
    ws.check("step_infer")
    return {k: v.cpu().numpy() for k, v in dict(c=c, h=h, ht=ht, logits=logits, alpha=alpha, argmax=am).items()}


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files)) + [k for k in a.files if k in b.files and not np.array_equal(a[k], b[k])]
    print(f"{len(a.files)} arrays in {a_path}, {len(b.files)} in {b_path}: " + ("all bit-equal" if not bad else f"{len(bad)} DIFFER: {bad}"))
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
    a, b = launches(a_dir), launches(b_dir)
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
    print(f"{len(a)} launches in {a_dir}, {len(b)} in {b_dir}: " + ("equal line for line" if first is None else f"DIFFER from launch {first}: "
                                                                     f"{a[first:first + 3]} / {b[first:first + 3]}"))
    return 0 if first is None else 1


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
        print(f"{name}: path {int(res['path'])}, loss {float(res['loss'][0]):.6f}", flush=True)
        out.update({f"{name}/{k}": v for k, v in res.items()})
    out.update({f"step_infer/{k}": v for k, v in run_step_infer(lib, G, torch).items()})
    np.savez(sys.argv[1], **out)
    print(f"wrote {len(out)} arrays to {sys.argv[1]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
