"""What resampling and speed perturbation cost, in one process:

    python scratch/resample_cost.py

(a) astk_resample alone with device events at B = 32 on utterances of 8 s of rounded Gaussian noise (int16 in, float32 out): 9/10 and
    11/10 at 8 kHz, 2/1 (16 kHz to 8 kHz) and 441/80 (44.1 kHz to 8 kHz); beside each its byte floor (input samples + output floats at
    the HBM rate bench.py uses, 8000 GB/s).  ALTERNATING block by block behind a warm-up, the median over the blocks and their spread.
(b) resample + compute_device against compute_device alone (8 kHz MFCC-13, device tensors in and out), the same way.
(c) Wall clock of both against scipy.signal.resample_poly on the host (float64, one utterance at a time)."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_GBS = 8000.0
SECONDS, B, BLOCKS, CALLS, WARMUP = 8, 32, 10, 10, 5
RATIOS = (("9/10 (speed 0.9), 8 kHz", 9, 10, 8000), ("11/10 (speed 1.1), 8 kHz", 11, 10, 8000), ("2/1, 16 kHz to 8 kHz", 2, 1, 16000),
          ("441/80, 44.1 kHz to 8 kHz", 441, 80, 44100))


def report(tag, v, unit):
    v = sorted(v)
    med = v[len(v) // 2]
    print(f"{tag:56s} median {med:10.3f} {unit}  spread {(v[-1] - v[0]) / med * 100:5.1f} %  blocks {[round(x, 3) for x in v]}")
    return med


def alternate(calls, measure):
    """calls: {key: f}; BLOCKS rounds over all keys, the order reversed every other round; measure(f) -> one number."""
    out = {k: [] for k in calls}
    for r in range(BLOCKS):
        for k in (list(calls) if r % 2 == 0 else list(calls)[::-1]):
            out[k].append(measure(calls[k]))
    return out


def device_us(f):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / CALLS * 1e3


def main():
    import numpy as np
    import scipy.signal
    import torch
    import resample_model as RM
    from ast_amd import _lib
    from ast_amd import features as F
    lib = _lib.load()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1)
    cfg = F.FeatureConfig()
    ops, floors, outs, host_waves = {}, {}, {}, {}
    for tag, p, q, rate in RATIOS:
        n = rate * SECONDS
        host = np.clip(np.round(rng.standard_normal((B, n)) * 3000), -32768, 32767).astype(np.int16)
        wave = torch.from_numpy(host).cuda()
        ns = torch.full((B,), n, dtype=torch.int32, device="cuda")
        M = RM.n_out(n, p, q)
        d = _lib.ResampleDesc(B=B, Nmax=n, Mmax=M, sample_type=_lib.FEAT_SAMPLE_I16, p=p, q=q, num_zeros=6, rolloff=0.99)
        nbytes = int(lib.astk_resample_workspace_bytes(C.byref(d)))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        _lib.check(lib.astk_resample_prepare(C.byref(d), ws.data_ptr(), nbytes, s))
        Y = torch.empty(B, M, dtype=torch.float32, device="cuda")
        no = torch.empty(B, dtype=torch.int32, device="cuda")

        def op(d=d, wave=wave, ns=ns, Y=Y, no=no, ws=ws, nbytes=nbytes):
            _lib.check(lib.astk_resample(C.byref(d), wave.data_ptr(), ns.data_ptr(), Y.data_ptr(), no.data_ptr(), None, ws.data_ptr(), nbytes, s))
        ops[tag] = op
        floors[tag] = (wave.numel() * 2 + Y.numel() * 4) / (HBM_GBS * 1e9) * 1e6
        outs[tag] = (M, RM.constants(p, q))
        host_waves[tag] = (host, wave, ns, p, q)
    for f in ops.values():
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    us = alternate(ops, device_us)
    print(f"(a) astk_resample alone, B = {B}, {SECONDS} s per row, int16 in, float32 out")
    for tag, v in us.items():
        M, (P, Q, _, K) = outs[tag]
        med = report(f"astk_resample  [{tag}]", v, "us/launch")
        print(f"    {B * M} outputs of {2 * K} taps ({Q} phases); byte floor {floors[tag]:.2f} us: {med / floors[tag]:.1f} x; "
              f"{B * M * 2 * K / med * 1e-6:.2f} T multiply-adds/s")

    # (b) in front of the features
    host, wave, ns, p, q = host_waves[RATIOS[0][0]]

    def feats_alone():
        F.compute_device(wave, ns, cfg)

    def resample_and_feats():
        Y, no = F.resample(wave, ns, 9, 10)
        F.compute_device(Y, no, cfg)
    chain = {"compute_device alone (8 kHz mfcc-13)": feats_alone, "resample 9/10 + compute_device": resample_and_feats}
    for f in chain.values():
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    print(f"(b) in front of the features, B = {B}, {SECONDS} s per row, device tensors in and out (the Python layer's allocations included)")
    for tag, v in alternate(chain, device_us).items():
        report(tag, v, "us/call")

    # (c) wall clock against the host
    def wall_ms(f, per):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) / per * 1e3
    print(f"(c) wall clock per utterance of {SECONDS} s, synchronised; scipy.signal.resample_poly in float64 on the host, one utterance at a time")
    for tag, _, _, _ in RATIOS:
        host, wave, ns, p, q = host_waves[tag]

        def on_device(wave=wave, ns=ns, p=p, q=q):
            F.resample(wave, ns, p, q)
            torch.cuda.synchronize()

        def on_host(host=host, p=p, q=q):
            for b in range(4):
                scipy.signal.resample_poly(host[b].astype(np.float64), q, p)
        on_device()
        on_host()
        paths = {f"features.resample, {B} per launch  [{tag}]": (on_device, B), f"scipy resample_poly (host)      [{tag}]": (on_host, 4)}
        ms = {k: [] for k in paths}
        for r in range(5):
            for k in (list(paths) if r % 2 == 0 else list(paths)[::-1]):
                ms[k].append(wall_ms(*paths[k]))
        for k, v in ms.items():
            report(k, v, "ms/utt")


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "a timing needs the GPU"
    main()
