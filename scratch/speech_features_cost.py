"""What the speech features cost, in one process:

    python scratch/speech_features_cost.py

(a) astk_speech_features alone with device events, on utterances of 8 s of rounded Gaussian noise: 8 kHz MFCC-13 and 16 kHz fbank-80 at
    B = 32, and 8 kHz MFCC-13 at B = 1; beside each its byte floor (input samples + output floats at the HBM rate bench.py uses, 8000
    GB/s) and a launch of astk_cmvn_apply on the result.  ALTERNATING block by block behind a warm-up, the median over the blocks and
    their spread.
(b) Wall clock of features.compute + cmvn per utterance (host lists in, device tensors out, synchronised) against the float64 NumPy
    model of tests/speech_features_model.py on the host, at 8 kHz MFCC-13."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_GBS = 8000.0
SECONDS, BLOCKS, CALLS, WARMUP = 8, 10, 10, 5


def report(tag, v, unit):
    v = sorted(v)
    med = v[len(v) // 2]
    print(f"{tag:52s} median {med:10.3f} {unit}  spread {(v[-1] - v[0]) / med * 100:5.1f} %  blocks {[round(x, 3) for x in v]}")
    return med


def operator_alone():
    import numpy as np
    import torch
    from ast_amd import _lib
    from ast_amd.features import FeatureConfig
    lib = _lib.load()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1)
    shapes = (("8 kHz mfcc-13, B 32", FeatureConfig(), 32), ("16 kHz fbank-80, B 32", FeatureConfig(kind="fbank", sample_frequency=16000.0, num_mel_bins=80), 32),
              ("8 kHz mfcc-13, B 1", FeatureConfig(), 1))
    calls = {}
    for tag, cfg, B in shapes:
        n = int(cfg.sample_frequency) * SECONDS
        wave = torch.from_numpy(np.clip(np.round(rng.standard_normal((B, n)) * 3000), -32768, 32767).astype(np.int16)).cuda()
        ns = torch.full((B,), n, dtype=torch.int32, device="cuda")
        Fmax = cfg.frames(n)
        d = cfg.descriptor(B, n, Fmax, _lib.FEAT_SAMPLE_I16)
        nbytes = int(lib.astk_speech_features_workspace_bytes(C.byref(d)))
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        _lib.check(lib.astk_speech_features_prepare(C.byref(d), ws.data_ptr(), nbytes, s))
        X = torch.empty(B, Fmax, cfg.dim, dtype=torch.float32, device="cuda")
        nf = torch.empty(B, dtype=torch.int32, device="cuda")
        group = torch.arange(B, dtype=torch.int32, device="cuda")
        stats = torch.zeros(B, 2, cfg.dim + 1, dtype=torch.float64, device="cuda")
        cd = _lib.CmvnDesc(B=B, Fmax=Fmax, D=cfg.dim, G=B, norm_vars=1)
        Y = torch.empty_like(X)

        def feat(d=d, wave=wave, ns=ns, X=X, nf=nf, ws=ws, nbytes=nbytes):
            _lib.check(lib.astk_speech_features(C.byref(d), wave.data_ptr(), ns.data_ptr(), X.data_ptr(), nf.data_ptr(), None, ws.data_ptr(), nbytes, s))

        def apply(cd=cd, X=X, Y=Y, nf=nf, group=group, stats=stats):
            _lib.check(lib.astk_cmvn_apply(C.byref(cd), X.data_ptr(), Y.data_ptr(), nf.data_ptr(), group.data_ptr(), stats.data_ptr(), s))

        def accumulate(cd=cd, X=X, nf=nf, group=group, stats=stats):
            _lib.check(lib.astk_cmvn_accumulate(C.byref(cd), X.data_ptr(), nf.data_ptr(), group.data_ptr(), stats.data_ptr(), None, s))
        feat()
        accumulate()
        floor_us = (wave.numel() * 2 + X.numel() * 4) / (HBM_GBS * 1e9) * 1e6
        frames = B * Fmax
        calls[tag] = dict(feat=feat, apply=apply, accumulate=accumulate, floor_us=floor_us, frames=frames,
                          apply_floor_us=2 * X.numel() * 4 / (HBM_GBS * 1e9) * 1e6)
    us = {(tag, k): [] for tag in calls for k in ("feat", "apply", "accumulate")}
    for (tag, k) in us:
        for _ in range(WARMUP):
            calls[tag][k]()
    torch.cuda.synchronize()
    for r in range(BLOCKS):
        for key in (list(us) if r % 2 == 0 else list(us)[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                calls[key[0]][key[1]]()
            b.record()
            b.synchronize()
            us[key].append(a.elapsed_time(b) / CALLS * 1e3)
    for tag, c in calls.items():
        print(f"(a) {tag}: {c['frames']} frames of {SECONDS} s utterances; byte floor {c['floor_us']:.2f} us (cmvn_apply: {c['apply_floor_us']:.2f} us)")
        med = report(f"astk_speech_features  [{tag}]", us[tag, "feat"], "us/launch")
        print(f"    {med / c['floor_us']:.0f} x its byte floor, {med * 1e3 / c['frames']:.1f} ns per frame, {c['frames'] / med:.2f} M frames/s")
        report(f"astk_cmvn_apply       [{tag}]", us[tag, "apply"], "us/launch")
        report(f"astk_cmvn_accumulate  [{tag}]", us[tag, "accumulate"], "us/launch")


def against_the_host_model():
    import numpy as np
    import torch
    import speech_features_model as SM
    from ast_amd import features as F
    rng = np.random.default_rng(2)
    cfg, mcfg, U = F.FeatureConfig(), SM.config(), 32
    waves = [np.clip(np.round(rng.standard_normal(8000 * SECONDS) * 3000), -32768, 32767).astype(np.int16) for _ in range(U)]

    def device(batch):
        def f():
            for lo in range(0, U, batch):
                X, nf = F.compute(waves[lo:lo + batch], cfg, "cuda")
                F.cmvn(X, nf)
            torch.cuda.synchronize()
        return f

    def host():
        for w in waves[:4]:
            x = SM.features(w, mcfg).astype(np.float32)[None]
            n = np.asarray([x.shape[1]])
            st, _ = SM.cmvn_stats(x, n, [0], 1)
            SM.cmvn_apply(x, n, [0], st, True)
    paths = {"features.compute + cmvn, 32 per launch": (device(32), U), "features.compute + cmvn, 1 per launch": (device(1), U),
             "NumPy float64 model (host)": (host, 4)}
    for f, _ in paths.values():
        f()
    ms = {k: [] for k in paths}
    for r in range(5):
        for k in (list(paths) if r % 2 == 0 else list(paths)[::-1]):
            t0 = time.perf_counter()
            paths[k][0]()
            ms[k].append((time.perf_counter() - t0) / paths[k][1] * 1e3)
    print(f"(b) {U} utterances of {SECONDS} s at 8 kHz, mfcc-13, per-utterance CMVN; wall clock, host lists in, synchronised")
    for k, v in ms.items():
        report(k, v, "ms/utt")


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "a timing needs the GPU"
    operator_alone()
    against_the_host_model()
