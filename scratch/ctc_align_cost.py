"""What a CTC forced alignment costs beside the CTC loss, operator against operator on the same logits:

    python scratch/ctc_align_cost.py

Per shape -- section 28's (B = 32, T'' = 200, V = 1098, L = 40) and the largest shipped one (T'' = 353, L = 175) -- one process times
astk_ctc_align alone and astk_ctc_loss alone with device events, ALTERNATING block by block (10 blocks of 20 calls each = 200 calls per
operator, behind 20 warm-up calls each), so that drift of the clocks hits both alike.  Reported: the median over the blocks of the us
per call, the blocks' spread (max - min) / median, and the alignment's byte floor at the HBM rate quoted in the line: the logits read
once (the lse pass; the row kernel's gathers touch a subset of the same lines) and the back-pointers written and read once.  Every row
carries L - 2 labels (GO and EOS are no labels), the longest recursion the shape admits.  The loss writes its gradient to a buffer of
its own here, so both operators read the same untouched logits in every call."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(32, 200, 1098, 40), (32, 353, 1098, 175)]          # (B, T'', V, L)
BLOCKS, CALLS, WARMUP = 10, 20, 20
HBM_TBS = 6.3          # achievable streaming rate the floor is quoted against (TB/s)


def main():
    import numpy as np
    import torch
    from ast_amd import _lib
    lib = _lib.load()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for B, T, V, L in SHAPES:
        rng = np.random.default_rng(T + L)
        Vp = (V + 3) // 4 * 4
        logits = torch.from_numpy(rng.standard_normal((B, T, Vp)).astype(np.float32)).cuda()
        y = rng.integers(3, V, size=(B, L)).astype(np.int32)
        y[:, 0], y[:, -1] = 1, 2
        yd = torch.from_numpy(y).cuda()
        d = _lib.CtcDesc(B, T, V, Vp, L, L, 3, 0)
        need_a, need_l = int(lib.astk_ctc_align_workspace_bytes(C.byref(d))), int(lib.astk_ctc_workspace_bytes(C.byref(d)))
        ws_a = torch.empty(need_a, dtype=torch.uint8, device="cuda")
        ws_l = torch.empty(need_l, dtype=torch.uint8, device="cuda")
        i32 = dict(dtype=torch.int32, device="cuda")
        fs, fc, l0, l1 = torch.empty(B, T, **i32), torch.empty(B, T, **i32), torch.empty(B, L, **i32), torch.empty(B, L, **i32)
        lp, score, nll = torch.empty(B, L, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        dlogits = torch.empty_like(logits)

        def align():
            _lib.check(lib.astk_ctc_align(C.byref(d), logits.data_ptr(), yd.data_ptr(), None, fs.data_ptr(), fc.data_ptr(), l0.data_ptr(),
                                          l1.data_ptr(), lp.data_ptr(), score.data_ptr(), None, ws_a.data_ptr(), need_a, s))

        def loss():
            _lib.check(lib.astk_ctc_loss(C.byref(d), logits.data_ptr(), yd.data_ptr(), None, 1.0, nll.data_ptr(), None, dlogits.data_ptr(), None,
                                         ws_l.data_ptr(), need_l, s))
        ops = {"astk_ctc_align": align, "astk_ctc_loss": loss}
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
        assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(nll).all()) and bool((score <= -nll + 1e-3 * nll.abs()).all())
        W = (2 * L + 1 + 63) // 64
        floor = (B * T * V * 4 + 2 * B * T * W * 16) / (HBM_TBS * 1e12) * 1e6
        med = {}
        for k, v in us.items():
            v = sorted(v)
            med[k] = v[len(v) // 2]
            print(f"B {B} T'' {T} V {V} L {L}: {k:15s} median {med[k]:7.1f} us/call  spread {(v[-1] - v[0]) / med[k] * 100:5.1f} %  "
                  f"blocks {[round(x, 1) for x in v]}")
        print(f"B {B} T'' {T} V {V} L {L}: align / loss = {med['astk_ctc_align'] / med['astk_ctc_loss']:.2f}; the alignment's byte floor "
              f"{floor:.2f} us at {HBM_TBS} TB/s (logits {B * T * V * 4 / 1e6:.1f} MB, back-pointers 2 x {B * T * W * 16 / 1e6:.2f} MB); "
              f"workspaces {need_a / 1e6:.2f} MB against the loss's {need_l / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
