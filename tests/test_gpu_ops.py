"""GPU parity tests, operator level: every C-ABI entry point of include/astk.h against a float64 CPU reference
(torch autograd restatement in oracle/ast_ref_torch.py, itself cross-checked against oracle/ast_ref.py).
Tolerances: float32 kernels vs float64 reference -> relative 2e-4 on tensors (north_star: 1e-4 on loss /
grad-norm, asserted in test_gpu_model.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import range_cases
from conftest import tiny_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


@pytest.fixture(params=["bf16x3", "fp16x2", "f32"])
def gemm_split(request, lib):
    """Every operator test runs under the three arithmetic schemes of the f32-accurate products (include/astk.h): "bf16x3" = the
    library's default (three bf16 terms, exact operands), "f32" = the f32-input MFMA chain, "fp16x2" = the opt-in two-term fp16 split,
    forced on all sizes (astk_set_gemm_bf16_split_below(0): by itself it hands launches below 3 GFLOP -- every shape of the small op
    tests -- to bf16x3).  The fixture moves the PROCESS DEFAULT, which is what descriptors with precision = ASTK_PREC_DEFAULT resolve to."""
    assert lib.astk_get_gemm_precision() == 1, "the library's default arithmetic must be bf16x3 (a reference-width scheme)"
    prev_below = lib.astk_set_gemm_bf16_split_below(C.c_double(0.0 if request.param == "fp16x2" else 3e9))
    prev = lib.astk_set_gemm_precision({"fp16x2": 0, "bf16x3": 1, "f32": 2}[request.param])
    assert prev == 1
    yield request.param
    lib.astk_set_gemm_precision(prev)
    lib.astk_set_gemm_bf16_split_below(C.c_double(prev_below))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to("cuda", dtype).contiguous()


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class GuardedWS:
    """Workspace with 64 KiB sentinel bands on both sides: every op test checks that nothing wrote outside."""
    G = 1 << 16

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.big = torch.full((self.nbytes + 2 * self.G,), 0x5A, dtype=torch.uint8, device="cuda")
        self.t = self.big[self.G:self.G + self.nbytes]

    def data_ptr(self):
        return self.t.data_ptr()

    def check(self, what=""):
        torch.cuda.synchronize()
        lo = int((self.big[:self.G] != 0x5A).sum())
        hi = int((self.big[self.G + self.nbytes:] != 0x5A).sum())
        assert lo == 0 and hi == 0, f"{what}: workspace overrun ({lo} bytes below, {hi} bytes above)"


def ok(lib, rc):
    assert rc == 0, lib.astk_last_error().decode()


def close(got, ref, rtol=2e-4, atol=None, msg=""):
    got = got.detach().cpu().double().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (msg, got.shape, ref.shape)
    scale = np.abs(ref).max() if ref.size else 1.0
    tol = (atol if atol is not None else rtol * max(scale, 1e-6))
    err = np.abs(got - ref).max() if ref.size else 0.0
    assert err <= tol, f"{msg}: max abs err {err:.3e} > {tol:.3e} (ref scale {scale:.3e})"


# ------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (200, 72, 120), (37, 1098, 512), (6, 8, 44), (300, 260, 1000), (1, 1, 4)])
def test_gemm_layouts(lib, layout, M, N, K, gemm_split):
    rng = np.random.default_rng(M * 7 + N * 3 + K + layout)
    A = rng.standard_normal((M, K))
    B = rng.standard_normal((N, K))
    bias = rng.standard_normal(N)
    ref = A @ B.T + bias
    pad = lambda n: (n + 3) // 4 * 4
    if layout == 0:
        Ad, lda, Bd, ldb = np.zeros((M, pad(K))), pad(K), np.zeros((N, pad(K))), pad(K)
        Ad[:, :K], Bd[:, :K] = A, B
    elif layout == 1:
        Ad, lda, Bd, ldb = np.zeros((M, pad(K))), pad(K), np.zeros((K, pad(N))), pad(N)
        Ad[:, :K], Bd[:, :N] = A, B.T
    else:
        Ad, lda, Bd, ldb = np.zeros((K, pad(M))), pad(M), np.zeros((K, pad(N))), pad(N)
        Ad[:, :M], Bd[:, :N] = A.T, B.T
    a, b, bi = dev(Ad), dev(Bd), dev(bias)
    c = torch.full((M, pad(N) + 4), 7.0, device="cuda")
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), lda, vp(b), ldb, vp(c), c.shape[1], vp(bi), 0, 1, 1, 0, 0, 0, stream()))
    close(c[:, :N], ref, rtol=2e-5, msg="store")
    assert float(c[:, N:].min()) == 7.0 and float(c[:, N:].max()) == 7.0, "wrote outside N"
    # accumulate
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), lda, vp(b), ldb, vp(c), c.shape[1], None, 1, 1, 1, 0, 0, 0, stream()))
    close(c[:, :N], 2 * ref - bias, rtol=2e-5, msg="accum")
    # split-K atomics into zeros
    c.zero_()
    ks = 3 if K >= 96 else 1
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), lda, vp(b), ldb, vp(c), c.shape[1], vp(bi), 2, ks, 1, 0, 0, 0, stream()))
    close(c[:, :N], ref, rtol=2e-5, msg="atomic split-K")


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", [(70, 45, 37), (130, 129, 16), (5, 3, 1), (129, 70, 531)])
def test_gemm_never_reads_padding_into_the_result(lib, layout, M, N, K, gemm_split):
    """Row padding (ld > extent) and whatever follows a ragged K tail hold NaNs: none may reach C, nor the columns beyond N."""
    rng = np.random.default_rng(M + N + K + layout)
    A = rng.standard_normal((M, K))
    B = rng.standard_normal((N, K))
    ref = A @ B.T
    pad = lambda n: (n + 3) // 4 * 4 + 4
    def padded(X):
        P = np.full((X.shape[0], pad(X.shape[1])), np.nan)
        P[:, :X.shape[1]] = X
        return P
    Ad = padded(A if layout != 2 else A.T)
    Bd = padded(B if layout == 0 else B.T)
    a, b = dev(Ad), dev(Bd)
    c = torch.full((M, pad(N)), 7.0, device="cuda")
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[1], vp(b), Bd.shape[1], vp(c), c.shape[1], None, 0, 1, 1, 0, 0, 0, stream()))
    close(c[:, :N], ref, rtol=2e-5, msg="store")
    assert float(c[:, N:].min()) == 7.0 and float(c[:, N:].max()) == 7.0, "wrote outside N"


def test_gemm_batched_tn(lib, gemm_split):
    rng = np.random.default_rng(3)
    Bt, M, N, K = 5, 22, 40, 9
    A = rng.standard_normal((K, Bt, 24))       # rows k, batch stride 24, M=22 valid cols
    Bm = rng.standard_normal((K, Bt, 40))
    ref = np.einsum("kbm,kbn->bmn", A[:, :, :M], Bm)
    a, b = dev(A), dev(Bm)
    c = torch.zeros(Bt, M, N, device="cuda")
    ok(lib, lib.astk_gemm_f32(2, M, N, K, vp(a), Bt * 24, vp(b), Bt * 40, vp(c), N, None, 0, 1, Bt, 24, 40, M * N, stream()))
    close(c, ref, rtol=2e-5)


# ------------------------------------------------------------------ CNN front-end
def _cnn_desc(cfg, B, T, D):
    from ast_amd._lib import CnnDesc
    cd = CnnDesc()
    cc = cfg["cnn_config"]["cnn_layers"]
    cd.B, cd.T, cd.D, cd.n_layers = B, T, D, len(cc)
    for i, l in enumerate(cc):
        cd.C[i] = l["out_channels"]
        cd.kt[i], cd.kf[i] = l["ksize"]
        cd.st[i], cd.sf[i] = l["stride"]
        cd.pt[i] = l["pad"][0]
    cd.bn_eps, cd.bn_decay = 2e-5, 0.9
    return cd


# (the fourth case: the shipped channel counts on 13-d features -- the conv GEMMs there are the small, 64-tile, two-level-row variants; the shapes with
#  16 / 128 layer-0 channels take the DIRECT layer-0 convolution under the default arithmetic (k_conv0_fwd_x3 + the window-matrix weight gradient):
#  80-d features = six frequency blocks, T = 331 / 170 = output lengths that are no multiple of the 80-step tiles, one shorter than a tile)
@pytest.mark.parametrize("B,T,D,c0,c1", [(3, 21, 26, 4, 8), (2, 50, 80, 8, 12), (2, 16, 13, 4, 4), (16, 400, 13, 128, 512), (3, 331, 80, 128, 32),
                                         (2, 170, 26, 16, 8), (2, 24, 80, 32, 8)])
@pytest.mark.parametrize("with_noise", [False, True])
def test_cnn_fwd_bwd(lib, B, T, D, c0, c1, with_noise, gemm_split):
    _cnn_case(lib, B, T, D, c0, c1, with_noise)


def _cnn_case(lib, B, T, D, c0, c1, with_noise, x_offset=0.0, seed=0, layer1_stats=False, layers=None, pool=None, all_stats=False,
              kink_free=False, expect_direct=None, **draw_kw):
    """x_offset, seed: tests/range_cases.py cnn_draws (the input with a per-bin offset: BatchNorm channels whose mean lies far from 0);
    layer1_stats: the running statistics of layer 1 are compared too; draw_kw: cnn_draws' ramp / centre_taps.
    layers: None = the shipped two layers with (c0, c1) channels, else the stack [(C, kt, kf, st, sf, pt), ...] (range_cases.cnn_geometry_cfg);
    pool: per-layer (time, frequency) max-pooling windows; all_stats: the running statistics of EVERY layer are compared;
    kink_free: the reference must have no near-kink unit in any layer (asserted: every gradient is then held to 5e-4);
    expect_direct: not None = the layer-0 path probe -- with the "conv.direct0" knob off the backward call on the forward's workspace is
    refused, before anything is launched, if and only if the forward took the direct kernel; the answer must equal expect_direct."""
    from ast_amd._lib import CnnLayerGrads, CnnLayerParams
    from oracle.ast_ref_torch import cnn_torch
    cfg, P, X, noise, rng = range_cases.cnn_draws(B, T, D, c0, c1, with_noise, x_offset=x_offset, seed=seed, layers=layers, pool=pool, **draw_kw)
    cc = cfg["cnn_config"]["cnn_layers"]
    n = len(cc)
    Pt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=k.startswith("CNN") and "avg" not in k) for k, v in P.items()}
    # Near-kink units: two valid float32 evaluations of one batch can disagree on the SIGN of a post-BatchNorm pre-activation that lies
    # within rounding of zero, and the unit's whole upstream gradient then enters or leaves its channel's sums -- ONE flipped unit moves that
    # channel's weight gradient by ~1 / sqrt(rows) of itself (round 6: a different, equally valid, summation order of the layer-1 forward
    # product -- pre-activations 4e-6 apart -- flipped units of the (16, 400, 13, 128, 512) case: CNN_1/W 3.7e-2, CNN_0/W 3.5e-3 of the
    # largest entry).  With ~10^6 units the float64 reference always has some within 1e-5 of the kink, whatever the draw.  So: the
    # upstream gradient is ZERO at the last layer's near-kink units (their sign then cannot matter), and the tensors of a layer at or BELOW
    # one (other than the last) with near-kink units are held to what a flipped unit can move (5e-3).  The exact comparison with named units
    # dropped on both sides is tests/test_golden.py's.
    bn_in = range_cases.cnn_bn_inputs(cfg, P, X, noise)       # per layer: (what its BatchNorm sees, the ReLU's pre-activation), float64
    near = [z.abs() < 2e-5 for _, z in bn_in]                 # (B, C, T_i, F_i)
    if kink_free:
        assert [int(m.sum()) for m in near] == [0] * n, "the case's seed must leave no unit within 2e-5 of the ReLU's kink"
    names = [f"CNN_{i}" for i in range(n)]
    grad_rtol = {names[i]: 5e-3 if any(bool(near[j].any()) for j in range(i, n - 1)) else 5e-4 for i in range(n)}
    out_ref = cnn_torch(cfg, Pt, torch.tensor(X), torch.tensor(noise) if with_noise else None)
    gout = rng.standard_normal(out_ref.shape)
    gout[range_cases.seq_layout(near[-1]).numpy()] = 0.0          # (T'', B, C F') with feature index c F' + f
    out_ref.backward(torch.tensor(gout))
    cd = _cnn_desc(cfg, B, T, D)
    for i, (wt, wf) in enumerate(pool or []):
        cd.pool_t[i], cd.pool_f[i] = wt, wf
    t2, f2, feat = C.c_int(), C.c_int(), C.c_int()
    ok(lib, lib.astk_conv_bn_relu_out_dims(C.byref(cd), C.byref(t2), C.byref(f2), C.byref(feat)))
    assert (t2.value, B, feat.value) == tuple(out_ref.shape)
    prm = {n_ + s: dev(P[n_ + s]) for n_ in names for s in ("/W", "_bn/gamma", "_bn/beta", "_bn/avg_mean", "_bn/avg_var")}
    grd = {k: torch.zeros_like(v) for k, v in prm.items()}
    cp, cg = (CnnLayerParams * n)(), (CnnLayerGrads * n)()
    for i, n_ in enumerate(names):
        cp[i].W, cp[i].gamma, cp[i].beta = prm[n_ + "/W"].data_ptr(), prm[n_ + "_bn/gamma"].data_ptr(), prm[n_ + "_bn/beta"].data_ptr()
        cp[i].avg_mean, cp[i].avg_var = prm[n_ + "_bn/avg_mean"].data_ptr(), prm[n_ + "_bn/avg_var"].data_ptr()
        cg[i].dW, cg[i].dgamma, cg[i].dbeta = grd[n_ + "/W"].data_ptr(), grd[n_ + "_bn/gamma"].data_ptr(), grd[n_ + "_bn/beta"].data_ptr()
    nbytes = lib.astk_conv_bn_relu_workspace_bytes(C.byref(cd))
    ws = GuardedWS(nbytes)
    out = torch.empty(t2.value, B, feat.value, device="cuda")
    xd, nd = dev(X), (dev(noise) if with_noise else None)
    ok(lib, lib.astk_conv_bn_relu_fwd(C.byref(cd), cp, vp(xd), vp(nd), vp(out), vp(ws), nbytes, 1, stream()))
    ws.check("cnn fwd")
    close(out, out_ref, msg="cnn out")
    # running statistics (A4): mean 0.1*mu, var 0.9 + 0.1*var*m/(m-1), of what each layer's BatchNorm sees (its own stride / pad / pooling)
    for i in range(n if all_stats else (2 if layer1_stats else 1)):
        y = bn_in[i][0]
        m = y.numel() // y.shape[1]
        tag = "" if i == 0 else f", layer {i}"
        close(prm[f"CNN_{i}_bn/avg_mean"], 0.1 * y.mean(dim=(0, 2, 3)), msg="avg_mean" + tag)
        close(prm[f"CNN_{i}_bn/avg_var"], 0.9 + 0.1 * y.var(dim=(0, 2, 3), unbiased=False) * m / (m - 1), msg="avg_var" + tag)
    g = dev(gout)
    probed = False
    if expect_direct is not None:
        prev = C.c_double()
        assert lib.astk_get_tuning(b"conv.direct0", C.byref(prev)) == 0 and prev.value == 1
        assert lib.astk_set_tuning(b"conv.direct0", 0.0) == 0
        try:
            rc = lib.astk_conv_bn_relu_bwd(C.byref(cd), cp, cg, vp(g), vp(ws), nbytes, stream())
        finally:
            assert lib.astk_set_tuning(b"conv.direct0", prev.value) == 0
        if rc != 0:        # refused in front of every launch: the forward took the direct kernel, this call would have taken im2col
            msg = lib.astk_last_error().decode()
            assert "took the direct-convolution layer-0 path" in msg, msg
            assert all(float(v.abs().max()) == 0.0 for v in grd.values()), "a refused backward call wrote gradients"
        else:              # im2col on both sides: the knob changed nothing, and this WAS the backward call
            probed = True
        assert (rc != 0) == expect_direct, f"layer 0 ran on the {'direct' if rc != 0 else 'im2col'} path"
    if not probed:
        ok(lib, lib.astk_conv_bn_relu_bwd(C.byref(cd), cp, cg, vp(g), vp(ws), nbytes, stream()))
    ws.check("cnn bwd")
    assert torch.equal(xd, dev(X)), "input clobbered"
    for n_ in names:
        for s in ("/W", "_bn/gamma", "_bn/beta"):
            close(grd[n_ + s], Pt[n_ + s].grad, rtol=grad_rtol[n_], msg="grad " + n_ + s)
    # A second backward call on the SAME forward pass, then a fresh forward + backward: the same gradients every time.  (Round 5: the
    # forward's last kernel zeroes the backward's accumulators -- statistics, maximum slots, weight-gradient scratch -- on its way out and
    # the library remembers that per workspace; the backward call that finds the mark taken has to fill them itself.)
    first = {k: v.clone() for k, v in grd.items()}
    for rep in range(2):
        for v in grd.values():
            v.zero_()
        if rep == 1:
            ok(lib, lib.astk_conv_bn_relu_fwd(C.byref(cd), cp, vp(xd), vp(nd), vp(out), vp(ws), nbytes, 1, stream()))
        g = dev(gout)
        ok(lib, lib.astk_conv_bn_relu_bwd(C.byref(cd), cp, cg, vp(g), vp(ws), nbytes, stream()))
        ws.check("cnn bwd again")
        for k in [n_ + s for s in ("/W", "_bn/gamma", "_bn/beta") for n_ in names]:
            close(grd[k], first[k].double().cpu().numpy(), rtol=2e-5, msg=f"backward call {rep + 2}: {k}")
    # eval mode uses the running statistics
    ok(lib, lib.astk_conv_bn_relu_fwd(C.byref(cd), cp, vp(xd), None, vp(out), vp(ws), nbytes, 0, stream()))
    hh = torch.tensor(X).unsqueeze(1)
    for i, l in enumerate(cc):
        hh = torch.nn.functional.conv2d(hh, Pt[f"CNN_{i}/W"].detach(), stride=tuple(l["stride"]), padding=tuple(l["pad"]))
        if pool:
            wt, wf = pool[i]
            k = (hh.shape[2] if wt == -1 else max(wt, 1), hh.shape[3] if wf == -1 else max(wf, 1))
            hh = torch.nn.functional.max_pool2d(hh, k, stride=k, ceil_mode=True)
        hh = torch.nn.functional.batch_norm(hh, prm[f"CNN_{i}_bn/avg_mean"].cpu().double(), prm[f"CNN_{i}_bn/avg_var"].cpu().double(),
                                            Pt[f"CNN_{i}_bn/gamma"].detach(), Pt[f"CNN_{i}_bn/beta"].detach(), training=False, eps=2e-5)
        hh = torch.relu(hh)
    close(out, range_cases.seq_layout(hh), msg="eval-mode out")


@pytest.mark.parametrize("B,T,D,c0,c1,pool", [(3, 42, 80, 4, 8, [[2, 1], [1, 1]]), (2, 50, 80, 8, 12, [[3, 2], [2, -1]]),
                                              (2, 76, 80, 4, 4, [[1, 4], [3, 2]]), (8, 400, 80, 128, 512, [[2, 2], [1, 3]]),
                                              (2, 30, 26, 4, 8, [[-1, 1], [1, 1]])])
def test_cnn_max_pool_fwd_bwd(lib, B, T, D, c0, c1, pool, gemm_split):
    """The old path's cnn_pool (enc_dec.py:444-456): max-pool between each convolution and its BatchNorm, per-layer (time, frequency)
    windows, -1 = whole extent, ragged last windows (cover_all) -- output and every parameter gradient against the torch restatement
    (max_pool2d with ceil_mode, the same operator)."""
    from ast_amd._lib import CnnLayerGrads, CnnLayerParams
    from oracle.ast_ref import init_params
    from oracle.ast_ref_torch import cnn_torch
    cfg = tiny_cfg(c0=c0, c1=c1)
    cfg["cnn_config"]["cnn_pool"] = pool
    P = init_params(cfg, D, 11, seed=1, dtype=np.float64)
    rng = np.random.default_rng(0)
    for i in range(2):
        P[f"CNN_{i}_bn/gamma"] = 1 + 0.3 * rng.standard_normal(P[f"CNN_{i}_bn/gamma"].shape)
        P[f"CNN_{i}_bn/beta"] = 0.2 * rng.standard_normal(P[f"CNN_{i}_bn/beta"].shape)
    X = rng.standard_normal((B, T, D))
    Pt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=k.startswith("CNN") and "avg" not in k) for k, v in P.items()}
    out_ref = cnn_torch(cfg, Pt, torch.tensor(X), None)
    gout = rng.standard_normal(out_ref.shape)
    out_ref.backward(torch.tensor(gout))
    cd = _cnn_desc(cfg, B, T, D)
    for i, (kt, kf) in enumerate(pool):
        cd.pool_t[i], cd.pool_f[i] = kt, kf
    t2, f2, feat = C.c_int(), C.c_int(), C.c_int()
    ok(lib, lib.astk_conv_bn_relu_out_dims(C.byref(cd), C.byref(t2), C.byref(f2), C.byref(feat)))
    assert (t2.value, B, feat.value) == tuple(out_ref.shape)
    assert feat.value == P["L0_enc/upward/W"].shape[1], "the oracle's LSTM input width follows the pooled frequency bins"
    names = ["CNN_0", "CNN_1"]
    prm = {n + s: dev(P[n + s]) for n in names for s in ("/W", "_bn/gamma", "_bn/beta", "_bn/avg_mean", "_bn/avg_var")}
    grd = {k: torch.zeros_like(v) for k, v in prm.items()}
    cp, cg = (CnnLayerParams * 2)(), (CnnLayerGrads * 2)()
    for i, n in enumerate(names):
        cp[i].W, cp[i].gamma, cp[i].beta = prm[n + "/W"].data_ptr(), prm[n + "_bn/gamma"].data_ptr(), prm[n + "_bn/beta"].data_ptr()
        cp[i].avg_mean, cp[i].avg_var = prm[n + "_bn/avg_mean"].data_ptr(), prm[n + "_bn/avg_var"].data_ptr()
        cg[i].dW, cg[i].dgamma, cg[i].dbeta = grd[n + "/W"].data_ptr(), grd[n + "_bn/gamma"].data_ptr(), grd[n + "_bn/beta"].data_ptr()
    nbytes = lib.astk_conv_bn_relu_workspace_bytes(C.byref(cd))
    ws = GuardedWS(nbytes)
    out = torch.empty(t2.value, B, feat.value, device="cuda")
    xd = dev(X)
    ok(lib, lib.astk_conv_bn_relu_fwd(C.byref(cd), cp, vp(xd), None, vp(out), vp(ws), nbytes, 1, stream()))
    ws.check("cnn fwd")
    close(out, out_ref, msg="cnn out")
    g = dev(gout)
    ok(lib, lib.astk_conv_bn_relu_bwd(C.byref(cd), cp, cg, vp(g), vp(ws), nbytes, stream()))
    ws.check("cnn bwd")
    for n in names:
        for s in ("/W", "_bn/gamma", "_bn/beta"):
            close(grd[n + s], Pt[n + s].grad, rtol=5e-4, msg="grad " + n + s)


# ------------------------------------------------------------------ encoder LSTM stacks
@pytest.mark.parametrize("T,B,in_dim,h,nl,masks", [(7, 3, 12, 4, 2, False), (9, 5, 24, 20, 3, True), (5, 33, 64, 36, 1, True), (1, 2, 8, 4, 2, False),
                                                   # h in {64,128,256,512}: the persistent wavefront kernels
                                                   (12, 5, 24, 64, 3, True), (7, 33, 16, 128, 2, False), (6, 16, 32, 256, 3, True),
                                                   (3, 4, 16, 512, 1, False), (1, 3, 8, 64, 2, True),
                                                   # 2 steps (the backward fetches the layer above's partials one step early; its last step has
                                                   # nothing left to fetch), 23 steps (the 4-deep sentinel ring of partial tiles comes round 5 times)
                                                   (2, 5, 16, 128, 3, True), (23, 17, 16, 64, 3, True),
                                                   # stacks whose (direction, layer) cells exceed one workgroup per CU: consecutive launches over
                                                   # groups of layers -- 3 layers as (2, 1) at batch 200 / h = 64, 6 layers as (2, 2, 2) at h = 512
                                                   # (the encoder of BASELINE configs[4]), 3 layers as (2, 1) at batch 64 / h = 256
                                                   (5, 200, 16, 64, 3, True), (4, 20, 24, 512, 6, False), (6, 64, 32, 256, 3, True),
                                                   # h = 64: one 16-k block per wave (half-empty 32-k MFMA operands of the split schemes)
                                                   (2, 5, 16, 64, 1, False), (2, 5, 16, 64, 2, False), (5, 5, 16, 64, 1, True), (5, 16, 16, 64, 2, False),
                                                   # h = 1024 per direction (the other reading of BASELINE configs[4]): the weight fragments of ONE product
                                                   # fill the registers -- the hoisted form of the persistent kernels (one launch per layer, the input
                                                   # projection and the gradient for the layer below as batched products between the launches);
                                                   # 32 rows = the two full batch tiles of that shape, 19 rows = a ragged second tile, 9 steps = the
                                                   # 4-deep ring of partial tiles comes round twice
                                                   (3, 4, 16, 1024, 2, False), (9, 19, 24, 1024, 3, True), (5, 32, 16, 1024, 2, True)])
def test_lstm_stack(lib, T, B, in_dim, h, nl, masks, gemm_split):
    _lstm_stack_case(lib, T, B, in_dim, h, nl, masks)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("side", [False, True])
@pytest.mark.parametrize("T,B,in_dim,h,nl,masks", [(6, 32, 32, 256, 3, True), (23, 33, 16, 64, 3, True), (9, 48, 24, 128, 2, False), (7, 64, 32, 256, 3, True),
                                                   (5, 17, 16, 256, 1, False), (2, 40, 16, 128, 3, True), (26, 64, 48, 64, 2, False), (12, 200, 16, 64, 3, True),
                                                   # 70 steps: ten and more 4-step chunks under either 32-row form (SIDE_FWD_CHUNKS)
                                                   (70, 33, 16, 64, 3, True), (70, 48, 24, 128, 2, False)])
def test_lstm_stack_32_row_workgroups_and_side_stream(lib, tune, T, B, in_dim, h, nl, masks, side, form, gemm_split):
    """Round 6.  (a) 32 batch rows per recurrence workgroup, both forms -- lstm.rows32 = 1: two 16-row tiles against one set of resident
    weight fragments in a 256-thread workgroup; = 2: two virtual 16-row workgroups in a 512-thread workgroup, two waves per SIMD, lo planes
    shared in LDS (bf16x3 only: under the other schemes the knob leaves the 16-row form) -- forced here where the library would choose them
    only when they spare launches: full, ragged (33, 17, 40, 48) and many (200) batch tiles, an odd tile count (the second half of the last
    512-thread workgroup has no rows), 1-3 layers, masks, every arithmetic scheme.  (b) `side`: the layer-0 input projection in time chunks on a second
    stream beside the forward recurrence (astk_lstm_stack_desc.side_stream; chunks of 4 steps here so that small T already has several),
    flag-gated inside the layer-0 cells; and the input gradient in chunks behind the backward recurrence's progress counter (lstm.side_bwd).
    Same float64 reference as test_lstm_stack.  With `side` the forward plan the library reports (astk_lstm_stack_side_plan) must be the one
    recorded in SIDE_FWD_CHUNKS -- the short shapes run everything in line, and only the plan tells them from the chunked ones -- and the
    forward results must be the BITS of the in-line call on the same inputs (astk.h; fp16x2: within the scheme's accuracy, capped launches
    run on bf16x3 operands)."""
    tune("lstm.rows32", form, lib)
    chunks = None
    if side:
        tune("lstm.overlap_chunk", 4, lib)
        tune("lstm.side_bwd", -1 if T % 2 else 2, lib)      # every chunk on the side stream / two chunks there and the rest of dx in line behind the recurrence
        rows_form = form if (form == 1 or gemm_split == "bf16x3") else 0      # (the 512-thread form is bf16x3's: the other schemes leave the 16-row form)
        chunks = SIDE_FWD_CHUNKS[(T, B, in_dim, h, nl)][rows_form]
    _lstm_stack_case(lib, T, B, in_dim, h, nl, masks, side=side, chunks=chunks, exact=gemm_split != "fp16x2")


@pytest.mark.parametrize("T,B,in_dim,h,nl,masks,knob", [(5, 17, 16, 64, 2, True, "lstm.persist"), (3, 4, 16, 1024, 2, False, "lstm.hoist")])
def test_lstm_stack_per_step_loop_at_the_persistent_widths(lib, T, B, in_dim, h, nl, masks, knob, gemm_split):
    """The route's per-step branch at widths where every other test takes a persistent path: "lstm.persist" 0 at h = 64 (two batch tiles, the
    second ragged) and "lstm.hoist" 0 at h = 1024.  astk_lstm_stack_path returns 0 and the per-step loop runs on a workspace whose
    row-sized buffers (counters, bias-gradient rows) are carved all the same.  Same float64 reference and tolerances as test_lstm_stack."""
    _lstm_stack_case(lib, T, B, in_dim, h, nl, masks, knobs={knob: 0}, path=0)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_lstm_stack_deterministic_bias_gradients_over_workgroup_rows(lib, form, gemm_split):
    """astk_lstm_stack_desc.deterministic = 1: the persistent backward kernel leaves its bias-gradient sums per (virtual) workgroup row and
    k_fold_db adds the rows in order.  33 batch rows are 3 rows of 16 under "lstm.rows32" 0, 2 rows of 32 under 1 and 4 virtual rows (the
    last without batch rows) under 2 -- which is bf16x3's: under the other schemes the knob leaves the 16-row form, as in
    test_lstm_stack_32_row_workgroups_and_side_stream -- with a ragged last tile each.  Within the usual tolerance of the float64 reference,
    and two calls on zeroed gradients give every db bit-equal."""
    _lstm_stack_case(lib, 6, 33, 16, 64, 2, True, knobs={"lstm.rows32": form}, path=1, deterministic=True)


# Forward chunks of 4 steps that plan_side_fwd's rate model puts on the side stream on an MI355X (256 CUs), per shape (T, B, in_dim, h, layers)
# and recurrence form (0: 16 rows per workgroup, 1 / 2: the 32-row forms), as astk_lstm_stack_side_plan reports them: a chunk of a 16-wide input
# costs ~15.7 model-us against 2.6-4 per recurrence step, so stacks of a few steps stay in line entirely.  (The counts follow from the device's
# CU count and the rate model's constants: whoever retunes plan_side_fwd is expected to update this table with what the query then returns.)
SIDE_FWD_CHUNKS = {(6, 32, 32, 256, 3): (0, 0, 0), (23, 33, 16, 64, 3): (3, 4, 3), (9, 48, 24, 128, 2): (0, 1, 0), (7, 64, 32, 256, 3): (0, 0, 0),
                   (5, 17, 16, 256, 1): (0, 0, 0), (2, 40, 16, 128, 3): (0, 0, 0), (26, 64, 48, 64, 2): (3, 5, 3), (12, 200, 16, 64, 3): (1, 2, 1),
                   (70, 33, 16, 64, 3): (11, 16, 12), (70, 48, 24, 128, 2): (10, 16, 12)}


def test_lstm_stack_late_side_stream_chunks(lib, tune, gemm_split):
    """The rate model sizes the in-line head so that no chunk is late; here the side stream is held back by a 1.5 ms spin (half of what the
    stream probe spins, far below the hand-off bound of seconds) while the recurrence is already running, so EVERY layer-0 cell finds its
    chunk flag down and takes the waiting branch: the acquire and the re-read of freshly written gates.  Same float64 reference, same bits as
    the in-line call, clean status word."""
    tune("lstm.overlap_chunk", 4, lib)
    _lstm_stack_case(lib, 70, 5, 96, 64, 2, False, side=True, chunks=9, exact=gemm_split != "fp16x2", late=True)


def _concurrent_stream(lib, main):
    """A second stream that really executes beside `main` (HIP multiplexes streams onto a few hardware queues; two streams that share one run
    in order, and a flag-gated consumer would then sit in front of its producer): probed like ast_amd/seq2seq.py does."""
    probe = torch.zeros(4, device="cuda")
    ok(lib, lib.astk_spin(10, None, C.c_void_p(main.cuda_stream)))            # (first launches load the code objects: not inside the probe)
    ok(lib, lib.astk_scale_f32(vp(probe), 4, 1.0, C.c_void_p(main.cuda_stream)))
    for _ in range(8):
        cand = torch.cuda.Stream()
        good = True
        for a, b in ((main, cand), (cand, main)):
            torch.cuda.synchronize()
            ok(lib, lib.astk_spin(3000, None, C.c_void_p(a.cuda_stream)))
            ea, eb = torch.cuda.Event(), torch.cuda.Event()
            ea.record(a)
            ok(lib, lib.astk_scale_f32(vp(probe), 4, 1.0, C.c_void_p(b.cuda_stream)))
            eb.record(b)
            eb.synchronize()
            good = good and not ea.query()
            ea.synchronize()
        if good:
            return cand
    pytest.skip("no pair of concurrently executing streams on this device")


def _lstm_stack_case(lib, *args, knobs=None, **kw):
    """knobs: tuning knobs (astk_set_tuning) in force for this case only; everything else: _lstm_stack_body."""
    prev = {}
    try:
        for k, v in (knobs or {}).items():
            prev[k] = C.c_double()
            assert lib.astk_get_tuning(k.encode(), C.byref(prev[k])) == 0 and lib.astk_set_tuning(k.encode(), float(v)) == 0, k
        _lstm_stack_body(lib, *args, **kw)
    finally:
        for k, v in prev.items():
            lib.astk_set_tuning(k.encode(), v.value)


def _lstm_stack_body(lib, T, B, in_dim, h, nl, masks, side=False, chunks=None, exact=True, late=False, bias_gain=1.0, x_gain=1.0, path=None,
                     deterministic=False):
    """chunks (with side): the forward chunks the library must plan for this case; exact: the side-stream forward results are compared bit for
    bit with an in-line call (else within close()); late: the side stream is held back (see below); bias_gain, x_gain: tests/range_cases.py
    lstm_draws (gains on the biases and the input: saturated gates); path: what astk_lstm_stack_path must return (default: 1 / 2 at the
    widths of the persistent / hoisted kernels); deterministic: the descriptor's field -- a second forward and backward on zeroed gradients
    must then give the bits of the first in every bias gradient."""
    from ast_amd._lib import LstmGrads, LstmParams, LstmStackDesc
    from oracle.ast_ref_torch import encoder_torch
    cfg = {"rnn_config": {"enc_layers": nl}}
    c = range_cases.lstm_draws(T, B, in_dim, h, nl, masks, bias_gain=bias_gain, x_gain=x_gain)
    P, names, x, mk, g_enc, g_c, g_h = (c[k] for k in ("P", "names", "x", "mk", "g_enc", "g_c", "g_h"))
    Pt = {k: torch.tensor(v, requires_grad=True) for k, v in P.items()}
    xt = torch.tensor(x, requires_grad=True)
    enc, cT, hT = encoder_torch(cfg, Pt, xt, torch.tensor(mk) if masks else None)
    assert g_enc.shape == enc.shape and g_c.shape == cT.shape and g_h.shape == hT.shape
    (enc * torch.tensor(g_enc)).sum().add((cT * torch.tensor(g_c)).sum()).add((hT * torch.tensor(g_h)).sum()).backward()
    d = LstmStackDesc(T, B, in_dim, h, nl, 2)
    d.deterministic = 1 if deterministic else 0
    if path is not None:
        assert lib.astk_lstm_stack_path(C.byref(d)) == path, "encoder path"
    elif h in (64, 128, 256, 512, 1024):
        assert lib.astk_lstm_stack_path(C.byref(d)) == (2 if h == 1024 else 1), "persistent encoder path not taken"
    main, side_s = None, None
    if side:                            # the op on a stream of its own + a second one for the chunked products (joined inside the calls)
        main = torch.cuda.Stream()
        side_s = _concurrent_stream(lib, main)
        d.side_stream = side_s.cuda_stream
        # (astk_lstm_stack_free_cus may be 0 -- a stack that fills the chip launch by launch: the library then keeps everything in line)
        torch.cuda.synchronize()

    def stream():                       # (shadows the module's helper: the stream this case launches on)
        return C.c_void_p(main.cuda_stream if main is not None else torch.cuda.current_stream().cuda_stream)
    prm = {k: dev(v) for k, v in P.items()}
    grd = {k: torch.zeros_like(v) for k, v in prm.items()}
    lp, lg = (LstmParams * (2 * nl))(), (LstmGrads * (2 * nl))()
    for i, n in enumerate(names):
        lp[i].Wu, lp[i].b, lp[i].Wl = (prm[n + s].data_ptr() for s in ("/upward/W", "/upward/b", "/lateral/W"))
        lg[i].dWu, lg[i].db, lg[i].dWl = (grd[n + s].data_ptr() for s in ("/upward/W", "/upward/b", "/lateral/W"))
    nbytes = lib.astk_lstm_stack_workspace_bytes(C.byref(d))
    ws = GuardedWS(nbytes)
    xd, md = dev(x), (dev(mk) if masks else None)
    enc_d = torch.zeros(B, T, 2 * h, device="cuda")
    cT_d, hT_d = torch.zeros(2, nl, B, h, device="cuda"), torch.zeros(2, nl, B, h, device="cuda")
    torch.cuda.synchronize()
    if side and chunks is not None:
        head, fwd_chunks, bwd_chunks = C.c_int(), C.c_int(), C.c_int()
        ok(lib, lib.astk_lstm_stack_side_plan(C.byref(d), C.byref(head), C.byref(fwd_chunks), C.byref(bwd_chunks)))
        plan = (head.value, fwd_chunks.value, bwd_chunks.value)
        assert plan[1] == chunks, (plan, chunks)
        assert plan[0] + 4 * plan[1] == T or plan[1] == 0, plan
    if late:
        # main spins 3 ms (the host queues the call behind it), the side stream waits for the end of that spin and then spins 1.5 ms itself:
        # the call orders the side stream behind the main one where it forks, so the spin sits in front of every chunk product
        ok(lib, lib.astk_spin(3000, None, stream()))
        go = torch.cuda.Event()
        go.record(main)
        side_s.wait_event(go)
        ok(lib, lib.astk_spin(1500, None, C.c_void_p(side_s.cuda_stream)))
    ok(lib, lib.astk_lstm_stack_fwd(C.byref(d), lp, vp(xd), vp(md), vp(enc_d), vp(cT_d), vp(hT_d), vp(ws), nbytes, stream()))
    torch.cuda.synchronize()
    ws.check("lstm fwd")
    close(enc_d, enc, msg="enc_states")
    close(cT_d, cT, msg="cT")
    close(hT_d, hT, msg="hT")
    if side:
        # the in-line call (no side stream in the descriptor) on the same inputs, in a workspace of its own
        d0 = LstmStackDesc(T, B, in_dim, h, nl, 2)
        ws0 = GuardedWS(lib.astk_lstm_stack_workspace_bytes(C.byref(d0)))
        enc_0 = torch.zeros_like(enc_d)
        cT_0, hT_0 = torch.zeros_like(cT_d), torch.zeros_like(hT_d)
        torch.cuda.synchronize()
        ok(lib, lib.astk_lstm_stack_fwd(C.byref(d0), lp, vp(xd), vp(md), vp(enc_0), vp(cT_0), vp(hT_0), vp(ws0), ws0.nbytes, stream()))
        torch.cuda.synchronize()
        ws0.check("lstm fwd in line")
        for got, want, what in ((enc_d, enc_0, "enc_states"), (cT_d, cT_0, "cT"), (hT_d, hT_0, "hT")):
            if exact:
                assert torch.equal(got, want), f"{what}: side-stream schedule differs from the in-line one by {float((got - want).abs().max()):.3e}"
            else:
                close(got, want, msg=what + " (side stream against in line)")
    dx = torch.zeros(T, B, in_dim, device="cuda")
    ge_d, gc_d, gh_d = dev(g_enc), dev(g_c), dev(g_h)     # keep alive: the call only enqueues work
    torch.cuda.synchronize()
    ok(lib, lib.astk_lstm_stack_bwd(C.byref(d), lp, lg, vp(xd), vp(md), vp(ge_d), vp(gc_d), vp(gh_d), vp(dx), vp(ws),
                                    nbytes, stream()))
    torch.cuda.synchronize()
    ws.check("lstm bwd")
    close(dx, xt.grad, rtol=5e-4, msg="dx")
    for k in P:
        ref_g = Pt[k].grad if Pt[k].grad is not None else torch.zeros_like(Pt[k])   # T=1: lateral.W is never used
        close(grd[k], ref_g, rtol=5e-4, atol=None if float(ref_g.abs().max()) > 0 else 1e-12, msg="grad " + k)
    if deterministic:
        first = {k: grd[k].clone() for k in P if k.endswith("/upward/b")}
        for v in grd.values():
            v.zero_()
        ok(lib, lib.astk_lstm_stack_fwd(C.byref(d), lp, vp(xd), vp(md), vp(enc_d), vp(cT_d), vp(hT_d), vp(ws), nbytes, stream()))
        ok(lib, lib.astk_lstm_stack_bwd(C.byref(d), lp, lg, vp(xd), vp(md), vp(ge_d), vp(gc_d), vp(gh_d), vp(dx), vp(ws),
                                        nbytes, stream()))
        torch.cuda.synchronize()
        ws.check("lstm fwd + bwd again")
        assert len(first) == 2 * nl
        for k, v in first.items():
            assert torch.equal(grd[k], v), f"grad {k}: two deterministic calls differ by {float((grd[k] - v).abs().max()):.3e}"
    if side:
        mask = C.c_uint(0)
        assert lib.astk_persist_status(C.byref(mask), 1) == 0 and mask.value == 0, mask.value


@pytest.mark.parametrize("nd,nl_enc,n,B,h", [(2, 3, 3, 5, 8), (2, 3, 1, 32, 256), (1, 2, 2, 3, 12), (2, 6, 1, 33, 512)])
def test_bridge_states_matches_the_strided_copies(lib, nd, nl_enc, n, B, h):
    """init_decoder_state (seq2seq.py:318-333) and its backward as one launch each: decoder layer k < n gets [fwd_k ; rev_k] of the encoder's
    final states (both tensors), the gradients go back the same way; layers >= n of either side are left alone."""
    rng = np.random.default_rng(nd * 100 + h)
    enc_c, enc_h = dev(rng.standard_normal((nd, nl_enc, B, h))), dev(rng.standard_normal((nd, nl_enc, B, h)))
    dec_c, dec_h = dev(rng.standard_normal((n + 1, B, nd * h))), dev(rng.standard_normal((n + 1, B, nd * h)))
    want_c, want_h = dec_c.clone(), dec_h.clone()
    for k in range(n):
        want_c[k].view(-1, nd, h).copy_(enc_c[:, k].permute(1, 0, 2))
        want_h[k].view(-1, nd, h).copy_(enc_h[:, k].permute(1, 0, 2))
    ok(lib, lib.astk_bridge_states(vp(dec_c), vp(dec_h), vp(enc_c), vp(enc_h), nd, nl_enc, n, B, h, 1, stream()))
    assert torch.equal(dec_c, want_c) and torch.equal(dec_h, want_h)
    # and back: the gradients of the bridged layers, the others untouched
    g_c, g_h = dev(rng.standard_normal((n + 1, B, nd * h))), dev(rng.standard_normal((n + 1, B, nd * h)))
    e_c, e_h = dev(rng.standard_normal((nd, nl_enc, B, h))), dev(rng.standard_normal((nd, nl_enc, B, h)))
    w_c, w_h = e_c.clone(), e_h.clone()
    for k in range(n):
        w_c[:, k].copy_(g_c[k].view(-1, nd, h).permute(1, 0, 2))
        w_h[:, k].copy_(g_h[k].view(-1, nd, h).permute(1, 0, 2))
    ok(lib, lib.astk_bridge_states(vp(g_c), vp(g_h), vp(e_c), vp(e_h), nd, nl_enc, n, B, h, 0, stream()))
    assert torch.equal(e_c, w_c) and torch.equal(e_h, w_h)
    assert lib.astk_bridge_states(vp(g_c), vp(g_h), vp(e_c), vp(e_h), nd, nl_enc, nl_enc + 1, B, h, 0, stream()) != 0      # more layers than the encoder has


def test_encoder_backward_last_arrival_waits_for_the_slowest_peer(monkeypatch):
    """Regression test of a hand-off race in lstm_persist_bwd_rs (round 4).  The layer below waits for `count >= NS * k` arrivals on the
    down-partials counter, which means "every slice has published k steps" only while the slices are at most one arrival apart; a slice's
    LAST arrival needs nothing from its peers, so a workgroup that finished early could make it while a slow peer was two arrivals behind,
    and a consumer then read the slow peer's tile of step 1 before it was written -- getting the PREVIOUS launch's tile.  ASTK_PERSIST_DBG=16
    makes slice 0 of every cell with a layer below dawdle exactly there; two different inputs alternate, so a stale tile is a wrong tile.
    The bias gradients are summed inside the kernel in a fixed order (two commutative atomic adds per element): bit-identical or broken.
    The dawdle is a TEST HOOK: it exists in libastk_test.so only (round 5; the product library's kernels never read ASTK_PERSIST_DBG --
    tests/test_host.py checks that), so the whole test runs on the instrumented build of the same kernel."""
    from ast_amd import _lib as L_
    from ast_amd._lib import LstmGrads, LstmParams, LstmStackDesc
    with L_.load_test_hooks() as lib:
        _last_arrival_body(lib, monkeypatch, LstmGrads, LstmParams, LstmStackDesc)


def _last_arrival_body(lib, monkeypatch, LstmGrads, LstmParams, LstmStackDesc):
    T, B, in_dim, h, nl = 200, 32, 64, 256, 3           # (T * B = 6400 rows: the batched products take their deterministic two-contributor tiles)
    rng = np.random.default_rng(11)
    names, prm, grd = [], {}, {}
    for pat in ("L{}_enc", "L{}_rev_enc"):
        n_in = in_dim
        for k in range(nl):
            n = pat.format(k); names.append(n)
            prm[n + "/Wu"], prm[n + "/b"] = dev(rng.standard_normal((4 * h, n_in)) / np.sqrt(n_in)), dev(rng.standard_normal(4 * h) * 0.3)
            prm[n + "/Wl"] = dev(rng.standard_normal((4 * h, h)) / np.sqrt(h)); n_in = h
    for k, v in prm.items():
        grd[k] = torch.zeros_like(v)
    lp, lg = (LstmParams * (2 * nl))(), (LstmGrads * (2 * nl))()
    for i, n in enumerate(names):
        lp[i].Wu, lp[i].b, lp[i].Wl = (prm[n + s].data_ptr() for s in ("/Wu", "/b", "/Wl"))
        lg[i].dWu, lg[i].db, lg[i].dWl = (grd[n + s].data_ptr() for s in ("/Wu", "/b", "/Wl"))
    d = LstmStackDesc(T, B, in_dim, h, nl, 2)
    assert lib.astk_lstm_stack_path(C.byref(d)) == 1
    nbytes = lib.astk_lstm_stack_workspace_bytes(C.byref(d))
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda")
    sets = [(dev(rng.standard_normal((T, B, in_dim))), dev(rng.standard_normal((B, T, 2 * h)))) for _ in range(2)]
    g_c, g_h = dev(rng.standard_normal((2, nl, B, h))), dev(rng.standard_normal((2, nl, B, h)))
    enc, cT, hT = torch.zeros(B, T, 2 * h, device="cuda"), torch.zeros(2, nl, B, h, device="cuda"), torch.zeros(2, nl, B, h, device="cuda")
    dx = torch.zeros(T, B, in_dim, device="cuda")

    def run(which):
        x, g_enc = sets[which]
        for v in grd.values():
            v.zero_()
        ok(lib, lib.astk_lstm_stack_fwd(C.byref(d), lp, vp(x), None, vp(enc), vp(cT), vp(hT), vp(ws), nbytes, stream()))
        ok(lib, lib.astk_lstm_stack_bwd(C.byref(d), lp, lg, vp(x), None, vp(g_enc), vp(g_c), vp(g_h), vp(dx), vp(ws), nbytes, stream()))
        return {n: grd[n + "/b"].clone() for n in names}

    ref = run(0)                       # no dawdling: the reference bias gradients of input 0
    monkeypatch.setenv("ASTK_PERSIST_DBG", "16")
    for it in range(12):
        run(1)
        got = run(0)
        for n in names:
            assert torch.equal(got[n], ref[n]), (it, n, float((got[n] - ref[n]).abs().max()))
    st = C.c_uint(0)
    lib.astk_persist_status(C.byref(st), 1)
    assert st.value == 0


# ------------------------------------------------------------------ attention scan
@pytest.mark.parametrize("B,T,H", [(3, 6, 8), (32, 50, 512), (5, 201, 260), (2, 9, 1024)])
def test_attention_step(lib, B, T, H):
    rng = np.random.default_rng(B * T)
    enc = rng.standard_normal((B, T, H)) * 0.5
    q = rng.standard_normal((B, H)) * 0.5
    et, qt = torch.tensor(enc, requires_grad=True), torch.tensor(q, requires_grad=True)
    alpha = torch.softmax(torch.einsum("bth,bh->bt", et, qt), dim=1)
    cv = torch.einsum("bth,bt->bh", et, alpha)
    g = rng.standard_normal(cv.shape)
    Tp = (T + 3) // 4 * 4
    nbytes = lib.astk_attn_workspace_bytes(B, T, H)
    ws = GuardedWS(nbytes)
    ed, qd = dev(enc), dev(q)
    a_d, cv_d = torch.zeros(B, Tp, device="cuda"), torch.zeros(B, H, device="cuda")
    ok(lib, lib.astk_attn_step_fwd(B, T, H, vp(ed), vp(qd), vp(a_d), vp(cv_d), vp(ws), nbytes, stream()))
    close(a_d[:, :T], alpha, msg="alpha")
    close(cv_d, cv, msg="cv")
    # backward: ds = dL/dscore, dq; d_enc is the deferred product alpha^T d_cv + ds^T q (checked in the decoder test)
    scores = torch.einsum("bth,bh->bt", et, qt)
    scores.retain_grad()
    al2 = torch.softmax(scores, dim=1)
    cv2 = torch.einsum("bth,bt->bh", et.detach(), al2)
    cv2.backward(torch.tensor(g))
    ds_ref = scores.grad
    dq_ref = torch.einsum("bt,bth->bh", ds_ref, et.detach())
    ds_d, dq_d = torch.zeros(B, Tp, device="cuda"), torch.zeros(B, H, device="cuda")
    g_d = dev(g)
    ok(lib, lib.astk_attn_step_bwd(B, T, H, vp(ed), vp(a_d), vp(cv_d), vp(g_d), vp(ds_d), vp(dq_d), vp(ws), nbytes, stream()))
    ws.check("attn")
    close(ds_d[:, :T], ds_ref, rtol=5e-4, msg="ds")
    close(dq_d, dq_ref, rtol=5e-4, msg="dq")


# ------------------------------------------------------------------ decoder loop
def _dec_setup(lib, B, L, T, H, E, A, V, nl, masks, seed=0, enc_gain=1.0, out_gain=1.0, bias_gain=1.0):
    """enc_gain, out_gain, bias_gain: tests/range_cases.py dec_draws (wide attention scores, wide logits, saturated gates)."""
    from ast_amd._lib import DecoderDesc, DecoderGrads, DecoderParams
    c = range_cases.dec_draws(B, L, T, H, E, A, V, nl, masks, seed=seed, enc_gain=enc_gain, out_gain=out_gain, bias_gain=bias_gain)
    P, enc, c0, h0, y, flags, em, rm, S = (c[k] for k in ("P", "enc", "c0", "h0", "y", "flags", "em", "rm", "S"))
    d = DecoderDesc(B, L, T, H, E, A, V, nl)
    prm = {k: dev(v) for k, v in P.items()}
    grd = {k: torch.zeros_like(v) for k, v in prm.items()}
    cw = torch.ones(V, device="cuda")
    cw[0] = 0
    dp, dg = DecoderParams(), DecoderGrads()
    dp.embed, dg.d_embed = prm["embed_dec/W"].data_ptr(), grd["embed_dec/W"].data_ptr()
    for k in range(nl):
        dp.lstm[k].Wu, dp.lstm[k].b, dp.lstm[k].Wl = (prm[f"L{k}_dec/" + s].data_ptr() for s in ("upward/W", "upward/b", "lateral/W"))
        dg.lstm[k].dWu, dg.lstm[k].db, dg.lstm[k].dWl = (grd[f"L{k}_dec/" + s].data_ptr() for s in ("upward/W", "upward/b", "lateral/W"))
    dp.Wa, dp.ba, dp.Wc, dp.bc, dp.Wo, dp.bo = (prm[k].data_ptr() for k in ("attn_Wa/W", "attn_Wa/b", "context/W", "context/b", "out/W", "out/b"))
    dg.dWa, dg.dba, dg.dWc, dg.dbc, dg.dWo, dg.dbo = (grd[k].data_ptr() for k in ("attn_Wa/W", "attn_Wa/b", "context/W", "context/b", "out/W", "out/b"))
    dp.class_weight = cw.data_ptr()
    return dict(P=P, enc=enc, c0=c0, h0=h0, y=y, flags=flags, em=em, rm=rm, d=d, dp=dp, dg=dg, prm=prm, grd=grd, cw=cw, S=S)


@pytest.mark.parametrize("B,L,T,H,E,A,V,nl,masks", [(3, 6, 6, 8, 4, 8, 11, 2, False), (5, 9, 23, 32, 12, 24, 57, 3, True),
                                                    (33, 4, 10, 64, 16, 64, 130, 1, True), (2, 2, 5, 8, 4, 8, 7, 1, False),
                                                    # 1 layer, H/A multiples of 16: the persistent decoder-loop kernel
                                                    (5, 9, 23, 64, 16, 32, 57, 1, False), (32, 7, 50, 512, 128, 512, 1098, 1, True),
                                                    (17, 5, 200, 256, 64, 128, 300, 1, True),
                                                    # 2 and 3 layers fused into the persistent decoder-loop kernels (generic attention phase, small
                                                    # and ragged batch tiles; then the shipped es_en_20h width with the H = 512 specialisation)
                                                    (5, 9, 23, 64, 16, 32, 57, 2, False), (19, 8, 37, 128, 32, 64, 130, 3, True),
                                                    (32, 7, 50, 512, 128, 512, 1098, 3, True), (30, 6, 200, 512, 128, 512, 1004, 2, False),
                                                    # long utterances: T'' = 300 / 420 (1200 / 1680 frames) at batch 32 -- slices of 38 / 53 rows, of which
                                                    # 28 stay in LDS and the rest is streamed every step
                                                    (32, 5, 300, 512, 128, 512, 1098, 1, False), (32, 4, 420, 512, 128, 512, 1098, 3, True),
                                                    (32, 4, 233, 512, 128, 512, 300, 1, True),
                                                    # ... and with 2 layers: slices of 30 rows, the smallest T'' and vocabulary that reach the
                                                    # streamed H = 512 scan of the two-layer kernels (forward and backward <8, 2, true>)
                                                    (32, 4, 233, 512, 128, 512, 300, 2, True),
                                                    # more than 32 rows at the shipped width: two persistent launches over halves of the rows (row split:
                                                    # 64 = 32 + 32, 48 = 32 + 16, 37 = 32 + 5; masks and initial states staged per half, loss over all rows)
                                                    (64, 6, 200, 512, 128, 512, 1098, 1, True), (48, 5, 200, 512, 128, 512, 1098, 3, True),
                                                    (37, 5, 50, 512, 128, 512, 300, 1, False),
                                                    # configs[4]'s decoder width on decoder_wide.hip's loops, WITHOUT the host copy of the flags (the
                                                    # kernel reads the device flags and computes the fed-back steps' logits itself)
                                                    (32, 7, 40, 1024, 128, 1024, 1098, 1, True), (9, 6, 30, 1024, 128, 1024, 8004, 1, False)])
def test_decoder_fwd_bwd(lib, B, L, T, H, E, A, V, nl, masks, gemm_split):
    s = _dec_setup(lib, B, L, T, H, E, A, V, nl, masks, seed=B + L)
    if H == 1024:
        assert lib.astk_decoder_path(C.byref(s["d"])) == 16
    elif H % 64 == 0 and A % 16 == 0 and E % 16 == 0 and nl <= 3:       # the shapes meant for the persistent kernels really take them
        assert lib.astk_decoder_path(C.byref(s["d"])) & 1, "persistent decoder path not taken"
        assert bool(lib.astk_decoder_path(C.byref(s["d"])) & 4) == (B > 32 and H == 512), "row split"
    _decoder_case(lib, s, B, L, T, H, E, A, V, nl, masks)


@pytest.mark.parametrize("B,L,T,H,E,A,V,nl,masks", [(5, 9, 23, 32, 12, 24, 57, 3, True), (32, 9, 50, 512, 128, 512, 1098, 1, True),
                                                    (19, 8, 37, 128, 32, 64, 130, 2, False), (2, 2, 5, 8, 4, 8, 7, 1, False),
                                                    # configs[4]'s decoder width and vocabulary: no persistent loop holds it, this is its path
                                                    (32, 8, 40, 1024, 128, 1024, 8004, 1, False),
                                                    # the wide forward loop: ragged batch tiles, dropout masks, slices of 25 rows, one-row slices
                                                    (19, 6, 200, 1024, 128, 1024, 300, 1, True), (4, 12, 40, 1024, 128, 1024, 8004, 1, True),
                                                    (32, 5, 256, 1024, 128, 1024, 1098, 1, False), (32, 4, 263, 1024, 128, 1024, 300, 1, False),
                                                    (1, 7, 7, 1024, 128, 1024, 50, 1, False), (64, 6, 200, 1024, 128, 1024, 300, 1, True), (45, 5, 40, 1024, 128, 1024, 300, 1, False)])
def test_decoder_per_launch_loop_scored_behind_the_loop(lib, tune, B, L, T, H, E, A, V, nl, masks, gemm_split):
    """The per-launch loop with the caller's HOST copy of the flags (astk_decoder_desc.use_truth_host): logits inside the loop only for the
    steps whose argmax is fed back, every step scored by one product and one softmax-CE launch behind it; in the backward, dlogits Wo as
    one product in front of the loop and the carry through input feeding from the epilogue of the next step's d_x0 product."""
    tune("dec.persist", 0, lib)
    s = _dec_setup(lib, B, L, T, H, E, A, V, nl, masks, seed=B + L + 1)
    assert not (lib.astk_decoder_path(C.byref(s["d"])) & 1)
    # configs[4]'s width: decoder_wide.hip's persistent loops
    Bw = B if B <= 32 else 32                                   # (more than 32 rows: two launches over halves, like the shipped width)
    slice_rows = -(-T // max(1, min(256 // Bw, T, 64)))         # rows of enc_states a workgroup keeps in LDS (4 KB each)
    assert bool(lib.astk_decoder_path(C.byref(s["d"])) & 16) == (H == 1024 and A == 1024 and E == 128 and nl == 1 and B <= 64 and slice_rows <= 32)
    assert bool(lib.astk_decoder_path(C.byref(s["d"])) & 4) == (H == 1024 and B > 32)
    host = (C.c_int32 * s["S"])(*[int(f) for f in s["flags"]])
    s["d"].use_truth_host = C.cast(host, C.POINTER(C.c_int32))
    assert 0 in list(host) or s["S"] < 3, "the case should feed at least one argmax back"
    _decoder_case(lib, s, B, L, T, H, E, A, V, nl, masks)


@pytest.mark.parametrize("env", ["dec.b6_fused", "dec.b6_split"])
@pytest.mark.parametrize("B,L,T,H,E,A,V,nl,masks", [(32, 7, 50, 512, 128, 512, 1098, 1, True), (17, 5, 60, 256, 64, 128, 300, 1, False),
                                                    (32, 6, 50, 512, 128, 512, 1098, 3, True)])
def test_decoder_backward_older_role_layouts(lib, tune, env, B, L, T, H, E, A, V, nl, masks):
    """The persistent backward kernel's role layouts of rounds 2-3, kept behind tuning knobs for A/B runs: dec.b6_fused 0 = a d_x0 role
    (two K halves per item) handing the carry to the d_pre items; dec.b6_split 0 (one layer only) = whole d_x0 items inside the kernel.
    The default (no d_x0 role, d_pre formed by the d_cvh items) is what every other decoder test runs."""
    if env == "dec.b6_split" and nl > 1:
        pytest.skip("the multi-layer role layout always splits the d_x0 items")
    tune(env, 0, lib)
    s = _dec_setup(lib, B, L, T, H, E, A, V, nl, masks, seed=B + L + 2)
    assert lib.astk_decoder_path(C.byref(s["d"])) & 1, "persistent decoder path not taken"
    _decoder_case(lib, s, B, L, T, H, E, A, V, nl, masks)


def test_decoder_backward_refuses_a_capped_phase_in_deterministic_mode(lib):
    """Argument validation (include/astk.h, astk_decoder_desc.side_wgs): the fix-up workspace of the deterministic split tiles is process-wide
    and serves one launch at a time, so a parameter-gradient phase that is CAPPED -- meant to run on a second stream beside other launches --
    is refused when `deterministic` holds, before anything is launched; the same phase without a cap runs, and chain + parameter phases
    leave the gradients of the one-call backward."""
    B, L, T, H, E, A, V, nl = 5, 9, 23, 64, 16, 32, 57, 1
    s = _dec_setup(lib, B, L, T, H, E, A, V, nl, False, seed=B + L + 3)
    d = s["d"]
    assert lib.astk_decoder_path(C.byref(d)) & 1, "persistent decoder path not taken"
    nbytes = lib.astk_decoder_workspace_bytes(C.byref(d))
    ws = GuardedWS(nbytes)
    enc_d, c0_d, h0_d = dev(s["enc"]), dev(s["c0"]), dev(s["h0"])
    y_d, fl_d = dev(s["y"], torch.int32), dev(np.asarray(s["flags"]), torch.int32)
    loss_d, pred_d = torch.zeros(1, device="cuda"), torch.zeros(s["S"], B, dtype=torch.int32, device="cuda")
    d_enc = torch.zeros(B, T, H, device="cuda")
    d_c0, d_h0 = torch.zeros(nl, B, H, device="cuda"), torch.zeros(nl, B, H, device="cuda")

    def fwd():
        ok(lib, lib.astk_decoder_fwd(C.byref(d), C.byref(s["dp"]), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), vp(fl_d), None, None,
                                     vp(loss_d), vp(pred_d), vp(ws), nbytes, stream()))

    def phase(which):
        return lib.astk_decoder_bwd_phase_ex(C.byref(d), C.byref(s["dp"]), C.byref(s["dg"]), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), None, None, None,
                                             vp(d_enc), vp(d_c0), vp(d_h0), vp(ws), nbytes, which, stream())
    d.deterministic = 1
    fwd()
    ok(lib, phase(1))                                            # ASTK_DEC_BWD_CHAIN
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in s["grd"].items()}
    d.side_wgs = 64
    assert phase(2) != 0                                         # ASTK_DEC_BWD_PARAMS, capped: refused
    msg = lib.astk_last_error().decode()
    assert "deterministic" in msg and "side_wgs" in msg, msg
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[k]) for k, v in s["grd"].items()), "the refused call launched something"
    d.side_wgs = 0
    ok(lib, phase(2))
    torch.cuda.synchronize()
    ws.check("decoder bwd, chain + parameter phases")
    split = {k: v.clone() for k, v in s["grd"].items()}
    for v in s["grd"].values():
        v.zero_()
    fwd()
    ok(lib, phase(0))                                            # ASTK_DEC_BWD_ALL
    torch.cuda.synchronize()
    for k, v in s["grd"].items():
        assert float((split[k] - v).abs().max()) <= 1e-5 * max(float(v.abs().max()), 1e-30), k
    d.side_wgs = 64                                              # without `deterministic` the capped phase is what the train step runs
    d.deterministic = 0
    fwd()
    ok(lib, phase(1))
    ok(lib, phase(2))
    torch.cuda.synchronize()
    ws.check("decoder bwd, capped parameter phase")


def test_decoder_backward_refuses_a_workspace_whose_forward_took_another_path(lib, tune):
    """The kernel path and the workspace carve follow the tuning knobs of each call, so a backward call made under other knobs than its
    forward call would read the saved activations at shifted offsets.  The forward records the path it took on the workspace; a backward
    call that would take another one (here: dec.persist switched off in between) is refused before anything is launched, and with the
    knob restored the same workspace serves forward and backward."""
    B, L, T, H, E, A, V, nl = 5, 9, 23, 64, 16, 32, 57, 1
    s = _dec_setup(lib, B, L, T, H, E, A, V, nl, False, seed=B + L + 4)
    d = s["d"]
    assert lib.astk_decoder_path(C.byref(d)) & 1, "persistent decoder path not taken"
    nbytes = lib.astk_decoder_workspace_bytes(C.byref(d))
    ws = GuardedWS(nbytes)
    enc_d, c0_d, h0_d = dev(s["enc"]), dev(s["c0"]), dev(s["h0"])
    y_d, fl_d = dev(s["y"], torch.int32), dev(np.asarray(s["flags"]), torch.int32)
    loss_d, pred_d = torch.zeros(1, device="cuda"), torch.zeros(s["S"], B, dtype=torch.int32, device="cuda")
    outs = {"d_enc": torch.full((B, T, H), 3.0, device="cuda"), "d_c0": torch.full((nl, B, H), 5.0, device="cuda"),
            "d_h0": torch.full((nl, B, H), 7.0, device="cuda")}
    for v in s["grd"].values():
        v.fill_(2.0)                                             # (a launch that accumulates, stores or zeroes would show)
    ok(lib, lib.astk_decoder_fwd(C.byref(d), C.byref(s["dp"]), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), vp(fl_d), None, None,
                                 vp(loss_d), vp(pred_d), vp(ws), nbytes, stream()))
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in list(s["grd"].items()) + list(outs.items())}
    tune("dec.persist", 0, lib)
    assert not (lib.astk_decoder_path(C.byref(d)) & 1)
    rc = lib.astk_decoder_bwd(C.byref(d), C.byref(s["dp"]), C.byref(s["dg"]), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), None, None,
                              vp(outs["d_enc"]), vp(outs["d_c0"]), vp(outs["d_h0"]), vp(ws), nbytes, stream())
    assert rc != 0
    msg = lib.astk_last_error().decode()
    assert "took kernel path 1" in msg, msg
    torch.cuda.synchronize()
    for k, v in list(s["grd"].items()) + list(outs.items()):
        assert torch.equal(v, before[k]), f"the refused call launched something ({k})"
    ws.check("decoder bwd, refused")
    tune("dec.persist", 1, lib)
    assert lib.astk_decoder_path(C.byref(d)) & 1
    for v in s["grd"].values():
        v.zero_()
    _decoder_case(lib, s, B, L, T, H, E, A, V, nl, False, ws=ws)


def test_wide_decoder_path_and_bounded_spins(lib, tune):
    """configs[4]'s decoder (H = A = 1024, E = 128, one layer, 32 rows, T'' = 200, V = 8004) reports decoder_wide.hip's persistent loops
    (astk_decoder_path bit 4), and their spins are bounded like every other persistent kernel's: with the knob persist.spin_limit = 1 the
    launches give up, drain and leave the decoder bits in the library's sticky status word instead of hanging."""
    from ast_amd._lib import DecoderDesc
    assert lib.astk_decoder_path(C.byref(DecoderDesc(32, 40, 200, 1024, 128, 1024, 8004, 1))) == 16
    assert lib.astk_decoder_path(C.byref(DecoderDesc(32, 40, 300, 1024, 128, 1024, 8004, 1))) == 0      # slices of 38 rows do not fit LDS
    assert lib.astk_decoder_path(C.byref(DecoderDesc(32, 40, 200, 1024, 128, 1024, 8004, 2))) == 0      # one layer only
    B, L, T, H, E, A, V, nl = 8, 6, 24, 1024, 128, 1024, 300, 1
    s = _dec_setup(lib, B, L, T, H, E, A, V, nl, False, seed=3)
    host = (C.c_int32 * s["S"])(*[int(f) for f in s["flags"]])
    s["d"].use_truth_host = C.cast(host, C.POINTER(C.c_int32))
    nbytes = lib.astk_decoder_workspace_bytes(C.byref(s["d"]))
    ws = GuardedWS(nbytes)
    enc_d, c0_d, h0_d = dev(s["enc"]), dev(s["c0"]), dev(s["h0"])
    y_d, fl_d = dev(s["y"], torch.int32), dev(np.asarray(s["flags"]), torch.int32)
    loss_d, pred_d = torch.zeros(1, device="cuda"), torch.zeros(s["S"], B, dtype=torch.int32, device="cuda")
    mask = C.c_uint(0)
    assert lib.astk_persist_status(C.byref(mask), 1) == 0
    tune("persist.spin_limit", 1, lib)
    ok(lib, lib.astk_decoder_fwd(C.byref(s["d"]), C.byref(s["dp"]), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), vp(fl_d), None, None,
                                 vp(loss_d), vp(pred_d), vp(ws), nbytes, stream()))
    assert lib.astk_persist_status(C.byref(mask), 1) == 0 and mask.value & 4, mask.value           # PERSIST_DEC_FWD
    d_enc = torch.zeros(B, T, H, device="cuda")
    d_c0, d_h0 = torch.zeros(nl, B, H, device="cuda"), torch.zeros(nl, B, H, device="cuda")
    ok(lib, lib.astk_decoder_bwd(C.byref(s["d"]), C.byref(s["dp"]), C.byref(s["dg"]), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), None,
                                 None, vp(d_enc), vp(d_c0), vp(d_h0), vp(ws), nbytes, stream()))
    assert lib.astk_persist_status(C.byref(mask), 1) == 0 and mask.value & 8, mask.value           # PERSIST_DEC_BWD
    tune("persist.spin_limit", 0, lib)
    ws.check("wide decoder, timed-out launches")


def _decoder_case(lib, s, B, L, T, H, E, A, V, nl, masks, ws=None):
    """ws: a GuardedWS of astk_decoder_workspace_bytes to run on (default: a fresh one)."""
    from oracle.ast_ref_torch import decoder_torch
    cfg = {"rnn_config": {"dec_layers": nl, "attn_units": A}}
    Pt = {k: torch.tensor(v, requires_grad=True) for k, v in s["P"].items()}
    enc_t = torch.tensor(s["enc"], requires_grad=True)
    c0_t, h0_t = torch.tensor(s["c0"], requires_grad=True), torch.tensor(s["h0"], requires_grad=True)
    tt = lambda a: None if a is None else torch.tensor(a)
    loss_ref, pred_ref = decoder_torch(cfg, Pt, enc_t, c0_t, h0_t, s["y"], s["flags"], V, tt(s["em"]), tt(s["rm"]))
    loss_ref.backward()
    nbytes = lib.astk_decoder_workspace_bytes(C.byref(s["d"]))
    ws = ws or GuardedWS(nbytes)
    assert ws.nbytes == nbytes
    enc_d, c0_d, h0_d = dev(s["enc"]), dev(s["c0"]), dev(s["h0"])
    y_d, fl_d = dev(s["y"], torch.int32), dev(np.asarray(s["flags"]), torch.int32)
    em_d, rm_d = (dev(s["em"]) if masks else None), (dev(s["rm"]) if masks else None)
    loss_d = torch.zeros(1, device="cuda")
    pred_d = torch.zeros(s["S"], B, dtype=torch.int32, device="cuda")
    ok(lib, lib.astk_decoder_fwd(C.byref(s["d"]), C.byref(s["dp"]), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), vp(fl_d), vp(em_d), vp(rm_d),
                                 vp(loss_d), vp(pred_d), vp(ws), nbytes, stream()))
    ws.check("decoder fwd")
    assert abs(float(loss_d) - float(loss_ref)) <= 1e-4 * abs(float(loss_ref)), (float(loss_d), float(loss_ref))
    assert (pred_d.cpu().numpy() == pred_ref.numpy()).all(), "argmax feedback tokens differ"
    d_enc = torch.zeros(B, T, H, device="cuda")
    d_c0, d_h0 = torch.zeros(nl, B, H, device="cuda"), torch.zeros(nl, B, H, device="cuda")
    ok(lib, lib.astk_decoder_bwd(C.byref(s["d"]), C.byref(s["dp"]), C.byref(s["dg"]), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), vp(em_d),
                                 vp(rm_d), vp(d_enc), vp(d_c0), vp(d_h0), vp(ws), nbytes, stream()))
    ws.check("decoder bwd")
    close(d_enc, enc_t.grad, rtol=5e-4, msg="d_enc")
    close(d_c0, c0_t.grad, rtol=5e-4, msg="d_c0")
    close(d_h0, h0_t.grad, rtol=5e-4, msg="d_h0")
    for k in s["P"]:
        close(s["grd"][k], Pt[k].grad, rtol=5e-4, msg="grad " + k)


def test_decoder_step_infer_matches_teacher_forced_step(lib):
    """One eval-mode step from the initial state equals step 0 of the training loop without dropout."""
    B, L, T, H, E, A, V, nl = 4, 5, 12, 16, 8, 16, 23, 2
    s = _dec_setup(lib, B, L, T, H, E, A, V, nl, False, seed=5)
    nbytes = lib.astk_decoder_workspace_bytes(C.byref(s["d"]))
    ws = GuardedWS(nbytes)
    enc_d = dev(s["enc"])
    c, h = dev(s["c0"]), dev(s["h0"])
    ht = torch.zeros(B, A, device="cuda")
    tok = dev(s["y"][:, 0], torch.int32)
    logits, alpha = torch.zeros(B, V, device="cuda"), torch.zeros(B, T, device="cuda")
    am = torch.zeros(B, dtype=torch.int32, device="cuda")
    ok(lib, lib.astk_decoder_step_infer(C.byref(s["d"]), C.byref(s["dp"]), vp(enc_d), vp(c), vp(h), vp(ht), vp(tok), vp(logits), vp(alpha),
                                        vp(am), vp(ws), nbytes, stream()))
    ws.check("decoder infer")
    P = {k: torch.tensor(v) for k, v in s["P"].items()}
    x = torch.cat([P["embed_dec/W"][torch.tensor(s["y"][:, 0]).long()], torch.zeros(B, A, dtype=torch.float64)], 1)
    cs, hs = torch.tensor(s["c0"]), torch.tensor(s["h0"])
    for k in range(nl):
        z = (x @ P[f"L{k}_dec/upward/W"].t() + P[f"L{k}_dec/upward/b"] + hs[k] @ P[f"L{k}_dec/lateral/W"].t()).view(B, -1, 4)
        a_, i_, f_, o_ = torch.tanh(z[..., 0]), torch.sigmoid(z[..., 1]), torch.sigmoid(z[..., 2]), torch.sigmoid(z[..., 3])
        cn = a_ * i_ + f_ * cs[k]
        x = o_ * torch.tanh(cn)
        close(c[k], cn, msg=f"c{k}")
        close(h[k], x, msg=f"h{k}")
    q = x @ P["attn_Wa/W"].t() + P["attn_Wa/b"]
    al = torch.softmax(torch.einsum("bth,bh->bt", torch.tensor(s["enc"]), q), 1)
    cv = torch.einsum("bth,bt->bh", torch.tensor(s["enc"]), al)
    htr = torch.tanh(torch.cat([cv, x], 1) @ P["context/W"].t() + P["context/b"])
    lg = htr @ P["out/W"].t() + P["out/b"]
    close(alpha, al, msg="alpha")
    close(ht, htr, msg="ht")
    close(logits, lg, msg="logits")
    assert (am.cpu().numpy() == lg.argmax(1).numpy()).all()


# ------------------------------------------------------------------ softmax-CE, optimizer, RNG
def test_softmax_ce(lib):
    rng = np.random.default_rng(1)
    B, V, ld = 7, 1098, 1100
    x = rng.standard_normal((B, V)) * 3
    t = rng.integers(0, V, B).astype(np.int32)
    t[2] = 0
    w = np.ones(V)
    w[0] = 0
    xt = torch.tensor(x, requires_grad=True)
    loss = torch.nn.functional.cross_entropy(xt, torch.tensor(t).long(), weight=torch.tensor(w), reduction="sum") / B
    loss.backward()
    buf = torch.zeros(B, ld, device="cuda")
    buf[:, :V] = dev(x)
    rows, am = torch.zeros(B, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    t_d, w_d = dev(t, torch.int32), dev(w)
    ok(lib, lib.astk_softmax_ce_fwd(B, V, ld, vp(buf), vp(t_d), 1, vp(w_d), 1.0 / B, vp(rows), vp(am), stream()))
    assert abs(float(rows.sum()) - float(loss)) < 1e-5 * abs(float(loss))
    assert float(rows[2]) == 0.0
    close(buf[:, :V], xt.grad, msg="dlogits")
    assert float(buf[:, V:].abs().max()) == 0.0
    assert (am.cpu().numpy() == x.argmax(1)).all()


def test_softmax_ce_loss_rows_are_read_before_the_gradient_overwrites_the_logits(lib):
    """The kernel turns the logits into their gradient IN PLACE and the loss row needs the target's logit: that read has to happen in
    front of the barrier that precedes the overwrite.  Until the end of round 3 it was an ordinary load whose only use sat behind the
    barrier (through a __restrict__ pointer), and about one loss row in a few thousand came out with exp(x - lse) * scale - scale in place
    of the logit, depending on which wave reached the store first; the gradient was never affected.  Many rows, every row checked."""
    rng = np.random.default_rng(5)
    B, V, ld = 16384, 300, 300
    x = (rng.standard_normal((B, V)) * 2).astype(np.float32)
    t = rng.integers(1, V, B).astype(np.int32)
    xt = torch.tensor(x, dtype=torch.float64)
    want = torch.nn.functional.cross_entropy(xt, torch.tensor(t).long(), reduction="none").numpy() / 32
    t_d = dev(t, torch.int32)
    worst = 0.0
    for rep in range(4):
        buf = dev(x).clone()
        rows = torch.zeros(B, device="cuda")
        ok(lib, lib.astk_softmax_ce_fwd(B, V, ld, vp(buf), vp(t_d), 1, None, 1.0 / 32, vp(rows), None, stream()))
        err = np.abs(rows.cpu().numpy().astype(np.float64) - want)
        worst = max(worst, float((err / np.maximum(want, 1e-3)).max()))
    assert worst < 1e-5, worst


def test_optimizer_step_matches_reference(lib):
    from oracle.ast_ref import RefOptimizer
    from optimizer_model import TOL
    from oracle import minichainer as F
    rng = np.random.default_rng(2)
    n = 10007
    p0, grads = rng.standard_normal(n), [rng.standard_normal(n) * s for s in (0.05, 0.001, 0.2)]

    class M:
        def __init__(self):
            self.p = {"a/W": F.Parameter(p0.copy())}

        def params(self):
            return list(self.p.items())
    m = M()
    ref = RefOptimizer(m, {"type": 0, "lr": 1e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []})
    npad = (n + 3) // 4 * 4
    p = torch.zeros(npad, device="cuda")
    p[:n] = dev(p0)
    mm, vv, vh = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    sq = torch.zeros(1, dtype=torch.float64, device="cuda")
    above = 0.0
    for t, g0 in enumerate(grads, 1):
        m.p["a/W"].grad = g0.copy()
        ref.update()
        g = torch.zeros(npad, device="cuda")
        g[:n] = dev(g0)
        ok(lib, lib.astk_grad_sqnorm(vp(g), vp(p), 1e-4, npad, vp(sq), stream()))
        assert abs(float(sq.sqrt()) - ref.last_grad_norm) < 1e-5 * ref.last_grad_norm
        lr_t = 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        ok(lib, lib.astk_decay_clip_amsgrad_step(vp(p), vp(g), vp(mm), vp(vv), vp(vh), npad, 1e-4, 2.0, vp(sq), lr_t, 0.9, 0.999, 1e-8, 1,
                                                 stream()))
        close(p[:n], m.p["a/W"].data, rtol=1e-5, msg=f"params after step {t}")
        # the moments too, at the tolerances tests/optimizer_model.py derives: p alone cannot tell AMSGrad from plain Adam
        for q, got in (("m", mm), ("v", vv), ("vhat", vh)):
            close(got[:n], ref.state["a/W"][q], rtol=TOL[q], msg=f"{q} after step {t}")
        st = ref.state["a/W"]
        above = max(above, float(np.mean(st["vhat"] > st["v"])))
    assert above > 0.25, "the draws must make AMSGrad's maximum matter at some step"
    assert float(p[n:].abs().max()) == 0.0


def test_rng_fills(lib):
    n = 1 << 20
    m = torch.zeros(n, device="cuda")
    ok(lib, lib.astk_fill_dropout_mask(vp(m), n, 0.3, 1234, 0, stream()))
    keep = float((m > 0).float().mean())
    assert abs(keep - 0.7) < 5e-3 and abs(float(m.max()) - 1 / 0.7) < 1e-6
    m2 = torch.zeros(n, device="cuda")
    ok(lib, lib.astk_fill_dropout_mask(vp(m2), n, 0.3, 1234, n, stream()))
    assert float((m != m2).float().mean()) > 0.3, "successive offsets must give fresh masks"
    z = torch.zeros(n, device="cuda")
    ok(lib, lib.astk_fill_normal(vp(z), n, 1.0, 0.25, 99, 0, stream()))
    assert abs(float(z.mean()) - 1.0) < 2e-3 and abs(float(z.std()) - 0.25) < 2e-3


def test_fused_random_fill_equals_the_separate_fills(lib):
    """astk_fill_random (the step's speech noise and dropout masks in one launch) gives every element exactly the value astk_fill_normal /
    astk_fill_dropout_mask give it for the same (seed, offset): bit-identical, ragged sizes, an odd-length normal segment, an empty one."""
    from ast_amd._lib import RandSeg, RAND_DROPOUT, RAND_NORMAL
    spec = [(RAND_NORMAL, 2048001, 1.0, 0.25, 0xABCDEF ^ 0x5EED, 0), (RAND_DROPOUT, 3 * 200 * 32 * 256 + 5, 0.3, 0.0, 0x5EED, 2048001),
            (RAND_DROPOUT, 39 * 32 * 128, 0.3, 0.0, 0x5EED, 7000000), (RAND_NORMAL, 0, 0.0, 1.0, 1, 0), (RAND_DROPOUT, 17, 0.5, 0.0, 9, 3)]
    segs = (RandSeg * len(spec))()
    fused, ref = [], []
    for i, (kind, n, a, b, seed, off) in enumerate(spec):
        t = torch.full((max(n, 1),), 7.0, device="cuda")
        fused.append(t)
        segs[i].out, segs[i].n, segs[i].kind, segs[i].a, segs[i].b, segs[i].seed, segs[i].offset = t.data_ptr(), n, kind, a, b, seed, off
        r = torch.full((max(n, 1),), 7.0, device="cuda")
        if kind == RAND_NORMAL:
            ok(lib, lib.astk_fill_normal(vp(r), n, a, b, seed, off, stream()))
        else:
            ok(lib, lib.astk_fill_dropout_mask(vp(r), n, a, seed, off, stream()))
        ref.append(r)
    ok(lib, lib.astk_fill_random(segs, len(spec), stream()))
    torch.cuda.synchronize()
    for f, r in zip(fused, ref):
        assert torch.equal(f, r)


def test_gemm_random_shapes_against_float64(lib, gemm_split):
    """Seeded sweep over layouts, ragged extents, leading-dimension padding (poisoned with NaN), batches and output modes."""
    rng = np.random.default_rng(2026)
    pad4 = lambda n: (n + 3) // 4 * 4
    for case in range(90):
        layout = int(rng.integers(0, 3))
        M, N = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        K = int(rng.choice([1, 3, 15, 16, 17, 31, 33, 64, 100, 257, 700]))
        batch = int(rng.choice([1, 1, 3]))
        mode = int(rng.integers(0, 3))
        extra = 4 * int(rng.integers(0, 3))
        A = rng.standard_normal((batch, M, K))
        B = rng.standard_normal((batch, N, K))
        ref = np.einsum("bmk,bnk->bmn", A, B)

        def store(X, transpose):                      # (batch, rows, cols) -> padded device array, NaN in the padding
            X = X.transpose(0, 2, 1) if transpose else X
            P = np.full((batch, X.shape[1], pad4(X.shape[2]) + extra), np.nan)
            P[:, :, :X.shape[2]] = X
            return P
        Ad, Bd = store(A, layout == 2), store(B, layout != 0)
        a, b = dev(Ad), dev(Bd)
        ldc = pad4(N) + extra
        c0 = rng.standard_normal((batch, M, ldc))
        c = dev(c0)
        bias = dev(rng.standard_normal(N)) if (mode == 0 and case % 2 == 0) else None
        ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[2], vp(b), Bd.shape[2], vp(c), ldc, vp(bias) if bias is not None else None,
                                  mode, 1, batch, Ad.shape[1] * Ad.shape[2], Bd.shape[1] * Bd.shape[2], M * ldc, stream()))
        want = ref + (bias.cpu().double().numpy() if bias is not None else 0.0) + (c0[:, :, :N] if mode != 0 else 0.0)
        msg = f"case {case}: layout {layout} M{M} N{N} K{K} batch {batch} mode {mode}"
        close(c[:, :, :N], want, rtol=2e-5, msg=msg)
        assert np.array_equal(c[:, :, N:].cpu().numpy(), c0[:, :, N:].astype(np.float32)), msg + ": wrote outside N"


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("M,N,K,batch", [(4100, 1150, 330, 1), (2100, 2100, 300, 1), (1100, 1200, 330, 4), (33000, 200, 200, 1)])
def test_gemm_hybrid_schedule_whole_tile_waves_and_stream_k_remainder(lib, layout, M, N, K, batch, gemm_split):
    """Products with more tiles than workgroups (round 5: hybrid schedule of the split schemes -- floor(tiles / 256) data-parallel waves of
    whole tiles in XCD-local blocks of the block tile order, then a stream-K split of the rest): ragged edges in M, N and K, every output
    mode, batches, a one-column-of-tiles shape (block order degenerates to tall blocks).  Against float64."""
    rng = np.random.default_rng(M + 3 * N + K + layout)
    pad4 = lambda n: (n + 3) // 4 * 4
    A = rng.standard_normal((batch, M, K)).astype(np.float32)
    B = rng.standard_normal((batch, N, K)).astype(np.float32)
    ref = np.einsum("bmk,bnk->bmn", A.astype(np.float64), B.astype(np.float64))

    def store(X, transpose):
        X = X.transpose(0, 2, 1) if transpose else X
        P = np.full((batch, X.shape[1], pad4(X.shape[2]) + 4), np.nan, np.float32)
        P[:, :, :X.shape[2]] = X
        return P
    Ad, Bd = store(A, layout == 2), store(B, layout != 0)
    a, b = dev(Ad), dev(Bd)
    ldc = pad4(N) + 4
    bias = rng.standard_normal(N)
    c = torch.full((batch, M, ldc), 7.0, device="cuda")
    sa, sb, sc = Ad.shape[1] * Ad.shape[2], Bd.shape[1] * Bd.shape[2], M * ldc
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[2], vp(b), Bd.shape[2], vp(c), ldc, vp(dev(bias)), 0, 1, batch, sa, sb, sc, stream()))
    close(c[:, :, :N], ref + bias, rtol=2e-5, msg="store")
    assert float(c[:, :, N:].min()) == 7.0 and float(c[:, :, N:].max()) == 7.0, "wrote outside N"
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[2], vp(b), Bd.shape[2], vp(c), ldc, None, 1, 1, batch, sa, sb, sc, stream()))
    close(c[:, :, :N], 2 * ref + bias, rtol=2e-5, msg="accum")
    c.zero_()
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[2], vp(b), Bd.shape[2], vp(c), ldc, None, 2, 1, batch, sa, sb, sc, stream()))
    close(c[:, :, :N], ref, rtol=2e-5, msg="atomic")
    assert float(c[:, :, N:].abs().max()) == 0.0, "wrote outside N"


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("M,N,K,mode", [(512, 1152, 38400, 2), (260, 200, 51200, 2), (512, 640, 24000, 1)])
def test_gemm_accumulating_products_of_few_tiles_and_deep_k(lib, layout, M, N, K, mode, gemm_split):
    """Weight-gradient shaped products (a handful of output tiles, thousands of k-iterations, GEMM_ATOMIC / GEMM_ACCUM): the stream-K
    ranges run CHUNK-major there (round 5: all tiles of one k-chunk, then the next chunk, so that the workgroups of an XCD share the
    operand lines of one k-range) -- every (tile, chunk) piece must be added exactly once, ragged M / N included.  Against float64."""
    rng = np.random.default_rng(M + N + K + layout)
    pad4 = lambda n: (n + 3) // 4 * 4
    A = (rng.standard_normal((M, K)) * 0.1).astype(np.float32)
    B = (rng.standard_normal((N, K)) * 0.1).astype(np.float32)
    ref = (torch.from_numpy(A).double().cuda() @ torch.from_numpy(B).double().cuda().T).cpu().numpy()

    def store(X, transpose):
        X = X.T if transpose else X
        P = np.zeros((X.shape[0], pad4(X.shape[1]) + 4), np.float32)
        P[:, :X.shape[1]] = X
        return P
    Ad, Bd = store(A, layout == 2), store(B, layout != 0)
    a, b = dev(Ad), dev(Bd)
    ldc = pad4(N) + 4
    c = torch.full((M, ldc), 0.5, device="cuda")
    for rep in range(2):
        ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[1], vp(b), Bd.shape[1], vp(c), ldc, None, mode, 1, 1, 0, 0, 0, stream()))
        close(c[:, :N], 0.5 + (rep + 1) * ref, rtol=3e-5, msg=f"pass {rep}")
        assert float(c[:, N:].min()) == 0.5 and float(c[:, N:].max()) == 0.5, "wrote outside N"


def _split_tiles_body(lib, M, N, K, reps):
    rng = np.random.default_rng(M + N + K)
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((N, K)).astype(np.float32)
    ref = (torch.from_numpy(A).double() @ torch.from_numpy(B).double().T).numpy()
    a, b = dev(A), dev(B)
    ldc = (N + 3) // 4 * 4 + 4
    for rep in range(reps):
        c = torch.full((M, ldc), float("nan"), device="cuda")
        ok(lib, lib.astk_gemm_f32(0, M, N, K, vp(a), K, vp(b), K, vp(c), ldc, None, 0, 1, 1, 0, 0, 0, stream()))
        assert bool(torch.isnan(c[:, N:]).all()), "wrote outside N"
        assert bool(torch.isfinite(c[:, :N]).all()), f"launch {rep}: a split tile was added onto what the buffer held"
        close(c[:, :N], ref, rtol=2e-5, msg=f"launch {rep}")


@pytest.mark.parametrize("M,N,K", [(4100, 1150, 332), (300, 260, 20000), (130, 70, 5000), (8200, 1930, 1100)])
def test_gemm_split_tiles_of_store_products_overwrite_what_the_buffer_held(lib, M, N, K, gemm_split):
    """Store-mode products whose tiles are shared by several workgroups (stream-K ranges: two contributors per tile in the first shape,
    tens in the deep ones; the last runs the 12-wave kernel under the default arithmetic) into NaN-poisoned outputs, several launches in
    a row: the split tiles are zeroed in front of the launch, the contributions are atomic adds."""
    _split_tiles_body(lib, M, N, K, 5)


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("M,N,K,mode", [(512, 1152, 38400, 2), (260, 200, 51200, 1), (4100, 1150, 332, 0), (1100, 3072, 1024, 0), (300, 260, 20000, 0)])
def test_gemm_deterministic_split_tiles_are_bit_reproducible_and_right(lib, tune, layout, M, N, K, mode):
    """The fix-up epilogue of deterministic calls (gemm.hip "Deterministic split tiles"; here through the process default gemm.deterministic):
    every contributor of a split tile leaves its accumulator block in the workspace, the last one sums the blocks in workgroup order and writes
    the tile.  Weight-gradient shapes (a few tiles, thousands of k-iterations, up to ~14 contributors), hybrid launches (whole-tile waves +
    stream-K remainder), store / accumulate / atomic output: (a) right against float64, (b) TEN launches give the same bits -- which the
    default schedule (float atomics in arrival order) does not promise for these shapes, (c) nothing outside N is written."""
    tune("gemm.deterministic", 1, lib)
    rng = np.random.default_rng(M + N + K + layout)
    pad4 = lambda n: (n + 3) // 4 * 4
    A = (rng.standard_normal((M, K)) * 0.1).astype(np.float32)
    B = (rng.standard_normal((N, K)) * 0.1).astype(np.float32)
    ref = (torch.from_numpy(A).double().cuda() @ torch.from_numpy(B).double().cuda().T).cpu().numpy()

    def store(X, transpose):
        X = X.T if transpose else X
        P = np.zeros((X.shape[0], pad4(X.shape[1]) + 4), np.float32)
        P[:, :X.shape[1]] = X
        return P
    Ad, Bd = store(A, layout == 2), store(B, layout != 0)
    a, b = dev(Ad), dev(Bd)
    ldc = pad4(N) + 4
    first = None
    for rep in range(10):
        c = torch.full((M, ldc), 0.5, device="cuda")
        ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[1], vp(b), Bd.shape[1], vp(c), ldc, None, mode, 1, 1, 0, 0, 0, stream()))
        if first is None:
            first = c.clone()
            close(c[:, :N], (0.5 if mode != 0 else 0.0) + ref, rtol=3e-5, msg=f"layout {layout} mode {mode}")
            assert float(c[:, N:].min()) == 0.5 and float(c[:, N:].max()) == 0.5, "wrote outside N"
        else:
            assert torch.equal(c, first), (rep, float((c - first).abs().max()))


@pytest.mark.parametrize("M,N,K", [(4100, 1150, 332), (300, 260, 20000), (130, 70, 5000), (8200, 1930, 1100)])
def test_gemm_split_tiles_ticket_protocol_on_the_instrumented_build(M, N, K):
    """The ticket protocol for the same tiles (round 5, gemm.hip "Split tiles without a zeroing launch": the first arrival at a split tile
    stores, the others add behind its DONE bit; measured against the zeroing launch and switched off in the product build, compiled IN in
    libastk_test.so).  Twenty launches in a row into the same poisoned buffer: a ticket word left non-zero by one launch would make the
    next one add onto the NaNs; tests/test_protocol_model.py enumerates the interleavings."""
    from ast_amd import _lib as L_
    with L_.load_test_hooks() as lib:
        _split_tiles_body(lib, M, N, K, 20)


@pytest.mark.parametrize("layout,shapes", [
    (0, [(256, 256, 16384)]),                                   # few tiles, deep K: without the rule 256 workgroups share four tiles
    (2, [(384, 128, 40000)]),
    (0, [(1248, 512, 512), (1248, 512, 1152), (640, 1024, 3072)]),      # a group of unequal K (not uniform: outside the hybrid branch)
    (1, [(2000, 640, 256), (700, 384, 2048)]),
    (0, [(38400, 512, 1152)]),                                  # the hybrid branch itself (the step's layer-1 convolution)
])
def test_gemm_forward_launches_have_two_contributors_per_split_tile_on_any_shape(layout, shapes):
    """GemmForwardScope (common.h) promises the forward ops run-to-run identical sums: every split tile of their launches has at most two
    contributors (two float atomic adds into a zeroed tile commute).  Round 5 kept the promise only inside the hybrid branch; since round 6
    the launcher shrinks the grid of every other forward launch until a stream-K range is at least one tile deep.  Shapes no op of the step
    produces -- few tiles with deep K, grouped products of unequal K -- go through the instrumented build's astk_debug_gemm_group (one
    grouped launch under the scope): twelve launches must agree BIT FOR BIT, and with float64.  The same launches without the scope are run
    once for their values (their sums are allowed to vary)."""
    from ast_amd import _lib as L_
    torch.manual_seed(11)
    n = len(shapes)
    As, Bs, refs = [], [], []
    for M, N, K in shapes:
        a = torch.randn((K, M) if layout == 2 else (M, K), device="cuda")
        b = torch.randn((N, K) if layout == 0 else (K, N), device="cuda")
        As.append(a); Bs.append(b)
        ad, bd = a.double(), b.double()
        refs.append((ad.t() if layout == 2 else ad) @ (bd.t() if layout == 0 else bd))
    arr = lambda vals: (C.c_int32 * n)(*vals)
    ptrs = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    with L_.load_test_hooks() as tl:
        for forward in (1, 0):
            first = None
            for rep in range(12 if forward else 1):
                Cs = [torch.full((M, N), float("nan"), device="cuda") for M, N, K in shapes]
                ok(tl, tl.astk_debug_gemm_group(layout, n, arr([s[0] for s in shapes]), arr([s[1] for s in shapes]), arr([s[2] for s in shapes]),
                                                ptrs(As), ptrs(Bs), ptrs(Cs), forward, L_.PREC_BF16X3, stream()))
                torch.cuda.synchronize()
                if first is None:
                    first = [c.clone() for c in Cs]
                    for c, r, sh in zip(Cs, refs, shapes):
                        close(c, r, rtol=3e-5, msg=f"layout {layout} {sh} forward {forward}")
                else:
                    for c, f, sh in zip(Cs, first, shapes):
                        assert torch.equal(c, f), (rep, sh, float((c - f).abs().max()))


@pytest.mark.parametrize("layout,M,N,K", [(0, 256, 256, 16384), (2, 384, 128, 40000), (1, 1200, 300, 6000), (0, 38400, 512, 1152)])
def test_gemm_forward_rule_on_the_product_library_is_bit_reproducible(lib, tune, layout, M, N, K):
    """The same promise on the SHIPPED library (zeroing launch + float atomics instead of the instrumented build's ticket protocol):
    `gemm.forward_pairs` = 2 puts every launch under the forward ops' rule, so plain astk_gemm_f32 calls reach it.  Twelve launches of a
    few-tiles / deep-K product (256 workgroups would share its tiles without the rule) agree bit for bit."""
    tune("gemm.forward_pairs", 2, lib)
    torch.manual_seed(12)
    a = torch.randn((K, M) if layout == 2 else (M, K), device="cuda")
    b = torch.randn((N, K) if layout == 0 else (K, N), device="cuda")
    ref = (a.double().t() if layout == 2 else a.double()) @ (b.double().t() if layout == 0 else b.double())
    first = None
    for rep in range(12):
        c = torch.full((M, N), float("nan"), device="cuda")
        ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), a.shape[1], vp(b), b.shape[1], vp(c), N, None, 0, 1, 1, 0, 0, 0, stream()))
        torch.cuda.synchronize()
        if first is None:
            first = c.clone()
            close(c, ref, rtol=3e-5, msg=f"layout {layout} {M}x{N}x{K}")
        else:
            assert torch.equal(c, first), (rep, float((c - first).abs().max()))


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_gemm_twelve_wave_256x128_kernel_on_a_big_ragged_product(lib, layout):
    """Launches of 20 GFLOP and more run 256 x 128 tiles on the 12-wave kernel (8 multiplying + 4 staging waves, round 5) under the default
    arithmetic: one such product per layout with ragged M (8200 = 32 tiles + 8 rows), N (1930) and K (1100), store / atomic modes, a bias,
    against float64 at the tolerance of the seeded sweep."""
    assert lib.astk_get_gemm_precision() == 1
    M, N, K = 8200, 1930, 1100
    assert 2.0 * M * N * K >= 2e10
    rng = np.random.default_rng(500 + layout)
    pad4 = lambda n: (n + 3) // 4 * 4
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((N, K)).astype(np.float32)
    bias = rng.standard_normal(N)
    ref = torch.from_numpy(A).double() @ torch.from_numpy(B).double().T
    ref = ref.numpy()

    def store(X, transpose):
        X = X.T if transpose else X
        P = np.full((X.shape[0], pad4(X.shape[1]) + 4), np.nan, np.float32)
        P[:, :X.shape[1]] = X
        return P
    Ad, Bd = store(A, layout == 2), store(B, layout != 0)
    a, b = dev(Ad), dev(Bd)
    ldc = pad4(N) + 4
    c = torch.full((M, ldc), 7.0, device="cuda")
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[1], vp(b), Bd.shape[1], vp(c), ldc, vp(dev(bias)), 0, 1, 1, 0, 0, 0, stream()))
    close(c[:, :N], ref + bias, rtol=2e-5, msg="store")
    assert float(c[:, N:].min()) == 7.0 and float(c[:, N:].max()) == 7.0, "wrote outside N"
    c.zero_()
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[1], vp(b), Bd.shape[1], vp(c), ldc, None, 2, 1, 1, 0, 0, 0, stream()))
    close(c[:, :N], ref, rtol=2e-5, msg="atomic")
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[1], vp(b), Bd.shape[1], vp(c), ldc, None, 1, 1, 1, 0, 0, 0, stream()))
    close(c[:, :N], 2 * ref, rtol=2e-5, msg="accum")


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("knob,value,K,rtol", [("gemm.tile", 64, 100, 2e-5), ("gemm.tile", 128, 100, 2e-5), ("gemm.tile", 256, 100, 2e-5),
                                               ("gemm.grid", 24, 1000, 3e-5)])
def test_gemm_forced_tile_and_forced_grid_on_a_ragged_product(lib, tune, layout, knob, value, K, rtol):
    """The launcher's tuning overrides, which no other test sets: "gemm.tile" 64 | 128 | 256 on a ragged 300 x 260 x 100 product that would
    take 64-tiles by itself (tests/test_gemm_plan_host.py force64 / force128 / force256: 25, 9 and 6 whole tiles), and "gemm.grid" 24 on
    300 x 260 x 1000 (forced-grid: 24 workgroups over 25 tiles of 63 k-iterations, every tile split, zeroed first).  Store mode into a
    poisoned buffer, against float64 at the bounds of the 12-wave test and of the split-tile tests."""
    assert lib.astk_get_gemm_precision() == 1
    tune(knob, value, lib)
    M, N = 300, 260
    rng = np.random.default_rng(900 + layout + K)
    pad4 = lambda n: (n + 3) // 4 * 4
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((N, K)).astype(np.float32)
    ref = (torch.from_numpy(A).double() @ torch.from_numpy(B).double().T).numpy()

    def store(X, transpose):
        X = X.T if transpose else X
        P = np.full((X.shape[0], pad4(X.shape[1]) + 4), np.nan, np.float32)
        P[:, :X.shape[1]] = X
        return P
    Ad, Bd = store(A, layout == 2), store(B, layout != 0)
    a, b = dev(Ad), dev(Bd)
    ldc = pad4(N) + 4
    c = torch.full((M, ldc), float("nan"), device="cuda")
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[1], vp(b), Bd.shape[1], vp(c), ldc, None, 0, 1, 1, 0, 0, 0, stream()))
    close(c[:, :N], ref, rtol=rtol, msg=f"{knob} {value} layout {layout}")
    assert bool(torch.isnan(c[:, N:]).all()), "wrote outside N"


@pytest.mark.parametrize("variant", ["scalar-zeroing", "det-clipped-grid", "det-f32-whole-tiles"])
def test_gemm_split_tile_handling_no_other_test_launches(lib, tune, variant):
    """Three split-tile decisions of the launcher on 4100 x 1150 x 332 (NT, store mode; tests/test_gemm_plan_host.py zero-scalar,
    det-clipped, det-f32), each one launch shape no other test produces.  "scalar-zeroing": an output whose ldc (1150) is no multiple
    of 4 -- the split tiles are zeroed with scalar stores (zero_vec = 0); every other split-tile test pads ldc to 16 bytes.
    "det-clipped-grid": deterministic mode with "gemm.grid" 512 -- the grid is clipped to the 256 workgroups the fix-up workspace
    serves.  "det-f32-whole-tiles": deterministic mode under the f32 scheme, which has no fix-up kernel -- one whole tile per
    workgroup.  Store into a NaN-poisoned buffer with a guard band behind it, against float64 at the split-tile tests' bound; the
    deterministic variants four times, bit for bit."""
    from ast_amd import _lib as L_
    assert lib.astk_get_gemm_precision() == 1
    M, N, K = 4100, 1150, 332
    rng = np.random.default_rng(4100 + 1150 + 332)
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((N, K)).astype(np.float32)
    ref = (torch.from_numpy(A).double() @ torch.from_numpy(B).double().T).numpy()
    a, b = dev(A), dev(B)
    det = variant != "scalar-zeroing"
    if det:
        tune("gemm.deterministic", 1, lib)
    if variant == "det-clipped-grid":
        tune("gemm.grid", 512, lib)
    ldc = N if variant == "scalar-zeroing" else (N + 3) // 4 * 4 + 4
    prec = L_.PREC_F32 if variant == "det-f32-whole-tiles" else L_.PREC_DEFAULT
    guard = 4096
    first = None
    for rep in range(4 if det else 2):
        buf = torch.full((M * ldc + guard,), float("nan"), device="cuda")
        c = buf[:M * ldc].view(M, ldc)
        ok(lib, lib.astk_gemm_f32_ex(0, M, N, K, vp(a), K, vp(b), K, vp(c), ldc, None, 0, 1, 1, 0, 0, 0, prec, stream()))
        assert bool(torch.isnan(buf[M * ldc:]).all()) and bool(torch.isnan(c[:, N:]).all()), "wrote outside the result"
        if first is None:
            first = c.clone()
            close(c[:, :N], ref, rtol=3e-5, msg=variant)
        elif det:
            assert torch.equal(c[:, :N], first[:, :N]), (variant, rep, float((c[:, :N] - first[:, :N]).abs().max()))
        else:
            close(c[:, :N], ref, rtol=3e-5, msg=f"{variant} launch {rep}")


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("sa,sb", [(1e-20, 1e15), (3e7, 2e-3), (1.0, 1e-30)])
def test_gemm_operand_magnitudes(lib, layout, sa, sb, gemm_split):
    """The default GEMM splits every operand into two fp16 terms behind a per-operand power-of-two scale taken from an absolute-maximum
    pass: operands far outside fp16's range must come out as accurately as N(0,1) ones, and rows 1e-4 below the operand's largest
    entries must keep their own relative accuracy (22 significant bits down to 2^-17 of the maximum, gemm.hip)."""
    rng = np.random.default_rng(int(abs(np.log10(sa))) + 31 * layout)
    M, N, K = 150, 130, 333
    rowscale = 10.0 ** (-(np.arange(M) % 5))
    A = rng.standard_normal((M, K)) * rowscale[:, None] * sa
    B = rng.standard_normal((N, K)) * sb
    A32, B32 = A.astype(np.float32).astype(np.float64), B.astype(np.float32).astype(np.float64)
    ref = A32 @ B32.T
    pad = lambda n: (n + 3) // 4 * 4
    def store(X, transpose):
        X = X.T if transpose else X
        P = np.zeros((X.shape[0], pad(X.shape[1])))
        P[:, :X.shape[1]] = X
        return P
    Ad, Bd = store(A32, layout == 2), store(B32, layout != 0)
    a, b = dev(Ad), dev(Bd)
    c = torch.zeros(M, pad(N), device="cuda")
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[1], vp(b), Bd.shape[1], vp(c), c.shape[1], None, 0, 1, 1, 0, 0, 0, stream()))
    got = c[:, :N].cpu().double().numpy()
    rowmax = np.abs(ref).max(axis=1)
    err = np.abs(got - ref).max(axis=1) / rowmax
    assert np.isfinite(got).all()
    assert err.max() < 2e-5, (layout, sa, sb, err.max(), int(err.argmax()))


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("M,N,K,sigma", [(1024, 1536, 2048, 2.5), (1024, 6400, 1024, 2.5), (1024, 1536, 2048, 3.5)])
def test_gemm_heavy_tailed_operands_every_scheme_against_the_exact_f32_kernel(lib, layout, M, N, K, sigma):
    """fp16x2 on hard data: log-normal magnitudes INSIDE every row and column of both operands (trained weights and BPTT gradients are
    heavy-tailed within rows; round-2's test spread whole rows).  The same product under the two-term fp16 split, the three-term bf16
    split and the exact-f32 MFMA chain (astk_set_gemm_precision), each against float64, element by element relative to the natural
    scale of the entry, sum_k |a_ik| |b_jk|.
      sigma = 2.5 nats: six to eight decades inside every row and column (median 7), eleven over an operand: the fp16 split must be at
        most twice as far off as the f32 kernel (it is closer: 22-bit products summed in wider blocks).
      sigma = 3.5 nats: nine decades inside a row, FIFTEEN (2^50) over an operand -- beyond the scheme's domain: one power-of-two scale per
        operand puts its largest entry at 2^15, an entry keeps all 22 bits down to 2^-17 of that maximum and 11 bits down to 2^-29
        (gemm.hip); here the MEDIAN entry sits 2^-25 below the maximum.  The error grows to 1e-4 .. 1e-3 of the entry's scale and the
        test pins that bound -- and that the bf16x3 scheme (no scales: bf16 has f32's exponent range), which astk_set_gemm_precision(1)
        selects at run time, is as accurate as the f32 kernel on the same data."""
    rng = np.random.default_rng(1000 * layout + M)
    def heavy(r, c):
        mag = np.exp(rng.normal(0.0, sigma, size=(r, c)))
        return (mag * rng.choice([-1.0, 1.0], size=(r, c))).astype(np.float32)
    A, Bm = heavy(M, K), heavy(N, K)
    for X in (A, Bm):
        for axis in (0, 1):
            dec = np.log10(np.abs(X).max(axis) / np.abs(X).min(axis))
            assert dec.min() > 5.5 and np.median(dec) > 6.5, (axis, dec.min(), np.median(dec))
    a64, b64 = torch.from_numpy(A).cuda().double(), torch.from_numpy(Bm).cuda().double()
    ref = a64 @ b64.T
    scale = a64.abs() @ b64.abs().T
    Ad = torch.from_numpy(A.T.copy() if layout == 2 else A).cuda()
    Bd = torch.from_numpy(Bm.T.copy() if layout != 0 else Bm).cuda()
    errs = {}
    from ast_amd import _lib as L_
    below = lib.astk_set_gemm_bf16_split_below(C.c_double(0.0))       # fp16x2 whatever the size
    try:
        # per-call arithmetic (astk_gemm_f32_ex: the `precision` every descriptor carries), and the process default last
        for name, prec in (("fp16x2", L_.PREC_FP16X2), ("bf16x3", L_.PREC_BF16X3), ("f32", L_.PREC_F32), ("default", L_.PREC_DEFAULT)):
            c = torch.empty(M, N, device="cuda")
            ok(lib, lib.astk_gemm_f32_ex(layout, M, N, K, vp(Ad), Ad.shape[1], vp(Bd), Bd.shape[1], vp(c), N, None, 0, 1, 1, 0, 0, 0, prec, stream()))
            assert bool(torch.isfinite(c).all())
            errs[name] = float(((c.double() - ref).abs() / scale).max())
            if name == "bf16x3":
                c_x3 = c
            if name == "default":
                assert torch.equal(c, c_x3), "ASTK_PREC_DEFAULT must resolve to bf16x3"
    finally:
        lib.astk_set_gemm_bf16_split_below(C.c_double(below))
    print("heavy-tailed GEMM errors (relative to sum |a||b|):", sigma, errs)
    assert lib.astk_get_gemm_precision() == 1
    assert errs["f32"] < 4e-6, errs
    assert errs["bf16x3"] <= 2.0 * errs["f32"], errs
    # THE DEFAULT ARITHMETIC is f32-equivalent on any data, sigma = 3.5 included (round-3 review, item 1a)
    assert errs["default"] <= 2.0 * errs["f32"], errs
    if sigma <= 2.5:
        assert errs["fp16x2"] <= 2.0 * errs["f32"], errs
    else:
        assert errs["fp16x2"] < 2e-3, errs       # the opt-in scheme's documented domain limit


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", [(7, 5, 3), (9, 6, 2), (33, 3, 7), (5, 3, 1), (130, 66, 19)])
def test_gemm_maximum_in_the_ragged_tail(lib, layout, M, N, K, gemm_split):
    """The operand scales of the fp16x2 GEMMs come from an absolute-maximum pass that reads rows in float4 quads plus a scalar tail: an
    operand whose largest entries sit in the last (non-multiple-of-4) positions of its rows must still be scaled by them -- a maximum
    taken too small overflows fp16 and the result is inf / NaN."""
    rng = np.random.default_rng(M * 131 + N * 17 + K + layout)
    A = rng.standard_normal((M, K)) * 1e-3
    B = rng.standard_normal((N, K)) * 1e-3
    A[:, K - 1] = 500.0 * (1 + rng.random(M))        # last k of every row
    A[M - 1, :] *= 3.0                                # ... and the last row
    B[N - 1, :] = 800.0 * (1 + rng.random(K))        # last row of B = last column of B^T
    B[:, K - 1] += 300.0
    A32, B32 = A.astype(np.float32).astype(np.float64), B.astype(np.float32).astype(np.float64)
    ref = A32 @ B32.T
    pad = lambda n: (n + 3) // 4 * 4
    def store(X, transpose):
        X = X.T if transpose else X
        P = np.zeros((X.shape[0], pad(X.shape[1])))
        P[:, :X.shape[1]] = X
        return P
    Ad, Bd = store(A32, layout == 2), store(B32, layout != 0)
    a, b = dev(Ad), dev(Bd)
    c = torch.zeros(M, pad(N), device="cuda")
    ok(lib, lib.astk_gemm_f32(layout, M, N, K, vp(a), Ad.shape[1], vp(b), Bd.shape[1], vp(c), c.shape[1], None, 0, 1, 1, 0, 0, 0, stream()))
    got = c[:, :N].cpu().double().numpy()
    assert np.isfinite(got).all(), (layout, M, N, K)
    close(got, ref, rtol=2e-5, msg=f"layout {layout} {M}x{N}x{K}")


def test_gemm_scale_slots_survive_ring_wraparound(lib):
    """The fp16x2 GEMMs keep their operands' absolute maxima in a ring of generation-tagged slots that is never cleared (gemm.hip):
    a launch must never pick up the scale of an earlier user of its slots.  1500 launches (the ring holds the slots of ~21) whose
    operand magnitudes jump by random powers of two -- an inherited maximum that is too small overflows fp16 (inf / NaN), one that is
    too large costs accuracy -- and whose operands are small and large matrices in turn (different numbers of maximum blocks, hence
    of shards written per slot), each result checked against float64."""
    rng = np.random.default_rng(77)
    shapes = [(1024, 1024, 1536), (2048, 512, 1600), (96, 8192, 2048)]          # all above the bf16x3 threshold (3 GFLOP)
    base = {}
    for (M, N, K) in shapes:
        a = torch.randn(M, K, device="cuda", generator=torch.Generator(device="cuda").manual_seed(M + K))
        b = torch.randn(N, K, device="cuda", generator=torch.Generator(device="cuda").manual_seed(N + K + 1))
        base[(M, N, K)] = (a, b, a.double() @ b.double().T)
    worst = 0.0
    for it in range(1500):
        M, N, K = shapes[int(rng.integers(0, len(shapes)))]
        a0, b0, ref0 = base[(M, N, K)]
        ea, eb = int(rng.integers(-40, 30)), int(rng.integers(-40, 30))
        a, b = a0 * (2.0 ** ea), b0 * (2.0 ** eb)
        c = torch.empty(M, N, device="cuda")
        ok(lib, lib.astk_gemm_f32_ex(0, M, N, K, vp(a), K, vp(b), K, vp(c), N, None, 0, 1, 1, 0, 0, 0, 1, stream()))      # ASTK_PREC_FP16X2
        if it % 10 == 0 or it > 1480:           # (every launch runs; every tenth is compared)
            got = c.double() * (2.0 ** -(ea + eb))
            assert bool(torch.isfinite(got).all()), (it, M, N, K, ea, eb)
            err = float((got - ref0).abs().max() / ref0.abs().max())
            worst = max(worst, err)
            assert err < 2e-5, (it, M, N, K, ea, eb, err)
    assert worst > 0.0


def test_gemm_scale_generation_counter_survives_its_32_bit_wrap():
    """The generation tag of the fp16x2 scale slots is the high half of a 64-bit atomicMax word; a tag that wrapped to a small value would lose
    to every stale word and freeze the scales (a week of training at ~40 passes per step).  The counter is preset 40 generations short
    of the wrap threshold: 120 launches whose operand magnitudes jump by up to 2^60 run across it and every result is checked -- a stale
    (larger or smaller) maximum shows as inf / NaN or as lost bits.  The preset is a test hook: it exists in libastk_test.so only."""
    from ast_amd import _lib as L_
    rng = np.random.default_rng(78)
    M, N, K = 1024, 1024, 1536
    a0 = torch.randn(M, K, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    b0 = torch.randn(N, K, device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    ref0 = a0.double() @ b0.double().T
    with L_.load_test_hooks() as lib:
        assert lib.astk_debug_set_amax_generation(0xFFFFFF00 - 40) == 0
        try:
            for it in range(120):
                ea, eb = int(rng.integers(-30, 30)), int(rng.integers(-30, 30))
                a, b = a0 * (2.0 ** ea), b0 * (2.0 ** eb)
                c = torch.empty(M, N, device="cuda")
                ok(lib, lib.astk_gemm_f32_ex(0, M, N, K, vp(a), K, vp(b), K, vp(c), N, None, 0, 1, 1, 0, 0, 0, L_.PREC_FP16X2, stream()))
                got = c.double() * (2.0 ** -(ea + eb))
                assert bool(torch.isfinite(got).all()), (it, ea, eb)
                err = float((got - ref0).abs().max() / ref0.abs().max())
                assert err < 2e-5, (it, ea, eb, err)
        finally:
            torch.cuda.synchronize()


def test_optimizer_grad_scale_equals_scaling_first(lib):
    """astk_*_scaled read the gradient as grad_scale * g (the 1/world mean of data parallelism applied on the fly, rounded like a
    separate scaling pass would round it): same result as scaling the buffer first and calling the unscaled entry points, up to the
    summation order of the float64 norm (atomics), which can move the clip factor by an ulp."""
    n, gs, l2, clip = 100003, float(np.float32(1.0 / 3.0)), 1e-4, 2.0     # not a power of two: the product rounds
    g = torch.Generator(device="cuda").manual_seed(4)
    p0 = torch.randn(n, device="cuda", generator=g)
    grad = torch.randn(n, device="cuda", generator=g) * 3
    res = []
    for scaled in (False, True):
        p, m, v, vh = p0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        gr = grad.clone() if scaled else grad * gs
        sq = torch.zeros(1, dtype=torch.float64, device="cuda")
        for t in range(1, 4):
            lr_t = 1e-3 * (1 - 0.999 ** t) ** 0.5 / (1 - 0.9 ** t)
            if scaled:
                ok(lib, lib.astk_grad_sqnorm_scaled(vp(gr), vp(p), gs, l2, n, vp(sq), stream()))
                ok(lib, lib.astk_decay_clip_amsgrad_step_scaled(vp(p), vp(gr), vp(m), vp(v), vp(vh), n, gs, l2, clip, vp(sq), lr_t, 0.9, 0.999, 1e-8, 1, stream()))
            else:
                ok(lib, lib.astk_grad_sqnorm(vp(gr), vp(p), l2, n, vp(sq), stream()))
                ok(lib, lib.astk_decay_clip_amsgrad_step(vp(p), vp(gr), vp(m), vp(v), vp(vh), n, l2, clip, vp(sq), lr_t, 0.9, 0.999, 1e-8, 1, stream()))
        res.append((p.clone(), float(sq.item())))
    assert abs(res[0][1] - res[1][1]) <= 1e-7 * res[0][1]
    assert float((res[0][0] - res[1][0]).abs().max()) <= 1e-6 * float(res[0][0].abs().max())
    ps = [p0.clone(), p0.clone()]
    sq = torch.zeros(1, dtype=torch.float64, device="cuda")
    gsc = grad * gs
    ok(lib, lib.astk_grad_sqnorm(vp(gsc), vp(ps[0]), l2, n, vp(sq), stream()))
    ok(lib, lib.astk_decay_clip_sgd_step(vp(ps[0]), vp(gsc), n, l2, clip, vp(sq), 0.05, stream()))
    ok(lib, lib.astk_decay_clip_sgd_step_scaled(vp(ps[1]), vp(grad), n, gs, l2, clip, vp(sq), 0.05, stream()))
    assert torch.equal(ps[0], ps[1])          # one norm, one clip factor: here the two paths are bit-identical


def test_spin_keeps_the_stream_busy(lib):
    """astk_spin: the concurrency probe's tool -- one wave busy for the requested time, then a flag increment."""
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    ok(lib, lib.astk_spin(500, vp(flag), stream()))
    e1.record()
    torch.cuda.synchronize()
    assert int(flag.item()) == 1 and 0.4 <= e0.elapsed_time(e1) <= 5.0
    assert lib.astk_spin(200000, None, stream()) != 0          # bounded: at most 100 ms


def test_zero_frames_on_device_follows_the_loaders_rule(lib):
    """dataloader.py:83-93 on the device (astk_zero_frames): utterance b loses int(rate * T_b) frames drawn WITH replacement from its own
    T_b frames -- never more than that many, at least one when n >= 1, never a padding row; whole frames; a different counter offset
    draws different frames; and the number of distinct frames hit follows the with-replacement law (mean n_distinct = T (1 - (1 - 1/T)^n))."""
    lens = np.array([400, 57, 80, 33, 9, 250], dtype=np.int32)
    B, T, D, rate = len(lens), 400, 13, 0.1
    X = torch.ones(B, T, D, device="cuda")
    ld = dev(lens, torch.int32)
    ok(lib, lib.astk_zero_frames(vp(X), B, T, D, vp(ld), rate, 1234, 0, stream()))
    x = X.cpu().numpy()
    rows0 = []
    for b, n_b in enumerate(lens):
        n = int(rate * n_b)
        zero_rows = np.where((x[b] == 0).all(axis=1))[0]
        partly = ((x[b] == 0).any(axis=1) & ~(x[b] == 0).all(axis=1)).sum()
        assert partly == 0 and len(zero_rows) <= n and (n == 0 or len(zero_rows) >= 1), (b, len(zero_rows), n)
        assert (zero_rows < n_b).all()
        rows0.append(set(zero_rows.tolist()))
    X2 = torch.ones(B, T, D, device="cuda")
    ok(lib, lib.astk_zero_frames(vp(X2), B, T, D, vp(ld), rate, 1234, B * T, stream()))
    assert set(np.where((X2[0].cpu().numpy() == 0).all(axis=1))[0].tolist()) != rows0[0]
    # with-replacement law over many draws: T = 400, n = 40 -> 38.1 distinct frames on average
    tot = 0
    for k in range(50):
        Xk = torch.ones(1, T, D, device="cuda")
        ok(lib, lib.astk_zero_frames(vp(Xk), 1, T, D, vp(ld), rate, 99, k * T, stream()))
        tot += int((Xk[0, :, 0] == 0).sum())
    assert abs(tot / 50 - 400 * (1 - (1 - 1 / 400) ** 40)) < 1.0


def test_gradient_noise_hook_follows_the_other_two(lib):
    """nn.py:108-110: GradientNoise(eta) behind WeightDecay and GradientClipping (insertion order, A7).  Same gradients with and without
    the hook: what is left in the gradient arena after update() is clip(g + l2 p) + noise, and the noise has mean 0 and variance
    eta / (1 + t)^0.55 with the optimizer's count BEFORE the update (t = 0 at the first update: Chainer runs the hooks, then increments t)."""
    import math
    from ast_amd import optimizers as O
    from ast_amd.params import ParamArena

    class _M:
        def __init__(self):
            self.arena = ParamArena({"a/W": (300, 400), "b/W": (50001,)}, torch.device("cuda"))
        def enabled_ranges(self):
            return [(0, self.arena.size)]
    gen = torch.Generator(device="cuda").manual_seed(1)
    m0, m1 = _M(), _M()
    p0 = torch.randn(m0.arena.size, device="cuda", generator=gen)
    eta, l2, clip = 0.3, 1e-2, 5.0
    opts = []
    for m, noisy in ((m0, False), (m1, True)):
        m.arena.data.copy_(p0)
        o = O.Adam(alpha=1e-3, amsgrad=True).setup(m)
        o.add_hook(O.WeightDecay(l2))
        o.add_hook(O.GradientClipping(clip))
        if noisy:
            o.add_hook(O.GradientNoise(eta))
        opts.append(o)
    for step in (1, 2):
        g = torch.randn(m0.arena.size, device="cuda", generator=gen) * 0.05
        for m, o in zip((m0, m1), opts):
            m.arena.grad.copy_(g)
            pb = m.arena.data.clone()
            o.update()
            if o is opts[0]:
                norm = o.last_grad_norm
                want = (g + l2 * pb) * min(1.0, clip / norm)
        noise = m1.arena.grad - want if step == 1 else None
        if step == 1:
            assert torch.equal(m0.arena.grad, g)                              # without the hook the arena keeps the raw gradient
            sig = math.sqrt(eta / 1.0 ** 0.55)
            assert abs(float(noise.mean())) < 5 * sig / math.sqrt(noise.numel())
            assert abs(float(noise.std()) - sig) < 0.01 * sig
    assert float((m1.arena.data - m0.arena.data).abs().max()) > 0             # the noise reached the update
