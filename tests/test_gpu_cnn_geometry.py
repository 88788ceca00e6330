"""GPU parity tests of the CNN front-end over its GEOMETRY: kernel, stride, time pad and layer count.  astk_cnn_desc takes 1 to 4 layers,
any layer-0 kernel (kt, kf) / stride (st, sf) / time pad, any (kt, 1) kernel with st <= kt above layer 0 and optional max-pooling; every
other CNN test of the suite runs the one shipped geometry ((9, 13) / (2, 13) / 4, then (9, 1) / (2, 1) / 4, two layers), where sf == kf
and the stride-phase decomposition of the input gradient sees two phases only.  Here tests/test_gpu_ops.py's operator case (_cnn_case:
output, every layer's W / gamma / beta gradient, running statistics of every layer, workspace guards, input intact, a second backward call
and a fresh forward + backward, eval mode) runs on the geometries of tests/range_cases.py CNN_GEOMETRY_CASES under the three arithmetic
schemes -- bf16x3 puts the direct-eligible layer-0 shapes on the direct kernel (proved by the path probe), f32 / fp16x2 put the same
geometry on im2col + GEMM -- with the suite's bounds: 2e-4 output and statistics, 5e-4 every gradient (the cases' seeds leave no unit near
the ReLU's kink, asserted), 2e-5 between repeated backward calls.  Then: max-pooling on a direct-eligible layer 0, the descriptor's
refusals, and three whole train steps on other stacks against the float64 oracle.  The two geometries whose last layer takes the tiled
sequence re-layout and the sequence-layout BatchNorm backward also run with those routes switched off ("conv.seq_fwd", "conv.seq_bwd")."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import range_cases as RC
from conftest import tiny_cfg
from test_gpu_ops import _cnn_case, _cnn_desc, gemm_split, lib  # noqa: F401  (the two fixtures)

pytestmark = pytest.mark.gpu

# the ids whose layer 0 is meant for the direct kernel under bf16x3 (the others: kt > 9 / kf > 14 / odd stride, stride 1 and 4 channels)
DIRECT_IDS = {"kt5-kf8-l1s1", "kf14-sf7-pt0", "gaps-pt6-l1s3", "kt2-st2", "kf1", "two-tiles", "one-layer", "three-layers", "four-layers",
              "one-layer-c64", "f10-c64-last", "f20-kf4"}


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("cid,B,T,D,layers,seed,seed_noisy", RC.CNN_GEOMETRY_CASES, ids=[c[0] for c in RC.CNN_GEOMETRY_CASES])
def test_cnn_geometry_fwd_bwd(lib, cid, B, T, D, layers, seed, seed_noisy, with_noise, gemm_split):
    """One geometry (what each reaches: the table's comment in tests/range_cases.py).  The path probe's answer is held against the
    restatement of conv.hip's conv0_direct_shape AND against the intent written down above."""
    shape_direct = RC.conv0_direct_shape(layers)
    assert shape_direct == (cid in DIRECT_IDS), "the case no longer reaches the layer-0 kernel it was written for"
    _cnn_case(lib, B, T, D, None, None, with_noise, seed=seed_noisy if with_noise else seed, layers=layers, all_stats=True, kink_free=True,
              expect_direct=shape_direct and gemm_split == "bf16x3")


@pytest.mark.parametrize("B,T,D,c0,c1,pool", RC.CNN_POOL_DIRECT_CASES)
def test_cnn_max_pool_on_a_direct_eligible_layer0(lib, B, T, D, c0, c1, pool, gemm_split):
    """Max-pooling between the convolution and its BatchNorm on a layer 0 with 16 channels of the shipped geometry -- the shape the
    direct kernel takes under the default arithmetic, with BatchNorm statistics fused into it: sums over the UN-pooled output.  A pooled
    layer's BatchNorm normalises the pooled rows, so a pooled layer 0 (a `-1` = whole-extent window included) must take im2col + GEMM;
    the probe shows it does.  Output, all gradients and the running statistics of both layers against the float64 reference."""
    layers = RC.shipped_layers(c0, c1)
    assert RC.conv0_direct_shape(layers) and not RC.conv0_direct_shape(layers, pool)
    _cnn_case(lib, B, T, D, c0, c1, False, pool=pool, all_stats=True, expect_direct=False)


# ------------------------------------------------------------------ the last layer's routes with their knobs off
SEQ_IDS = ["one-layer-c64", "f10-c64-last"]             # the geometries that take k_bn_relu_to_seq_tiled and k_bn_bwd_*_seq by default
SEQ_KNOBS_OFF = [("conv.seq_fwd",), ("conv.seq_bwd",), ("conv.seq_fwd", "conv.seq_bwd")]


def _geometry(cid):
    return next(c for c in RC.CNN_GEOMETRY_CASES if c[0] == cid)


@contextlib.contextmanager
def _knobs_off(lib, names):
    prev = {k: C.c_double() for k in names}
    try:
        for k, v in prev.items():
            assert lib.astk_get_tuning(k.encode(), C.byref(v)) == 0 and v.value == 1, k
            assert lib.astk_set_tuning(k.encode(), 0.0) == 0, k
        yield
    finally:
        for k, v in prev.items():
            assert lib.astk_set_tuning(k.encode(), v.value) == 0, k


@pytest.mark.parametrize("off", SEQ_KNOBS_OFF, ids=["+".join(k.split(".")[1] for k in ks) + "-off" for ks in SEQ_KNOBS_OFF])
@pytest.mark.parametrize("cid", SEQ_IDS)
def test_cnn_seq_routes_with_knobs_off(lib, cid, off, gemm_split):
    """The un-tiled re-layout (k_bn_relu_to_seq) and the row-layout BatchNorm backward (k_seq_to_rows + k_bn_bwd_stats / _apply) on shapes
    that take the tiled / sequence-layout kernels by default -- the routes no other operator test reaches: the same operator case, the
    same float64 reference, the same bounds."""
    _, B, T, D, layers, seed, _ = _geometry(cid)
    with _knobs_off(lib, off):
        _cnn_case(lib, B, T, D, None, None, False, seed=seed, layers=layers, all_stats=True, kink_free=True,
                  expect_direct=gemm_split == "bf16x3")


@pytest.mark.parametrize("cid", SEQ_IDS)
def test_cnn_tiled_relayout_equals_untiled(lib, cid, gemm_split):
    """k_bn_relu_to_seq_tiled and k_bn_relu_to_seq apply the same per-element scale / shift / ReLU to the same convolution output: the
    frames are equal bit for bit, in evaluation mode (scale / shift from the same running statistics) and in training mode (from the
    batch statistics, which both calls form with the same launches)."""
    from ast_amd._lib import CnnLayerParams
    from test_gpu_ops import GuardedWS, dev, ok, stream, vp
    _, B, T, D, layers, seed, _ = _geometry(cid)
    cfg, P, X, _, _ = RC.cnn_draws(B, T, D, None, None, False, seed=seed, layers=layers)
    n = len(layers)
    cd = _cnn_desc(cfg, B, T, D)
    t2, f2, feat = C.c_int(), C.c_int(), C.c_int()
    ok(lib, lib.astk_conv_bn_relu_out_dims(C.byref(cd), C.byref(t2), C.byref(f2), C.byref(feat)))
    sfx = ("/W", "_bn/gamma", "_bn/beta", "_bn/avg_mean", "_bn/avg_var")
    nbytes = lib.astk_conv_bn_relu_workspace_bytes(C.byref(cd))
    xd = dev(X)

    def frames(train, knobs):
        prm = {f"CNN_{i}{s}": dev(P[f"CNN_{i}{s}"]) for i in range(n) for s in sfx}      # (fresh running statistics for every call)
        cp = (CnnLayerParams * n)()
        for i in range(n):
            cp[i].W, cp[i].gamma, cp[i].beta, cp[i].avg_mean, cp[i].avg_var = (prm[f"CNN_{i}{s}"].data_ptr() for s in sfx)
        ws = GuardedWS(nbytes)
        out = torch.full((t2.value, B, feat.value), 7.0, device="cuda")
        with _knobs_off(lib, knobs):
            ok(lib, lib.astk_conv_bn_relu_fwd(C.byref(cd), cp, vp(xd), None, vp(out), vp(ws), nbytes, train, stream()))
        ws.check("cnn fwd")
        return out

    for train in (0, 1):
        tiled, plain = frames(train, ()), frames(train, ("conv.seq_fwd",))
        assert float(tiled.abs().max()) > 0 and float((tiled == 7.0).sum()) == 0
        assert torch.equal(tiled, plain), f"train = {train}: the tiled re-layout differs from the un-tiled one by {float((tiled - plain).abs().max()):.3e}"


# ------------------------------------------------------------------ the descriptor's refusals
def _desc(B, T, D, layers, pool=None):
    cd = _cnn_desc(RC.cnn_geometry_cfg(layers), B, T, D)
    for i, (wt, wf) in enumerate(pool or []):
        cd.pool_t[i], cd.pool_f[i] = wt, wf
    return cd


GOOD = [(8, 9, 13, 2, 13, 4), (8, 9, 1, 2, 1, 4)]
REFUSALS = [
    ("no-layers", dict(n_layers=0), "1..4 layers"),
    ("five-layers", dict(n_layers=5), "1..4 layers"),
    ("kt<st-layer0", dict(layers=[(8, 2, 13, 3, 13, 1), GOOD[1]]), "time kernel must be >= time stride (layer 0)"),
    ("kt<st-layer1", dict(layers=[GOOD[0], (8, 2, 1, 3, 1, 0)]), "time kernel must be >= time stride (layer 1)"),
    ("channels-6", dict(layers=[(6, 9, 13, 2, 13, 4), GOOD[1]]), "multiples of 4 (layer 0: 6)"),
    ("channels-10-layer1", dict(layers=[GOOD[0], (10, 9, 1, 2, 1, 4)]), "multiples of 4 (layer 1: 10)"),
    ("kf>D", dict(layers=[(8, 9, 27, 2, 13, 4), GOOD[1]]), "bad layer-0 frequency kernel"),
    ("sf=0", dict(layers=[(8, 9, 13, 2, 0, 4), GOOD[1]]), "bad layer-0 frequency kernel"),
    ("kf=3-layer1", dict(layers=[GOOD[0], (8, 9, 3, 2, 1, 4)]), "layers >= 1 must have a (kt,1) kernel and frequency stride 1"),
    ("sf=2-layer1", dict(layers=[GOOD[0], (8, 9, 1, 2, 2, 4)]), "layers >= 1 must have a (kt,1) kernel and frequency stride 1"),
    ("pt<0", dict(layers=[GOOD[0], (8, 9, 1, 2, 1, -1)]), "bad layer 1"),
    ("short-layer0", dict(T=4, layers=[(8, 9, 13, 2, 13, 2), GOOD[1]]), "input too short for layer 0"),
    ("short-layer1", dict(T=12, layers=[GOOD[0], (8, 9, 1, 2, 1, 1)]), "input too short for layer 1"),
    ("pool-2", dict(pool=[[1, 1], [-2, 1]]), "bad pooling window (layer 1)"),
]


@pytest.mark.parametrize("cid,change,cause", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_cnn_descriptor_refusals(lib, cid, change, cause):
    """What astk_cnn_desc does not take is refused by astk_conv_bn_relu_out_dims, by _workspace_bytes (0 bytes) and by the forward call,
    each naming the cause, before anything is launched: the output buffer keeps what it held."""
    from ast_amd._lib import CnnLayerParams
    B, T, D = 2, change.get("T", 40), 26
    cd = _desc(B, T, D, change.get("layers", GOOD), change.get("pool"))
    if "n_layers" in change:
        cd.n_layers = change["n_layers"]
    t2, f2, feat = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    assert lib.astk_conv_bn_relu_out_dims(C.byref(cd), C.byref(t2), C.byref(f2), C.byref(feat)) != 0
    assert cause in lib.astk_last_error().decode(), lib.astk_last_error().decode()
    assert (t2.value, f2.value, feat.value) == (-7, -7, -7)
    assert lib.astk_conv_bn_relu_workspace_bytes(C.byref(cd)) == 0
    assert cause in lib.astk_last_error().decode(), lib.astk_last_error().decode()
    x = torch.zeros(B, T, D, device="cuda")
    out = torch.full((4096,), 7.0, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    w = torch.zeros(1 << 16, device="cuda")            # every parameter pointer of every layer: valid memory, never read
    cp = (CnnLayerParams * 4)()
    for i in range(4):
        cp[i].W = cp[i].gamma = cp[i].beta = cp[i].avg_mean = cp[i].avg_var = w.data_ptr()
    rc = lib.astk_conv_bn_relu_fwd(C.byref(cd), cp, C.c_void_p(x.data_ptr()), None, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()),
                                   ws.numel(), 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0
    assert cause in lib.astk_last_error().decode(), lib.astk_last_error().decode()
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0 and int(ws.count_nonzero()) == 0, "a refused forward call wrote"


def test_model_refuses_frequency_padding():
    """ast_amd/seq2seq.py builds the descriptor from model_cfg.json; the C ABI has no frequency pad, so a config with one must not be
    run as if it had none."""
    from ast_amd.seq2seq import SpeechEncoderDecoder
    from oracle import ast_ref as R
    cfg = tiny_cfg()
    B, T, D, V = 2, 21, 26, 11
    P = R.init_params(cfg, D, V, seed=0, dtype=np.float32)
    cfg["cnn_config"]["cnn_layers"][0]["pad"] = [4, 1]
    m = SpeechEncoderDecoder(0, cfg).materialize(D, values=P)
    with pytest.raises(NotImplementedError, match="frequency padding"):
        m._shape_state(B, T, D, 5)


# ------------------------------------------------------------------ whole model
def _model_cfg(layers):
    def cfgf(drop):
        cfg = tiny_cfg(enc_layers=2, dec_layers=1, H=128, E=16, A=64, V=57, drop=drop)
        cfg["cnn_config"]["cnn_layers"] = RC.cnn_geometry_cfg(layers)["cnn_config"]["cnn_layers"]
        return cfg
    return cfgf


@pytest.mark.parametrize("name,layers,B,T,D,L,drop", [
    ("geometry-three-layers", [(16, 9, 13, 2, 13, 4), (12, 9, 1, 2, 1, 4), (8, 3, 1, 1, 1, 1)], 4, 120, 80, 6, 0.0),
    ("geometry-kf14-sf7-l1s3-drop", [(16, 7, 14, 2, 7, 3), (8, 6, 1, 3, 1, 2)], 5, 150, 40, 6, 0.3),      # speech noise through the direct kernel
    ("geometry-one-layer", [(16, 9, 13, 2, 13, 4)], 4, 60, 26, 5, 0.0),
])
def test_train_step_parity_on_other_cnn_stacks(name, layers, B, T, D, L, drop, gemm_scheme):
    """The whole train step on CNN stacks other than the shipped one: the descriptor built from the config's cnn_layers, the LSTM input
    width following the geometry, astk_conv_out_amax feeding the encoder, three updates and every layer's running statistics --
    schedule_helpers.train_step_parity with its bounds as they are."""
    from schedule_helpers import train_step_parity
    train_step_parity(name, _model_cfg(layers), B, T, D, L, 57, drop, 0.8, gemm_scheme)
