"""The fp16-operand mode (`gemm_operands: "fp16"` / ASTK_OPERANDS_FP16, gemm.hip PREC_F16) against the product of rounded operands.

tests/lowp_model.py models the mode exactly (operands rounded to fp16's grid behind their power-of-two scale, float64 products);
tests/test_lowp_host.py shows on the CPU that every case here separates that arithmetic from the f32-accurate one and that the helpers
used below reject the wrong one.  Kernel level: one grouped launch through the instrumented build's astk_debug_gemm_group_lowp, held to
the model within 2e-5 of each row's largest entry (the gate of test_gemm_operand_magnitudes: the model leaves only f32 summation).  Op
level: the encoder stack and the decoder through the C ABI with the descriptor's gemm_operands = ASTK_OPERANDS_FP16; every tensor at the
op tests' tolerance (2e-4 outputs, 5e-4 gradients) against the model, every directly affected tensor also within gap / 4."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lowp_model as M
from test_gpu_ops import GuardedWS, dev, ok, stream, vp

pytestmark = pytest.mark.gpu

NT, NN, TN = 0, 1, 2
PREC = {"default": 0, "fp16x2": 1, "f32": 3}        # astk.h ASTK_PREC_*
OPERANDS_F32, OPERANDS_FP16 = 1, 2


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


@pytest.fixture
def tl():
    """The instrumented build (libastk_test.so), for the kernel-level tests only: the op tests run on the product library."""
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    with _lib.load_test_hooks() as t:
        yield t


# ------------------------------------------------------------------ kernel level
def _pad(n):
    return (n + 3) // 4 * 4 + 4


def _store(X, transpose):
    """(batch, rows, inner) -> the device image (batch, rows', ld) with NaN in the leading-dimension padding."""
    X = X.transpose(0, 2, 1) if transpose else X
    P = np.full(X.shape[:2] + (_pad(X.shape[2]),), np.nan)
    P[:, :, :X.shape[2]] = X
    return dev(P)


class Group:
    """The operands of one grouped launch on the device, in `layout`."""

    def __init__(self, layout, prods):
        self.layout, self.n = layout, len(prods)
        self.shapes = [(A.shape[1], B.shape[1], A.shape[2], A.shape[0]) for A, B in prods]      # M, N, K, batch
        self.a = [_store(A, layout == TN) for A, _ in prods]
        self.b = [_store(B, layout != NT) for _, B in prods]

    def run(self, tl, precision, operands=OPERANDS_FP16, mode=0, lowp=None, measure=None, c0=None):
        """-> per product the result (batch, M, N).  c0: what C holds in front of an accumulating launch (default: zeros); a store
        launch finds 7.0 everywhere and must leave it in the padding."""
        n = self.n
        ia = lambda v: (C.c_int32 * n)(*v)
        la = lambda v: (C.c_long * n)(*v)
        pa = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        cs = []
        for i, (m, nn, k, bt) in enumerate(self.shapes):
            c = torch.full((bt, m, _pad(nn)), 7.0, device="cuda")
            if mode != 0:
                c[:, :, :nn] = 0.0 if c0 is None else dev(c0[i])
            cs.append(c)
        stride = lambda t: t.shape[1] * t.shape[2]
        ok(tl, tl.astk_debug_gemm_group_lowp(self.layout, n, ia([s[0] for s in self.shapes]), ia([s[1] for s in self.shapes]),
                                             ia([s[2] for s in self.shapes]), ia([s[3] for s in self.shapes]), ia([mode] * n),
                                             ia(lowp or [1] * n), ia(measure or [3] * n),
                                             pa(self.a), la([t.shape[2] for t in self.a]), la([stride(t) for t in self.a]),
                                             pa(self.b), la([t.shape[2] for t in self.b]), la([stride(t) for t in self.b]),
                                             pa(cs), la([t.shape[2] for t in cs]), la([stride(t) for t in cs]), precision, operands, stream()))
        torch.cuda.synchronize()
        out = []
        for c, (m, nn, k, bt) in zip(cs, self.shapes):
            assert float(c[:, :, nn:].min()) == 7.0 and float(c[:, :, nn:].max()) == 7.0, "wrote outside N"
            out.append(c[:, :, :nn].double().cpu().numpy())
        return out


@functools.lru_cache(maxsize=None)
def _kernel_case(name):
    """Operands and the models of one row of M.GEMM_CASES (computed once, shared by the layouts)."""
    _, group, batch, modes = next(c for c in M.GEMM_CASES if c[0] == name)
    prods = [M.gemm_operands(f"{name}/{i}", *shape, batch) for i, shape in enumerate(group)]
    return prods, [M.gemm_refs(A, B, 3) for A, B in prods], modes


@pytest.mark.parametrize("layout", [NT, NN, TN])
@pytest.mark.parametrize("name", [c[0] for c in M.GEMM_CASES])
def test_kernel_equals_the_product_of_rounded_operands(tl, name, layout):
    """Every shape of the case table, all three layouts, precision in {default, fp16x2, f32} (the descriptor's `precision` must not matter:
    the launch takes the fp16-operand kernel), leading-dimension padding full of NaN.  With both operands measured the scaled model
    holds; without a measured maximum (values inside fp16's range) the plain-cast model holds."""
    prods, refs, modes = _kernel_case(name)
    g = Group(layout, prods)
    rng = np.random.default_rng(5)
    c0 = [0.5 * rng.standard_normal(r["ref16"].shape).astype(np.float32).astype(np.float64) for r in refs]
    for pname, prec in PREC.items():
        for mode in modes:
            for measure, which in ((3, "ref16"), (0, "plain")):
                got = g.run(tl, prec, mode=mode, measure=[measure] * g.n, c0=c0)
                for i, r in enumerate(refs):
                    res = got[i] - (c0[i] if mode != 0 else 0.0)
                    M.assert_rows(res, r[which], f"{name}/{i} layout {layout} precision {pname} mode {mode} measured {measure}")


@pytest.mark.parametrize("layout", [NT, NN, TN])
@pytest.mark.parametrize("sa,sb", M.MAGNITUDES)
def test_kernel_measured_operands_far_outside_fp16_range(tl, layout, sa, sb):
    """Operands scaled by (sa, sb), rows of A spread over five decades, both maxima measured in front of the launch as an op measures
    them: the scaled model must hold for every row.  This is the case that fails if a maximum is dropped on the way to the kernel (a
    1e-6 operand cast as it is lands on fp16's subnormals)."""
    A, B = M.gemm_operands(f"mag-{sa:g}-{sb:g}/0", *M.MAG_SHAPE, 1, sa, sb, 5)
    r = M.gemm_refs(A, B, 3)
    g = Group(layout, [(A, B)])
    for pname, prec in PREC.items():
        M.assert_rows(g.run(tl, prec)[0], r["ref16"], f"magnitudes {sa:g} {sb:g} layout {layout} precision {pname}")


@pytest.mark.parametrize("layout", [NT, NN, TN])
def test_kernel_group_with_one_product_not_marked_eligible(tl, layout):
    """One product of three is not marked: the whole launch is refused the mode.  Nothing is rounded (ref32 within 2e-5 of each row's
    largest entry), and the results are the bits of the same launch under ASTK_OPERANDS_F32."""
    prods, refs, _ = _kernel_case("unmarked3")
    g = Group(layout, prods)
    for pname, prec in PREC.items():
        got = g.run(tl, prec, lowp=[1, 0, 1])
        f32 = g.run(tl, prec, operands=OPERANDS_F32, lowp=[1, 0, 1])
        for i, r in enumerate(refs):
            M.assert_rows(got[i], r["ref32"], f"unmarked3/{i} layout {layout} precision {pname}, one product unmarked")
            assert np.array_equal(got[i], f32[i]), (pname, i, np.abs(got[i] - f32[i]).max())


# ------------------------------------------------------------------ encoder
def _enc_call(lib, case, T, B, in_dim, h, nl, masks, precision, operands, deterministic=0):
    """astk_lstm_stack_fwd + _bwd under the descriptor's (precision, gemm_operands) -> every tensor, named as the model names them."""
    from ast_amd._lib import LstmGrads, LstmParams, LstmStackDesc
    c, gain = case["draws"], case["gain"]
    d = LstmStackDesc(T, B, in_dim, h, nl, 2)
    d.precision, d.gemm_operands, d.deterministic = precision, operands, deterministic
    prm = {k: dev(v) for k, v in c["P"].items()}
    grd = {k: torch.zeros_like(v) for k, v in prm.items()}
    lp, lg = (LstmParams * (2 * nl))(), (LstmGrads * (2 * nl))()
    for i, n in enumerate(c["names"]):
        lp[i].Wu, lp[i].b, lp[i].Wl = (prm[n + s].data_ptr() for s in ("/upward/W", "/upward/b", "/lateral/W"))
        lg[i].dWu, lg[i].db, lg[i].dWl = (grd[n + s].data_ptr() for s in ("/upward/W", "/upward/b", "/lateral/W"))
    nbytes = lib.astk_lstm_stack_workspace_bytes(C.byref(d))
    ws = GuardedWS(nbytes)
    xd, md = dev(c["x"]), (dev(c["mk"]) if masks else None)
    enc_d = torch.zeros(B, T, 2 * h, device="cuda")
    cT_d, hT_d = torch.zeros(2, nl, B, h, device="cuda"), torch.zeros(2, nl, B, h, device="cuda")
    ok(lib, lib.astk_lstm_stack_fwd(C.byref(d), lp, vp(xd), vp(md), vp(enc_d), vp(cT_d), vp(hT_d), vp(ws), nbytes, stream()))
    ws.check("lstm fwd")
    dx = torch.zeros(T, B, in_dim, device="cuda")
    ge_d, gc_d, gh_d = (dev((np.asarray(c[k]) * gain).astype(np.float32)) for k in ("g_enc", "g_c", "g_h"))
    ok(lib, lib.astk_lstm_stack_bwd(C.byref(d), lp, lg, vp(xd), vp(md), vp(ge_d), vp(gc_d), vp(gh_d), vp(dx), vp(ws), nbytes, stream()))
    ws.check("lstm bwd")
    out = {"enc_states": enc_d, "cT": cT_d, "hT": hT_d, "dx": dx}
    out.update({"grad " + k: v for k, v in grd.items()})
    return {k: v.cpu() for k, v in out.items()}, lib.astk_lstm_stack_path(C.byref(d))


@pytest.mark.parametrize("precision", ["default", "fp16x2"])
@pytest.mark.parametrize("row", M.ENC_CASES, ids=lambda r: "-".join(str(v) for v in r))
def test_encoder_stack_with_fp16_operands(lib, row, precision):
    """The layer-0 input projection of both directions (persistent kernels only: the per-step loop has no batched projection), its dWu
    and dx run with fp16 operands, every operand behind its measured scale (frames and weights by a pass, dz by the recurrence kernel or a
    pass); everything else is exact.  Upstream gain 1 and 1e-4: at 1e-4 dz spans 1e-5 ... 1e-9, which a plain fp16 cast flushes."""
    T, B, in_dim, h, nl, masks = row[:6]
    case = M.enc_case_of(row)
    got, path = _enc_call(lib, case, T, B, in_dim, h, nl, masks, PREC[precision], OPERANDS_FP16)
    assert (path != 0) == case["persistent"], "the first two shapes run on the persistent kernels, the third on the per-step loop"
    M.assert_op({k: v.double().numpy() for k, v in got.items()}, case)


def test_encoder_process_setting_and_descriptor_precedence(lib):
    """astk_set_low_precision_gemms(1) is the default of descriptors that say ASTK_OPERANDS_DEFAULT and nothing more: ASTK_OPERANDS_F32
    gives the bits of the plain call, ASTK_OPERANDS_DEFAULT those of an ASTK_OPERANDS_FP16 descriptor."""
    row = M.ENC_CASES[0]                # (deterministic calls: fixed-order sums, so that equal arithmetic means equal bits)
    T, B, in_dim, h, nl, masks = row[:6]
    case = M.enc_case_of(row)
    call = lambda operands: _enc_call(lib, case, T, B, in_dim, h, nl, masks, 0, operands, deterministic=1)[0]
    assert lib.astk_get_low_precision_gemms() == 0
    plain, fp16 = call(0), call(OPERANDS_FP16)
    assert not torch.equal(plain["enc_states"], fp16["enc_states"]), "the fp16-operand mode changed nothing"
    try:
        ok(lib, lib.astk_set_low_precision_gemms(1))
        forced_f32, by_default = call(OPERANDS_F32), call(0)
    finally:
        lib.astk_set_low_precision_gemms(0)
    for k in plain:
        assert torch.equal(forced_f32[k], plain[k]), f"{k}: ASTK_OPERANDS_F32 under the process setting is not the plain call"
        assert torch.equal(by_default[k], fp16[k]), f"{k}: ASTK_OPERANDS_DEFAULT under the process setting is not the fp16-operand call"


# ------------------------------------------------------------------ decoder
def _dec_call(lib, case, precision, operands):
    from ast_amd._lib import DecoderDesc, DecoderGrads, DecoderParams
    B, L, T, H, E, A, V, nl, masks = case["shape"]
    c = case["draws"]
    d = DecoderDesc(B, L, T, H, E, A, V, nl)
    d.precision, d.gemm_operands = precision, operands
    prm = {k: dev(v) for k, v in c["P"].items()}
    grd = {k: torch.zeros_like(v) for k, v in prm.items()}
    cw = torch.full((V,), float(np.float32(case["gain"])), device="cuda")
    cw[0] = 0
    dp, dg = DecoderParams(), DecoderGrads()
    dp.embed, dg.d_embed = prm["embed_dec/W"].data_ptr(), grd["embed_dec/W"].data_ptr()
    for k in range(nl):
        dp.lstm[k].Wu, dp.lstm[k].b, dp.lstm[k].Wl = (prm[f"L{k}_dec/" + s].data_ptr() for s in ("upward/W", "upward/b", "lateral/W"))
        dg.lstm[k].dWu, dg.lstm[k].db, dg.lstm[k].dWl = (grd[f"L{k}_dec/" + s].data_ptr() for s in ("upward/W", "upward/b", "lateral/W"))
    dp.Wa, dp.ba, dp.Wc, dp.bc, dp.Wo, dp.bo = (prm[k].data_ptr() for k in ("attn_Wa/W", "attn_Wa/b", "context/W", "context/b", "out/W", "out/b"))
    dg.dWa, dg.dba, dg.dWc, dg.dbc, dg.dWo, dg.dbo = (grd[k].data_ptr() for k in ("attn_Wa/W", "attn_Wa/b", "context/W", "context/b", "out/W", "out/b"))
    dp.class_weight = cw.data_ptr()
    nbytes = lib.astk_decoder_workspace_bytes(C.byref(d))
    ws = GuardedWS(nbytes)
    enc_d, c0_d, h0_d = dev(c["enc"]), dev(c["c0"]), dev(c["h0"])
    y_d, fl_d = dev(c["y"], torch.int32), dev(np.asarray(c["flags"]), torch.int32)
    em_d, rm_d = (dev(c["em"]) if masks else None), (dev(c["rm"]) if masks else None)
    loss_d = torch.zeros(1, device="cuda")
    pred_d = torch.zeros(c["S"], B, dtype=torch.int32, device="cuda")
    ok(lib, lib.astk_decoder_fwd(C.byref(d), C.byref(dp), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), vp(fl_d), vp(em_d), vp(rm_d),
                                 vp(loss_d), vp(pred_d), vp(ws), nbytes, stream()))
    ws.check("decoder fwd")
    d_enc = torch.zeros(B, T, H, device="cuda")
    d_c0, d_h0 = torch.zeros(nl, B, H, device="cuda"), torch.zeros(nl, B, H, device="cuda")
    ok(lib, lib.astk_decoder_bwd(C.byref(d), C.byref(dp), C.byref(dg), vp(enc_d), vp(c0_d), vp(h0_d), vp(y_d), vp(em_d), vp(rm_d),
                                 vp(d_enc), vp(d_c0), vp(d_h0), vp(ws), nbytes, stream()))
    ws.check("decoder bwd")
    out = {"d_enc": d_enc, "d_c0": d_c0, "d_h0": d_h0}
    out.update({"grad " + k: v for k, v in grd.items()})
    return {k: v.cpu() for k, v in out.items()}, loss_d.cpu(), pred_d.cpu(), lib.astk_decoder_path(C.byref(d))


@pytest.mark.parametrize("precision", ["default", "fp16x2"])
@pytest.mark.parametrize("row", M.DEC_CASES, ids=lambda r: "-".join(str(v) for v in r[0]) + f"-gain{r[1]:g}")
def test_decoder_with_fp16_operands(lib, row, precision):
    """No forward product of the decoder is eligible: loss and fed-back tokens are the bits of the ASTK_OPERANDS_F32 call.  Backward: dWo,
    every layer's dWu / dWl and the embedding columns of d_x0 run with fp16 operands, dlogits and the cells' dz behind their measured
    scale; attn_Wa, context, all biases, d_enc, d_c0, d_h0 are the exact model's.  The last shape has the shipped width and vocabulary
    (a non-target dlogit is about 3e-5); the gain-1e-4 rows scale every class weight, and with it every gradient operand, to where a
    plain cast flushes it.
    Margins: these products sum over S x B of about a hundred rows, so gap is only a few fp16 ulps of the largest contributions, and
    an operand the loop computed (dz, h) that lands on the other fp16 neighbour than the float64 model's moves a sum by one such ulp.
    Measured with the scaled operands: (19, 8, 37, 128, ...) L2 upward/W 9.9e-7 against gap / 4 = 1.01e-6, L1 upward/W 4.4e-7 against
    4.8e-7; the shipped shape's out/W 1.5e-5 against 2.3e-5; every other tensor below half of gap / 4.  A change of the loop's summation
    order can move the first two over the line without the arithmetic being wrong: tests/test_lowp_host.py is where a seed is chosen."""
    case = M.dec_case_of(row)
    H, nl = case["shape"][3], case["shape"][7]
    got, loss, pred, path = _dec_call(lib, case, PREC[precision], OPERANDS_FP16)
    assert bool(path & 1) == case["persistent"], "persistent loops at H = 64, 128, 512; the per-launch loop at H = 32"
    _, loss32, pred32, _ = _dec_call(lib, case, PREC[precision], OPERANDS_F32)
    assert torch.equal(loss, loss32) and torch.equal(pred, pred32), "the forward pass must not depend on gemm_operands"
    assert abs(float(loss) - case["loss"]) <= 1e-4 * abs(case["loss"]), (float(loss), case["loss"])
    assert (pred.numpy() == case["preds"]).all(), "argmax feedback tokens differ"
    M.assert_op({k: v.double().numpy() for k, v in got.items()}, case)


# ------------------------------------------------------------------ CNN front-end
def _cnn_call(lib, case, B, T, D, precision, operands):
    from ast_amd._lib import CnnLayerGrads, CnnLayerParams
    from test_gpu_ops import _cnn_desc
    cfg, P = case["cfg"], case["P"]
    n = len(cfg["cnn_config"]["cnn_layers"])
    cd = _cnn_desc(cfg, B, T, D)
    cd.precision, cd.gemm_operands = precision, operands
    t2, f2, feat = C.c_int(), C.c_int(), C.c_int()
    ok(lib, lib.astk_conv_bn_relu_out_dims(C.byref(cd), C.byref(t2), C.byref(f2), C.byref(feat)))
    assert (t2.value, B, feat.value) == case["ref16"]["out"].shape
    names = [f"CNN_{i}" for i in range(n)]
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
    xd, g = dev(case["X"]), dev(np.asarray(case["gout"]).astype(np.float32))
    ok(lib, lib.astk_conv_bn_relu_fwd(C.byref(cd), cp, vp(xd), None, vp(out), vp(ws), nbytes, 1, stream()))
    ws.check("cnn fwd")
    ok(lib, lib.astk_conv_bn_relu_bwd(C.byref(cd), cp, cg, vp(g), vp(ws), nbytes, stream()))
    ws.check("cnn bwd")
    res = {"out": out}
    res.update({"grad " + n_ + s: grd[n_ + s] for n_ in names for s in ("/W", "_bn/gamma", "_bn/beta")})
    return {k: v.double().cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("precision", ["default", "fp16x2"])
@pytest.mark.parametrize("row", M.CNN_CASES, ids=lambda r: "-".join(str(v) for v in r))
def test_cnn_with_fp16_operands(lib, row, precision):
    """Layers >= 1: forward, both stride phases of the input gradient and the weight gradient run with fp16 operands; every operand's
    maximum comes from the kernel that writes it, whatever the scheme.  Kink-free seeds (tests/test_lowp_host.py): every gradient at 5e-4."""
    B, T, D = row[:3]
    case = M.cnn_case_of(row)
    M.assert_op(_cnn_call(lib, case, B, T, D, PREC[precision], OPERANDS_FP16), case)
