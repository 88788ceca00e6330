"""Model of the fp16-operand mode (gemm.hip PREC_F16; `gemm_operands: "fp16"` / ASTK_OPERANDS_FP16), shared by tests/test_lowp_host.py and
tests/test_gpu_lowp.py.  Nothing here touches a GPU.

The mode can be modelled exactly: a product is sum_k fp16(a s_A) fp16(b s_B) / (s_A s_B) with f32 accumulation and power-of-two scales,
i.e. the float64 product of the operands rounded to fp16's grid plus f32 summation noise.  round_operand is that rounding; LowpProduct
puts it into torch's autograd for one batched product; DecoderTaps does the same for the decoder, whose eligible products are batched
over all steps behind the loop (one maximum per matrix of all steps, which a per-step autograd node cannot know).

Per case `ref16` is the model with rounding, `ref32` the model without, `plain` the model with every rounded operand cast as it is
(no scale: what the kernel does for an operand nobody measured), and `n32` the distance of ref16 evaluated in float32 from ref16."""
import functools

import numpy as np
import torch

F32_GATE = 2e-5          # the gate test_gemm_operand_magnitudes holds the f32-accurate schemes to, per row of the result


def scale_of(amax):
    """The kernel's scale_exp: the power of two that brings the maximum into [2^14, 2^15); 1 for a zero (or subnormal) maximum."""
    amax = float(np.float32(amax))
    if not amax >= 2.0 ** -126:
        return 1.0
    e = int(np.floor(np.log2(amax)))
    return 2.0 ** min(max(14 - e, -126), 126)


def round_operand(x, amax=None):
    """float64 image of what the stager puts into LDS for the f32 value x, divided by the scale again.  amax=None: the plain cast."""
    x = np.asarray(x, np.float32).astype(np.float64)
    s = 1.0 if amax is None else scale_of(amax)
    with np.errstate(over="ignore"):
        return (x * s).astype(np.float16).astype(np.float64) / s


def round_measured(x, measured=True):
    x = np.asarray(x)
    return round_operand(x, float(np.abs(x).max()) if (measured and x.size) else None)


class LowpSpec:
    """Which directions of one product run with fp16 operands, and which operands carry a measured maximum."""

    def __init__(self, fwd=True, dgrad=True, wgrad=True, mx=True, mw=True, mg=True):
        self.fwd, self.dgrad, self.wgrad, self.mx, self.mw, self.mg = fwd, dgrad, wgrad, mx, mw, mg

    def plain(self):
        return LowpSpec(self.fwd, self.dgrad, self.wgrad, False, False, False)


def _rt(t, measured):
    return torch.from_numpy(round_measured(t.detach().double().numpy(), measured)).to(t.dtype)


class LowpProduct(torch.autograd.Function):
    """y = x w^T (x: (..., K), w: (N, K)).  Forward multiplies rounded operands; backward multiplies the rounded incoming gradient with
    the rounded saved operands; the sums run in the tensors' dtype (float64: the model; float32: its f32 evaluation)."""

    @staticmethod
    def forward(ctx, x, w, spec):
        ctx.spec = spec
        ctx.save_for_backward(x, w)
        if not spec.fwd:
            return x @ w.t()
        return _rt(x, spec.mx) @ _rt(w, spec.mw).t()

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        s = ctx.spec
        K, N = x.shape[-1], w.shape[0]
        g2, x2 = g.reshape(-1, N), x.reshape(-1, K)
        rg = _rt(g2, s.mg) if (s.dgrad or s.wgrad) else None
        dx = (rg @ _rt(w, s.mw)) if s.dgrad else g2 @ w
        dw = (rg.t() @ _rt(x2, s.mx)) if s.wgrad else g2.t() @ x2
        return dx.reshape(x.shape), dw, None


def lowp_linear(spec):
    return lambda x, w: LowpProduct.apply(x, w, spec)


# ------------------------------------------------------------------ assertion helpers (the GPU test's; the host test runs them on the models)
def rows_err(got, ref):
    """max |got - ref| per row over the row's largest |ref| (rows of zeros: over 1)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    rowmax = np.abs(ref).max(axis=1)
    return np.abs(got - ref).max(axis=1) / np.where(rowmax > 0, rowmax, 1.0)


def assert_rows(got, ref, what, rel=F32_GATE):
    assert np.isfinite(np.asarray(got, np.float64)).all(), f"{what}: not finite"
    err = rows_err(got, ref)
    print(f"{what}: worst row {err.max():.3e} of its largest entry (gate {rel:.1e})")
    assert err.max() <= rel, f"{what}: row {int(err.argmax())} is {err.max():.3e} of its largest entry from the model (gate {rel:.1e})"


def maxdiff(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max()) if a.size else 0.0


def assert_tensor(got, ref, what, rtol, gap=None):
    """The op tests' gate (max abs error within rtol of the reference's largest entry) and, for a directly affected tensor, gap / 4."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, scale = maxdiff(got, ref), float(np.abs(ref).max()) if ref.size else 1.0
    print(f"{what}: err {err:.3e}  scale {scale:.3e}  gate {rtol * max(scale, 1e-6):.3e}" + ("" if gap is None else f"  gap/4 {gap / 4:.3e}"))
    assert np.isfinite(got).all(), f"{what}: not finite"
    assert err <= rtol * max(scale, 1e-6), f"{what}: max abs err {err:.3e} > {rtol * max(scale, 1e-6):.3e} (ref scale {scale:.3e})"
    if gap is not None:
        assert err <= gap / 4, f"{what}: max abs err {err:.3e} > gap / 4 = {gap / 4:.3e}: not the fp16-operand arithmetic of the model"


def assert_op(got, case, which="ref16"):
    """Every tensor of an op case against the model `which` names; the directly affected ones also within gap / 4."""
    ref = case[which]
    for k in sorted(ref):
        rtol = 2e-4 if k in case["outputs"] else 5e-4
        assert_tensor(got[k], ref[k], f"{case['name']} {k}", rtol, case["gap"][k] if k in case["affected"] else None)


def finish_case(case):
    """gap and n32 per directly affected tensor."""
    case["gap"] = {k: maxdiff(case["ref16"][k], case["ref32"][k]) for k in case["affected"]}
    case["n32"] = {k: maxdiff(case["ref16_f32"][k], case["ref16"][k]) for k in case["affected"]}
    return case


# ------------------------------------------------------------------ kernel level: the case table
# name, [(M, N, K)] (a group), batch, modes tested.  PREC_F16 exists for 128-tiles only: the edges are those of that tile.
GEMM_CASES = [
    ("one", [(1, 1, 4)], 1, (0,)),
    ("ragged-k19", [(130, 70, 19)], 1, (0,)),             # ragged second tile, K tail below one k-iteration and no multiple of 4
    ("k531", [(129, 70, 531)], 1, (0,)),
    ("vocab", [(37, 1098, 512)], 1, (0,)),
    ("deep", [(260, 200, 20480)], 1, (0, 1, 2)),          # few tiles, deep K, split tiles
    ("batch3", [(150, 130, 100)], 3, (0,)),
    ("group3", [(70, 45, 19), (150, 130, 333), (129, 70, 64)], 1, (0,)),
    # at most two k-iterations per tile: however the launcher splits the tiles, no tile has more than two contributors, and two float
    # atomic adds into a zeroed tile commute -- the f32-accurate launch of this group is bit-reproducible
    ("unmarked3", [(70, 45, 19), (150, 130, 32), (129, 70, 20)], 1, (0,)),
]
MAGNITUDES = [(1.0, 1.0), (1e-6, 1e3), (3e-9, 1.0)]      # operand gains of the measured cases; rows of A spread over four decades
MAG_SHAPE = (150, 130, 333)


def gemm_operands(name, M, N, K, batch=1, sa=1.0, sb=1.0, decades=0):
    """A (batch, M, K), B (batch, N, K) as float32-valued float64 arrays (product = A B^T per slice)."""
    seed = int.from_bytes(name.encode(), "little") % (2 ** 31) + 7 * M + 3 * N + K
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((batch, M, K)) * sa
    if decades:
        A = A * (10.0 ** (-(np.arange(M) % decades)))[None, :, None]
    B = rng.standard_normal((batch, N, K)) * sb
    return A.astype(np.float32).astype(np.float64), B.astype(np.float32).astype(np.float64)


def gemm_refs(A, B, measure):
    """ref16 with the measured operands (bit 0: A, bit 1: B) behind their scale, ref32, and the plain-cast model."""
    mm = lambda a, b: a @ b.transpose(0, 2, 1)
    return dict(ref16=mm(round_measured(A, measure & 1), round_measured(B, measure & 2)), ref32=mm(A, B),
                plain=mm(round_operand(A), round_operand(B)))


def gemm_f32_eval(A, B, measure):
    a, b = round_measured(A, measure & 1).astype(np.float32), round_measured(B, measure & 2).astype(np.float32)
    return (a @ b.transpose(0, 2, 1)).astype(np.float64)


# ------------------------------------------------------------------ encoder
# (T, B, in, h, layers, masks): the first two on the persistent kernels, the third on the per-step loop
ENC_SHAPES = [(7, 5, 24, 64, 2, False), (9, 33, 16, 128, 2, True), (5, 3, 12, 20, 2, False)]
GAINS = [1.0, 1e-4]      # upstream gain: with a loss divided by the batch, 1e-4 is where dz really lives (1e-5 ... 1e-9: below fp16's normal range)
ENC_SEEDS = [1, 0, 11]   # of range_cases.lstm_draws, per shape: chosen in tests/test_lowp_host.py (gap >= 8 n32 at both gains)
ENC_CASES = [shape + (gain, seed) for shape, seed in zip(ENC_SHAPES, ENC_SEEDS) for gain in GAINS]
ENC_OUTPUTS = ("enc_states", "cT", "hT")
ENC_PERSISTENT_WIDTHS = (64, 128, 256, 512, 1024)        # h at which astk_lstm_stack_path takes a persistent kernel


def _enc_run(c, nl, masks, spec, gain, dtype):
    from oracle.ast_ref_torch import encoder_torch
    cfg = {"rnn_config": {"enc_layers": nl}}
    Pt = {k: torch.tensor(np.asarray(v, np.float32), dtype=dtype, requires_grad=True) for k, v in c["P"].items()}
    xt = torch.tensor(np.asarray(c["x"], np.float32), dtype=dtype, requires_grad=True)
    mk = torch.tensor(np.asarray(c["mk"], np.float32), dtype=dtype) if masks else None
    enc, cT, hT = encoder_torch(cfg, Pt, xt, mk, proj0=None if spec is None else lowp_linear(spec))
    up = [torch.tensor((np.asarray(c[k]) * gain).astype(np.float32), dtype=dtype) for k in ("g_enc", "g_c", "g_h")]
    ((enc * up[0]).sum() + (cT * up[1]).sum() + (hT * up[2]).sum()).backward()
    out = {"enc_states": enc, "cT": cT, "hT": hT, "dx": xt.grad}
    out.update({"grad " + k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in Pt.items()})
    return {k: v.detach().double().numpy() for k, v in out.items()}


def enc_case(T, B, in_dim, h, nl, masks, gain, seed=None):
    """The encoder's eligible products (lstm.hip): the layer-0 input projection of both directions, its dWu, dx.  Every operand is measured:
    the frames and the two weights by a pass, dz by the recurrence kernel (persistent paths) or a pass (per-step loop)."""
    import range_cases
    c = range_cases.lstm_draws(T, B, in_dim, h, nl, masks, seed=seed)
    # the per-step loop has no batched input projection (its fused cell launches multiply x_t themselves, exactly): no forward product
    # is eligible there, the outputs are the exact model's, and only dx and the two layer-0 dWu are directly affected
    persistent = h in ENC_PERSISTENT_WIDTHS
    spec = LowpSpec(fwd=persistent)
    case = dict(name=f"enc T{T} B{B} in{in_dim} h{h} L{nl}{' masks' if masks else ''} gain {gain:g}", draws=c, gain=gain, outputs=ENC_OUTPUTS,
                persistent=persistent, affected=(ENC_OUTPUTS if persistent else ()) + ("dx", "grad L0_enc/upward/W", "grad L0_rev_enc/upward/W"))
    case["ref16"] = _enc_run(c, nl, masks, spec, gain, torch.float64)
    case["ref32"] = _enc_run(c, nl, masks, None, gain, torch.float64)
    case["plain"] = _enc_run(c, nl, masks, spec.plain(), gain, torch.float64)
    case["ref16_f32"] = _enc_run(c, nl, masks, spec, gain, torch.float32)
    case["small_gradient_operand"] = gain <= 1e-4
    return finish_case(case)


@functools.lru_cache(maxsize=None)
def enc_case_of(row):
    return enc_case(*row[:6], row[6], seed=row[7])


# ------------------------------------------------------------------ decoder
# (B, L, T, H, E, A, V, layers, masks): two on the persistent loops, one on the per-launch loop, one at the shipped width and vocabulary
DEC_SHAPES = [(5, 9, 23, 64, 16, 32, 57, 1, False), (19, 8, 37, 128, 32, 64, 130, 3, True), (5, 9, 23, 32, 12, 24, 57, 3, True),
              (32, 4, 50, 512, 128, 512, 1098, 1, False)]
# (shape, class-weight gain, seed, alphabet).  Seeds (and, at the shipped width, transcripts over ONE token) chosen in
# tests/test_lowp_host.py for gap >= 8 n32.  The gain-1e-4 rows: every class weight 1e-4 scales the loss and with it dlogits and dz to
# where a plain fp16 cast flushes them -- at gain 1 the largest dlogits (1 / B) are inside fp16's range and carry the largest entries of
# every weight gradient, so the plain cast and the scaled rounding differ by a hundredth of gap there.
DEC_CASES = [(DEC_SHAPES[0], 1.0, 7, None), (DEC_SHAPES[1], 1.0, 40, None), (DEC_SHAPES[2], 1.0, 7, None), (DEC_SHAPES[3], 1.0, 19, 1),
             (DEC_SHAPES[0], 1e-4, 7, None), (DEC_SHAPES[2], 1e-4, 7, None)]


class _Tap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, sink):
        ctx.sink = sink
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        ctx.sink.append(g.detach().clone())
        return g, None


class DecoderTaps:
    """decoder_torch's hook: records, per step, the operands of the products the library batches over all steps behind the loop (the
    incoming gradients through an identity node), and forms those products afterwards with one maximum per gradient matrix."""

    def __init__(self):
        self.rec = {}

    def __call__(self, name, t, *operands):
        r = self.rec.setdefault(name, {"g": [], "ops": []})
        r["ops"].append([o.detach().clone() for o in operands])
        return _Tap.apply(t, r["g"])

    def stacked(self, name):
        """(G, operands...) over all steps in step order (autograd delivers the gradients last step first)."""
        r = self.rec[name]
        G = torch.cat(list(reversed(r["g"])), 0)
        ops = [torch.cat([o[i] for o in r["ops"]], 0) for i in range(len(r["ops"][0]))]
        return [G] + ops

    def grads(self, P, nl, E, measured=True, rounded=True, embed=True):
        """The eligible products (decoder.hip bwd_params): dWo, every layer's dWu / dWl, the embedding columns of d_x0 (scattered into
        d_embed).  Gradient operands (dlogits, the cells' dz) behind their measured scale, everything else cast as it is."""
        dt = P["out/W"].dtype
        rg = (lambda t: _rt(t, measured)) if rounded else (lambda t: t)
        ro = (lambda t: _rt(t, False)) if rounded else (lambda t: t)
        out = {}
        G, HT = self.stacked("out")
        out["grad out/W"] = rg(G).t() @ ro(HT)
        for k in range(nl):
            G, X, Hp = self.stacked(f"L{k}")
            Gr = rg(G)
            out[f"grad L{k}_dec/upward/W"] = Gr.t() @ ro(X)
            out[f"grad L{k}_dec/lateral/W"] = Gr.t() @ ro(Hp)
            if k == 0 and embed:
                dxe = Gr @ ro(P["L0_dec/upward/W"].detach()[:, :E].contiguous())
                _, tok, mask = self.stacked("embed")
                de = torch.zeros_like(P["embed_dec/W"].detach())
                de.index_add_(0, tok.long().reshape(-1), dxe * mask)
                out["grad embed_dec/W"] = de
        return {k: v.to(dt).detach().double().numpy() for k, v in out.items()}


def _dec_run(c, shape, dtype, gain=1.0):
    from oracle.ast_ref_torch import decoder_torch
    B, L, T, H, E, A, V, nl, masks = shape
    cfg = {"rnn_config": {"dec_layers": nl, "attn_units": A}}
    f = lambda a: torch.tensor(np.asarray(a, np.float32), dtype=dtype)
    Pt = {k: f(v).requires_grad_(True) for k, v in c["P"].items()}
    enc_t, c0_t, h0_t = (f(c[k]).requires_grad_(True) for k in ("enc", "c0", "h0"))
    taps = DecoderTaps()
    loss, preds = decoder_torch(cfg, Pt, enc_t, c0_t, h0_t, c["y"], c["flags"], V, f(c["em"]) if masks else None, f(c["rm"]) if masks else None,
                                tap=taps)
    (loss * gain).backward()
    exact = {"d_enc": enc_t.grad, "d_c0": c0_t.grad, "d_h0": h0_t.grad}
    exact.update({"grad " + k: v.grad for k, v in Pt.items()})
    exact = {k: v.detach().double().numpy() for k, v in exact.items()}
    return exact, taps, Pt, float(loss.detach()) * gain, preds.numpy()


def dec_case(shape, gain=1.0, seed=None, alphabet=None):
    """No forward product of the decoder is eligible: loss and fed-back tokens are those of the f32 call.  Directly affected: out/W, every
    layer's upward/W and lateral/W, embed_dec/W; everything else is held to ref32.
    gain: every class weight (the loss and every gradient scale with it); alphabet: not None = the transcripts' tokens are redrawn from
    that many distinct ones (more rows then share a target, and more rows carry the largest entries of the output layer's gradient)."""
    import range_cases
    B, L, T, H, E, A, V, nl, masks = shape
    seed = B + L if seed is None else seed
    c = range_cases.dec_draws(B, L, T, H, E, A, V, nl, masks, seed=seed)
    if alphabet is not None:
        rng = np.random.default_rng(seed + 1000)
        letters, inner = rng.integers(4, V, size=alphabet), c["y"] >= 4
        c["y"][inner] = letters[rng.integers(0, alphabet, size=int(inner.sum()))]
    # the embedding columns of d_x0 are a batched product behind the loop on the persistent and the wide loops only (decoder.hip gx); the
    # per-launch loop forms them step by step inside its exact input-gradient product: embed_dec/W is the exact model's there
    embed = H % 64 == 0
    case = dict(name="dec " + " ".join(str(v) for v in shape) + f" gain {gain:g}", draws=c, shape=shape, gain=gain, outputs=(), persistent=embed)
    exact, taps, Pt, loss, preds = _dec_run(c, shape, torch.float64, gain)
    case["loss"], case["preds"] = loss, preds
    case["ref32"] = exact
    case["ref16"] = dict(exact, **taps.grads(Pt, nl, E, embed=embed))
    case["plain"] = dict(exact, **taps.grads(Pt, nl, E, measured=False, embed=embed))
    case["affected"] = tuple(sorted(set(taps.grads(Pt, nl, E, rounded=False, embed=embed))))
    exact32, taps32, Pt32, _, _ = _dec_run(c, shape, torch.float32, gain)
    case["ref16_f32"] = dict(exact32, **taps32.grads(Pt32, nl, E, embed=embed))
    case["small_gradient_operand"] = gain <= 1e-4
    return finish_case(case)


@functools.lru_cache(maxsize=None)
def dec_case_of(row):
    return dec_case(row[0], row[1], seed=row[2], alphabet=row[3])


# ------------------------------------------------------------------ CNN front-end
# (B, T, D, c0, c1): the shipped two-layer geometry (stride 2 in time: two phases of the input gradient)
CNN_SHAPES = [(3, 21, 26, 4, 8), (2, 50, 80, 8, 12), (2, 16, 13, 4, 4)]
CNN_SEEDS = [0, 3, 0]     # of range_cases.cnn_draws, per shape: kink-free on the rounded reference (asserted in tests/test_lowp_host.py)
CNN_CASES = [shape + (gain, seed) for shape, seed in zip(CNN_SHAPES, CNN_SEEDS) for gain in GAINS]


class LowpConv2d(torch.autograd.Function):
    """The window products of a CNN layer >= 1 (conv.hip): forward round(activations) * round(weights); input gradient round(dY) *
    round(phase weights) -- one product, one maximum per stride phase: the taps kt with the same kt mod stride --; weight gradient
    round(dY)^T round(activations).  Every operand's maximum is taken by the kernel that writes it, whatever the scheme."""

    @staticmethod
    def forward(ctx, x, w, stride, padding, measured):
        ctx.args = (stride, padding, measured)
        ctx.save_for_backward(x, w)
        return torch.nn.functional.conv2d(_rt(x, measured), _rt(w, measured), stride=stride, padding=padding)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        stride, padding, measured = ctx.args
        rg = _rt(g, measured)
        wp = torch.empty_like(w)
        for r in range(min(stride[0], w.shape[2])):
            wp[:, :, r::stride[0]] = _rt(w[:, :, r::stride[0]], measured)
        dx = torch.nn.grad.conv2d_input(x.shape, wp, rg, stride=stride, padding=padding)
        dw = torch.nn.grad.conv2d_weight(_rt(x, measured), w.shape, rg, stride=stride, padding=padding)
        return dx, dw, None, None, None


def _cnn_run(cfg, P, X, gout, lowp, measured, dtype, kink=False):
    from oracle.ast_ref_torch import cnn_torch
    Pt = {k: torch.tensor(np.asarray(v, np.float32), dtype=dtype, requires_grad=k.startswith("CNN") and "avg" not in k) for k, v in P.items()}
    pre = []

    def conv(i, h, W, stride, padding):
        y = LowpConv2d.apply(h, W, stride, padding, measured) if (lowp and i >= 1) else torch.nn.functional.conv2d(h, W, stride=stride, padding=padding)
        pre.append((y.detach(), Pt[f"CNN_{i}_bn/gamma"].detach(), Pt[f"CNN_{i}_bn/beta"].detach()))
        return y
    out = cnn_torch(cfg, Pt, torch.tensor(np.asarray(X, np.float32), dtype=dtype), None, conv=conv)
    out.backward(torch.tensor(np.asarray(gout, np.float32), dtype=dtype))
    res = {"out": out}
    res.update({"grad " + k: v.grad for k, v in Pt.items() if v.requires_grad})
    res = {k: v.detach().double().numpy() for k, v in res.items()}
    if kink:        # the smallest |post-BatchNorm pre-activation| per layer: the distance of the nearest unit from the ReLU's kink
        near = []
        for y, gamma, beta in pre:
            z = torch.nn.functional.batch_norm(y, None, None, gamma, beta, training=True, eps=2e-5)
            near.append(float(z.abs().min()))
        res["_kink"] = near
    return res


def cnn_case(B, T, D, c0, c1, gain, seed=0):
    """Layers >= 1: forward, every stride phase of the input gradient, the weight gradient run with fp16 operands, every operand behind
    its measured scale; layer 0 is exact.  Directly affected: the output, CNN_1/W and, through the input gradient, every CNN_0 gradient."""
    import range_cases
    cfg, P, X, _, rng = range_cases.cnn_draws(B, T, D, c0, c1, False, seed=seed)
    from oracle.ast_ref_torch import cnn_torch
    shape = tuple(cnn_torch(cfg, {k: torch.tensor(v) for k, v in P.items()}, torch.tensor(X)).shape)
    gout = rng.standard_normal(shape) * gain
    case = dict(name=f"cnn B{B} T{T} D{D} c{c0},{c1} gain {gain:g}", cfg=cfg, P=P, X=X, gout=gout, gain=gain, outputs=("out",),
                affected=("out", "grad CNN_1/W", "grad CNN_0/W", "grad CNN_0_bn/gamma", "grad CNN_0_bn/beta"), small_gradient_operand=gain <= 1e-4)
    case["ref16"] = _cnn_run(cfg, P, X, gout, True, True, torch.float64, kink=True)
    case["kink"] = case["ref16"].pop("_kink")
    case["ref32"] = _cnn_run(cfg, P, X, gout, False, True, torch.float64)
    case["plain"] = _cnn_run(cfg, P, X, gout, True, False, torch.float64)
    case["ref16_f32"] = _cnn_run(cfg, P, X, gout, True, True, torch.float32)
    return finish_case(case)


@functools.lru_cache(maxsize=None)
def cnn_case_of(row):
    return cnn_case(*row[:5], row[5], seed=row[6])
