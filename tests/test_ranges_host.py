"""CPU feasibility of the value-range cases of tests/test_gpu_ranges.py (no GPU): for every case there, the straightforward float32
restatement of the operator -- oracle/ast_ref_torch.py's functions or plain torch formulas on float32 tensors, two-pass variances --
must meet, against float64, a quarter of the tolerance the GPU test applies (half for the BatchNorm offset cases: their float32 input
itself carries r * 2^-24), pick the same feedback tokens, and the case's defining property (score range, logit range, saturation share,
channel mean over standard deviation) must hold on the float64 reference.  That is what makes a GPU failure on one of these cases the
kernel's fault.  A case that fails here is not loosened: it moves one rung down its ladder in tests/range_cases.py.  The last three
tests show the assertions have teeth: deliberately naive float32 restatements (one-pass variance, softmax without the maximum
subtracted, tanh from e^{2x}) fail them at the chosen rungs."""
import numpy as np
import pytest
import torch

import range_cases as RC

FWD, GRAD, LOSS = 2e-4, 5e-4, 1e-4            # the GPU tests' tolerances (tests/test_gpu_ops.py: close())


def _ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else None


def frac(got, ref):
    """max |got - ref| as a fraction of max |ref|: what close() bounds."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref).max() if ref.size else 0.0
    return float(err / max(np.abs(ref).max() if ref.size else 1.0, 1e-6)) if np.isfinite(err) else float("inf")


# ------------------------------------------------------------------ decoder
def dec_run(s, nl, A, V, dt):
    from oracle.ast_ref_torch import decoder_torch
    cfg = {"rnn_config": {"dec_layers": nl, "attn_units": A}}
    Pt = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in s["P"].items()}
    ins = [torch.tensor(s[k], dtype=dt, requires_grad=True) for k in ("enc", "c0", "h0")]
    tt = lambda a: None if a is None else torch.tensor(a, dtype=dt)
    loss, pred = decoder_torch(cfg, Pt, *ins, s["y"], s["flags"], V, tt(s["em"]), tt(s["rm"]))
    loss.backward()
    grads = {k: p.grad.numpy() for k, p in Pt.items()}
    grads.update({"d_" + k: t.grad.numpy() for k, t in zip(("enc", "c0", "h0"), ins)})
    return float(loss.detach()), pred.numpy(), grads


HOST_ROWS = 4          # the wide-logit and saturated-gate shapes with H >= 512 run here on the first four batch rows of the GPU test's draws: rows
                       # are independent and those families sit 5-100 x inside their budget.  The wide-score cases run whole: peaked attention
                       # leaves so little margin that the same case on a subset of its rows (another summation order) can miss the budget.


def dec_feasibility(shape, seed_off, rows=None, **gains):
    """-> (loss distance, tokens equal, worst gradient tensor's frac, its name, the (row-limited) dec_draws case)."""
    B, L, T, H, E, A, V, nl, masks = shape
    s = RC.dec_draws(B, L, T, H, E, A, V, nl, masks, seed=B + L + seed_off, **gains)
    if rows and H >= 512:
        s = RC.dec_rows(s, rows)
    l64, p64, g64 = dec_run(s, nl, A, V, torch.float64)
    l32, p32, g32 = dec_run(s, nl, A, V, torch.float32)
    worst = max((frac(g32[k], g64[k]), k) for k in g64)
    return abs(l32 - l64) / abs(l64), bool((p32 == p64).all()), worst[0], worst[1], s


@pytest.mark.parametrize("shape,seed_off,rung", [c[:3] for c in RC.DEC_ENC_CASES] + [RC.DEC_ENC_KNOB_CASE], ids=_ids)
def test_decoder_enc_gain_rungs_are_feasible(shape, seed_off, rung):
    dl, same, worst, name, s = dec_feasibility(shape, seed_off, enc_gain=rung)
    scores = RC.dec_step0(s, shape[7])[0]
    rng = scores.max(1) - scores.min(1)
    print(f"{shape} x{rung}: loss {dl:.1e} worst grad {worst:.1e} ({name}) step-0 score range {rng.min():.0f}-{rng.max():.0f}")
    RC.assert_score_ranges(rng, shape[3])
    assert same, "feedback tokens differ between float32 and float64"
    assert dl <= LOSS / 4 and worst <= GRAD / 4, (dl, worst, name)


@pytest.mark.parametrize("shape,seed_off", [c[:2] for c in RC.DEC_OUT_CASES], ids=_ids)
def test_decoder_out_gain_is_feasible(shape, seed_off):
    dl, same, worst, name, s = dec_feasibility(shape, seed_off, HOST_ROWS, out_gain=RC.OUT_GAIN)
    lg = RC.dec_step0(s, shape[7])[1]
    rng = lg.max(1) - lg.min(1)
    print(f"{shape} out x{RC.OUT_GAIN}: loss {dl:.1e} worst grad {worst:.1e} ({name}) step-0 logit range {rng.min():.0f}-{rng.max():.0f}")
    assert rng.min() >= 200
    assert same and dl <= LOSS / 4 and worst <= GRAD / 4, (same, dl, worst, name)


@pytest.mark.parametrize("bias_gain", RC.DEC_BIAS_GAINS)
@pytest.mark.parametrize("shape,seed_off", RC.DEC_BIAS_CASES, ids=_ids)
def test_decoder_bias_gain_is_feasible(shape, seed_off, bias_gain):
    dl, same, worst, name, s = dec_feasibility(shape, seed_off, HOST_ROWS, bias_gain=bias_gain)
    share, zmax = RC.saturation(RC.dec_step0(s, shape[7])[2])
    print(f"{shape} bias x{bias_gain}: loss {dl:.1e} worst grad {worst:.1e} ({name}) saturated share {share:.2f} max |z| {zmax:.1f}")
    assert share >= RC.DEC_SATURATED[bias_gain][0] and zmax >= RC.DEC_SATURATED[bias_gain][1], (share, zmax)
    assert same and dl <= LOSS / 4 and worst <= GRAD / 4, (same, dl, worst, name)


# ------------------------------------------------------------------ encoder stacks
def encoder_with(tanh, P, feats, nl, masks):
    """oracle/ast_ref_torch.py's encoder_torch restated with the activation passed in (the teeth test runs it with a naive tanh):
    interleaved gates a, i, f, o; the reverse direction consumes steps 0, T - 1, ..., 1; masks (2, nl, T, B, h) by loop step."""
    def run(xs, Wu, b, Wl, mk):
        zx, h, c, outs = xs @ Wu.t() + b, None, torch.zeros(xs.shape[1], Wl.shape[1], dtype=xs.dtype), []
        for t in range(xs.shape[0]):
            z = (zx[t] if h is None else zx[t] + h @ Wl.t()).view(xs.shape[1], -1, 4)
            c = tanh(z[..., 0]) * torch.sigmoid(z[..., 1]) + torch.sigmoid(z[..., 2]) * c
            h = torch.sigmoid(z[..., 3]) * tanh(c)
            outs.append(h if mk is None else h * mk[t])
        return torch.stack(outs, 0), c, h
    T2 = feats.shape[0]
    xs = [feats, feats[[(-i) % T2 for i in range(T2)]]]
    cT, hT = [[], []], [[], []]
    for k in range(nl):
        for d, pat in enumerate(("L{}_enc", "L{}_rev_enc")):
            n = pat.format(k)
            xs[d], cc, hh = run(xs[d], P[n + "/upward/W"], P[n + "/upward/b"], P[n + "/lateral/W"], None if masks is None else masks[d][k])
            cT[d].append(cc); hT[d].append(hh)
    enc = torch.cat([xs[0], torch.flip(xs[1], [0])], 2).transpose(0, 1)
    return enc, torch.stack([torch.stack(cT[0]), torch.stack(cT[1])]), torch.stack([torch.stack(hT[0]), torch.stack(hT[1])])


def lstm_run(c, nl, masks, dt, tanh=None):
    """tanh None: oracle/ast_ref_torch.py's encoder_torch itself; else the local restatement with that activation."""
    from oracle.ast_ref_torch import encoder_torch
    Pt = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in c["P"].items()}
    xt = torch.tensor(c["x"], dtype=dt, requires_grad=True)
    mk = torch.tensor(c["mk"], dtype=dt) if masks else None
    if tanh is None:
        enc, cT, hT = encoder_torch({"rnn_config": {"enc_layers": nl}}, Pt, xt, mk)
    else:
        enc, cT, hT = encoder_with(tanh, Pt, xt, nl, mk)
    tt = lambda a: torch.tensor(a, dtype=dt)
    (enc * tt(c["g_enc"])).sum().add((cT * tt(c["g_c"])).sum()).add((hT * tt(c["g_h"])).sum()).backward()
    fwd = {"enc": enc.detach().numpy(), "cT": cT.detach().numpy(), "hT": hT.detach().numpy()}
    grads = {k: (p.grad.numpy() if p.grad is not None else np.zeros(p.shape)) for k, p in Pt.items()}
    grads["dx"] = xt.grad.numpy()
    return fwd, grads


def lstm_feasibility(shape, rung, tanh=None):
    T, B, in_dim, h, nl, masks = shape
    c = RC.lstm_draws(T, B, in_dim, h, nl, masks, bias_gain=rung[0], x_gain=rung[1])
    f64, g64 = lstm_run(c, nl, masks, torch.float64)
    f32, g32 = lstm_run(c, nl, masks, torch.float32, tanh)
    return max(frac(f32[k], f64[k]) for k in f64), max(frac(g32[k], g64[k]) for k in g64), c


@pytest.mark.parametrize("shape,rung", [c[:2] for c in RC.LSTM_CASES] + [RC.LSTM_ROWS32_CASE], ids=_ids)
def test_lstm_saturation_rungs_are_feasible(shape, rung):
    fwd, grad, c = lstm_feasibility(shape, rung)
    share, zmax = RC.saturation(RC.lstm_preacts(c, shape[4], shape[5]))
    print(f"{shape} {rung}: fwd {fwd:.1e} grad {grad:.1e} saturated share {share:.2f} max |z| {zmax:.1f}")
    assert share >= 0.10 and zmax >= 44, (share, zmax)
    assert fwd <= FWD / 4 and grad <= GRAD / 4, (fwd, grad)


# ------------------------------------------------------------------ CNN front-end with offset channels
def cnn_f32(cfg, P, X, noise, gout, dt=torch.float32, one_pass=False, eps=2e-5):
    """The front-end in plain torch formulas on `dt` tensors, training-mode BatchNorm with a two-pass variance (one_pass: E[y^2] - E[y]^2,
    what the teeth test runs): -> (out (T'', B, C F'), per-layer (mean, biased variance), gradients of W / gamma / beta)."""
    Pt = {k: torch.tensor(v, dtype=dt, requires_grad="avg" not in k) for k, v in P.items() if k.startswith("CNN")}
    h = torch.tensor(X * (noise if noise is not None else 1.0), dtype=dt).unsqueeze(1)
    stats = []
    for i, l in enumerate(cfg["cnn_config"]["cnn_layers"]):
        y = torch.nn.functional.conv2d(h, Pt[f"CNN_{i}/W"], stride=tuple(l["stride"]), padding=tuple(l["pad"]))
        mean = y.mean(dim=(0, 2, 3), keepdim=True)
        var = ((y * y).mean(dim=(0, 2, 3), keepdim=True) - mean * mean).clamp_min(0) if one_pass else ((y - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        stats.append((mean.detach().flatten().numpy(), var.detach().flatten().numpy()))
        g, b = Pt[f"CNN_{i}_bn/gamma"].view(1, -1, 1, 1), Pt[f"CNN_{i}_bn/beta"].view(1, -1, 1, 1)
        h = torch.relu((y - mean) / torch.sqrt(var + eps) * g + b)
    Bc, Cc, T2, F2 = h.shape
    out = h.permute(2, 0, 1, 3).reshape(T2, Bc, Cc * F2)
    if gout is not None:
        out.backward(torch.tensor(gout, dtype=dt))
    return out.detach().numpy(), stats, {k: p.grad.numpy() for k, p in Pt.items() if p.grad is not None}


def cnn_feasibility(shape, with_noise, x_offset, one_pass=False, seed=0, **kw):
    """-> dict of fracs (out, layer-0/1 mean and variance, worst gradient of each layer), r, near-kink flag of layer 0."""
    B, T, D, c0, c1 = shape
    cfg, P, X, noise, rng = RC.cnn_draws(B, T, D, c0, c1, with_noise, x_offset=x_offset, seed=seed, **kw)
    X32 = X.astype(np.float32).astype(np.float64)                       # what the device sees; the float64 reference keeps the float64 draw
    n32 = None if noise is None else noise.astype(np.float32).astype(np.float64)
    out64, st64, _ = cnn_f32(cfg, P, X, noise, None, torch.float64)
    gout = rng.standard_normal(out64.shape)
    near = RC.cnn_near_kink(cfg, P, X, noise)
    gout[near[1]] = 0.0
    out64, st64, g64 = cnn_f32(cfg, P, X, noise, gout, torch.float64)
    out32, st32, g32 = cnn_f32(cfg, P, X32, n32, gout, torch.float32, one_pass)
    res = {"out": frac(out32, out64)}
    for i in range(2):
        res[f"mean{i}"] = frac(0.1 * st32[i][0], 0.1 * st64[i][0])
        res[f"var{i}"] = frac(0.9 + 0.1 * st32[i][1], 0.9 + 0.1 * st64[i][1])
        res[f"grad{i}"] = max(frac(g32[k], g64[k]) for k in g64 if k.startswith(f"CNN_{i}"))
    return res, RC.cnn_layer0_ratio(cfg, P, X, noise), bool(near[0].any())


def cnn_within(res, near0, share=0.5):
    return (res["out"] <= FWD * share and all(res[k] <= FWD * share for k in ("mean0", "var0", "mean1", "var1"))
            and res["grad1"] <= GRAD * share and res["grad0"] <= (5e-3 if near0 else GRAD) * share)


@pytest.mark.parametrize("shape,with_noise,x_offset,seed,centre,_one_pass_fails", RC.CNN_CASES, ids=_ids)
def test_cnn_offset_rungs_are_feasible(shape, with_noise, x_offset, seed, centre, _one_pass_fails):
    res, r, near0 = cnn_feasibility(shape, with_noise, x_offset, seed=seed, **RC.cnn_case_kw(centre))
    print(f"{shape} noise {with_noise} x_offset {x_offset}: r {r:.1f} " + " ".join(f"{k} {v:.1e}" for k, v in res.items()))
    assert r >= x_offset / 2, r
    assert cnn_within(res, near0), res


def cnn_geometry_feasibility(B, T, D, layers, with_noise, seed):
    """A geometry case of RC.CNN_GEOMETRY_CASES on the CPU: oracle.ast_ref_torch.cnn_torch in float32 against its float64 self -> (near-kink
    units per layer on the float64 reference, output error, worst gradient error), errors as fractions of the reference tensor's maximum."""
    from oracle.ast_ref_torch import cnn_torch
    cfg, P, X, noise, rng = RC.cnn_draws(B, T, D, None, None, with_noise, seed=seed, layers=layers)
    near = [int(m.sum()) for m in RC.cnn_near_kink_layers(cfg, P, X, noise)]
    res, gout = {}, None
    for dt in (torch.float64, torch.float32):
        Pt = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in P.items() if k.startswith("CNN") and "avg" not in k}
        out = cnn_torch(cfg, Pt, torch.tensor(X, dtype=dt), None if noise is None else torch.tensor(noise, dtype=dt))
        if gout is None:
            gout = rng.standard_normal(tuple(out.shape))
        out.backward(torch.tensor(gout, dtype=dt))
        res[dt] = (out.detach().numpy(), {k: p.grad.numpy() for k, p in Pt.items()})
    o64, g64 = res[torch.float64]
    o32, g32 = res[torch.float32]
    return near, frac(o32, o64), max(frac(g32[k], g64[k]) for k in g64)


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("cid,B,T,D,layers,seed,seed_noisy", RC.CNN_GEOMETRY_CASES, ids=[c[0] for c in RC.CNN_GEOMETRY_CASES])
def test_cnn_geometry_cases_are_kink_free_and_feasible(cid, B, T, D, layers, seed, seed_noisy, with_noise):
    """The committed seeds leave no unit of any layer within 2e-5 of the ReLU's kink on the float64 reference (so the GPU test holds every
    gradient to 5e-4), and the plain float32 restatement meets a quarter of the GPU test's bounds on every case."""
    near, out, grad = cnn_geometry_feasibility(B, T, D, layers, with_noise, seed_noisy if with_noise else seed)
    print(f"{cid} noise {with_noise}: near {near} out {out:.1e} grad {grad:.1e}")
    assert near == [0] * len(layers), near
    assert out <= FWD / 4 and grad <= GRAD / 4, (out, grad)


# ------------------------------------------------------------------ attention and softmax-CE value cases (operator level)
def attn_f32(enc, q, dt=torch.float32, subtract_max=True):
    e, qq = torch.tensor(enc, dtype=dt), torch.tensor(q, dtype=dt)
    s = torch.einsum("bth,bh->bt", e, qq)
    if subtract_max:
        a = torch.softmax(s, 1)
    else:
        w = torch.exp(s)
        a = w / w.sum(1, keepdim=True)
    return a.numpy(), torch.einsum("bth,bt->bh", e, a).numpy()


def attn_bwd(enc, q, g, dt):
    e, qq = torch.tensor(enc, dtype=dt), torch.tensor(q, dtype=dt)
    s = torch.einsum("bth,bh->bt", e, qq).requires_grad_()
    torch.einsum("bth,bt->bh", e, torch.softmax(s, 1)).backward(torch.tensor(g, dtype=dt))
    return s.grad.numpy(), torch.einsum("bt,bth->bh", s.grad, e).numpy()


@pytest.mark.parametrize("B,T,H", RC.ATTN_SHAPES)
def test_attention_value_cases_are_feasible(B, T, H):
    enc, q = RC.attn_case("wide", B, T, H)
    a64, cv64 = attn_f32(enc, q, torch.float64)
    s = np.einsum("bth,bh->bt", enc.astype(np.float64), q.astype(np.float64))
    assert (s.max(1) - s.min(1)).min() >= 200
    a32, cv32 = attn_f32(enc, q)
    g = RC.attn_upstream(B, T, H)
    ds64, dq64 = attn_bwd(enc, q, g, torch.float64)
    ds32, dq32 = attn_bwd(enc, q, g, torch.float32)
    figs = dict(alpha=frac(a32, a64), cv=frac(cv32, cv64), ds=frac(ds32, ds64), dq=frac(dq32, dq64))
    print(f"wide {(B, T, H)}: " + " ".join(f"{k} {v:.1e}" for k, v in figs.items()))
    assert figs["alpha"] <= FWD / 4 and figs["cv"] <= FWD / 4 and figs["ds"] <= GRAD / 4 and figs["dq"] <= GRAD / 4, figs
    for kind, pos in [("plant", p) for p in RC.attn_positions(T)] + [("tie", None)]:
        enc, q = RC.attn_case(kind, B, T, H, pos=pos)
        a64, cv64 = attn_f32(enc, q, torch.float64)
        want = np.zeros((B, T))
        if kind == "plant":
            want[:, pos] = 1.0
        else:
            want[:, 0] = want[:, T - 1] = 0.5
        assert frac(a64, want) <= 1e-12, (kind, pos)                   # the defining property, on the reference
        a32, cv32 = attn_f32(enc, q)
        assert frac(a32, want) <= FWD / 4 and frac(cv32, enc[:, 0 if kind == "tie" else pos]) <= FWD / 4, (kind, pos)
    enc0, q0 = RC.attn_case("base", B, T, H)
    a0 = attn_f32(enc0, q0, torch.float64)[0]
    level = RC.ATTN_LEVEL[(B, T, H)]
    for sign in (-1, 1):
        enc, q = RC.attn_case("level", B, T, H, level=sign * level)
        s = np.einsum("bth,bh->bt", enc.astype(np.float64), q.astype(np.float64))
        assert np.abs(s.mean(1) - sign * level).max() <= 0.05 * level
        f = frac(attn_f32(enc, q)[0], a0)
        print(f"level {sign * level:+.0f} {(B, T, H)}: alpha {f:.1e}")
        assert f <= FWD / 4, (sign, f)


def ce_f32(x, t, w, scale, dt=torch.float32):
    V = x.shape[1]
    xt = torch.tensor(x, dtype=dt, requires_grad=True)
    tc = torch.tensor(np.minimum(t, V - 1)).long()
    rows = torch.nn.functional.cross_entropy(xt, tc, weight=torch.tensor(w, dtype=dt), reduction="none") * scale
    rows.sum().backward()
    return rows.detach().numpy(), xt.grad.numpy()


@pytest.mark.parametrize("V", RC.CE_VOCABS)
@pytest.mark.parametrize("kind", RC.CE_KINDS)
def test_softmax_ce_value_cases_are_feasible(kind, V):
    x, t, w = RC.ce_case(kind, V)
    r64, g64 = ce_f32(x, t, w, 1.0 / x.shape[0], torch.float64)
    r32, g32 = ce_f32(x, t, w, 1.0 / x.shape[0])
    assert np.abs(r32 - r64).max() <= RC.ce_row_bound(x, r64, rel=0.25e-5), (r32, r64)
    assert np.abs(g32 - g64).max() <= RC.ce_grad_bound(x, g64, FWD / 4)
    if kind == "wide" and V >= 255:
        assert (x.max(1) - x.min(1)).min() >= 200
    if kind.startswith("tie") and V > 2:
        assert ((x == x.max(1, keepdims=True)).sum(1) == 2).all()


# ------------------------------------------------------------------ the assertions have teeth
def norm_f32(x, gamma, beta, eps, dt, one_pass=False):
    """relu-less normalisation over dim 1 of x (.., n, ..) in plain formulas on `dt` tensors: -> y = (x - mu) / sqrt(var + eps) * gamma + beta."""
    x, gamma, beta = x.to(dt), gamma.to(dt), beta.to(dt)
    mu = x.mean(1, keepdim=True)
    var = ((x * x).mean(1, keepdim=True) - mu * mu).clamp_min(0) if one_pass else ((x - mu) ** 2).mean(1, keepdim=True)
    return ((x - mu) / torch.sqrt(var + eps) * gamma + beta).double()


def norm_offset_rows():
    """The offset rows of tests/test_gpu_options.py (same distributions; the draws there come from the device's generator): per-step
    BatchNorm over the B rows of a step (z (T, B, C) + 64, statistics over dim 1, bound 2e-5) and LayerNorm (x (rows, n) + 64, bound 1e-5).
    -> name, x, gamma, beta, eps, bound, keep (the two-row shape: the (step, channel) pairs with |z1 - z2| >= 0.5, as the GPU test compares)."""
    gen = torch.Generator().manual_seed(7)
    for T, B, Cc in ((17, 2, 100), (40, 32, 64)):
        z = (torch.randn(T, B, Cc, generator=gen) * 1.5 + 0.3 + 64).float()
        keep = ((z[:, 0] - z[:, 1]).abs() >= 0.5).double().unsqueeze(1) if B == 2 else 1.0
        yield f"step-bn {(T, B, Cc)}", z, torch.randn(Cc, generator=gen), torch.randn(Cc, generator=gen), 2e-5, 2e-5, keep
    for rows, n in ((33, 100), (130, 256)):
        x = (torch.randn(rows, n, generator=gen) * 2 + 0.5 + 64).float()
        yield f"layernorm {(rows, n)}", x, torch.randn(1, n, generator=gen), torch.randn(1, n, generator=gen), 1e-6, 1e-5, 1.0


def norm_frac(got, ref, keep):
    return float(((got - ref) * keep).abs().max() / ref.abs().max())


def test_norm_offset_rows_are_feasible():
    for name, x, gamma, beta, eps, bound, keep in norm_offset_rows():
        ref = norm_f32(x, gamma, beta, eps, torch.float64)
        f = norm_frac(norm_f32(x, gamma, beta, eps, torch.float32), ref, keep)
        print(f"{name}: two-pass float32 {f:.1e} (bound {bound:.0e})")
        assert f <= bound / 2, (name, f)


def test_one_pass_float32_variance_fails_the_offset_cases():
    """E[y^2] - E[y]^2 in float32 fails the bounds of the statistics family where a channel's mean really lies far from 0: the CNN
    operator's rows marked one_pass_fails (r = 98-154: the very assertions of the GPU test, cnn_within at the full tolerance), and the
    offset rows of the per-step BatchNorm and LayerNorm kernels."""
    for shape, with_noise, x_offset, seed, centre, fails in RC.CNN_CASES:
        if fails:
            res, r, near0 = cnn_feasibility(shape, with_noise, x_offset, one_pass=True, seed=seed, **RC.cnn_case_kw(centre))
            print(f"one-pass {shape} x_offset {x_offset}: r {r:.1f} " + " ".join(f"{k} {v:.1e}" for k, v in res.items()))
            assert not cnn_within(res, near0, share=1.0), (shape, res)
    for name, x, gamma, beta, eps, bound, keep in norm_offset_rows():
        ref = norm_f32(x, gamma, beta, eps, torch.float64)
        f = norm_frac(norm_f32(x, gamma, beta, eps, torch.float32, one_pass=True), ref, keep)
        print(f"{name}: one-pass float32 {f:.1e} (bound {bound:.0e})")
        assert not f <= bound, (name, f)


def test_softmax_without_the_maximum_fails_the_wide_and_level_cases():
    for B, T, H in RC.ATTN_SHAPES:
        for kind, kw in (("wide", {}), ("plant", {"pos": T - 1}), ("level", {"level": RC.ATTN_LEVEL[(B, T, H)]})):
            enc, q = RC.attn_case(kind, B, T, H, **kw)
            with np.errstate(all="ignore"):
                a32 = attn_f32(enc, q, subtract_max=False)[0]
            a64 = attn_f32(enc, q, torch.float64)[0]
            assert not frac(a32, a64) <= FWD, (kind, B, T, H)


def test_tanh_from_exp_2x_fails_the_saturated_cases():
    def naive(x):
        e = torch.exp(2 * x)
        return (e - 1) / (e + 1)
    for shape, rung, _, _ in RC.LSTM_CASES[:2]:
        fwd, grad, _ = lstm_feasibility(shape, rung, tanh=torch.tanh)          # the local restatement itself is right
        assert fwd <= FWD / 4 and grad <= GRAD / 4, (shape, fwd, grad)
        fwd, grad, _ = lstm_feasibility(shape, rung, tanh=naive)
        assert not (fwd <= FWD and grad <= GRAD), (shape, fwd, grad)
