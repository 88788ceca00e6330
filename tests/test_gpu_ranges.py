"""GPU parity tests outside the benign value range: the operator tests of tests/test_gpu_ops.py draw zero-mean unit Gaussians throughout
(attention scores within +-20, logits and gate pre-activations within a few units, BatchNorm channels centred on 0); here the same
operators run on offset, peaked, tied, flat and saturated inputs -- where exp(s - max) reaches 0, a gate sits at 0 or 1, a merge meets
an empty partial or a channel's mean lies several standard deviations from 0.  Same references (float64), same helpers and the same
tolerances as the operator tests: 2e-4 forward, 5e-4 gradients, 1e-4 loss, tokens equal; close() fails on NaN / inf.  The cases, their
gain rungs and defining properties live in tests/range_cases.py; tests/test_ranges_host.py shows on the CPU that a plain float32
restatement meets a quarter of these tolerances on every one of them.  Schemes: bf16x3 and f32 (fp16x2's documented domain -- 22 bits
below the operand's largest entry -- excludes an offset of 64 on unit-variance data by construction)."""
import ctypes as C

import numpy as np
import pytest
import torch

import range_cases as RC
from test_gpu_ops import GuardedWS, _cnn_case, _dec_setup, _decoder_case, _lstm_stack_case, close, dev, ok, stream, vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


@pytest.fixture(params=["bf16x3", "f32"])
def scheme(request, lib):
    """Moves the PROCESS DEFAULT arithmetic of the f32-accurate products the way test_gpu_ops.py's gemm_split does, and puts it back."""
    prev = lib.astk_set_gemm_precision({"bf16x3": 1, "f32": 2}[request.param])
    yield request.param
    lib.astk_set_gemm_precision(prev)


def _ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else None


# ------------------------------------------------------------------ 2. BatchNorm statistics with offset channels
@pytest.mark.parametrize("shape,with_noise,x_offset,seed,centre", [c[:5] for c in RC.CNN_CASES], ids=_ids)
def test_cnn_batchnorm_statistics_with_offset_channels(lib, shape, with_noise, x_offset, seed, centre, scheme):
    """astk_conv_bn_relu_fwd / _bwd, train and eval mode, on an input with an offset (tests/range_cases.py, CNN_CASES: the largest layer-0
    |channel mean| / std is at least x_offset / 2 -- 51 to 154 on the x_offset = 64 rows): output, running statistics of both layers'
    formulas, the six gradient tensors under the near-kink rule, eval-mode output -- the operator test's body on the offset input."""
    kw = RC.cnn_case_kw(centre)
    cfg, P, X, noise, _ = RC.cnn_draws(*shape, with_noise, x_offset=x_offset, seed=seed, **kw)
    assert RC.cnn_layer0_ratio(cfg, P, X, noise) >= x_offset / 2
    _cnn_case(lib, *shape, with_noise, x_offset=x_offset, seed=seed, layer1_stats=True, **kw)


# ------------------------------------------------------------------ 3a. attention, operator level
def _attn_fwd(lib, enc, q, rows=None):
    """-> alpha (B, T), cv (B, H) of astk_attn_step_fwd (rows = (row_utt, row_len): astk_attn_step_fwd_rows), plus what the backward needs."""
    R, H = q.shape
    T = enc.shape[1]
    Tp = (T + 3) // 4 * 4
    nbytes = lib.astk_attn_workspace_bytes(R, T, H)
    ws = GuardedWS(nbytes)
    ed, qd = dev(enc), dev(q)
    a_d, cv_d = torch.full((R, Tp), 7.0, device="cuda"), torch.zeros(R, H, device="cuda")
    if rows is None:
        ok(lib, lib.astk_attn_step_fwd(R, T, H, vp(ed), vp(qd), vp(a_d), vp(cv_d), vp(ws), nbytes, stream()))
    else:
        ru, rl = dev(rows[0], torch.int32), dev(rows[1], torch.int32)
        ok(lib, lib.astk_attn_step_fwd_rows(R, T, H, vp(ed), vp(ru), vp(rl), vp(qd), vp(a_d), vp(cv_d), vp(ws), nbytes, stream()))
    ws.check("attn fwd")
    return a_d, cv_d, ed, ws, nbytes


def _attn_bwd(lib, ed, a_d, cv_d, g, ws, nbytes):
    B, H = cv_d.shape
    T = ed.shape[1]
    ds_d, dq_d = torch.zeros_like(a_d), torch.zeros(B, H, device="cuda")
    g_d = dev(g)
    ok(lib, lib.astk_attn_step_bwd(B, T, H, vp(ed), vp(a_d), vp(cv_d), vp(g_d), vp(ds_d), vp(dq_d), vp(ws), nbytes, stream()))
    ws.check("attn bwd")
    return ds_d[:, :T], dq_d


def _attn_ref(enc, q, g=None):
    e, qq = torch.tensor(enc, dtype=torch.float64), torch.tensor(q, dtype=torch.float64)
    s = torch.einsum("bth,bh->bt", e, qq).requires_grad_()
    a = torch.softmax(s, 1)
    cv = torch.einsum("bth,bt->bh", e, a)
    if g is None:
        return s.detach(), a.detach(), cv.detach()
    cv.backward(torch.tensor(g, dtype=torch.float64))
    return s.detach(), a.detach(), cv.detach(), s.grad, torch.einsum("bt,bth->bh", s.grad, e)


@pytest.mark.parametrize("B,T,H", RC.ATTN_SHAPES)
def test_attention_wide_scores(lib, B, T, H):
    """Every row's scores span more than 200: most partials underflow against the row's maximum, inside a wave, across the waves of a
    workgroup and across the splits."""
    enc, q = RC.attn_case("wide", B, T, H)
    g = RC.attn_upstream(B, T, H)
    s, alpha, cv, ds, dq = _attn_ref(enc, q, g)
    assert float((s.max(1).values - s.min(1).values).min()) >= 200
    a_d, cv_d, ed, ws, nbytes = _attn_fwd(lib, enc, q)
    close(a_d[:, :T], alpha, msg="alpha")
    close(cv_d, cv, msg="cv")
    ds_d, dq_d = _attn_bwd(lib, ed, a_d, cv_d, g, ws, nbytes)
    close(ds_d, ds, rtol=5e-4, msg="ds")
    close(dq_d, dq, rtol=5e-4, msg="dq")


@pytest.mark.parametrize("B,T,H", RC.ATTN_SHAPES)
def test_attention_planted_maximum_at_every_position_class(lib, B, T, H):
    """One enc row scores 300 above the rest -- first and last row, the rows around the waves' stride of 8 with its +4 pair, the middle
    (a split boundary) -- and, last, rows 0 and T - 1 tie at that level (the maximum in the first AND the last split): alpha is the one-hot
    (0.5 / 0.5) vector, cv that row, the backward finite."""
    g = RC.attn_upstream(B, T, H)
    for kind, pos in [("plant", p) for p in RC.attn_positions(T)] + [("tie", None)]:
        enc, q = RC.attn_case(kind, B, T, H, pos=pos)
        want = np.zeros((B, T))
        if kind == "plant":
            want[:, pos] = 1.0
        else:
            want[:, 0] = want[:, T - 1] = 0.5
        assert float((_attn_ref(enc, q)[1] - torch.tensor(want)).abs().max()) < 1e-12
        a_d, cv_d, ed, ws, nbytes = _attn_fwd(lib, enc, q)
        close(a_d[:, :T], want, msg=f"alpha ({kind} {pos})")
        close(cv_d, enc[:, 0 if kind == "tie" else pos], msg=f"cv ({kind} {pos})")
        ds_d, dq_d = _attn_bwd(lib, ed, a_d, cv_d, g, ws, nbytes)
        assert bool(torch.isfinite(ds_d).all()) and bool(torch.isfinite(dq_d).all()), (kind, pos)


@pytest.mark.parametrize("B,T,H", RC.ATTN_SHAPES)
def test_attention_flat_scores_and_score_level(lib, B, T, H):
    """q = 0: alpha = 1 / T to 1e-6 relative, cv the mean of the rows.  Then every score shifted by -level and +level: alpha must be the
    unshifted case's -- nothing may depend on the absolute level, the running maximum starts at -inf."""
    enc, q = RC.attn_case("flat", B, T, H)
    a_d, cv_d = _attn_fwd(lib, enc, q)[:2]
    assert float((a_d[:, :T].double() * T - 1).abs().max()) <= 1e-6
    close(cv_d, enc.astype(np.float64).mean(1), msg="cv (flat)")
    enc0, q0 = RC.attn_case("base", B, T, H)
    alpha0 = _attn_ref(enc0, q0)[1]
    close(_attn_fwd(lib, enc0, q0)[0][:, :T], alpha0, msg="alpha (base)")
    level = RC.ATTN_LEVEL[(B, T, H)]
    for sign in (-1, 1):
        enc, q = RC.attn_case("level", B, T, H, level=sign * level)
        close(_attn_fwd(lib, enc, q)[0][:, :T], alpha0, msg=f"alpha (level {sign * level:+.0f})")


@pytest.mark.parametrize("kind", ["wide", "plant"])
def test_attention_rows_with_whole_splits_behind_a_rows_length(lib, kind):
    """astk_attn_step_fwd_rows: six rows over two utterances, lengths 1, 2, 50 and 201 of T = 201 -- the splits that lie behind a short
    row's length contribute empty partials (m = -inf, l = 0) to the merge -- under the wide and the planted-at-the-last-row scores."""
    enc, q, row_utt, row_len = RC.attn_rows_case(kind)
    a_d, cv_d = _attn_fwd(lib, enc, q, rows=(row_utt, row_len))[:2]
    a, cv = a_d.cpu().double().numpy(), cv_d.cpu().double().numpy()
    for r in range(len(row_len)):
        n, e = int(row_len[r]), enc[row_utt[r]].astype(np.float64)
        s = e[:n] @ q[r].astype(np.float64)
        if kind == "wide" and n > 1:
            assert s.max() - s.min() >= 200
        w = np.exp(s - s.max())
        w /= w.sum()
        if kind == "plant":
            assert w[n - 1] > 1 - 1e-12
        assert (a[r, n:] == 0).all(), f"row {r}: alpha behind the row's length"
        close(a[r, :n], w, msg=f"alpha row {r}")
        close(cv[r], w @ e[:n], msg=f"cv row {r}")


# ------------------------------------------------------------------ 3b / 4 / 5. through the decoder loops
def _decoder_range_case(lib, tune, shape, seed_off, loop="persist", knobs=(), **gains):
    B, L, T, H, E, A, V, nl, masks = shape
    per_launch = loop == "per_launch"
    if per_launch:
        tune("dec.persist", 0, lib)
    for k in knobs:
        tune(k, 0, lib)
    s = _dec_setup(lib, B, L, T, H, E, A, V, nl, masks, seed=B + L + seed_off, **gains)
    path = lib.astk_decoder_path(C.byref(s["d"]))
    if per_launch:
        assert not (path & 1)
        host = (C.c_int32 * s["S"])(*[int(f) for f in s["flags"]])
        s["d"].use_truth_host = C.cast(host, C.POINTER(C.c_int32))
        s["_host_flags"] = host
    elif H == 1024:
        assert path == 16
    else:
        assert path & 1, "persistent decoder path not taken"
        assert bool(path & 4) == (B > 32 and H == 512), "row split"
    scores, logits, z = RC.dec_step0(s, nl)
    if gains.get("enc_gain", 1.0) != 1.0:
        RC.assert_score_ranges(scores.max(1) - scores.min(1), H)
    if gains.get("out_gain", 1.0) != 1.0:
        assert (logits.max(1) - logits.min(1)).min() >= 200
    if gains.get("bias_gain", 1.0) != 1.0:
        share, zmax = RC.saturation(z)
        assert share >= RC.DEC_SATURATED[gains["bias_gain"]][0] and zmax >= RC.DEC_SATURATED[gains["bias_gain"]][1], (share, zmax)
    _decoder_case(lib, s, B, L, T, H, E, A, V, nl, masks)


@pytest.mark.parametrize("shape,seed_off,rung,loop", [c[:4] for c in RC.DEC_ENC_CASES], ids=_ids)
def test_decoder_loops_over_wide_attention_scores(lib, tune, shape, seed_off, rung, loop, scheme):
    """astk_decoder_fwd + _bwd with the encoder states at the table's gain: one shape per attention-scan implementation (generic, resident
    H = 512 with 1 and 3 layers, streamed, row split, wide, and the per-launch loop), step-0 score ranges past exp's underflow."""
    _decoder_range_case(lib, tune, shape, seed_off, loop, enc_gain=rung)


@pytest.mark.parametrize("env", ["dec.b6_fused", "dec.b6_split"])
def test_decoder_older_role_layouts_over_wide_attention_scores(lib, tune, env):
    shape, seed_off, rung = RC.DEC_ENC_KNOB_CASE
    _decoder_range_case(lib, tune, shape, seed_off, knobs=(env,), enc_gain=rung)


@pytest.mark.parametrize("shape,seed_off,loop", RC.DEC_OUT_CASES, ids=_ids)
def test_decoder_loops_cross_entropy_roles_over_wide_logits(lib, tune, shape, seed_off, loop, scheme):
    """The CE roles inside the loops (per launch, persistent with 1 and 3 layers, wide with the largest vocabulary: the most per-tile
    (max, sum) pairs to merge) on logits that span more than 200 in every row of step 0."""
    _decoder_range_case(lib, tune, shape, seed_off, loop, out_gain=RC.OUT_GAIN)


@pytest.mark.parametrize("bias_gain", RC.DEC_BIAS_GAINS)
@pytest.mark.parametrize("shape,seed_off", RC.DEC_BIAS_CASES, ids=_ids)
def test_decoder_loops_with_saturated_gates(lib, tune, shape, seed_off, bias_gain, scheme):
    """The fast gates of the persistent loops (rcp(1 + __expf(..)), csrc/handoff.h) on pre-activations far from 0, forward and backward."""
    _decoder_range_case(lib, tune, shape, seed_off, bias_gain=bias_gain)


# ------------------------------------------------------------------ 5. encoder stacks with saturated gates
@pytest.mark.parametrize("shape,rung", [c[:2] for c in RC.LSTM_CASES], ids=_ids)
def test_lstm_stacks_with_saturated_gates(lib, shape, rung, scheme):
    """One shape per kernel family (per launch, persistent h = 64 / 256 / 512, hoisted h = 1024): forward states and all gradients with
    at least a tenth of the i / f / o gates within 1e-6 of 0 or 1 and pre-activations beyond |z| = 44, where __expf's argument overflows."""
    T, B, in_dim, h, nl, masks = shape
    c = RC.lstm_draws(T, B, in_dim, h, nl, masks, bias_gain=rung[0], x_gain=rung[1])
    share, zmax = RC.saturation(RC.lstm_preacts(c, nl, masks))
    assert share >= 0.10 and zmax >= 44, (share, zmax)
    _lstm_stack_case(lib, T, B, in_dim, h, nl, masks, bias_gain=rung[0], x_gain=rung[1])


@pytest.mark.parametrize("form", [1, 2])
def test_lstm_32_row_forms_with_saturated_gates(lib, tune, form, scheme):
    shape, rung = RC.LSTM_ROWS32_CASE
    tune("lstm.rows32", form, lib)
    T, B, in_dim, h, nl, masks = shape
    _lstm_stack_case(lib, T, B, in_dim, h, nl, masks, bias_gain=rung[0], x_gain=rung[1])


# ------------------------------------------------------------------ 4. softmax cross-entropy, operator level
def _ce_run(lib, x, t, w, ld, t_stride=1, t_col=0, rows=True, argmax=True):
    B, V = x.shape
    buf = torch.zeros(B, ld, device="cuda")
    buf[:, :V] = dev(x)
    tm = np.full((B, t_stride), -7, np.int32)                         # the targets in column t_col of a (B, t_stride) matrix
    tm[:, t_col] = t
    t_d, w_d = dev(tm, torch.int32), dev(w)
    rows_d = torch.zeros(B, device="cuda") if rows else None
    am_d = torch.full((B,), -1, dtype=torch.int32, device="cuda") if argmax else None
    ok(lib, lib.astk_softmax_ce_fwd(B, V, ld, vp(buf), C.c_void_p(t_d.data_ptr() + 4 * t_col), t_stride, vp(w_d), 1.0 / B, vp(rows_d),
                                    vp(am_d), stream()))
    torch.cuda.synchronize()
    return buf, rows_d, am_d


@pytest.mark.parametrize("V", RC.CE_VOCABS)
@pytest.mark.parametrize("kind", RC.CE_KINDS)
def test_softmax_ce_value_cases(lib, kind, V):
    """astk_softmax_ce_fwd against float64 cross_entropy on logits ~ N(0, 60^2), at +-1e4, with the target at the row's minimum / maximum,
    an exact maximum duplicated inside one thread's stride and across waves (argmax = the first), a target id of V (clamped, quirk Q8), a
    class-weight-0 target, vocabularies below, at and above a workgroup: loss rows to 1e-5 relative (range_cases.ce_row_bound), gradient through close(), argmax
    exact, padding columns exactly 0; then the same through a (B, L) target matrix read at a middle column, and with null outputs."""
    x, t, w = RC.ce_case(kind, V)
    B, ld = x.shape[0], V + 3
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tc = torch.tensor(np.minimum(t, V - 1)).long()
    want = torch.nn.functional.cross_entropy(xt, tc, weight=torch.tensor(w, dtype=torch.float64), reduction="none") / B
    want.sum().backward()
    want = want.detach().numpy()
    for t_stride, t_col in ((1, 0), (5, 2)):
        buf, rows_d, am_d = _ce_run(lib, x, t, w, ld, t_stride, t_col)
        got = rows_d.cpu().double().numpy()
        assert np.abs(got - want).max() <= RC.ce_row_bound(x, want), (got, want)
        close(buf[:, :V], xt.grad, atol=RC.ce_grad_bound(x, xt.grad.numpy()), msg="dlogits")
        assert float(buf[:, V:].abs().max()) == 0.0
        assert (am_d.cpu().numpy() == x.argmax(1)).all(), "argmax (first maximum)"
        if V > 1:                                                     # row 0's target has class weight 0
            assert float(rows_d[0]) == 0.0 and float(buf[0, :V].abs().max()) == 0.0
        if kind == "tmin" and V > 1:                                  # p underflows: the gradient at the target is -scale w
            g = buf.cpu().numpy()
            assert all(g[b, t[b]] == np.float32(-1.0 / B) for b in range(1, B) if xt.grad[b, t[b]] == -1.0 / B)
    buf2, _, _ = _ce_run(lib, x, t, w, ld, rows=False, argmax=False)
    assert torch.equal(buf2, buf), "null loss_rows / argmax change the gradient"
