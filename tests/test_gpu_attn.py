"""GPU tests of the attention scan (ast_amd/csrc/attn.hip) at every width, split plan and row length: astk_attn_step_fwd, _bwd and
_fwd_rows against the float64 reference of tests/attn_model.py on its case tables -- every instantiation NCH = 1, 2, 4, 8 with ragged and
one-lane last chunks, nsplit = 1 by T and by B >= 512 (both sides of 511 / 512 rows), exactly MAX_SPLIT = 128, the clamp, last chunks of one
and two rows, row lengths 0, 1, around a chunk boundary, T and above T.  Bounds: the operator test's (2e-4 of the largest reference entry
for alpha and cv, 5e-4 for ds and dq); tests/test_attn_host.py shows on the CPU that a float32 restatement of the kernel stays below 0.4 %
of them on every case and that planted mistakes in these branches break them.  Outputs start NaN-filled with a spare NaN row behind alpha
and ds, the workspace sits between guard bands, the ticket counters must read zero after every launch, and a second forward with other
inputs runs on the same workspace (a partial left over from the first launch must not be read)."""
import numpy as np
import pytest
import torch

import attn_model as AM
from test_gpu_ops import GuardedWS, close, dev, ok, stream, vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _counters(ws, c):
    torch.cuda.synchronize()
    off = AM.counters_offset(c.B, c.T, c.H)
    return ws.t[off:off + 4 * c.B].view(torch.int32)


def _workspace(lib, c):
    nbytes = lib.astk_attn_workspace_bytes(c.B, c.T, c.H)
    assert nbytes == AM.workspace_bytes(c.B, c.T, c.H), "tests/attn_model.py no longer restates attn.hip's plan"
    return GuardedWS(nbytes), nbytes


def _ratios(c, tag, **pairs):
    """prints error / bound per output (the figures DESIGN.md records), then asserts with the operator tests' close()."""
    r = {k: AM.bound_ratio(got.detach().cpu().numpy(), ref, AM.RTOL[k]) for k, (got, ref) in pairs.items()}
    print(f"attn-ratio {'rows-' if c.rows else ''}{c.id} {tag} " + " ".join(f"{k}={v:.4f}" for k, v in r.items()))
    for k, (got, ref) in pairs.items():
        close(got, ref, rtol=AM.RTOL[k], msg=f"{k} ({tag})")


def _forward(lib, c, which, ws, nbytes):
    """one forward launch into NaN-filled outputs -> alpha (B, Tp), cv (B, H) on the device, after every check of the forward."""
    enc, q, _ = c.inputs(which)
    Tp = AM.padded(c.T)
    a_d, cv_d = _nan(c.B + 1, Tp), _nan(c.B + 1, c.H)
    if c.rows:
        ed, qd = dev(c.poisoned(enc, which)), dev(q)
        ru, rl = dev(np.asarray(c.row_utt), torch.int32), dev(c.lengths(which), torch.int32)
        ok(lib, lib.astk_attn_step_fwd_rows(c.B, c.T, c.H, vp(ed), vp(ru), vp(rl), vp(qd), vp(a_d), vp(cv_d), vp(ws), nbytes, stream()))
        alpha, cv = AM.reference(enc, q, c.row_utt, c.lengths(which))
    else:
        ed, qd = dev(enc), dev(q)
        ok(lib, lib.astk_attn_step_fwd(c.B, c.T, c.H, vp(ed), vp(qd), vp(a_d), vp(cv_d), vp(ws), nbytes, stream()))
        alpha, cv = AM.reference(enc, q)
    tag = f"forward {which}"
    assert int(_counters(ws, c).abs().sum()) == 0, f"{tag}: ticket counters not back at zero"
    ws.check(tag)
    assert _all_nan(a_d[c.B]) and _all_nan(cv_d[c.B]), f"{tag}: wrote behind the last row"
    a_d, cv_d = a_d[:c.B], cv_d[:c.B]
    Tb = torch.as_tensor(AM.clamp_len(c.lengths(which), c.T) if c.rows else np.full(c.B, c.T), device="cuda")
    behind = torch.arange(Tp, device="cuda")[None, :] >= Tb[:, None]
    assert bool((a_d[behind] == 0).all()), f"{tag}: alpha behind a row's length / in the pad columns must be exactly 0"
    _ratios(c, tag, alpha=(a_d[:, :c.T], alpha[:, :c.T]), cv=(cv_d, cv))
    return ed, a_d, cv_d, alpha, cv


@pytest.mark.parametrize("c", AM.CASES, ids=lambda c: c.id)
def test_attention_scan_forward_backward_forward(lib, c):
    """forward -> backward (on the device's own alpha and cv) -> forward with other inputs, all on one workspace.  Measured on an MI355X,
    largest error / bound over the table: alpha 0.0020 and cv 0.0031 at (1, 1024, 1028), ds 0.0008 at (1, 8, 256), dq 0.0012 at
    (3, 1100, 1540) -- what the float32 model of tests/attn_model.py shows on the CPU."""
    ws, nbytes = _workspace(lib, c)
    ed, a_d, cv_d, alpha, cv = _forward(lib, c, 0, ws, nbytes)
    # backward on the device's own alpha and cv
    enc, _, g = c.inputs(0)
    ds, dq = AM.reference_bwd(enc, alpha, cv, g)
    Tp = AM.padded(c.T)
    ds_d, dq_d, g_d = _nan(c.B + 1, Tp), _nan(c.B + 1, c.H), dev(g)
    ok(lib, lib.astk_attn_step_bwd(c.B, c.T, c.H, vp(ed), vp(a_d), vp(cv_d), vp(g_d), vp(ds_d), vp(dq_d), vp(ws), nbytes, stream()))
    assert int(_counters(ws, c).abs().sum()) == 0, "backward: ticket counters not back at zero"
    ws.check("backward")
    assert _all_nan(ds_d[c.B]) and _all_nan(dq_d[c.B]), "backward: wrote behind the last row"
    _ratios(c, "backward", ds=(ds_d[:c.B, :c.T], ds[:, :c.T]), dq=(dq_d[:c.B], dq))
    # the same workspace, other inputs: nothing of the two launches before may be read
    _forward(lib, c, 1, ws, nbytes)


@pytest.mark.parametrize("c", AM.ROWS_CASES, ids=lambda c: c.id)
def test_attention_scan_rows(lib, c):
    """astk_attn_step_fwd_rows.  enc is NaN behind each utterance's longest row length (a position stays clean if some row of that
    utterance may read it), so a read behind those lengths shows as NaN in alpha or cv; alpha must be exactly 0 at and behind each
    row's clamped length.  The second launch has other inputs AND other lengths on the same workspace."""
    ws, nbytes = _workspace(lib, c)
    _forward(lib, c, 0, ws, nbytes)
    _forward(lib, c, 1, ws, nbytes)


# ------------------------------------------------------------------ refusals
def _refusal_buffers(B, T, H):
    """operands and NaN-filled outputs of the full size (B, T, H) -- were a refused call launched after all, it would stay inside them."""
    rng = np.random.default_rng(B + T + H)
    Tp, nbytes = AM.padded(T), AM.workspace_bytes(B, T, H)
    return dict(enc=dev(rng.standard_normal((B, T, H))), q=dev(rng.standard_normal((B, H))), g=dev(rng.standard_normal((B, H))),
                ru=dev(np.arange(B), torch.int32), rl=dev(np.full(B, T), torch.int32),
                alpha=_nan(B, Tp), cv=_nan(B, H), ds=_nan(B, Tp), dq=_nan(B, H), ws=GuardedWS(nbytes), nbytes=nbytes)


def _refused(lib, t, rc, what, says):
    torch.cuda.synchronize()
    assert rc != 0, f"{what}: accepted"
    assert says in lib.astk_last_error().decode(), (what, lib.astk_last_error().decode())
    for k in ("alpha", "cv", "ds", "dq"):
        assert _all_nan(t[k]), f"{what}: {k} was written"
    assert bool((t["ws"].big == 0x5A).all()), f"{what}: the workspace was written"


def _calls(lib, B, T, H, t, nbytes):
    a = (B, T, H, vp(t["enc"]))
    yield "fwd", lambda: lib.astk_attn_step_fwd(*a, vp(t["q"]), vp(t["alpha"]), vp(t["cv"]), vp(t["ws"]), nbytes, stream())
    yield "rows", lambda: lib.astk_attn_step_fwd_rows(*a, vp(t["ru"]), vp(t["rl"]), vp(t["q"]), vp(t["alpha"]), vp(t["cv"]), vp(t["ws"]),
                                                      nbytes, stream())
    yield "bwd", lambda: lib.astk_attn_step_bwd(*a, vp(t["alpha"]), vp(t["cv"]), vp(t["g"]), vp(t["ds"]), vp(t["dq"]), vp(t["ws"]), nbytes,
                                                stream())


@pytest.mark.parametrize("B,T,H", AM.REFUSED_WIDTHS + [(0, 9, 8), (2, 0, 8)])
def test_attention_refuses_bad_dimensions(lib, B, T, H):
    """H = 2052 (above the widest instantiation), H = 6 (no float4 rows), no rows, no positions: refused by all three entry points with
    nothing launched -- the outputs keep their NaNs and the workspace its fill (the counters are not even zeroed)."""
    t = _refusal_buffers(max(B, 2), max(T, 9), H)
    for name, call in _calls(lib, B, T, H, t, t["nbytes"]):
        _refused(lib, t, call(), f"{name} ({B}, {T}, {H})", "attn: need")
    assert lib.astk_attn_workspace_bytes(0, 9, 8) == 0 and lib.astk_attn_workspace_bytes(2, 0, 8) == 0


def test_attention_refuses_a_short_workspace_and_a_null_row_map(lib):
    B, T, H = 5, 201, 260
    t = _refusal_buffers(B, T, H)
    for name, call in _calls(lib, B, T, H, t, t["nbytes"] - 1):
        _refused(lib, t, call(), f"{name}, workspace one byte short", "workspace too small")
    a = (B, T, H, vp(t["enc"]))
    tail = (vp(t["q"]), vp(t["alpha"]), vp(t["cv"]), vp(t["ws"]), t["nbytes"], stream())
    _refused(lib, t, lib.astk_attn_step_fwd_rows(*a, vp(t["ru"]), None, *tail), "null row_len", "null row map")
    _refused(lib, t, lib.astk_attn_step_fwd_rows(*a, None, vp(t["rl"]), *tail), "null row_utt", "null row map")
    # the very same buffers, whole: accepted
    ok(lib, lib.astk_attn_step_fwd_rows(*a, vp(t["ru"]), vp(t["rl"]), *tail))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(t["alpha"][:, :T]).any()) and not bool(torch.isnan(t["cv"]).any())
