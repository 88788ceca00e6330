"""The encoder recurrences (ast_amd/csrc/lstm_persist.hip) held to float32-level accuracy: every instantiation named by (width, workgroup
form, arithmetic) -- tests/recurrence_accuracy_model.py cases() -- runs astk_lstm_stack_fwd + _bwd on float32-representable inputs and is
compared with the float64 model of that file.  Two gates per case: the error gate (every slice within TOL[kind] of its largest reference
entry; TOL is 4 x the plain float32 evaluation, 100 ... 250 x tighter than close()), and, for the split schemes, the projection gates (the
result must not contain the displacement a lost lowest plane would cause: |c| <= 0.25 on every direction, where a kernel that loses the
plane has c = 1).  tests/test_recurrence_accuracy_host.py shows on the CPU where the tolerances come from and what each gate catches.

Each case asserts that it ran what it names: astk_lstm_stack_path, and the workgroup form and arithmetic from astk_lstm_stack_form."""
import ctypes as C

import numpy as np
import pytest
import torch

import recurrence_accuracy_model as M
from test_gpu_ops import GuardedWS, dev, ok, stream, vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


def _device_call(lib, c):
    """astk_lstm_stack_fwd + _bwd of the case on zeroed gradients -> (every tensor as float64 arrays, named as the model names them; path, rows, xs)."""
    from ast_amd._lib import LstmGrads, LstmParams, LstmStackDesc
    T, B, in_dim, h, nl, masks = M.shape_of(c)
    dr = M.draws(M.shape_of(c))
    d = LstmStackDesc(T, B, in_dim, h, nl, 2)
    d.precision = M.PREC[c.scheme]          # the descriptor's field, not the process default
    rows, xs = C.c_int(-1), C.c_int(-1)
    ok(lib, lib.astk_lstm_stack_form(C.byref(d), C.byref(rows), C.byref(xs)))
    launch = (lib.astk_lstm_stack_path(C.byref(d)), rows.value, xs.value)
    prm = {k: dev(v) for k, v in dr["P"].items()}
    grd = {k: torch.zeros_like(v) for k, v in prm.items()}
    lp, lg = (LstmParams * (2 * nl))(), (LstmGrads * (2 * nl))()
    for i, n in enumerate(dr["names"]):
        lp[i].Wu, lp[i].b, lp[i].Wl = (prm[n + s].data_ptr() for s in ("/upward/W", "/upward/b", "/lateral/W"))
        lg[i].dWu, lg[i].db, lg[i].dWl = (grd[n + s].data_ptr() for s in ("/upward/W", "/upward/b", "/lateral/W"))
    nbytes = lib.astk_lstm_stack_workspace_bytes(C.byref(d))
    assert nbytes > 0, lib.astk_last_error().decode()
    ws = GuardedWS(nbytes)
    xd, md = dev(dr["x"]), (dev(dr["mk"]) if masks else None)
    enc = torch.zeros(B, T, 2 * h, device="cuda")
    cT, hT = torch.zeros(2, nl, B, h, device="cuda"), torch.zeros(2, nl, B, h, device="cuda")
    ok(lib, lib.astk_lstm_stack_fwd(C.byref(d), lp, vp(xd), vp(md), vp(enc), vp(cT), vp(hT), vp(ws), nbytes, stream()))
    ws.check("lstm fwd")
    dx = torch.zeros(T, B, in_dim, device="cuda")
    ge, gc, gh = (dev(dr[k]) for k in ("g_enc", "g_c", "g_h"))
    ok(lib, lib.astk_lstm_stack_bwd(C.byref(d), lp, lg, vp(xd), vp(md), vp(ge), vp(gc), vp(gh), vp(dx), vp(ws), nbytes, stream()))
    ws.check("lstm bwd")
    status = C.c_uint(0)
    ok(lib, lib.astk_persist_status(C.byref(status), 1))
    assert status.value == 0, f"sticky status word {status.value:#x}"
    out = {"enc_states": enc, "cT": cT, "hT": hT, "dx": dx}
    out.update({"grad " + k: v for k, v in grd.items()})
    return {k: v.double().cpu().numpy() for k, v in out.items()}, launch


@pytest.mark.parametrize("case", M.cases(), ids=M.case_id)
def test_recurrence_meets_the_float32_gates(lib, tune, case):
    """One instantiation: it ran what the case names; every slice within TOL[kind] (4 x TOL under fp16x2); |c| <= 0.25 on every direction of
    the case's scheme.  The worst figure per kind and the largest |c| are printed before anything is asserted."""
    tune("lstm.rows32", M.ROWS32_KNOB[case.form], lib)
    shape = M.shape_of(case)
    got, launch = _device_call(lib, case)
    assert launch == M.expected_launch(case), f"(path, rows, xs) = {launch}, the case names {M.expected_launch(case)}"
    for k, v in got.items():
        assert np.isfinite(v).all(), f"{k}: not finite"
    errs = M.slice_errors(got, shape)
    worst = M.worst_by_kind(errs)
    cs = M.coefficients(got, shape, case.scheme)
    cmax = max(cs, key=lambda nc: abs(nc[1])) if cs else ("none", 0.0)
    print(f"{M.case_id(case)}: " + "  ".join(f"{k} {worst[k]:.2e} (tol {M.tolerance(case, k):.0e})" for k in M.KINDS)
          + f"  largest |c| {abs(cmax[1]):.3f} ({cmax[0]})")
    bad = [f"{name}: {e:.2e} > {M.tolerance(case, kind):.0e}" for name, kind, e in errs if not e <= M.tolerance(case, kind)]
    assert not bad, "error gate: " + "; ".join(bad)
    bad = [f"{name}: c = {c:+.3f}" for name, c in cs if not abs(c) <= M.C_GATE]
    assert not bad, f"projection gate (|c| <= {M.C_GATE}): " + "; ".join(bad)
