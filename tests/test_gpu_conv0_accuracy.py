"""The direct layer-0 convolution k_conv0_fwd_x3 of ast_amd/csrc/conv.hip against tests/conv0_accuracy_model.py,
on the GPU, through the product library alone.

Y itself: a one-layer stack with no_bn = 1 and a zero bias is out = relu(Y), run with W and with -W; Y_hat = out(W) - out(-W).
 (a) selection identities, bit for bit: forward (every output is 2^e times the selected noisy input element, over kt * kf passes) and
     window (XF read back through CNN_0/W's gradient: 2^e times the selected position's patch, every output position in some pass);
 (b) every entry's error against float64 within TOL[kt] of its own sqrt(sum x^2 w^2);  (c) |c| <= C_GATE on every lost-term direction;
 (d) with BatchNorm and bn_decay = 0: the fused statistics against the float64 statistics of the reference Y on a benign and an offset
     draw, and on the benign draw the output, dW, dgamma, dbeta at float32-level tolerances.
Every case proves that it ran the direct kernel (the backward call with "conv.direct0" off is refused on the forward's workspace), keeps a
guarded workspace, finds its input intact and the sticky status word at zero, and sets the scheme through the descriptor's `precision`.
tests/test_conv0_accuracy_host.py shows on the CPU where every number comes from and what each gate catches."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv0_accuracy_model as M
from test_gpu_ops import GuardedWS, _cnn_desc, dev, ok, stream, vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


class Stack:
    """One case as a one-layer stack on the device: parameters, gradients, a guarded workspace."""

    def __init__(self, lib, c, no_bn, X, noise):
        from ast_amd._lib import CnnLayerGrads, CnnLayerParams
        self.lib, self.c = lib, c
        self.cd = _cnn_desc(M.cfg_of(c, True), c.B, c.T, c.D)
        self.cd.no_bn, self.cd.precision, self.cd.bn_decay = int(no_bn), M.PREC_BF16X3, 0.0
        t2, f2, feat = C.c_int(), C.c_int(), C.c_int()
        ok(lib, lib.astk_conv_bn_relu_out_dims(C.byref(self.cd), C.byref(t2), C.byref(f2), C.byref(feat)))
        F, T1, _, _ = M.dims(c)
        assert (t2.value, f2.value, feat.value) == (T1, F, c.C * F)
        z = lambda n, v=0.0: torch.full((n,), v, device="cuda")
        self.prm = dict(W=z(c.C * c.kt * c.kf), gamma=z(c.C, 1.0), beta=z(c.C), avg_mean=z(c.C), avg_var=z(c.C, 1.0), bias=z(c.C))
        self.grd = dict(dW=z(c.C * c.kt * c.kf), dgamma=z(c.C), dbeta=z(c.C), dbias=z(c.C))
        self.cp, self.cg = (CnnLayerParams * 1)(), (CnnLayerGrads * 1)()
        for k, v in self.prm.items():
            setattr(self.cp[0], k, v.data_ptr())
        for k, v in self.grd.items():
            setattr(self.cg[0], k, v.data_ptr())
        self.nbytes = lib.astk_conv_bn_relu_workspace_bytes(C.byref(self.cd))
        self.ws = GuardedWS(self.nbytes)
        self.out = torch.empty(T1, c.B, c.C * F, device="cuda")
        self.X, self.noise = X, noise
        self.xd, self.nd = dev(X), (dev(noise) if noise is not None else None)
        self.probed = False

    def set(self, **kw):
        for k, v in kw.items():
            self.prm[k].copy_(dev(np.asarray(v, np.float32).ravel()))

    def fwd(self):
        ok(self.lib, self.lib.astk_conv_bn_relu_fwd(C.byref(self.cd), self.cp, vp(self.xd), vp(self.nd), vp(self.out), vp(self.ws), self.nbytes, 1, stream()))
        if not self.probed:
            self.probe()
        return self.out

    def probe(self):
        """The path probe of test_gpu_ops._cnn_case: with "conv.direct0" off, a backward call on this forward's workspace is refused in
        front of every launch if and only if the forward took the direct kernel."""
        lib = self.lib
        prev = C.c_double()
        assert lib.astk_get_tuning(b"conv.direct0", C.byref(prev)) == 0 and prev.value == 1
        assert lib.astk_set_tuning(b"conv.direct0", 0.0) == 0
        g = torch.zeros_like(self.out)
        try:
            rc = lib.astk_conv_bn_relu_bwd(C.byref(self.cd), self.cp, self.cg, vp(g), vp(self.ws), self.nbytes, stream())
        finally:
            assert lib.astk_set_tuning(b"conv.direct0", prev.value) == 0
        assert rc != 0, f"{self.c.name}: layer 0 ran on the im2col path"
        assert M.DIRECT_MSG in lib.astk_last_error().decode(), lib.astk_last_error().decode()
        assert all(float(v.abs().max()) == 0.0 for v in self.grd.values()), "a refused backward call wrote gradients"
        self.probed = True

    def y_hat(self, W):
        """out(W) - out(-W) as rows (B F' T', C), on the device."""
        c = self.c
        F, T1, _, _ = M.dims(c)
        self.set(W=W)
        plus = self.fwd().clone()
        self.set(W=-np.asarray(W, np.float32))
        y = plus - self.fwd()
        return y.view(T1, c.B, c.C, F).permute(1, 3, 0, 2).reshape(-1, c.C)

    def bwd(self, gout):
        for v in self.grd.values():
            v.zero_()
        g = dev(gout)
        ok(self.lib, self.lib.astk_conv_bn_relu_bwd(C.byref(self.cd), self.cp, self.cg, vp(g), vp(self.ws), self.nbytes, stream()))

    def done(self):
        self.ws.check(self.c.name)
        assert self.probed
        assert torch.equal(self.xd, dev(self.X)), "input clobbered"
        assert self.nd is None or torch.equal(self.nd, dev(self.noise)), "noise clobbered"
        mask = C.c_uint(0)
        ok(self.lib, self.lib.astk_persist_status(C.byref(mask), 0))
        assert mask.value == 0


def _rows_equal(got, expect, what):
    if not torch.equal(got, expect):
        bad = (got != expect).nonzero()
        r, ch = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {expect.numel()} entries differ, first at row {r} channel {ch}: "
                             f"{float(got[r, ch])!r} for {float(expect[r, ch])!r}")


# ------------------------------------------------------------------ gate (a)
@pytest.mark.parametrize("name", M.FWD_SELECTION_ROWS)
def test_forward_selection_identities_bit_for_bit(lib, name):
    c = M.by_name(name)
    X, noise, xn, _ = M.heavy_input(name, "fwd")
    s = Stack(lib, c, True, X, noise)
    if name == "tile-loop":
        assert M.dims(c)[3] > 2 * lib.astk_device_cu_count(), "the tile-loop row must give a workgroup more than one tile: raise B"
    for p in range(c.kt * c.kf):
        W, expect = M.selection_fwd(name, p)
        _rows_equal(s.y_hat(W), dev(expect), f"{name} pass {p}")
    s.done()
    print(f"CONV0ACC {name} forward selection: {2 * c.kt * c.kf} launches bit-exact")


@pytest.mark.parametrize("name", M.XF_SELECTION_ROWS)
def test_window_selection_identities_bit_for_bit(lib, name):
    c = M.by_name(name)
    X, noise, xn, _ = M.heavy_input(name, "xf")
    W, bias, Y = M.xf_setup(name)
    s = Stack(lib, c, True, X, noise)
    if name == "tile-loop":
        assert M.dims(c)[3] > 2 * lib.astk_device_cu_count()
    s.set(W=W, bias=bias)
    out = s.fwd()
    assert float(out.min()) > 0.0, "every unit must be active"
    for p in range(M.xf_passes(c)):
        gout, dW, val, rows = M.selection_xf(name, p)
        s.bwd(gout)
        _rows_equal(s.grd["dW"].view(c.C, -1), dev(dW.reshape(c.C, -1)), f"{name} pass {p}: CNN_0/W gradient")
        assert torch.equal(s.grd["dbias"], dev(val)), f"{name} pass {p}: dbias"
    s.done()
    print(f"CONV0ACC {name} window selection: {M.xf_passes(c)} backward calls bit-exact")


# ------------------------------------------------------------------ gates (b), (c)
@pytest.mark.parametrize("name", [c.name for c in M.CASES])
def test_error_and_projection_gates(lib, name):
    c = M.by_name(name)
    W, X, noise = M.dense(name)
    Wk, Pk, ref, scale = M.dense_parts(name)
    s = Stack(lib, c, True, X, noise)
    got = s.y_hat(W).cpu().numpy().astype(np.float64)
    s.done()
    err = float((np.abs(got - ref) / scale).max())
    dirs = M.directions(c)
    cs = [M.coefficient(got, ref, M.model(c, Wk, Pk, mutant=m, f32=False) - ref, scale) for m in dirs]
    worst = max(range(len(dirs)), key=lambda i: abs(cs[i]))
    print(f"CONV0ACC {name} kt {c.kt}: error {err:.3e} (gate {M.TOL[c.kt]:.2e})  largest |c| {abs(cs[worst]):.4f} on '{M.mutant_name(dirs[worst])}' "
          f"(gate {M.C_GATE}, {len(dirs)} directions)")
    assert err <= M.TOL[c.kt], f"{name}: {err:.3e} of an entry's own scale, gate {M.TOL[c.kt]:.2e}"
    for m, x in zip(dirs, cs):
        assert abs(x) <= M.C_GATE, f"{name}: c = {x:.3f} on '{M.mutant_name(m)}'"


# ------------------------------------------------------------------ gate (d)
@pytest.mark.parametrize("offset", [False, True], ids=["benign", "offset"])
@pytest.mark.parametrize("name", M.STAT_ROWS)
def test_fused_statistics_and_the_batchnorm_path(lib, name, offset):
    c = M.by_name(name)
    cfg, P, X, noise, _ = M.bn_draws(name, offset)
    W = P["CNN_0/W"].reshape(c.C, c.kt, c.kf)
    s = Stack(lib, c, False, X, noise)
    if name == "tile-loop":
        assert M.dims(c)[3] > 2 * lib.astk_device_cu_count()
    s.set(W=W, gamma=P["CNN_0_bn/gamma"], beta=P["CNN_0_bn/beta"])
    out = s.fwd().cpu().numpy()
    Y64 = M.reference(c, W, M.noisy(X, noise))
    rm, rv, m = M.stats_reference(Y64)
    em, ev = M.stat_errors(s.prm["avg_mean"].cpu().numpy().astype(np.float64), s.prm["avg_var"].cpu().numpy().astype(np.float64), rm, rv)
    tol = M.STAT_TOL[name]
    kind = "offset" if offset else "benign"
    print(f"CONV0ACC {name} {kind}: mean {em:.3e} of a standard deviation (gate {tol['mean']:.2e})  variance {ev:.3e} relative (gate {tol['var']:.2e})")
    e = {}
    if not offset:
        ref_out, gout, dW, dgamma, dbeta = M.bn_reference(c, cfg, P, X, noise)
        s.bwd(gout)
        g = {k: v.cpu().numpy().astype(np.float64) for k, v in s.grd.items()}
        e = {"out": M.tensor_error(out, ref_out), "dW": M.tensor_error(g["dW"].reshape(dW.shape), dW),
             "dparam": max(M.tensor_error(g["dgamma"], dgamma), M.tensor_error(g["dbeta"], dbeta))}
        print(f"CONV0ACC {name} benign: " + "  ".join(f"{k} {v:.3e} (gate {M.BN_TOL[name][k]:.2e})" for k, v in e.items()))
    s.done()
    assert em <= tol["mean"], f"{name} {kind}: batch mean {em:.3e} of a standard deviation off, gate {tol['mean']:.2e}"
    assert ev <= tol["var"], f"{name} {kind}: batch variance {ev:.3e} off, gate {tol['var']:.2e}"
    for k, v in e.items():
        assert v <= M.BN_TOL[name][k], f"{name}: {k} {v:.3e} of the largest entry, gate {M.BN_TOL[name][k]:.2e}"
