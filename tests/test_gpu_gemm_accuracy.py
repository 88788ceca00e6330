"""Every kernel and operand form of ast_amd/csrc/gemm.hip against tests/gemm_accuracy_model.py, on the GPU.

Per case of the table: the launcher's plan is asserted before anything is launched (tile, scheme, fix-up, two-level, unit, zeroing, grid),
then three gates: (a) selection identities, bit for bit, in both roles, store and atomic mode on every case (accumulate where the case
names it, into zeros), every k of [0, K) selected in some pass; (b) every entry's error against float64 within TOL[scheme][K] of its own
sqrt(sum a^2 b^2); (c) the projection coefficient on every lost-term direction within C_GATE.  Every launch goes into a NaN-poisoned
buffer with a guard band behind it: the padding, the columns behind N, the gaps between two-level rows and the band stay untouched.
Dense-row cases run through astk_gemm_f32_ex of the product library; cases with views and the single-term fp16 cases through
astk_debug_gemm_views of the instrumented build.  tests/test_gemm_accuracy_host.py shows on the CPU what these gates catch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gemm_accuracy_model as G
from test_gpu_ops import ok, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


@pytest.fixture
def tl(lib):
    from ast_amd import _lib
    with _lib.load_test_hooks() as t:
        yield t


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


class Launcher:
    """One case on the device: asserts the plan, launches, returns the valid region and checks everything around it."""

    def __init__(self, lib, tl, c):
        self.lib, self.tl, self.c = lib, tl, c
        self.scheme = G.kernel_of(c)[0]
        self.view = G.is_view(c)
        # (the fp16x2 scheme takes the maximum of a view over its whole span, gaps included: they hold 0.5 there -- finite, below every
        #  operand's maximum, so the scale is the operand's own, and a gap value that reached a sum would still break gate (a))
        self.fill = 0.5 if (self.scheme == "fp16x2" and self.view) else np.nan
        self.rc = G.Result(c.M, c.N, c.batch, c.c_tn)
        self.index = torch.as_tensor(self.rc.index.ravel()).cuda()
        self.outside = torch.ones(self.rc.size + G.Result.GUARD, dtype=torch.bool, device="cuda")
        self.outside[self.index] = False

    def run(self, A, B, mode, bias=None, c0=None):
        c, rc = self.c, self.rc
        ia, ib = G.operand_images(c, A, B, self.fill)
        a, b = _dev(ia.buf), _dev(ib.buf)
        ra = _dev(ia.rowidx, torch.int32) if ia.rowidx is not None else None
        rb = _dev(ib.rowidx, torch.int32) if ib.rowidx is not None else None
        bv = _dev(bias) if bias is not None else None
        buf = torch.full((rc.size + G.Result.GUARD,), float("nan"), device="cuda")
        if mode != G.STORE:
            buf[self.index] = 0.0 if c0 is None else _dev(c0).ravel()
        p = lambda t: None if t is None else t.data_ptr()
        ptrs = (p(a), p(b), p(buf), p(ra), p(rb), p(bv))
        rcode, text = G.views_call(self.tl, c, mode, ia, ib, rc, ptrs, launch=0)
        ok(self.tl, rcode)
        got, want = G.plan_fields(text), G.expected_plan(c, mode)
        assert {k: got[k] for k in want} == want, (c.name, mode, text)
        if self.view:
            ok(self.tl, G.views_call(self.tl, c, mode, ia, ib, rc, ptrs, launch=1, stream=stream())[0])
        else:
            ok(self.lib, self.lib.astk_gemm_f32_ex(c.layout, c.M, c.N, c.K, C.c_void_p(p(a)), ia.ld, C.c_void_p(p(b)), ib.ld, C.c_void_p(p(buf)), rc.ld,
                                                   None if bv is None else C.c_void_p(p(bv)), mode, 1, c.batch, ia.stride, ib.stride, rc.stride,
                                                   G.PREC_API[self.scheme], stream()))
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[self.outside]).all()), f"{c.name} mode {mode}: wrote outside the result"
        res = buf[self.index].view(c.batch, c.M, c.N)
        assert bool(torch.isfinite(res).all()), f"{c.name} mode {mode}: not finite"
        return res.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _dense(key, name, mode):
    """Operands, reference, scale and the directions of one arithmetic (computed once, shared by the cases that have it)."""
    c = G.by_name(name)
    scheme, TLM, TL, _ = G.kernel_of(c)
    A, B, bias, c0 = G.dense_operands(key)
    c0 = c0 if mode == G.ACCUM else None
    ref, scale = G.reference_case(c, A, B, bias, c0), G.scale_case(A, B, bias, c0)
    dirs = G.directions(scheme, TLM)
    ps = [G.model_case(c, A, B, bias, c0, mutant=m, f32=False) - ref for m in dirs]
    return A, B, bias, c0, ref, scale, dirs, ps


FIRST_OF_KEY = {}
for _c in G.CASES:
    FIRST_OF_KEY.setdefault(G.arithmetic_key(_c), _c.name)


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_gemm_kernel_against_the_float32_model(lib, tl, name):
    c = G.by_name(name)
    key = G.arithmetic_key(c)
    scheme, TLM, TL, _ = G.kernel_of(c)
    with G.Knobs([lib, tl], c):
        L = Launcher(lib, tl, c)
        # (a) selection identities
        launches = 0
        for role in "AB":
            for phase in range(G.phases(key, role)):
                A, B, expect, _ = G.selection(key, role, phase)
                for mode in sorted(set(c.modes) | {G.STORE, G.ATOMIC}):
                    got = L.run(A, B, mode)
                    launches += 1
                    same = got == expect
                    assert same.all(), (f"{name} role {role} pass {phase} mode {mode}: {int((~same).sum())} of {same.size} entries differ from "
                                        f"the selected operand entries, first at {tuple(np.argwhere(~same)[0])}")
        print(f"GEMMACC {name} {scheme} K {c.K} selection: {launches} launches bit-exact")
        # (b), (c) dense operands
        for mode in c.modes:
            A, B, bias, c0, ref, scale, dirs, ps = _dense(key, FIRST_OF_KEY[key], mode)
            got = L.run(A, B, mode, bias, c0).astype(np.float64)
            err = float((np.abs(got - ref) / scale).max())
            cs = [G.coefficient(got, ref, p, scale) for p in ps]
            worst_c = max([abs(x) for x in cs], default=0.0)
            print(f"GEMMACC {name} {scheme} K {c.K} mode {mode}: error {err:.3e} (gate {G.TOL[scheme][c.K]:.2e})  |c| {worst_c:.4f} (gate {G.C_GATE})")
            assert err <= G.TOL[scheme][c.K], f"{name} mode {mode}: {err:.3e} of an entry's own scale, gate {G.TOL[scheme][c.K]:.2e}"
            for m, x in zip(dirs, cs):
                assert abs(x) <= G.C_GATE, f"{name} mode {mode}: c = {x:.3f} on '{G.mutant_name(m, scheme, TLM)}'"
    for which in (lib, tl):
        mask = C.c_uint(0)
        ok(which, which.astk_persist_status(C.byref(mask), 0))
        assert mask.value == 0
