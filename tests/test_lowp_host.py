"""The model of the fp16-operand mode (tests/lowp_model.py) on the CPU: known answers of the rounding, the autograd node against a
hand-written product, and -- for every case of tests/test_gpu_lowp.py -- that the case can tell the arithmetics apart (sharpness) and
that the GPU test's assertion helpers reject the wrong arithmetic (negative controls).  Prints gap and n32 per case and tensor (-s).

gap = max |ref16 - ref32|; n32 = max |ref16 evaluated in float32 - ref16|.  Kernel cases: gap >= 4 x 2e-5 x max |ref16|.  Op cases:
gap >= 8 n32 for every directly affected tensor -- the GPU test holds those to gap / 4, and a result in the right arithmetic sits where
the float32 evaluation does.  What n32 measures at op level is not summation noise: an operand the op computed (dz, dlogits, h) differs
between two float32 evaluations in its last bits, and an entry that lies within that of a rounding boundary lands on the other fp16
neighbour -- one fp16 ulp of that entry, against a gap of about 0.3 sqrt(rows) such ulps.  The draws' seeds are chosen here for this
condition; with the decoder's S x B of about a hundred rows it is met by little."""
import numpy as np
import pytest
import torch

import lowp_model as M


# ------------------------------------------------------------------ round_operand
def test_round_operand_known_answers():
    r = M.round_operand
    # ties to even on the 11-bit grid: 2049 -> 2048, 2051 -> 2052, 2050 stays
    assert list(r([2049.0, 2050.0, 2051.0, 2053.0])) == [2048.0, 2050.0, 2052.0, 2052.0]
    assert list(r([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20])) == [1.0, 1 + 2.0 ** -9, 1 + 2.0 ** -10]
    # plain cast: the subnormal floor (grid 2^-24 below 2^-14, ties to even, zero below 2^-25), overflow above 65504 + half a step
    assert list(r([2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 3e-8, 2.9e-8, 5e-5])) == [2.0 ** -24, 0.0, 2.0 ** -23, 2.0 ** -24, 0.0, 839 * 2.0 ** -24]
    assert r(65519.0) == 65504.0 and np.isinf(r(65520.0)) and r(-70000.0) == -np.inf
    # the binade edges of the maximum: 2^14 and just below 2^15 give scale 1, 2^15 gives 1/2, just below 2^14 gives 2
    assert M.scale_of(2.0 ** 14) == 1.0 and M.scale_of(np.nextafter(np.float32(2.0 ** 15), np.float32(0))) == 1.0
    assert M.scale_of(2.0 ** 15) == 0.5 and M.scale_of(np.nextafter(np.float32(2.0 ** 14), np.float32(0))) == 2.0
    assert M.scale_of(1.0) == 2.0 ** 14 and M.scale_of(3e-9) == 2.0 ** 43 and M.scale_of(0.0) == 1.0 and M.scale_of(1e-40) == 1.0
    # behind the scale the floor moves with the maximum: 2^-24 of 2^15 x the binade's lower edge
    x = np.array([3e-9, 3e-9 * 2.0 ** -30, 3e-9 * 2.0 ** -41, 1e-12])
    got = r(x, 3e-9)
    s = 2.0 ** 43
    assert got[0] == float(np.float16(np.float64(np.float32(3e-9)) * s)) / s and abs(got[0] / 3e-9 - 1) < 2.0 ** -11
    assert abs(got[1] / x[1] - 1) < 2.0 ** -2 and got[2] == 0.0 and abs(got[3] / 1e-12 - 1) < 2.0 ** -11
    assert (r(x) == 0.0).all()                       # ... where the plain cast has nothing left
    # idempotent, odd, and the maximum itself never overflows
    rng = np.random.default_rng(0)
    v = rng.standard_normal(4096) * 10.0 ** rng.uniform(-12, 3, 4096)
    for amax in (None, float(np.abs(v).max())):
        once = r(v, amax)
        assert (r(once, amax) == once).all() and (r(-v, amax) == -once).all()
    assert np.isfinite(r(v, float(np.abs(v).max()))).all()
    big = np.nextafter(np.float32(2.0 ** 15), np.float32(0))
    assert r(big, big) == 2.0 ** 15       # (rounds up to 2^15 < 65504: finite)


def test_lowp_product_against_a_hand_written_product():
    rng = np.random.default_rng(1)
    x, w, g = rng.standard_normal((3, 5, 7)) * 1e-3, rng.standard_normal((4, 7)) * 30, rng.standard_normal((3, 5, 4)) * 1e-7
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    x, w, g = f32(x), f32(w), f32(g)
    def rnd(a, measured):
        s = 2.0 ** (14 - np.floor(np.log2(np.abs(a).max()))) if measured else 1.0
        return (a * s).astype(np.float16).astype(np.float64) / s
    for spec in (M.LowpSpec(), M.LowpSpec(mg=False), M.LowpSpec(fwd=False, dgrad=False), M.LowpSpec(wgrad=False, mx=False), M.LowpSpec().plain()):
        xt, wt = torch.tensor(x, requires_grad=True), torch.tensor(w, requires_grad=True)
        y = M.LowpProduct.apply(xt, wt, spec)
        (y * torch.tensor(g)).sum().backward()
        rx, rw, rg = rnd(x, spec.mx), rnd(w, spec.mw), rnd(g, spec.mg)
        want_y = np.einsum("tbk,nk->tbn", rx, rw) if spec.fwd else np.einsum("tbk,nk->tbn", x, w)
        want_dx = np.einsum("tbn,nk->tbk", rg, rw) if spec.dgrad else np.einsum("tbn,nk->tbk", g, w)
        want_dw = np.einsum("tbn,tbk->nk", rg, rx) if spec.wgrad else np.einsum("tbn,tbk->nk", g, x)
        for got, want in ((y.detach().numpy(), want_y), (xt.grad.numpy(), want_dx), (wt.grad.numpy(), want_dw)):
            assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    # the plain cast of a 1e-7 gradient is not the scaled rounding: the two specs must differ
    assert np.abs(rnd(g, True) - rnd(g, False)).max() > 0.1 * np.abs(g).max() * 2.0 ** -11


# ------------------------------------------------------------------ kernel level
def _gemm_rows():
    rows = [(name, i, shape, batch, 1.0, 1.0, 0) for name, group, batch, _ in M.GEMM_CASES for i, shape in enumerate(group)]
    rows += [(f"mag-{sa:g}-{sb:g}", 0, M.MAG_SHAPE, 1, sa, sb, 5) for sa, sb in M.MAGNITUDES]
    return rows


@pytest.mark.parametrize("name,i,shape,batch,sa,sb,decades", _gemm_rows(), ids=lambda v: v if isinstance(v, str) else None)
def test_gemm_cases_tell_the_arithmetics_apart(name, i, shape, batch, sa, sb, decades):
    A, B = M.gemm_operands(f"{name}/{i}", *shape, batch, sa, sb, decades)
    r = M.gemm_refs(A, B, 3)
    gap, top = M.maxdiff(r["ref16"], r["ref32"]), np.abs(r["ref16"]).max()
    n32 = M.maxdiff(M.gemm_f32_eval(A, B, 3), r["ref16"]) if shape[2] <= 1024 else float("nan")
    print(f"{name}/{i} {shape} x{batch}: gap {gap:.3e} = {gap / top:.2e} of the largest entry, n32 {n32 / top:.1e} of it")
    assert gap >= 4 * M.F32_GATE * top
    # negative control: the row gate rejects ref32 in place of the device's result
    with pytest.raises(AssertionError):
        M.assert_rows(r["ref32"], r["ref16"], name)
    M.assert_rows(M.gemm_f32_eval(A, B, 3) if shape[2] <= 1024 else r["ref16"], r["ref16"], name)
    if sa < 1e-3:       # a gradient-sized operand: the plain cast in place of the scaled rounding is rejected too
        with pytest.raises(AssertionError):
            M.assert_rows(r["plain"], r["ref16"], name)


# ------------------------------------------------------------------ op level
def _report(case):
    for k in case["affected"]:
        plain = M.maxdiff(case["plain"][k], case["ref16"][k])
        print(f"{case['name']:46s} {k:30s} gap {case['gap'][k]:.3e}  n32 {case['n32'][k]:.3e}  gap/n32 {case['gap'][k] / max(case['n32'][k], 1e-300):7.1f}"
              f"  plain-cast model {plain:.3e}")


def _sharp(case):
    _report(case)
    for k in case["affected"]:
        assert case["gap"][k] >= 8 * case["n32"][k], (case["name"], k, case["gap"][k], case["n32"][k])


def _controls(case):
    M.assert_op(case["ref16_f32"], case)                  # the float32 evaluation of the model passes ...
    with pytest.raises(AssertionError):                     # ... ref32 as if it were the device's result does not
        M.assert_op(case["ref32"], case)
    if case["small_gradient_operand"]:                      # ... nor the plain cast of a gradient operand below fp16's normal range
        with pytest.raises(AssertionError):
            M.assert_op(case["plain"], case)


@pytest.mark.parametrize("row", M.ENC_CASES, ids=lambda r: "-".join(str(v) for v in r))
def test_encoder_cases(row):
    case = M.enc_case_of(row)
    _sharp(case)
    _controls(case)


@pytest.mark.parametrize("row", M.DEC_CASES, ids=lambda r: "-".join(str(v) for v in r))
def test_decoder_cases(row):
    case = M.dec_case_of(row)
    _sharp(case)
    _controls(case)
    for k in case["ref32"]:                                 # what is not directly affected is the exact model's
        if k not in case["affected"]:
            assert case["ref16"][k] is case["ref32"][k]


@pytest.mark.parametrize("row", M.CNN_CASES, ids=lambda r: "-".join(str(v) for v in r))
def test_cnn_cases(row):
    """Also: the seed is kink-free on the ROUNDED reference (no unit of any layer within 2e-5 of the ReLU's kink, tests/test_gpu_ops.py
    _cnn_case(kink_free=True)'s condition), so that no gradient falls under the near-kink allowance."""
    case = M.cnn_case_of(row)
    print(f"{case['name']}: nearest unit to the kink per layer {case['kink']}")
    assert min(case["kink"]) >= 2e-5
    _sharp(case)
    _controls(case)
