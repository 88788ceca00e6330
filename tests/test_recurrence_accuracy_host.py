"""CPU side of the recurrences' float32-level gates (tests/recurrence_accuracy_model.py; the kernels: tests/test_gpu_recurrence_accuracy.py).
Shows that the local float64 model is the oracle's encoder, where the tolerances come from, that the float32 evaluation stays far from
every projection direction while a model that loses the plane sits on it, and what the error gate alone catches."""
import numpy as np
import pytest
import torch

import recurrence_accuracy_model as M

SHAPES = M.shapes()
BF16X3_SHAPES = [s for s in SHAPES if any(M.shape_of(c) == s and c.scheme == "bf16x3" for c in M.cases())]
_id = lambda s: "T{}-B{}-in{}-h{}-L{}{}".format(*s[:5], "-masks" if s[5] else "")


@pytest.fixture(scope="module")
def f32_eval():
    """The plain float32 evaluation of every shape (computed once, left unchanged)."""
    return {s: M.run(s, torch.float32) for s in SHAPES}


def test_case_table_names_every_instantiation():
    cs = M.cases()
    assert len(cs) == 28
    named = {(c.h, c.form, M.expected_launch(c)[2]) for c in cs}
    want = {(h, M.ROWS_16, xs) for h in (64, 128, 256) for xs in (M.XS_F32, M.XS_FP16X2, M.XS_BF16X3)}
    want |= {(h, M.ROWS_16, xs) for h in (512, 1024) for xs in (M.XS_F32, M.XS_FP16X2, M.XS_BF16X3_LDS)}
    want |= {(h, M.ROWS_MT2, xs) for h in (64, 128, 256) for xs in (M.XS_F32, M.XS_FP16X2, M.XS_BF16X3)}
    want |= {(h, M.ROWS_DUO, M.XS_BF16X3_LDS) for h in (64, 128, 256)}
    assert named == want and len(want) == 27
    assert any(c.T == 2 for c in cs) and {c.h for c in cs if c.masks and c.form == M.ROWS_16} == {128, 512}
    for s in SHAPES:                                 # the inputs are float32 numbers, and a mask has both of its values
        d = M.draws(s)
        assert all(v.dtype == np.float32 for v in d["P"].values()) and d["x"].dtype == np.float32 and d["g_enc"].dtype == np.float32
        if s[5]:
            assert d["mk"].min() == 0 and d["mk"].max() > 1


@pytest.mark.parametrize("shape", [(5, 17, 16, 64, 2, False), (5, 5, 16, 512, 2, True)], ids=_id)
def test_local_model_is_the_oracles_encoder(shape):
    """run() in float64 against oracle.ast_ref_torch.encoder_torch on the same float32-representable inputs: every output and gradient
    within 1e-12 of the tensor's largest entry."""
    from oracle.ast_ref_torch import encoder_torch
    T, B, in_dim, h, nl, masks = shape
    d = M.draws(shape)
    P = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in d["P"].items()}
    x = torch.tensor(d["x"], dtype=torch.float64, requires_grad=True)
    mk = torch.tensor(d["mk"], dtype=torch.float64) if masks else None
    enc, cT, hT = encoder_torch({"rnn_config": {"enc_layers": nl}}, P, x, mk)
    up = [torch.tensor(d[k], dtype=torch.float64) for k in ("g_enc", "g_c", "g_h")]
    ((enc * up[0]).sum() + (cT * up[1]).sum() + (hT * up[2]).sum()).backward()
    want = {"enc_states": enc, "cT": cT, "hT": hT, "dx": x.grad}
    want.update({"grad " + k: v.grad for k, v in P.items()})
    got = M.reference(shape)
    assert set(got) == set(want)
    for k, v in want.items():
        v = v.detach().numpy()
        assert np.abs(got[k] - v).max() <= 1e-12 * np.abs(v).max(), k
    # ... and a spec of untouched passes is the same model (the product hook itself changes nothing)
    hooked = M.run(shape, spec={"lateral": (M.Pass(), M.Pass()), "upward": (M.Pass(), M.Pass())})
    for k, v in got.items():
        assert np.abs(hooked[k] - v).max() <= 1e-12 * np.abs(v).max(), k


def test_float32_model_error_is_what_the_tolerances_were_taken_from(f32_eval):
    """The plain float32 evaluation stays within TOL / 4 on every slice of every case; the recorded figures still describe the cases (between
    half of them and 1.25 times them, as tests/test_ctc_host.py holds its own: float32 sums differ in the last bits between builds); and
    TOL is the smallest {1, 2, 5} x 10^k at four times the figure."""
    worst = {k: 0.0 for k in M.KINDS}
    for s in SHAPES:
        errs = M.slice_errors(f32_eval[s], s)
        w = M.worst_by_kind(errs)
        print(_id(s), "  ".join(f"{k} {w[k]:.2e}" for k in M.KINDS))
        for name, kind, e in errs:
            assert e <= M.TOL[kind] / 4, (s, name, e)
        worst = {k: max(worst[k], w[k]) for k in M.KINDS}
    print("worst", worst)
    for k in M.KINDS:
        assert 0.5 * M.F32_MODEL_ERR[k] <= worst[k] <= 1.25 * M.F32_MODEL_ERR[k], (k, worst[k])
        assert M.TOL[k] == pytest.approx(M.smallest_125(4 * M.F32_MODEL_ERR[k]), rel=1e-9), k
    assert M.FP16X2_FACTOR == 2.0 ** -22 / 2.0 ** -24


@pytest.mark.parametrize("scheme", ["bf16x3", "fp16x2"])
def test_float32_model_is_far_from_every_direction(f32_eval, scheme):
    """|c| <= C_F32_MAX = 0.1 for the float32 evaluation on every direction of every shape: rounding noise is not aligned with the
    displacement of a lost plane, so the device gate of 0.25 leaves a margin of 2.5 over what float32 arithmetic itself shows."""
    assert len(M.directions("bf16x3")) == 20 and len(M.directions("fp16x2")) == 8 and M.directions("f32") == []
    assert len(M.directions("bf16x3", hoisted=True)) == 10 and len(M.directions("fp16x2", hoisted=True)) == 4
    top = 0.0
    for s in SHAPES:
        cs = M.coefficients(f32_eval[s], s, scheme)
        name, c = max(cs, key=lambda nc: abs(nc[1]))
        print(f"{_id(s)} {scheme}: largest |c| {abs(c):.4f} ({name})")
        assert abs(c) <= M.C_F32_MAX, (s, name, c)
        top = max(top, abs(c))
    print("largest", top)


@pytest.mark.parametrize("scheme", ["bf16x3", "fp16x2"])
def test_a_model_that_loses_the_plane_sits_on_its_direction(scheme):
    """The float64 model with a mutant has c = 1 on the mutant's direction by construction (asserted as >= 0.9 for the record).  What a
    kernel with that fault would show is the mutant evaluated in FLOAT32: the displacement, plus float32's own noise (at most C_F32_MAX
    along the direction, shown above), and with an activation's lowest plane taken from the float32 pass's activations instead of the
    reference's (they differ in their last bits, which is where that plane lives).  So it must reach 1 - 2 C_F32_MAX = 0.8: the gate of
    0.25 fires with a margin of three.  Measured: >= 0.90.  The directions of one side are orthogonal -- the cosine of every pair is
    <= 0.25 (measured: <= 0.1) -- so a mutant's coefficient on ANOTHER direction is that cosine times the ratio of the two displacements'
    lengths (measured: up to 0.43 where a tanh gate's direction is projected on a shorter one); the largest is printed."""
    low, cos_top, cross_top = 1.0, 0.0, 0.0
    for s in SHAPES:
        dv = M.direction_vectors(s, scheme)
        for d, p in dv:
            c64 = dict(M.coefficients(M.run(s, spec=d.spec), s, scheme))[d.name] if s == SHAPES[0] else 1.0
            assert c64 >= 0.9 and abs(c64 - 1.0) < 1e-9, (s, d.name, c64)
            got = M.run(s, torch.float32, spec=d.spec)
            c = dict(M.coefficients(got, s, scheme))[d.name]
            assert c >= 1.0 - 2 * M.C_F32_MAX, (s, d.name, c)
            low = min(low, c)
            for e, q in dv:
                if e.side == d.side and e.name != d.name:
                    pq, pp, qq = (float(np.dot(u, v)) for u, v in ((p, q), (p, p), (q, q)))
                    cos = abs(pq) / np.sqrt(pp * qq)
                    assert cos <= 0.25, (s, d.name, e.name, cos)
                    cos_top, cross_top = max(cos_top, cos), max(cross_top, abs(pq) / qq)
    print(f"{scheme}: smallest own c {low:.3f}, largest cosine {cos_top:.3f}, largest coefficient of a mutant on another direction {cross_top:.3f}")


@pytest.mark.parametrize("shape", BF16X3_SHAPES, ids=_id)
def test_what_the_error_gate_catches_alone(shape):
    """Mutation power of the error gate on the forward lateral product.  A lost MID plane and one missing term product of the six
    (activation mid x weight hi) exceed TOL["state"] on EVERY state slice, by a factor of hundreds.  The lowest plane does not: lost, or
    garbage (rolled by one row: every row gets another gate's lo fragment), or its term product lo x hi missing, it moves the state
    slices by 0.2 ... 1.9 x TOL -- above on some shapes, below on others -- which is why those need the projection gate: each of them has
    |c| > C_GATE on a lateral lo direction.  The ratios are printed."""
    for name, (spec, exceeds) in M.error_gate_mutants().items():
        got = M.run(shape, spec=spec)
        errs = M.slice_errors(got, shape)
        state = [e / M.TOL["state"] for _, kind, e in errs if kind == "state"]
        w = M.worst_by_kind(errs)
        print(f"{name}: state slices {min(state):.2f} ... {max(state):.2f} x TOL; worst per kind "
              + "  ".join(f"{k} {w[k] / M.TOL[k]:.2f}" for k in M.KINDS))
        if exceeds:
            assert min(state) > 1.0, (name, min(state))
        else:
            cs = [(n, c) for n, c in M.coefficients(got, shape, "bf16x3") if n.startswith("fwd lateral")]
            n, c = max(cs, key=lambda nc: abs(nc[1]))
            print(f"    projection: c = {c:+.2f} on '{n}'")
            assert abs(c) >= 0.9, (name, cs)
