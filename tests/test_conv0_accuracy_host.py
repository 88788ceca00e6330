"""What tests/test_gpu_conv0_accuracy.py relies on, shown on the CPU (tests/conv0_accuracy_model.py): the case
table reaches what it says; the references agree with the float64 oracle; the selection identities are exact in the kernel's order of
terms on every drawn value; every tolerance is 4 x a float32 model's worst figure, re-measured here; the error gate rejects a lost mid
plane, a missing mid x hi term and a shifted k order on every case; every projection direction separates the float32 model (|c| <= 0.1)
from its mutant (|c| >= 0.8) and the directions of a case are nearly orthogonal; the statistics gate rejects raw one-pass sums and a
miscounted ragged tile on the offset draw."""
import functools

import numpy as np
import pytest
import torch

import conv0_accuracy_model as M
import gemm_accuracy_model as G

NAMES = [c.name for c in M.CASES]


# ------------------------------------------------------------------ the table
def test_the_table_reaches_what_it_says():
    assert all(M.direct_shape(c) and c.st == 2 for c in M.CASES)
    assert not M.direct_shape(M.by_name("base-c128")._replace(st=4)) and not M.direct_shape(M.by_name("base-c128")._replace(st=1))
    base = M.by_name("base-c128")
    assert M.dims(base) == (2, 167, 3, 12) and 167 - 2 * M.TT == 7
    assert set(M.sites(base).tolist()) == {0, 1, 2}
    assert {c.C for c in M.CASES} >= {16, 48, 128}
    assert {c.kf for c in M.CASES} >= {13, 14, 8, 1} and {c.kt for c in M.CASES} == set(M.TOL) == {9, 5, 2}
    assert any(c.kf == 14 and c.sf == 7 for c in M.CASES) and any(c.kf == 5 and c.sf == 9 for c in M.CASES)
    assert any(c.pt == 0 for c in M.CASES) and any(c.pt == 4 and c.kt == 9 for c in M.CASES) and any(c.pt == c.kt - 1 for c in M.CASES)
    assert sum(c.noise for c in M.CASES) >= 3
    loop = M.by_name("tile-loop")
    assert M.dims(loop) == (80, 10, 1, 720) and 720 > 2 * 256            # (the GPU test asserts it against the device's CU count)
    rows = {M.by_name(n) for n in M.FWD_SELECTION_ROWS}
    assert len(rows) >= 6 and loop in rows and any(c.noise for c in rows) and {c.kf for c in rows} >= {13, 14, 1}
    xf = [M.by_name(n) for n in M.XF_SELECTION_ROWS]
    assert loop in xf and any(c.pt == 0 for c in xf) and {c.kf for c in xf if c.T >= 333} >= {13, 14}
    st = [M.by_name(n) for n in M.STAT_ROWS]
    assert base in st and loop in st and any(c.C == 48 for c in st)
    for c in M.CASES:
        assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in M.dense(c.name) if v is not None)


@pytest.mark.parametrize("name", NAMES)
def test_reference_agrees_with_the_oracle_on_a_config_without_batchnorm(name):
    """relu(conv(W)) - relu(conv(-W)) of oracle.ast_ref_torch.cnn_torch (bn = False) on the float32 product x * noise, float64."""
    from oracle.ast_ref_torch import cnn_torch
    c = M.by_name(name)
    W, X, noise = M.dense(name)
    xn = M.noisy(X, noise)
    cfg = M.cfg_of(c, bn=False)
    run = lambda w: cnn_torch(cfg, {"CNN_0/W": torch.tensor(w.astype(np.float64)).reshape(c.C, 1, c.kt, c.kf)}, torch.tensor(xn.astype(np.float64)))
    want = M.to_rows(c, (run(W) - run(-W)).numpy())
    ref = M.reference(c, W, xn)
    assert np.abs(ref - want).max() <= 1e-12 * np.abs(want).max()


# ------------------------------------------------------------------ gate (a)
@pytest.mark.parametrize("name", M.FWD_SELECTION_ROWS)
def test_forward_selection_is_exact_in_the_kernels_order_of_terms(name):
    c = M.by_name(name)
    X, noise, xn, redrawn = M.heavy_input(name, "fwd")
    print(f"{name}: redrawn share {redrawn:.4%}")
    assert redrawn <= 0.01
    hi, mid, lo = M.planes(xn)
    assert (hi + mid + lo == xn.astype(np.float64)).all() and (lo != 0).mean() > 0.9
    # the kernel's order with a weight that has a hi plane only: w.hi x x.lo, then w.hi x x.mid, then w.hi x x.hi -- on EVERY drawn value
    assert (M._f32(lo + mid) == lo + mid).all() and (M._f32(M._f32(lo + mid) + hi) == xn).all()
    Pk = M.window_k(c, xn)
    seen = np.zeros((c.C, c.kt, c.kf), int)
    passes = c.kt * c.kf
    for p in range(passes):
        W, expect = M.selection_fwd(name, p)
        assert ((W != 0).reshape(c.C, -1).sum(axis=1) == 1).all()
        seen += W != 0
        if p < 3 or p == passes - 1:                  # the whole model, rounding after every MFMA
            assert np.array_equal(M.model(c, M.weight_k(c, W), Pk).astype(np.float32), expect), (name, p)
    assert (seen == 1).all(), "every (channel, tap) pair is selected once"
    seq = M.tap_sequence(c)
    ks = [i * M.JP + j for i, j in seq]
    for b in range(32, c.kt * M.JP, 32):
        below, above = max(k for k in ks if k < b), min((k for k in ks if k >= b), default=None)
        assert below in ks[:2 * M.NKS] and (above is None or above in ks[:2 * M.NKS])
    pad = M.windows(c, xn)
    if c.pt:
        assert (pad[:, :, 0, :c.pt] == 0).all() and (expect == 0).any(), "taps that fall into the time padding select an exact zero"


@pytest.mark.parametrize("name", M.XF_SELECTION_ROWS)
def test_window_selection_every_unit_active_every_position_once(name):
    c = M.by_name(name)
    X, noise, xn, redrawn = M.heavy_input(name, "xf")
    print(f"{name}: redrawn share {redrawn:.4%}")
    assert redrawn <= 0.01
    W, bias, Y = M.xf_setup(name)
    assert (Y + bias.astype(np.float64) >= 0.5 * bias[0]).all(), "every unit is active with a margin of half the bias"
    F, T1, tiles_t, _ = M.dims(c)
    seen = np.zeros(c.B * F * T1, int)
    for p in range(M.xf_passes(c)):
        g, dW, val, rows = M.selection_xf(name, p)
        seen[rows[:max(0, seen.size - p * c.C)]] += 1            # (the last pass wraps round to positions of the first)
        assert ((M.to_rows(c, g) != 0).sum(axis=0) == 1).all()
        if p < 2:        # the library's weight gradient: a bf16x3 product of dY^T (selecting) and the windows -- exact in its order of terms
            w = M.windows(c, xn).reshape(-1, c.kt * c.kf)
            got = G.product(np.ascontiguousarray(M.to_rows(c, g).T), np.ascontiguousarray(w.T), "bf16x3", 128, 128)
            assert np.array_equal(got.astype(np.float32).reshape(dW.shape), dW)
    assert (seen == 1).all(), "every output position of every (b, f) is selected once"
    first = M.position_sequence(c)[:2 * c.B * F * tiles_t]
    assert set(first) == {g * T1 + t for g in range(c.B * F) for tt in range(tiles_t) for t in (tt * M.TT, min(T1, (tt + 1) * M.TT) - 1)}


# ------------------------------------------------------------------ gate (b)
def _err(x, ref, scale):
    return float((np.abs(x - ref) / scale).max())


@functools.lru_cache(maxsize=None)
def _model(name):
    Wk, Pk, ref, scale = M.dense_parts(name)
    return M.model(M.by_name(name), Wk, Pk)


def test_float32_model_error_is_what_the_tolerances_were_taken_from():
    worst = {}
    for c in M.CASES:
        Wk, Pk, ref, scale = M.dense_parts(c.name)
        e = _err(_model(c.name), ref, scale)
        print(f"{c.name:16s} kt {c.kt}: float32 model {e:.3e}")
        worst[c.kt] = max(worst.get(c.kt, 0.0), e)
    bad = []
    for kt, e in sorted(worst.items()):
        tab = M.F32_MODEL_ERR[kt]
        print(f"kt {kt}: float32 model {e:.3e}  table {tab:.2e}  tolerance {M.TOL[kt]:.2e}")
        bad += [(kt, e, tab)] * (not 0.8 * tab <= e <= tab)
        assert M.TOL[kt] == 4.0 * tab
    assert not bad, bad


@pytest.mark.parametrize("name", NAMES)
def test_error_gate_rejects_a_lost_mid_plane_a_missing_term_and_a_shifted_k_order(name):
    c = M.by_name(name)
    Wk, Pk, ref, scale = M.dense_parts(name)
    for m in M.GATE_B_MUTANTS:
        e = _err(M.model(c, Wk, Pk, mutant=m), ref, scale)
        print(f"{name}: {M.mutant_name(m)}: {e:.3e} (gate {M.TOL[c.kt]:.2e})")
        assert e > M.TOL[c.kt], (name, M.mutant_name(m), e)


# ------------------------------------------------------------------ gate (c)
@pytest.mark.parametrize("name", NAMES)
def test_projection_gates_separate_the_float32_model_from_every_mutant(name):
    c = M.by_name(name)
    Wk, Pk, ref, scale = M.dense_parts(name)
    dirs = M.directions(c)
    assert len(dirs) == len(set(M.sites(c).tolist())) * (2 + len(set(M.halves(c).tolist())))
    ps = {m: M.model(c, Wk, Pk, mutant=m, f32=False) - ref for m in dirs}
    worst_model, worst_mutant, worst_cos = 0.0, 9.0, 0.0
    for m, p in ps.items():
        cm = M.coefficient(_model(name), ref, p, scale)
        cx = M.coefficient(M.model(c, Wk, Pk, mutant=m), ref, p, scale)
        worst_model, worst_mutant = max(worst_model, abs(cm)), min(worst_mutant, abs(cx))
        assert abs(cm) <= M.C_F32_MAX, (name, M.mutant_name(m), cm)
        assert abs(cx) >= M.C_MUTANT_MIN, (name, M.mutant_name(m), cx)
    q = [(p / scale).ravel() for p in ps.values()]
    for i in range(len(q)):
        for j in range(i):
            worst_cos = max(worst_cos, abs(float(q[i] @ q[j])) / np.sqrt(float(q[i] @ q[i]) * float(q[j] @ q[j])))
    assert worst_cos <= M.COS_MAX, (name, worst_cos)
    # the merged defects: a lost lo plane of the weights (per fragment) or of the window shows on every component direction
    merged = [("zero", "w", 2, h) for h in sorted(set(M.halves(c).tolist()))] + [("zero", "x", 2, None)]
    for m in merged + [("x-lo-swap",)]:
        got = M.model(c, Wk, Pk, mutant=m)
        comp = M.components(c, ("zero", "x", 2, None) if m == ("x-lo-swap",) else m)
        cs = [M.coefficient(got, ref, ps[d], scale) for d in comp]
        print(f"{name}: {M.mutant_name(m)}: c = {min(cs):.3f} .. {max(cs):.3f} on its {len(comp)} component directions")
        assert comp and min(abs(x) for x in cs) >= M.C_MUTANT_MIN, (name, M.mutant_name(m), cs)
    print(f"{name}: {len(dirs)} directions, float32 model |c| <= {worst_model:.3f}, mutants |c| >= {worst_mutant:.3f}, largest cosine {worst_cos:.3f}")


# ------------------------------------------------------------------ gate (d)
@functools.lru_cache(maxsize=None)
def _bn(name, offset):
    c = M.by_name(name)
    cfg, P, X, noise, rng = M.bn_draws(name, offset)
    W = P["CNN_0/W"].reshape(c.C, c.kt, c.kf)
    xn = M.noisy(X, noise)
    Y64 = M.reference(c, W, xn)
    Y32 = M.model(c, M.weight_k(c, W), M.window_k(c, xn))
    return cfg, P, X, noise, rng, W, xn, Y64, Y32, M.pivots(c, W, X, noise)


def test_statistics_model_is_what_the_tolerances_were_taken_from_and_the_gate_rejects_two_mutants():
    bad = []
    for name in M.STAT_ROWS:
        c = M.by_name(name)
        worst = {"mean": 0.0, "var": 0.0}
        for offset in (False, True):
            cfg, P, X, noise, rng, W, xn, Y64, Y32, piv = _bn(name, offset)
            rm, rv, m = M.stats_reference(Y64)
            em, ev = M.stat_errors(*M.stats_model(c, Y32, piv)[:2], rm, rv)
            r = float((np.abs(rm) / np.sqrt(rv)).max())
            print(f"{name:16s} {'offset' if offset else 'benign'}: |mean| / std <= {r:6.1f}; float32 model: mean {em:.3e} var {ev:.3e}")
            worst["mean"], worst["var"] = max(worst["mean"], em), max(worst["var"], ev)
            if offset:
                assert r >= 20.0, "the offset draw must put channel means tens of standard deviations out"
                assert M.dims(c)[1] % M.TT != 0, "the last tile of a group must be ragged"
                for mut in ("raw", "cum80"):
                    xm, xv = M.stat_errors(*M.stats_model(c, Y32, piv, mutant=mut)[:2], rm, rv)
                    print(f"{name:16s} offset, mutant {mut}: mean {xm:.3e} var {xv:.3e}")
                    assert xm > M.STAT_TOL[name]["mean"] or xv > M.STAT_TOL[name]["var"], (name, mut, xm, xv)
        for k, e in worst.items():
            tab = M.STAT_MODEL_ERR[name][k]
            print(f"{name:16s} statistics {k}: float32 model {e:.3e}  table {tab:.2e}  tolerance {M.STAT_TOL[name][k]:.2e}")
            assert M.STAT_TOL[name][k] == 4.0 * tab
            bad += [(name, k, e, tab)] * (not 0.8 * tab <= e <= tab)
    assert not bad, bad
    assert set(M.STAT_MODEL_ERR) == set(M.BN_MODEL_ERR) == set(M.STAT_ROWS)


def test_batchnorm_step_model_is_what_the_out_and_gradient_tolerances_were_taken_from():
    bad = []
    for name in M.STAT_ROWS:
        c = M.by_name(name)
        cfg, P, X, noise, rng, W, xn, Y64, Y32, piv = _bn(name, False)
        out, gout, dW, dgamma, dbeta = M.bn_reference(c, cfg, P, X, noise)
        _, _, mean, var = M.stats_model(c, Y32, piv)
        o32, w32, g32, b32 = M.f32_bn_step(c, P, Y32.astype(np.float32), mean, var, gout, xn)
        e = {"out": M.tensor_error(o32, out), "dW": M.tensor_error(w32, dW), "dparam": max(M.tensor_error(g32, dgamma), M.tensor_error(b32, dbeta))}
        for k, v in e.items():
            tab = M.BN_MODEL_ERR[name][k]
            print(f"{name:16s} {k:6s}: float32 model {v:.3e}  table {tab:.2e}  tolerance {M.BN_TOL[name][k]:.2e}")
            assert M.BN_TOL[name][k] == 4.0 * tab
            bad += [(name, k, v, tab)] * (not 0.8 * tab <= v <= tab)
    assert not bad, bad
