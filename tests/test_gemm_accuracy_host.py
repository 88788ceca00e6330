"""What tests/test_gpu_gemm_accuracy.py relies on, shown on the CPU (tests/gemm_accuracy_model.py): the case table
reaches every kernel and operand form and plans the way it says; the selection identities are exact in the kernel's order of terms; the
float32 model stays within a quarter of every tolerance; the model's mutants exceed the error gate where it is expected to separate
(K <= 100) and every direction of the projection gates separates the float32 model (|c| <= 0.1) from the mutant (|c| >= 0.8)."""
import functools

import numpy as np
import pytest

import gemm_accuracy_model as G

KEYS = {}
for _c in G.CASES:
    KEYS.setdefault(G.arithmetic_key(_c), _c)
KEY_CASES = list(KEYS.values())          # one case per arithmetic: the model does not depend on layout or addressing


@pytest.fixture
def tlib():
    from ast_amd import _lib
    with _lib.load_test_hooks() as t:
        yield t


def test_the_table_reaches_every_kernel_and_operand_form():
    for kernel, (scheme, TLM, TL, fix) in G.KERNELS.items():
        mine = [c for c in G.CASES if c.kernel == kernel]
        forms = {(c.layout, G.expected_plan(c, G.STORE)["twolvl"]) for c in mine}
        assert forms == {(G.NT, 0), (G.NN, 0), (G.NN, 1), (G.TN, 0), (G.TN, 1)}, (kernel, forms)
        assert {c.K for c in mine} == set(G.KS), kernel
        assert all((c.M, c.N) == (TLM + 6, TL + 3) for c in mine)
        assert {m for c in mine if "split" in c.name for m in c.modes} == {G.STORE, G.ATOMIC, G.ACCUM}
        assert any(c.batch == 3 for c in mine) and any(c.bias for c in mine) and any(c.c_tn for c in mine)
        views = {v[0] for c in mine for v in (c.a_view, c.b_view) if v}
        assert views == {"2l", "perm", "tall"}, (kernel, views)
        # two-level M / N rows, and K-major two-level rows whose k-tiles lie inside one group and straddle one
        assert any(c.layout == G.NT and c.a_view and c.a_view[0] == "2l" for c in mine)
        assert any(c.layout != G.NT and c.b_view and c.b_view[0] == "2l" and c.b_view[1] > G.BK and c.b_view[1] % G.BK for c in mine)
        for c in mine:
            if "split" in c.name:
                n = [len(r) for r in G.ranges_of(c)]
                assert max(n) >= 3 and 2 in n, (c.name, n)
            if fix:
                assert G.expected_plan(c, G.STORE)["fix"] == 1, c.name


def test_every_case_plans_as_it_says(tlib):
    """astk_debug_gemm_views (plan only, made-up addresses) under the case's knobs, field by field; the dense cases also through
    astk_debug_gemm_plan.  tests/golden/gemm_plans.txt is not involved."""
    import ctypes as C
    seen = set()
    for c in G.CASES:
        A = np.zeros((c.batch, c.M, c.K), np.float32)
        B = np.zeros((c.batch, c.N, c.K), np.float32)
        ia, ib = G.operand_images(c, A, B)
        rc = G.Result(c.M, c.N, c.batch, c.c_tn)
        scheme, TLM, TL, fix = G.kernel_of(c)
        with G.Knobs([tlib], c):
            for mode in c.modes:
                rcode, text = G.views_call(tlib, c, mode, ia, ib, rc, (0x1000, 0x2000, 0x3000, 0x5000, 0x6000, 0x7000 if c.bias else None), launch=0)
                assert rcode == 0, (c.name, tlib.astk_last_error().decode())
                got, want = G.plan_fields(text), G.expected_plan(c, mode)
                assert {k: got[k] for k in want} == want, (c.name, mode, text)
                seen.add((got["tile"], got["prec"], got["fix"], c.layout, got["twolvl"]))
                # the library's own count of every tile's contributors against the model's copy of the stream-K split
                ranges = G.ranges_of(c)
                per_tile = [1] * len(G.plan_contributors(text)) if ranges is None else [len(r) for r in ranges]
                assert G.plan_contributors(text) == per_tile, (c.name, text, per_tile)
                if "split" in c.name:
                    assert max(G.plan_contributors(text)) >= 3 and 2 in G.plan_contributors(text), (c.name, text)
                if not G.is_view(c):
                    one = lambda v: (C.c_int32 * 1)(v)
                    buf = C.create_string_buffer(1 << 12)
                    assert tlib.astk_debug_gemm_plan(c.layout, 1, one(c.M), one(c.N), one(c.K), one(c.batch), one(mode), one(0), one(0), 0,
                                                     G.PREC_API[scheme], 0, 0, 0, 1, buf, len(buf)) == 0
                    dense = G.plan_fields(buf.value.decode())
                    assert {k: dense[k] for k in want} == want, (c.name, mode, buf.value.decode())
    assert len(seen) == 9 * 5, sorted(seen)


def test_knobs_are_restored(tlib):
    import ctypes as C
    v = C.c_double()
    before = {}
    for k in ("gemm.tile", "gemm.grid", "gemm.deterministic", "gemm.ticket"):
        assert tlib.astk_get_tuning(k.encode(), C.byref(v)) == 0
        before[k] = v.value
    with G.Knobs([tlib], G.by_name("x3-128-fix-split-store")):
        assert tlib.astk_get_tuning(b"gemm.tile", C.byref(v)) == 0 and v.value == 128
    for k, old in before.items():
        assert tlib.astk_get_tuning(k.encode(), C.byref(v)) == 0 and v.value == old, k


# ------------------------------------------------------------------ gate (a)
def test_bf16_split_represents_every_float32_value_and_rounds_to_nearest_even():
    rng = np.random.default_rng(1)
    x = G._heavy(rng, (200000,), "bf16x3")
    (hi, mid, lo), s = G.planes(x, "bf16x3")
    assert s == 1.0 and (hi + mid + lo == x.astype(np.float64)).all()
    import torch
    assert np.array_equal(hi.astype(np.float32), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    assert (lo != 0).mean() > 0.9


@pytest.mark.parametrize("role", ["A", "B"])
def test_selection_identities_are_exact_in_the_kernels_order(role):
    """Per arithmetic: the model in the kernel's order of terms (and its split) reproduces every selected entry exactly; at most 1 % of
    the draws had to be redrawn; the passes of a case together put a selecting entry on every k of [0, K)."""
    worst = 0.0
    for c in KEY_CASES:
        key = G.arithmetic_key(c)
        ks = set()
        for phase in range(G.phases(key, role)):
            A, B, expect, redrawn = G.selection(key, role, phase)
            worst = max(worst, redrawn)
            assert redrawn <= 0.01, (c.name, redrawn)
            got = G.model_case(c, A, B)
            assert np.array_equal(got.astype(np.float32), expect), c.name
            S = B if role == "A" else A
            assert ((S != 0).sum(axis=2) == 1).all()
            ks |= set(np.nonzero(S[0])[1].tolist())
        assert ks == set(range(c.K)), (c.name, sorted(set(range(c.K)) - ks))
    print(f"role {role}: worst redrawn share {worst:.4%}")


def test_some_order_of_the_bf16_terms_is_inexact_so_the_redraw_rule_has_work():
    rng = np.random.default_rng(2)
    x = G._heavy(rng, (2000000,), "bf16x3")
    bad = ~G.exact_under_every_order(x, "bf16x3")
    print(f"inexact under some order: {bad.mean():.4%}")
    assert 0 < bad.mean() <= 0.01


# ------------------------------------------------------------------ gate (b)
@functools.lru_cache(maxsize=None)
def _dense(name, mode):
    c = G.by_name(name)
    A, B, bias, c0 = G.dense_operands(G.arithmetic_key(c))
    c0 = c0 if mode == G.ACCUM else None
    return c, A, B, bias, c0, G.reference_case(c, A, B, bias, c0), G.scale_case(A, B, bias, c0)


def _err(x, ref, scale):
    return float((np.abs(x - ref) / scale).max())


def test_float32_model_error_is_what_the_tolerances_were_taken_from():
    worst = {}
    for c in KEY_CASES:
        for mode in c.modes:
            c, A, B, bias, c0, ref, scale = _dense(c.name, mode)
            e = _err(G.model_case(c, A, B, bias, c0), ref, scale)
            k = (G.kernel_of(c)[0], c.K)
            worst[k] = max(worst.get(k, 0.0), e)
    bad = []
    for (scheme, K), e in sorted(worst.items()):
        tab = G.F32_MODEL_ERR[scheme][K]
        print(f"{scheme:7s} K {K:4d}: float32 model {e:.3e}  table {tab:.2e}  tolerance {G.TOL[scheme][K]:.2e}")
        bad += [(scheme, K, e, tab)] * (not 0.8 * tab <= e <= tab)
        assert G.TOL[scheme][K] == 4.0 * tab
    assert not bad, bad
    assert set(worst) == {(s, K) for s in G.F32_MODEL_ERR for K in G.KS}


def test_error_gate_rejects_every_mutant_up_to_k_100():
    """Case by case (one per arithmetic), store mode: which mutants of the model exceed TOL.  K <= 100: every one must.  Deeper: recorded."""
    deep = {}
    for c in KEY_CASES:
        scheme, TLM, TL, _ = G.kernel_of(c)
        c, A, B, bias, c0, ref, scale = _dense(c.name, c.modes[0])
        tol = G.TOL[scheme][c.K]
        for m in G.mutants(scheme, TLM):
            e = _err(G.model_case(c, A, B, bias, c0, mutant=m), ref, scale)
            if c.K <= 100:
                assert e > tol, (c.name, G.mutant_name(m, scheme, TLM), e, tol)
            else:
                deep.setdefault((scheme, c.K), []).append((G.mutant_name(m, scheme, TLM), e > tol, e / tol))
    for k, rows in sorted(deep.items()):
        missed = sorted({n for n, hit, _ in rows if not hit})
        print(f"{k}: {sum(h for _, h, _ in rows)} of {len(rows)} mutant runs exceed the tolerance; smallest ratio {min(r for _, _, r in rows):.2f}; passing: {missed}")


# ------------------------------------------------------------------ gate (c)
def test_projection_gates_separate_the_float32_model_from_every_mutant():
    worst_model, worst_mutant, worst_cos = 0.0, 9.0, 0.0
    for c in KEY_CASES:
        scheme, TLM, TL, _ = G.kernel_of(c)
        dirs = G.directions(scheme, TLM)
        if not dirs:
            continue
        c, A, B, bias, c0, ref, scale = _dense(c.name, c.modes[0])
        model = G.model_case(c, A, B, bias, c0)
        ps = [G.model_case(c, A, B, bias, c0, mutant=m, f32=False) - ref for m in dirs]
        for m, p in zip(dirs, ps):
            cm = G.coefficient(model, ref, p, scale)
            cx = G.coefficient(G.model_case(c, A, B, bias, c0, mutant=m), ref, p, scale)
            worst_model, worst_mutant = max(worst_model, abs(cm)), min(worst_mutant, abs(cx))
            assert abs(cm) <= G.C_F32_MAX, (c.name, G.mutant_name(m, scheme, TLM), cm)
            assert abs(cx) >= G.C_MUTANT_MIN, (c.name, G.mutant_name(m, scheme, TLM), cx)
        # near-orthogonality: zeroing an operand's lowest plane IS leaving out the one term that uses it (cosine 1, by construction);
        # every other pair must be nearly orthogonal
        q = [(p / scale).ravel() for p in ps]
        for i in range(len(dirs)):
            for j in range(i):
                cos = abs(float(q[i] @ q[j])) / np.sqrt(float(q[i] @ q[i]) * float(q[j] @ q[j]))
                if dirs[i][0] == "zero" and dirs[j][0] == "drop" and G.SAME_DIRECTION[scheme][dirs[i][1]] == G.term_order(scheme, TLM)[dirs[j][2]]:
                    assert cos > 0.999, (c.name, i, j, cos)
                else:
                    worst_cos = max(worst_cos, cos)
                    assert cos <= G.COS_MAX, (c.name, G.mutant_name(dirs[i], scheme, TLM), G.mutant_name(dirs[j], scheme, TLM), cos)
    print(f"projection gates: float32 model |c| <= {worst_model:.3f}, mutants |c| >= {worst_mutant:.3f}, largest cosine of a distinct pair {worst_cos:.3f}")
