"""Host-side checks of the models behind tests/test_gpu_optimizer.py (no GPU): the tolerances the GPU tests apply are DERIVED here from
the float32 evaluation of tests/optimizer_model.py against its float64 evaluation on every case the GPU suite runs (the project's rule:
plain float32 must stay within a quarter of the tolerance); every named mutant of the update must miss a tolerance on some case; the
cases have the properties that make the mutants visible; and tests/rng_model.py is a sane random stream with the concatenation
property the kernels' (seed, offset) contract promises."""
import numpy as np
import pytest

import optimizer_model as OM
import rng_model as RM
from conftest import tiny_cfg

QUANT = ("p", "m", "v", "vhat")


def _figs(got, ref, quantities):
    """worst error of a trajectory, per quantity, relative to the reference tensor's maximum at that step (the norm: to itself)."""
    out = {q: 0.0 for q in quantities}
    for a, b in zip(got, ref):
        for q in quantities:
            e = abs(a["norm"] - b["norm"]) / b["norm"] if q == "norm" and b["norm"] > 0 else OM.relerr(a[q], b[q]) if q != "norm" else abs(a["norm"])
            out[q] = max(out[q], e)
    return out


def _tiny_arena():
    from ast_amd.params import param_shapes
    from oracle import ast_ref as R
    cfg = tiny_cfg()
    shapes, _ = param_shapes(cfg, 26, 11)
    P = R.init_params(cfg, 26, 11, seed=0, dtype=np.float32)
    return shapes, OM.arena_vector(shapes, P), OM.arena_gradients(shapes, OM.FREEZE, OM.ARENA_STEPS)


_ARENA_RUNS = [(kind, eta) for kind in ("adam", "sgd") for eta in (0.0, OM.NOISE_ETA)]


@pytest.fixture(scope="module")
def float32_figures():
    """{quantity: worst float32-model error over every case of the GPU suite}."""
    worst = {k: 0.0 for k in OM.TOL}

    def take(figs, rename=None):
        for q, e in figs.items():
            q = (rename or {}).get(q, q)
            worst[q] = max(worst[q], e)
    for c in OM.adam_cases():
        take(_figs(c.run(np.float32), c.build().ref, QUANT + ("norm",)))
    for c in OM.sgd_cases():
        take(_figs(c.run(np.float32), c.build().ref, ("p", "norm")), {"p": "sgd_p"})
    for n in OM.SIZES:
        for l2, gsc in OM.NORM_PARAMS:
            p, g = OM.norm_inputs(n, l2, gsc)
            n64 = OM.finished_gradient(p, g, gsc=gsc, l2=l2)[1]
            n32 = OM.finished_gradient(p, g, gsc=gsc, l2=l2, dtype=np.float32)[1]
            take({"norm": abs(n32 - n64) / n64})
    for n in OM.HOOK_SIZES:
        p, g, l2, gsc, clip = OM.hook_inputs(n)
        for off in OM.HOOK_OFFSETS:
            for sigma in OM.HOOK_SIGMAS:
                z = RM.hook_noise(n, OM.NOISE_SEED, off)
                g64 = OM.finished_gradient(p, g, gsc=gsc, l2=l2, clip=clip)[0] + sigma * z
                g32 = OM.finished_gradient(p, g, gsc=gsc, l2=l2, clip=clip, dtype=np.float32)[0] + (np.float32(sigma) * z.astype(np.float32))
                assert g32.dtype == np.float32
                take({"hook": OM.relerr(g32, g64)})
    shapes, p0, grads = _tiny_arena()
    for kind, eta in _ARENA_RUNS:
        ref = OM.arena_run(shapes, p0, OM.FREEZE, grads, kind, eta)
        got = OM.arena_run(shapes, p0, OM.FREEZE, grads, kind, eta, dtype=np.float32)
        take(_figs(got, ref, (QUANT if kind == "adam" else ("p",)) + ("norm",)), {"p": "sgd_p"} if kind == "sgd" else None)
        if eta > 0:
            take({"hook": max(OM.relerr(a["grad"], b["grad"]) for a, b in zip(got, ref))})
    return worst


def _smallest_125(x):
    """the smallest value of the form {1, 2, 5} x 10^k that is >= x."""
    k = int(np.floor(np.log10(x)))
    for kk in (k - 1, k, k + 1):
        for d in (1, 2, 5):
            if d * 10.0 ** kk >= x:
                return float(f"{d}e{kk}")
    raise AssertionError(x)


def test_tolerances_are_the_quarter_rule_applied_to_the_float32_model(float32_figures):
    """Each constant of optimizer_model.TOL is the smallest {1, 2, 5} x 10^k that leaves the float32 evaluation within a quarter of it."""
    print({q: f"{e:.2e}" for q, e in float32_figures.items()})
    for q, e in float32_figures.items():
        assert e <= OM.TOL[q] / 4, (q, e, OM.TOL[q])
        assert OM.TOL[q] == _smallest_125(4 * e), (q, e, OM.TOL[q], _smallest_125(4 * e))


def _misses(got, ref, quantities, rename=None):
    figs = _figs(got, ref, quantities)
    return {q: e for q, e in figs.items() if e > OM.TOL[(rename or {}).get(q, q)]}


def _small(cases):
    return [c for c in cases if c.n <= 10007]


@pytest.mark.parametrize("mutant", OM.MUTANTS)
def test_every_mutant_misses_a_tolerance_on_a_case_the_gpu_suite_runs(mutant):
    """A wrong update must not pass: each mutant, evaluated in float64, is outside the stated tolerance on at least one case."""
    hits = []
    if mutant == "norm_over_enabled_only":
        shapes, p0, grads = _tiny_arena()
        for kind, eta in _ARENA_RUNS:
            ref = OM.arena_run(shapes, p0, OM.FREEZE, grads, kind, eta)
            got = OM.arena_run(shapes, p0, OM.FREEZE, grads, kind, eta, mutant=mutant)
            if _misses(got, ref, ("norm", "p"), {"p": "sgd_p"} if kind == "sgd" else None):
                hits.append((kind, eta))
    elif mutant == "sgd_without_decay":
        hits = [c.name for c in _small(OM.sgd_cases()) if _misses(c.run(mutant=mutant), c.build().ref, ("p",), {"p": "sgd_p"})]
    else:
        hits = [c.name for c in _small(OM.adam_cases()) if _misses(c.run(mutant=mutant), c.build().ref, QUANT + ("norm",))]
        hits += [c.name for c in _small(OM.sgd_cases()) if _misses(c.run(mutant=mutant), c.build().ref, ("p", "norm"), {"p": "sgd_p"})]
    assert hits, f"{mutant} passes every case: the cases are too weak"


def test_cases_have_the_properties_that_make_the_mutants_visible():
    active = inactive = 0
    for c in OM.adam_cases() + OM.sgd_cases():
        c.build()
        for st in c.ref:
            if c.zero or c.clip == OM.NO_CLIP:
                continue
            assert not 0.67 * c.clip <= st["norm"] <= 1.5 * c.clip, (c.name, st["norm"])       # float32 and float64 on the same side
            active += st["norm"] > c.clip
            inactive += st["norm"] < c.clip
        assert all(np.isfinite(st[q]).all() for st in c.ref for q in QUANT)
    assert active >= 8 and inactive >= 8
    # AMSGrad's maximum matters: vhat > v on at least a quarter of the elements at the last step of a multi-step case
    for name in ("amsgrad-10007", "amsgrad-1023"):
        last = next(c for c in OM.adam_cases() if c.name == name).ref[-1]
        assert np.mean(last["vhat"] > last["v"]) >= 0.25, name
    # the frozen links carry more than half of the clip norm's sum of squares, and the clip is active
    shapes, p0, grads = _tiny_arena()
    offsets, sizes, total = OM.arena_layout(shapes)
    ranges = OM.enabled_ranges(shapes, OM.FREEZE)
    enabled = np.zeros(total, bool)
    for o, n in ranges:
        enabled[o:o + n] = True
    assert 0 < enabled.sum() < total and len(ranges) >= 2
    for kind, eta in _ARENA_RUNS:
        pin = p0
        for g, st in zip(grads, OM.arena_run(shapes, p0, OM.FREEZE, grads, kind, eta)):
            gd, norm = OM.finished_gradient(pin, g, **{k: v for k, v in OM.ARENA_HYPER.items() if k == "l2"})
            assert (gd[~enabled] ** 2).sum() > 0.5 * norm ** 2 and norm > 1.5 * OM.ARENA_HYPER["clip"]
            assert abs(norm - st["norm"]) <= 1e-6 * norm
            pin = st["p"]
            # frozen tensors never move, their moments stay 0
            assert np.array_equal(st["p"][~enabled], p0[~enabled].astype(np.float64)) and not st["m"][~enabled].any()


def test_model_reproduces_the_freeze_example_worked_by_hand():
    """a = [3, 4] frozen, b = [1], gradients equal to the values, l2 = 0, clip = 2, SGD lr 0.1: norm sqrt(26), b -> 1 - 0.1 * 2 / sqrt(26)."""
    shapes = {"a/W": (2,), "b/W": (1,)}
    p0 = OM.arena_vector(shapes, {"a/W": [3, 4], "b/W": [1]})
    s = OM.update(OM.State(p0), p0.copy(), kind="sgd", l2=0.0, clip=2.0, lr=0.1, ranges=OM.enabled_ranges(shapes, {"a"}))
    assert abs(s.norm - np.sqrt(26)) < 1e-12 and abs(s.p[4] - (1 - 0.1 * 2 / np.sqrt(26))) < 1e-8
    assert list(s.p[:4]) == [3, 4, 0, 0]


# ------------------------------------------------------------------ the RNG model
N20 = 1 << 20


@pytest.mark.parametrize("ratio", [0.1, 0.3, 0.5])
def test_rng_model_keep_rate(ratio):
    keep = RM.dropout_mask(N20, ratio, 1234, 0) > 0
    sd = np.sqrt(ratio * (1 - ratio) / N20)
    assert abs(keep.mean() - (1 - ratio)) < 4 * sd
    assert set(np.unique(RM.dropout_mask(4096, ratio, 1, 0))) == {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(ratio))}


def test_rng_model_halves_of_one_hash_are_uncorrelated():
    keep = (RM.dropout_mask(2 * N20, 0.3, 77, 0) > 0).astype(np.float64)
    assert abs(np.corrcoef(keep[0::2], keep[1::2])[0, 1]) < 4 / np.sqrt(N20)
    z = RM.unit_normals(2 * N20, 78, 0)
    assert abs(np.corrcoef(z[0::2], z[1::2])[0, 1]) < 4 / np.sqrt(N20)
    h = RM.hook_noise(2 * N20, 79, 0)
    assert abs(np.corrcoef(h[0::2], h[1::2])[0, 1]) < 4 / np.sqrt(N20)


def test_rng_model_normals_have_the_moments_asked_for():
    for z, mean, sigma in ((RM.normal_fill(N20, 1.0, 0.25, 99, 0), 1.0, 0.25), (RM.hook_noise(N20, 5, 2 ** 33 + 1), 0.0, 1.0)):
        assert abs(z.mean() - mean) < 4 * sigma / np.sqrt(N20)
        assert abs(z.std() - sigma) < 4 * sigma / np.sqrt(2 * N20)


@pytest.mark.parametrize("n1", [1, 6, 7])
@pytest.mark.parametrize("off", [0, 3, 2 ** 33 + 1, 2 ** 33 + 2])
def test_rng_model_dropout_concatenates(n1, off):
    """A fill is a function of the global index alone: mask(n1 + n2, off) = mask(n1, off) ++ mask(n2, off + n1), odd and even n1 / off."""
    n2 = 9
    whole = RM.dropout_mask(n1 + n2, 0.3, 5, off)
    assert np.array_equal(whole, np.concatenate([RM.dropout_mask(n1, 0.3, 5, off), RM.dropout_mask(n2, 0.3, 5, off + n1)]))
    assert 0 < (whole > 0).sum() < n1 + n2 or n1 + n2 < 8


def test_rng_model_numpy_hash_equals_the_plain_integer_hash():
    for seed, ctr in ((0, 0), (0x5EED, 1), (1234, 2 ** 33 + 1), (2 ** 64 - 1, 2 ** 63 + 5)):
        assert int(RM._hash(seed, [ctr])[0]) == RM.scalar_hash(seed, ctr)
    # element g of a mask reads the half of the pair's hash its parity selects
    h = RM.scalar_hash(9, 3 >> 1)
    u = (((h >> 32) >> 8) + 1) * 2.0 ** -24
    assert RM.dropout_uniforms(1, 9, 3)[0] == u
