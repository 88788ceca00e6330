"""GPU tests of astk_risk_weights (include/astk.h; csrc/risk.hip) through the C ABI on the named cases of
tests/risk_model.py against ast_amd.mrt.risk_weights_host, bad lists, the host refusals, run-to-run equality, and
eval.pair_stats(return_device=True)."""
import ctypes as C

import numpy as np
import pytest
import torch

import risk_model as RM
from test_gpu_ops import dev, ok, stream, vp

pytestmark = pytest.mark.gpu
CASES = RM.cases()
POISON = -123.5


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


def _arrays(first, score, stats, lens, pairs, flags):
    return (dev(first, torch.int32), dev(np.asarray(score, np.float32)), dev(stats, torch.int32), dev(lens, torch.int32), dev(pairs, torch.int32),
            dev(flags, torch.int32))


def _run(lib, case, cost, desc=None, outs=True, with_n_bad=True, null=None):
    """astk_risk_weights on a case's host arrays: (status, weight, risk, cost_out, n_bad) with the outputs as host arrays; the output
    buffers start poisoned and carry a spare poisoned element behind them."""
    from ast_amd import _lib
    U, R = len(case["first"]) - 1, len(case["flags"])
    ins = list(_arrays(*(case[k] for k in ("first", "score", "stats", "lens", "pairs", "flags"))))
    d = desc or _lib.RiskDesc(U, R, _lib.RISK_COSTS[cost], case["alpha"], case["risk_scale"], case["ref_weight"])
    w = torch.full((R + 1,), POISON, device="cuda")
    risk = torch.full((U + 1,), POISON, device="cuda")
    c = torch.full((R + 1,), POISON, device="cuda")
    n_bad = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    ptrs = [vp(t) for t in ins] + [vp(w)]
    if null is not None:
        ptrs[null] = None
    rc = lib.astk_risk_weights(C.byref(d), *ptrs, vp(risk) if outs else None, vp(c) if outs else None, vp(n_bad) if with_n_bad else None,
                               stream())
    torch.cuda.synchronize()
    return rc, w.cpu().numpy(), risk.cpu().numpy(), c.cpu().numpy(), n_bad.cpu().numpy()


@pytest.mark.parametrize("cost", RM.COSTS)
@pytest.mark.parametrize("name", list(CASES))
def test_risk_weights_against_the_host_model(lib, name, cost):
    """Every named case under both costs: weight, risk and cost_out within 2^-23 |model| + 1e-12 (|risk_scale| alpha max c + |ref_weight|)
    (risk_model.bounds) of risk_weights_host, nothing written behind the arrays, n_bad 0; a second run gives the same bits, and so does
    a run without the optional outputs."""
    case = CASES[name]
    rc, w, risk, c, n_bad = _run(lib, case, cost)
    ok(lib, rc)
    R, U = len(case["flags"]), len(case["first"]) - 1
    want = RM.host(case, cost)
    assert w[R] == POISON and risk[U] == POISON and c[R] == POISON and n_bad.tolist() == [0, -7]
    worst = []
    for got, ref, bound, what in zip((w[:R], risk[:U], c[:R]), want[:3], RM.bounds(case, RM.direct(case, cost)), ("weight", "risk", "cost")):
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        worst.append(float((err / np.maximum(bound, 1e-300)).max()))
        print(name, cost, what, "worst err", err.max(), "as a fraction of its bound", worst[-1], "bit-equal", bool((got == ref).all()))
        assert (err <= bound).all(), (name, cost, what, err.max())
    again = _run(lib, case, cost)
    assert again[1].tobytes() == w.tobytes() and again[2].tobytes() == risk.tobytes() and again[3].tobytes() == c.tobytes()
    bare = _run(lib, case, cost, outs=False, with_n_bad=False)
    assert bare[0] == 0 and bare[1].tobytes() == w.tobytes()
    assert (bare[2] == POISON).all() and (bare[3] == POISON).all() and bare[4].tolist() == [-7, -7]


def test_bad_lists_are_counted_and_zeroed_and_leave_their_neighbours_alone(lib):
    """A list of 65 rows between two good ones, and a descent in the offsets: counted in n_bad, their rows' weights 0, the neighbours'
    results those of the lists alone; the host model agrees row for row."""
    from ast_amd import mrt
    a, b, big = RM.make_case([3], seed=20, risk_scale=2.0), RM.make_case([4], seed=21, risk_scale=2.0), RM.make_case([65], seed=22)
    cat = lambda k: np.concatenate([a[k], big[k], b[k]])
    pairs = np.concatenate([a["pairs"], big["pairs"] + len(a["lens"]), b["pairs"] + len(a["lens"]) + len(big["lens"])])
    R = 72
    alone_a, alone_b = _run(lib, a, "bleu"), _run(lib, b, "bleu")
    for first, n_want in (([0, 3, 68, 72], 1), ([0, 3, 2, 72], 2)):
        case = dict(first=np.asarray(first, np.int32), score=cat("score"), stats=cat("stats"), lens=cat("lens"), pairs=pairs, flags=cat("flags"),
                    alpha=1.0, risk_scale=2.0, ref_weight=0.0)
        rc, w, risk, c, n_bad = _run(lib, case, "bleu")
        ok(lib, rc)
        assert n_bad.tolist() == [n_want, -7] and w[R] == POISON and c[R] == POISON and risk[3] == POISON
        assert (w[3:68] == 0).all() and (c[3:68] == 0).all() and risk[1] == 0
        assert w[:3].tobytes() == alone_a[1][:3].tobytes() and risk[0] == alone_a[2][0]
        hw, hr, hc, hn = mrt.risk_weights_host(case["first"], case["score"], case["stats"], case["lens"], case["pairs"], case["flags"], "bleu",
                                               1.0, 2.0, 0.0, fill=POISON)
        assert hn == n_want
        np.testing.assert_array_equal(hw == 0, w[:R] == 0)
        if n_want == 1:
            assert w[68:72].tobytes() == alone_b[1][:4].tobytes() and risk[2] == alone_b[2][0]
        else:
            assert (w[68:72] == 0).all() and risk[2] == 0


def test_refusals_launch_nothing(lib):
    from ast_amd import _lib
    case = CASES["ragged"]
    U, R = len(case["first"]) - 1, len(case["flags"])
    good = dict(U=U, R=R, cost=0, alpha=1.0, risk_scale=1.0, ref_weight=0.0)
    bad = [("struct_size", dict(struct_size=8)), ("U", dict(U=0)), ("R", dict(R=0)), ("cost", dict(cost=2)), ("cost", dict(cost=-1)),
           ("alpha", dict(alpha=-0.5)), ("alpha", dict(alpha=float("nan"))), ("alpha", dict(alpha=float("inf"))),
           ("risk_scale", dict(risk_scale=float("inf"))), ("ref_weight", dict(ref_weight=float("nan")))]
    for word, change in bad:
        d = _lib.RiskDesc(**good)
        for k, v in change.items():
            setattr(d, k, v)
        rc, w, risk, c, n_bad = _run(lib, case, "bleu", desc=d)
        assert rc != 0 and word in lib.astk_last_error().decode(), (word, lib.astk_last_error())
        assert (w == POISON).all() and (risk == POISON).all() and (c == POISON).all() and n_bad.tolist() == [-7, -7]
    for null, word in enumerate(("first", "score", "stats", "lens", "pairs", "flags", "weight")):
        rc, w, risk, c, n_bad = _run(lib, case, "bleu", null=null)
        assert rc != 0 and word in lib.astk_last_error().decode()
        assert (w == POISON).all() and (risk == POISON).all() and (c == POISON).all() and n_bad.tolist() == [-7, -7]


def test_python_call_and_pair_stats_on_the_device(lib):
    """eval.pair_stats(return_device=True) returns the default call's numbers as device tensors, with the lengths and pairs it read; fed to
    mrt.risk_weights they give risk_weights_host's weights on the host statistics."""
    from ast_amd import mrt
    from ast_amd.eval import pair_stats
    samples = [[np.array([5, 6, 2]), np.array([5, 9, 7, 2]), np.array([5, 6, 2])], [np.array([4, 6, 8, 2]), np.array([8, 8, 2]), np.array([2])]]
    refs = np.array([[1, 5, 6, 7, 2, 0], [1, 4, 6, 8, 9, 2]], np.int32)
    b = mrt.build_mrt_batch(samples, refs)
    host = pair_stats(b["pool"], b["pairs"])
    stats, lens, pairs = pair_stats(b["pool"], b["pairs"], return_device=True)
    assert stats.is_cuda and stats.dtype == torch.int32 and tuple(stats.shape) == (8, 8)
    np.testing.assert_array_equal(stats.cpu().numpy(), host)
    np.testing.assert_array_equal(lens.cpu().numpy(), [len(s) for s in b["pool"]])
    np.testing.assert_array_equal(pairs.cpu().numpy(), b["pairs"])
    score = np.array([-1.0, -2.5, -1.0, 0.0, -0.5, -3.0, -4.0, 0.0], np.float32)
    n_bad = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    w, risk, c = mrt.risk_weights(dev(b["first"], torch.int32), dev(score), stats, lens, pairs, dev(b["flags"], torch.int32), "edit", 0.5, 4.0,
                                  1.0, with_cost=True, n_bad=n_bad)
    hw, hr, hc, hn = mrt.risk_weights_host(b["first"], score, host, [len(s) for s in b["pool"]], b["pairs"], b["flags"], "edit", 0.5, 4.0, 1.0)
    case = dict(alpha=0.5, risk_scale=4.0, ref_weight=1.0)
    bw, br, bc = RM.bounds(case, (hw, hr, hc))
    assert int(n_bad) == 0 == hn
    assert (np.abs(w.cpu().numpy().astype(np.float64) - hw) <= bw).all() and (np.abs(risk.cpu().numpy().astype(np.float64) - hr) <= br).all()
    assert (np.abs(c.cpu().numpy().astype(np.float64) - hc) <= bc).all()
    assert hw[3] == 1.0 and hw[7] == 1.0 and hw[2] == 0.0, "reference rows carry ref_weight alone, the duplicate nothing"
