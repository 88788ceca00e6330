"""Host-side checks of tests/attn_model.py, the model behind tests/test_gpu_attn.py (no GPU): the case tables reach the branches of
ast_amd/csrc/attn.hip they are there for (a retune of split_for fails HERE instead of silently emptying the GPU test), the float64
reference agrees with torch autograd, a float32 restatement in the kernel's order of operations meets the GPU test's bounds on every case,
and the planted mistakes do not."""
import functools

import numpy as np
import pytest
import torch

import attn_model as AM

ALL = AM.CASES + AM.ROWS_CASES
_id = lambda c: ("rows-" if c.rows else "") + c.id


def _branches(c):
    if not c.rows:
        return AM.branches(c.B, c.T, c.H)
    return AM.branches(c.B, c.T, c.H, c.lengths(0)) | AM.branches(c.B, c.T, c.H, c.lengths(1))


@functools.lru_cache(maxsize=None)
def _reference(i, which=0):
    """(alpha, cv, ds, dq) of case i in float64; ds, dq None for a rows case (the rows variant has no backward)."""
    c = ALL[i]
    enc, q, g = c.inputs(which)
    if c.rows:
        return AM.reference(enc, q, c.row_utt, c.lengths(which)) + (None, None)
    alpha, cv = AM.reference(enc, q)
    return (alpha, cv) + AM.reference_bwd(enc, alpha, cv, g)


def _model_ratios(i, mistake=None, which=0):
    """{output: error of the float32 kernel model / the GPU test's bound}; the backward runs on the model's own alpha and cv."""
    c = ALL[i]
    enc, q, g = c.inputs(which)
    alpha, cv, ds, dq = _reference(i, which)
    if c.rows:
        a32, cv32 = AM.kernel_model(enc, q, c.row_utt, c.lengths(which), mistake=mistake)
        behind = np.arange(a32.shape[1])[None, :] >= AM.clamp_len(c.lengths(which), c.T)[:, None]
        assert mistake or (a32[behind] == 0).all()
    else:
        a32, cv32 = AM.kernel_model(enc, q, mistake=mistake)
    out = {"alpha": AM.bound_ratio(a32, alpha, AM.RTOL["alpha"]), "cv": AM.bound_ratio(cv32, cv, AM.RTOL["cv"])}
    if not c.rows:
        ds32, dq32 = AM.kernel_model_bwd(enc, a32, cv32, g, mistake=mistake)
        out["ds"] = AM.bound_ratio(ds32, ds, AM.RTOL["ds"])
        out["dq"] = AM.bound_ratio(dq32, dq, AM.RTOL["dq"])
    return out


# ------------------------------------------------------------------ the plan and the tables
def test_plan_restates_attn_hip_on_hand_worked_shapes():
    assert AM.split_for(32, 50) == (7, 8)              # want 16 -> cdiv(50, 16) = 4 -> the floor of 8 rows
    assert AM.split_for(3, 6) == (1, 6)                # chunk 8 > T -> T
    assert AM.split_for(5, 201) == (26, 8)
    assert AM.split_for(1, 1024) == (128, 8)           # exactly MAX_SPLIT: the clamp is not taken
    assert AM.split_for(1, 1025) == (114, 9)           # 129 chunks of 8 -> cdiv(1025, 128) = 9
    assert AM.split_for(4, 100000) == (128, 782)
    assert AM.split_for(512, 20) == (1, 20) and AM.split_for(511, 20) == (2, 10) and AM.split_for(100000, 3) == (1, 3)
    # partial rows of H + 4 floats, both parts aligned to 256 bytes
    assert AM.workspace_bytes(1, 1, 4) == 256 + 256
    assert AM.workspace_bytes(5, 201, 260) == AM.align_up(5 * 26 * 264 * 4, 256) + 256
    assert AM.workspace_bytes(600, 37, 1028) == AM.align_up(600 * 1032 * 4, 256) + AM.align_up(2400, 256)
    assert AM.counters_offset(600, 37, 1028) == AM.workspace_bytes(600, 37, 1028) - 2560
    assert [AM.nch(H) for H in (4, 256, 260, 512, 516, 1024, 1028, 2048)] == [1, 1, 2, 2, 4, 4, 8, 8]


@pytest.mark.parametrize("c", ALL, ids=_id)
def test_every_case_reaches_what_its_entry_says(c):
    assert AM.split_for(c.B, c.T) == c.plan
    assert c.reaches <= _branches(c), sorted(c.reaches - _branches(c))
    assert c.H % 4 == 0 and c.H <= 2048
    if c.rows:
        assert len(c.row_utt) == len(c.row_len) == len(c.row_len2) == c.B and set(c.row_utt) == set(range(c.U))
        for which in (0, 1):                            # part of enc is poisoned in each launch, and not all of it
            bad = np.isnan(c.poisoned(np.zeros((c.U, c.T, 1), np.float32), which)[:, :, 0])
            assert bad.any() and not bad.all(1).any()


def test_tables_cover_every_branch_of_the_scan():
    reached = set().union(*(c.reaches for c in AM.CASES))
    assert {"nch1", "nch2", "nch4", "nch8", "nsplit1", "nsplit128", "clamp", "last_chunk_1", "last_chunk_2", "empty_wave", "lone_row",
            "lone_beside_pair", "one_lane_chunk", "ragged_chunk", "B511", "B512"} <= reached
    by = {(c.B, c.T, c.H): c for c in AM.CASES}
    assert by[(511, 20, 8)].plan[0] == 2 and by[(512, 20, 8)].plan[0] == 1            # the boundary at 511 / 512 rows is crossed
    assert any(c.plan[0] == 128 and "clamp" not in _branches(c) for c in AM.CASES)    # exactly MAX_SPLIT, not clamped
    assert any("clamp" in c.reaches and AM.nch(c.H) == 8 for c in AM.CASES)
    # with the operator test's (.., 512) and (.., 1024): both sides of every boundary of the instantiation table
    assert {c.H for c in AM.CASES} >= {4, 252, 256, 260, 516, 1028, 1540, 2048}
    rows = set().union(*(c.reaches for c in AM.ROWS_CASES))
    assert {"nch8", "nch2", "clamp", "nsplit1", "empty_partial", "mostly_empty", "len0", "len_above_T", "len_chunk-1", "len_chunk",
            "len_chunk+1"} <= rows
    assert any(c.B >= 512 for c in AM.ROWS_CASES)
    for c in AM.ROWS_CASES[:2]:                         # between the two launches: every length of the issue's set
        nsplit, chunk = c.plan
        assert set(c.row_len) | set(c.row_len2) == {0, 1, chunk - 1, chunk, chunk + 1, c.T, c.T + 5}


def test_drawn_scores_leave_no_split_without_weight():
    """Inputs of standard deviation H ** -0.25 make the scores ~ N(0, 1): on the long cases no position holds more than a fifth of a
    row's weight (as drawn: 0.008 at (1, 2000, 2048), 0.118 at (64, 420, 1540), the largest of them)."""
    big = {(c.B, c.T, c.H): _reference(i)[0].max() for i, c in enumerate(AM.CASES) if c.T >= 420}
    print({k: f"{v:.3f}" for k, v in big.items()})
    assert big[(1, 2000, 2048)] < 0.02 and max(big.values()) < 0.2


# ------------------------------------------------------------------ the reference against torch float64
@pytest.mark.parametrize("i", [0, 1, 4, 10], ids=lambda i: ALL[i].id)
def test_reference_against_torch_autograd(i):
    c = ALL[i]
    enc, q, g = c.inputs()
    e, qq = torch.tensor(enc, dtype=torch.float64), torch.tensor(q, dtype=torch.float64)
    s = torch.einsum("bth,bh->bt", e, qq).requires_grad_()
    a = torch.softmax(s, 1)
    cv = torch.einsum("bth,bt->bh", e, a)
    cv.backward(torch.tensor(g, dtype=torch.float64))
    alpha, cv_ref, ds, dq = _reference(i)
    assert alpha.shape == (c.B, AM.padded(c.T)) and (alpha[:, c.T:] == 0).all() and (ds[:, c.T:] == 0).all()
    np.testing.assert_allclose(alpha[:, :c.T], a.detach().numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(cv_ref, cv.detach().numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(ds[:, :c.T], s.grad.numpy(), rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(dq, torch.einsum("bt,bth->bh", s.grad, e).numpy(), rtol=1e-10, atol=1e-15)


@pytest.mark.parametrize("i", [len(AM.CASES) + 1, len(AM.CASES) + 3], ids=lambda i: "rows-" + ALL[i].id)
def test_rows_reference_against_torch(i):
    c = ALL[i]
    enc, q, _ = c.inputs()
    alpha, cv = _reference(i)[:2]
    Tb = AM.clamp_len(c.lengths(), c.T)
    assert Tb.min() == 1 and Tb.max() == c.T
    e = torch.tensor(enc, dtype=torch.float64)[torch.tensor(c.row_utt)]
    s = torch.einsum("bth,bh->bt", e, torch.tensor(q, dtype=torch.float64))
    s = s.masked_fill(torch.arange(c.T)[None, :] >= torch.tensor(Tb)[:, None], -float("inf"))
    a = torch.softmax(s, 1)
    assert (alpha[np.arange(alpha.shape[1])[None, :] >= Tb[:, None]] == 0).all()
    np.testing.assert_allclose(alpha[:, :c.T], a.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(cv, torch.einsum("bth,bt->bh", e, a).numpy(), rtol=1e-12, atol=1e-15)
    # nothing behind a row's length is read: the reference is unchanged on the poisoned encoder states
    a2, cv2 = AM.reference(c.poisoned(enc), q, c.row_utt, c.lengths())
    assert np.array_equal(a2, alpha) and np.array_equal(cv2, cv)


# ------------------------------------------------------------------ the kernel model against the reference
def test_kernel_model_meets_the_gpu_bounds_on_every_case():
    """The float32 restatement of the kernel stays within the GPU test's bounds (2e-4 of the largest entry for alpha and cv, 5e-4 for ds
    and dq) of the float64 reference on every case, both draws of a case: the bounds are reachable in float32 at these shapes.
    Largest error / bound over the tables, as measured: alpha 0.0018 at (1, 2000, 2048), cv 0.0037 at (1, 1024, 1028), ds 0.0008 at
    (64, 420, 1540), dq 0.0014 at (3, 1100, 1540)."""
    worst = {}
    for i, c in enumerate(ALL):
        for which in (0, 1):
            for k, v in _model_ratios(i, which=which).items():
                if v > worst.get(k, (0, None))[0]:
                    worst[k] = (v, _id(c))
                assert v <= 1, (_id(c), which, k, v)
    print({k: (f"{v:.4f}", w) for k, (v, w) in worst.items()})
    assert max(v for v, _ in worst.values()) <= 0.25     # the project's rule: plain float32 within a quarter of the tolerance


# ------------------------------------------------------------------ planted mistakes
def _with(tag):
    return [i for i, c in enumerate(ALL) if tag in c.reaches]


@pytest.mark.parametrize("i", _with("nch8"), ids=lambda i: _id(ALL[i]))
def test_mistake_columns_from_1024_dropped_breaks_every_nch8_case(i):
    r = _model_ratios(i, "nch4")
    print(r)
    assert r["cv"] > 1 and r["alpha"] > 1 and r.get("dq", 2) > 1, r


@pytest.mark.parametrize("i", sorted(set(_with("lone_row") + _with("lone_beside_pair"))), ids=lambda i: _id(ALL[i]))
def test_mistake_lone_row_waves_second_row_read_breaks_every_lone_row_case(i):
    r = _model_ratios(i, "lone_row_pair")
    print(r)
    assert r["alpha"] > 1 or r["cv"] > 1, r
    assert ALL[i].rows or r["ds"] > 1 or r["dq"] > 1, r


@pytest.mark.parametrize("i", _with("empty_partial"), ids=lambda i: _id(ALL[i]))
def test_mistake_in_the_weight_of_an_empty_partial(i):
    """An empty partial carries l = 0 and acc = 0, so the weight 1 in place of 0 changes no value at all (shown here: bit-identical
    outputs) -- what the `-inf -> weight 0` guard keeps out is expf(-inf - -inf) = NaN in a workgroup ALL of whose waves are empty, which
    the merge would multiply into the row.  The mistake that breaks the bounds is therefore the guard dropped, and it breaks them on
    every case with a split wholly behind a row's length."""
    c = ALL[i]
    enc, q, _ = c.inputs()
    good = AM.kernel_model(enc, q, c.row_utt, c.lengths())
    one = AM.kernel_model(enc, q, c.row_utt, c.lengths(), mistake="empty_weight_1")
    assert np.array_equal(good[0], one[0]) and np.array_equal(good[1], one[1])
    r = _model_ratios(i, "empty_guard_dropped")
    assert r["alpha"] > 1 and r["cv"] > 1, r


def test_mistakes_leave_the_other_cases_alone():
    """The planted mistakes are confined to their branch: without it the model is unchanged (so a case's entry is what shows them)."""
    for i, c in enumerate(ALL):
        if c.B * c.T * c.H > 1 << 18:
            continue
        enc, q, _ = c.inputs()
        args = (enc, q) + ((c.row_utt, c.lengths()) if c.rows else ())
        good = AM.kernel_model(*args)
        for mistake, tags in (("nch4", {"nch8"}), ("lone_row_pair", {"lone_row", "lone_beside_pair"}),
                              ("empty_guard_dropped", {"empty_partial"})):
            if not (tags & _branches(c)) and not (c.rows and mistake == "lone_row_pair"):   # a row's length ends chunks anywhere
                bad = AM.kernel_model(*args, mistake=mistake)
                assert np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1]), (_id(c), mistake)
