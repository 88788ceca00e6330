"""Host-side checks of the models behind tests/test_gpu_row_panel.py (no GPU): the tolerances the GPU tests apply are DERIVED here from
the float32 evaluations of tests/row_panel_model.py against its float64 evaluation on every case of the shared case list (the project's
rule: plain float32 must stay within a quarter of the tolerance); every named mutant of the three operations must miss a tolerance on
some case; a case list that cannot show a mutant is rejected; the cell models agree with the oracle's LSTM cell and with float64
autograd; and the route the launchers of ast_amd/csrc/rowgemm.hip must take is tabulated for the case list."""
import numpy as np
import pytest
import torch

import row_panel_model as RP

CU = 256


def _smallest_125(x):
    """the smallest value of the form {1, 2, 5} x 10^k that is >= x."""
    k = int(np.floor(np.log10(x)))
    for kk in (k - 1, k, k + 1):
        for d in (1, 2, 5):
            if d * 10.0 ** kk >= x:
                return float(f"{d}e{kk}")
    raise AssertionError(x)


@pytest.fixture(scope="module")
def case_list():
    return RP.cases(CU)


@pytest.fixture(scope="module")
def float32_figures(case_list):
    """{quantity: worst float32-model error over the case list}, the K sum in index order and in the kernel's wave split."""
    worst = {q: 0.0 for q in RP.TOL}
    for c in case_list:
        ref = c.run()
        for waves in (None, c.waves(CU)):
            for got, want in zip(c.run(np.float32, waves), ref):
                assert got.keys() == want.keys()
                for q in want:
                    worst[q] = max(worst[q], RP.relerr(got[q], want[q]))
    return worst


def test_tolerances_are_the_quarter_rule_applied_to_the_float32_model(float32_figures):
    """Each constant of row_panel_model.TOL is the smallest {1, 2, 5} x 10^k that leaves the float32 evaluation within a quarter of it."""
    print({q: f"{e:.2e}" for q, e in float32_figures.items()})
    for q, e in float32_figures.items():
        assert e <= RP.TOL[q] / 4, (q, e, RP.TOL[q])
        assert RP.TOL[q] == _smallest_125(4 * e), (q, e, RP.TOL[q], _smallest_125(4 * e))


def _misses(c, mutant):
    return any(RP.relerr(got[q], want[q]) > RP.TOL[q] for got, want in zip(c.run(mutant=mutant), c.run()) for q in want)


@pytest.mark.parametrize("mutant", list(RP.MUTANTS))
def test_every_mutant_misses_a_tolerance_on_a_case_of_the_list(case_list, mutant):
    """A wrong kernel must not pass: each mutant, evaluated in float64, is outside a tolerance on a case -- and on EVERY case of the
    list that has the inputs the mutant mishandles and more than one element, so no such case is a wasted launch."""
    kind, needs = RP.MUTANTS[mutant]
    able = [c for c in case_list if c.kind == kind and needs(c.spec) and c.spec.get("N", 2) * c.spec.get("B", 2) * c.spec.get("h", 2) > 4
            and not c.spec.get("saturate")]
    hits = [c for c in able if _misses(c, mutant)]
    assert hits, f"{mutant} passes every case: the cases are too weak"
    assert len(hits) == len(able), (mutant, [c.name for c in able if c not in hits][:5])
    others = [c for c in case_list if c.kind == kind and not needs(c.spec)]
    assert not any(_misses(c, mutant) for c in others[:20]), "the mutant shows where it should not: its precondition is misstated"


def test_a_case_list_that_cannot_show_a_mutant_is_rejected(case_list):
    assert RP.case_list_problems(case_list, CU) == []
    rg = [c for c in case_list if c.kind == "rowgemm"]
    no_carry = [c for c in case_list if not (c.kind == "rowgemm" and c.spec["carry_col0"] is not None)]
    assert any("carry_from_col0_plus_1" in p for p in RP.case_list_problems(no_carry, CU))
    beyond = no_carry + [RP._rg("x", "beyond", 5, 7, (12,), carry_col0=7)]
    assert any("outside [0, N)" in p for p in RP.case_list_problems(beyond, CU))
    zero_old = RP._rg("x", "zero-old", 5, 7, (12,), carry_col0=4)
    zero_old.inputs()[0]["carry"][:] = 0
    assert any("old carry" in p for p in RP.case_list_problems(case_list + [zero_old], CU))
    flat_aux = RP._rg("x", "flat-aux", 5, 7, (12,), carry_col0=4)
    flat_aux.inputs()[0]["aux"][:] = 0
    assert any("aux" in p for p in RP.case_list_problems(case_list + [flat_aux], CU))
    unmasked = [c for c in case_list if not (c.kind == "bwd" and c.spec["mask"])]
    assert {"mask_on_dh_rec", "dh_add_masked", "pair1_into_dh_rec"} <= {p.split()[1].rstrip(":") for p in RP.case_list_problems(unmasked, CU)
                                                                       if p.startswith("mutant")}
    ones = RP._bw("x", "ones", 5, 6, (24,))
    ones.inputs()[0]["mask"][:] = 1
    assert any("mask without both values" in p for p in RP.case_list_problems(case_list + [ones], CU))
    assert any("rowgemm<2, 8>" in p for p in RP.case_list_problems([c for c in case_list if c.group != "rg-two-tiles"], CU))
    assert len(rg) >= 225


def test_forward_cell_model_agrees_with_the_oracle_lstm_cell():
    """oracle/minichainer.py's F.lstm on the model's pre-activation: the same c and h, and the model's gates are its a, i, f, o."""
    from oracle import minichainer as F
    c = RP._fw("x", "oracle", 5, 6, (8, 20), mask=False)
    inp = c.inputs()[0]
    got = c.run()[0]
    z = sum(A.astype(np.float64) @ W.astype(np.float64).T for A, W in inp["pairs"]) + inp["zx"] + inp["bias"][None, :]
    fn = F._LSTM()
    c_ref, h_ref = fn.forward((inp["c_prev"].astype(np.float64), z))
    assert np.abs(got["c"] - c_ref).max() < 1e-14 and np.abs(got["h"] - h_ref).max() < 1e-14
    g = got["gates"].reshape(5, 6, 4)
    for k, ref in enumerate((fn.a, fn.i, fn.f, fn.o)):
        assert np.abs(g[:, :, k] - ref).max() < 1e-14
    assert np.array_equal(got["hd"], got["h"])


def test_backward_cell_model_agrees_with_float64_autograd_of_the_forward_model():
    """One cell inside the chain the backward kernel serves: h feeds the same layer's next step through Wl (pair 0, unmasked), and -- as
    the dropped output h * mask -- the layer above through Wu (pair 1) and two further consumers (dy, dy2); d_hT reaches h unmasked
    (dh_add); c feeds the next step (dc_next).  torch float64 autograd of that graph gives dz and dc_prev."""
    B, h, Ka = 5, 6, 12
    c = RP._bw("x", "autograd", B, h, (4 * h, Ka))
    inp = c.inputs()[0]
    t = lambda a, grad=False: torch.tensor(np.asarray(a, np.float64), requires_grad=grad)
    fw = RP._fw("x", "autograd", B, h, (8,), mask=False).inputs()[0]
    z = t(sum(A.astype(np.float64) @ W.astype(np.float64).T for A, W in fw["pairs"]) + fw["zx"], True)
    c_prev = t(fw["c_prev"], True)
    r = z.reshape(B, h, 4)
    a, i, f, o = torch.tanh(r[:, :, 0]), torch.sigmoid(r[:, :, 1]), torch.sigmoid(r[:, :, 2]), torch.sigmoid(r[:, :, 3])
    cc = a * i + f * c_prev
    hh = o * torch.tanh(cc)
    mask = t(inp["mask"])
    (dz_next, WlT), (dz_above, WuT) = inp["pairs"]
    hd = hh * mask
    # a scalar whose gradient wrt each consumer is the upstream quantity the kernel is handed
    loss = ((hh @ t(WlT)) * t(dz_next)).sum() + ((hd @ t(WuT)) * t(dz_above)).sum() + (hd * t(inp["dy"])).sum() + (hd * t(inp["dy2"])).sum() \
        + (hh * t(inp["dh_add"])).sum() + (cc * t(inp["dc_next"])).sum()
    dz_ref, dc_prev_ref = torch.autograd.grad(loss, (z, c_prev))
    model_in = dict(inp, c_prev=c_prev.detach().numpy(), c_cur=cc.detach().numpy(),
                    gates=torch.stack([a, i, f, o], dim=2).reshape(B, 4 * h).detach().numpy())
    got = RP.cell_bwd({k: (v.astype(np.float64) if isinstance(v, np.ndarray) else v) for k, v in model_in.items()})
    assert RP.relerr(got["dz"], dz_ref.numpy()) < 1e-12 and RP.relerr(got["dc_prev"], dc_prev_ref.numpy()) < 1e-12


def test_route_table_of_the_case_list(case_list):
    """The launchers' one decision, restated (row_panel_model.route) and tabulated: worked rows at 256 compute units, every one of the
    twelve instantiations taken by some case, and each kernel keyed on its own K."""
    rg = lambda M, N, Ks, longk=None: RP.route("rowgemm", dict(M=M, N=N, Ks=Ks, longk=longk), CU)
    assert rg(17, 4096, (4,)) == [1, 256, 1, 1] and rg(32, 4096, (20,), 4) == [3, 256, 1, 1]
    assert rg(32, 4080, (4,)) == [0, 255, 2, 1]                    # one column tile short of the chip: two workgroups per column tile
    assert rg(33, 2048, (4,)) == [1, 128, 2, 1] and rg(64, 2048, (4,)) == [1, 128, 2, 1] and rg(16, 8192, (4,)) == [0, 512, 1, 1]
    assert rg(5, 7, (2044,)) == [0, 1, 1, 1] and rg(5, 7, (2048,)) == [2, 1, 1, 1] and rg(5, 7, (1024, 1028)) == [2, 1, 1, 1]
    assert rg(5, 7, (4096,), 0) == [0, 1, 1, 1]                    # 0 = never
    cell = lambda kind, B, h, Ks, n, longk=None: RP.route(kind, dict(B=B, h=h, Ks=Ks, ncells=n, longk=longk), CU)
    assert cell("fwd", 17, 128, (20, 12), 8) == [1, 32, 1, 8] and cell("fwd", 17, 124, (20, 12), 8) == [0, 31, 2, 8]
    assert cell("bwd", 17, 512, (20, 36), 8) == [1, 32, 1, 8] and cell("bwd", 17, 496, (20, 36), 8) == [0, 31, 2, 8]
    assert cell("fwd", 5, 6, (1024, 1028), 1) == [2, 2, 1, 1] and cell("bwd", 5, 6, (1024, 1028), 1) == [0, 1, 1, 1]     # sum against maximum
    table = {}
    for c in case_list:
        table.setdefault(RP.instantiation(c.kind, c.spec, CU), []).append(c.name)
    print({k: len(v) for k, v in sorted(table.items())})
    assert set(table) == {(k, mt, nw) for k in RP.OPS for mt in (1, 2) for nw in (4, 8)}
    # the other chip sizes the two-row-tile shapes are stated for: the decision still falls on both sides
    for cu in (64, 104, 304):
        seen = {RP.instantiation(c.kind, c.spec, cu) for c in RP.cases(cu) if "two-tiles" in c.group}
        assert {(k, mt) for k, mt, _ in seen} == {(k, mt) for k in RP.OPS for mt in (1, 2)}, cu
