"""CPU tests of the CTC prefix-score model (tests/ctc_prefix_model.py) that the GPU tests of the joint
CTC-attention beam search compare against: brute force over all alignments, the CTC loss model of tests/ctc_model.py, monotonicity and
the -inf cases; and the argument checks of the Python entry points."""
import itertools
import types

import numpy as np
import pytest

import ctc_model as CM
import ctc_prefix_model as PM


def _collapse(path, blank=0):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return tuple(out)


@pytest.mark.parametrize("T,V", [(1, 2), (2, 3), (3, 4), (4, 3), (5, 4), (5, 2)])
def test_model_matches_brute_force_over_all_alignments(T, V):
    rng = np.random.default_rng(100 * T + V)
    x = PM.log_softmax64(rng.standard_normal((T, V)) * 2)
    by_string = {}
    for path in itertools.product(range(V), repeat=T):
        s = _collapse(path)
        by_string[s] = by_string.get(s, 0.0) + float(np.exp(sum(x[t, c] for t, c in enumerate(path))))
    labels = list(range(1, V))
    for n in range(4):
        for g in itertools.product(labels, repeat=n):                      # repeated labels included
            psi, r = PM.prefix_state(x, list(g), blank=0, first_label=1)
            p_prefix = sum(p for s, p in by_string.items() if s[:n] == g)
            p_exact = by_string.get(g, 0.0)
            eos, r2, n2 = PM.extend(x, r, n, g[-1] if n else -1, 99, blank=0, first_label=1, eos=99)
            assert r2 is r and n2 == n
            for got, p in ((psi, p_prefix), (eos, p_exact)):
                assert not np.isnan(got)
                if p == 0.0:
                    assert got == -np.inf, (g, got)
                else:
                    assert abs(got - np.log(p)) <= 1e-12 * max(1.0, abs(np.log(p))), (g, got, np.log(p))


def _not_above(a, b):
    return a == -np.inf or (np.isfinite(b) and a <= b + 1e-13 * max(1.0, abs(b)))


CASES = ["t1-v5", "t2-v5", "b33-ragged", "all-equal", "all-equal-one-path", "offset+", "offset-", "peaked", "u31-log-domain", "u32-ragged",
         "u255-infeasible-between"]


@pytest.mark.parametrize("name", CASES)
def test_eos_score_is_the_ctc_loss_models_log_likelihood(name):
    """psi(g.EOS) = -nll of ctc_model.ctc_row on the families short, offset, peaked and long; psi(g.c) <= psi(g) along the way; -inf
    exactly where the prefix has no path; no NaN anywhere."""
    assert CM.OP_CASES[name]["family"] in ("short", "offset", "peaked", "long")
    logits, y, lens = CM.op_case(name)
    B, T, V = logits.shape
    for b in range(B):
        n = T if lens is None else int(lens[b])
        labels = CM.labels_of(y[b], CM.UNK_ID, V)
        x = PM.log_softmax64(logits[b, :n])
        r, psi, last = PM.empty_state(x), 0.0, -1
        for k, c in enumerate(labels):
            new_psi, r, cnt = PM.extend(x, r, k, last, c)
            last = c
            assert cnt == k + 1 and not np.isnan(new_psi) and not np.isnan(r).any()
            # psi(g.c) <= psi(g): the strings that start with g.c are among those that start with g.  (Both are sums of the same
            # positive terms in another order: a float64 rounding of each, 2.2e-16 per frame over at most 64 frames, is allowed for.)
            assert _not_above(new_psi, psi), (name, b, k, new_psi, psi)
            assert (new_psi == -np.inf) == (not CM.feasible(labels[:k + 1], n)), (name, b, k)
            psi = new_psi
        eos, _, _ = PM.extend(x, r, len(labels), last, PM.EOS_ID)
        nll = float(CM.ctc_row(logits[b, :n], labels, CM.PAD_ID)[0])
        assert not np.isnan(eos)
        if np.isinf(nll):
            assert eos == -np.inf
        else:
            assert abs(eos + nll) <= 1e-10 * max(1.0, abs(nll)), (name, b, eos, -nll)
        assert _not_above(eos, psi)


def test_ids_that_are_no_label_have_no_ctc_path():
    x = PM.log_softmax64(np.random.default_rng(0).standard_normal((4, 7)))
    r = PM.empty_state(x)
    for c in (PM.PAD_ID, PM.GO_ID):
        psi, st, n = PM.extend(x, r, 0, -1, c)
        assert psi == -np.inf and np.isneginf(st).all() and n == 1
        assert PM.extend(x, st, 1, c, 5)[0] == -np.inf                  # ... and neither has anything behind it
        assert PM.extend(x, st, 1, c, PM.EOS_ID)[0] == -np.inf
    assert PM.joint_score(1.0, -np.inf, -3.0) == -np.inf                # 0 * -inf is NaN: ranked as -inf
    assert PM.joint_score(0.3, -1.0, -np.inf) == -np.inf
    assert PM.joint_score(0.3, -1.0, -2.0) == pytest.approx(-1.3, abs=1e-15)


def test_host_search_keeps_the_reference_order():
    """A two-step search by hand: proposals in candidate order, stable top-N, a finished hypothesis carried."""
    x = PM.log_softmax64(np.array([[0.0, 0, 0, 2.0, 1.0], [1.0, 0, 0, 0.5, 2.0], [2.0, 0, 0, 0.0, 0.0]]))

    def propose(ctx):
        return [(3, -0.5, ctx + 1), (4, -1.0, ctx + 1), (PM.EOS_ID, -1.5, ctx + 1)]
    got = PM.joint_beam_search(x, propose, 0, 2, 3, 0.5)
    assert len(got) == 3 and [e["score"] for e in got] == sorted((e["score"] for e in got), reverse=True)
    for e in got:
        toks = [t for t in e["hyp"][1:] if t != PM.EOS_ID]
        psi, r = PM.prefix_state(x, toks)
        if e["hyp"][-1] == PM.EOS_ID:
            psi = PM.extend(x, r, len(toks), toks[-1] if toks else -1, PM.EOS_ID)[0]
        assert e["psi"] == pytest.approx(psi, abs=1e-12) and e["score"] == pytest.approx(0.5 * e["att"] + 0.5 * psi, abs=1e-12)


def test_entry_points_check_the_weight():
    from ast_amd import _lib
    from ast_amd import nn as gnn
    head, bare = types.SimpleNamespace(ctc_head=True), types.SimpleNamespace(ctc_head=False)
    for bad in (-0.1, 1.5, float("nan"), True, "0.3"):
        with pytest.raises(ValueError, match="ctc_weight"):
            gnn.decode_beam_batch(head, [], 5, 3, 3, ctc_weight=bad)
    with pytest.raises(ValueError, match="needs the CTC head: set rnn_config.ctc = true"):
        gnn.decode_beam_batch(bare, [], 5, 3, 3, ctc_weight=0.3)
    for fn, args in ((gnn.decode_beam_device, ([], 5, 3, 3)), (gnn.decode_beam, (None, 5, 3, 3))):
        with pytest.raises(ValueError, match="decode_beam_batch"):
            fn(head, *args, ctc_weight=0.3)
    assert gnn.checked_beam_ctc_weight(head, 1) == 1.0 and gnn.checked_beam_ctc_weight(bare, 0.0) == 0.0
    import ctypes as C
    assert C.sizeof(_lib.BeamCtc) == 88 and _lib.BeamCtc(0.5).struct_size == 88 and _lib.BEAM_CTC_MAX_T == 2048
