"""Beam search on the device loop, the host side (no GPU): the tile packing planner, the backtracking that decode_beam_batch and
decode_beam_device share, the two entry points' declarations and exports, and the CPU model check of the parent-word hand-off
(tests/beam_parent_model.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from beam_parent_model import explore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_plan_one_slot_per_utterance_fills_both_tiles():
    from ast_amd.nn import plan_beam_tiles
    plan = plan_beam_tiles(40, 1)
    assert [B for B, _ in plan] == [32, 8]
    assert plan[0][1] == [(u, u) for u in range(32)]
    assert plan[1][1] == [(32 + k, k) for k in range(8)]


def test_plan_five_slots_three_utterances_per_tile():
    from ast_amd.nn import plan_beam_tiles
    plan = plan_beam_tiles(8, 5)
    # 16 // 5 = 3 utterances per tile (row 15 is padding), 6 per launch
    assert plan[0] == (31, [(0, 0), (1, 5), (2, 10), (3, 16), (4, 21), (5, 26)])
    assert plan[1] == (10, [(6, 0), (7, 5)])
    # a count that does not fill a tile, and one that ends on a tile's first utterance
    assert plan_beam_tiles(2, 5) == [(10, [(0, 0), (1, 5)])]
    assert plan_beam_tiles(4, 5) == [(21, [(0, 0), (1, 5), (2, 10), (3, 16)])]
    assert plan_beam_tiles(0, 5) == []


def test_plan_sixteen_slots_one_utterance_per_tile():
    from ast_amd.nn import plan_beam_tiles
    assert plan_beam_tiles(3, 16) == [(32, [(0, 0), (1, 16)]), (16, [(2, 0)])]


@pytest.mark.parametrize("N", [1, 2, 3, 5, 7, 8, 9, 16])
def test_plan_keeps_an_utterance_inside_one_tile(N):
    from ast_amd.nn import plan_beam_tiles
    seen = []
    for B, rows in plan_beam_tiles(23, N):
        assert 1 <= B <= 32 and B == rows[-1][1] + N
        for u, r0 in rows:
            assert r0 // 16 == (r0 + N - 1) // 16 and (r0 % 16) % N == 0
            seen.append(u)
        firsts = [r0 for _, r0 in rows]
        assert all(b - a >= N for a, b in zip(firsts, firsts[1:]))
    assert seen == list(range(23))


def test_plan_refuses_seventeen_slots():
    from ast_amd.nn import plan_beam_tiles
    with pytest.raises(ValueError, match="N = 17"):
        plan_beam_tiles(4, 17)
    with pytest.raises(ValueError, match="N = 0"):
        plan_beam_tiles(4, 0)


# ---------------------------------------------------------------------------------------------------------------- backtracking
def test_backtracking_follows_parents_and_skips_carried_steps():
    from ast_amd.nn import backtrack_beam_history
    # N = 3, four steps.  (parent slot, token, carried, 0) per step and new slot; EOS = 2
    hist = np.array([
        [[0, 7, 0, 0], [0, 5, 0, 0], [0, 9, 0, 0]],        # step 0: slot 0 expands into 7, 5, 9
        [[1, 2, 0, 0], [0, 4, 0, 0], [2, 6, 0, 0]],        # step 1: 5 -> EOS (finished), 7 -> 4, 9 -> 6
        [[0, 2, 1, 0], [2, 8, 0, 0], [1, 2, 0, 0]],        # step 2: slot 0 carried; 9 6 -> 8; 7 4 -> EOS
        [[1, 3, 0, 0], [0, 2, 1, 0], [2, 2, 1, 0]],        # step 3: 9 6 8 -> 3 now ranks first; both finished slots carried, moved down
    ], dtype=np.int32)
    got = backtrack_beam_history(hist, np.array([1, 2, 2]))
    assert [(i, toks) for i, toks, _ in got] == [(0, [9, 6, 8, 3]), (1, [5, 2]), (2, [7, 4, 2])]
    # the trace names, per token, the step, the slot that received it and the parent slot it was expanded from
    assert got[0][2] == [(0, 2, 0), (1, 2, 2), (2, 1, 2), (3, 0, 1)]
    assert got[1][2] == [(0, 1, 0), (1, 0, 1)]
    assert got[2][2] == [(0, 0, 0), (1, 1, 0), (2, 2, 1)]


def test_backtracking_stops_at_the_first_empty_slot_and_takes_no_steps():
    from ast_amd.nn import backtrack_beam_history
    hist = np.array([[[0, 4, 0, 0], [0, 3, 0, 0], [-1, 0, 0, 0]]], dtype=np.int32)
    got = backtrack_beam_history(hist, np.array([1, 1, 0]))
    assert [(i, toks) for i, toks, _ in got] == [(0, [4]), (1, [3])]
    assert backtrack_beam_history(hist[:0], np.array([1, 0, 0])) == [(0, [], [])]


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_listed_and_exported():
    from ast_amd import _lib
    text = open(os.path.join(ROOT, "include", "astk.h")).read()
    for name in ("astk_beam_decode_workspace_bytes", "astk_beam_decode"):
        assert name + "(" in text, name
        assert name in _lib.SIGNATURES, name
        for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
            assert hasattr(C.CDLL(path), name), (path, name)
    assert len(_lib.SIGNATURES["astk_beam_decode"][1]) == 23
    assert _lib.SIGNATURES["astk_beam_decode_workspace_bytes"][0] is C.c_size_t


def test_workspace_query_returns_zero_for_bad_arguments():
    """No GPU is touched: the query is arithmetic on the descriptor."""
    from ast_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    lib.astk_beam_decode_workspace_bytes.restype = C.c_size_t
    lib.astk_beam_decode_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    assert lib.astk_beam_decode_workspace_bytes(None, 5, 5, 12, 1) == 0
    dd = _lib.DecoderDesc()
    dd.struct_size = 1          # a wrong size: refused before any field is read
    assert lib.astk_beam_decode_workspace_bytes(C.byref(dd), 5, 5, 12, 1) == 0


# ---------------------------------------------------------------------------------------------------------------- the model check
@pytest.mark.parametrize("layers", [1, 2, 3])
def test_no_cell_reads_an_unwritten_parent_word(layers):
    violations, n_states = explore(steps=3, layers=layers)
    assert not violations, violations
    assert n_states > 20


def test_top_layer_cell_without_its_wait_is_flagged():
    violations, _ = explore(steps=3, layers=3, top_no_wait=True)
    assert "unwritten_parent" in violations, violations
    assert "deadlock" not in violations


def test_parent_word_written_behind_the_arrival_is_flagged():
    for layers in (1, 3):
        violations, _ = explore(steps=3, layers=layers, late_parent=True)
        assert "unwritten_parent" in violations, (layers, violations)
