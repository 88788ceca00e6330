"""Per-row source lengths in the on-device decode modes, the host side (no GPU): the four *_rows entry points are declared, listed and
exported; the packing planner of ast_amd.nn; what a RowBatch refuses."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"astk_greedy_decode_rows": "astk_greedy_decode", "astk_greedy_decode_scored_rows": "astk_greedy_decode_scored",
         "astk_sample_decode_rows": "astk_sample_decode", "astk_forced_score_rows": "astk_forced_score"}


def _params(text, name):
    m = re.search(r"int " + name + r"\((.*?)\);", text, re.S)
    assert m, name
    return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]


def test_rows_entry_points_are_declared_listed_and_exported():
    from ast_amd import _lib
    text = open(os.path.join(ROOT, "include", "astk.h")).read()
    libs = [C.CDLL(_lib.LIB_PATH), C.CDLL(_lib.TEST_LIB_PATH)]
    for rows, plain in PAIRS.items():
        # the header: the counterpart's parameters, then the lengths
        assert _params(text, rows) == _params(text, plain) + ["const int32_t* row_len"], rows
        res, args = _lib.SIGNATURES[rows]
        pres, pargs = _lib.SIGNATURES[plain]
        assert res is pres is C.c_int and args == pargs + [C.c_void_p], rows
        assert len(args) == len(_params(text, rows))
        for lib in libs:
            assert hasattr(lib, rows), (rows, lib._name)
    lib = _lib.load()
    for rows in PAIRS:
        assert getattr(lib, rows).argtypes == _lib.SIGNATURES[rows][1]


def test_planner_keeps_order_and_fills_calls():
    from ast_amd.nn import plan_row_packs
    assert plan_row_packs([]) == [] and plan_row_packs([0, 0]) == []
    assert plan_row_packs([5, 5, 5, 5]) == [[(0, 0, 5), (1, 0, 5), (2, 0, 5), (3, 0, 5)]]
    # U = 1: one utterance per call, today's path
    assert plan_row_packs([5, 0, 3], max_utts=1) == [[(0, 0, 5)], [(2, 0, 3)]]
    # an utterance of 40 rows splits 32 + 8, and the remainder shares its call with what follows
    assert plan_row_packs([40]) == [[(0, 0, 32)], [(0, 32, 40)]]
    assert plan_row_packs([5, 40, 3]) == [[(0, 0, 5)], [(1, 0, 32)], [(1, 32, 40), (2, 0, 3)]]
    # an utterance that fits a call is not split
    assert plan_row_packs([20, 20]) == [[(0, 0, 20)], [(1, 0, 20)]]
    assert plan_row_packs([5] * 8, max_utts=6) == [[(u, 0, 5) for u in range(6)], [(6, 0, 5), (7, 0, 5)]]
    rng = np.random.default_rng(0)
    for _ in range(200):
        counts = rng.integers(0, 70, size=int(rng.integers(0, 12))).tolist()
        U = int(rng.integers(1, 9))
        calls = plan_row_packs(counts, max_utts=U)
        flat = [p for call in calls for p in call]
        assert all(1 <= sum(hi - lo for _, lo, hi in call) <= 32 and 1 <= len(call) <= U for call in calls)
        assert flat == sorted(flat)                                    # order kept
        got = [0] * len(counts)
        for u, lo, hi in flat:
            assert lo == got[u] and hi > lo                            # contiguous pieces, nothing twice
            got[u] = hi
        assert got == counts
        assert all(sum(1 for p in flat if p[0] == u) == -(-n // 32) for u, n in enumerate(counts))    # split only above 32 rows
    with pytest.raises(ValueError):
        plan_row_packs([3], max_utts=0)
    with pytest.raises(ValueError):
        plan_row_packs([-1])


def test_row_batch_refuses_bad_lengths_and_shapes():
    from ast_amd.seq2seq import RowBatch
    enc, c0 = torch.zeros(3, 7, 8), torch.zeros(2, 3, 8)
    rb = RowBatch(enc, [7, 1, 4], c0, c0)
    assert rb.B == 3 and rb.T == 7 and rb.lens.dtype == np.int32 and rb.lens.tolist() == [7, 1, 4]
    assert RowBatch(enc, np.array([7, 1, 4], dtype=np.int64), c0, c0).lens.tolist() == [7, 1, 4]
    assert RowBatch(enc, torch.tensor([1, 2, 3]), c0, c0).lens.tolist() == [1, 2, 3]
    one = rb.row(2)
    assert one.B == 1 and one.T == 4 and one.lens.tolist() == [4] and tuple(one.c0.shape) == (2, 1, 8)
    for lens in ([0, 1, 1], [7, 8, 1], [7, 7], [7, 7, 7, 7], [7.0, 1.0, 4.0], np.array([7, 1, 4], dtype=np.float32), torch.tensor([1.0, 2.0, 3.0]),
                 [[7, 1, 4]]):
        with pytest.raises(ValueError, match="RowBatch"):
            RowBatch(enc, lens, c0, c0)
    with pytest.raises(ValueError, match="RowBatch"):
        RowBatch(torch.zeros(3, 7), [7, 1, 4], c0, c0)
    with pytest.raises(ValueError, match="RowBatch"):
        RowBatch(enc, [7, 1, 4], torch.zeros(2, 4, 8), c0)
    with pytest.raises(ValueError, match="RowBatch"):
        RowBatch(enc, [7, 1, 4], c0, torch.zeros(2, 3, 9))
    with pytest.raises(ValueError, match="32"):
        RowBatch(torch.zeros(33, 7, 8), [7] * 33, torch.zeros(2, 33, 8), torch.zeros(2, 33, 8))
