"""Host tests of the CTC forced alignment: the NumPy model of tests/ctc_align_model.py against a brute-force
maximum over all valid alignments, its paths against the labels, the loss model and the planted / tie-rule cases, the float32 figures
the operator's bounds are taken from, and the host logic: the input-frame formula, the argument checks, the .npz keys, the ABI mirror
and the descriptor refusals."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import ctc_align_model as AM
import ctc_model as CM
from conftest import ROOT, tiny_cfg

_RUNS = {}


def _run(name, dtype):
    """The model's result on one case in one dtype, computed once and shared."""
    key = (name, np.dtype(dtype).name)
    if key not in _RUNS:
        x, y, lens = AM.case(name)
        _RUNS[key] = AM.align(x.astype(dtype), y, lens, dtype=dtype)
    return _RUNS[key]


def _rows(name):
    """(b, n, labels, float64 emissions) of every feasible row of a case."""
    x, y, lens = AM.case(name)
    B, T, V = x.shape
    for b in range(B):
        n = T if lens is None else int(np.clip(lens[b], 0, T))
        labels = CM.labels_of(y[b], CM.UNK_ID, V)
        if CM.feasible(labels, n):
            yield b, n, labels, AM.emissions(x[b, :n].astype(np.float64), labels, CM.PAD_ID)


# ------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("T,labels", [(1, []), (1, [4]), (2, [4]), (3, [4, 4]), (4, [3, 4]), (5, [4, 4]), (6, [3, 4]), (6, [3, 3]), (6, [5]), (4, [])],
                         ids=repr)
def test_model_score_is_the_brute_force_maximum(T, labels):
    """Tiny rows: the float64 score equals the largest rescored log-probability over ALL valid alignments, the path attains it, and the
    number of valid alignments is what the loss's recursion counts (all emissions 0: alpha counts paths)."""
    rng = np.random.default_rng(7 * T + len(labels))
    x = rng.standard_normal((T, 6))
    z, skip = AM.extended(labels, CM.PAD_ID)
    e = AM.emissions(x, labels, CM.PAD_ID)
    score, path = AM.viterbi(e, skip)
    valid = [p for p in itertools.product(range(len(z)), repeat=T) if AM.is_valid_path(list(p), labels, CM.PAD_ID)]
    assert valid and AM.is_valid_path(list(path), labels, CM.PAD_ID)
    best = max(AM.rescore(e, np.asarray(p)) for p in valid)
    assert abs(score - best) <= 1e-12 and abs(AM.rescore(e, path) - best) <= 1e-12
    nll, _ = CM.ctc_row(np.zeros((T, 6)), labels, CM.PAD_ID)               # p = (number of paths) * 6^-T
    assert round(float(np.exp(-nll) * 6.0 ** T)) == len(valid)


@pytest.mark.parametrize("name", AM.ALL_CASES)
def test_model_paths_are_valid_collapse_to_the_labels_and_stay_below_the_full_sum(name):
    """Every feasible row, both dtypes: a legal path whose classes collapse to the labels, spans that tile the label states, label_logp
    summing to the score with the blanks' emissions, row_score <= -row_nll of the loss model; infeasible rows and the frames behind
    input_len exactly as defined."""
    x, y, lens = AM.case(name)
    B, T, V = x.shape
    seen = 0
    for dtype in (np.float64, np.float32):
        r = _run(name, dtype)
        feas = dict((b, (n, labels, e)) for b, n, labels, e in _rows(name))
        assert r["n_infeasible"] == B - len(feas)
        for b in range(B):
            if b not in feas:
                assert r["row_score"][b] == -np.inf and (r["frame_state"][b] == -1).all() and (r["frame_class"][b] == CM.PAD_ID).all()
                assert (r["label_start"][b] == -1).all() and (r["label_end"][b] == -1).all()
                continue
            n, labels, e = feas[b]
            U = len(labels)
            path = r["frame_state"][b, :n]
            assert AM.is_valid_path(list(path), labels, CM.PAD_ID)
            assert (r["frame_state"][b, n:] == -1).all() and (r["frame_class"][b, n:] == CM.PAD_ID).all()
            assert CM.collapse(r["frame_class"][b, :n]) == labels
            s0, s1 = r["label_start"][b], r["label_end"][b]
            assert (s0[U:] == -1).all() and (s1[U:] == -1).all() and (s1[:U] > s0[:U]).all() and (s0[1:U] >= s1[:max(U - 1, 0)]).all()
            for u in range(U):
                assert (path[s0[u]:s1[u]] == 2 * u + 1).all() and (path == 2 * u + 1).sum() == s1[u] - s0[u]
            nll, _ = CM.ctc_row(x[b, :n].astype(np.float64), labels, CM.PAD_ID)
            score = float(r["row_score"][b])
            assert score <= -nll + 1e-5 * max(1.0, abs(nll))
            blanks = e[np.arange(n), path][path % 2 == 0].sum()
            assert abs(r["label_logp"][b, :U].astype(np.float64).sum() + blanks - score) <= 2e-5 * max(1.0, abs(score))
            seen += 1
    assert seen


@pytest.mark.parametrize("name", AM.PLANTED_CASES + list(AM.UNIFORM_CASES))
def test_planted_and_tie_rule_paths_are_found_exactly(name):
    """Planted: the unique optimum (margin 4 per frame) in float64 and float32.  Uniform: every path scores bitwise the same in either
    dtype, and the tie rule leaves each label as early as possible, then the trailing blank."""
    x, y, lens, paths = (AM.planted_case if name in AM.PLANTED_CASES else AM.uniform_case)(name)
    for dtype in (np.float64, np.float32):
        r = _run(name, dtype)
        for b, want in enumerate(paths):
            n = len(want)
            assert n == (x.shape[1] if lens is None else int(lens[b]))
            assert np.array_equal(r["frame_state"][b, :n], want), (name, dtype, b)
    if name in AM.PLANTED_CASES:
        T, V, U = AM.PLANTED_SHAPES[AM.PLANTED_CASES.index(name)]
        labels = [CM.labels_of(y[b], CM.UNK_ID, V) for b in range(2)]
        assert [sum(a == c for a, c in zip(l[:-1], l[1:])) for l in labels] == [0, 1] and all(len(l) == U for l in labels)
        for b in range(2):                         # the planted class is the frame's maximum by exactly the margin over the runner-up
            top2 = np.sort(x[b], -1)[:, -2:]
            assert (top2[:, 1] - top2[:, 0] >= 4 - 1e-5).all()
    else:
        for b, want in enumerate(paths):           # every valid path scores the same, in both dtypes: rescoring another one
            labels = CM.labels_of(y[b], CM.UNK_ID, x.shape[2])
            other = AM.random_valid_path(labels, len(want), np.random.default_rng(b))
            for dtype in (np.float64, np.float32):
                e = AM.emissions(x[b, :len(want)].astype(dtype), labels, CM.PAD_ID, dtype)
                acc = [dtype(0), dtype(0)]
                for t in range(len(want)):
                    acc = [dtype(acc[0] + e[t, want[t]]), dtype(acc[1] + e[t, other[t]])]
                assert acc[0] == acc[1] == _run(name, dtype)["row_score"][b]


def test_float32_model_figures_are_what_the_bounds_were_taken_from():
    """The model in float32 against itself in float64, per case family: the score's relative error lies between half the recorded figure
    and 1.25 times it (NumPy's float32 exp / log differ in the last bit between builds); the deficit of the float32 path, rescored in
    float64, is the recorded 0; a label's label_logp stays within the row's absolute score figure."""
    rerr, deficit = {}, {}
    for name in AM.ALL_CASES:
        a, b = _run(name, np.float64), _run(name, np.float32)
        fam = AM.family(name)
        assert b["row_score"].dtype == np.float32 and b["label_logp"].dtype == np.float32
        assert np.isinf(a["row_score"]).tolist() == np.isinf(b["row_score"]).tolist()
        for r, n, labels, e64 in _rows(name):
            s64 = float(a["row_score"][r])
            if n == 0:
                assert s64 == 0.0 and b["row_score"][r] == 0.0
                continue
            rerr[fam] = max(rerr.get(fam, 0.0), abs(float(b["row_score"][r]) - s64) / abs(s64))
            d = AM.rescore(e64, a["frame_state"][r, :n]) - AM.rescore(e64, b["frame_state"][r, :n])
            deficit[fam] = max(deficit.get(fam, 0.0), d)
            lp = np.abs(b["label_logp"][r].astype(np.float64) - a["label_logp"][r]).max()
            assert lp <= AM.F32_SCORE_RERR[fam] * abs(s64), (name, r, lp)
    print(rerr, deficit)
    assert set(rerr) == set(AM.F32_SCORE_RERR) == set(AM.F32_DEFICIT)
    for fam, fig in AM.F32_SCORE_RERR.items():
        assert 0.5 * fig <= rerr[fam] <= 1.25 * fig, (fam, rerr[fam], fig)
        assert deficit[fam] <= AM.F32_DEFICIT[fam], (fam, deficit[fam])


def test_model_never_forms_nan_and_handles_the_empty_rows():
    """U = 0 is the all-blank path; n = 0 with U = 0 is the empty path of score 0; logits at +-30 in float32 give finite scores."""
    x = CM.op_logits("normal", 2, 4, 5, 3)
    r = AM.align(x.astype(np.float64), np.zeros((2, 3), np.int32), np.asarray([4, 0], np.int32))
    logp = x[0].astype(np.float64) - np.log(np.exp(x[0].astype(np.float64)).sum(-1, keepdims=True))
    assert abs(r["row_score"][0] - logp[:, 0].sum()) < 1e-12 and (r["frame_state"][0] == 0).all()
    assert r["row_score"][1] == 0.0 and (r["frame_state"][1] == -1).all() and r["n_infeasible"] == 0
    for kind in ("offset+", "offset-", "peaked"):
        q = AM.align(CM.op_logits(kind, 2, 9, 57, 1), np.array([[1, 7, 7, 2], [1, 9, 2, 0]], np.int32), dtype=np.float32)
        assert np.isfinite(q["row_score"]).all() and np.isfinite(q["label_logp"]).all()


# ------------------------------------------------------------------ 2. host logic
def test_input_span_is_the_receptive_field_through_the_layers():
    """Against a brute-force receptive field: mark the input frames that reach an encoder frame by running the layers' index sets."""
    from ast_amd.seq2seq import cnn_out_lens, input_span
    for layers in ([dict(ksize=[3, 3], stride=[2, 2], pad=[1, 1]), dict(ksize=[3, 3], stride=[2, 2], pad=[1, 1])],
                   [dict(ksize=[5, 3], stride=[3, 1], pad=[0, 1])], [dict(ksize=[4, 3], stride=[1, 1], pad=[2, 1]), dict(ksize=[3, 3], stride=[2, 1], pad=[0, 0])]):
        x_len = 37
        T2 = cnn_out_lens(layers, x_len)[-1]
        for a, e in ((0, 1), (0, T2), (T2 - 1, T2), (2, 5)):
            reach = set(range(a, e))
            for l in reversed(layers):
                kt, st, pt = l["ksize"][0], l["stride"][0], l["pad"][0]
                reach = {j * st - pt + k for j in reach for k in range(kt)}
            lo, hi = input_span(layers, a, e, x_len)
            assert (lo, hi) == (min(max(min(reach), 0), x_len), min(max(max(reach) + 1, 0), x_len))
            assert 0 <= lo <= hi <= x_len
        spans = [input_span(layers, j, j + 1, x_len) for j in range(T2)]
        assert all(p[0] <= q[0] and p[1] <= q[1] for p, q in zip(spans[:-1], spans[1:]))


def test_ctc_align_refuses_before_it_touches_the_library(monkeypatch):
    """A model without the head gets ctc_predict's ValueError, in front of everything else."""
    from ast_amd import _lib
    from ast_amd.seq2seq import SpeechEncoderDecoder
    m = SpeechEncoderDecoder(None, tiny_cfg())

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(m, "encode", touched)
    with pytest.raises(ValueError, match="rnn_config.ctc"):
        m.ctc_align(np.zeros((1, 16, 8), np.float32), np.array([[1, 5, 2]], np.int32))
    with pytest.raises(ValueError, match="rnn_config.ctc"):
        m.ctc_predict(np.zeros((1, 16, 8), np.float32))


def test_score_py_option_and_the_npz_keys():
    """score.py gains exactly one option, registered beside the code that serves it; a row's arrays get the documented keys."""
    import argparse
    from ast_amd import nn
    p = argparse.ArgumentParser()
    nn.add_alignment_arguments(p)
    assert vars(p.parse_args([]))["ctc_alignments"] is None
    assert vars(p.parse_args(["--ctc-alignments", "a.npz"]))["ctc_alignments"] == "a.npz"
    assert nn.write_alignment_file(None, "dev", {"ctc_alignments": None}) is None              # without the flag: nothing, not even the model
    row = dict(labels=np.array([5, 7]), segments=np.zeros((2, 2), np.int32), segments_input=np.zeros((2, 2), np.int32),
               confidence=np.ones(2, np.float32), score=-1.5, total_logp=-1.0, frame_state=np.zeros(4, np.int32))
    got = nn.ctc_alignment_arrays("utt#3", row)
    assert sorted(got) == sorted("utt#3/" + k for k in ("segments", "segments_input", "labels", "confidence", "score", "total_logp"))
    src = open(os.path.join(ROOT, "score.py")).read()
    assert "add_alignment_arguments(parser)" in src and "write_alignment_file(nn, set_key, args" in src
    assert hasattr(nn.NN, "ctc_align_set")


def test_loader_frame_counts_are_the_training_batches_x_len(tmp_path):
    import random
    from ast_amd.dataloader import SyntheticDataLoader
    data = {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 21, "syn_dev": 5}, "frames": [20, 400],
            "targets": [1, 30], "buckets_num": 4, "buckets_width": 80, "max_pred": 12, "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w"}
    dl = SyntheticDataLoader(data, str(tmp_path), -1)
    dl.keep_lens = True
    random.seed("s")
    for b in dl.get_batch(8, "syn_train", train=True, labels=True):
        got = dl.frame_counts("syn_train", b["utts"])
        assert got.dtype == np.int32 and got.tolist() == b["x_len"].tolist()


def test_symbols_are_declared_listed_and_exported():
    from ast_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "astk.h")).read()
    for lib_path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        lib = C.CDLL(lib_path)
        for n in ("astk_ctc_align_workspace_bytes", "astk_ctc_align"):
            assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.SIGNATURES
            assert isinstance(getattr(lib, n), C._CFuncPtr)
    decl = re.search(r"int astk_ctc_align\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["astk_ctc_align"][1]) == 14
    assert "const float* logits" in decl                                       # read-only by declaration
    srcs = open(os.path.join(ROOT, "ast_amd", "csrc", "build.sh")).read().split("SRCS=")[1].split("\n")[0]
    assert " ctc_align" in srcs


def test_descriptor_refusals_need_no_device():
    """The refusals of astk_ctc_loss from the descriptor alone, with null pointers and no stream; a good descriptor's workspace holds
    the back-pointers, T * ceil((2L + 1) / 64) * 16 bytes per row, the lse, and little else; null pointers and a short workspace."""
    from ast_amd import _lib
    lib = _lib.load()
    good = dict(B=2, T=4, V=7, ldv=8, L=3, ldy=3, first_label=3, blank=0)
    nul = (None,) * 10

    def call(d, ws=None, nbytes=0):
        return lib.astk_ctc_align(C.byref(d), *nul, ws, nbytes, None)
    for field, value, word in (("V", 1, "V"), ("blank", 7, "blank"), ("blank", -1, "blank"), ("first_label", 0, "first_label"), ("B", 0, "B"),
                               ("T", -1, "T"), ("L", 0, "L"), ("L", 256, "labels"), ("ldv", 6, "ldv"), ("ldy", 2, "ldy")):
        d = _lib.CtcDesc(**{**good, field: value})
        if field == "L":
            d.ldy = max(value, 1)
        assert lib.astk_ctc_align_workspace_bytes(C.byref(d)) == 0 and word in lib.astk_last_error().decode()
        assert call(d) < 0 and word in lib.astk_last_error().decode(), (field, lib.astk_last_error().decode())
        assert (lib.astk_ctc_workspace_bytes(C.byref(d)) == 0) and word in lib.astk_last_error().decode()     # the loss refuses the same
    d = _lib.CtcDesc(**good)
    d.struct_size -= 4
    assert lib.astk_ctc_align_workspace_bytes(C.byref(d)) == 0 and "struct_size" in lib.astk_last_error().decode()
    d = _lib.CtcDesc(32, 420, 8004, 8004, 177, 177, 3, 0)
    need = lib.astk_ctc_align_workspace_bytes(C.byref(d))
    floor = 32 * 420 * ((2 * 177 + 1 + 63) // 64) * 16 + 32 * 420 * 4
    assert floor < need < floor + (1 << 12)
    assert need < lib.astk_ctc_workspace_bytes(C.byref(d))                      # (a caller may share the loss's allocation)
    assert call(_lib.CtcDesc(**good)) < 0 and "null" in lib.astk_last_error().decode()
