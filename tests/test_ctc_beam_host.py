"""Host tests of the CTC prefix beam search: the NumPy model of tests/ctc_beam_model.py against brute force and
the CTC loss model where the search is exhaustive, the lower bound everywhere, the guard that lets the GPU test demand exact equality
(every named case's smallest non-zero gap), the coverage the named cases were chosen for, and the refusals that need no GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ctc_beam_model as BM
import ctc_model as CM
from conftest import tiny_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _log_p_ctc(x, labels):
    nll, _ = CM.ctc_row(np.asarray(x, np.float64), list(labels), BM.PAD_ID)
    return -float(nll)


@pytest.mark.parametrize("T", [1, 2, 3])
def test_exhaustive_search_equals_brute_force(T):
    """T <= 3, V = 5 (two labels), N = 16, C = 2: every label string fits the beam, so nothing is pruned -- every score is
    log p_ctc(labels) (ctc_model.ctc_row) to 1e-10 and the ranking is brute force's over all alignments."""
    for seed in range(4):
        x = np.random.default_rng(900 + 10 * T + seed).standard_normal((T, 5)).astype(np.float32)
        beam, st = BM.search_row(x, 16, 2, T)
        want = BM.brute_force(x)
        assert {l for l, _, _, _ in beam} == set(want) and len(beam) <= 16
        for l, s, _, _ in beam:
            assert abs(s - want[l]) <= 1e-10 and abs(s - _log_p_ctc(x, l)) <= 1e-10, (l, s, want[l])
        ranked = sorted(want.items(), key=lambda kv: -kv[1])
        assert min(a[1] - b[1] for a, b in zip(ranked[:-1], ranked[1:])) > 1e-9                 # (no tie to break among the strings)
        assert [l for l, _, _, _ in beam] == [l for l, _ in ranked]


@pytest.mark.parametrize("name", BM.ALL_CASES)
def test_scores_are_lower_bounds_of_the_full_sum(name):
    c, r = BM.result(name)
    B, T, _ = c["logits"].shape
    for b in range(B):
        n = T if c["lens"] is None else int(np.clip(c["lens"][b], 0, T))
        for k in range(c["N"]):
            u = r["n_labels"][b, k]
            if u < 0:
                assert r["score"][b, k] == -math.inf and (r["tokens"][b, k] == BM.PAD_ID).all()
                continue
            labels = r["tokens"][b, k, :u].tolist()
            assert all(l >= BM.UNK_ID for l in labels) and (r["tokens"][b, k, u:] == BM.PAD_ID).all() and u <= c["max_labels"]
            assert r["score"][b, k] <= _log_p_ctc(c["logits"][b, :n], labels) + 1e-9, (name, b, k)
        live = r["score"][b][r["n_labels"][b] >= 0]
        assert len(live) >= 1 and (np.diff(live) <= 0).all()                                     # rank order
        strings = [tuple(r["tokens"][b, k, :r["n_labels"][b, k]]) for k in range(len(live))]
        assert len(set(strings)) == len(strings)                                                # distinct prefixes
        if n == 0:
            assert r["n_labels"][b].tolist() == [0] + [-1] * (c["N"] - 1) and r["score"][b, 0] == 0.0


@pytest.mark.parametrize("name", BM.ALL_CASES)
def test_the_guard_every_named_case_has_a_gap_of_1e_7(name):
    """The condition of the GPU test's exact equality: no two candidates adjacent in rank at or above the cut closer than 1e-7 (and
    not equal), in any frame of any row.  1e-7 is three orders above the operator's score tolerance."""
    _, r = BM.result(name)
    gaps = [st["min_gap"] for st in r["stats"]]
    print(name, "smallest non-zero gap", min(gaps))
    assert min(gaps) >= 1e-7


def test_the_named_cases_cover_what_they_were_chosen_for():
    stats = {name: BM.result(name)[1]["stats"] for name in BM.ALL_CASES}
    for name in ("small-v", "blank-biased"):
        assert sum(st["merges"] for st in stats[name]) > 0, name
    assert sum(st["merges"] for st in stats["small-v"]) > 100
    assert any(st["reentry_live_descendant"] for sts in stats.values() for st in sts)
    assert any(st["reentries"] > 0 for st in stats["small-v"])
    c, r = BM.result("cap")
    assert (r["n_labels"] == c["max_labels"]).any() and r["n_labels"].max() == c["max_labels"] == 3
    for name in ("twin-columns", "twin-columns-odd"):
        assert sum(st["cut_ties"] for st in stats[name]) > 0, name
    assert BM.case("c-lt-stay")["C"] == 1 and all(st["stay_outside"] > 0 for st in stats["c-lt-stay"][:2])
    lens = [BM.case(n)["lens"] for n in BM.ALL_CASES if BM.case(n)["lens"] is not None]
    assert any(0 in l for l in lens) and any(1 in l for l in lens)
    assert BM.case("ldv")["logits"].shape[2] == 1098 and BM.case("long")["logits"].shape[:2] == (3, 300)


def test_model_pieces():
    assert BM.logaddexp(-math.inf, -math.inf) == -math.inf and BM.logaddexp(-math.inf, -2.0) == -2.0
    assert BM.logaddexp(-1.0, -3.0) == BM.logaddexp(-3.0, -1.0) and abs(BM.logaddexp(0.0, 0.0) - math.log(2)) < 1e-15
    xt = np.asarray([9.0, 9.0, 9.0, 1.0, 2.0, 2.0, 0.5])
    assert BM.proposals(xt, 3, 3) == [4, 5, 3]                                                  # equal values: the lower id first


# ------------------------------------------------------------------ the Python layer and the library without a GPU
def test_ctc_beam_refuses_before_it_touches_the_library(monkeypatch):
    from ast_amd import _lib
    from ast_amd.seq2seq import SpeechEncoderDecoder, checked_ctc_beam_width
    m = SpeechEncoderDecoder(None, tiny_cfg())

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(m, "encode", touched)
    with pytest.raises(ValueError, match="rnn_config.ctc"):
        m.ctc_beam(np.zeros((1, 16, 8), np.float32))
    cfg = tiny_cfg()
    cfg["rnn_config"]["ctc"] = True
    h = SpeechEncoderDecoder(None, cfg)
    monkeypatch.setattr(h, "encode", touched)
    X = np.zeros((1, 16, 8), np.float32)
    for kw in (dict(N=0), dict(N=17), dict(C=0), dict(C=17), dict(N=2.5), dict(C=True), dict(max_labels=0), dict(max_labels=256)):
        with pytest.raises(ValueError, match="ctc_beam"):
            h.ctc_beam(X, **kw)
    assert checked_ctc_beam_width(16, 16) == (16, 16) and checked_ctc_beam_width(np.int64(3), 2, V=5) == (3, 2)
    with pytest.raises(ValueError, match="1..2"):
        checked_ctc_beam_width(4, 3, V=5)                                                       # C above V - first_label


def test_rescore_refuses_bad_arguments_and_nn_has_the_set_method():
    from ast_amd import nn
    assert hasattr(nn.NN, "ctc_beam_set")
    for w in (-0.1, 1.5):
        with pytest.raises(ValueError, match="weight"):
            nn.rescore_ctc_nbest(None, [], [], w)
    with pytest.raises(ValueError, match="n-best"):
        nn.rescore_ctc_nbest(None, [None], [], 0.5)


def test_ctc_decode_command_line():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ctc_decode_cli", os.path.join(ROOT, "ctc_decode.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                                                # (no main: nothing runs)
    a = vars(mod.build_parser().parse_args(["-m", "d", "-s", "dev", "-n", "5", "-c", "4"]))
    assert (a["N"], a["C"], a["rescore"], a["batch"], a["out"], a["batch_encode"]) == (5, 4, None, 1, None, False)
    a = vars(mod.build_parser().parse_args(["-m", "d", "-s", "dev", "-n", "5", "-c", "4", "--rescore", "0.3", "-b", "8", "-w", "o.p", "--batch-encode"]))
    assert (a["rescore"], a["batch"], a["out"], a["batch_encode"]) == (0.3, 8, "o.p", True)
    assert mod.default_name("dev", 5, 4) == "dev_ctc_N-5_C-4.p" and mod.default_name("dev", 5, 4, 0.3) == "dev_ctc_N-5_C-4_W-0.30.p"
    for f in ("beam.py", "score.py", "sample.py"):                                              # the other command lines are as they were
        assert "ctc_beam" not in open(os.path.join(ROOT, f)).read()


def test_symbols_are_declared_listed_and_exported():
    from ast_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "astk.h")).read()
    for lib_path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        lib = C.CDLL(lib_path)
        for n in ("astk_ctc_beam_workspace_bytes", "astk_ctc_beam"):
            assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.SIGNATURES
            assert isinstance(getattr(lib, n), C._CFuncPtr)
    decl = re.search(r"int astk_ctc_beam\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["astk_ctc_beam"][1]) == 9
    assert "const float* logits" in decl                                       # read-only by declaration
    fields = re.search(r"typedef struct \{([^}]*)\} astk_ctc_beam_desc;", hdr).group(1)
    names = re.findall(r"\b(struct_size|B|T|V|ldv|N|C|max_labels|first_label|blank)\b\s*[,;]", fields)
    assert names == [f[0] for f in _lib.CtcBeamDesc._fields_]
    srcs = open(os.path.join(ROOT, "ast_amd", "csrc", "build.sh")).read().split("SRCS=")[1].split("\n")[0]
    assert " ctc_beam" in srcs
    assert (_lib.CTC_BEAM_MAX_N, _lib.CTC_BEAM_MAX_C, _lib.CTC_BEAM_MAX_T) == (16, 16, _lib.BEAM_CTC_MAX_T)


GOOD = dict(B=2, T=4, V=7, ldv=8, N=3, C=2, max_labels=4, first_label=3, blank=0)
REFUSALS = (("B", 0, "B"), ("T", 0, "T"), ("T", 2049, "T"), ("V", 3, "V"), ("ldv", 6, "ldv"), ("blank", 7, "blank"), ("blank", -1, "blank"),
            ("blank", 3, "blank"), ("N", 0, "N"), ("N", 17, "N"), ("C", 0, "C"), ("C", 17, "C"), ("C", 5, "C"), ("max_labels", 0, "max_labels"),
            ("max_labels", 256, "max_labels"))


def test_descriptor_refusals_need_no_device():
    """Every refusal from the descriptor alone, with null pointers and no stream; the query returns 0 for each; the good descriptor's
    workspace is the frames' records and the tries and little else; null pointers and a short workspace."""
    from ast_amd import _lib
    lib = _lib.load()

    def call(d, ws=None, nbytes=0):
        return lib.astk_ctc_beam(C.byref(d), None, None, None, None, None, ws, nbytes, None)
    for field, value, word in REFUSALS:
        d = _lib.CtcBeamDesc(**{**GOOD, field: value})
        if field == "V":
            d.ldv = value
        assert lib.astk_ctc_beam_workspace_bytes(C.byref(d)) == 0 and word in lib.astk_last_error().decode(), (field, value)
        assert call(d) < 0 and word in lib.astk_last_error().decode(), (field, lib.astk_last_error().decode())
        assert "ASTK_" not in lib.astk_last_error().decode()
    d = _lib.CtcBeamDesc(**GOOD)
    d.struct_size -= 4
    assert lib.astk_ctc_beam_workspace_bytes(C.byref(d)) == 0 and "struct_size" in lib.astk_last_error().decode()
    assert call(d) < 0 and "struct_size" in lib.astk_last_error().decode()
    d = _lib.CtcBeamDesc(32, 200, 1098, 1100, 5, 5, 200, 3, 0)
    need = lib.astk_ctc_beam_workspace_bytes(C.byref(d))
    floor = 32 * 200 * (16 + 12 * 5) + 32 * 2048 * 8                           # 2 (T N + 1) = 2002 entries: 2048
    assert floor <= need < floor + (1 << 12)
    assert call(_lib.CtcBeamDesc(**GOOD)) < 0 and "null" in lib.astk_last_error().decode()
