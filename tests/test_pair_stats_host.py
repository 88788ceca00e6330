"""Host tests of the pair statistics: the model of tests/pair_stats_model.py against a textbook Levenshtein
distance and the Counter-based n-gram counts of ast_amd.eval, the identities every cell's counts obey, ast_amd.eval's own host
restatement against the model, bleu_from_counts against corpus_bleu bit for bit, the Python layer's pieces that need no GPU, and the
refusals and declarations of astk_pair_stats."""
import ctypes as C
import math
import os
import random
import re

import numpy as np
import pytest

import pair_stats_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _good_rows(name):
    c, (stats, n_bad) = PM.result(name)
    for r, (a, b) in enumerate(c["pairs"].tolist()):
        if not PM.row_is_bad(c["lens"].tolist(), c["tokens"].shape[1], a, b):
            yield c["tokens"][a, :c["lens"][a]].tolist(), c["tokens"][b, :c["lens"][b]].tolist(), stats[r].tolist()


@pytest.mark.parametrize("name", PM.ALL_CASES)
def test_model_distance_is_the_textbook_one_and_the_counts_add_up(name):
    seen = set()
    for a, b, st in _good_rows(name):
        key = (tuple(a), tuple(b))
        if key in seen:
            continue
        seen.add(key)
        dist, sub, dele, ins = st[:4]
        assert dist == PM.levenshtein(a, b), (name, len(a), len(b))
        assert sub + dele + ins == dist and dele - ins == len(b) - len(a) and min(sub, dele, ins) >= 0


@pytest.mark.parametrize("name", PM.ALL_CASES)
def test_model_matches_are_the_counter_based_counts(name):
    from ast_amd import eval as E
    seen = set()
    for a, b, st in _good_rows(name):
        key = (tuple(a), tuple(b))
        if key in seen:
            continue
        seen.add(key)
        for n in range(1, 5):
            ca, cb = E._ngrams(a, n), E._ngrams(b, n)
            assert st[3 + n] == sum((ca & cb).values()), (name, n)
            if min(len(a), len(b)) < n:
                assert st[3 + n] == 0
        assert tuple(st[4:]) == PM.clipped_matches(b, a) == E.clipped_matches(a, b)             # symmetric


def test_the_named_cases_cover_what_they_were_chosen_for():
    shapes = {(len(a), len(b)) for name in PM.ALL_CASES for a, b, _ in _good_rows(name)}
    for want in [(0, 0), (0, 1), (1, 0), (0, 512), (512, 0), (1, 1), (512, 512), (511, 512), (512, 511)]:
        assert want in shapes, want
    for la in (63, 64, 65):
        for lb in (1, 64, 65, 130):
            assert (la, lb) in shapes and (lb, la) in shapes
    assert len(PM.case("one-pair")["pairs"]) == 1 and len(PM.case("p5000")["pairs"]) == 5000
    c, (stats, n_bad) = PM.result("bad-rows")
    assert n_bad == 9 and (stats[[1, 3, 4, 5, 6, 8, 9, 11, 12]] == -1).all() and (stats[[0, 2, 7, 10, 13]] >= 0).all()
    c = PM.case("garbage")
    assert c["tokens"].shape[1] == 40 > c["lens"].max() and len(set(c["tokens"][1].tolist())) > 1
    assert {int(t) for t in PM.case("extreme-ids")["tokens"].ravel()} >= {0, -1, PM.I32_MAX, PM.I32_MIN}
    assert any(a == b for a, b in PM.case("identical")["pairs"].tolist())
    # ties: [1 2] against [2 1] costs 2 as two substitutions or as a deletion and an insertion; the diagonal is tried first
    assert PM.edit_stats([1, 2], [2, 1]) == (2, 2, 0, 0) and PM.edit_stats([1], [2, 1]) == (1, 0, 1, 0)
    assert PM.edit_stats([1, 2, 3], [1, 3]) == (1, 0, 0, 1) and PM.clipped_matches([3, 3, 3, 3], [3, 3]) == (2, 1, 0, 0)


def test_eval_host_restatement_equals_the_model():
    from ast_amd import eval as E
    rng = random.Random(5)
    for _ in range(200):
        a = [rng.randrange(3) for _ in range(rng.randrange(0, 12))]
        b = [rng.randrange(3) for _ in range(rng.randrange(0, 12))]
        assert tuple(E.edit_stats(a, b)) == PM.edit_stats(a, b), (a, b)
        assert E.pair_stats_host([a, b], [(0, 1)])[0] == list(PM.edit_stats(a, b) + PM.clipped_matches(a, b))


def test_bleu_from_counts_is_corpus_bleu_bit_for_bit():
    from ast_amd import eval as E
    rng = random.Random(6)
    pairs = [([], [1]), ([1], []), ([1], [2]), ([1], [1]), ([1, 2], [1, 2]), ([1, 2, 3], [1, 2, 3, 4]), ([1, 2, 3, 4], [4, 3, 2, 1])]
    for _ in range(500):
        V = rng.choice((2, 4, 30))
        pairs.append(([rng.randrange(V) for _ in range(rng.randrange(0, 14))], [rng.randrange(V) for _ in range(rng.randrange(0, 14))]))
    zero = short = 0
    for h, r in pairs:
        m = PM.clipped_matches(h, r)
        got, want = E.bleu_from_counts(m, len(h), len(r)), E.corpus_bleu([[r]], [h])
        assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (h, r, got, want)
        zero += m[0] == 0
        short += min(len(h), len(r)) < 4
    assert zero >= 10 and short >= 50 and len(pairs) >= 500


def test_posterior_weights_known_answers():
    from ast_amd.nn import posterior_weights
    assert posterior_weights([0.0, 0.0]) == [0.5, 0.5] and posterior_weights([-3.5], 2.0) == [1.0]
    assert posterior_weights([-1.0, -7.0, -2.5], 0.0) == [1 / 3] * 3
    w = posterior_weights([math.log(1.0), math.log(3.0)], 1.0)
    assert abs(w[0] - 0.25) < 1e-15 and abs(w[1] - 0.75) < 1e-15
    w = posterior_weights([math.log(1.0), math.log(3.0)], 2.0)
    assert abs(w[0] - 0.1) < 1e-15 and abs(w[1] - 0.9) < 1e-15
    w = posterior_weights([-1000.0, -1001.0, -5000.0])                                           # no underflow to 0 / 0
    assert abs(sum(w) - 1.0) < 1e-15 and abs(w[0] / w[1] - math.e) < 1e-12 and w[2] == 0.0


def test_dense_ids_and_the_host_error_rate():
    from ast_amd import eval as E
    ids, table = E.dense_ids([["a", "b", "a"], [], ["c", "b"], [7, "7"]])
    assert ids == [[0, 1, 0], [], [2, 1], [3, 4]] and table == {"a": 0, "b": 1, "c": 2, 7: 3, "7": 4}
    refs = [[["the", "cat", "sat"], ["a", "cat", "sat", "down"]], [["hello"]], [["x", "y"], ["y", "x"]], [[], ["q"]]]
    hyps = [["a", "cat", "sat"], ["hello", "there"], ["z"], []]
    got = E.error_rate(refs, hyps, device="cpu")
    # segment 0: the first reference at distance 1 (the second is at 1 too: ties to the first): 1 sub, N 3; segment 1: 1 ins, N 1;
    # segment 2: both references at distance 2: the first, 1 sub + 1 del, N 2; segment 3: the empty reference at 0, N 0
    assert got == {"S": 2, "D": 1, "I": 1, "N": 6, "rate": 4 / 6} == PM.error_rate(refs, hyps)
    assert E.error_rate([], [], device="cpu") == {"S": 0, "D": 0, "I": 0, "N": 0, "rate": 0.0}
    assert hasattr(E.Eval, "calc_wer")


def test_mbr_select_lists_refuses_bad_arguments():
    from ast_amd import nn
    e = {"hyp": [1, 5, 2], "score": -1.0}
    with pytest.raises(ValueError, match="utility"):
        nn.mbr_select_lists([[e]], utility="wer")
    with pytest.raises(ValueError, match="no hypotheses"):
        nn.mbr_select_lists([[e], []])
    with pytest.raises(ValueError, match="weight"):
        nn.mbr_select_lists([[e]], weights=[[1.0], [1.0]])
    with pytest.raises(ValueError, match="weights"):
        nn.mbr_select_lists([[e, e]], weights=[[1.0]])
    # one-element lists and lists beyond the device's length take no launch: they work without a GPU
    long = [{"hyp": [1] + [4 + (k * i) % 7 for k in range(520)] + [2], "score": -float(i)} for i in range(1, 3)]
    assert nn.mbr_select_lists([[e], long], "bleu") == [0, nn.mbr_select(long)]
    lists = [[(h["hyp"], h["score"]) for h in long]]
    assert nn.mbr_select_lists([long, [e]], "edit") == [PM.mbr_edit(lists)[0][0], 0]


def test_command_lines_parse():
    import importlib.util

    def load(name):
        spec = importlib.util.spec_from_file_location(name.replace(".", "_") + "_cli", os.path.join(ROOT, name))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)                                                            # (no main: nothing runs)
        return mod
    a = vars(load("mbr.py").build_parser().parse_args(["-m", "d", "-s", "dev", "--nbest", "n.p"]))
    assert (a["utility"], a["posterior_scale"], a["batch"], a["out"]) == ("bleu", None, 1, None)
    a = vars(load("mbr.py").build_parser().parse_args(["-m", "d", "-s", "dev", "--nbest", "n.p", "--utility", "edit", "--posterior-scale", "0.5",
                                                      "-b", "32", "-w", "o"]))
    assert (a["utility"], a["posterior_scale"], a["batch"], a["out"]) == ("edit", 0.5, 32, "o")
    a = vars(load("sample.py").build_parser().parse_args(["-m", "d", "-s", "dev", "-n", "4"]))
    assert a["utility"] is None and a["mbr"] is False
    a = vars(load("sample.py").build_parser().parse_args(["-m", "d", "-s", "dev", "-n", "4", "--utility", "edit"]))
    assert a["utility"] == "edit"
    a = vars(load("ctc_decode.py").build_parser().parse_args(["-m", "d", "-s", "dev", "-n", "5", "-c", "4"]))
    assert a["wer"] is False
    assert vars(load("ctc_decode.py").build_parser().parse_args(["-m", "d", "-s", "dev", "-n", "5", "-c", "4", "--wer"]))["wer"] is True


# ------------------------------------------------------------------ the library without a GPU
def test_symbols_are_declared_listed_and_exported():
    from ast_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "astk.h")).read()
    for lib_path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        lib = C.CDLL(lib_path)
        assert re.search(r"\bastk_pair_stats\s*\(", hdr) and "astk_pair_stats" in _lib.SIGNATURES
        assert isinstance(lib.astk_pair_stats, C._CFuncPtr)
    decl = re.search(r"int astk_pair_stats\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(_lib.SIGNATURES["astk_pair_stats"][1]) == 7
    for name in ("tokens", "lens", "pairs"):
        assert "const int32_t* " + name in decl                                                 # read-only by declaration
    fields = re.search(r"typedef struct \{([^}]*)\} astk_pair_stats_desc;", hdr).group(1)
    names = re.findall(r"\b(struct_size|S|Lmax|P)\b\s*[,;]", fields)
    assert names == [f[0] for f in _lib.PairStatsDesc._fields_] == ["struct_size", "S", "Lmax", "P"]
    assert int(re.search(r"#define ASTK_PAIR_MAX_LEN (\d+)", hdr).group(1)) == _lib.PAIR_MAX_LEN == PM.MAX_LEN == 512
    srcs = open(os.path.join(ROOT, "ast_amd", "csrc", "build.sh")).read().split("SRCS=")[1].split("\n")[0]
    assert " pairs" in srcs


GOOD = dict(S=3, Lmax=8, P=4)
REFUSALS = (("S", 0, "S"), ("S", -2, "S"), ("P", 0, "P"), ("P", -1, "P"), ("Lmax", 0, "Lmax"), ("Lmax", 513, "Lmax"), ("Lmax", -1, "Lmax"))


def test_descriptor_refusals_need_no_device():
    """Every refusal comes from the descriptor and the pointers alone, before any launch: with a fake non-null pointer for the
    buffers no device is touched."""
    from ast_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)

    def call(d, tokens=fake, lens=fake, pairs=fake, stats=fake):
        return lib.astk_pair_stats(C.byref(d), tokens, lens, pairs, stats, None, None)
    for field, value, word in REFUSALS:
        d = _lib.PairStatsDesc(**{**GOOD, field: value})
        assert call(d) != 0 and word in lib.astk_last_error().decode(), (field, lib.astk_last_error().decode())
        assert "ASTK_" not in lib.astk_last_error().decode()
    d = _lib.PairStatsDesc(**GOOD)
    d.struct_size -= 4
    assert call(d) != 0 and "struct_size" in lib.astk_last_error().decode()
    d = _lib.PairStatsDesc(**GOOD)
    for kw in (dict(tokens=None), dict(lens=None), dict(pairs=None), dict(stats=None)):
        assert call(d, **kw) != 0 and "null" in lib.astk_last_error().decode(), kw
    assert _lib.PairStatsDesc(**{**GOOD, "Lmax": 512}).Lmax == 512
