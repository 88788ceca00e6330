"""GPU tests of the pair statistics (include/astk.h astk_pair_stats): the operator through the C ABI on the named
cases of tests/pair_stats_model.py -- all eight integers of every row EQUAL to the host model's, bad rows eight -1 and n_bad exact,
nothing excluded -- run-to-run bytes, untouched inputs, untouched rows behind P, the refusals; then mbr_select_lists against mbr_select
and the model's integer risks, error_rate, and the three command lines."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import pair_stats_model as PM
from conftest import tiny_cfg
from test_gpu_ops import dev, ok, stream, vp
from test_pair_stats_host import GOOD, REFUSALS

pytestmark = pytest.mark.gpu

FILL = -7


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


def _run_op(lib, c, with_n_bad=True, spare_rows=3):
    """astk_pair_stats on one case's host arrays: the (P + spare_rows, 8) buffer and n_bad as host arrays, the inputs before and after."""
    from ast_amd import _lib
    S, Lmax = c["tokens"].shape
    P = len(c["pairs"])
    ins = [dev(c["tokens"], torch.int32), dev(c["lens"], torch.int32), dev(c["pairs"], torch.int32)]
    before = [t.clone() for t in ins]
    stats = torch.full((P + spare_rows, 8), FILL, dtype=torch.int32, device="cuda")
    n_bad = torch.full((3,), FILL, dtype=torch.int32, device="cuda")
    d = _lib.PairStatsDesc(S, Lmax, P)
    ok(lib, lib.astk_pair_stats(C.byref(d), vp(ins[0]), vp(ins[1]), vp(ins[2]), vp(stats), C.c_void_p(n_bad.data_ptr() + 4) if with_n_bad else None,
                                stream()))
    torch.cuda.synchronize()
    return dict(stats=stats.cpu().numpy(), n_bad=n_bad.cpu().numpy(), before=before, after=ins)


@pytest.mark.parametrize("name", PM.ALL_CASES)
def test_pair_stats_equals_the_host_model(lib, name):
    c, (want, want_bad) = PM.result(name)
    P = len(c["pairs"])
    r = _run_op(lib, c)
    wrong = np.flatnonzero((r["stats"][:P] != want).any(axis=1))
    assert wrong.size == 0, (name, len(wrong), [(c["pairs"][k].tolist(), r["stats"][k].tolist(), want[k].tolist()) for k in wrong[:4]])
    assert r["n_bad"].tolist() == [FILL, want_bad, FILL], (name, r["n_bad"])
    assert (r["stats"][P:] == FILL).all(), "rows behind P were written"
    for b, a in zip(r["before"], r["after"]):
        assert torch.equal(b, a), "an input buffer was written"
    bad = np.asarray([PM.row_is_bad(c["lens"].tolist(), c["tokens"].shape[1], a, b) for a, b in c["pairs"].tolist()])
    assert (r["stats"][:P][bad] == -1).all() and (r["stats"][:P][~bad] >= 0).all() and int(bad.sum()) == want_bad


@pytest.mark.parametrize("name", ["cap", "p5000", "bad-rows", "boundaries-2-symbols"])
def test_pair_stats_is_bit_identical_from_run_to_run_and_n_bad_is_optional(lib, name):
    c, (want, _) = PM.result(name)
    a, b = _run_op(lib, c), _run_op(lib, c, with_n_bad=False)
    assert a["stats"].tobytes() == b["stats"].tobytes()
    assert b["n_bad"].tolist() == [FILL] * 3


def test_pair_stats_refuses_bad_arguments_before_any_launch(lib):
    from ast_amd import _lib
    g = GOOD
    tokens = torch.full((g["S"], g["Lmax"]), 3, dtype=torch.int32, device="cuda")
    lens = torch.full((g["S"],), 5, dtype=torch.int32, device="cuda")
    pairs = torch.zeros((g["P"], 2), dtype=torch.int32, device="cuda")
    stats = torch.full((g["P"], 8), FILL, dtype=torch.int32, device="cuda")
    n_bad = torch.full((1,), FILL, dtype=torch.int32, device="cuda")

    def call(d, t=tokens, l=lens, p=pairs, s=stats):
        return lib.astk_pair_stats(C.byref(d), vp(t), vp(l), vp(p), vp(s), vp(n_bad), stream())

    def untouched():
        torch.cuda.synchronize()
        assert int((stats != FILL).sum()) == 0 and int(n_bad[0]) == FILL, "the refused call launched something"
    for field, value, word in REFUSALS + (("struct_size", 8, "struct_size"),):
        d = _lib.PairStatsDesc(**{**g, **({field: value} if field != "struct_size" else {})})
        if field == "struct_size":
            d.struct_size = value
        assert call(d) != 0
        assert word in lib.astk_last_error().decode(), (field, lib.astk_last_error().decode())
        untouched()
    d = _lib.PairStatsDesc(**g)
    for kw in (dict(t=None), dict(l=None), dict(p=None), dict(s=None)):
        assert call(d, **kw) != 0 and "null" in lib.astk_last_error().decode(), kw
        untouched()
    assert call(d) == 0                                                       # (and the good call goes through)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [[0, 0, 0, 0, 5, 4, 3, 2]] * g["P"] and int(n_bad[0]) == 0


# ------------------------------------------------------------------ 2. the Python layer
def _random_lists(seed):
    """8 lists, N from 1 to 32 mixed in one call: duplicated hypotheses, forced ties in gain (a duplicate with another score) and in
    gain and score together (a duplicate with the same score)."""
    rng = random.Random(seed)
    lists = []
    for n in (1, 2, 32, 5, 3, 17, 8, 31):
        base = [rng.randrange(4, 12) for _ in range(rng.randrange(3, 14))]
        lst = []
        for _ in range(n):
            h = [t if rng.random() < 0.8 else rng.randrange(4, 12) for t in base][:rng.randrange(1, len(base) + 1)]
            lst.append({"hyp": [1] + h + [2], "score": -rng.random() * 9})
        if n >= 3:
            lst[-1] = {"hyp": list(lst[0]["hyp"]), "score": lst[0]["score"] - 0.5}           # the same gain, a lower score
            lst[-2] = dict(lst[1], hyp=list(lst[1]["hyp"]))                                  # the same gain and score: the lower index
        lists.append(lst)
    return lists


def test_mbr_select_lists_bleu_is_mbr_select(lib):
    from ast_amd.nn import mbr_select, mbr_select_lists
    lists = _random_lists(3)
    want = [mbr_select(l) for l in lists]
    assert mbr_select_lists(lists, "bleu") == want
    assert mbr_select_lists(lists, "bleu", weights=[[1.0] * len(l) for l in lists]) == want      # equal weights: the plain mean
    assert mbr_select_lists(lists[2:3]) == want[2:3]
    # the best members of a list all tie, and the tie rule decides: a list of duplicates
    dup = [{"hyp": [1, 5, 6, 2], "score": s} for s in (-2.0, -1.0, -1.0, -3.0)]
    assert mbr_select_lists([dup, lists[3]]) == [1, want[3]] == [mbr_select(dup), want[3]]


def test_mbr_select_lists_edit_is_the_models_integer_risk(lib):
    from ast_amd import eval as E
    from ast_amd.nn import mbr_select_lists
    lists = _random_lists(4)
    want, risks = PM.mbr_edit([[(h["hyp"], h["score"]) for h in l] for l in lists])
    assert mbr_select_lists(lists, "edit") == want
    for lst, risk in zip(lists, risks):                                       # the risks themselves, from the device's statistics
        n = len(lst)
        pairs = [(i, j) for i in range(n) for j in range(n) if i != j]
        st = E.pair_stats([h["hyp"] for h in lst], pairs)
        got = [sum(int(st[k][0]) for k, (i, _) in enumerate(pairs) if i == m) for m in range(n)]
        assert got == risk
    assert any(sorted(r)[0] == sorted(r)[1] for r in risks if len(r) > 1)        # ties in the risk occurred


def test_mbr_select_lists_weighted_known_answers(lib):
    from ast_amd.eval import corpus_bleu
    from ast_amd.nn import mbr_select_lists, posterior_weights
    # d(A, A') = 0, d(A, B) = 1, d(A, C) = 2, d(B, C) = 1: unweighted risks 3, 3, 3, 5 -- the tie goes to the highest score (B)
    A, B, Cc = [4, 5, 6], [4, 5, 7], [4, 8, 7]
    lst = [{"hyp": A, "score": -1.0}, {"hyp": list(A), "score": -2.0}, {"hyp": B, "score": -0.5}, {"hyp": Cc, "score": -3.0}]
    assert mbr_select_lists([lst], "edit") == [2]
    # weighted means over the others: A 1.7 / 0.95, A' the same, B 0.9 / 0.9, C 0.3 / 0.2
    assert mbr_select_lists([lst], "edit", weights=[[0.05, 0.05, 0.1, 0.8]]) == [2]
    # A 0.15 / 0.2, A' 0.15 / 0.9, B 0.95 / 0.95, C 1.85 / 0.95
    assert mbr_select_lists([lst, lst], "edit", weights=[[0.8, 0.1, 0.05, 0.05], [0.05, 0.05, 0.1, 0.8]]) == [1, 2]
    # bleu: the weighted mean of corpus_bleu against the others, in float64 on the host
    lists = _random_lists(5)[2:6]
    weights = [posterior_weights([h["score"] for h in l], 0.7) for l in lists]
    want = []
    for l, w in zip(lists, weights):
        gain = []
        for i, h in enumerate(l):
            others = [j for j in range(len(l)) if j != i]
            gain.append(sum(w[j] * corpus_bleu([[l[j]["hyp"]]], [h["hyp"]]) for j in others) / sum(w[j] for j in others))
        want.append(max(range(len(l)), key=lambda i: (gain[i], l[i]["score"], -i)))
    assert mbr_select_lists(lists, "bleu", weights=weights) == want


def test_error_rate_on_the_device_equals_the_model(lib):
    from ast_amd import eval as E
    refs = [[["the", "cat", "sat"], ["a", "cat", "sat", "down"]], [["hello"]], [["x", "y"], ["y", "x"]], [[], ["q"]]]
    hyps = [["a", "cat", "sat"], ["hello", "there"], ["z"], []]
    assert E.error_rate(refs, hyps, device="cuda") == {"S": 2, "D": 1, "I": 1, "N": 6, "rate": 4 / 6}
    rng = random.Random(8)
    words = ["w%d" % k for k in range(6)]
    refs = [[[rng.choice(words) for _ in range(rng.randrange(0, 70))] for _ in range(rng.randrange(1, 4))] for _ in range(40)]
    hyps = [[rng.choice(words) for _ in range(rng.randrange(0, 70))] for _ in range(40)]
    refs[7][0], hyps[7] = [rng.choice(words) for _ in range(530)], [rng.choice(words) for _ in range(40)]      # beyond the device's length
    want = PM.error_rate(refs, hyps)
    assert E.error_rate(refs, hyps) == want == E.error_rate(refs, hyps, device="cpu") and want["N"] > 0


def test_the_command_lines(tmp_path):
    """On a tiny synthetic experiment with the CTC head, as child processes: `sample.py --utility edit` writes one hypothesis per
    utterance and prints both metrics; `mbr.py` on its pickle makes the same choice; `ctc_decode.py --wer` prints the counts
    Eval.calc_wer gives for its pickle's first hypotheses."""
    import json, os, pickle, re, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mcfg = tiny_cfg(enc_layers=2, dec_layers=1, H=32, E=16, A=32, c0=8, c1=16, V=31, drop=0.0)
    del mcfg["rnn_config"]["dec_vocab_size"]
    mcfg["rnn_config"]["ctc"] = True
    tcfg = {"seed": "seed-ast-20h", "gpuid": 0, "batch_size": 4, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 1,
            "optimizer": {"type": 0, "lr": 2e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0},
            "data": {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 8, "syn_dev": 6},
                     "frames": [60, 300], "targets": [2, 9], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w", "refs_path": str(tmp_path / "refs"), "n_evals": 1}}
    json.dump(mcfg, open(tmp_path / "model_cfg.json", "w"))
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))
    from ast_amd.eval import Eval
    from ast_amd.nn import NN
    nn = NN(str(tmp_path))
    refs = tmp_path / "refs" / "syn_dev"
    os.makedirs(refs)
    utts = sorted(nn.data_loader.info["syn_dev"])
    truth = nn.data_loader.get_hyps([(u, list(nn.data_loader.ids["syn_dev"][u])) for u in utts])
    (refs / "eval.ids").write_text("".join(u + "\n" for u in utts))
    (refs / "ref.en0").write_text("".join(" ".join(truth[u]) + "\n" for u in utts))

    def run(script, *extra):
        r = subprocess.run([sys.executable, os.path.join(root, script), "-m", str(tmp_path), "-s", "syn_dev"] + list(extra), cwd=root,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    pk = str(tmp_path / "samples.p")
    out = run("sample.py", "-n", "6", "--seed", "11", "--utility", "edit", "-b", "4", "-w", pk)
    assert "MBR BLEU = " in out and "MBR WER = " in out
    chosen = open(pk + ".mbr.en").read()
    assert len(chosen.split("\n")) == len(utts) + 1 and chosen.endswith("\n")
    samples = pickle.load(open(pk, "rb"))
    assert sorted(samples) == utts and all(len(v) == 6 for v in samples.values())
    out2 = run("mbr.py", "--nbest", pk, "--utility", "edit", "-b", "3", "-w", str(tmp_path / "again"))
    assert open(tmp_path / "again.mbr.en").read() == chosen
    metrics = [[l for l in o.splitlines() if l.startswith(("MBR BLEU = ", "MBR WER = "))] for o in (out, out2)]
    assert metrics[0] == metrics[1] and len(metrics[0]) == 2
    nb = str(tmp_path / "nbest.p")
    out3 = run("ctc_decode.py", "-n", "3", "-c", "4", "--wer", "-w", nb)
    m = re.search(r"^WER = (\d+\.\d\d) \(S (\d+), D (\d+), I (\d+), N (\d+)\)$", out3, re.M)
    assert m, out3[-600:]
    nbest = pickle.load(open(nb, "rb"))
    wer = Eval(str(refs), 1).calc_wer(nn.data_loader.get_hyps((u, list(lst[0][0])) for u, lst in nbest.items()))
    assert [int(v) for v in m.groups()[1:]] == [wer["S"], wer["D"], wer["I"], wer["N"]] and m.group(1) == "{0:.2f}".format(wer["rate"] * 100)
    assert wer["N"] == sum(len(truth[u]) for u in utts) > 0
