"""GPU tests of the CTC forced alignment (include/astk.h astk_ctc_align): the operator through the C ABI on the
cases of tests/ctc_align_model.py -- validity of every path, the infeasible rows, the score and the float64 deficit of the kernel's own
path within 4 x the float32 model's figures, exact paths where the optimum is unique (planted) or the tie rule decides (uniform),
label_logp, run-to-run bits, untouched logits, coexistence with astk_ctc_loss -- then Seq2Seq.ctc_align, score.py and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_align_model as AM
import ctc_model as CM
import schedule_helpers as SH
from conftest import tiny_cfg
from test_gpu_ops import GuardedWS, dev, ok, stream, vp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


# ------------------------------------------------------------------ 1. operator level
# Bounds per case family = 4 x the figures of the NumPy model run in float32 against its float64 run (ctc_align_model.F32_SCORE_RERR,
# F32_DEFICIT; measured on the CPU, held by tests/test_ctc_align_host.py).  The factor is section 28's, for another summation order in
# the lse.  The deficits are 0: the kernel's path must be optimal in float64, though it need not be the model's where two are.
SCORE_RTOL = {k: 4.0 * v for k, v in AM.F32_SCORE_RERR.items()}
DEFICIT_BOUND = {k: 4.0 * v for k, v in AM.F32_DEFICIT.items()}

_MODEL = {}


def _model(name):
    """(logits, y, lens, the float64 model's result) of one case, computed once and shared."""
    if name not in _MODEL:
        x, y, lens = AM.case(name)
        _MODEL[name] = (x, y, lens, AM.align(x.astype(np.float64), y, lens))
    return _MODEL[name]


def _run_op(lib, x, y, lens, ldv=None, first_label=CM.UNK_ID, blank=CM.PAD_ID, optional=True, ws=None):
    """astk_ctc_align on host arrays; returns the outputs as host arrays, the logits buffer before and after, and the count."""
    from ast_amd import _lib
    B, T, V = x.shape
    L = y.shape[1]
    ldv = ldv or V
    buf = torch.full((B, T, ldv), 7.0, device="cuda")
    buf[:, :, :V] = dev(x)
    before = buf.clone()
    y_d = dev(y, torch.int32)
    len_d = None if lens is None else dev(lens, torch.int32)
    d = _lib.CtcDesc(B, T, V, ldv, L, L, first_label, blank)
    nbytes = lib.astk_ctc_align_workspace_bytes(C.byref(d))
    assert nbytes > 0, lib.astk_last_error().decode()
    ws = ws or GuardedWS(nbytes)
    i32 = dict(dtype=torch.int32, device="cuda")
    fs, fc = torch.full((B, T), -7, **i32), torch.full((B, T), -7, **i32)
    l0, l1 = torch.full((B, L), -7, **i32), torch.full((B, L), -7, **i32)
    lp = torch.full((B, L), -7.0, device="cuda")
    score = torch.full((B,), 5.0, device="cuda")
    bad = torch.full((1,), -9, **i32)
    opt = (lambda t: vp(t)) if optional else (lambda t: None)
    ok(lib, lib.astk_ctc_align(C.byref(d), vp(buf), vp(y_d), vp(len_d), vp(fs), opt(fc), opt(l0), opt(l1), opt(lp), vp(score), opt(bad),
                               vp(ws), ws.nbytes, stream()))
    ws.check("ctc_align")
    return dict(frame_state=fs.cpu().numpy(), frame_class=fc.cpu().numpy(), label_start=l0.cpu().numpy(), label_end=l1.cpu().numpy(),
                label_logp=lp.cpu().numpy(), row_score=score.cpu().numpy(), n_infeasible=int(bad), logits_before=before, logits_after=buf)


@pytest.mark.parametrize("name", AM.ALL_CASES)
def test_ctc_align_against_the_float64_model(lib, name):
    """Every row of every case: a legal path that collapses to the labels, spans and label_logp consistent with it, the frames behind
    input_len and the rows without a path exactly as defined, the count; row_score within 4 x the family's float32-model figure of the
    float64 optimum; the kernel's own path rescored in float64 within 4 x the family's deficit figure (0: an optimal path) of it;
    label_logp within the row's absolute score bound of the float64 sums over the kernel's own spans; exact path equality on the
    planted and uniform cases; the logits untouched."""
    x, y, lens, m = _model(name)
    fam = AM.family(name)
    B, T, V = x.shape
    L = y.shape[1]
    r = _run_op(lib, x, y, lens, ldv=CM.OP_CASES.get(name, {}).get("ldv"))
    assert torch.equal(r["logits_before"].view(torch.int32), r["logits_after"].view(torch.int32)), "the logits were written"
    assert r["n_infeasible"] == m["n_infeasible"]
    worst = dict(score=0.0, deficit=0.0, label=0.0)
    for b in range(B):
        n = T if lens is None else int(np.clip(lens[b], 0, T))
        labels = m["labels"][b]
        U = len(labels)
        fs, fc = r["frame_state"][b], r["frame_class"][b]
        assert (fs[n:] == -1).all() and (fc[n:] == CM.PAD_ID).all(), "frames behind the row's length"
        assert (r["label_start"][b, U:] == -1).all() and (r["label_end"][b, U:] == -1).all() and (r["label_logp"][b, U:] == 0).all()
        if not CM.feasible(labels, n):
            assert r["row_score"][b] == -np.inf and (fs == -1).all() and (fc == CM.PAD_ID).all()
            assert (r["label_start"][b] == -1).all() and (r["label_end"][b] == -1).all() and (r["label_logp"][b] == 0).all()
            continue
        path = fs[:n].astype(np.int64)
        assert AM.is_valid_path(list(path), labels, CM.PAD_ID), (name, b, path)
        z, _ = AM.extended(labels, CM.PAD_ID)
        assert np.array_equal(fc[:n], z[path]) and CM.collapse(fc[:n]) == labels
        s0, s1 = AM.spans(path, U)
        assert np.array_equal(r["label_start"][b, :U], s0) and np.array_equal(r["label_end"][b, :U], s1)
        e64 = AM.emissions(x[b, :n].astype(np.float64), labels, CM.PAD_ID)
        best = AM.rescore(e64, m["frame_state"][b, :n])                       # the float64 optimum, summed as the deficit's other term is
        got = float(r["row_score"][b])
        if n == 0:
            assert got == 0.0
            continue
        worst["score"] = max(worst["score"], abs(got - best) / abs(best))
        worst["deficit"] = max(worst["deficit"], best - AM.rescore(e64, path))
        want_lp = AM.label_logp(e64, path, U)
        err_lp = np.abs(r["label_logp"][b, :U].astype(np.float64) - want_lp).max(initial=0.0)
        worst["label"] = max(worst["label"], err_lp / abs(best))
        assert abs(got - best) <= SCORE_RTOL[fam] * abs(best), (name, b, got, best)
        assert best - AM.rescore(e64, path) <= DEFICIT_BOUND[fam], (name, b)
        assert err_lp <= SCORE_RTOL[fam] * abs(best), (name, b, err_lp)
        if name not in CM.OP_CASES:
            assert np.array_equal(path, m["frame_state"][b, :n]), (name, b)
    print(name, fam, "score rel err", worst["score"], "bound", SCORE_RTOL[fam], "deficit", worst["deficit"], "bound", DEFICIT_BOUND[fam],
          "label err / |score|", worst["label"])
    if name not in CM.OP_CASES:                                               # the expected paths themselves (the model is held to them on the host)
        paths = (AM.planted_case if name in AM.PLANTED_CASES else AM.uniform_case)(name)[3]
        for b, want in enumerate(paths):
            assert np.array_equal(r["frame_state"][b, :len(want)], want)


@pytest.mark.parametrize("name", ["b33-ragged", "u255-infeasible-between", "all-equal", "v1098-one-path", "u255-s511", "uniform-s67"])
def test_ctc_align_is_bit_identical_from_run_to_run(lib, name):
    x, y, lens, _ = _model(name)
    a, b = _run_op(lib, x, y, lens), _run_op(lib, x, y, lens)
    for k in ("frame_state", "frame_class", "label_start", "label_end"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("label_logp", "row_score"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def test_ctc_align_without_the_optional_outputs(lib):
    """frame_class, the spans, label_logp and n_infeasible NULL, input_len NULL, another blank / first label: frame_state and row_score
    as with them, and as the model has them."""
    x, y, _, _ = _model("all-equal")
    m = AM.align(x.astype(np.float64), y, None, first_label=5, blank=4)
    full = _run_op(lib, x, y, None, first_label=5, blank=4)
    bare = _run_op(lib, x, y, None, first_label=5, blank=4, optional=False)
    assert np.array_equal(full["frame_state"], bare["frame_state"]) and np.array_equal(full["row_score"].view(np.int32), bare["row_score"].view(np.int32))
    assert (bare["frame_class"] == -7).all() and (bare["label_start"] == -7).all() and (bare["label_logp"] == -7).all() and bare["n_infeasible"] == -9
    assert np.array_equal(full["frame_state"], m["frame_state"]) and np.array_equal(full["frame_class"], m["frame_class"])
    np.testing.assert_allclose(full["row_score"], m["row_score"], rtol=SCORE_RTOL["short"])


def test_ctc_loss_keeps_its_bits_beside_an_align_call(lib):
    """astk_ctc_loss on the same inputs, in ONE workspace allocation the two calls share (the way Seq2Seq.ctc_align uses them): the
    loss's row_nll and dlogits are the same bits before and after an align call, and the alignment is what it is on a workspace of
    its own."""
    from ast_amd import _lib
    for name in ("u32-ragged", "u255-infeasible-between"):
        x, y, lens, _ = _model(name)
        B, T, V = x.shape
        L = y.shape[1]
        d = _lib.CtcDesc(B, T, V, V, L, L, CM.UNK_ID, CM.PAD_ID)
        need = max(lib.astk_ctc_workspace_bytes(C.byref(d)), lib.astk_ctc_align_workspace_bytes(C.byref(d)))
        ws = GuardedWS(need)
        y_d, len_d = dev(y, torch.int32), dev(lens, torch.int32)

        def loss():
            buf, nll = dev(x), torch.zeros(B, device="cuda")
            ok(lib, lib.astk_ctc_loss(C.byref(d), vp(buf), vp(y_d), vp(len_d), 0.5, vp(nll), None, vp(buf), None, vp(ws), ws.nbytes, stream()))
            ws.check("ctc_loss")
            return nll.view(torch.int32).clone(), buf.view(torch.int32).clone()
        a = loss()
        shared = _run_op(lib, x, y, lens, ws=ws)
        b = loss()
        own = _run_op(lib, x, y, lens)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert np.array_equal(shared["frame_state"], own["frame_state"]) and np.array_equal(shared["row_score"].view(np.int32), own["row_score"].view(np.int32))


def test_ctc_align_refuses_bad_arguments_before_any_launch(lib):
    from ast_amd import _lib
    B, T, V, L = 2, 4, 7, 3
    buf = torch.full((B, T, V), 2.0, device="cuda")
    y_d = torch.full((B, L), 4, dtype=torch.int32, device="cuda")
    fs = torch.full((B, T), -5, dtype=torch.int32, device="cuda")
    score = torch.full((B,), -1.0, device="cuda")
    ws = GuardedWS(1 << 16)
    good = dict(B=B, T=T, V=V, ldv=V, L=L, ldy=L, first_label=3, blank=0)

    def call(d, logits=buf, y=y_d, frame_state=fs, row_score=score, w=ws, nbytes=None):
        return lib.astk_ctc_align(C.byref(d), vp(logits), vp(y), None, vp(frame_state), None, None, None, None, vp(row_score), None, vp(w),
                                  ws.nbytes if nbytes is None else nbytes, stream())

    def untouched():
        torch.cuda.synchronize()
        assert float((buf - 2.0).abs().max()) == 0.0 and float((score + 1.0).abs().max()) == 0.0 and int((fs != -5).sum()) == 0
        assert int((ws.t != 0x5A).sum()) == 0, "the refused call launched something"
    for field, value, word in (("V", 1, "V"), ("blank", V, "blank"), ("blank", -1, "blank"), ("first_label", 0, "first_label"), ("B", 0, "B"),
                               ("T", 0, "T"), ("L", 0, "L"), ("L", 256, "labels"), ("ldv", V - 1, "ldv"), ("ldy", L - 1, "ldy"),
                               ("struct_size", 8, "struct_size")):
        d = _lib.CtcDesc(**{**good, **({field: value} if field != "struct_size" else {})})
        if field == "struct_size":
            d.struct_size = value
        if field == "L":
            d.ldy = max(value, 1)
        assert lib.astk_ctc_align_workspace_bytes(C.byref(d)) == 0
        assert call(d) < 0
        assert word in lib.astk_last_error().decode(), (field, lib.astk_last_error().decode())
        untouched()
    d = _lib.CtcDesc(**good)
    need = lib.astk_ctc_align_workspace_bytes(C.byref(d))
    assert call(d, nbytes=need - 1) < 0 and "workspace" in lib.astk_last_error().decode()
    untouched()
    for kw in (dict(logits=None), dict(y=None), dict(frame_state=None), dict(row_score=None), dict(w=None)):
        assert call(d, **kw) < 0 and "null" in lib.astk_last_error().decode(), kw
        untouched()
    assert call(d, nbytes=need) == 0                                          # (and the good call goes through)
    torch.cuda.synchronize()
    assert int((fs == -5).sum()) == 0


# ------------------------------------------------------------------ 2. model level
def _head_model(x_lens=None):
    """A model with the head on the small golden shape (B = 2, T = 37), a bias on the blank so that the paths hold blanks."""
    cfg = tiny_cfg(c1=8)
    cfg["rnn_config"]["ctc"] = True
    B, T, D, L, V = 2, 37, 26, 6, 11
    P, X, y = SH.make_inputs(cfg, B, T, D, L, V)
    P = dict(P)
    P.update(CM.head_params(cfg["rnn_config"]["hidden_units"], V))
    P["ctc_out/b"] = P["ctc_out/b"].copy()
    P["ctc_out/b"][0] += 0.3
    return cfg, SH.gpu_model(cfg, P, D, V), X, y, V


def test_seq2seq_ctc_align_against_the_model_on_the_heads_logits(lib):
    """Ragged x_lens: every row's dict against the float64 model run on the head's logits read back from the device (the same product
    again: bit-identical from run to run); total_logp = -ctc_nll of a forward_loss(ctc_weight > 0) step's rows at that test's 1e-4;
    segments_input inside [0, x_len] and monotone; the dict's pieces consistent with each other."""
    from ast_amd.seq2seq import cnn_out_lens, using_config
    cfg, g, X, y, V = _head_model()
    x_lens = np.asarray([37, 29], np.int32)
    rows = g.ctc_align(torch.from_numpy(X), y, x_lens=x_lens)
    logits, Vp = g._ctc_logits(g._cur, g._stream())
    T2 = g._cur["T2"]
    lg = logits.view(len(X), T2, Vp)[:, :, :V].cpu().numpy()
    lens = np.asarray([cnn_out_lens(cfg["cnn_config"]["cnn_layers"], int(n))[-1] for n in x_lens], np.int32)
    m = AM.align(lg.astype(np.float64), y, lens)
    with using_config("train", False):                                        # (eval mode, like the alignment: the same encoder states)
        g.forward_loss(X=torch.from_numpy(X), y=torch.from_numpy(y), teach_ratio=1.0, ctc_weight=0.3, x_lens=x_lens)
    nll = g.ctc_nll.cpu().double().numpy()
    assert len(rows) == len(X) and (lens < T2).any()
    for b, r in enumerate(rows):
        labels = m["labels"][b]
        U, n = len(labels), int(lens[b])
        assert U > 0 and r["labels"].tolist() == labels and r["n_frames"] == n and r["frame_state"].shape == (T2,)
        path = r["frame_state"][:n].astype(np.int64)
        assert AM.is_valid_path(list(path), labels, CM.PAD_ID) and (r["frame_state"][n:] == -1).all()
        assert CM.collapse(r["frame_class"][:n]) == labels
        e64 = AM.emissions(lg[b, :n].astype(np.float64), labels, CM.PAD_ID)
        best = AM.rescore(e64, m["frame_state"][b, :n])
        print("row", b, "score", r["score"], "model", best, "total_logp", r["total_logp"], "-nll", -nll[b], "segments", r["segments"].tolist())
        assert abs(r["score"] - best) <= SCORE_RTOL["short"] * abs(best)
        assert best - AM.rescore(e64, path) <= DEFICIT_BOUND["short"]
        s0, s1 = AM.spans(path, U)
        assert np.array_equal(r["segments"], np.stack([s0, s1], 1))
        want_lp = AM.label_logp(e64, path, U)
        assert np.abs(r["label_logp"] - want_lp).max() <= SCORE_RTOL["short"] * abs(best)
        np.testing.assert_allclose(r["confidence"], np.exp(want_lp / (s1 - s0)), rtol=1e-5)
        assert ((r["confidence"] > 0) & (r["confidence"] <= 1)).all()
        np.testing.assert_allclose(r["total_logp"], -nll[b], rtol=1e-4)
        assert r["score"] <= r["total_logp"] + 1e-4 * abs(r["total_logp"])
        si = r["segments_input"]
        assert si.shape == (U, 2) and (si >= 0).all() and (si <= x_lens[b]).all() and (si[:, 0] < si[:, 1]).all()
        assert (np.diff(si[:, 0]) >= 0).all() and (np.diff(si[:, 1]) >= 0).all()
    # without x_lens every frame is valid; a model without the head and targets beyond the label limit are refused
    full = g.ctc_align(torch.from_numpy(X), y)
    assert all(r["n_frames"] == T2 for r in full)
    with pytest.raises(ValueError, match="rnn_config.ctc"):
        SH.gpu_model(tiny_cfg(), SH.make_inputs(tiny_cfg(), 2, 21, 26, 5, 11)[0], 26, 11).ctc_align(torch.zeros(2, 21, 26), y[:, :5])
    with pytest.raises(ValueError, match="ASTK_CTC_MAX_LABELS"):
        g.ctc_align(torch.from_numpy(X), np.zeros((2, 256), np.int32))


def test_score_py_writes_the_ctc_alignments(tmp_path):
    """`python score.py --ctc-alignments` on the synthetic corpus: the documented keys for every reference, consistent shapes, score <=
    total_logp; the same writer on a beam.py-style n-best list: one entry per hypothesis (utt#rank)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mcfg = tiny_cfg(enc_layers=2, dec_layers=1, H=32, E=16, A=32, c0=8, c1=16, V=31, drop=0.0)
    del mcfg["rnn_config"]["dec_vocab_size"]
    mcfg["rnn_config"]["ctc"] = True
    tcfg = {"seed": "seed-ast-20h", "gpuid": 0, "batch_size": 4, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 1,
            "optimizer": {"type": 0, "lr": 2e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0},
            "data": {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 8, "syn_dev": 6},
                     "frames": [60, 300], "targets": [2, 9], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w"}}
    json.dump(mcfg, open(tmp_path / "model_cfg.json", "w"))
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))
    out = str(tmp_path / "ctc_align.npz")
    r = subprocess.run([sys.executable, os.path.join(root, "score.py"), "-m", str(tmp_path), "-s", "syn_dev", "--ctc-alignments", out], cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "CTC alignments written to" in r.stdout and "Alignments written to: " not in r.stdout.replace("CTC alignments written to: ", "")
    from ast_amd import nn as N
    nn = N.NN(str(tmp_path))
    utts = sorted(nn.data_loader.info["syn_dev"])

    def check(z, names, labels_of):
        assert sorted(z.files) == sorted(n + "/" + k for n in names for k in N.ALIGNMENT_KEYS)
        for n in names:
            U = len(z[n + "/labels"])
            assert z[n + "/labels"].tolist() == labels_of(n) and z[n + "/segments"].shape == (U, 2) == z[n + "/segments_input"].shape
            assert z[n + "/confidence"].shape == (U,) and np.isfinite(z[n + "/score"]) and z[n + "/score"] <= z[n + "/total_logp"] + 1e-3
            seg = z[n + "/segments"]
            assert (seg[:, 0] < seg[:, 1]).all() and (seg[1:, 0] >= seg[:-1, 1]).all()
    with np.load(out) as z:
        check(z, utts, lambda u: [int(i) for i in nn.data_loader.ids["syn_dev"][u]][:10])
    beam = {u: [([1, 5, 6, 2], -1.0, []), ([1, 7, 2], -2.0, [])] for u in utts[:2]}
    out2 = str(tmp_path / "nbest_align.npz")
    assert N.write_alignment_file(nn, "syn_dev", {"ctc_alignments": out2}, beam) == out2
    with np.load(out2) as z:
        check(z, ["{0:s}#{1:d}".format(u, k) for u in utts[:2] for k in range(2)], lambda n: [[5, 6], [7]][int(n[-1])])
