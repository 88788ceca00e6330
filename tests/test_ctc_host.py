"""Host tests of the auxiliary CTC loss: the NumPy model of tests/ctc_model.py against an independent
implementation (torch.nn.functional.ctc_loss on float64 log-softmax inputs, CPU), the float32 figures the operator's bounds are taken
from, the wrapped oracle's gradients by finite differences, and the host logic: parameter shapes, argument checks, the loader's
`x_len`, the configuration keys, the ABI mirror and the descriptor refusals."""
import ctypes as C
import inspect
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import ctc_model as CM
from conftest import ROOT, tiny_cfg


# ------------------------------------------------------------------ 1. the model
@pytest.mark.parametrize("name", list(CM.OP_CASES))
def test_model_is_torch_ctc_loss(name):
    """Loss rows and the gradient with respect to the logits agree with torch's CTC (autograd through log_softmax) to 1e-10; rows
    without a path are +inf in the model and 0 with zero gradient under zero_infinity=True."""
    x, y, lens = CM.op_case(name)
    B, T, V = x.shape
    m = CM.ctc_loss_grad(x.astype(np.float64), y, lens)
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    labs = [CM.labels_of(y[b], CM.UNK_ID, V) for b in range(B)]
    il = torch.tensor([T] * B if lens is None else [int(v) for v in lens])
    loss = torch.nn.functional.ctc_loss(torch.log_softmax(xt, 2).transpose(0, 1), torch.tensor([i for l in labs for i in l], dtype=torch.long),
                                        il, torch.tensor([len(l) for l in labs]), blank=CM.PAD_ID, reduction="none", zero_infinity=True)
    loss.sum().backward()
    want, grad = loss.detach().numpy(), xt.grad.numpy()
    bad = np.isinf(m["row_nll"])
    assert bad.sum() == m["n_infeasible"] == sum(not CM.feasible(l, int(n)) for l, n in zip(labs, il))
    assert (want[bad] == 0).all()
    assert np.abs(m["row_nll"][~bad] - want[~bad]).max(initial=0.0) <= 1e-10
    assert np.abs(m["dlogits"] - grad).max() <= 1e-10
    assert abs(m["loss"] - want.sum()) <= 1e-10 * max(1.0, want.sum())
    if name == "u255-infeasible-between":
        assert bad.tolist() == [False, True, False]
    if name in ("v1098-one-path", "all-equal-one-path", "u64-one-path"):         # T = U + repeats: the one path's probability
        b = 1 if name == "v1098-one-path" else 0
        logp = torch.log_softmax(xt, 2).detach().numpy()[b]
        z = labs[b]
        path = [z[0]] + [c for p, c in zip(z[:-1], z[1:]) for c in (([CM.PAD_ID, c]) if p == c else [c])]
        assert len(path) == T
        assert abs(m["row_nll"][b] + logp[np.arange(T), path].sum()) <= 1e-10


def test_float32_model_error_is_what_the_bounds_were_taken_from():
    """The model in float32 against itself in float64, per case family: the recorded figure still describes the cases -- the error
    lies between half of it and 1.25 times it (NumPy's float32 exp / log differ in the last bit between builds; a figure far off
    either way would make the operator's bound arbitrary)."""
    worst = {}
    for name, c in CM.OP_CASES.items():
        x, y, lens = CM.op_case(name)
        a = CM.ctc_loss_grad(x.astype(np.float64), y, lens)
        b = CM.ctc_loss_grad(x, y, lens, dtype=np.float32)
        assert b["dlogits"].dtype == np.float32 and np.isinf(a["row_nll"]).tolist() == np.isinf(b["row_nll"]).tolist()
        ok = ~np.isinf(a["row_nll"])
        assert (np.abs(b["row_nll"][ok] - a["row_nll"][ok]) <= 1e-6 * a["row_nll"][ok]).all()
        worst[c["family"]] = max(worst.get(c["family"], 0.0), float(np.abs(b["dlogits"] - a["dlogits"]).max()))
    print(worst)
    assert set(worst) == set(CM.F32_MODEL_ERR)
    for fam, fig in CM.F32_MODEL_ERR.items():
        assert 0.5 * fig <= worst[fam] <= 1.25 * fig, (fam, worst[fam], fig)


def test_model_handles_dead_states_and_the_empty_label_row():
    """U = 0 is the all-blank path; logits at +-30 and a float32 run give no NaN (all -inf terms in the three-way log-add)."""
    x = CM.op_logits("normal", 1, 4, 5, 3).astype(np.float64)
    y = np.zeros((1, 3), np.int32)
    m = CM.ctc_loss_grad(x, y)
    logp = x[0] - np.log(np.exp(x[0]).sum(-1, keepdims=True))
    assert abs(m["row_nll"][0] + logp[:, 0].sum()) < 1e-12
    for kind in ("offset+", "offset-", "peaked"):
        r = CM.ctc_loss_grad(CM.op_logits(kind, 2, 9, 57, 1), np.array([[1, 7, 7, 2], [1, 9, 2, 0]], np.int32), dtype=np.float32)
        assert np.isfinite(r["row_nll"]).all() and np.isfinite(r["dlogits"]).all()
        assert np.abs(r["dlogits"].sum(-1)).max() < 1e-4
    assert CM.collapse([0, 5, 5, 0, 5, 7, 7, 0]) == [5, 5, 7]


def test_wrapped_oracle_passes_directional_finite_differences():
    """The float64 oracle with the CTC term: d loss along a random direction of every parameter group against central differences."""
    from oracle import ast_ref as R
    cfg = tiny_cfg(c1=8)
    cfg["rnn_config"]["ctc"] = True
    B, T, D, L, V = 3, 21, 26, 6, 11
    P = R.init_params(cfg, D, V, seed=0, dtype=np.float64)
    P.update(CM.head_params(cfg["rnn_config"]["hidden_units"], V, dtype=np.float64))
    X, y = R.synth_batch(B, T, D, L, V, seed=1, dtype=np.float64)
    x_lens = [21, 17, 13]

    def loss_of(params):
        m = R.RefModel(cfg, {k: v.copy() for k, v in params.items()}, V)
        with CM.ctc_oracle(0.3, x_lens):
            return m, m.forward_loss(X, y, 1.0, pyrandom=random.Random(1))
    m, loss = loss_of(P)
    assert m.ctc_infeasible == 0 and m.ctc_term > 0
    plain = R.RefModel(cfg, {k: v.copy() for k, v in P.items()}, V).forward_loss(X, y, 1.0, pyrandom=random.Random(1))
    assert abs(float(loss.data) - float(plain.data) - m.ctc_term) < 1e-12
    m.cleargrads()
    loss.backward()
    grads = {k: p.grad for k, p in m.params()}
    rng = np.random.default_rng(4)
    for name in ("ctc_out/W", "ctc_out/b", "L1_enc/upward/W", "L0_rev_enc/lateral/W", "CNN_1/W"):
        d = rng.standard_normal(P[name].shape)
        h = 1e-5
        up, dn = dict(P), dict(P)
        up[name], dn[name] = P[name] + h * d, P[name] - h * d
        fd = (float(loss_of(up)[1].data) - float(loss_of(dn)[1].data)) / (2 * h)
        an = float((grads[name] * d).sum())
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)), (name, fd, an)
    # weight 0, or a model without the head: the oracle as it is, bit for bit
    with CM.ctc_oracle(0.0):
        z = R.RefModel(cfg, {k: v.copy() for k, v in P.items()}, V).forward_loss(X, y, 1.0, pyrandom=random.Random(1))
    assert float(z.data) == float(plain.data)


# ------------------------------------------------------------------ 2. host logic
NAMES_WITHOUT_THE_KEY = [
    "CNN_0/W", "CNN_0_bn/gamma", "CNN_0_bn/beta", "CNN_1/W", "CNN_1_bn/gamma", "CNN_1_bn/beta",
    "L0_enc/upward/W", "L0_enc/upward/b", "L0_enc/lateral/W", "L1_enc/upward/W", "L1_enc/upward/b", "L1_enc/lateral/W",
    "L0_rev_enc/upward/W", "L0_rev_enc/upward/b", "L0_rev_enc/lateral/W", "L1_rev_enc/upward/W", "L1_rev_enc/upward/b", "L1_rev_enc/lateral/W",
    "attn_Wa/W", "attn_Wa/b", "context/W", "context/b", "embed_dec/W",
    "L0_dec/upward/W", "L0_dec/upward/b", "L0_dec/lateral/W", "L1_dec/upward/W", "L1_dec/upward/b", "L1_dec/lateral/W", "out/W", "out/b"]


def test_param_shapes_append_exactly_the_head():
    from ast_amd.params import ParamArena, init_values, param_shapes
    cfg = tiny_cfg()
    for off in (cfg, {**cfg, "rnn_config": {**cfg["rnn_config"], "ctc": False}}):
        train, persist = param_shapes(off, 26, 11)
        assert list(train) == NAMES_WITHOUT_THE_KEY
    on = {**cfg, "rnn_config": {**cfg["rnn_config"], "ctc": True}}
    train_on, persist_on = param_shapes(on, 26, 11)
    assert list(train_on) == NAMES_WITHOUT_THE_KEY + ["ctc_out/W", "ctc_out/b"] and persist_on == persist
    assert train_on["ctc_out/W"] == (11, 8) and train_on["ctc_out/b"] == (11,)
    a0, a1 = ParamArena(train, torch.device("cpu")), ParamArena(train_on, torch.device("cpu"))
    assert all(a1.offsets[k] == a0.offsets[k] for k in train) and a1.offsets["ctc_out/W"] == a0.size
    v0, v1 = init_values(cfg, 26, 11, seed=3), init_values(on, 26, 11, seed=3)
    assert all(np.array_equal(v0[k], v1[k]) for k in v0)                       # every other initial value is what it was
    assert abs(v1["ctc_out/W"].std() - 1 / np.sqrt(8)) < 0.1 and not v1["ctc_out/b"].any()      # the reference's Linear initialiser
    from ast_amd import dist
    src = inspect.getsource(dist)
    assert '"enc" if is_enc else "dec"' in src                                 # (the head falls into the `dec` gradient range)


BAD = [-0.1, float("nan"), float("inf"), "0.3", None, True]


def test_checked_ctc_weight():
    from ast_amd.seq2seq import SpeechEncoderDecoder, checked_ctc_weight
    assert checked_ctc_weight(0, False) == 0.0 and checked_ctc_weight(np.float32(0.5), True) == 0.5 and checked_ctc_weight(3, True) == 3.0
    for bad in BAD:
        with pytest.raises(ValueError):
            checked_ctc_weight(bad, True)
    with pytest.raises(ValueError, match="rnn_config.ctc"):
        checked_ctc_weight(0.3, False)
    p = inspect.signature(SpeechEncoderDecoder.forward_loss).parameters
    names = list(p)
    assert names[names.index("label_smoothing") + 1:] == ["ctc_weight", "x_lens"] and p["ctc_weight"].default == 0.0 and p["x_lens"].default is None


@pytest.mark.parametrize("bad", BAD + [0.3], ids=repr)
def test_forward_loss_refuses_before_it_touches_the_library(bad, monkeypatch):
    """A bad weight -- or a good one on a model without the head -- is refused in front of everything else."""
    from ast_amd import _lib
    from ast_amd.seq2seq import SpeechEncoderDecoder
    m = SpeechEncoderDecoder(None, tiny_cfg())

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(m, "encode", touched)
    X, y = np.zeros((1, 16, 8), np.float32), np.array([[1, 5, 2]], np.int32)
    with pytest.raises(ValueError, match="ctc_weight"):
        m.forward_loss(X, y, 1.0, ctc_weight=bad)
    assert "off" in m.paths()["ctc"] and "nothing is launched" in m.paths()["ctc"]


def test_checked_x_lens():
    from ast_amd.seq2seq import checked_x_lens, cnn_out_lens
    assert checked_x_lens(np.array([5, 9], np.int32), 2, 9).tolist() == [5, 9]
    for bad in (np.array([5, 10]), np.array([0, 9]), np.array([5.0, 9.0]), np.array([5]), np.array([[5, 9]])):
        with pytest.raises(ValueError):
            checked_x_lens(bad, 2, 9)
    layers = tiny_cfg()["cnn_config"]["cnn_layers"]
    assert [cnn_out_lens(layers, n)[-1] for n in (120, 101, 77, 64)] == CM.t2_lens(layers, [120, 101, 77, 64]).tolist()


def _data():
    return {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 21, "syn_dev": 5},
            "frames": [20, 400], "targets": [1, 30], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
            "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w"}


def test_loader_yields_x_len_only_when_asked(tmp_path):
    from ast_amd.dataloader import SyntheticDataLoader
    dl = SyntheticDataLoader(_data(), str(tmp_path), -1)
    assert dl.keep_lens is False
    random.seed("s")
    plain = list(dl.get_batch(8, "syn_train", train=True, labels=True))
    assert all(sorted(b) == ["X", "utts", "y"] for b in plain)
    dl = SyntheticDataLoader(_data(), str(tmp_path), -1)              # (a fresh one: an epoch shuffles the loader's buckets in place)
    dl.keep_lens = True
    random.seed("s")
    kept = list(dl.get_batch(8, "syn_train", train=True, labels=True))
    assert len(kept) == len(plain)
    for a, b in zip(plain, kept):
        assert sorted(b) == ["X", "utts", "x_len", "y"] and a["utts"] == b["utts"] and torch.equal(a["X"], b["X"])
        xl = b["x_len"]
        assert isinstance(xl, np.ndarray) and xl.dtype == np.int32 and xl.shape == (len(b["utts"]),)
        assert xl.tolist() == [min(int(dl.info["syn_train"][u]["sp"]), 400) for u in b["utts"]] and xl.max() == b["X"].shape[1]
    assert all("x_len" not in b for b in dl.get_batch(8, "syn_dev", train=False, labels=True))      # evaluation batches never carry it
    src = inspect.getsource(SyntheticDataLoader.get_batch)
    assert src.count('out["x_len"]') == 2                                      # the host-tensor path and the device path


@pytest.mark.parametrize("weight,head", [(w, True) for w in BAD if w is not None] + [(0.3, False)], ids=repr)
def test_nn_refuses_a_bad_extras_ctc_weight(weight, head, tmp_path):
    """extras.ctc_weight is checked when the experiment directory is read, in front of the loader and the model; a positive weight
    needs rnn_config.ctc."""
    from ast_amd.nn import NN
    mcfg = tiny_cfg()
    del mcfg["rnn_config"]["dec_vocab_size"]
    mcfg["rnn_config"]["ctc"] = head
    tcfg = {"seed": "s", "gpuid": 0, "batch_size": 4, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 1,
            "optimizer": {"type": 0, "lr": 1e-3, "l2": 0, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0, "ctc_weight": weight},
            "data": {**_data(), "vocab_size": 11}}
    json.dump(mcfg, open(tmp_path / "model_cfg.json", "w"))
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))
    with pytest.raises(ValueError, match="extras.ctc_weight"):
        NN(str(tmp_path))


def test_train_py_and_nn_read_extras_ctc_weight():
    from ast_amd import nn
    src = inspect.getsource(nn.NN)
    assert '.get("ctc_weight", 0.0)' in src and "keep_lens = True" in src and 'batch.get("x_len")' in src
    train = open(os.path.join(ROOT, "train.py")).read()
    assert "nn.ctc_epoch" in train and "CTC term" in train
    for tool in ("score.py", "sample.py", "beam.py"):                          # evaluation does not know the key
        assert "ctc" not in open(os.path.join(ROOT, tool)).read()


def test_symbols_are_declared_listed_and_exported():
    from ast_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "astk.h")).read()
    names = ["astk_ctc_workspace_bytes", "astk_ctc_loss", "astk_ctc_greedy", "astk_ctc_head_fwd", "astk_ctc_head_bwd"]
    for lib_path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        lib = C.CDLL(lib_path)
        for n in names:
            assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.SIGNATURES
            assert isinstance(getattr(lib, n), C._CFuncPtr)
    assert re.search(r"#define ASTK_CTC_MAX_LABELS (\d+)", hdr).group(1) == str(_lib.CTC_MAX_LABELS) == "255"
    fields = re.search(r"typedef struct \{([^}]*)\} astk_ctc_desc;", hdr).group(1)
    declared = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields))
    assert declared == [f[0] for f in _lib.CtcDesc._fields_]
    assert " ctc" in open(os.path.join(ROOT, "ast_amd", "csrc", "build.sh")).read().split("SRCS=")[1].split("\n")[0]


def test_descriptor_refusals_need_no_device():
    """Every refusal comes from the descriptor alone: with null pointers and no stream the calls fail with their message, and a good
    descriptor's workspace holds alpha and the emissions, 2 T (2L + 1) floats per row, and little else."""
    from ast_amd import _lib
    lib = _lib.load()
    good = dict(B=2, T=4, V=7, ldv=8, L=3, ldy=3, first_label=3, blank=0)
    for field, value, word in (("V", 1, "V"), ("blank", 7, "blank"), ("blank", -1, "blank"), ("first_label", 0, "first_label"), ("B", 0, "B"),
                               ("T", -1, "T"), ("L", 0, "L"), ("L", 256, "labels"), ("ldv", 6, "ldv"), ("ldy", 2, "ldy")):
        d = _lib.CtcDesc(**{**good, field: value})
        if field == "L":
            d.ldy = max(value, 1)
        assert lib.astk_ctc_workspace_bytes(C.byref(d)) == 0 and word in lib.astk_last_error().decode()
        assert lib.astk_ctc_loss(C.byref(d), None, None, None, 1.0, None, None, None, None, None, 0, None) != 0
        assert word in lib.astk_last_error().decode(), (field, lib.astk_last_error().decode())
        assert lib.astk_ctc_greedy(C.byref(d), None, None, None, None) != 0 and word in lib.astk_last_error().decode()
    d = _lib.CtcDesc(**good)
    d.struct_size -= 4
    assert lib.astk_ctc_workspace_bytes(C.byref(d)) == 0 and "struct_size" in lib.astk_last_error().decode()
    d = _lib.CtcDesc(32, 420, 8004, 8004, 177, 177, 3, 0)
    need = lib.astk_ctc_workspace_bytes(C.byref(d))
    floor = 2 * 32 * 420 * (2 * 177 + 1) * 4
    assert floor < need < floor + (1 << 20)
    assert lib.astk_ctc_loss(C.byref(_lib.CtcDesc(**good)), None, None, None, 1.0, None, None, None, None, None, 0, None) != 0
    assert "null" in lib.astk_last_error().decode()
    assert lib.astk_ctc_head_bwd(0, 7, 8, None, 8, None, None, None, None, None, 0, 0, None) != 0
    assert lib.astk_ctc_head_fwd(4, 7, 8, None, None, None, None, 8, 9, None) != 0
