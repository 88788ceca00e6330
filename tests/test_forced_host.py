"""Forced decoding, the parts that need no GPU: the two entry points are exported with the argument types include/astk.h declares, the
workspace query answers 0 where the greedy one does, the host-side assembly of a ForcedScore from raw read-back rows
(ast_amd.seq2seq.forced_from_rows: weight, score, n_tokens, loss with PAD positions and an all-PAD row) against hand-made numbers, and
the host check of the token ids."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT


def test_symbols_are_exported_with_the_declared_types():
    from ast_amd import _lib
    lib = _lib.load()
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    res, args = _lib.SIGNATURES["astk_forced_score"]
    assert res is C.c_int
    assert args == [C.POINTER(_lib.DecoderDesc), C.POINTER(_lib.DecoderParams), vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, sz, vp]
    assert lib.astk_forced_score.argtypes == args and lib.astk_forced_score.restype is C.c_int
    assert _lib.SIGNATURES["astk_forced_workspace_bytes"] == (sz, [C.POINTER(_lib.DecoderDesc), i, i])
    assert lib.astk_forced_workspace_bytes.restype is sz and lib.astk_forced_workspace_bytes.argtypes == [C.POINTER(_lib.DecoderDesc), i, i]
    # the header's declarations, parameter by parameter
    text = open(ROOT + "/include/astk.h").read()
    names = lambda m: [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
    got = names(re.search(r"int astk_forced_score\((.*?)\);", text, re.S))
    assert got == ["d", "p", "enc", "c0", "h0", "y", "ldy", "logp", "logp_max", "pred", "alpha", "status_dst", "ws", "ws_bytes", "stream"]
    assert len(got) == len(args)
    assert names(re.search(r"size_t astk_forced_workspace_bytes\((.*?)\);", text, re.S)) == ["d", "n_steps", "with_alpha"]
    # the neighbours keep their signatures
    assert len(_lib.SIGNATURES["astk_greedy_decode"][1]) == 14 and len(_lib.SIGNATURES["astk_greedy_decode_scored"][1]) == 19


def test_workspace_query_answers_zero_where_the_greedy_one_does():
    """Without a device every query answers 0, so here this checks the call, its three arguments and the refusals; the byte counts of
    the alpha part are checked where the device loop runs (tests/test_gpu_forced.py, the bad-argument test)."""
    from ast_amd import _lib
    lib = _lib.load()
    for desc, S in (((32, 2, 200, 512, 128, 512, 1098, 3, 1, 0, 0), 175), ((32, 2, 200, 512, 128, 512, 1098, 1, 1, 0, 0), 39),
                    ((5, 2, 30, 64, 16, 64, 57, 2, 1, 0, 0), 24), ((32, 2, 420, 512, 128, 512, 1098, 3, 1, 0, 0), 512)):
        d = _lib.DecoderDesc(*desc)
        # (the device loop needs 256 compute units: on a machine without the GPU every query answers 0)
        g = lib.astk_greedy_workspace_bytes(C.byref(d), S)
        plain, with_alpha = lib.astk_forced_workspace_bytes(C.byref(d), S, 0), lib.astk_forced_workspace_bytes(C.byref(d), S, 1)
        assert plain == g
        if g:
            B, T = desc[0], desc[2]
            assert with_alpha >= g + 4 * S * B * (T + 2) and with_alpha <= g + 4 * S * B * ((T + 3) // 4 * 4 + 2) + 512
        else:
            assert with_alpha == 0
    for desc, S in (((32, 2, 200, 1024, 128, 1024, 1098, 1, 1, 0, 0), 175), ((48, 2, 200, 512, 128, 512, 1098, 3, 1, 0, 0), 175),
                    ((32, 2, 200, 512, 128, 512, 1098, 3, 1, 0, 0), 513), ((32, 2, 200, 512, 128, 512, 1098, 3, 1, 0, 0), 0)):
        d = _lib.DecoderDesc(*desc)
        assert lib.astk_forced_workspace_bytes(C.byref(d), S, 0) == 0 and lib.astk_forced_workspace_bytes(C.byref(d), S, 1) == 0
    bad = _lib.DecoderDesc(32, 2, 200, 512, 128, 512, 1098, 3, 1, 0, 0)
    bad.struct_size -= 8
    assert lib.astk_forced_workspace_bytes(C.byref(bad), 175, 1) == 0


def test_forced_score_from_hand_made_rows():
    """B = 3, S = 4.  Row 0: no PAD.  Row 1: PAD at target positions 1 and 3.  Row 2: every target PAD.  All values are exact binary
    fractions, so the expected sums are exact."""
    from ast_amd.seq2seq import ForcedScore, forced_from_rows
    B, S = 3, 4
    y = np.array([[1, 5, 6, 7, 2],
                  [1, 9, 0, 8, 0],
                  [1, 0, 0, 0, 0]], dtype=np.int32)
    logp = np.array([[-1.0, -2.0, -0.5, -4.0],          # (B, S)
                     [-0.25, -8.0, -1.5, -16.0],
                     [-3.0, -3.0, -3.0, -3.0]], dtype=np.float32)
    logp_max = logp / 2
    pred = np.arange(B * S, dtype=np.int32).reshape(B, S) + 3
    weight = (y[:, 1:] != 0).astype(np.float32)
    words = np.concatenate([logp.T.ravel().view(np.int32), logp_max.T.ravel().view(np.int32), pred.T.ravel(),
                            np.full(5, -7, dtype=np.int32)])            # (trailing words of a pooled buffer: never read)
    r = forced_from_rows(words, B, S, weight)
    assert isinstance(r, ForcedScore)
    assert r.logp.shape == r.logp_max.shape == r.pred.shape == r.weight.shape == (B, S)
    assert r.logp.dtype == np.float32 and r.logp_max.dtype == np.float32 and r.pred.dtype == np.int32 and r.weight.dtype == np.float32
    assert (r.logp == logp).all() and (r.logp_max == logp_max).all() and (r.pred == pred).all()
    assert (r.weight == np.array([[1, 1, 1, 1], [1, 0, 1, 0], [0, 0, 0, 0]], dtype=np.float32)).all()
    assert r.score.dtype == np.float64 and r.score.tolist() == [-7.5, -1.75, 0.0]
    assert r.n_tokens.tolist() == [4, 2, 0]
    # loss = sum over steps of (1 / B) sum over rows of weight * (-logp): steps (1 + 0.25) / 3 + 2 / 3 + (0.5 + 1.5) / 3 + 4 / 3
    assert isinstance(r.loss, float) and abs(r.loss - 9.25 / 3) < 1e-15
    assert r.alpha is None
    alpha = np.random.default_rng(0).random((B, S, 7)).astype(np.float32)
    assert forced_from_rows(words, B, S, weight, alpha).alpha is alpha


def test_sums_are_float64():
    from ast_amd.seq2seq import ForcedScore
    B, S = 2, 4096
    logp = np.full((B, S), -1e-4, dtype=np.float32)
    logp[0, 0] = -4096.0
    r = ForcedScore(logp, logp, np.zeros((B, S), dtype=np.int32), np.ones((B, S), dtype=np.float32))
    small = float(np.float32(1e-4))
    assert abs(r.score[0] + 4096.0 + (S - 1) * small) < 1e-9 * 4096 and abs(r.score[1] + S * small) < 1e-12 * S
    want = (4096.0 + (2 * S - 1) * small) / B
    assert abs(r.loss - want) < 1e-9 * want


def test_token_ids_outside_the_vocabulary_raise_before_any_launch(monkeypatch):
    from conftest import tiny_cfg
    from ast_amd import _lib
    from ast_amd.seq2seq import SpeechEncoderDecoder, checked_targets
    V = 57
    ok = np.array([[1, 5, 0, 56], [1, 2, 0, 0]], dtype=np.int64)
    assert checked_targets(ok, V).dtype == np.int32 and (checked_targets(ok, V) == ok).all()
    for bad in (np.array([[1, 5, V, 2]]), np.array([[1, -1, 3, 2]]), np.array([[1]]), np.array([1, 2, 3]), np.array([[1.0, 2.0]])):
        with pytest.raises(ValueError):
            checked_targets(bad, V)
    # through the model: no library call, no encode
    cfg = tiny_cfg()
    cfg["rnn_config"]["dec_vocab_size"] = V
    m = SpeechEncoderDecoder(None, cfg)

    def touched(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "load", touched)
    monkeypatch.setattr(m, "encode", touched)
    X = np.zeros((1, 16, 8), dtype=np.float32)
    for call in (m.score, m.score_async):
        with pytest.raises(ValueError, match="token ids"):
            call(X, np.array([[1, 5, V, 2]], dtype=np.int32))
        with pytest.raises(ValueError, match="token ids"):
            call(X, np.array([[1, -3, 4, 2]], dtype=np.int32), return_alpha=True)
