"""Scored greedy decoding, the parts that need no GPU: the two entry points are exported with the argument types include/astk.h declares,
the workspace query follows the unscored one, and the host-side reduction of a scored decode (ast_amd.seq2seq.scored_from_rows /
ScoredPrediction: n_steps slicing, the dev loss, the per-row score with its first-EOS cut) against a NumPy restatement on hand-made rows."""
import ctypes as C
import re

import numpy as np

from conftest import ROOT

GO, EOS = 1, 2


def test_symbols_are_exported_with_the_declared_types():
    from ast_amd import _lib
    lib = _lib.load()
    res, args = _lib.SIGNATURES["astk_greedy_decode_scored"]
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    assert res is C.c_int
    assert args == [C.POINTER(_lib.DecoderDesc), C.POINTER(_lib.DecoderParams), vp, vp, vp, i, i, i, vp, i, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    assert lib.astk_greedy_decode_scored.argtypes == args and lib.astk_greedy_decode_scored.restype is C.c_int
    assert _lib.SIGNATURES["astk_greedy_scored_workspace_bytes"] == (sz, [C.POINTER(_lib.DecoderDesc), i])
    assert lib.astk_greedy_scored_workspace_bytes.restype is sz
    # the header's declaration, parameter by parameter
    text = open(ROOT + "/include/astk.h").read()
    m = re.search(r"int astk_greedy_decode_scored\((.*?)\);", text, re.S)
    names = [p.strip().split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
    assert names == ["d", "p", "enc", "c0", "h0", "go", "eos", "stop_limit", "y", "ldy", "class_weight", "tokens", "logp", "nll", "n_steps",
                     "status_dst", "ws", "ws_bytes", "stream"]
    assert len(names) == len(args)
    # the unscored entry keeps its signature
    assert len(_lib.SIGNATURES["astk_greedy_decode"][1]) == 14


def test_workspace_query_follows_the_unscored_one():
    from ast_amd import _lib
    lib = _lib.load()
    for desc, stop in (((32, 2, 200, 512, 128, 512, 1098, 3, 1, 0, 0), 175), ((32, 2, 200, 512, 128, 512, 1098, 1, 1, 0, 0), 40),
                       ((5, 2, 30, 64, 16, 64, 57, 2, 1, 0, 0), 24), ((32, 2, 420, 512, 128, 512, 1098, 3, 1, 0, 0), 512)):
        d = _lib.DecoderDesc(*desc)
        # (the device loop needs 256 compute units: on a machine without the GPU both queries answer 0)
        assert lib.astk_greedy_scored_workspace_bytes(C.byref(d), stop) == lib.astk_greedy_workspace_bytes(C.byref(d), stop)
    for desc, stop in (((32, 2, 200, 1024, 128, 1024, 1098, 1, 1, 0, 0), 175), ((48, 2, 200, 512, 128, 512, 1098, 3, 1, 0, 0), 175),
                       ((32, 2, 200, 512, 128, 512, 1098, 3, 1, 0, 0), 513), ((32, 2, 200, 512, 128, 512, 1098, 3, 1, 0, 0), 0)):
        d = _lib.DecoderDesc(*desc)
        assert lib.astk_greedy_scored_workspace_bytes(C.byref(d), stop) == 0
    bad = _lib.DecoderDesc(32, 2, 200, 512, 128, 512, 1098, 3, 1, 0, 0)
    bad.struct_size -= 8
    assert lib.astk_greedy_scored_workspace_bytes(C.byref(bad), 175) == 0


def _restate(tokens, logp, nll, n, B):
    """NumPy restatement, row by row and step by step."""
    loss = 0.0
    for s in range(n):
        loss += sum(float(nll[s, b]) for b in range(B)) / B
    score = []
    for b in range(B):
        k = n
        for s in range(n):
            if tokens[s, b] == EOS:
                k = s + 1
                break
        score.append(sum(float(logp[s, b]) for s in range(k)))
    return loss, np.array(score)


def _words(tokens, logp, nll):
    parts = [tokens.astype(np.int32).ravel(), logp.astype(np.float32).ravel().view(np.int32)]
    if nll is not None:
        parts.append(nll.astype(np.float32).ravel().view(np.int32))
    return np.concatenate(parts)


def test_host_reduction_matches_a_numpy_restatement():
    from ast_amd.seq2seq import ScoredPrediction, scored_from_rows
    rng = np.random.default_rng(0)
    for B, stop, n in ((5, 9, 6), (17, 12, 12), (1, 4, 1), (3, 7, 3)):            # B not a multiple of 16; n_steps below and at stop_limit
        tokens = rng.integers(3, 40, size=(stop, B)).astype(np.int32)
        tokens[n:] = -7                                                       # rows at and past n_steps: unspecified, never read
        if B >= 3:
            tokens[0, 1] = EOS                                                # a row whose first token is EOS (it keeps decoding)
            tokens[min(2, n - 1), 1] = EOS                                    # ... and emits it again: only the first one cuts
            tokens[n - 1, 2] = EOS                                            # a row that ends on the last step
            # row 0 never emits EOS
        logp = -rng.random((stop, B)).astype(np.float32) * 15
        nll = (rng.random((stop, B)) * 15).astype(np.float32)
        nll[:, B - 1] = 0.0                                                   # PAD targets weigh 0
        logp[n:], nll[n:] = np.nan, np.nan                                    # must not reach any sum
        r = scored_from_rows(_words(tokens, logp, nll), n, B, stop, True, EOS)
        assert isinstance(r, ScoredPrediction)
        assert r.n_steps == n and r.tokens.shape == r.logp.shape == r.nll.shape == (B, n)
        assert r.tokens.dtype == np.int32 and r.logp.dtype == np.float32 and r.nll.dtype == np.float32
        assert (r.tokens == tokens[:n].T).all() and (r.logp == logp[:n].T).all() and (r.nll == nll[:n].T).all()
        loss, score = _restate(tokens, logp, nll, n, B)
        assert isinstance(r.loss, float) and abs(r.loss - loss) <= 1e-12 * max(1.0, abs(loss)), (r.loss, loss)
        assert r.score.dtype == np.float64 and r.score.shape == (B,)
        assert np.abs(r.score - score).max() <= 1e-12 * max(1.0, np.abs(score).max())
        if B >= 3:
            assert r.score[1] == float(logp[0, 1])                            # first token EOS: one term
            assert abs(r.score[0] - float(logp[:n, 0].astype(np.float64).sum())) < 1e-12 * 15 * n      # never EOS: all n terms
        # without targets: no nll, no loss, the same tokens and scores
        r2 = scored_from_rows(_words(tokens, logp, None), n, B, stop, False, EOS)
        assert r2.nll is None and r2.loss is None
        assert (r2.tokens == r.tokens).all() and (r2.score == r.score).all()


def test_loss_is_summed_in_float64():
    """Terms whose float32 running sum would lose the small ones."""
    from ast_amd.seq2seq import ScoredPrediction
    B, n = 2, 4096
    nll = np.full((B, n), 1e-4, dtype=np.float32)
    nll[0, 0] = 4096.0
    tokens = np.full((B, n), 5, dtype=np.int32)
    r = ScoredPrediction(tokens, -nll, nll, EOS)
    want = (4096.0 + (2 * n - 1) * float(np.float32(1e-4))) / B
    assert abs(r.loss - want) < 1e-9 * want
    assert abs(r.score[1] + n * float(np.float32(1e-4))) < 1e-12 * n
