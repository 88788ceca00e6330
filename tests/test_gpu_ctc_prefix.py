"""Joint CTC-attention beam search (ast_amd.nn.decode_beam_batch(ctc_weight=), csrc/ctc_prefix.hip, csrc/beam.hip; DESIGN.md section
30): the prefix scorer -- the shipped wavefront kernel and the plain serial one -- against the float64 model of tests/ctc_prefix_model.py
and against each other, one joint selection step against the model's, whole searches against the host joint search driven by the GPU
model's own per-hypothesis steps, an independent cross-check of every finished hypothesis, and beam.py --ctc-weight.

The bound on psi and the CTC state entries is 1e-10 * max(1, |value|): a recursion of at most 512 frames commits a few float64 ulp
(2.2e-16) per step relative to magnitudes no larger than |psi|, about 5e-13; the bound leaves 200x for another composition order (the
wavefront scan) and the device's exp / log.  -inf must match exactly."""
import copy
import ctypes as C
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import ctc_model as CM
import ctc_prefix_model as PM
import decode_helpers as DH
from conftest import tiny_cfg

pytestmark = pytest.mark.gpu

GO, EOS = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any(), what
    inf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), inf), (what, "-inf pattern")
    err = np.abs(np.where(inf, 0.0, got) - np.where(inf, 0.0, want))
    bound = 1e-10 * np.maximum(1.0, np.abs(np.where(inf, 0.0, want)))
    assert (err <= bound).all(), (what, float((err / bound).max()))


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _alpha_state(x, labels, blank=0):
    """The state of the prefix `labels` from the CTC forward variables over its extended sequence (tests/ctc_model.py's recursion,
    vectorised over the states): r_n = alpha of the last label, r_b = alpha of the blank behind it."""
    T, n = x.shape[0], len(labels)
    if n == 0:
        return PM.empty_state(x, blank)
    S = 2 * n + 1
    z = np.full(S, blank, np.int64)
    z[1::2] = labels
    skip = np.zeros(S, bool)
    skip[3::2] = z[3::2] != z[1:-2:2]
    e = x[:, z]
    prev = np.full(S, -np.inf)
    prev[0] = 0.0
    out = np.full((T, 2), -np.inf)
    for t in range(T):
        a1 = np.concatenate(([-np.inf], prev[:-1]))
        a2 = np.where(skip, np.concatenate(([-np.inf, -np.inf], prev[:-2])), -np.inf)
        prev = PM.lae(PM.lae(prev, a1), a2) + e[t]
        out[t] = prev[S - 2], prev[S - 1]
    return out


class _Search:
    """The device buffers of a search of U utterances (lens), N slots, K proposals over CTC logits (U, Tmax, V) float32."""

    def __init__(self, L, lens, N, K, V, ctc_logits, w=0.3, S=2, nl=1, H=8, A=8):
        U, T = len(lens), max(lens)
        R = U * N
        dev = "cuda"
        i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
        self.U, self.N, self.K, self.V, self.T, self.R, self.nl, self.H, self.A = U, N, K, V, T, R, nl, H, A
        self.lens = np.asarray(lens, np.int32)
        self.st = dict(row_utt=torch.arange(R, **i32) // N, row_len=torch.tensor(np.repeat(self.lens, N), **i32),
                       c=torch.randn(nl, R, H, device=dev), h=torch.randn(nl, R, H, device=dev), ht=torch.randn(R, A, device=dev),
                       tokens=torch.full((R,), GO, **i32), score=torch.zeros(R, **f64), status=torch.zeros(R, **i32),
                       frozen=torch.zeros(U, **i32), n_frozen=torch.zeros(1, **i32), hist=torch.zeros(S, R, 4, **i32),
                       hist_alpha=torch.zeros(S, R, T, device=dev))
        self.bd = L.BeamDesc(U, N, K, S, T, V, EOS, self.lens.ctypes.data_as(C.POINTER(C.c_int32)))
        keys = ("row_utt", "row_len", "c", "h", "ht", "tokens", "score", "status", "frozen", "n_frozen", "hist", "hist_alpha")
        self.bs = L.BeamState(*[self.st[k].data_ptr() for k in keys])
        self.Vp = (V + 3) // 4 * 4 + 4                       # (a row stride that is not V)
        lg = torch.full((U, T, self.Vp), float("nan"), device=dev)          # the padding columns and the frames behind T''_u are never read
        for u in range(U):
            lg[u, :lens[u], :V] = torch.from_numpy(ctc_logits[u, :lens[u]])
        self.logits = lg
        self.state = torch.full((R, T, 2), float("nan"), **f64)
        self.att, self.psi, self.nlab = torch.full((R,), 9.0, **f64), torch.full((R,), 9.0, **f64), torch.full((R,), 9, **i32)
        self.bc = L.BeamCtc(w, 0, 3, lg.data_ptr(), self.Vp, self.state.data_ptr(), self.att.data_ptr(), self.psi.data_ptr(),
                            self.nlab.data_ptr(), None, 0)
        lib = L.load()
        nbytes = int(lib.astk_beam_ctc_workspace_bytes(C.byref(self.bd), C.byref(self.bc)))
        assert nbytes > 0, lib.astk_last_error()
        self.ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.bc.ws, self.bc.ws_bytes = self.ws.data_ptr(), nbytes
        L.check(lib.astk_beam_ctc_init(C.byref(self.bd), C.byref(self.bs), C.byref(self.bc), _stream()))

    def set_slots(self, slots):
        """slots[r] = dict(status, token, score, att, psi, n, state (T_u, 2) or None) -> the device buffers."""
        R, T = self.R, self.T
        state = np.full((R, T, 2), np.nan)
        for r, s in enumerate(slots):
            if s["state"] is not None:
                state[r, :s["state"].shape[0]] = s["state"]
        self.state.copy_(torch.from_numpy(state))
        for name, key, dt in (("tokens", "token", np.int32), ("score", "score", np.float64), ("status", "status", np.int32)):
            self.st[name].copy_(torch.from_numpy(np.asarray([s[key] for s in slots], dt)))
        self.att.copy_(torch.from_numpy(np.asarray([s["att"] for s in slots], np.float64)))
        self.psi.copy_(torch.from_numpy(np.asarray([s["psi"] for s in slots], np.float64)))
        self.nlab.copy_(torch.from_numpy(np.asarray([s["n"] for s in slots], np.int32)))


# ---------------------------------------------------------------- 1. the scorer: both kernels against the model and each other
LENS = [1, 3, 23, 64, 65, 300]          # T'' per utterance: below, at and across the lane-slice boundaries of a 64-lane wavefront
KINDS = ["normal", "offset+", "peaked", "offset-"]


def _prefix(rng, V, want_len, T):
    """Labels of a prefix: no adjacent repeats where the prefix should still have a path (length T: exactly one)."""
    labs, prev = [], -1
    for _ in range(want_len):
        c = int(rng.integers(3, V))
        if c == prev:
            c = 3 + (c - 3 + 1) % (V - 3)
        labs.append(c)
        prev = c
    return labs


@pytest.mark.parametrize("N,K", [(1, 1), (3, 4), (16, 16)])
@pytest.mark.parametrize("V", [6, 45, 57, 1098])
def test_prefix_scores_of_both_kernels_match_the_model(V, N, K):
    from ast_amd import _lib as L
    case = [6, 45, 57, 1098].index(V) + [(1, 1), (3, 4), (16, 16)].index((N, K))
    K = min(K, V)                                 # (a search proposes at most V tokens: the library refuses K > V, so V = 6 runs (16, 6))
    kind = KINDS[case % 4]                        # every value family of ctc_model.op_logits occurs for every (N, K) and for every V
    rng = np.random.default_rng(1000 * V + N)
    U, T = len(LENS), max(LENS)
    ctc_logits = CM.op_logits(kind, U, T, V, seed=V + N)
    xs = [PM.log_softmax64(ctc_logits[u, :LENS[u]]) for u in range(U)]
    with L.load_test_hooks() as lib:
        s = _Search(L, LENS, N, K, V, ctc_logits)
        torch.cuda.synchronize()
        # ---- the init: the empty prefix in slot 0 of every utterance, zeros in every slot's scalars
        st0 = s.state.cpu().numpy()
        for u in range(U):
            _close(st0[u * N, :LENS[u]], PM.empty_state(xs[u]), ("empty", u))
        assert (s.att.cpu() == 0).all() and (s.psi.cpu() == 0).all() and (s.nlab.cpu() == 0).all()
        # ---- slots: prefixes of 0, 1, T'', T'' + 1 (no path) and a few labels; one slot that is not live
        slots, cands = [], np.zeros((U * N, K), np.int32)
        for u in range(U):
            Tu = LENS[u]
            for j in range(N):
                r = u * N + j
                n = [0, 1, Tu, Tu + 1, min(Tu, 4)][(u + j) % 5]
                labs = _prefix(rng, V, n, Tu)
                last = labs[-1] if labs else GO
                live = not (N >= 3 and r == 4)
                slots.append(dict(status=1 if live else 2, token=last, score=0.0, att=0.0, psi=0.0, n=n, state=_alpha_state(xs[u], labs)))
                # PAD, GO, EOS, a repeat of the last label and ordinary labels: all in one call (K = 1: one kind per row in turn)
                special = [0, GO, EOS, last if n else 3, int(rng.integers(3, V))]
                pool = special[(r % 5):] + special[:(r % 5)] + [int(c) for c in rng.integers(3, V, size=K)]
                cands[r] = pool[:K]
        assert {0, GO, EOS} <= set(cands.ravel().tolist()) and any(cands[r, k] == slots[r]["token"] and slots[r]["n"] > 0
                                                                    for r in range(U * N) for k in range(K))
        assert {sl["n"] - LENS[r // N] for r, sl in enumerate(slots)} >= {0, 1} and {sl["n"] for sl in slots} >= {0, 1}
        s.set_slots(slots)
        cand_dev = torch.from_numpy(cands).cuda()
        got = {}
        for form in (0, 1, 2):                    # shipped, plain serial, shipped with strided emission reads
            psi = torch.full((U * N, K), 7.0, dtype=torch.float64, device="cuda")
            new = torch.full((U * N, K, T, 2), 7.0, dtype=torch.float64, device="cuda")
            L.check(lib.astk_debug_ctc_prefix(C.byref(s.bd), C.byref(s.bs), C.byref(s.bc), _vp(cand_dev), form, _vp(psi), _vp(new), _stream()))
            torch.cuda.synchronize()
            got[form] = (psi.cpu().numpy(), new.cpu().numpy())
    n_dead = 0
    for r, sl in enumerate(slots):
        u = r // N
        Tu = LENS[u]
        for k in range(K):
            if sl["status"] != 1:
                for form in (0, 1, 2):
                    assert got[form][0][r, k] == 7.0 and (got[form][1][r, k] == 7.0).all()          # not live: untouched
                continue
            c = int(cands[r, k])
            psi, st, _ = PM.extend(xs[u], sl["state"], sl["n"], sl["token"] if sl["n"] else -1, c)
            n_dead += psi == -np.inf
            for form in (0, 1, 2):
                _close(got[form][0][r, k], psi, (kind, "psi", form, r, k, c))
                if c != EOS:
                    _close(got[form][1][r, k, :Tu], st, (kind, "state", form, r, k, c))
                assert (got[form][1][r, k, Tu:] == 7.0).all()                                     # frames behind T''_u: never written
            _close(got[0][0][r, k], got[1][0][r, k], ("psi, wave against serial", r, k))
            assert got[0][0][r, k] == got[2][0][r, k]                      # the same arithmetic on the same values: the same bits
            if c != EOS:
                _close(got[0][1][r, k, :Tu], got[1][1][r, k, :Tu], ("state, wave against serial", r, k))
                assert np.array_equal(got[0][1][r, k, :Tu], got[2][1][r, k, :Tu])
    assert n_dead > 0


def test_c_abi_refuses_bad_joint_arguments():
    from ast_amd import _lib as L
    lib = L.load()
    lg = np.zeros((1, 4, 9), np.float32)
    s = _Search(L, [4], 2, 2, 9, lg)

    def init(**over):
        bc = L.BeamCtc.from_buffer_copy(s.bc)
        for k, v in over.items():
            setattr(bc, k, v)
        return lib.astk_beam_ctc_init(C.byref(s.bd), C.byref(s.bs), C.byref(bc), _stream())
    assert init(weight=0.0) != 0 and b"outside (0, 1]" in lib.astk_last_error()
    assert init(weight=1.5) != 0 and b"outside (0, 1]" in lib.astk_last_error()
    assert init(first_label=0) != 0 and b"first_label" in lib.astk_last_error()
    assert init(first_label=2) != 0 and b"eos" in lib.astk_last_error()
    assert init(ldv=8) != 0 and b"ldv" in lib.astk_last_error()
    assert init(ws_bytes=64) != 0 and b"workspace too small" in lib.astk_last_error()
    assert init(struct_size=8) != 0 and b"struct_size" in lib.astk_last_error()
    assert init() == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. one joint selection step
def test_joint_selection_and_gather_match_the_model():
    """astk_beam_select_ctc on supplied logits and states: live, finished and empty slots; the finished slot 1 of utterance 0 has the
    best score, moves to row 0 and keeps its own CTC state while its neighbours' expansions move around it; an eos expansion keeps
    its parent's state."""
    from ast_amd import _lib as L
    lib = L.load()
    rng = np.random.default_rng(5)
    N, K, V, w, lens = 3, 3, 9, 0.4, [7, 4]
    U, T, R = 2, 7, 6
    ctc_logits = (rng.standard_normal((U, T, V)) * 2).astype(np.float32)
    ctc_logits[1, 0, 7] += 6.0                                   # utterance 1 says "7" and nothing else: eos behind [7] ranks first
    ctc_logits[1, 1:, 0] += 6.0
    xs = [PM.log_softmax64(ctc_logits[u, :lens[u]]) for u in range(U)]
    s = _Search(L, lens, N, K, V, ctc_logits, w=w, nl=2, H=16, A=8)

    def slot(u, labs, status, att):
        toks = [t for t in labs if t >= 3]
        psi, st = PM.prefix_state(xs[u], toks)
        tok = labs[-1] if labs else GO
        if status == 2:
            psi = PM.extend(xs[u], st, len(toks), toks[-1], EOS)[0]
            tok = EOS
        return dict(status=status, token=tok, score=PM.joint_score(w, att, psi), att=att, psi=psi, n=len(toks), state=st)
    empty = dict(status=0, token=0, score=0.0, att=0.0, psi=0.0, n=0, state=None)
    slots = [slot(0, [5], 1, -1.2), slot(0, [4, 6], 2, -0.1), slot(0, [5, 6], 1, -2.0), slot(1, [7], 1, -0.3), slot(1, [8, 3], 1, -0.2), dict(empty)]
    slots[1]["score"] = -0.5                                    # (the carried slot wins whatever its terms say)
    s.set_slots(slots)
    logits = (rng.standard_normal((R, V)) * 2).astype(np.float32)
    logits[3, EOS] = logits[3].max() + 1.0                      # row 3 proposes eos first
    logits[2, 6] = logits[2].max() + 0.5                        # row 2 proposes a repeat of its last label
    want = PM.np_select_ctc(logits, [xs[r // N] for r in range(R)], slots, N, K, w)
    # the candidates' scores are at least 1e-6 apart: the ranking cannot depend on the bound
    every = PM.np_select_ctc(logits, [xs[r // N] for r in range(R)], slots, N, K, w, keep=N * K)
    for u in range(U):
        sc = sorted(c["score"] for c in every[u * N * K:(u + 1) * N * K] if c["status"] != 0)
        fin = [v for v in sc if np.isfinite(v)]
        assert all(b - a >= 1e-6 for a, b in zip(fin[:-1], fin[1:]))
    assert (want[0]["carried"], want[0]["parent"]) == (1, 1) and (want[3]["token"], want[3]["carried"], want[3]["parent"]) == (EOS, 0, 0)
    assert any(not c["carried"] and c["token"] != EOS and c["status"] for c in want)
    old = {k: s.st[k].clone() for k in ("c", "h", "ht")}
    new = dict(c=torch.randn(2, R, 16, device="cuda"), h=torch.randn(2, R, 16, device="cuda"), ht=torch.randn(R, 8, device="cuda"))
    alpha = torch.randn(R, T, device="cuda")
    lg = torch.from_numpy(logits).cuda()
    L.check(lib.astk_beam_select_ctc(C.byref(s.bd), 2, 16, 8, _vp(lg), _vp(alpha), T, _vp(new["c"]), _vp(new["h"]), _vp(new["ht"]),
                                     C.byref(s.bs), C.byref(s.bc), 1, _stream()))
    torch.cuda.synchronize()
    hist, tok, stt = s.st["hist"][1].cpu().numpy(), s.st["tokens"].cpu().numpy(), s.st["status"].cpu().numpy()
    sc, att, psi, nlab, state = (t.cpu().numpy() for t in (s.st["score"], s.att, s.psi, s.nlab, s.state))
    for r, c in enumerate(want):
        u = r // N
        assert stt[r] == c["status"], (r, stt[r], c)
        if c["status"] == 0:
            assert hist[r, 0] == -1 and (sc[r], att[r], psi[r], nlab[r]) == (0.0, 0.0, 0.0, 0)
            continue
        assert (hist[r, 0], hist[r, 1], hist[r, 2], tok[r], nlab[r]) == (c["parent"], c["token"], c["carried"], c["token"], c["n"]), (r, hist[r], c)
        _close(sc[r], c["score"], ("score", r))
        _close(att[r], c["att"], ("att", r))
        _close(psi[r], c["psi"], ("psi", r))
        _close(state[r, :lens[u]], c["state"], ("state", r))
        for k in ("c", "h", "ht"):
            ref = (old if c["carried"] else new)[k][..., u * N + c["parent"], :]
            assert torch.equal(s.st[k][..., r, :], ref), (k, r)
    fro = [all(c["status"] != 1 for c in want[u * N:(u + 1) * N]) for u in range(U)]
    assert s.st["frozen"].cpu().tolist() == [int(f) for f in fro] and int(s.st["n_frozen"][0]) == sum(fro)


# ---------------------------------------------------------------- 3. whole searches
CONFIGS = {
    "tiny-3x3": lambda: tiny_cfg(enc_layers=3, dec_layers=3, H=64, E=16, A=64, c0=8, c1=16, V=57),
    "dec-1-layer": lambda: tiny_cfg(enc_layers=2, dec_layers=1, H=64, E=16, A=32, c0=8, c1=16, V=45),
}
FRAMES = (90, 71, 12)                    # the last has T'' = 3 < stop_limit: its long prefixes die
# Parameter seeds for which the host joint search alone, run on the CPU with the float64 oracle (oracle/ast_ref.py) and the NumPy
# scorer, keeps every pair of kept scores at least 1.1e-3 apart in all twelve (w, N, K) cases: the 1e-5 exemption below stays unused.
SEED = {"tiny-3x3": 21, "dec-1-layer": 21}
_cache = {}


def _setup(name):
    """(cfg, P with the head, D, V, Xs, the GPU model), built once per config."""
    if name not in _cache:
        from oracle import ast_ref as R
        from ast_amd.seq2seq import SpeechEncoderDecoder
        cfg = CONFIGS[name]()
        cfg["rnn_config"]["ctc"] = True
        V, D = cfg["rnn_config"]["dec_vocab_size"], 80
        P = dict(R.init_params(cfg, D, V, seed=SEED[name], dtype=np.float32))
        P["out/b"] = P["out/b"].copy()
        P["out/b"][EOS] += 2.0                      # some hypotheses finish before stop_limit: the carry path runs
        P.update(CM.head_params(cfg["rnn_config"]["hidden_units"], V))
        Xs = [R.synth_batch(1, T, D, 4, V, seed=30 + i, dtype=np.float32)[0] for i, T in enumerate(FRAMES)]
        g = SpeechEncoderDecoder(0, copy.deepcopy(cfg)).materialize(D, values=P)
        _cache[name] = (cfg, P, D, V, Xs, g)
    return _cache[name]


def _host_search(g, X, x, stop, N, K, w):
    """The host joint search of one utterance on the GPU model's own per-hypothesis steps (ast_amd.nn.decode_beam_step)."""
    from ast_amd import nn as gnn
    from ast_amd.seq2seq import using_config

    def propose(entry):
        return [(e["hyp"][-1], e["score"], e) for e in gnn.decode_beam_step(g, dict(entry, score=0.0), K)]
    with using_config("train", False):
        g.encode(torch.from_numpy(X) if isinstance(X, np.ndarray) else X)
        return PM.joint_beam_search(x, propose, gnn.init_hyp(g), stop, N, w)


def _cross_check(g, X, x_logits, lst, w):
    """score = (1 - w) A + w C on every finished hypothesis: A the forced-decoding score of its tokens, C = -nll of the CTC loss model."""
    from ast_amd import nn as gnn
    fin = [e for e in lst if e["hyp"][-1] == EOS and np.isfinite(e["score"])]
    if not fin:
        return 0
    A, _ = gnn.score_hypotheses(g, X, [e["hyp"] for e in fin])
    for e, a in zip(fin, A):
        labels = [t for t in e["hyp"] if t >= 3]
        c = -float(CM.ctc_row(x_logits, labels, 0)[0])
        ta, tc = float(DH.tol(a)), 1e-10 * max(1.0, abs(c))
        assert abs(e["att_score"] - a) <= ta, (e["hyp"], e["att_score"], a)
        assert abs(e["ctc_score"] - c) <= tc, (e["hyp"], e["ctc_score"], c)
        assert abs(e["score"] - ((1 - w) * a + w * c)) <= (1 - w) * ta + w * tc + 1e-12 * abs(e["score"]), (e["hyp"], e["score"], a, c)
    return len(fin)


@pytest.mark.parametrize("N,K", [(3, 4), (4, 2), (1, 3)])
@pytest.mark.parametrize("w", [0.3, 1.0])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_joint_search_matches_the_host_joint_search(name, w, N, K):
    from ast_amd import nn as gnn
    cfg, P, D, V, Xs, g = _setup(name)
    stop = 7
    got = gnn.decode_beam_batch(g, [torch.from_numpy(X) for X in Xs], stop, N, K, ctc_weight=w)
    logits, lens = g.last_beam_ctc
    logits = logits.cpu().numpy()
    assert lens[2] == 3
    exempt, early, checked = 0, False, 0
    for u, (X, lst) in enumerate(zip(Xs, got)):
        xl = logits[u, :lens[u]]
        want = _host_search(g, X, PM.log_softmax64(xl), stop, N, K, w)
        assert list(lst[0])[:2] == ["hyp", "score"] and set(lst[0]) == {"hyp", "score", "dec_state", "attn_v", "attn_history", "att_score", "ctc_score"}
        if PM.tight([e["score"] for e in want]):
            exempt += 1
        else:
            assert [e["hyp"] for e in lst] == [e["hyp"] for e in want], (name, u, [e["hyp"] for e in lst], [e["hyp"] for e in want])
            for a, b in zip(lst, want):
                assert isinstance(a["score"], float) and isinstance(a["att_score"], float) and isinstance(a["ctc_score"], float)
                if b["score"] == -np.inf:
                    assert a["score"] == -np.inf
                else:
                    assert abs(a["score"] - b["score"]) <= 1e-5 * max(1.0, abs(b["score"])), (a["score"], b["score"])
                    assert abs(a["att_score"] - b["att"]) <= 1e-5 * max(1.0, abs(b["att"]))
                    _close(a["ctc_score"], b["psi"], ("ctc_score", name, u))
                assert len(a["attn_history"]) == len(a["hyp"]) - 1
        checked += _cross_check(g, X, xl, lst, w)
        early |= any(e["hyp"][-1] == EOS and len(e["hyp"]) <= stop for e in lst)
    assert exempt * 4 <= len(Xs), "the near-tie exemption was used by more than 1 utterance in 4"
    assert early, "no hypothesis finished before stop_limit: the carry path was not exercised"
    assert checked > 0


def test_weight_zero_is_the_plain_search():
    from ast_amd import nn as gnn
    cfg, P, D, V, Xs, g = _setup("dec-1-layer")
    Xt = [torch.from_numpy(X) for X in Xs]
    a = gnn.decode_beam_batch(g, Xt, 7, 3, 4)
    g.last_beam_ctc = None
    b = gnn.decode_beam_batch(g, Xt, 7, 3, 4, ctc_weight=0.0)
    assert g.last_beam_ctc is None
    for la, lb in zip(a, b):
        assert [e["hyp"] for e in la] == [e["hyp"] for e in lb] and [e["score"] for e in la] == [e["score"] for e in lb]
        assert all(list(e) == ["hyp", "score", "dec_state", "attn_v", "attn_history"] for e in lb)


def test_joint_search_does_not_depend_on_the_batch():
    from ast_amd import nn as gnn
    cfg, P, D, V, Xs, g = _setup("tiny-3x3")
    Xt = [torch.from_numpy(X) for X in Xs]
    alone = gnn.decode_beam_batch(g, [Xt[1]], 7, 3, 4, ctc_weight=0.3)[0]
    inside = gnn.decode_beam_batch(g, Xt, 7, 3, 4, ctc_weight=0.3)[1]
    assert [e["hyp"] for e in alone] == [e["hyp"] for e in inside]
    for a, b in zip(alone, inside):
        for k in ("score", "att_score", "ctc_score"):
            assert a[k] == b[k] or abs(a[k] - b[k]) <= 1e-6 * max(1.0, abs(b[k])), (k, a[k], b[k])


def test_joint_search_at_the_shipped_width_passes_the_cross_check():
    from oracle import ast_ref as R
    from ast_amd import nn as gnn
    from ast_amd.seq2seq import SpeechEncoderDecoder
    cfg = tiny_cfg(**DH.CFG1)
    cfg["rnn_config"]["ctc"] = True
    V, D, w = DH.CFG1["V"], 80, 0.3
    P = dict(R.init_params(cfg, D, V, seed=3, dtype=np.float32))
    P["out/W"] = (P["out/W"] * 3).astype(np.float32)
    P.update(CM.head_params(cfg["rnn_config"]["hidden_units"], V))
    cfg["rnn_config"]["dec_vocab_size"] = V
    g = SpeechEncoderDecoder(0, cfg).materialize(D, values=P)
    Xs = [torch.from_numpy(R.synth_batch(1, 240, D, 4, V, seed=60 + i, dtype=np.float32)[0]) for i in range(2)]
    got = gnn.decode_beam_batch(g, Xs, 12, 5, 5, ctc_weight=w)
    logits, lens = g.last_beam_ctc
    logits = logits.cpu().numpy()
    for u, (X, lst) in enumerate(zip(Xs, got)):
        assert 1 <= len(lst) <= 5 and not any(np.isnan(e["score"]) for e in lst)
        _cross_check(g, X, logits[u, :lens[u]], lst, w)
        for e in lst:                    # an unfinished hypothesis: ctc_score is its prefix score
            if e["hyp"][-1] != EOS and np.isfinite(e["score"]):
                psi, _ = PM.prefix_state(PM.log_softmax64(logits[u, :lens[u]]), e["hyp"][1:])
                _close(e["ctc_score"], psi, ("prefix score", u))
                assert abs(e["score"] - ((1 - w) * e["att_score"] + w * e["ctc_score"])) <= 1e-12 * abs(e["score"])


# ---------------------------------------------------------------- 4. beam.py --ctc-weight
def test_beam_py_ctc_weight_writes_the_library_calls_hypotheses(tmp_path):
    mcfg = tiny_cfg(enc_layers=2, dec_layers=1, H=32, E=16, A=32, c0=8, c1=16, V=31, drop=0.0)
    del mcfg["rnn_config"]["dec_vocab_size"]
    mcfg["rnn_config"]["ctc"] = True
    tcfg = {"seed": "seed-ast-20h", "gpuid": 0, "batch_size": 8, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 1,
            "optimizer": {"type": 0, "lr": 2e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0, "ctc_weight": 0.3},
            "data": {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 16, "syn_dev": 5},
                     "frames": [60, 300], "targets": [2, 9], "buckets_num": 4, "buckets_width": 80, "max_pred": 8,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w"}}
    json.dump(mcfg, open(tmp_path / "model_cfg.json", "w"))
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "-m", str(tmp_path), "-e", "1"], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    from ast_amd.nn import NN
    nn = NN(str(tmp_path))
    refs = tmp_path / "refs" / "syn_dev"
    os.makedirs(refs)
    utts = sorted(nn.data_loader.info["syn_dev"])
    truth = nn.data_loader.get_hyps([(u, list(nn.data_loader.ids["syn_dev"][u])) for u in utts])
    (refs / "eval.ids").write_text("".join(u + "\n" for u in utts))
    (refs / "ref.en0").write_text("".join(" ".join(truth[u]) + "\n" for u in utts))
    tcfg["data"].update(refs_path=str(tmp_path / "refs"), n_evals=1)
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))
    want = {}
    for utt in nn.data_loader.get_batch(1, "syn_dev", train=False, labels=False):
        want[utt["utts"][0]] = nn.decode_beam_batch([utt["X"]], 8, 3, 4, ctc_weight=0.3)[0]
    del nn
    torch.cuda.empty_cache()
    base = [sys.executable, os.path.join(ROOT, "beam.py"), "-m", str(tmp_path), "-n", "3", "-k", "4", "-s", "syn_dev", "-w", "0.6"]
    r = subprocess.run(base + ["-b", "2", "--ctc-weight", "0.3"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BLEU = " in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    with open(tmp_path / "syn_dev_beam_N-3_K-4.p", "rb") as f:
        beam = pickle.load(f)
    assert sorted(beam) == sorted(want) and len(beam) == 5
    for u, lst in beam.items():
        assert [e[0] for e in lst] == [e["hyp"] for e in want[u]]
        for e, ref in zip(lst, want[u]):
            assert len(e) == 5
            np.testing.assert_allclose([e[1], e[3], e[4]], [ref["score"], ref["att_score"], ref["ctc_score"]], rtol=1e-5)
    # without -b, or with --device, the flag is refused with a message that names the batched search
    for extra in (["--ctc-weight", "0.3"], ["--device", "--ctc-weight", "0.3"]):
        r = subprocess.run(base + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "decode_beam_batch" in r.stderr, r.stdout[-1000:] + r.stderr[-1000:]
