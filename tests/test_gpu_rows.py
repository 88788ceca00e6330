"""Per-row source lengths in the four on-device decode modes (include/astk.h astk_*_rows; SpeechEncoderDecoder.encode_rows and rows=;
ast_amd.nn score_hypotheses_packed / sample_hypotheses_packed; score.py / sample.py -b U).

The reference of every masked call is the same row run ALONE, unmasked, at B = 1 and T = its length, on paths the project already
tests: the per-step loop (astk_decoder_step_infer, float32 logits, the rest in float64 on the host) for the kernel-level cases, the
float64 oracle for the model-level one, beam search's own scores and the unpacked helpers for the rest.  Lengths are chosen against
the chunk plan nsplit = min(64, 256 // B, T''), chunk = ceil(T'' / nsplit).  Bounds: tokens equal at the positions guarded at a top-2
gap of 1e-4 (at least 0.95 of all positions), log-probabilities under tol(), attention rows within 1e-5 and exactly 0 beyond a row's
length.  Every test prints its figures before it asserts."""
import copy
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from conftest import tiny_cfg
from decode_helpers import CFG1, EOS, ES_EN, GO, MID, OUT_SCALE, guard, lse64, setup, targets, tol

pytestmark = pytest.mark.gpu

SEED = 2024
GAP = 1e-4
SHARE = 0.95


def _status_is_clear():
    from ast_amd import _lib
    mask = C.c_uint(7)
    return _lib.load().astk_persist_status(C.byref(mask), 0) == 0 and mask.value == 0


@pytest.fixture(autouse=True)
def _status_word_stays_clear():
    yield
    torch.cuda.synchronize()
    assert _status_is_clear()


def _plan(B, T):
    nsplit = min(64, 256 // B, T)
    return nsplit, -(-T // nsplit)


def _synthetic(shape, lens, T, seed, pad=0.0, **over):
    """A model of `shape` and a RowBatch of seeded random memories: any length is reachable.  What lies beyond a row's length is `pad`
    (0, or seeded values of that magnitude)."""
    from ast_amd.seq2seq import RowBatch
    _, _, _, m = setup(shape, 1, 64, seed=seed, eos_bias=-1e4, **over)      # (no EOS ever: every free-running decode runs stop_limit steps)
    rng = np.random.default_rng(seed + 100)
    B, H, nl = len(lens), shape["H"], shape["dec_layers"]
    enc = rng.uniform(-0.5, 0.5, size=(B, T, H)).astype(np.float32)
    junk = (rng.uniform(0.5, 1.0, size=(B, T, H)) * rng.choice([-1.0, 1.0], size=(B, T, H)) * pad).astype(np.float32)
    for b, n in enumerate(lens):
        enc[b, n:] = junk[b, n:]
    c0 = (rng.standard_normal((nl, B, H)) * 0.3).astype(np.float32)
    h0 = np.tanh(rng.standard_normal((nl, B, H)) * 0.3).astype(np.float32)
    return m, RowBatch(torch.from_numpy(enc), lens, torch.from_numpy(c0), torch.from_numpy(h0))


def _keys(streams):
    from ast_amd.seq2seq import sample_row_key
    return [sample_row_key(SEED, int(s)) for s in streams]


def _alone(m, rb, S, y, modes):
    """Every row of rb ALONE on the per-step loop, B = 1 and T = its length, once per mode: a namespace per mode of (B, S) arrays --
    tokens / pred, logp (float64), the top-2 gaps (S, B) -- and, forced, alpha (B, S, T''max) with zeros beyond the length."""
    from ast_amd.seq2seq import gumbel_noise, using_config
    V = m.V
    out = {k: types.SimpleNamespace(tokens=np.zeros((rb.B, S), np.int32), logp=np.zeros((rb.B, S)), gaps=np.zeros((S, rb.B)),
                                    logp_max=np.zeros((rb.B, S)), alpha=np.zeros((rb.B, S, rb.T))) for k in modes}
    keys = _keys(range(rb.B))
    with using_config("train", False):
        for b in range(rb.B):
            for mode in modes:
                m._adopt_rows(rb.row(b))
                ht = torch.zeros(1, m.A, dtype=torch.float32, device=m.device)
                word = GO
                r = out[mode]
                for s in range(S):
                    feed = int(y[b, s]) if mode == "forced" else word
                    logits, ht, al = m.decode_step(torch.tensor([feed], dtype=torch.int32), ht)
                    lg = logits.double().cpu().numpy()
                    z = lg[0] + (gumbel_noise(keys[b], s, V)[1] if mode == "sampled" else 0.0)
                    srt = np.sort(z)
                    word = int(z.argmax())
                    r.tokens[b, s], r.gaps[s, b] = word, srt[-1] - srt[-2]
                    lse = lse64(lg)[0]
                    r.logp_max[b, s] = lg[0].max() - lse
                    r.logp[b, s] = lg[0, int(y[b, s + 1]) if mode == "forced" else word] - lse
                    if mode == "forced":
                        r.alpha[b, s, :int(rb.lens[b])] = al[0, :, 0].double().cpu().numpy()
    return out


def _check_free(tag, got_tokens, got_logp, ref):
    """A free-running decode against the rows alone: tokens equal and logp under tol() at the guarded positions."""
    ok = guard(ref.tokens, ref.gaps, GAP)
    share = ok.sum() / ok.size
    err = np.abs(got_logp.astype(np.float64) - ref.logp)[ok]
    rel = float((err / tol(ref.logp[ok])).max())
    wrong = int((got_tokens[ok] != ref.tokens[ok]).sum())
    print(f"  {tag}: guarded {share:.4f} (smallest gap {ref.gaps.min():.2e}), {wrong} tokens differ, logp max abs err {err.max():.3e}, "
          f"max err / tol {rel:.3f}")
    assert got_tokens.shape == ref.tokens.shape, (got_tokens.shape, ref.tokens.shape)
    assert share >= SHARE and wrong == 0 and rel <= 1.0, (tag, share, wrong, rel)


def _check_forced(tag, got, ref, lens):
    ok = ref.gaps.T >= GAP
    share = ok.sum() / ok.size
    r1 = float((np.abs(got.logp.astype(np.float64) - ref.logp) / tol(ref.logp)).max())
    r2 = float((np.abs(got.logp_max.astype(np.float64) - ref.logp_max) / tol(ref.logp_max)).max())
    wrong = int((got.pred[ok] != ref.tokens[ok]).sum())
    ea = float(np.abs(got.alpha.astype(np.float64) - ref.alpha).max())
    beyond = max(float(np.abs(got.alpha[b, :, n:]).max()) if n < got.alpha.shape[2] else 0.0 for b, n in enumerate(lens))
    rs = float(np.abs(got.alpha.astype(np.float64).sum(axis=2) - 1).max())
    print(f"  {tag}: logp max err / tol {r1:.3f}, logp_max {r2:.3f}, argmax compared {share:.4f} ({wrong} differ), alpha max abs err {ea:.3e}, "
          f"largest |alpha| beyond a length {beyond!r}, max |row sum - 1| {rs:.3e}")
    assert got.alpha.shape == ref.alpha.shape
    assert r1 <= 1.0 and r2 <= 1.0 and share >= SHARE and wrong == 0 and ea <= 1e-5 and beyond == 0.0 and rs <= 1e-5, tag


def _run(m, rb, mode, S, y):
    if mode == "greedy":
        r = m.predict(None, GO, EOS, S, rows=rb)
        path = m.last_predict_path
    elif mode == "scored":
        r = m.predict_scored(None, GO, EOS, S, rows=rb)
        path = m.last_predict_path
    elif mode == "sampled":
        r = m.sample(None, GO, EOS, S, SEED, rows=rb)
        path = m.last_predict_path
    else:
        r = m.score(None, y, return_alpha=True, rows=rb)
        path = m.last_score_path
    return r, path


def _check_mode(tag, m, rb, mode, S, y, ref, path="device"):
    got, took = _run(m, rb, mode, S, y)
    assert took == path, (mode, took)
    if mode == "greedy":
        ok = guard(ref["greedy"].tokens, ref["greedy"].gaps, GAP)
        print(f"  {tag} greedy: guarded {ok.sum() / ok.size:.4f}, {int((got[ok] != ref['greedy'].tokens[ok]).sum())} tokens differ")
        assert got.shape == ok.shape and ok.sum() >= SHARE * ok.size and (got[ok] == ref["greedy"].tokens[ok]).all()
    elif mode == "scored":
        _check_free(f"{tag} scored", got.tokens, got.logp, ref["greedy"])
    elif mode == "sampled":
        _check_free(f"{tag} sampled", got.tokens, got.logp, ref["sampled"])
    else:
        _check_forced(f"{tag} forced", got, ref["forced"], rb.lens)
    return got


# ---------------------------------------------------------------- 1-3. the three attention code paths, synthetic memory
def _lens_generic():
    return [40, 39, 38, 37, 36, 3, 2, 1, 40, 35, 20, 19, 18, 4, 6, 33, 1]


def _lens_resident():
    return [200, 199, 176, 175, 100, 26, 25, 1] * 4


def _lens_streamed():
    # chunk 53 > 28 resident rows: ends in a streamed tail (53k + 40), in the resident part (53k + 10: the tail is empty), exactly on
    # the resident rows (53k + 28), on a chunk boundary, the full row and 1
    return [420, 1, 53 * 3 + 40, 53 * 2 + 10, 53 * 4 + 28, 53 * 5, 53 * 7 + 1, 40, 10, 28, 29, 53, 54, 419, 53 * 6 + 29, 300] * 2


CASES = {"generic": (MID, _lens_generic, 40, 12, 3, ("greedy", "sampled", "forced"), (15, 3)),
         "resident": (CFG1, _lens_resident, 200, 10, 5, ("greedy", "forced"), (8, 25)),
         "streamed": (ES_EN, _lens_streamed, 420, 10, 7, ("sampled", "forced"), (8, 53))}


@functools.lru_cache(maxsize=None)
def _case(name):
    shape, lens, T, S, seed, modes, plan = CASES[name]
    lens = lens()
    assert _plan(len(lens), T) == plan
    m, rb = _synthetic(shape, lens, T, seed)
    y = targets(len(lens), S + 1, shape["V"], seed=seed + 1, go_first=True)
    return m, rb, y, S, _alone(m, rb, S, y, modes)


@pytest.mark.parametrize("mode", ["greedy", "scored", "sampled", "forced"])
def test_generic_scan_rows_decode_as_alone(mode):
    """MID (H = 64: the generic scan), B = 17 (two batch tiles, the second with one row), T''max = 40: nsplit 15, chunk 3 -- a full row,
    ends inside the last chunk, on a chunk boundary, whole chunks empty, length 1."""
    m, rb, y, S, ref = _case("generic")
    print()
    _check_mode("generic", m, rb, mode, S, y, ref)


@pytest.mark.parametrize("mode", ["greedy", "forced"])
def test_resident_scan_rows_decode_as_alone(mode):
    """configs[1] (NC = 8, every slice row resident), B = 32, T''max = 200: chunk 25."""
    m, rb, y, S, ref = _case("resident")
    print()
    _check_mode("resident", m, rb, mode, S, y, ref)


@pytest.mark.parametrize("mode", ["sampled", "forced"])
def test_streamed_scan_rows_decode_as_alone(mode):
    """es_en_20h (NC = 8, three layers), B = 32, T''max = 420: chunk 53, of which 28 rows are resident and the rest streamed."""
    m, rb, y, S, ref = _case("streamed")
    print()
    _check_mode("streamed", m, rb, mode, S, y, ref)


# ---------------------------------------------------------------- 4. padding is never read into a result
def test_padding_is_never_read_into_a_result():
    """Two calls whose memories differ only beyond the lengths (zeros against seeded values of magnitude 1e3): every output word is
    the same to the bit, alpha included."""
    shape, lens, T, S, seed, _, _ = CASES["resident"]
    y = targets(32, S + 1, shape["V"], seed=seed + 1, go_first=True)
    outs = []
    for pad in (0.0, 1e3):
        m, rb = _synthetic(shape, lens(), T, seed, pad=pad)
        beyond = float(max(rb.enc[b, n:].abs().max() if n < T else 0.0 for b, n in enumerate(rb.lens)))
        f, path = _run(m, rb, "forced", S, y)
        g, path2 = _run(m, rb, "scored", S, y)
        assert path == path2 == "device"
        outs.append((f, g))
        print(f"\npad {pad:g}: largest |enc| beyond a length {beyond:.1f}, forced loss {f.loss!r}, greedy score[0] {g.score[0]!r}")
    (f0, g0), (f1, g1) = outs
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for k in ("logp", "logp_max", "alpha"):
        assert (bits(getattr(f0, k)) == bits(getattr(f1, k))).all(), k
    assert (f0.pred == f1.pred).all() and (g0.tokens == g1.tokens).all() and (bits(g0.logp) == bits(g1.logp)).all()
    assert np.isfinite(f1.alpha).all() and np.isfinite(f1.logp).all()


# ---------------------------------------------------------------- 5. all-full lengths are the old path
@pytest.mark.parametrize("B", [5, 32])
def test_full_lengths_are_the_existing_entry_points_to_the_bit(B):
    from ast_amd.seq2seq import RowBatch
    _, _, X, m = setup(MID, B, 120, seed=9, eos_bias=-1e4)
    y = targets(B, 13, MID["V"], seed=3, go_first=True)
    Xt = torch.from_numpy(X)
    f0 = m.score(Xt, y, return_alpha=True)
    st = m._cur
    rb = RowBatch(st["enc_states"].clone(), [st["T2"]] * B, st["c0"].clone(), st["h0"].clone())
    g0 = m.predict_scored(Xt, GO, EOS, 12)
    p0 = m.predict(Xt, GO, EOS, 12)
    assert m.last_score_path == "device" and m.last_predict_path == "device"
    f1, g1, p1 = m.score(None, y, return_alpha=True, rows=rb), m.predict_scored(None, GO, EOS, 12, rows=rb), m.predict(None, GO, EOS, 12, rows=rb)
    assert m.last_score_path == "device" and m.last_predict_path == "device" and m._cur["row_len"].tolist() == [st["T2"]] * B
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    print(f"\nB {B}: T'' {st['T2']}, forced loss {f0.loss!r} / {f1.loss!r}, greedy n_steps {g0.n_steps} / {g1.n_steps}")
    for k in ("logp", "logp_max", "alpha"):
        assert (bits(getattr(f0, k)) == bits(getattr(f1, k))).all(), k
    assert (f0.pred == f1.pred).all() and f0.loss == f1.loss
    assert (g0.tokens == g1.tokens).all() and (bits(g0.logp) == bits(g1.logp)).all() and (p0 == p1).all()


# ---------------------------------------------------------------- 6. model-level against the float64 oracle
FRAMES = (316, 400, 404, 796, 800, 1680)


@functools.lru_cache(maxsize=None)
def _oracle_case():
    from oracle import ast_ref as R
    cfg, P, _, m = setup(ES_EN, 1, 64, seed=0)
    V, D, n, L = ES_EN["V"], 80, 5, 12
    Xs = [R.synth_batch(1, T, D, 3, V, seed=40 + i, dtype=np.float32)[0] for i, T in enumerate(FRAMES)]
    y = targets(n * len(Xs), L, V, seed=2, go_first=True)
    ref = types.SimpleNamespace(logp=np.zeros((len(y), L - 1)), logp_max=np.zeros((len(y), L - 1)), pred=np.zeros((len(y), L - 1), np.int32),
                                gaps=np.zeros((len(y), L - 1)), alpha=[], lens=[])
    for u, X in enumerate(Xs):          # every utterance encoded alone (its 5 rows are 5 copies of it), decode_step along the targets
        o = R.RefModel(cfg, {k: v.astype(np.float64) for k, v in P.items()}, V)
        o.train = False
        o.encode(np.repeat(X, n, axis=0).astype(np.float64))
        o.init_decoder_state()
        ht = R.Variable(np.zeros((n, cfg["rnn_config"]["attn_units"])))
        yu = y[u * n:(u + 1) * n]
        al_u = []
        for s in range(L - 1):
            logits, ht, al = o.decode_step(yu[:, s].astype(np.int32), ht, step=s)
            lg = np.asarray(logits.data, dtype=np.float64)
            lse, srt = lse64(lg), np.sort(lg, axis=1)
            rows = slice(u * n, (u + 1) * n)
            ref.logp[rows, s], ref.logp_max[rows, s] = lg[np.arange(n), yu[:, s + 1]] - lse, srt[:, -1] - lse
            ref.pred[rows, s], ref.gaps[rows, s] = lg.argmax(axis=1), srt[:, -1] - srt[:, -2]
            al_u.append(np.asarray(al.data, dtype=np.float64).reshape(n, -1))
        ref.alpha.append(np.stack(al_u, 1))
        ref.lens.append(ref.alpha[-1].shape[2])
    return m, Xs, y, n, ref


def test_packed_utterances_match_the_float64_oracle():
    """es_en_20h, 6 utterances of 316 .. 1680 frames, 5 target rows each (30 rows, L = 12) in ONE call, against the oracle encoding
    every utterance alone: the bounds of tests/test_gpu_forced.py."""
    m, Xs, y, n, ref = _oracle_case()
    rows_of = [u for u in range(len(Xs)) for _ in range(n)]
    rb = m.encode_rows([torch.from_numpy(X) for X in Xs], rows_of)
    assert rb.B == 30 and rb.lens.tolist() == [ref.lens[u] for u in rows_of] and rb.T == max(ref.lens)
    got = m.score(None, y, return_alpha=True, rows=rb)
    assert m.last_score_path == "device" and got.alpha.shape == (30, 11, rb.T)
    ok = ref.gaps >= 1e-3
    share = ok.sum() / ok.size
    r1 = float((np.abs(got.logp.astype(np.float64) - ref.logp) / tol(ref.logp)).max())
    r2 = float((np.abs(got.logp_max.astype(np.float64) - ref.logp_max) / tol(ref.logp_max)).max())
    wrong = int((got.pred[ok] != ref.pred[ok]).sum())
    w = (y[:, 1:] != 0).astype(np.float64)
    loss = float((w * -ref.logp).sum() / len(y))
    rl = abs(got.loss - loss) / abs(loss)
    ea = beyond = 0.0
    for u in range(len(Xs)):
        a = got.alpha[u * n:(u + 1) * n]
        ea = max(ea, float(np.abs(a[:, :, :ref.lens[u]].astype(np.float64) - ref.alpha[u]).max()))
        beyond = max(beyond, float(np.abs(a[:, :, ref.lens[u]:]).max()) if ref.lens[u] < rb.T else 0.0)
    print(f"\nlengths {ref.lens}: logp max err / tol {r1:.3f}, logp_max {r2:.3f}, argmax compared {share:.4f} ({wrong} differ), loss {got.loss:.6f} "
          f"(oracle {loss:.6f}, rel {rl:.3e}), alpha max abs err {ea:.3e}, beyond the lengths {beyond!r}")
    assert share >= SHARE
    assert r1 <= 1.0 and r2 <= 1.0 and wrong == 0 and rl <= 1e-4 and ea <= 1e-5 and beyond == 0.0


# ---------------------------------------------------------------- 7. beam consistency across utterances, in one call
@functools.lru_cache(maxsize=None)
def _beam_case():
    from oracle import ast_ref as R
    from ast_amd import nn as gnn
    from ast_amd.seq2seq import SpeechEncoderDecoder
    cfg = tiny_cfg(**MID)
    V, D, N = MID["V"], 80, 5
    P = R.init_params(cfg, D, V, seed=21, dtype=np.float32)
    P["out/W"] = (P["out/W"] * OUT_SCALE).astype(np.float32)
    P["out/b"] = P["out/b"].copy()
    P["out/b"][EOS] += 2.0                      # some hypotheses finish early: lengths differ inside an n-best list
    m = SpeechEncoderDecoder(0, copy.deepcopy(cfg)).materialize(D, values=P)
    Xs = [torch.from_numpy(R.synth_batch(1, T, D, 4, V, seed=30 + i, dtype=np.float32)[0]) for i, T in enumerate((90, 71, 120, 150))]
    return m, Xs, gnn.decode_beam_batch(m, Xs, 12, N, N)


def test_beam_scores_are_forced_scores_in_one_call():
    from ast_amd import nn as gnn
    m, Xs, lists = _beam_case()
    calls = []
    score = m.score
    m.score = lambda *a, **k: (calls.append(1), score(*a, **k))[1]
    try:
        res = gnn.score_hypotheses_packed(m, Xs, [[e["hyp"] for e in lst] for lst in lists], return_alpha=True)
    finally:
        del m.score
    n_hyp = sum(len(lst) for lst in lists)
    assert len(calls) == 1 and m.last_score_path == "device" and n_hyp == 20 and len({int(r.alpha.shape[2]) for _, r in res}) > 1
    worst, worst_a, lens = 0.0, 0.0, set()
    print()
    for u, (lst, (scores, r)) in enumerate(zip(lists, res)):
        for k, (e, sc) in enumerate(zip(lst, scores)):
            n = len(e["hyp"]) - 1
            bound = float(tol(r.logp[k, :n].astype(np.float64)).sum())
            ah = np.stack(e["attn_history"], 0)
            assert ah.shape == (n, r.alpha.shape[2])
            err, ea = abs(sc - e["score"]), float(np.abs(r.alpha[k, :n] - ah).max())
            print(f"utt {u} hyp {k}: {n} steps, beam {e['score']:.6f}, forced {sc:.6f}, |diff| {err:.3e} (bound {bound:.3e}), alpha max err {ea:.3e}")
            worst, worst_a = max(worst, err / bound), max(worst_a, ea)
            lens.add(n)
    print(f"{n_hyp} hypotheses in one call, lengths {sorted(lens)}: largest |diff| / bound {worst:.3f}, largest alpha error {worst_a:.3e}")
    assert len(lens) > 1 and worst <= 1.0 and worst_a <= 1e-5


# ---------------------------------------------------------------- 8. packing does not change answers
def test_packing_does_not_change_scores_or_samples():
    from ast_amd import nn as gnn
    m, Xs, lists = _beam_case()
    Xs, lists = Xs[:3], lists[:3]
    hyps = [[e["hyp"] for e in lst] for lst in lists]
    packed = gnn.score_hypotheses_packed(m, Xs, hyps, return_alpha=True)
    print()
    for u, (X, (sc_p, r_p)) in enumerate(zip(Xs, packed)):
        sc_1, r_1 = gnn.score_hypotheses(m, X, hyps[u], return_alpha=True)
        assert r_p.logp.shape == r_1.logp.shape and r_p.alpha.shape == r_1.alpha.shape and (r_p.weight == r_1.weight).all()
        bound = (r_1.weight * tol(r_1.logp.astype(np.float64))).sum(axis=1)
        err = np.abs(np.array(sc_p) - np.array(sc_1))
        rel = float((np.abs(r_p.logp.astype(np.float64) - r_1.logp) / tol(r_1.logp.astype(np.float64))).max())
        ea = float(np.abs(r_p.alpha - r_1.alpha).max())
        print(f"utt {u}: scores max abs diff {err.max():.3e}, logp max diff / tol {rel:.3f}, alpha max abs diff {ea:.3e}")
        assert rel <= 1.0 and ea <= 1e-5 and (err <= np.maximum(bound, tol(np.array(sc_1)))).all()
    # samples: an utterance's streams give the same samples packed and alone, at the draws the per-step loop guards
    n, stop = 4, 12
    one = [gnn.sample_hypotheses(m, X, n, stop, SEED, first_stream=u * n) for u, X in enumerate(Xs)]
    pk = gnn.sample_hypotheses_packed(m, Xs, n, stop, SEED)
    assert m.last_predict_path == "device" and [len(l) for l in pk] == [n] * 3
    # more rows than a call holds: utterance 0 with 40 samples splits 32 + 8 and still draws its own streams
    big = gnn.sample_hypotheses_packed(m, Xs[:2], 40, stop, SEED, first_streams=[0, 1000])
    assert len(big[0]) == len(big[1]) == 40
    checks = [(u, u * n + i, (one[u][i], pk[u][i])) for u in range(3) for i in range(n)] + [(0, i, (big[0][i],)) for i in (0, 3, 31, 32, 39)]
    guarded = 0
    for u, stream, hyps_got in checks:
        hyp, lp, ok = _sample_alone(m, Xs[u], stream, stop)
        guarded += ok
        for h in hyps_got if ok else ():
            assert h["hyp"] == hyp, (u, stream)
            assert abs(h["score"] - lp.sum()) <= tol(lp).sum(), (u, stream)
    print(f"samples: {guarded} of {len(checks)} checked draws are guarded at a gap of {GAP:g}; packed and unpacked equal the per-step loop there")
    assert guarded >= 0.9 * len(checks)        # (the reference decides the share: the seed is chosen so that the test is not empty)


def _sample_alone(m, X, stream, stop):
    """One utterance alone on the per-step loop, drawing from `stream`: the hypothesis cut behind its first EOS, the float64
    log-probabilities of its tokens, and whether every draw up to there has a top-2 gap of at least GAP."""
    from ast_amd.seq2seq import gumbel_noise, sample_row_key, using_config
    key = sample_row_key(SEED, stream)
    with using_config("train", False):
        m._adopt_rows(m.encode_rows([X]))
        ht = torch.zeros(1, m.A, dtype=torch.float32, device=m.device)
        word, hyp, lps, ok = GO, [GO], [], True
        for s in range(stop):
            logits, ht, _ = m.decode_step(torch.tensor([word], dtype=torch.int32), ht)
            lg = logits.double().cpu().numpy()
            z = lg[0] + gumbel_noise(key, s, m.V)[1]
            srt = np.sort(z)
            word = int(z.argmax())
            ok = ok and srt[-1] - srt[-2] >= GAP
            hyp.append(word)
            lps.append(lg[0, word] - lse64(lg)[0])
            if word == EOS:
                break
    return hyp, np.array(lps), bool(ok)


def test_sample_py_and_score_py_round_trip_packed(tmp_path):
    """sample.py -b 4 then score.py --nbest -b 4 on a tiny synthetic experiment, as child processes: the pickle has the format and
    the utterances of -b 1, and the model scores agree with the sampled ones, as in the round trip of tests/test_gpu_sample.py."""
    import json, os, pickle, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mcfg = tiny_cfg(enc_layers=2, dec_layers=1, H=64, E=16, A=64, c0=8, c1=16, V=31, drop=0.0)       # (H = 64: runs on the device loop)
    del mcfg["rnn_config"]["dec_vocab_size"]
    tcfg = {"seed": "seed-ast-20h", "gpuid": 0, "batch_size": 8, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 1,
            "optimizer": {"type": 0, "lr": 2e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0},
            "data": {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 16, "syn_dev": 7},
                     "frames": [60, 300], "targets": [2, 9], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w", "refs_path": str(tmp_path / "refs"), "n_evals": 1}}
    json.dump(mcfg, open(tmp_path / "model_cfg.json", "w"))
    json.dump(tcfg, open(tmp_path / "train_cfg.json", "w"))

    def run(script, *extra):
        r = subprocess.run([sys.executable, os.path.join(root, script), "-m", str(tmp_path)] + list(extra), cwd=root, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r.stdout
    run("train.py", "-e", "1")
    pk1, pk4 = str(tmp_path / "s1.p"), str(tmp_path / "s4.p")
    run("sample.py", "-s", "syn_dev", "-n", "6", "--seed", "11", "-w", pk1)
    out = run("sample.py", "-s", "syn_dev", "-n", "6", "--seed", "11", "-w", pk4, "-b", "4")
    s1, s4 = pickle.load(open(pk1, "rb")), pickle.load(open(pk4, "rb"))
    assert sorted(s1) == sorted(s4) and len(s4) == 7 and all(len(v) == 6 for v in s4.values()) and "path: device" in out
    same = sum(a[0] == b[0] for u in s1 for a, b in zip(s1[u], s4[u]))
    print(f"\n-b 4 against -b 1: {same} of 42 samples equal (a figure: draws at a tiny gap may differ)")
    out3 = run("score.py", "-s", "syn_dev", "--nbest", pk4, "-b", "4")
    rows = [l.split() for l in open(pk4 + ".scores.txt").read().splitlines()]
    assert len(rows) == 42 and "path: device" in out3
    worst = max(abs(float(r[2]) - float(r[3])) / (int(r[4]) * float(tol(float(r[2]))) + 1e-6) for r in rows)
    print(out3.strip().splitlines()[-2], f"(worst ratio {worst:.3f})")
    assert "largest |beam score - model score|" in out3 and worst <= 1.0
    run("score.py", "-s", "syn_dev", "--nbest", pk4)
    rows1 = [l.split() for l in open(pk4 + ".scores.txt").read().splitlines()]
    assert [r[:2] for r in rows1] == [r[:2] for r in rows]
    assert max(abs(float(a[3]) - float(b[3])) / (int(a[4]) * float(tol(float(a[3]))) + 1e-6) for a, b in zip(rows, rows1)) <= 1.0


# ---------------------------------------------------------------- 9. shapes off the device loop: every row alone on the per-step loops
@pytest.mark.parametrize("over,knob", [({"ln": True}, None), ({"n_attn": 2}, None), ({"feed_attn": False}, None), ({}, 0)],
                         ids=["ln", "n_attn2", "no_feed_attn", "persist0"])
def test_fallback_shapes_run_every_row_alone(over, knob, tune):
    lens, T, S = [9, 1, 5, 9, 2], 9, 6
    m, rb = _synthetic(MID, lens, T, 13, **over)
    y = targets(len(lens), S + 1, MID["V"], seed=4, go_first=True)
    ref = _alone(m, rb, S, y, ("greedy", "sampled", "forced"))
    dev = {}
    if knob is not None:
        dev = {mode: _run(m, rb, mode, S, y) for mode in ("scored", "forced")}
        assert all(p == "device" for _, p in dev.values())
        tune("dec.persist", knob)
    print()
    got = {mode: _check_mode("fallback", m, rb, mode, S, y, ref, path="steps") for mode in ("greedy", "scored", "sampled", "forced")}
    if dev:         # the plain model: the per-step path against the device loop
        ok = guard(ref["greedy"].tokens, ref["greedy"].gaps, GAP)
        a, b = dev["scored"][0], got["scored"]
        assert (a.tokens[ok] == b.tokens[ok]).all() and (np.abs(a.logp.astype(np.float64) - b.logp)[ok] <= tol(b.logp.astype(np.float64))[ok]).all()
        a, b = dev["forced"][0], got["forced"]
        assert (np.abs(a.logp.astype(np.float64) - b.logp) <= tol(b.logp.astype(np.float64))).all() and np.abs(a.alpha - b.alpha).max() <= 1e-5


# ---------------------------------------------------------------- 10. bad arguments, and nothing else moved
def test_bad_rows_raise_before_anything_is_launched():
    from ast_amd.seq2seq import RowBatch
    m, rb = _synthetic(MID, [5, 3, 1], 5, 17)
    y = targets(3, 6, MID["V"], seed=4, go_first=True)
    X = torch.zeros(3, 120, 80)
    with pytest.raises(ValueError, match="rows"):
        m.score(None, y[:2], rows=rb)
    with pytest.raises(ValueError, match="B = 3"):
        m.predict_scored(None, GO, EOS, 5, y=y[:2], rows=rb)
    with pytest.raises(ValueError, match="streams"):
        m.sample(None, GO, EOS, 5, SEED, streams=[0, 1], rows=rb)
    with pytest.raises(ValueError, match="not both"):
        m.predict(X, GO, EOS, 5, rows=rb)
    with pytest.raises(ValueError, match="RowBatch"):
        m.predict(None, GO, EOS, 5, rows=(rb.enc, rb.lens))
    with pytest.raises(ValueError, match="X or rows"):
        m.predict(None, GO, EOS, 5)
    with pytest.raises(ValueError, match="H ="):
        m.predict(None, GO, EOS, 5, rows=RowBatch(torch.zeros(2, 4, 32), [4, 4], torch.zeros(2, 2, 32), torch.zeros(2, 2, 32)))
    with pytest.raises(ValueError, match="32"):
        m.encode_rows([X[:1]] * 2, rows_of=[0, 1] * 17)
    with pytest.raises(ValueError, match="rows_of"):
        m.encode_rows([X[:1]], rows_of=[0, 1])


def test_predict_score_and_training_are_untouched_by_a_masked_decode():
    from ast_amd.seq2seq import using_config
    from oracle import ast_ref as R
    cfg, P, X, m = setup(MID, 17, 120, seed=9, eos_bias=8.0)
    rng = np.random.default_rng(3)
    y = rng.integers(1, MID["V"], size=(17, 12)).astype(np.int32)
    Xt = torch.from_numpy(X)
    a = m.predict(Xt, GO, EOS, 30)
    sa = m.predict_scored(Xt, GO, EOS, 30, y=torch.from_numpy(y))
    fa = m.score(Xt, y)
    assert m.last_predict_path == "device" and m.last_score_path == "device"
    rb = m.encode_rows([Xt[b, :T] for b, T in ((0, 120), (1, 64), (2, 8), (3, 100))], rows_of=[0, 0, 1, 2, 3, 3, 2])
    assert rb.lens.tolist() == [30, 30, 16, 2, 25, 25, 2]
    for _ in range(2):
        m.score(None, y[:7], return_alpha=True, rows=rb)
        m.sample(None, GO, EOS, 30, SEED, rows=rb)
        m.predict_scored(None, GO, EOS, 30, y=y[:7], rows=rb)
    assert m.last_predict_path == "device" and m.last_score_path == "device"
    b = m.predict(Xt, GO, EOS, 30)
    sb = m.predict_scored(Xt, GO, EOS, 30, y=torch.from_numpy(y))
    fb = m.score(Xt, y)
    bits = lambda v: v.view(np.uint32)
    assert a.shape == b.shape and (a == b).all()
    assert (sa.tokens == sb.tokens).all() and (bits(sa.logp) == bits(sb.logp)).all() and (bits(sa.nll) == bits(sb.nll)).all() and sa.loss == sb.loss
    assert (bits(fa.logp) == bits(fb.logp)).all() and (fa.pred == fb.pred).all() and fa.loss == fb.loss
    assert _status_is_clear()
    # a train step after the masked decodes gives the same bits as on a model that never decoded
    _, _, _, fresh = setup(MID, 17, 120, seed=9, eos_bias=8.0)
    Xs, ys = R.synth_batch(17, 120, 80, 9, MID["V"], seed=21, dtype=np.float32)
    out = []
    for g in (m, fresh):
        g.deterministic = True
        g.inject = {"use_truth": [1] * 8, "enc_masks": None, "emb_mask": None, "rnn_masks": None}
        with using_config("train", True):
            loss = g.forward_loss(torch.from_numpy(Xs), torch.from_numpy(ys), 1.0)
            g.cleargrads()
            loss.backward()
        torch.cuda.synchronize()
        out.append((float(loss.data), g.arena.grad.clone()))
    assert out[0][0] == out[1][0]
    assert torch.equal(out[0][1], out[1][1])
