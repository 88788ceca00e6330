"""NN drop-in (nn.py:42-322 of the reference): builds the model + optimizer from <cfg_dir>, resumes from the newest
seq2seq_<N>.model, and runs the train step of nn.py:168-194 -- forward_loss -> cleargrads -> backward -> update --
on the HIP path.  Data-parallel runs (one process per GPU, torchrun) shard every bucketed batch over the ranks and
all-reduce the flat gradient arena over RCCL before the hooks (ast_amd.dist)."""
import itertools
import math
import os
import random

import torch
from tqdm import tqdm

from . import dist as adist
from . import mrt, optimizers, serializers
from .config import Config
from .dataloader import SYMBOLS, FisherDataLoader, GlobalPhoneDataLoader, SyntheticDataLoader
from .seq2seq import (SpeechEncoderDecoder, checked_ctc_weight, checked_label_smoothing, ctc_count_of, raise_if_aborted,
                      using_config)
from .spec_augment import checked_spec_augment

_ADAM = 0
_SGD = 1


# ---- beam search (nn.py:235-322 of the reference): one utterance, N best hypotheses kept, K expansions per live hypothesis.
# Module-level so that it works on a bare SpeechEncoderDecoder too; NN.decode_beam / init_hyp / decode_beam_step delegate here.
def init_hyp(model):
    import torch
    return {"hyp": [SYMBOLS.GO_ID], "score": 0, "dec_state": model.get_encoder_states(),
            "attn_v": torch.zeros(1, model.cfg["rnn_config"]["attn_units"], dtype=torch.float32, device=model.device), "attn_history": []}


def decode_beam_step(model, decode_entry, beam_width):
    import torch
    with using_config("train", False):
        model.set_decoder_states(decode_entry["dec_state"])
        word = torch.full((1,), int(decode_entry["hyp"][-1]), dtype=torch.int32)
        logits, ht, alphas = model.decode_step(word, decode_entry["attn_v"])
        logp = torch.log_softmax(logits[0].double(), dim=0).cpu().numpy()
        top = logp.argsort()[-beam_width:]
        state = model.get_decoder_states()
        return [{"hyp": decode_entry["hyp"] + [int(pi)], "score": decode_entry["score"] + float(logp[pi]), "dec_state": state, "attn_v": ht,
                 "attn_history": decode_entry["attn_history"] + [alphas.squeeze().cpu().numpy()]} for pi in top[::-1]]


def checked_beam_ctc_weight(model, ctc_weight, only_batch=None):
    """ctc_weight of a beam search as a float in [0, 1] (checked_ctc_weight's rules, and at most 1: the two terms' weights are
    1 - w and w); a positive one needs the model's CTC head.  only_batch names the entry point that cannot rank jointly."""
    w = checked_ctc_weight(ctc_weight, bool(getattr(model, "ctc_head", False)))
    if w > 1.0:
        raise ValueError(f"ctc_weight must be <= 1 in beam search (the terms weigh 1 - w and w), got {ctc_weight!r}")
    if w > 0.0 and only_batch:
        raise ValueError(f"{only_batch}: ctc_weight > 0 (joint CTC-attention ranking) runs in decode_beam_batch only")
    return w


# beam.py's joint decoding options live here, with the search they configure: the command line itself stays the reference's.
def add_joint_decoding_arguments(parser):
    parser.add_argument("--ctc-weight", dest="ctc_weight", type=float, default=0.0,
                        help="joint CTC-attention decoding: weight of the CTC prefix score in the ranking, 0..1 (needs -b U and rnn_config.ctc)")


def joint_decoding_kwargs(args, batched, device):
    """The keyword arguments of decode_beam_batch for the parsed options (none: the plain search); SystemExit with a message where the
    search that would run cannot rank jointly (no -b U, or --device)."""
    from . import _lib
    w = args["ctc_weight"]
    if w == 0:
        return {}
    if not batched or device:
        raise SystemExit("--ctc-weight: joint CTC-attention ranking runs in decode_beam_batch only: give -b U (N, K at most {0:d} / {1:d}) "
                         "and drop --device".format(_lib.BEAM_MAX_N, _lib.BEAM_MAX_K))
    return {"ctc_weight": w}


def joint_entry_scores(entry):
    """(att_score, ctc_score) of an n-best entry of a joint search, () of a plain one: what beam.py appends to its pickle's tuples."""
    return (entry["att_score"], entry["ctc_score"]) if "ctc_score" in entry else ()


def decode_beam(model, X, stop_limit, N, K, ctc_weight=0.0):
    checked_beam_ctc_weight(model, ctc_weight, "decode_beam")
    with using_config("train", False):
        model.encode(X)
        n_best = [init_hyp(model)]
        for _ in range(stop_limit):
            if all(e["hyp"][-1] == SYMBOLS.EOS_ID for e in n_best):
                break
            cur = []
            for e in n_best:
                if e["hyp"][-1] != SYMBOLS.EOS_ID:
                    cur.extend(decode_beam_step(model, e, K))
                else:
                    cur.append(e)
            n_best = sorted(cur, reverse=True, key=lambda t: t["score"])[:N]
    return n_best


def decode_beam_batch(model, Xs, stop_limit, N, K, ctc_weight=0.0):
    """decode_beam for many utterances at once: Xs is a list of (1, T_u, D) inputs; returns one N-best list per utterance, each the
    list decode_beam(model, Xs[u], stop_limit, N, K) returns (same hypotheses, order and types).  Every slot of every utterance is one
    row of a single decoder step (include/astk.h astk_beam_step: decoder step, float64 top-K / top-N selection and state gather on the
    device); the host reads one counter per step, a step late, and backtracks the device's history once at the end.
    ctc_weight = w > 0 (extension; needs rnn_config.ctc): joint CTC-attention decoding -- the K proposals of
    every live hypothesis are ranked by (1 - w) * log p_att + w * log p_ctc(prefix) (astk_beam_step_ctc; the head runs once per search
    on the padded encoder states); "score" is that joint score and every dict gains "att_score" and "ctc_score" (the CTC prefix
    score, for a finished hypothesis log p_ctc of exactly its tokens).  0 is the search above: nothing else is allocated or launched."""
    import ctypes as C
    import numpy as np
    from . import _lib
    ctc_weight = checked_beam_ctc_weight(model, ctc_weight)
    if not (1 <= N <= _lib.BEAM_MAX_N and 1 <= K <= _lib.BEAM_MAX_K):
        raise ValueError(f"decode_beam_batch: N = {N} and K = {K} must lie in 1..{_lib.BEAM_MAX_N} / 1..{_lib.BEAM_MAX_K} (use decode_beam)")
    lib = model._require_gpu()
    dev = model.device
    GO, EOS = SYMBOLS.GO_ID, SYMBOLS.EOS_ID
    with using_config("train", False):
        # ---- every utterance encoded at its own length (no length masks in the encoder, quirk Q2), copied out of the pooled buffers
        seeds = []
        encs, _, _ = model._encode_utts(Xs, seeds)      # (model.batch_encode: padded batches with per-row lengths)
        if stop_limit <= 0:
            return [[_init_hyp_from(model, s)] for s in seeds]
        U, nl, H, A, V = len(Xs), len(model.rnn_dec), model.H, model.A, model.V
        R, lens = U * N, [int(e.shape[0]) for e in encs]
        Tmax = max(lens)
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        enc = torch.zeros(U, Tmax, H, **f32)
        c, h = torch.zeros(nl, R, H, **f32), torch.zeros(nl, R, H, **f32)
        # slot 0 of utterance u: the encoder's final states layer by layer (set_decoder_states(get_encoder_states()) of init_hyp)
        for u, (e, sd) in enumerate(zip(encs, seeds)):
            enc[u, :lens[u]] = e
            for l in range(min(nl, len(sd["c"]))):
                c[l, u * N] = sd["c"][l][0]
                h[l, u * N] = sd["h"][l][0]
        ht = torch.zeros(R, A, **f32)
        tokens = torch.full((R,), GO, **i32)
        score = torch.zeros(R, dtype=torch.float64, device=dev)
        status = torch.zeros(R, **i32)
        status[::N] = 1
        frozen, n_frozen = torch.zeros(U, **i32), torch.zeros(1, **i32)
        hist = torch.zeros(stop_limit, R, 4, **i32)
        hist_alpha = torch.empty(stop_limit, R, Tmax, **f32)
        row_utt = torch.arange(R, **i32) // N
        row_len = torch.tensor(lens, **i32)[row_utt.long()].contiguous()
        lens_host = np.asarray(lens, dtype=np.int32)
        bd = _lib.BeamDesc(U, N, K, stop_limit, Tmax, V, EOS, lens_host.ctypes.data_as(C.POINTER(C.c_int32)))
        bs = _lib.BeamState(*[t.data_ptr() for t in (row_utt, row_len, c, h, ht, tokens, score, status, frozen, n_frozen, hist, hist_alpha)])
        dd = _lib.DecoderDesc.from_buffer_copy(model._cur["dd"])
        dd.B, dd.T, dd.L, dd.status_dst, dd.use_truth_host = R, Tmax, 2, None, None
        nbytes = int(lib.astk_beam_workspace_bytes(C.byref(bd), C.byref(dd)))
        if nbytes == 0:
            _lib.check(-1)
        ws = model._workspace("beam", nbytes)
        dp, stream = model._cur["dp"], torch.cuda.current_stream(dev)
        sp = C.c_void_p(stream.cuda_stream)
        bc = None
        if ctc_weight > 0:
            # ---- the head once on the padded (U, Tmax, H) encoder states, then the per-frame lse, the (U, V, T) copy and the empty prefix
            from .seq2seq import PAD_ID, UNK_ID
            if Tmax > _lib.BEAM_CTC_MAX_T:
                raise ValueError(f"decode_beam_batch: ctc_weight > 0 with T'' = {Tmax} above ASTK_BEAM_CTC_MAX_T = {_lib.BEAM_CTC_MAX_T}")
            Vp = (V + 3) // 4 * 4
            ctc_logits = torch.zeros(U * Tmax, Vp, **f32)
            _lib.check(lib.astk_ctc_head_fwd(U * Tmax, V, H, C.c_void_p(enc.data_ptr()), model.arena.p("ctc_out/W"), model.arena.p("ctc_out/b"),
                                             C.c_void_p(ctc_logits.data_ptr()), Vp, _lib.PREC_BY_NAME[model.gemm_precision], sp))
            f64 = dict(dtype=torch.float64, device=dev)
            ctc_state = torch.empty(R, Tmax, 2, **f64)
            att_score, psi, n_labels = torch.zeros(R, **f64), torch.zeros(R, **f64), torch.zeros(R, **i32)
            bc = _lib.BeamCtc(ctc_weight, PAD_ID, UNK_ID, ctc_logits.data_ptr(), Vp, ctc_state.data_ptr(), att_score.data_ptr(),
                              psi.data_ptr(), n_labels.data_ptr(), None, 0)
            cbytes = int(lib.astk_beam_ctc_workspace_bytes(C.byref(bd), C.byref(bc)))
            if cbytes == 0:
                _lib.check(-1)
            cws = model._workspace("beam_ctc", cbytes)
            bc.ws, bc.ws_bytes = cws.data_ptr(), cws.numel()
            _lib.check(lib.astk_beam_ctc_init(C.byref(bd), C.byref(bs), C.byref(bc), sp))
            model.last_beam_ctc = (ctc_logits.view(U, Tmax, Vp)[:, :, :V], lens)     # the head's logits and T''_u, for callers that re-score
        # ---- the loop: one astk_beam_step per step; the frozen-utterance count of step s is read after step s+1 is enqueued (steps on
        # frozen utterances only carry them again, so a step too many changes nothing)
        seen = torch.zeros(2, dtype=torch.int32, pin_memory=True)
        events, steps = [None, None], 0
        for step in range(stop_limit):
            if bc is None:
                _lib.check(lib.astk_beam_step(C.byref(bd), C.byref(dd), C.byref(dp), C.c_void_p(enc.data_ptr()), C.byref(bs), step,
                                              C.c_void_p(ws.data_ptr()), ws.numel(), sp))
            else:
                _lib.check(lib.astk_beam_step_ctc(C.byref(bd), C.byref(dd), C.byref(dp), C.c_void_p(enc.data_ptr()), C.byref(bs), C.byref(bc),
                                                  step, C.c_void_p(ws.data_ptr()), ws.numel(), sp))
            steps = step + 1
            slot = step % 2
            seen[slot:slot + 1].copy_(n_frozen, non_blocking=True)
            events[slot] = torch.cuda.Event()
            events[slot].record(stream)
            if step > 0:
                events[1 - slot].synchronize()
                if int(seen[1 - slot]) >= U:
                    break
        stream.synchronize()
        # ---- backtrack the history once
        H_ = hist[:steps].cpu().numpy()
        sc, stt = score.cpu().numpy(), status.cpu().numpy()
        found, rows_s, rows_r = [], [], []
        for u in range(U):
            lst = []
            for i, toks, trace in backtrack_beam_history(H_[:, u * N:(u + 1) * N], stt[u * N:(u + 1) * N]):
                arow = list(range(len(rows_s), len(rows_s) + len(trace)))
                rows_s.extend(s for s, _, _ in trace)
                rows_r.extend(u * N + j for _, j, _ in trace)
                lst.append((u * N + i, toks, arow))
            found.append(lst)
        alphas = hist_alpha[torch.tensor(rows_s, dtype=torch.long, device=dev), torch.tensor(rows_r, dtype=torch.long, device=dev)].cpu().numpy() \
            if rows_s else np.zeros((0, Tmax), np.float32)
        out = []
        for u, lst in enumerate(found):
            out.append([{"hyp": [GO] + toks, "score": float(sc[r]),
                         "dec_state": {"c": [c[l, r:r + 1].clone() for l in range(nl)], "h": [h[l, r:r + 1].clone() for l in range(nl)]},
                         "attn_v": ht[r:r + 1].clone(), "attn_history": [alphas[k, :lens[u]].copy() for k in arow]}
                        for r, toks, arow in lst])
        if bc is not None:
            att, ps = att_score.cpu().numpy(), psi.cpu().numpy()
            for lst, entries in zip(found, out):
                for (r, _, _), e in zip(lst, entries):
                    e["att_score"], e["ctc_score"] = float(att[r]), float(ps[r])
        return out


def backtrack_beam_history(hist, status):
    """The hypotheses of ONE utterance from its history (include/astk.h astk_beam_state.hist): hist (steps, N, >= 3) int -- per step
    and new slot its parent slot, token and carried flag -- and status (N) of the slots after the last step (0 = empty: the kept slots
    come first).  Returns [(slot i, tokens, trace)] for every kept slot in order: its tokens without GO, and trace = [(step, slot,
    parent slot)] of the expansions that produced them, in step order (a carried step adds no token).  The per-step search keeps an
    expansion's attention row with its new slot, the device loop with its parent row.  Host only."""
    import numpy as np
    out = []
    hist = np.asarray(hist).tolist()          # (plain ints: the walk below touches every step of every kept slot)
    for i in range(len(status)):
        if int(status[i]) == 0:
            break
        toks, trace, j = [], [], i
        for s in range(len(hist) - 1, -1, -1):
            p, t, carried = hist[s][j][:3]
            if not carried:
                toks.append(t)
                trace.append((s, j, p))
            j = p
        out.append((i, toks[::-1], trace[::-1]))
    return out


def plan_beam_tiles(n_utts, N, max_rows=32):
    """The rows of a device beam search (include/astk.h astk_beam_decode): the N slots of an utterance lie inside one 16-row tile, a tile
    holds 16 // N utterances, a launch max_rows // 16 tiles.  Returns a list of launches, each (B, [(utterance, first row)]) with B =
    the launch's row count (it ends with the last slot of its last utterance).  Host only."""
    n_utts, N = int(n_utts), int(N)
    from . import _lib
    if not 1 <= N <= _lib.BEAM_MAX_N:
        raise ValueError(f"plan_beam_tiles: N = {N} outside 1..{_lib.BEAM_MAX_N}: the slots of an utterance must fit one 16-row tile")
    if n_utts < 0 or max_rows < 16 or max_rows % 16:
        raise ValueError(f"plan_beam_tiles: {n_utts} utterances, max_rows = {max_rows} (a positive multiple of 16)")
    per_tile = 16 // N
    per_launch = per_tile * (max_rows // 16)
    launches = []
    for lo in range(0, n_utts, per_launch):
        rows = [(u, 16 * ((u - lo) // per_tile) + N * ((u - lo) % per_tile)) for u in range(lo, min(n_utts, lo + per_launch))]
        launches.append((rows[-1][1] + N, rows))
    return launches


def decode_beam_device(model, Xs, stop_limit, N, K, ctc_weight=0.0):
    """decode_beam_batch with the whole search of up to 32 rows in ONE persistent launch (include/astk.h astk_beam_decode): the same
    return value -- keys, types and order.  Utterances are packed into launches by plan_beam_tiles; every launch's results come back
    in one copy into one of two pinned buffers, read after the next launch has been enqueued.  Shapes the library does not run on
    the device loop (its workspace query returns 0) go to decode_beam_batch; model.last_beam_path says which ran ("device" / "steps").
    An utterance's hypotheses and score bits do not depend on the utterances it shares a launch with."""
    import ctypes as C
    import numpy as np
    from . import _lib
    from .seq2seq import _Pending, _vp
    checked_beam_ctc_weight(model, ctc_weight, "decode_beam_device")
    if not (1 <= N <= _lib.BEAM_MAX_N and 1 <= K <= _lib.BEAM_MAX_K):
        raise ValueError(f"decode_beam_device: N = {N} and K = {K} must lie in 1..{_lib.BEAM_MAX_N} / 1..{_lib.BEAM_MAX_K} (use decode_beam)")
    lib = model._require_gpu()
    dev = model.device
    GO, EOS = SYMBOLS.GO_ID, SYMBOLS.EOS_ID
    stop = int(stop_limit)
    with using_config("train", False):
        seeds = []
        encs, _, _ = model._encode_utts(Xs, seeds)      # (model.batch_encode: padded batches with per-row lengths)
        if stop <= 0:
            model.last_beam_path = None          # (no search ran)
            return [[_init_hyp_from(model, s)] for s in seeds]
        nl, H, A = len(model.rnn_dec), model.H, model.A
        lens = [int(e.shape[0]) for e in encs]
        launches = plan_beam_tiles(len(Xs), N)
        dp, _ = model._decoder_tables()

        def desc(B, T2):
            dd = model._decoder_desc(B, 2, T2)
            dd.precision, dd.gemm_operands = _lib.PREC_BY_NAME[model.gemm_precision], _lib.OPERANDS_BY_NAME[model.gemm_operands]
            dd.deterministic = 1 if model.deterministic else 0
            return dd
        # (a row's arithmetic does not depend on its launch: the kernel cuts every row's attention by the row's own length)
        plans = []
        for B, rows in launches:
            T2 = max(lens[u] for u, _ in rows)
            dd = desc(B, T2)
            plans.append((B, rows, T2, dd, int(lib.astk_beam_decode_workspace_bytes(C.byref(dd), N, K, stop, 1))))
        if any(p[4] == 0 for p in plans):
            model.last_beam_path = "steps"
            return decode_beam_batch(model, Xs, stop_limit, N, K)
        model.last_beam_path, model.last_beam_steps = "device", []          # (the steps every launch ran: its n_steps)
        f32 = dict(dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev)

        def enqueue(k):
            B, rows, T2, dd, nbytes = plans[k]
            enc = torch.zeros(B, T2, H, **f32)
            c0, h0 = torch.zeros(nl, B, H, **f32), torch.zeros(nl, B, H, **f32)
            row_len = np.ones(B, dtype=np.int32)          # (padding rows attend over one zero position: finite, never live)
            for u, r0 in rows:
                enc[r0:r0 + N, :lens[u]] = encs[u]
                row_len[r0:r0 + N] = lens[u]
                sd = seeds[u]          # slot 0: the encoder's final states layer by layer (set_decoder_states(get_encoder_states()))
                for l in range(min(nl, len(sd["c"]))):
                    c0[l, r0] = sd["c"][l][0]
                    h0[l, r0] = sd["h"][l][0]
            row_len_dev = torch.from_numpy(row_len).to(dev)
            # words: [n_steps, status word (float), 2 pad | hist (S, B, 4) | slot status (B) | score (B) float64 | c, h (nl, B, H) | ht (B, A)
            #         | alpha (S, B, T2)]
            o_hist, o_st = 4, 4 + stop * B * 4
            o_sc = (o_st + B + 1) // 2 * 2
            o_c = o_sc + 2 * B
            o_h, o_ht = o_c + nl * B * H, o_c + 2 * nl * B * H
            o_al = o_ht + B * A
            n = o_al + stop * B * T2
            ws = model._workspace("decode", nbytes)
            out, host = model._readback("beam_device", k % 2, n, torch.int32)
            base = out.data_ptr()
            at = lambda w: C.c_void_p(base + 4 * w)
            _lib.check(lib.astk_beam_decode(C.byref(dd), C.byref(dp), _vp(enc), _vp(c0), _vp(h0), _vp(row_len_dev), N, K, GO, EOS, stop, at(0),
                                            at(1), at(o_hist), at(o_st), at(o_sc), at(o_c), at(o_h), at(o_ht), at(o_al), _vp(ws), ws.numel(),
                                            C.c_void_p(stream.cuda_stream)))
            host.copy_(out, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)

            def parse(v, _):
                steps = int(v[0])
                model.last_beam_steps.append(steps)
                hist = v[o_hist:o_hist + stop * B * 4].reshape(stop, B, 4)[:steps]
                stt, sc = v[o_st:o_st + B], v[o_sc:o_sc + 2 * B].view(np.float64)
                alpha = v[o_al:o_al + stop * B * T2].view(np.float32).reshape(stop, B, T2)
                # the final states stay on the device: one copy of the launch's (the buffer is reused two launches on), cut into rows
                dev_f = out.view(torch.float32)[o_c:o_al].clone()
                state = lambda o, r, w, l=0: dev_f[o - o_c + (l * B + r) * w:o - o_c + (l * B + r) * w + w].reshape(1, w)

                def history(u, r0, trace):          # the alpha of every expansion, from the PARENT row of its step: one gather
                    if not trace:
                        return []
                    return list(alpha[[s for s, _, _ in trace], [r0 + p for _, _, p in trace], :lens[u]])
                res = []
                for u, r0 in rows:
                    res.append([{"hyp": [GO] + toks, "score": float(sc[r0 + i]),
                                 "dec_state": {"c": [state(o_c, r0 + i, H, l) for l in range(nl)], "h": [state(o_h, r0 + i, H, l) for l in range(nl)]},
                                 "attn_v": state(o_ht, r0 + i, A), "attn_history": history(u, r0, trace)}
                                for i, toks, trace in backtrack_beam_history(hist[:, r0:r0 + N], stt[r0:r0 + N])])
                return res
            return _Pending(host, None, ev, status_at=1, where="decode_beam_device", parse=parse, keep=(enc, c0, h0, row_len_dev))
        out_lists, pending = [], None
        for k in range(len(plans) + 1):
            cur = enqueue(k) if k < len(plans) else None
            if pending is not None:
                out_lists.extend(pending.result())
            pending = cur
        return out_lists


def score_hypotheses(model, X, hyps, return_alpha=False):
    """Forced scores of several token lists for ONE utterance: X (1, T, D) is repeated over the rows and the lists `hyps` (each
    [GO, t1, .., tn], as beam search returns them) are PAD-padded to one length -- the encoding decode_beam saw (score_hypotheses_packed
    scores several utterances per call).  Returns (scores, r): scores[i] = the float64 sum of log p(t_k | t_<k) over hypothesis i's own n steps (a PAD id
    inside a hypothesis counts like any other token, the padding behind it does not), r = the ForcedScore of the padded batch."""
    import numpy as np
    X = model._as_input(X)
    if X.dim() == 2:
        X = X[None]
    y = np.zeros((len(hyps), max(2, max(len(h) for h in hyps))), dtype=np.int32)
    for i, h in enumerate(hyps):
        y[i, :len(h)] = h
    r = model.score(X.expand(len(hyps), -1, -1), y, return_alpha=return_alpha)
    return [float(r.logp[i, :len(h) - 1].astype(np.float64).sum()) for i, h in enumerate(hyps)], r


# ---- ancestral sampling: n scored samples of one utterance, and a minimum-Bayes-risk choice among them
def cut_at_eos(tokens, end_token=SYMBOLS.EOS_ID):
    """A decoded row as a token list cut behind its first `end_token`, keeping it (the whole row when it has none)."""
    toks = [int(t) for t in tokens]
    return toks[:toks.index(end_token) + 1] if end_token in toks else toks


# ---- rows of several utterances in one call (SpeechEncoderDecoder.encode_rows, rows=): every row attends over its own utterance's length
def plan_row_packs(counts, max_utts=None, max_rows=32):
    """Packs the rows of consecutive utterances into calls: counts[u] = the rows utterance u needs; returns a list of calls, each a
    list of (u, lo, hi) -- rows lo..hi-1 of utterance u -- in order, with at most max_rows rows and at most max_utts utterances per
    call.  An utterance that fits a call is never split: it opens a new call when the current one has no room for all of it.  One with
    more than max_rows rows opens a call of its own and is split across calls, max_rows at a time; the remainder shares its call with
    the utterances behind it.  Utterances without rows appear in no call.  Host only."""
    max_rows = int(max_rows)
    max_utts = max_rows if max_utts is None else int(max_utts)
    if max_rows < 1 or max_utts < 1:
        raise ValueError(f"plan_row_packs: max_rows = {max_rows} and max_utts = {max_utts} must be at least 1")
    calls, cur, used = [], [], 0
    for u, n in enumerate(int(c) for c in counts):
        if n < 0:
            raise ValueError(f"plan_row_packs: utterance {u} has {n} rows")
        lo = 0
        while lo < n:
            if cur and (len(cur) == max_utts or used == max_rows or (lo == 0 and n > max_rows - used)):
                calls.append(cur)
                cur, used = [], 0
            take = min(n - lo, max_rows - used)
            cur.append((u, lo, lo + take))
            used += take
            lo += take
    if cur:
        calls.append(cur)
    return calls


def _pack_rows(model, Xs, call):
    """The RowBatch of one planned call (each of its utterances encoded once) and rows_of, the call's piece index of every row."""
    rows_of = [k for k, (_, lo, hi) in enumerate(call) for _ in range(hi - lo)]
    return model.encode_rows([Xs[u] for u, _, _ in call], rows_of), rows_of


def score_hypotheses_packed(model, Xs, hyps_lists, return_alpha=False, max_utts=None):
    """score_hypotheses for many utterances, their hypotheses packed into calls of up to 32 rows (plan_row_packs; at most max_utts
    utterances per call): Xs a list of (1, T_u, D) inputs, hyps_lists[u] the token lists of utterance u.  Returns one (scores, r) per
    utterance as score_hypotheses returns them -- r the ForcedScore of the utterance's own PAD-padded batch, its alpha (n, L_u - 1,
    T''_u) -- and ([], None) for an utterance without hypotheses."""
    import numpy as np
    from .seq2seq import ForcedScore
    ys = []
    for hyps in hyps_lists:
        y = np.zeros((len(hyps), max([2] + [len(h) for h in hyps])), dtype=np.int32)
        for i, h in enumerate(hyps):
            y[i, :len(h)] = h
        ys.append(y)
    parts = [[] for _ in Xs]
    for call in plan_row_packs([len(h) for h in hyps_lists], max_utts):
        rows, _ = _pack_rows(model, Xs, call)
        L = max(ys[u].shape[1] for u, _, _ in call)
        y = np.zeros((rows.B, L), dtype=np.int32)
        at = 0
        for u, lo, hi in call:
            y[at:at + hi - lo, :ys[u].shape[1]] = ys[u][lo:hi]
            at += hi - lo
        r = model.score(None, y, return_alpha=return_alpha, rows=rows)
        at = 0
        for u, lo, hi in call:
            S, T2 = ys[u].shape[1] - 1, int(rows.lens[at])
            cut = lambda a: a[at:at + hi - lo, :S]
            parts[u].append((cut(r.logp), cut(r.logp_max), cut(r.pred), cut(r.alpha)[:, :, :T2] if return_alpha else None))
            at += hi - lo
    out = []
    for u, hyps in enumerate(hyps_lists):
        if not hyps:
            out.append(([], None))
            continue
        cat = lambda k: np.concatenate([p[k] for p in parts[u]], axis=0)
        r = ForcedScore(cat(0), cat(1), cat(2), (ys[u][:, 1:] != 0).astype(np.float32), cat(3) if return_alpha else None)
        out.append(([float(r.logp[i, :len(h) - 1].astype(np.float64).sum()) for i, h in enumerate(hyps)], r))
    return out


def sample_hypotheses_packed(model, Xs, n, stop_limit, seed, temperature=1.0, first_streams=None, max_utts=None, top_k=None, top_p=1.0):
    """sample_hypotheses for many utterances, their n rows each packed into calls of up to 32 rows (plan_row_packs; at most max_utts
    utterances per call).  Utterance k draws from the streams first_streams[k] .. first_streams[k] + n - 1 of `seed` (default k * n:
    the numbering of NN.sample_set), so packing does not change which samples an utterance gets.  Returns one list per utterance as
    sample_hypotheses returns it.  top_k / top_p: truncated sampling (SpeechEncoderDecoder.sample)."""
    n = int(n)
    first_streams = [k * n for k in range(len(Xs))] if first_streams is None else [int(v) for v in first_streams]
    if len(first_streams) != len(Xs):
        raise ValueError(f"sample_hypotheses_packed: first_streams must name {len(Xs)} utterances, got {len(first_streams)}")
    out = [[] for _ in Xs]
    for call in plan_row_packs([n] * len(Xs), max_utts):
        rows, _ = _pack_rows(model, Xs, call)
        streams = [first_streams[u] + i for u, lo, hi in call for i in range(lo, hi)]
        r = model.sample(None, SYMBOLS.GO_ID, SYMBOLS.EOS_ID, stop_limit, seed, streams=streams, temperature=temperature, rows=rows,
                         top_k=top_k, top_p=top_p)
        at = 0
        for u, lo, hi in call:
            out[u].extend({"hyp": [SYMBOLS.GO_ID] + cut_at_eos(r.tokens[i]), "score": float(r.score[i])} for i in range(at, at + hi - lo))
            at += hi - lo
    return out


def sample_hypotheses(model, X, n, stop_limit, seed, temperature=1.0, first_stream=0, top_k=None, top_p=1.0):
    """n samples of ONE utterance X (1, T, D), drawn by SpeechEncoderDecoder.sample from the streams first_stream .. first_stream + n - 1
    of `seed`: X is repeated over the rows (the encoding decode_beam sees; sample_hypotheses_packed packs several utterances), at most 32 rows -- the device
    loop's batch -- per call.  Returns a list in stream order of {"hyp": [GO, t1, .., tk], "score": float}, each cut behind its first
    EOS and keeping it, like decode_beam's entries; score = the log-probability of t1..tk under the sampled distribution.  A stream's
    sample does not depend on n or on its row, so a list can be extended later from first_stream = n.
    top_k / top_p: truncated sampling (SpeechEncoderDecoder.sample) -- the score is then the log-probability under the renormalised
    kept set that was actually sampled, not the model's full-softmax log-probability (score_hypotheses gives that)."""
    X = model._as_input(X)
    if X.dim() == 2:
        X = X[None]
    out = []
    for lo in range(0, int(n), 32):
        m = min(32, int(n) - lo)
        r = model.sample(X.expand(m, -1, -1), SYMBOLS.GO_ID, SYMBOLS.EOS_ID, stop_limit, seed,
                         streams=range(first_stream + lo, first_stream + lo + m), temperature=temperature, top_k=top_k, top_p=top_p)
        out.extend({"hyp": [SYMBOLS.GO_ID] + cut_at_eos(r.tokens[i]), "score": float(r.score[i])} for i in range(m))
    return out


def mbr_select(hyps):
    """Minimum-Bayes-risk choice among samples (entries with "hyp" and "score", as sample_hypotheses returns): the index of the
    candidate with the highest mean sentence BLEU (ast_amd.eval.corpus_bleu, smoothed) against every OTHER sample as its reference.
    Ties go to the higher score, then to the lower index; a single hypothesis is its own choice.  Host only."""
    from .eval import corpus_bleu
    if not hyps:
        raise ValueError("mbr_select: no hypotheses")
    toks = [list(h["hyp"]) for h in hyps]
    best = None
    for i, cand in enumerate(toks):
        others = [r for j, r in enumerate(toks) if j != i]
        gain = sum(corpus_bleu([[r]], [cand]) for r in others) / len(others) if others else 0.0
        key = (gain, float(hyps[i]["score"]), -i)
        if best is None or key > best[0]:
            best = (key, i)
    return best[1]


def posterior_weights(scores, scale=1.0):
    """softmax(scale * score) in float64, the maximum subtracted: the weights mbr_select_lists takes when the members of a list are
    to count by their (scaled) posterior instead of equally."""
    z = [float(scale) * float(s) for s in scores]
    top = max(z)
    e = [math.exp(v - top) for v in z]
    total = sum(e)
    return [v / total for v in e]


def _mbr_choice(hyps, value, utility, weights):
    """The index mbr_select_lists returns for one list: value(i, j) is the sentence BLEU ("bleu") or the edit distance ("edit") of
    member i against member j as its reference.  Sums run over j in ascending order; ties go to the higher score, then the lower index."""
    n, best = len(hyps), None
    for i in range(n):
        others = [j for j in range(n) if j != i]
        if weights is None:
            total = sum(value(i, j) for j in others)
            merit = (total / len(others) if others else 0.0) if utility == "bleu" else -total
        else:
            mass = sum(float(weights[j]) for j in others)
            total = sum(float(weights[j]) * value(i, j) for j in others)
            merit = (total / mass if mass > 0.0 else 0.0) * (1.0 if utility == "bleu" else -1.0)
        key = (merit, float(hyps[i]["score"]), -i)
        if best is None or key > best[0]:
            best = (key, i)
    return best[1]


def mbr_select_lists(lists, utility="bleu", weights=None, device=None):
    """Minimum-Bayes-risk choice in many n-best lists at once: lists[u] holds the entries {"hyp", "score"} of
    utterance u; returns one chosen index per list.  The lists of a call share one pool and one astk_pair_stats launch over the pairs
    i < j inside each list (distance and matches are symmetric; the host fills both directions).
      utility="bleu"  the member with the highest mean sentence BLEU (ast_amd.eval.bleu_from_counts) against every other member as
                      its reference -- with weights=None exactly mbr_select(lst) for every list
      utility="edit"  the member with the least summed edit distance to the others (an integer)
    Ties go to the higher score, then the lower index; a one-element list chooses 0.  weights: one sequence per list (e.g.
    posterior_weights of its scores); the mean becomes the weighted mean over the other members, in float64 on the host.  A list with a
    hypothesis longer than PAIR_MAX_LEN tokens is handled on the host, that list only."""
    from .eval import PAIR_MAX_LEN, bleu_from_counts, clipped_matches, edit_stats, pair_stats
    if utility not in ("bleu", "edit"):
        raise ValueError(f"mbr_select_lists: utility must be \"bleu\" or \"edit\", got {utility!r}")
    if weights is not None and len(weights) != len(lists):
        raise ValueError(f"mbr_select_lists: {len(weights)} weight sequences for {len(lists)} lists")
    toks = []
    for u, lst in enumerate(lists):
        if not lst:
            raise ValueError("mbr_select_lists: no hypotheses in list {0:d}".format(u))
        if weights is not None and len(weights[u]) != len(lst):
            raise ValueError(f"mbr_select_lists: {len(weights[u])} weights for the {len(lst)} hypotheses of list {u}")
        toks.append([[int(t) for t in h["hyp"]] for h in lst])
    on_dev = [len(ts) > 1 and max(len(t) for t in ts) <= PAIR_MAX_LEN for ts in toks]
    pool, pairs = [], []
    for ts, f in zip(toks, on_dev):
        if f:
            base = len(pool)
            pool.extend(ts)
            pairs.extend((base + i, base + j) for i in range(len(ts)) for j in range(i + 1, len(ts)))
    rows = iter(pair_stats(pool, pairs, device).tolist())
    col = slice(4, 8) if utility == "bleu" else 0
    out = []
    for u, (lst, ts, f) in enumerate(zip(lists, toks, on_dev)):
        w = None if weights is None else weights[u]
        if f:
            table = {}
            for i in range(len(ts)):
                for j in range(i + 1, len(ts)):
                    table[i, j] = table[j, i] = next(rows)[col]
        elif utility == "bleu" and w is None:
            out.append(mbr_select(lst))
            continue
        else:
            table = {(i, j): clipped_matches(ts[i], ts[j]) if utility == "bleu" else edit_stats(ts[i], ts[j])[0]
                     for i in range(len(ts)) for j in range(len(ts)) if i != j}
        if utility == "bleu":
            out.append(_mbr_choice(lst, lambda i, j: bleu_from_counts(table[i, j], len(ts[i]), len(ts[j])), utility, w))
        else:
            out.append(_mbr_choice(lst, lambda i, j: table[i, j], utility, w))
    return out


def mbr_select_set(nbest, utility="bleu", posterior_scale=None, utts_per_call=1, device=None):
    """mbr_select_lists over an n-best pickle ({utt: [(hyp, score, ..), ..]}, as beam.py, ctc_decode.py and sample.py write it), the
    lists of utts_per_call utterances per launch: {utt: the chosen hyp}.  posterior_scale: weigh the members of a list by
    posterior_weights(scores, scale) instead of equally."""
    utts, chosen = list(nbest), {}
    for lo in range(0, len(utts), max(1, int(utts_per_call))):
        group = utts[lo:lo + max(1, int(utts_per_call))]
        lists = [[{"hyp": e[0], "score": e[1]} for e in nbest[u]] for u in group]
        weights = None if posterior_scale is None else [posterior_weights([e["score"] for e in lst], posterior_scale) for lst in lists]
        for u, k in zip(group, mbr_select_lists(lists, utility, weights, device)):
            chosen[u] = list(nbest[u][k][0])
    return chosen


def _init_hyp_from(model, enc_states):
    return {"hyp": [SYMBOLS.GO_ID], "score": 0, "dec_state": enc_states,
            "attn_v": torch.zeros(1, model.cfg["rnn_config"]["attn_units"], dtype=torch.float32, device=model.device), "attn_history": []}


def read_one_batch_late(nn, set_key, labels, enqueue):
    """The inference loop of an NN over a set, read one batch late like train_epoch's loss: enqueue(batch, slot) starts batch i on the
    read-back buffers of slot i % 2 (SpeechEncoderDecoder.predict_async) and returns its handle; what the handle holds is read after
    batch i+1 has been enqueued, so the device never waits for the host.  Yields (utts, padded target length or None, handle.result())."""
    pending = None
    with tqdm(total=nn.data_loader.n_utts[set_key], ncols=80, disable=adist.rank() != 0) as pbar:
        batches = nn.data_loader.get_batch(nn.cfg.train["batch_size"], set_key, train=False, labels=labels)
        for i, batch in enumerate(itertools.chain(batches, [None])):
            cur = None
            if batch is not None:
                with using_config("train", False):
                    cur = (batch["utts"], len(batch["X"]), int(batch["y"].shape[1]) if labels else None, enqueue(batch, i % 2))
            if pending is not None:
                utts, n, L, handle = pending
                yield utts, L, handle.result()
                pbar.update(n)
            pending = cur


class NN:
    def __init__(self, cfg_path, vocab_size=None):
        self.cfg = Config(cfg_path, vocab_size=vocab_size)
        # extension key: extras.label_smoothing = eps of the TRAINING loss (default 0 = the reference's loss).  The
        # training loop alone passes it: dev loss, predict_scored and score never smooth, so dev losses compare across runs with different eps.
        self.label_smoothing = checked_label_smoothing(self.cfg.train.get("extras", {}).get("label_smoothing", 0.0), "extras.label_smoothing")
        # extension key: extras.ctc_weight = weight of the auxiliary CTC loss on the encoder states in the TRAINING loss (default 0 = off;
        # needs model_cfg.json rnn_config.ctc).  Evaluation (dev loss, forced dev loss, beam, score, sample) never sees it.
        self.ctc_weight = checked_ctc_weight(self.cfg.train.get("extras", {}).get("ctc_weight", 0.0),
                                             bool(self.cfg.model["rnn_config"].get("ctc", False)), "extras.ctc_weight")
        self.ctc_epoch = None                          # (mean CTC term per utterance, rows without a path) of the last train_epoch
        # extension key: extras.mrt = {"samples", "alpha", "cost", "mle_weight", "max_len", "temperature", "top_k", "top_p", "seed",
        # "start_epoch"}: minimum-risk training (ast_amd.mrt); absent or null = off, nothing of the branch runs.
        # A train_epoch call runs MRT steps once `start_epoch` epochs have been trained (the checkpoint's and this object's together).
        ex_ = self.cfg.train.get("extras", {})
        self.mrt = mrt.checked_mrt(ex_.get("mrt"), "extras.mrt")
        mrt.checked_mrt_setup(self.mrt, self.ctc_weight, ex_.get("random_out", 0), adist.world_size(), "extras.mrt")
        self.mrt_epoch = None                          # mean expected cost per utterance of the last train_epoch that ran MRT steps
        self.mrt_stream = 0                            # the running sample counter: the first stream no step has drawn from (set below)
        self.epochs_trained = 0                        # train_epoch calls of this object
        self.model_dir = self.cfg.model["model_dir"]
        self.gpuid = self.cfg.train["gpuid"]
        if adist.is_distributed():
            self.gpuid = adist.local_rank()           # one process per GPU: the rank picks the device
        random.seed(self.cfg.train["seed"])            # nn.py:54 -- the teacher-forcing / shuffling stream (Q4)
        data = self.cfg.train["data"]
        kind = data.get("dataloader", "fisher")
        loader = {"globalphone": GlobalPhoneDataLoader, "synthetic": SyntheticDataLoader}.get(kind, FisherDataLoader)
        self.data_loader = loader(data, self.model_dir, self.gpuid)
        if adist.is_distributed():
            self.data_loader.rank, self.data_loader.world = adist.rank(), adist.world_size()
        self.get_model()
        self.mrt_stream = self.max_epoch << 40         # a resumed run draws behind every stream of the epochs already trained
        # extension key: extras.spec_augment = {"freq_masks", "freq_width", "time_masks", "time_width", "time_ratio", "fill", "seed"} masks
        # the TRAINING batches inside the loader (ast_amd.spec_augment); absent, null or {} = off.  Evaluation
        # batches are never masked.  A resumed run starts its presentation counter behind every counter of the epochs already trained.
        self.data_loader.spec_augment = checked_spec_augment(self.cfg.train.get("extras", {}).get("spec_augment"), "extras.spec_augment")
        self.data_loader.spec_counter = self.max_epoch << 40
        if self.data_loader.spec_augment is not None:
            print("SpecAugment: {0}".format(self.data_loader.spec_augment))
        if self.ctc_weight > 0:
            self.data_loader.keep_lens = True          # training batches carry batch["x_len"], the rows' true frame counts
            print("CTC weight: {0:g}".format(self.ctc_weight))
        # extension key (BASELINE configs[4], "fp16 MFMA GEMMs"): extras.gemm_operands = "fp16" runs the batched products of the CNN
        # layers >= 1 and of the encoder's input projection with fp16 operands / f32 accumulation; default "f32" (f32-accurate products)
        # extras.gemm_precision = "bf16x3" (library default: exact f32 operands as three bf16 terms) | "f32" (f32-input MFMAs) | "fp16x2"
        # (two scaled fp16 terms: faster, narrower than float32).  Both go into the op descriptors of THIS model (no process-wide state).
        ops = self.cfg.train.get("extras", {}).get("gemm_operands", "f32")
        if ops not in ("f32", "fp16"):
            raise ValueError("extras.gemm_operands must be 'f32' or 'fp16'")
        prec = self.cfg.train.get("extras", {}).get("gemm_precision")
        if prec not in (None, "bf16x3", "f32", "fp16x2"):
            raise ValueError("extras.gemm_precision must be 'bf16x3', 'f32' or 'fp16x2'")
        self.model.gemm_operands, self.model.gemm_precision = ops, prec
        # extension key: extras.deterministic = true -> every gradient sum in a fixed order (include/astk.h `deterministic`; a few per cent slower)
        self.model.deterministic = bool(self.cfg.train.get("extras", {}).get("deterministic", False))
        self.init_optimizer(self.cfg.train["optimizer"])
        if self.cfg.train.get("save_optimizer", False) and self.loaded_from and self.model.arena is not None:
            # extension key: checkpoints also carry the Adam moments, so a resumed run continues instead of re-warming them
            if serializers.load_optimizer(self.loaded_from, self.model, self.optimizer):
                print("optimizer state restored (step {0:d})".format(self.optimizer.t))
        self.train_log = os.path.join(self.model_dir, "train.log")
        self.dev_log = os.path.join(self.model_dir, "dev.log")

    def init_optimizer(self, opt_cfg):
        print("Setting up optimizer")
        if opt_cfg["type"] == _ADAM:
            print("using ADAM")
            self.optimizer = optimizers.Adam(alpha=opt_cfg["lr"], beta1=0.9, beta2=0.999, eps=1e-08, amsgrad=True)
        else:
            print("using SGD")
            self.optimizer = optimizers.SGD(lr=opt_cfg["lr"])
        print("learning rate: {0:f}".format(opt_cfg["lr"]))
        self.optimizer.setup(self.model)
        if opt_cfg["l2"] > 0:
            print("Adding WeightDecay: {0:f}".format(opt_cfg["l2"]))
            self.optimizer.add_hook(optimizers.WeightDecay(opt_cfg["l2"]))
        print("Clipping gradients at: {0:d}".format(opt_cfg["grad_clip"]))
        self.optimizer.add_hook(optimizers.GradientClipping(threshold=opt_cfg["grad_clip"]))
        if opt_cfg["grad_noise_eta"] > 0:
            print("Adding gradient noise: {0:f}".format(opt_cfg["grad_noise_eta"]))
            self.optimizer.add_hook(optimizers.GradientNoise(eta=opt_cfg["grad_noise_eta"]))
        links = {n.split("/")[0] for n in (self.model.arena.shapes if self.model.arena is not None else [])}
        for l in opt_cfg["freeze"]:
            if not links or l in links:
                print("freezing: {0:s}".format(l))
                self.model[l].disable_update()
            else:
                print("layer {0:s} not in model".format(l))
        if adist.is_distributed():
            # replicas draw different dropout masks / speech noise for their different rows (the teacher-forcing stream stays common)
            self.model.rng_seed = (self.model.rng_seed + 0x9E3779B97F4A7C15 * adist.rank()) & 0xFFFFFFFFFFFFFFFF
            if self.model.arena is not None:
                self.model.grad_buckets = adist.make_grad_buckets(self.model)
                self.optimizer.grad_sync = self.model.grad_buckets.finish
            else:      # parameters materialise lazily on the first batch: fall back to one all-reduce of the whole arena
                self.optimizer.grad_sync = adist.allreduce_grads
            if self.cfg.train.get("sync_bn", False):    # extension key: BatchNorm statistics over the global batch
                self.model.stat_exchange = adist.StatExchange()

    def get_model(self):
        self.model_fname = os.path.join(self.model_dir, "seq2seq.model")
        self.model = SpeechEncoderDecoder(self.gpuid, self.cfg.model)
        self.model.to_gpu(self.gpuid)
        feat_dim = self.cfg.train["data"].get("feat_dim")
        if feat_dim:
            self.model.materialize(int(feat_dim), seed=0)     # same seed on every rank: replicas start identical
        self.max_epoch = 0
        self.loaded_from = None
        print("Checking for model in: {0:s}".format(self.model_dir))
        stem = os.path.basename(self.model_fname).replace(".model", "")
        files = [f for f in os.listdir(os.path.dirname(self.model_fname)) if stem in f and f.endswith(".model")]
        if files:
            newest = max(files, key=lambda s: int(s.split("_")[-1].split(".")[0]))
            path = os.path.join(os.path.dirname(self.model_fname), newest)
            print("model found = \n{0:s}".format(path))
            serializers.load_npz(path, self.model)
            self.loaded_from = path
            self.max_epoch = int(newest.split("_")[-1].split(".")[0])
        else:
            print("model not found")

    def train_epoch(self, set_key):
        total_loss, n_batches = 0.0, 0
        n_utts = self.data_loader.n_utts[set_key]
        ex = self.cfg.train["extras"]
        avg_loss = 0.0
        # nn.py:189 reads the loss back after every step (a device sync).  Here the read of step i happens after step i+1 has been
        # enqueued, so the device never waits for the host; the reported numbers are the same, the progress bar lags by one batch.
        pending = None
        ctc_sum = [0.0, 0]                     # extras.ctc_weight > 0: sum of the steps' CTC terms / batch size, rows without a path
        kw = {}
        use_mrt = self.mrt is not None and self.max_epoch + self.epochs_trained >= self.mrt["start_epoch"]
        risk_sum = [0.0, 0]                    # MRT steps: sum of the steps' mean expected costs, steps

        def settle(p):
            nonlocal total_loss, n_batches, avg_loss
            vals = p[0].tolist()                                       # [loss, status word of the persistent kernels]
            raise_if_aborted(vals[1], "NN.train_epoch")
            if len(vals) > 2:                                          # ... rows without a CTC path (int32), the attention term alone
                ctc_sum[0] += (vals[0] - vals[3]) / p[1]
                ctc_sum[1] += ctc_count_of(vals[2])
            if len(p) > 3:                                             # an MRT step: the utterances' expected costs, read with the loss
                risks = p[3].tolist()
                risk_sum[0] += sum(risks) / len(risks)
                risk_sum[1] += 1
            loss_val = vals[0] / p[1]                                  # quirk Q5: divided by the batch size
            n_batches += 1
            total_loss += loss_val
            avg_loss = total_loss / n_batches
            pbar.set_description("loss={0:0.4f}".format(avg_loss))
            pbar.update(p[2] * self.data_loader.world)
        # (a stream of its own rather than the legacy default stream: slightly faster, and what lets the model's side stream run beside the recurrences)
        if getattr(self, "_compute_stream", None) is None:
            self._compute_stream = torch.cuda.Stream(device=self.model.device)
        torch.cuda.synchronize(self.model.device)
        with tqdm(total=n_utts, ncols=80, disable=adist.rank() != 0) as pbar, torch.cuda.stream(self._compute_stream):
            for batch in self.data_loader.get_batch(self.cfg.train["batch_size"], set_key, train=True, labels=True):
                if use_mrt:
                    st = mrt.mrt_step(self.model, batch["X"], batch["y"], self.mrt, self.mrt_stream, self.optimizer)
                    self.mrt_stream = st.next_stream
                    cur = (st.loss.pair.clone(), len(st.batch["y"]), len(batch["X"]), st.risk.clone())
                    if pending is not None:
                        settle(pending)
                    pending = cur
                    continue
                if self.ctc_weight > 0:
                    kw = {"ctc_weight": self.ctc_weight, "x_lens": batch.get("x_len")}
                with using_config("train", True):
                    loss = self.model.forward_loss(X=batch["X"], y=batch["y"], teach_ratio=ex["teach_ratio"],
                                                   random_out=ex["random_out"], add_noise=ex["speech_noise"],
                                                   y_global=batch.get("y_global"), label_smoothing=self.label_smoothing, **kw)
                    self.model.cleargrads()
                    loss.backward()
                    self.optimizer.update()
                # the loss buffer is reused by the next step
                cur = ((loss.quad if loss.quad is not None else loss.pair).clone(), len(batch["y"]), len(batch["X"]))
                if pending is not None:
                    settle(pending)
                pending = cur
            if pending is not None:
                settle(pending)
        torch.cuda.synchronize(self.model.device)      # later default-stream work (predict, checkpoint) sees the epoch's updates
        self.ctc_epoch = (ctc_sum[0] / max(n_batches, 1), ctc_sum[1]) if self.ctc_weight > 0 else None
        self.mrt_epoch = risk_sum[0] / max(risk_sum[1], 1) if use_mrt else None
        self.epochs_trained += 1
        return avg_loss

    # ---- nn.py:235-322
    def init_hyp(self):
        return init_hyp(self.model)

    def decode_beam_step(self, decode_entry, beam_width):
        return decode_beam_step(self.model, decode_entry, beam_width)

    def decode_beam(self, X, stop_limit, N, K, ctc_weight=0.0):
        return decode_beam(self.model, X, stop_limit, N, K, ctc_weight)

    def decode_beam_batch(self, Xs, stop_limit, N, K, ctc_weight=0.0):
        return decode_beam_batch(self.model, Xs, stop_limit, N, K, ctc_weight)

    def decode_beam_device(self, Xs, stop_limit, N, K, ctc_weight=0.0):
        return decode_beam_device(self.model, Xs, stop_limit, N, K, ctc_weight)

    def predict(self, set_key):
        preds = []
        stop_limit = self.cfg.train["data"]["max_pred"]
        for utts, _, tokens in read_one_batch_late(self, set_key, False, lambda batch, slot: self.model.predict_async(
                batch["X"], SYMBOLS.GO_ID, SYMBOLS.EOS_ID, stop_limit, slot=slot)):
            preds.extend(zip(utts, tokens.tolist()))
        return preds

    def predict_scored(self, set_key):
        """predict() with the dev loss of the reference's older trainer and a score per hypothesis: returns (preds, dev_loss, scores).
        `preds` is what predict() returns; dev_loss = the mean over the batches of (the free-running cross-entropy summed over the decoded
        steps / the padded target length) (nmt_run.py:543, 558-560; SpeechEncoderDecoder.predict_scored); scores = (utt, log-probability of
        the hypothesis up to and including its first EOS) pairs.  Read one batch late like predict()."""
        preds, scores, losses = [], [], []
        stop_limit = self.cfg.train["data"]["max_pred"]
        for utts, L, r in read_one_batch_late(self, set_key, True, lambda batch, slot: self.model.predict_scored_async(
                batch["X"], SYMBOLS.GO_ID, SYMBOLS.EOS_ID, stop_limit, batch["y"], slot=slot)):
            preds.extend(zip(utts, r.tokens.tolist()))
            scores.extend(zip(utts, r.score.tolist()))
            losses.append(r.loss / L)
        return preds, (sum(losses) / len(losses) if losses else 0.0), scores

    def sample_set(self, set_key, n, seed, temperature=1.0, utts_per_call=1, top_k=None, top_p=1.0):
        """n samples of every utterance of a set (sample_hypotheses; utterance k of the set, in the loader's order, draws from the
        streams k * n .. k * n + n - 1 of `seed`): returns {utt: [(hyp, score, [])]}, the n-best format of beam.py's pickle without
        attention histories.  utts_per_call = U > 1 packs the rows of up to U utterances into one call (sample_hypotheses_packed):
        the same streams, so the same samples.  top_k / top_p: truncated sampling (SpeechEncoderDecoder.sample)."""
        out = {}
        stop_limit = self.cfg.train["data"]["max_pred"]
        with tqdm(total=self.data_loader.n_utts[set_key], ncols=80, disable=adist.rank() != 0) as pbar:
            if utts_per_call > 1:
                group, k0 = [], 0
                for utt in itertools.chain(self.data_loader.get_batch(1, set_key, train=False, labels=False), [None]):
                    if utt is not None:
                        group.append(utt)
                    if group and (utt is None or len(group) == utts_per_call):
                        with using_config("train", False):
                            lists = sample_hypotheses_packed(self.model, [g["X"] for g in group], n, stop_limit, seed, temperature,
                                                             first_streams=[(k0 + i) * n for i in range(len(group))], max_utts=utts_per_call,
                                                             top_k=top_k, top_p=top_p)
                        for g, hyps in zip(group, lists):
                            out[g["utts"][0]] = [(h["hyp"], h["score"], []) for h in hyps]
                        pbar.update(len(group))
                        k0 += len(group)
                        group = []
                return out
            for k, utt in enumerate(self.data_loader.get_batch(1, set_key, train=False, labels=False)):
                with using_config("train", False):
                    hyps = sample_hypotheses(self.model, utt["X"], n, stop_limit, seed, temperature, first_stream=k * n, top_k=top_k, top_p=top_p)
                out[utt["utts"][0]] = [(h["hyp"], h["score"], []) for h in hyps]
                pbar.update(1)
        return out

    def score_set(self, set_key):
        """Forced decoding of a set's references (SpeechEncoderDecoder.score): returns (scores, dev_loss, ppl).  scores = (utt,
        log-probability of the reference, its number of non-PAD target tokens) triples; dev_loss = the mean over the batches of (the
        teacher-forced cross-entropy summed over the steps / the padded target length) -- the normalisation of predict_scored's dev loss,
        so the two are comparable; ppl = exp(-sum of the log-probabilities / sum of the token counts).  Read one batch late like predict()."""
        scores, losses = [], []
        for utts, L, r in read_one_batch_late(self, set_key, True, lambda batch, slot: self.model.score_async(batch["X"], batch["y"], slot=slot)):
            scores.extend(zip(utts, r.score.tolist(), r.n_tokens.tolist()))
            losses.append(r.loss / L)
        n_tok = sum(n for _, _, n in scores)
        ppl = math.exp(-sum(lp for _, lp, _ in scores) / n_tok) if n_tok else float("nan")
        return scores, (sum(losses) / len(losses) if losses else 0.0), ppl

    def ctc_align_set(self, set_key):
        """Forced alignment of a set's references through the CTC head (SpeechEncoderDecoder.ctc_align), batch by
        batch: {utt: the row's dict}.  The rows' true frame counts are batch["x_len"] where the loader's batches carry it, the loader's
        own record of the utterances' lengths otherwise (evaluation batches have the keys they always had)."""
        out = {}
        for batch in self.data_loader.get_batch(self.cfg.train["batch_size"], set_key, train=False, labels=True):
            x_len = batch.get("x_len")
            if x_len is None:
                x_len = self.data_loader.frame_counts(set_key, batch["utts"])
            for u, row in zip(batch["utts"], self.model.ctc_align(batch["X"], batch["y"], x_lens=x_len)):
                out[u] = row
        return out

    def ctc_beam_set(self, set_key, N, C):
        """CTC prefix beam search of a set through the head alone (SpeechEncoderDecoder.ctc_beam), batch by
        batch with the rows' true frame counts as ctc_align_set takes them: {utt: [(hyp, score, [])]}, the n-best format of beam.py's
        pickle without attention histories (hyp = [GO] + labels + [EOS], score = the pruned CTC sum)."""
        out = {}
        for batch in self.data_loader.get_batch(self.cfg.train["batch_size"], set_key, train=False, labels=True):
            x_len = batch.get("x_len")
            if x_len is None:
                x_len = self.data_loader.frame_counts(set_key, batch["utts"])
            for u, row in zip(batch["utts"], self.model.ctc_beam(batch["X"], x_lens=x_len, N=N, C=C)):
                out[u] = [(h["hyp"], h["score"], []) for h in row]
        return out


def rescore_ctc_nbest(model, Xs, nbest, weight, max_utts=None):
    """The second pass over CTC n-best lists (SpeechEncoderDecoder.ctc_beam): Xs a list of (1, T_u, D) inputs, nbest[u] the list of
    utterance u's entries ({"hyp", "score", ..}).  The attention decoder scores every hypothesis (score_hypotheses_packed: calls of up
    to 32 rows, at most max_utts utterances each); returns per utterance the entries ranked by (1 - weight) * att + weight * ctc
    (equal scores keep the first pass's order), each a copy with "score" = that sum and "att_score", "ctc_score" beside it, the keys
    joint_entry_scores reads."""
    w = float(weight)
    if not 0.0 <= w <= 1.0:
        raise ValueError(f"rescore_ctc_nbest: weight must lie in [0, 1] (the terms weigh 1 - w and w), got {weight!r}")
    if len(Xs) != len(nbest):
        raise ValueError(f"rescore_ctc_nbest: {len(Xs)} inputs for {len(nbest)} n-best lists")
    with using_config("train", False):
        res = score_hypotheses_packed(model, Xs, [[list(e["hyp"]) for e in lst] for lst in nbest], max_utts=max_utts)
    out = []
    for lst, (att, _) in zip(nbest, res):
        new = [dict(e, score=(1.0 - w) * a + w * float(e["score"]), att_score=a, ctc_score=float(e["score"])) for e, a in zip(lst, att)]
        out.append(sorted(new, key=lambda e: -e["score"]))
    return out


# score.py's CTC alignment option lives here, with the alignment it writes: the command line itself stays the forced decoder's.
ALIGNMENT_KEYS = ("segments", "segments_input", "labels", "confidence", "score", "total_logp")


def add_alignment_arguments(parser):
    parser.add_argument("--ctc-alignments", dest="ctc_alignments", metavar="OUT.npz",
                        help="write the CTC head's forced alignments (Viterbi segments per token, confidences, best-path and full-sum "
                             "scores) of the references, or with --nbest of every hypothesis, to this .npz (needs rnn_config.ctc)")


def ctc_alignment_arrays(name, row):
    """The .npz entries of one aligned row: name/segments (U, 2) encoder frames, name/segments_input (U, 2) input frames, name/labels
    (U,), name/confidence (U,), name/score, name/total_logp."""
    import numpy as np
    return {"{0:s}/{1:s}".format(name, k): np.asarray(row[k]) for k in ALIGNMENT_KEYS}


def write_alignment_file(nn, set_key, args, beam=None):
    """score.py --ctc-alignments: nothing without the flag; the references of the set (NN.ctc_align_set), or with a beam.py pickle its
    hypotheses, one utterance per call with X repeated over them and the hypotheses PAD-padded (key utt#rank)."""
    import numpy as np
    path = args.get("ctc_alignments")
    if not path:
        return None
    arrays = {}
    if beam is None:
        for u, row in nn.ctc_align_set(set_key).items():
            arrays.update(ctc_alignment_arrays(u, row))
    else:
        for utt in nn.data_loader.get_batch(1, set_key, train=False, labels=False):
            u = utt["utts"][0]
            if u not in beam:
                continue
            hyps = [[int(t) for t in h[0]] for h in beam[u]]
            y = np.zeros((len(hyps), max(max(len(h) for h in hyps), 1)), np.int32)
            for k, h in enumerate(hyps):
                y[k, :len(h)] = h
            rows = nn.model.ctc_align(utt["X"].expand(len(hyps), -1, -1), y)
            for k, row in enumerate(rows):
                arrays.update(ctc_alignment_arrays("{0:s}#{1:d}".format(u, k), row))
    np.savez_compressed(path, **arrays)
    print("CTC alignments written to: {0:s} ({1:d} rows)".format(path, len(arrays) // len(ALIGNMENT_KEYS)))
    return path
