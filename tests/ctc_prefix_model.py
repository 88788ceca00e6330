"""Shared by the CTC prefix-score tests (tests/test_ctc_prefix_host.py, tests/test_gpu_ctc_prefix.py): a NumPy float64 model of the
prefix scorer of include/astk.h "joint CTC-attention beam search" (DESIGN.md section 30), of one joint selection step, and a host joint
beam search that takes the per-step attention log-probabilities from a callback.

x (T, V) is the float64 log_softmax of one utterance's logits.  A prefix g of n labels with last label `last` has the state r (T, 2):
r[t][0] / r[t][1] = log-probability of all alignments of g over frames 0..t that end in a non-blank / a blank, and psi(g) = the
log-probability of all label strings that start with g.  Every logaddexp of dead terms is -inf, never NaN."""
import numpy as np

PAD_ID, GO_ID, EOS_ID, UNK_ID = 0, 1, 2, 3
NINF = -np.inf


def log_softmax64(logits):
    x = np.asarray(logits, np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def lae(a, b):
    with np.errstate(invalid="ignore"):
        return np.logaddexp(a, b)


def empty_state(x, blank=PAD_ID):
    r = np.full((x.shape[0], 2), NINF)
    r[:, 1] = np.cumsum(x[:, blank])
    return r


def extend(x, r, n, last, c, blank=PAD_ID, first_label=UNK_ID, eos=EOS_ID):
    """(psi(g.c), the state of g.c, its label count) from the state r of g (n labels, the last one `last`).  eos: the probability that
    the utterance is exactly g, the state and the count stay g's; an id that is no label: -inf and a dead state."""
    T = x.shape[0]
    if c == eos:
        return float(lae(r[T - 1, 0], r[T - 1, 1])), r, n
    out = np.full((T, 2), NINF)
    m = max(n, 1)
    if c < first_label or c == blank or m > T:
        return NINF, out, n + 1
    phi = r[:, 1] if (n > 0 and c == last) else lae(r[:, 0], r[:, 1])
    if n == 0:
        out[0, 0] = x[0, c]
    psi = out[m - 1, 0]
    for t in range(m, T):
        out[t, 0] = lae(out[t - 1, 0], phi[t - 1]) + x[t, c]
        out[t, 1] = lae(out[t - 1, 0], out[t - 1, 1]) + x[t, blank]
        psi = lae(psi, phi[t - 1] + x[t, c])
    return float(psi), out, n + 1


def prefix_state(x, labels, blank=PAD_ID, first_label=UNK_ID):
    """(psi, state) of the prefix `labels` from the empty one (no eos among them)."""
    r, psi, last = empty_state(x, blank), 0.0, -1
    for n, c in enumerate(labels):
        psi, r, _ = extend(x, r, n, last, c, blank, first_label, eos=-1)
        last = c
    return psi, r


def joint_score(w, att, psi):
    """(1 - w) * att + w * psi from the two absolute terms; a dead CTC term and NaN rank as -inf."""
    if psi == NINF:
        return NINF
    with np.errstate(invalid="ignore"):
        s = (1.0 - w) * att + w * psi
    return NINF if np.isnan(s) else float(s)


def np_select_ctc(logits, x_of_row, slots, N, K, w, eos=EOS_ID, keep=None):
    """One joint step on host arrays.  logits (R, V) float32: the decoder's; x_of_row[r] (T_u, V): the utterance's CTC log-probabilities;
    slots[r] = dict(status 0 / 1 / 2, token, score, att, psi, n, state).  Returns per new slot dict(parent, token, carried, status,
    score, att, psi, n, state) -- status 0: an empty slot -- in the candidate order of the plain step, stable top-N (keep: top-`keep`
    instead, to look at every candidate)."""
    keep = keep or N
    R, V = logits.shape
    out = []
    for u in range(R // N):
        cands = []
        for j in range(N):
            s = slots[u * N + j]
            if s["status"] == 0:
                continue
            if s["status"] == 2:
                cands.append(dict(parent=j, token=s["token"], carried=1, status=2, score=s["score"], att=s["att"], psi=s["psi"], n=s["n"],
                                  state=s["state"]))
                continue
            lp = log_softmax64(logits[u * N + j])
            order = np.lexsort((np.arange(V), -lp))[:K]          # higher logp first, equal ones lower token id first
            last = s["token"] if s["n"] > 0 else -1
            for c in order:
                psi, st, n2 = extend(x_of_row[u * N + j], s["state"], s["n"], last, int(c), eos=eos)
                att = s["att"] + float(lp[c])
                cands.append(dict(parent=j, token=int(c), carried=0, status=2 if c == eos else 1, score=joint_score(w, att, psi), att=att,
                                  psi=psi, n=n2, state=st))
        best = sorted(cands, key=lambda t: -t["score"])[:keep]   # stable: equal scores keep the earlier candidate
        out += best + [dict(parent=-1, token=0, carried=0, status=0, score=0.0, att=0.0, psi=0.0, n=0, state=None)] * (keep - len(best))
    return out


def joint_beam_search(x, propose, first, stop_limit, N, w, eos=EOS_ID):
    """The host joint search of one utterance.  propose(ctx) -> [(token, logp, new ctx)], the K proposals of a live hypothesis in
    candidate order; first = the ctx of [GO].  Returns the kept hypotheses, best first: dict(hyp, score, att, psi, ctx)."""
    n_best = [dict(hyp=[GO_ID], score=0.0, att=0.0, psi=0.0, n=0, state=empty_state(x), ctx=first)]
    for _ in range(stop_limit):
        if all(e["hyp"][-1] == eos for e in n_best):
            break
        cur = []
        for e in n_best:
            if e["hyp"][-1] == eos:
                cur.append(e)
                continue
            last = e["hyp"][-1] if e["n"] > 0 else -1
            for tok, logp, ctx in propose(e["ctx"]):
                psi, st, n2 = extend(x, e["state"], e["n"], last, int(tok), eos=eos)
                att = e["att"] + float(logp)
                cur.append(dict(hyp=e["hyp"] + [int(tok)], score=joint_score(w, att, psi), att=att, psi=psi, n=n2, state=st, ctx=ctx))
        n_best = sorted(cur, key=lambda t: -t["score"])[:N]
    return n_best


def tight(scores, eps=1e-5):
    """Two of the kept scores lie within eps: the order of the hypotheses may depend on float32 noise of the decoder."""
    s = [v for v in scores if np.isfinite(v)]
    return any(abs(s[i] - s[j]) <= eps for i in range(len(s)) for j in range(i))
