"""Shared by the CTC prefix beam search tests (tests/test_ctc_beam_host.py, tests/test_gpu_ctc_beam.py): a NumPy float64 model of
include/astk.h astk_ctc_beam with a dictionary keyed by label tuples, instrumented, and its named input cases.
Every case is a pure function of its name."""
import math

import numpy as np

PAD_ID, GO_ID, EOS_ID, UNK_ID = 0, 1, 2, 3
NEG = -math.inf


def logaddexp(a, b):
    """log(exp(a) + exp(b)) in float64, symmetric in its arguments; -inf for two -inf terms."""
    m = max(a, b)
    if m == NEG:
        return NEG
    return m + math.log1p(math.exp(min(a, b) - m))


def log_softmax_rows(x):
    """float64 log-softmax of (n, V) logits: the log-sum-exp over all V classes with the maximum subtracted."""
    x = np.asarray(x, np.float64)
    if not len(x):
        return x
    mx = x.max(axis=1, keepdims=True)
    return x - (np.log(np.exp(x - mx).sum(axis=1, keepdims=True)) + mx)


def proposals(xt, C, first_label):
    """The C labels c >= first_label with the largest xt[c]: higher value first, equal values lower id first."""
    ids = np.arange(first_label, len(xt))
    order = np.lexsort((ids, -xt[first_label:]))
    return [int(ids[i]) for i in order[:C]]


def search_row(x, N, C, max_labels, first_label=UNK_ID, blank=PAD_ID):
    """One row: x (n, V) logits of the valid frames.  Returns (beam, stats): beam = [(labels tuple, score, p_b, p_nb)] in rank order;
    stats = dict(min_gap: the smallest non-zero gap between candidates adjacent in rank at or above the cut, merges, reentries: prefixes
    kept that were kept before and then dropped, reentry_live_descendant: one of them while a descendant was in the beam, cut_ties:
    frames with an exact tie across the cut, stay_outside: stay candidates whose last label was not among the frame's proposals, max_len)."""
    lx = log_softmax_rows(x)
    beam = [((), 0.0, NEG)]                                # (prefix, p_b, p_nb), rank order
    ever, dropped = {()}, set()
    st = dict(min_gap=math.inf, merges=0, reentries=0, reentry_live_descendant=False, cut_ties=0, stay_outside=0, max_len=0)
    for t in range(len(lx)):
        xt = lx[t]
        props = proposals(xt, C, first_label)
        slot_of = {l: j for j, (l, _, _) in enumerate(beam)}
        stay = []
        for l, pb, pnb in beam:
            tot = logaddexp(pb, pnb)
            stay.append([tot + xt[blank], pnb + xt[l[-1]] if l else NEG])
            st["stay_outside"] += 1 if l and l[-1] not in props else 0
        ext = []                                             # (slot, proposal rank, p_nb')
        for j, (l, pb, pnb) in enumerate(beam):
            if len(l) >= max_labels:
                continue
            tot = logaddexp(pb, pnb)
            for k, c in enumerate(props):
                p = (pb if l and c == l[-1] else tot) + xt[c]
                other = slot_of.get(l + (c,))
                if other is not None:                        # the same string as a member of the beam: into its stay candidate
                    stay[other][1] = logaddexp(stay[other][1], p)
                    st["merges"] += 1
                else:
                    ext.append((j, k, p))
        cands = [(logaddexp(pb, pnb), 0, j, 0, beam[j][0], pb, pnb) for j, (pb, pnb) in enumerate(stay)]
        cands += [(p, 1, j, k, beam[j][0] + (props[k],), NEG, p) for j, k, p in ext]
        cands = [c for c in cands if c[0] > NEG]
        cands.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
        _note_gaps(st, [c[0] for c in cands], N)
        kept = cands[:N]
        new = {c[4] for c in kept}
        for l in new:
            if l in dropped:
                st["reentries"] += 1
                if any(len(o) > len(l) and o[:len(l)] == l for o, _, _ in beam):
                    st["reentry_live_descendant"] = True
                dropped.discard(l)
        dropped |= {l for l, _, _ in beam if l not in new}
        ever |= new
        beam = [(c[4], c[5], c[6]) for c in kept]
        st["max_len"] = max([st["max_len"]] + [len(l) for l in new])
    return [(l, logaddexp(pb, pnb), pb, pnb) for l, pb, pnb in beam], st


def _note_gaps(st, scores, N):
    """Gaps between candidates adjacent in rank at or above the cut (the last kept one and the first dropped one included)."""
    top = scores[:N + 1]
    for a, b in zip(top[:-1], top[1:]):
        if a != b:
            st["min_gap"] = min(st["min_gap"], a - b)
    if len(scores) > N and scores[N - 1] == scores[N]:
        st["cut_ties"] += 1


def search(logits, input_len, N, C, max_labels, first_label=UNK_ID, blank=PAD_ID):
    """The contract of astk_ctc_beam on host arrays: dict(tokens (B, N, max_labels) int32, n_labels (B, N) int32, score (B, N) float64,
    stats: one dict per row)."""
    B, T, _ = logits.shape
    tokens = np.full((B, N, max_labels), blank, np.int32)
    n_labels = np.full((B, N), -1, np.int32)
    score = np.full((B, N), NEG, np.float64)
    stats = []
    for b in range(B):
        n = T if input_len is None else int(np.clip(input_len[b], 0, T))
        beam, st = search_row(logits[b, :n], N, C, max_labels, first_label, blank)
        for r, (l, s, _, _) in enumerate(beam):
            tokens[b, r, :len(l)] = l
            n_labels[b, r] = len(l)
            score[b, r] = s
        stats.append(st)
    return dict(tokens=tokens, n_labels=n_labels, score=score, stats=stats)


# ---- the named cases: name -> dict(logits (B, T, V) float32, lens or None, N, C, max_labels, ldv or None)
def _normal(seed, B, T, V):
    return np.random.default_rng(seed).standard_normal((B, T, V)).astype(np.float32)


def _ragged(T, B):
    """B row lengths that include 0, 1 and T."""
    base = [T, 0, 1, max(T - 3, 1), T // 2 + 1, T]
    return np.asarray((base * ((B + len(base) - 1) // len(base)))[:B], np.int32)


def _peaked(seed, B, T, V, label_of_frame):
    x = _normal(seed, B, T, V)
    for t in range(T):
        x[:, t, label_of_frame(t)] += 9.0
    return x


def _twin(seed, B, T, V):
    x = _normal(seed, B, T, V)
    x[:, :, 4] = x[:, :, 3]                                  # two label columns bit-identical in every frame
    return x


CASES = {
    "random": lambda: dict(logits=_normal(101, 4, 40, 12), lens=_ragged(40, 4), N=4, C=4, max_labels=40),
    "random-2": lambda: dict(logits=_normal(102, 3, 40, 12), lens=None, N=4, C=4, max_labels=40),
    "blank-biased": lambda: dict(logits=_normal(103, 4, 40, 12) + np.eye(12, dtype=np.float32)[0] * 3, lens=_ragged(40, 4), N=4, C=4,
                                 max_labels=40),
    "small-v": lambda: dict(logits=_normal(104, 4, 24, 6), lens=_ragged(24, 4), N=16, C=3, max_labels=24),
    "small-v-2": lambda: dict(logits=_normal(105, 3, 24, 6), lens=None, N=16, C=3, max_labels=24),
    "offset+": lambda: dict(logits=_normal(106, 3, 40, 12) + 30, lens=np.asarray([40, 17, 0], np.int32), N=4, C=4, max_labels=40),
    "offset-": lambda: dict(logits=_normal(107, 3, 40, 12) - 30, lens=np.asarray([1, 40, 33], np.int32), N=4, C=4, max_labels=40),
    "cap": lambda: dict(logits=_normal(108, 4, 24, 8) - np.eye(8, dtype=np.float32)[0] * 2, lens=_ragged(24, 4), N=6, C=4, max_labels=3),
    "c-lt-stay": lambda: dict(logits=_peaked(109, 3, 30, 9, lambda t: (0, 5, 0, 7, 7, 0, 4)[t % 7]), lens=np.asarray([30, 22, 1], np.int32),
                              N=5, C=1, max_labels=30),
    "ldv": lambda: dict(logits=_normal(110, 3, 8, 1098), lens=np.asarray([8, 5, 0], np.int32), N=5, C=5, max_labels=8, ldv=1100),
    "long": lambda: dict(logits=_normal(111, 3, 300, 40) + np.eye(40, dtype=np.float32)[0] * 2, lens=np.asarray([300, 257, 1], np.int32), N=16,
                         C=16, max_labels=255),
    "twin-columns": lambda: dict(logits=_twin(112, 3, 20, 7), lens=np.asarray([20, 13, 2], np.int32), N=4, C=4, max_labels=20),
    "twin-columns-odd": lambda: dict(logits=_twin(113, 2, 16, 8), lens=None, N=5, C=3, max_labels=16),
}
ALL_CASES = list(CASES)

_RESULT = {}


def case(name):
    return CASES[name]()


def result(name):
    """(case dict, the model's result), computed once and shared; callers leave both unchanged."""
    if name not in _RESULT:
        c = case(name)
        _RESULT[name] = (c, search(c["logits"], c["lens"], c["N"], c["C"], c["max_labels"]))
    return _RESULT[name]


# ---- references for the exhaustive checks
def collapse(path, blank=PAD_ID):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return tuple(out)


def brute_force(x, first_label=UNK_ID, blank=PAD_ID):
    """{labels tuple: log p_ctc} of one row by enumeration of all alignments over the blank and the classes >= first_label."""
    import itertools
    lx = log_softmax_rows(x)
    classes = [blank] + list(range(first_label, lx.shape[1]))
    acc = {}
    for path in itertools.product(classes, repeat=len(lx)):
        lp = float(sum(lx[t, c] for t, c in enumerate(path)))
        key = collapse(path, blank)
        acc[key] = logaddexp(acc.get(key, NEG), lp)
    return acc
