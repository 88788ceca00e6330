"""Shared by the CTC alignment tests (tests/test_ctc_align_host.py, tests/test_gpu_ctc_align.py): a NumPy model of include/astk.h
astk_ctc_align, runnable in float64 and float32, and its input cases.  Rows, labels and the operator cases are
those of tests/ctc_model.py, imported unchanged.

For a row with labels l_1 .. l_U, the extended sequence z (S' = 2U + 1 states, blanks at the even positions) and e[t][s] =
logits[t][z_s] - lse[t] over the n = input_len valid frames:

    delta[0][0] = e[0][0], delta[0][1] = e[0][1], the rest -inf
    delta[t][s] = e[t][s] + max(delta[t-1][s], delta[t-1][s-1], [skip] delta[t-1][s-2])      [skip]: z_s is a label and z_s != z_{s-2}
    tie rule: a predecessor replaces the current choice only if it is strictly greater, tried in the order s, s - 1, s - 2; the final
    state is S' - 1 unless delta[n-1][S'-2] is strictly greater.

The float32 run orders its operations the way the kernel does: e = x - lse rounded once, delta = best + e, label_logp summed in frame
order from the first frame's e; only the sum inside the log-sum-exp has another order (NumPy's pairwise sum against the kernel's
lane-strided one), which is what the operator bounds' factor 4 covers, as in section 28."""
import numpy as np

from ctc_model import OP_CASES, PAD_ID, UNK_ID, feasible, labels_of, op_case  # noqa: F401  (re-exported for the tests)


def extended(labels, blank):
    """(z (S',), skip (S',)) of a label list."""
    S = 2 * len(labels) + 1
    z = np.full(S, blank, np.int64)
    z[1::2] = labels
    skip = np.zeros(S, bool)
    skip[3::2] = z[3::2] != z[1:-2:2]
    return z, skip


def emissions(x, labels, blank, dtype=np.float64):
    """e (n, S') of one row's valid frames x (n, V): x[t][z_s] - lse[t], every operation in `dtype`."""
    x = np.asarray(x, dtype)
    z, _ = extended(labels, blank)
    m = x.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(axis=1, keepdims=True, dtype=dtype))
    return (x[:, z] - lse).astype(dtype)


def viterbi(e, skip):
    """(score, path (n,) of state indices) of the max-plus recursion over emissions e (n, S') under the tie rule; e's dtype throughout."""
    n, S = e.shape
    dtype = e.dtype.type
    ninf = dtype(-np.inf)
    if n == 0:
        return dtype(0), np.zeros(0, np.int64)

    def shifted(a, k):
        out = np.full(S, ninf, dtype)
        out[k:] = a[:S - k]
        return out
    back = np.zeros((n, S), np.int8)
    delta = np.full(S, ninf, dtype)
    delta[:2] = e[0, :2]
    for t in range(1, n):
        best, bk = delta, np.zeros(S, np.int8)
        p1, p2 = shifted(delta, 1), np.where(skip, shifted(delta, 2), ninf)
        m1 = p1 > best
        best, bk = np.where(m1, p1, best), np.where(m1, 1, bk)
        m2 = p2 > best
        best, bk = np.where(m2, p2, best), np.where(m2, 2, bk)
        delta = (best + e[t]).astype(dtype)
        back[t] = bk
    s = S - 1
    if S >= 2 and delta[S - 2] > delta[S - 1]:
        s = S - 2
    score = delta[s]
    path = np.zeros(n, np.int64)
    for t in range(n - 1, -1, -1):
        path[t] = s
        s -= int(back[t, s])
    return score, path


def rescore(e64, path):
    """The float64 log-probability of a path: the sum of its emissions."""
    return float(np.asarray(e64, np.float64)[np.arange(len(path)), path].sum())


def spans(path, U):
    """(start (U,), end (U,)): the frames [start, end) a path spends in label u's state 2u + 1."""
    start, end = np.full(U, -1, np.int64), np.full(U, -1, np.int64)
    for t, s in enumerate(path):
        if s & 1:
            u = int(s) >> 1
            if start[u] < 0:
                start[u] = t
            end[u] = t + 1
    return start, end


def label_logp(e, path, U):
    """(U,) in e's dtype: the sum of e[t][2u+1] over label u's frames, in frame order."""
    out = np.zeros(U, e.dtype)
    start, end = spans(path, U)
    for u in range(U):
        acc = e.dtype.type(0)
        for t in range(start[u], end[u]):
            acc = e.dtype.type(acc + e[t, 2 * u + 1])
        out[u] = acc
    return out


def is_valid_path(path, labels, blank):
    """A legal alignment: starts in {0, 1}, steps in {0, 1, 2 where skip allows}, ends in {S' - 2, S' - 1}."""
    z, skip = extended(labels, blank)
    S = len(z)
    if len(path) == 0:
        return S == 1
    if path[0] not in (0, 1) or path[-1] not in (S - 1, S - 2) or min(path) < 0 or max(path) >= S:
        return False
    for a, b in zip(path[:-1], path[1:]):
        d = int(b) - int(a)
        if d not in (0, 1, 2) or (d == 2 and not skip[b]):
            return False
    return True


def align(logits, y, input_len=None, first_label=UNK_ID, blank=PAD_ID, dtype=np.float64):
    """The contract of astk_ctc_align on host arrays: dict(frame_state (B, T), frame_class (B, T), label_start / label_end (B, L),
    label_logp (B, L), row_score (B), n_infeasible) and, for the tests, labels (a list per row)."""
    logits = np.asarray(logits)
    B, T, V = logits.shape
    L = y.shape[1]
    lens = np.full(B, T, np.int64) if input_len is None else np.clip(np.asarray(input_len).astype(np.int64), 0, T)
    r = dict(frame_state=np.full((B, T), -1, np.int32), frame_class=np.full((B, T), blank, np.int32),
             label_start=np.full((B, L), -1, np.int32), label_end=np.full((B, L), -1, np.int32), label_logp=np.zeros((B, L), dtype),
             row_score=np.zeros(B, dtype), n_infeasible=0, labels=[])
    for b in range(B):
        n, labels = int(lens[b]), labels_of(y[b], first_label, V)
        r["labels"].append(labels)
        if not feasible(labels, n):
            r["row_score"][b] = -np.inf
            r["n_infeasible"] += 1
            continue
        U = len(labels)
        z, skip = extended(labels, blank)
        e = emissions(logits[b, :n], labels, blank, dtype)
        r["row_score"][b], path = viterbi(e, skip)
        r["frame_state"][b, :n], r["frame_class"][b, :n] = path, z[path]
        r["label_start"][b, :U], r["label_end"][b, :U] = spans(path, U)
        r["label_logp"][b, :U] = label_logp(e, path, U)
    return r


# ------------------------------------------------------------------ cases
def _targets(rows, L, seed):
    """y (B, L) int32: every row's labels at sorted random positions, reserved ids (< UNK_ID) elsewhere -- op_case's layout."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, UNK_ID, size=(len(rows), L)).astype(np.int32)
    for b, labels in enumerate(rows):
        y[b, np.sort(rng.choice(L, size=len(labels), replace=False))] = labels
    return y


def random_valid_path(labels, n, rng, blank=PAD_ID):
    """A uniformly stepped valid alignment of `labels` over n frames: at every frame one of the allowed moves that still reaches the end."""
    z, skip = extended(labels, blank)
    S = len(z)
    rem = np.zeros(S, np.int64)                    # the least number of further frames from state s to a final state
    for s in range(S - 3, -1, -1):
        rem[s] = 1 + min(rem[s + 1], rem[s + 2] if skip[s + 2] else 1 << 30)
    path = []
    for t in range(n):
        cand = [s for s in ((0, 1) if t == 0 else (path[-1], path[-1] + 1, path[-1] + 2))
                if s < S and rem[s] <= n - 1 - t and (t == 0 or s - path[-1] < 2 or skip[s])]
        path.append(int(cand[rng.integers(len(cand))]))
    return np.asarray(path, np.int64)


PLANTED_SHAPES = [(9, 57, 3), (64, 57, 31), (64, 1098, 20), (300, 57, 255)]          # (T, V, U)
PLANTED_CASES = ["planted-t%d-v%d-u%d" % s for s in PLANTED_SHAPES]
PLANT_MARGIN = np.float32(4)


def planted_case(name):
    """(logits (2, T, V) float32, y (2, L) int32, None, paths): row 0 random labels without an adjacent repeat, row 1 with one forced; a
    random valid alignment per row whose class's logit is raised to the frame's maximum + 4 at every frame.  Any other valid path has
    another class in at least one frame (a class sequence determines its state path), loses at least 4 there and gains nowhere: the
    optimum is unique, by a margin far above the float32 rounding of a sum of T emissions, and `paths` is it."""
    T, V, U = PLANTED_SHAPES[PLANTED_CASES.index(name)]
    rng = np.random.default_rng(1000 + T + V + U)
    x = rng.standard_normal((2, T, V)).astype(np.float32)
    rows, paths = [], []
    for b in range(2):
        while True:
            labels = [int(v) for v in rng.integers(UNK_ID, V, size=U)]
            for i in range(1, U):                  # no chance repeats: row 0 has none, row 1 exactly the forced one
                while labels[i] == labels[i - 1]:
                    labels[i] = int(rng.integers(UNK_ID, V))
            if b == 1:
                labels[U // 2] = labels[U // 2 - 1]
                if U // 2 + 1 < U and labels[U // 2 + 1] == labels[U // 2]:
                    continue
            break
        assert feasible(labels, T)
        path = random_valid_path(labels, T, rng)
        z, _ = extended(labels, PAD_ID)
        cls = z[path]
        x[b, np.arange(T), cls] = x[b].max(axis=1) + PLANT_MARGIN
        rows.append(labels)
        paths.append(path)
    return x, _targets(rows, min(U + 3, 255), 2000 + T + V + U), None, paths


UNIFORM_CASES = {"uniform-t9": dict(T=9, V=11, rows=[[5, 5, 7], [], [4]], lens=[9, 9, 4], L=5),
                 "uniform-s67": dict(T=80, V=11, rows=[[UNK_ID + (i * 3) % 8 for i in range(33)], [6] * 20], lens=[80, 47], L=40)}


def earliest_path(labels, n):
    """What the tie rule leaves when every path scores the same: each label as early as possible (one blank frame in front of a
    repeated label, none otherwise), then the trailing blank -- built frame by frame, without the recursion."""
    path, s = [], 1
    for i, l in enumerate(labels):
        if i and labels[i - 1] == l:
            path.append(s - 1)
        path.append(s)
        s += 2
    assert len(path) <= n
    return np.asarray(path + [2 * len(labels)] * (n - len(path)), np.int64)


def uniform_case(name):
    """(all-zero logits, y, lens, paths): every valid path has bitwise the same score in float32 and in float64 (the same addends in the
    same order), so the tie rule alone decides."""
    c = UNIFORM_CASES[name]
    x = np.zeros((len(c["rows"]), c["T"], c["V"]), np.float32)
    lens = np.asarray(c["lens"], np.int32)
    return x, _targets(c["rows"], c["L"], len(name)), lens, [earliest_path(r, int(n)) for r, n in zip(c["rows"], lens)]


def family(name):
    return OP_CASES[name]["family"] if name in OP_CASES else name.split("-")[0]


def case(name):
    """(logits, y, lens) of any case by name."""
    if name in OP_CASES:
        return op_case(name)
    return (planted_case(name) if name in PLANTED_CASES else uniform_case(name))[:3]


ALL_CASES = list(OP_CASES) + PLANTED_CASES + list(UNIFORM_CASES)

# This model run in float32 against its float64 run, worst over the cases of a family; measured on the CPU and held by
# tests/test_ctc_align_host.py::test_float32_model_figures_are_what_the_bounds_were_taken_from.
#   F32_SCORE_RERR  |row_score32 - row_score64| / |row_score64|
#   F32_DEFICIT     the float64 optimum - the float64 rescoring of the float32 run's path (0: the float32 run found an optimal path)
#                   with both sums taken by rescore(), so that equal paths give exactly 0
# The operator's bounds are 4 x these figures (tests/test_gpu_ctc_align.py); the factor covers another summation order in the lse.
# The score figures are a few float32 ulps of the score (|score| up to 66 in `short`, 42 in `offset`, 268 in `peaked`, 478 in `long`,
# 1159 in `s511`, 53 in `planted`, 192 in `uniform`); the deficits are 0 in every family -- on these cases the float32 run finds the float64 optimum, the gap to the runner-up
# being far above the rounding -- so the operator, too, is held to an optimal path, though not to the same one where two are optimal.
# A label's label_logp is a part of its row's sum with the same addends' errors: it is held to the row's ABSOLUTE score bound,
# 4 x F32_SCORE_RERR x |row_score| (measured here: the float32 run's labels stay within 0.5 x F32_SCORE_RERR x |row_score|).
F32_SCORE_RERR = {"short": 1.5e-7, "offset": 3.1e-7, "peaked": 4.4e-8, "long": 1.4e-7, "s511": 3.4e-7, "planted": 7.1e-7, "uniform": 8.9e-7}
F32_DEFICIT = {"short": 0.0, "offset": 0.0, "peaked": 0.0, "long": 0.0, "s511": 0.0, "planted": 0.0, "uniform": 0.0}
