"""Shared by the risk-weight tests (tests/test_risk_host.py, tests/test_gpu_risk.py): the named cases of astk_risk_weights (include/astk.h,
DESIGN.md section 37), a direct float64 evaluation of its definition written apart from ast_amd.mrt.risk_weights_host, and the bound
both sides are compared under.  A case holds host arrays: first (U+1), score (R), stats (R, 8), lens, pairs (R, 2), flags (R) and the
three scalars alpha, risk_scale, ref_weight."""
import numpy as np

from ast_amd.eval import pair_stats_host

LIVE, REFERENCE = 1, 2
COSTS = ("bleu", "edit")


def _strings(rng, sizes, empty_hyp=None, disjoint=None):
    """A pool for lists of the given sizes: per list a reference of 4..11 tokens and candidates that are edits of it; then the references.
    Returns (pool, pairs, first)."""
    hyps, refs, pairs, first = [], [], [], [0]
    for u, n in enumerate(sizes):
        ref = rng.integers(4, 14, rng.integers(4, 12)).tolist()
        refs.append(ref)
        for k in range(n):
            h = list(ref)
            for _ in range(int(rng.integers(0, 4))):
                op, at = rng.integers(0, 3), int(rng.integers(0, max(1, len(h))))
                if op == 0 and h:
                    h[at] = int(rng.integers(4, 14))
                elif op == 1 and len(h) > 1:
                    del h[at]
                else:
                    h.insert(at, int(rng.integers(4, 14)))
            hyps.append(h)
        first.append(len(hyps))
    if empty_hyp is not None:
        hyps[empty_hyp] = []
    if disjoint is not None:
        hyps[disjoint] = [100, 101, 102, 103, 104]          # shares no token with any reference: m1 = 0
    R = len(hyps)
    u_of = np.repeat(np.arange(len(sizes)), sizes)
    pairs = [(i, R + int(u_of[i])) for i in range(R)]
    return hyps + refs, pairs, first


def make_case(sizes, seed=0, alpha=1.0, risk_scale=1.0, ref_weight=0.0, scores=None, dead=(), ref_rows=(), bad_stats=(), empty_hyp=None,
              disjoint=None):
    rng = np.random.default_rng(seed)
    pool, pairs, first = _strings(rng, sizes, empty_hyp, disjoint)
    R = first[-1]
    stats = np.asarray(pair_stats_host(pool, pairs), np.int32).reshape(R, 8)
    pairs = np.asarray(pairs, np.int32)
    for i in bad_stats:                                      # the bad row of astk_pair_stats: eight -1, its pair names no string
        stats[i] = -1
        pairs[i] = (10**6, -5)
    flags = np.full(R, LIVE, np.int32)
    for i in dead:
        flags[i] = 0
    for i in ref_rows:
        flags[i] = REFERENCE
    score = (-rng.random(R) * 6).astype(np.float32) if scores is None else np.asarray(scores, np.float32)
    assert len(score) == R
    return dict(first=np.asarray(first, np.int32), score=score, stats=stats, lens=np.asarray([len(s) for s in pool], np.int32), pairs=pairs,
                flags=flags, alpha=alpha, risk_scale=risk_scale, ref_weight=ref_weight)


def cases():
    """name -> case.  Every case of the issue's list."""
    c = {}
    c["one"] = make_case([1], seed=1, alpha=2.0, risk_scale=3.0)
    c["two"] = make_case([2], seed=2, alpha=0.5, risk_scale=2.0, ref_weight=0.25, ref_rows=())
    c["full64"] = make_case([64], seed=3, alpha=0.3, risk_scale=65.0, ref_weight=0.5, ref_rows=(63,))
    sizes = [1, 2, 3, 4, 5, 6, 7]
    c["ragged"] = make_case(sizes, seed=4, alpha=1.0, risk_scale=4.0, ref_weight=1.5, ref_rows=tuple(np.cumsum(sizes) - 1))
    c["equal_scores"] = make_case([5, 3], seed=5, alpha=1.0, risk_scale=-2.0, scores=np.full(8, -3.25))
    c["far_scores"] = make_case([4, 3], seed=6, alpha=1.0, risk_scale=2.0, scores=[-1e4, 0.0, -2e4, -1e4, -5.0, -1e4 - 5.0, -2e4])
    c["alpha0"] = make_case([4, 2], seed=7, alpha=0.0, risk_scale=5.0, ref_weight=0.75, ref_rows=(3, 5))
    c["dead_middle"] = make_case([7, 5], seed=8, alpha=0.8, risk_scale=3.0, dead=(2, 3, 9))
    c["no_live"] = make_case([3, 4, 2], seed=9, alpha=1.0, risk_scale=3.0, ref_weight=0.5, dead=(3, 4, 5), ref_rows=(6,))
    c["bad_stats"] = make_case([4, 3], seed=10, alpha=1.0, risk_scale=2.0, bad_stats=(1, 6))
    c["zero_match"] = make_case([4, 2], seed=11, alpha=1.0, risk_scale=2.0, disjoint=2)
    c["hyp_len0"] = make_case([3, 3], seed=12, alpha=1.0, risk_scale=2.0, empty_hyp=4)
    return c


def _bleu_cost(m, hyp_len, ref_len):
    """1 - sentence BLEU, written out from the definition (method-2 smoothing, one reference)."""
    if m[0] == 0:
        return 1.0
    p = [m[0] / max(1, hyp_len)] + [(m[n] + 1) / (max(1, hyp_len - n) + 1) for n in (1, 2, 3)]
    bp = 1.0 if hyp_len > ref_len else (0.0 if hyp_len == 0 else np.exp(1.0 - ref_len / hyp_len))
    return 1.0 - bp * np.exp(0.25 * np.sum(np.log(p)))


def direct(case, cost):
    """(weight, risk, cost) of the definition in float64, NOT rounded: vectorised per list, apart from risk_weights_host.  Every list of the
    named cases is a good one."""
    first, flags, stats = case["first"], case["flags"], case["stats"].astype(np.int64)
    alpha, rs, rw = (float(np.float32(case[k])) for k in ("alpha", "risk_scale", "ref_weight"))
    R = len(flags)
    weight, costs, risk = np.zeros(R), np.zeros(R), np.zeros(len(first) - 1)
    for u in range(len(first) - 1):
        idx = np.arange(first[u], first[u + 1])
        live = ((flags[idx] & LIVE) != 0) & (stats[idx, 0] >= 0)
        c = np.zeros(len(idx))
        for k, i in enumerate(idx):
            if live[k]:
                hl, rl = int(case["lens"][case["pairs"][i, 0]]), int(case["lens"][case["pairs"][i, 1]])
                c[k] = _bleu_cost(stats[i, 4:8], hl, rl) if cost == "bleu" else stats[i, 0] / max(1, rl)
        q = np.zeros(len(idx))
        if live.any():
            s = case["score"][idx].astype(np.float64)
            z = np.where(live, alpha * (s - s[live].max()), -np.inf)
            q = np.exp(z) / np.exp(z).sum()
        rbar = float((q * c).sum())
        weight[idx] = rs * alpha * q * (rbar - c) + np.where(flags[idx] & REFERENCE, rw, 0.0)
        costs[idx], risk[u] = c, rbar
    return weight, risk, costs


def bounds(case, model):
    """The bounds on |device - model| (and |host - direct|) for (weight, risk, cost): both sides compute in float64 and round once, so
    they differ by one float32 ulp of the element plus what the float64 exp / log differences leave after the cancellation in
    Rbar - c_i: 2^-23 |x_model| + 1e-12 (|risk_scale| alpha max_i c_i + |ref_weight|); for risk and cost the second term is 1e-12 max c."""
    w, risk, c = (np.abs(np.asarray(v, np.float64)) for v in model)
    cmax = float(c.max()) if len(c) else 0.0
    alpha, rs, rw = (abs(float(np.float32(case[k]))) for k in ("alpha", "risk_scale", "ref_weight"))
    u = 2.0 ** -23
    return u * w + 1e-12 * (rs * alpha * cmax + rw), u * risk + 1e-12 * cmax, u * c + 1e-12 * cmax


def host(case, cost, **k):
    from ast_amd import mrt
    return mrt.risk_weights_host(case["first"], case["score"], case["stats"], case["lens"], case["pairs"], case["flags"], cost, case["alpha"],
                                 case["risk_scale"], case["ref_weight"], **k)
