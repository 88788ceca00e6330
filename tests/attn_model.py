"""Model of the attention scan (ast_amd/csrc/attn.hip) for tests/test_attn_host.py and tests/test_gpu_attn.py -- pure NumPy, no GPU.

  split_for / workspace_bytes / counters_offset / nch   the launch plan, RESTATED from attn.hip (split_for, attn_ws_bytes, attn_counters,
                                                        cdiv(H, 256)); the GPU test holds astk_attn_workspace_bytes against
                                                        workspace_bytes byte for byte, so a retune of either side shows.
  reference / reference_bwd                             float64, by the defining formulas.
  kernel_model / kernel_model_bwd                       float32 in the kernel's order of operations: per-wave online softmax over rows
                                                        t0 + wave, +8 with the t + 4 pair, the four-wave merge with the -inf -> weight 0
                                                        guard, the per-split partials, the merge over nsplit.  `mistake=` plants a defect.
  CASES / ROWS_CASES                                    the tables the GPU test runs; `reaches` names the branches an entry is there for,
                                                        branches() works them out from the plan (test_attn_host.py holds one to the other).

Bounds (the operator test's: tests/test_gpu_ops.py test_attention_step): max |got - ref| <= rtol * max |ref| with rtol 2e-4 for alpha and
cv, 5e-4 for ds and dq."""
from dataclasses import dataclass

import numpy as np

PART_PAD = 4
MAX_SPLIT = 128
RTOL = {"alpha": 2e-4, "cv": 2e-4, "ds": 5e-4, "dq": 5e-4}
MISTAKES = ("nch4", "empty_weight_1", "empty_guard_dropped", "lone_row_pair")


def cdiv(a, b):
    return -(-a // b)


def align_up(n, a):
    return cdiv(n, a) * a


# ------------------------------------------------------------------ the plan, as attn.hip has it
def _split(B, T):
    want = max(cdiv(512, B), 1)               # ~2 workgroups per CU
    chunk = max(cdiv(T, want), 8)             # at least 2 rows per wave
    chunk = min(chunk, T)
    clamped = cdiv(T, chunk) > MAX_SPLIT
    if clamped:
        chunk = cdiv(T, MAX_SPLIT)
    return cdiv(T, chunk), chunk, clamped


def split_for(B, T):
    """-> (nsplit, chunk)"""
    return _split(B, T)[:2]


def counters_offset(B, T, H):
    """byte offset of the B ticket counters (uint32) in the workspace: behind the partial rows of H + 4 floats."""
    return align_up(B * split_for(B, T)[0] * (H + PART_PAD) * 4, 256)


def workspace_bytes(B, T, H):
    return counters_offset(B, T, H) + align_up(B * 4, 256)


def nch(H):
    """the instantiation attn_fwd_impl / attn_bwd_launch pick: float4 chunks of 256 columns per lane."""
    c = cdiv(H, 256)
    return 1 if c <= 1 else 2 if c <= 2 else 4 if c <= 4 else 8


def padded(T):
    return (T + 3) // 4 * 4


def clamp_len(row_len, T):
    return np.minimum(np.maximum(np.asarray(row_len, np.int64), 1), T)


def branches(B, T, H, row_len=None):
    """the set of branch names the launch (B, T, H) reaches, from the plan alone."""
    nsplit, chunk, clamped = _split(B, T)
    last = T - (nsplit - 1) * chunk
    out = {f"nch{nch(H)}", f"B{B}"}
    if H % 256:
        out.add("ragged_chunk")                          # the last 256-column chunk is partly out of H
    if H % 256 == 4:
        out.add("one_lane_chunk")
    if nsplit == 1:
        out.add("nsplit1")
    if nsplit == MAX_SPLIT:
        out.add("nsplit128")
    if clamped:
        out.add("clamp")
    if nsplit > 1 and last == 1:
        out.add("last_chunk_1")
    if nsplit > 1 and last == 2:
        out.add("last_chunk_2")
    lens = {chunk, last}
    if any(n < 4 for n in lens):
        out.add("empty_wave")                            # a wave of a workgroup holds no row
    if any(n % 8 for n in lens):
        out.add("lone_row")                              # a wave's last step has no t + 4 partner
    if any(n % 8 and n > 4 for n in lens):
        out.add("lone_beside_pair")
    if row_len is not None:
        Tb = clamp_len(row_len, T)
        rl = np.asarray(row_len)
        if (Tb <= (nsplit - 1) * chunk).any():
            out.add("empty_partial")                     # a split workgroup lies wholly behind a row's length
        if 2 * int((nsplit - -(-Tb // chunk)).sum()) > B * nsplit:
            out.add("mostly_empty")                      # more than half of the split workgroups store the empty partial
        if (rl <= 0).any():
            out.add("len0")
        if (rl > T).any():
            out.add("len_above_T")
        for d, name in ((-1, "len_chunk-1"), (0, "len_chunk"), (1, "len_chunk+1")):
            if (rl == chunk + d).any():
                out.add(name)
    return out


# ------------------------------------------------------------------ float64 reference
def reference(enc, q, row_utt=None, row_len=None):
    """-> alpha (B, Tp), cv (B, H), float64.  Row b attends over enc[row_utt[b], :min(max(row_len[b], 1), T)] (no rows: enc[b], all T)."""
    B, H = q.shape
    T = enc.shape[1]
    Tb = clamp_len(row_len, T) if row_len is not None else np.full(B, T)
    alpha, cv = np.zeros((B, padded(T))), np.zeros((B, H))
    for b in range(B):
        e = enc[b if row_utt is None else int(row_utt[b]), :Tb[b]].astype(np.float64)
        s = e @ q[b].astype(np.float64)
        w = np.exp(s - s.max())
        w /= w.sum()
        alpha[b, :Tb[b]] = w
        cv[b] = w @ e
    return alpha, cv


def reference_bwd(enc, alpha, cv, d_cv):
    """-> ds (B, Tp), dq (B, H), float64: ds = alpha (enc.d_cv - cv.d_cv), dq = sum_t ds enc."""
    B, T, H = enc.shape
    alpha, cv, d_cv = (np.asarray(x, np.float64) for x in (alpha, cv, d_cv))
    ds, dq = np.zeros((B, padded(T))), np.zeros((B, H))
    for b in range(B):
        e = enc[b].astype(np.float64)
        ds[b, :T] = alpha[b, :T] * (e @ d_cv[b] - cv[b] @ d_cv[b])
        dq[b] = ds[b, :T] @ e
    return ds, dq


def bound_ratio(got, ref, rtol):
    """max |got - ref| as a fraction of the bound rtol * max |ref| (test_gpu_ops.close's); NaN / inf anywhere -> inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not np.isfinite(got).all():
        return np.inf
    return float(np.abs(got - ref).max() / (rtol * max(np.abs(ref).max(), 1e-6)))


# ------------------------------------------------------------------ float32, in the kernel's order
F = np.float32


def _dot(a, b, H):
    """wave_sum(dot_row(a, b)): lane l holds columns 256 c + 4 l .. + 3 of every chunk c; per chunk x + y + z + w, chunks in order, then
    the xor butterfly over the 64 lanes.  a, b: (B, H) float32 -> (B,) float32."""
    n = nch(H)
    p = np.zeros((a.shape[0], n * 256), F)
    p[:, :H] = a * b
    p = p.reshape(-1, n, 64, 4)
    s = np.zeros((a.shape[0], 64), F)
    for c in range(n):
        s = s + (((p[:, c, :, 0] + p[:, c, :, 1]) + p[:, c, :, 2]) + p[:, c, :, 3])
    o = 32
    while o:
        s = s[:, :o] + s[:, o:2 * o]
        o >>= 1
    return s[:, 0]


def _steps(t0, chunk, wave):
    return range(t0 + wave, t0 + chunk, 8)


def _rows_of(enc, utt, t, T):
    """enc[utt[b], t] per row b; a row index at or past T reads zeros (what the planted lone-row mistake reads behind the buffer)."""
    if t >= T:
        return np.zeros((len(utt), enc.shape[2]), F)
    return enc[utt, t]


def kernel_model(enc, q, row_utt=None, row_len=None, mistake=None):
    """-> alpha (B, Tp), cv (B, H), float32, computed the way attn_fwd_partial computes them.  mistake (MISTAKES): "nch4" = columns >= 1024
    never loaded (the NCH = 4 body launched for an NCH = 8 width); "empty_weight_1" = the merges weigh an empty partial (m = -inf) with
    1 instead of 0; "empty_guard_dropped" = they weigh it with expf(m - M) as written, with no guard; "lone_row_pair" = a wave whose last
    step holds one row reads the t + 4 row all the same (the next chunk's, or behind the buffer: zeros here)."""
    assert mistake is None or mistake in MISTAKES, mistake
    enc, q = np.asarray(enc, F), np.asarray(q, F)
    B, H = q.shape
    T = enc.shape[1]
    Tp = padded(T)
    if mistake == "nch4" and H > 1024:
        enc, q = enc.copy(), q.copy()
        enc[:, :, 1024:] = 0
        q[:, 1024:] = 0
    nsplit, chunk = split_for(B, T)
    utt = np.arange(B) if row_utt is None else np.asarray(row_utt, np.int64)
    Tb = clamp_len(row_len, T) if row_len is not None else np.full(B, T)
    scores = np.zeros((B, Tp), F)
    pm, pl, pacc = np.zeros((nsplit, B), F), np.zeros((nsplit, B), F), np.zeros((nsplit, B, H), F)

    def weight(m, M):
        with np.errstate(invalid="ignore"):
            w = np.exp(m - M).astype(F)
        if mistake == "empty_guard_dropped":
            return w
        return np.where(np.isneginf(m), F(1 if mistake == "empty_weight_1" else 0), w)

    with np.errstate(invalid="ignore", over="ignore"):
        for sp in range(nsplit):
            t0 = sp * chunk
            t1 = np.minimum(Tb, t0 + chunk)
            wm, wl, wacc = np.full((4, B), -np.inf, F), np.zeros((4, B), F), np.zeros((4, B, H), F)
            for wave in range(4):
                m, l, acc = wm[wave], wl[wave], wacc[wave]
                for t in _steps(t0, chunk, wave):
                    one = t < t1
                    if not one.any():
                        break
                    two = one if mistake == "lone_row_pair" else t + 4 < t1
                    for tt, on in ((t, one), (t + 4, two)):
                        if not on.any():
                            continue
                        e = _rows_of(enc, utt, tt, T)
                        s = _dot(e, q, H)
                        if tt < T:
                            scores[on, tt] = s[on]
                        mn = np.maximum(m, s)
                        sc, p = np.exp(m - mn).astype(F), np.exp(s - mn).astype(F)
                        sc = np.where(np.isneginf(m), F(0), sc)        # expf(-inf - mn) = 0
                        l[:] = np.where(on, l * sc + p, l)
                        acc[:] = np.where(on[:, None], acc * sc[:, None] + p[:, None] * e, acc)
                        m[:] = np.where(on, mn, m)
            M = wm.max(0)
            w = [weight(wm[k], M) for k in range(4)]
            pm[sp] = M
            pl[sp] = ((wl[0] * w[0] + wl[1] * w[1]) + wl[2] * w[2]) + wl[3] * w[3]
            pacc[sp] = ((wacc[0] * w[0][:, None] + wacc[1] * w[1][:, None]) + wacc[2] * w[2][:, None]) + wacc[3] * w[3][:, None]
        Mx = pm.max(0)
        wgt = np.exp(pm - Mx).astype(F)                                  # the split merge has no guard: Mx is finite, expf(-inf) = 0
        if mistake == "empty_weight_1":
            wgt = np.where(np.isneginf(pm), F(1), wgt)
        L, v = np.zeros(B, F), np.zeros((B, H), F)
        for sp in range(nsplit):
            L = L + pl[sp] * wgt[sp]
            v = v + pacc[sp] * wgt[sp][:, None]
        inv = F(1) / L
        cv = v * inv[:, None]
        alpha = np.exp(scores - Mx[:, None]).astype(F) * inv[:, None]
        alpha[np.arange(Tp)[None, :] >= Tb[:, None]] = 0
    return alpha, cv


def kernel_model_bwd(enc, alpha, cv, d_cv, mistake=None):
    """-> ds (B, Tp), dq (B, H), float32, the way attn_bwd_partial computes them (pad columns of ds, which the kernel leaves alone, 0)."""
    assert mistake is None or mistake in MISTAKES, mistake
    enc, alpha, cv, d_cv = (np.asarray(x, F) for x in (enc, alpha, cv, d_cv))
    B, T, H = enc.shape
    if mistake == "nch4" and H > 1024:
        enc, cv, d_cv = enc.copy(), cv.copy(), d_cv.copy()
        enc[:, :, 1024:] = 0
        cv[:, 1024:] = 0
        d_cv[:, 1024:] = 0
    nsplit, chunk = split_for(B, T)
    utt = np.arange(B)
    cd = _dot(cv, d_cv, H)
    ds, dq = np.zeros((B, padded(T)), F), np.zeros((B, H), F)
    for sp in range(nsplit):
        t0 = sp * chunk
        t1 = min(T, t0 + chunk)
        wacc = np.zeros((4, B, H), F)
        for wave in range(4):
            for t in range(t0 + wave, t1, 8):
                for tt in (t, t + 4):
                    if tt >= t1 and not (mistake == "lone_row_pair" and tt == t + 4):
                        continue
                    e = _rows_of(enc, utt, tt, T)
                    a = alpha[:, tt] if tt < T else np.zeros(B, F)
                    d = a * (_dot(e, d_cv, H) - cd)
                    if tt < T:
                        ds[:, tt] = d
                    wacc[wave] += d[:, None] * e
        dq = dq + (((wacc[0] + wacc[1]) + wacc[2]) + wacc[3])
    return ds, dq


# ------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class Case:
    B: int
    T: int
    H: int
    plan: tuple                                  # (nsplit, chunk) split_for gives today
    reaches: frozenset = frozenset()             # the branches (names of branches()) the entry is in the table for
    U: int = 0                                   # rows cases: utterances, row map and the row lengths of the two launches
    row_utt: tuple = ()
    row_len: tuple = ()
    row_len2: tuple = ()

    @property
    def id(self):
        return f"{self.B}-{self.T}-{self.H}"

    @property
    def rows(self):
        return self.U > 0

    def inputs(self, which=0):
        """-> enc (B or U, T, H), q (B, H), d_cv (B, H), float32.  Standard deviation H ** -0.25: scores ~ N(0, 1), so that no split's
        weight vanishes (a peaked softmax would hide a wrong low-weight partial).  which = 1: the other draw of the repeat launches."""
        rng = np.random.default_rng([self.B, self.T, self.H, which])
        sd = F(self.H ** -0.25)
        enc = rng.standard_normal((self.U or self.B, self.T, self.H), dtype=F) * sd
        q = rng.standard_normal((self.B, self.H), dtype=F) * sd
        g = rng.standard_normal((self.B, self.H), dtype=F)
        return enc, q, g

    def lengths(self, which=0):
        return np.asarray(self.row_len2 if which else self.row_len, np.int32)

    def poisoned(self, enc, which=0):
        """enc with NaN behind each utterance's longest (clamped) row length: positions no row of that utterance may read."""
        enc = enc.copy()
        Tb = clamp_len(self.lengths(which), self.T)
        for u in range(self.U):
            mine = Tb[np.asarray(self.row_utt) == u]
            enc[u, (mine.max() if mine.size else 0):] = np.nan
        return enc


def _case(B, T, H, plan, *reaches):
    return Case(B, T, H, plan, frozenset(reaches) | {f"nch{nch(H)}"})


CASES = [
    _case(1, 1, 4, (1, 1), "nsplit1", "empty_wave", "one_lane_chunk"),
    _case(1, 7, 252, (1, 7), "nsplit1", "ragged_chunk", "lone_beside_pair"),
    _case(1, 8, 256, (1, 8), "nsplit1"),
    _case(1, 9, 2048, (2, 8), "last_chunk_1", "empty_wave", "lone_row"),
    _case(1, 13, 516, (2, 8), "lone_beside_pair", "one_lane_chunk"),
    _case(1, 1024, 1028, (128, 8), "nsplit128", "one_lane_chunk"),
    _case(1, 1025, 260, (114, 9), "clamp", "lone_beside_pair", "one_lane_chunk"),
    _case(1, 2000, 2048, (125, 16), "clamp"),
    _case(3, 1100, 1540, (123, 9), "clamp", "last_chunk_2", "empty_wave", "ragged_chunk", "lone_beside_pair"),
    _case(64, 420, 1540, (8, 53), "ragged_chunk", "lone_beside_pair"),
    _case(511, 20, 8, (2, 10), "B511", "lone_beside_pair"),
    _case(512, 20, 8, (1, 20), "B512", "nsplit1"),
    _case(600, 37, 1028, (1, 37), "nsplit1", "one_lane_chunk", "lone_beside_pair"),
]


def _rows_case(R, U, T, H, plan, row_utt, row_len, row_len2, *reaches):
    return Case(R, T, H, plan, frozenset(reaches) | {f"nch{nch(H)}"}, U, tuple(row_utt), tuple(row_len), tuple(row_len2))


def _len_set(chunk, T):
    return [0, 1, chunk - 1, chunk, chunk + 1, T, T + 5]


_UTT6 = [1, 0, 1, 1, 0, 0]
_S12, _S8, _S9, _S37 = _len_set(12, 1025), _len_set(8, 201), _len_set(9, 1025), _len_set(37, 37)
ROWS_CASES = [
    # six rows over two utterances; every value of {0, 1, chunk - 1, chunk, chunk + 1, T, T + 5} occurs in one of the two launches, and
    # in each launch one utterance's rows all end early (so part of enc is poisoned)
    _rows_case(6, 2, 1025, 2048, (86, 12), _UTT6, [_S12[i] for i in (0, 1, 2, 3, 4, 6)], [_S12[i] for i in (3, 5, 1, 2, 4, 0)],
               "empty_partial", "mostly_empty", "len0", "len_above_T", "len_chunk-1", "len_chunk", "len_chunk+1"),
    _rows_case(6, 2, 201, 1028, (26, 8), _UTT6, [_S8[i] for i in (5, 2, 6, 0, 4, 3)], [_S8[i] for i in (1, 6, 2, 3, 0, 4)],
               "empty_partial", "len0", "len_above_T", "len_chunk-1", "len_chunk", "len_chunk+1", "one_lane_chunk"),
    # the clamped plan needs R <= 4 rows: three rows, two of them short -- most split workgroups store the empty partial
    _rows_case(3, 2, 1025, 260, (114, 9), [1, 0, 1], [_S9[i] for i in (2, 6, 4)], [_S9[i] for i in (3, 0, 5)],
               "clamp", "empty_partial", "mostly_empty", "len_chunk-1", "len_chunk+1", "len_above_T"),
    # one workgroup per row: the last arriver is the only arriver
    _rows_case(600, 5, 37, 260, (1, 37), [r % 5 for r in range(600)], [_S37[r % 7] if r % 5 else 1 + r % 9 for r in range(600)],
               [_S37[(r + 3) % 7] if (r + 2) % 5 else 2 + r % 11 for r in range(600)], "nsplit1", "len0", "len_above_T", "len_chunk-1",
               "len_chunk"),
]

# the refusals of the exported entry points: (B, T, H), what is wrong
REFUSED_WIDTHS = [(2, 9, 2052), (2, 9, 6)]
