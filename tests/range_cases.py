"""Shared by the operator tests (tests/test_gpu_ops.py), the value-range GPU tests (tests/test_gpu_ranges.py) and their CPU feasibility
module (tests/test_ranges_host.py): the NumPy draws of the decoder, encoder-stack and CNN operator cases with GAINS on them -- `enc_gain`
(encoder states: wide attention scores), `out_gain` (output projection: wide logits), `bias_gain` (LSTM biases: saturated gates),
`x_gain` / `x_offset` (operator input: saturated layer-0 gates / BatchNorm channels with a mean far from 0) -- plus the attention and
softmax-CE value cases and the committed case tables.  Nothing here touches a GPU.  With every gain at its default the draws are, bit for
bit, the ones the operator tests have always used (a gain of 1 / an offset of 0 is not applied at all).

Ladders: each family has a ladder of gains; the tables below hold, per shape, the LARGEST rung at which the straightforward float32
restatement of the operator (oracle/ast_ref_torch.py on float32 tensors, two-pass variances) still meets a fraction of the GPU test's
tolerance against float64 (a quarter; half for the BatchNorm offset cases, whose float32 input already carries r * 2^-24), together
with that restatement's measured error and the case's defining property on the float64 reference.  tests/test_ranges_host.py asserts
both for every row: a rung that fails there is not loosened, it moves one rung down."""
import numpy as np


def _gain(a, g):
    return a if g == 1.0 else a * g


# ------------------------------------------------------------------ decoder
def dec_draws(B, L, T, H, E, A, V, nl, masks, seed=0, enc_gain=1.0, out_gain=1.0, bias_gain=1.0):
    rng = np.random.default_rng(seed)
    P = {"embed_dec/W": rng.standard_normal((V, E)), "attn_Wa/W": rng.standard_normal((H, H)) / np.sqrt(H),
         "attn_Wa/b": rng.standard_normal(H) * 0.1, "context/W": rng.standard_normal((A, 2 * H)) / np.sqrt(2 * H),
         "context/b": rng.standard_normal(A) * 0.1, "out/W": rng.standard_normal((V, A)) / np.sqrt(A),
         "out/b": rng.standard_normal(V) * 0.1}
    n_in = E + A
    for k in range(nl):
        P[f"L{k}_dec/upward/W"] = rng.standard_normal((4 * H, n_in)) / np.sqrt(n_in)
        P[f"L{k}_dec/upward/b"] = rng.standard_normal(4 * H) * 0.2
        P[f"L{k}_dec/lateral/W"] = rng.standard_normal((4 * H, H)) / np.sqrt(H)
        n_in = H
    enc = rng.standard_normal((B, T, H)) * 0.5
    c0, h0 = rng.standard_normal((nl, B, H)) * 0.5, np.tanh(rng.standard_normal((nl, B, H)))
    y = np.zeros((B, L), np.int32)
    for b in range(B):
        n = L if (b == 0 or L <= 3) else int(rng.integers(max(L // 2, 3), L + 1))
        y[b, 0], y[b, 1:n - 1], y[b, n - 1] = 1, rng.integers(4, V, size=n - 2), 2
    S = L - 1
    flags = [1] + [int(rng.random() < 0.5) for _ in range(S - 2)] + [1] if S >= 2 else [1] * S
    em = ((rng.random((S, B, E)) >= 0.3) / 0.7) if masks else None
    rm = ((rng.random((nl, S, B, H)) >= 0.3) / 0.7) if masks else None
    # the gains, behind every draw (the stream of random numbers does not depend on them)
    enc = _gain(enc, enc_gain)
    P["out/W"] = _gain(P["out/W"], out_gain)
    for k in range(nl):
        P[f"L{k}_dec/upward/b"] = _gain(P[f"L{k}_dec/upward/b"], bias_gain)
    return dict(P=P, enc=enc, c0=c0, h0=h0, y=y, flags=flags, em=em, rm=rm, S=S)


# ------------------------------------------------------------------ encoder stacks
def lstm_draws(T, B, in_dim, h, nl, masks, bias_gain=1.0, x_gain=1.0, seed=None):
    """Parameters, input, masks and the three upstream gradients (enc_states (B, T, 2h); cT, hT (2, nl, B, h)) in the operator test's draw order.
    seed: default T + B, the operator test's."""
    rng = np.random.default_rng(T + B if seed is None else seed)
    P, names = {}, []
    for pat in ("L{}_enc", "L{}_rev_enc"):
        n_in = in_dim
        for k in range(nl):
            n = pat.format(k)
            names.append(n)
            P[n + "/upward/W"] = rng.standard_normal((4 * h, n_in)) / np.sqrt(n_in)
            P[n + "/upward/b"] = rng.standard_normal(4 * h) * 0.3
            P[n + "/lateral/W"] = rng.standard_normal((4 * h, h)) / np.sqrt(h)
            n_in = h
    x = rng.standard_normal((T, B, in_dim))
    mk = ((rng.random((2, nl, T, B, h)) >= 0.3) / 0.7) if masks else None
    g_enc, g_c, g_h = rng.standard_normal((B, T, 2 * h)), rng.standard_normal((2, nl, B, h)), rng.standard_normal((2, nl, B, h))
    for n in names:
        P[n + "/upward/b"] = _gain(P[n + "/upward/b"], bias_gain)
    x = _gain(x, x_gain)
    return dict(P=P, names=names, x=x, mk=mk, g_enc=g_enc, g_c=g_c, g_h=g_h)


# ------------------------------------------------------------------ CNN front-end
def cnn_cfg(c0, c1):
    from conftest import tiny_cfg
    return tiny_cfg(c0=c0, c1=c1)


def cnn_geometry_cfg(layers, pool=None):
    """tiny_cfg with its convolution stack replaced: layers = [(C, kt, kf, st, sf, pt), ...] (no frequency padding); pool: the optional
    per-layer (time, frequency) max-pooling windows of the old path (cnn_config["cnn_pool"])."""
    from conftest import tiny_cfg
    cfg = tiny_cfg()
    cfg["cnn_config"]["cnn_layers"] = [{"in_channels": None, "out_channels": C, "ksize": [kt, kf], "stride": [st, sf], "pad": [pt, 0]}
                                       for C, kt, kf, st, sf, pt in layers]
    if pool is not None:
        cfg["cnn_config"]["cnn_pool"] = [list(w) for w in pool]
    return cfg


def shipped_layers(c0, c1):
    """The shipped two-layer geometry as a `layers` list."""
    return [(c0, 9, 13, 2, 13, 4), (c1, 9, 1, 2, 1, 4)]


def cnn_draws(B, T, D, c0, c1, with_noise, x_offset=0.0, seed=0, ramp=True, centre_taps=False, layers=None, pool=None):
    """-> cfg, P (float64), X, noise, rng (the generator behind the draws: the upstream gradient comes from it once the output shape is known).
    x_offset: X = N(0, 1) + x_offset * (0.5 + d / D) per frequency bin d (ramp = False: + x_offset on every bin); seed: of the weights
    (seed + 1) and of everything else; centre_taps: the layer-0 weights keep their centre time tap only (the other time taps are 0), so
    that no output step loses taps to the zero padding in time -- with ramp = False every output of a channel then carries the same
    offset x_offset * (tap sum) and the channel's spread is the noise's alone.  layers: None = the shipped two layers with (c0, c1)
    channels; else the stack as cnn_geometry_cfg takes it (c0, c1 are not used then), the draws in the same order: weights, then per layer
    gamma and beta, then X, then the noise.  pool: cnn_geometry_cfg's."""
    from oracle.ast_ref import init_params
    cfg = cnn_cfg(c0, c1) if layers is None else cnn_geometry_cfg(layers)
    if pool is not None:
        cfg["cnn_config"]["cnn_pool"] = [list(w) for w in pool]
    P = init_params(cfg, D, 11, seed=seed + 1, dtype=np.float64)
    rng = np.random.default_rng(seed)
    for i in range(len(cfg["cnn_config"]["cnn_layers"])):      # non-trivial BN affine, every layer
        P[f"CNN_{i}_bn/gamma"] = 1 + 0.3 * rng.standard_normal(P[f"CNN_{i}_bn/gamma"].shape)
        P[f"CNN_{i}_bn/beta"] = 0.2 * rng.standard_normal(P[f"CNN_{i}_bn/beta"].shape)
    X = rng.standard_normal((B, T, D))
    noise = rng.normal(1.0, 0.25, X.shape) if with_noise else None
    if x_offset != 0.0:
        X = X + (x_offset * (0.5 + np.arange(D) / D) if ramp else x_offset)
    if centre_taps:
        W = P["CNN_0/W"]                     # (C, 1, kt, kf)
        keep = np.zeros_like(W)
        keep[:, :, W.shape[2] // 2] = W[:, :, W.shape[2] // 2]
        P["CNN_0/W"] = keep
    return cfg, P, X, noise, rng


# ------------------------------------------------------------------ attention value cases (operator level)
ATTN_SHAPES = [(3, 6, 8), (32, 50, 512), (5, 201, 260), (2, 9, 1024)]
ATTN_PLANT = 300.0            # how far a planted maximum stands above every other score
ATTN_WIDE = 220.0             # score range of every row of the `wide` case (asserted >= 200 on the reference)


def attn_positions(T):
    """Where the planted maximum goes: the waves stride 8 rows with a +4 pair, chunks split T."""
    return sorted({p for p in (0, 1, 4, 7, 8, T // 2, T - 2, T - 1) if 0 <= p < T})


def attn_case(kind, B, T, H, pos=None, level=0.0):
    """float32 inputs (enc (B, T, H), q (B, H)) of one value case, on the operator test's base draw.  kind: "base"; "wide" (q scaled so that
    every row's scores span ATTN_WIDE); "plant" (row `pos` of enc = c q / |q|^2: its score stands ATTN_PLANT above the rest); "tie"
    (rows 0 and T - 1 identical and both ATTN_PLANT above the rest); "flat" (q = 0); "level" (every score shifted by `level`: a multiple
    of q / |q|^2 added to every enc row).  The float64 reference is formed from these float32 values."""
    rng = np.random.default_rng(B * T)
    enc = rng.standard_normal((B, T, H)) * 0.5
    q = rng.standard_normal((B, H)) * 0.5
    s = np.einsum("bth,bh->bt", enc, q)
    unit = q / (q * q).sum(1, keepdims=True)                 # enc row u * unit scores u
    if kind == "wide":
        q = q * (ATTN_WIDE / (s.max(1) - s.min(1)))[:, None]
    elif kind == "plant":
        enc[:, pos] = (s.max(1) + ATTN_PLANT)[:, None] * unit
    elif kind == "tie":
        enc[:, 0] = (s.max(1) + ATTN_PLANT)[:, None] * unit
        enc[:, T - 1] = enc[:, 0]
    elif kind == "flat":
        q = np.zeros_like(q)
    elif kind == "level":
        enc = enc + level * unit[:, None, :]
    else:
        assert kind == "base", kind
    return enc.astype(np.float32), q.astype(np.float32)


def attn_rows_case(kind):
    """The per-row variant: R = 6 rows over U = 2 utterances, (T, H) = (201, 260), row_len in {1, 2, 50, 201} (whole splits lie behind a
    short row's length).  kind "wide": every row's scores over its OWN length span ATTN_WIDE (rows of length 1 have no range);
    "plant": row r's maximum sits at row_len[r] - 1, planted in a copy of the utterance per row (U = R then)."""
    T, H = 201, 260
    row_len = np.array([1, 2, 50, 201, 50, 2], np.int32)
    row_utt = np.array([0, 0, 0, 0, 1, 1], np.int32)
    rng = np.random.default_rng(77)
    enc = rng.standard_normal((2, T, H)) * 0.5
    q = rng.standard_normal((6, H)) * 0.5
    if kind == "wide":
        for r in range(6):
            s = enc[row_utt[r], :row_len[r]] @ q[r]
            if row_len[r] > 1:
                q[r] *= ATTN_WIDE / (s.max() - s.min())
    else:
        assert kind == "plant", kind
        enc = enc[row_utt].copy()                              # one utterance per row: each gets its own planted row
        row_utt = np.arange(6, dtype=np.int32)
        for r in range(6):
            s = enc[r, :row_len[r]] @ q[r]
            enc[r, row_len[r] - 1] = (s.max() + ATTN_PLANT) * q[r] / (q[r] * q[r]).sum()
    return enc.astype(np.float32), q.astype(np.float32), row_utt, row_len


# ------------------------------------------------------------------ softmax cross-entropy value cases (operator level)
CE_VOCABS = [1, 5, 255, 256, 257, 1098]
CE_KINDS = ["wide", "plus", "minus", "tmin", "tmax", "tie_stride", "tie_waves", "clamp"]


def ce_case(kind, V, B=6):
    """float32 logits (B, V), targets (B,), class weights (V,) of one value case.  "wide": logits ~ N(0, 60^2); "plus" / "minus": the same
    at +1e4 / -1e4; "tmin" / "tmax": the target at the row's minimum (its probability underflows) / maximum; "tie_stride" / "tie_waves":
    the exact maximum duplicated at v1 < v2 = v1 + 256 (one thread's stride of a 256-thread workgroup) / at v2 in another wave;
    "clamp": a target id equal to V in row 1 (quirk Q8: clamped to V - 1).  Row 0's target always has class weight 0."""
    rng = np.random.default_rng(1000 + V)
    x = (rng.standard_normal((B, V)) * 60).astype(np.float32)
    t = rng.integers(0, V, B).astype(np.int32)
    w = np.ones(V, np.float32)
    if V > 1:
        t[0] = 0
        t[1:] = np.maximum(t[1:], 1)
        w[0] = 0
    if kind == "plus":
        x = (x.astype(np.float64) + 1e4).astype(np.float32)
    elif kind == "minus":
        x = (x.astype(np.float64) - 1e4).astype(np.float32)
    elif kind in ("tmin", "tmax") and V > 1:
        xs = x.copy()
        xs[:, 0] = np.nan                                       # (class 0 weighs nothing: keep the targets off it)
        t[1:] = (np.nanargmin(xs, 1) if kind == "tmin" else np.nanargmax(xs, 1))[1:]
    elif kind in ("tie_stride", "tie_waves") and V > 1:
        for b in range(B):
            v1 = b % min(V - 1, 60)
            v2 = v1 + 256 if kind == "tie_stride" else v1 + 70 + 64 * (b % 3)
            v2 = min(v2, V - 1) if v2 >= V else v2
            top = np.float32(x[b].max() + np.float32(3.0))
            x[b, v1] = x[b, v2] = top
    elif kind == "clamp":
        t[1 % B] = V
    else:
        assert kind == "wide" or V == 1, kind
    return x, t, w


def ce_row_bound(x, want, rel=1e-5):
    """Bound on a loss row's error: `rel` of the case's largest loss row, plus one float32 ulp of the largest |logit| (times the 1 / B the
    rows carry): the row is lse - x[t] formed in float32 from two numbers of the logits' size, so that ulp is its resolution whatever the
    kernel -- a target at the row's maximum has a loss of 1e-9..1e-5 behind logits of 150, and at a level of 1e4 one ulp is 1e-3."""
    return rel * np.abs(want).max() + float(np.spacing(np.float32(np.abs(x).max()))) / x.shape[0]


def ce_grad_bound(x, ref, rtol=2e-4):
    """Bound on the gradient's error: close()'s `rtol` of the largest entry, but no less than what the rounding of x - lse allows: two
    float32 ulps of the largest |logit| move every probability by that fraction of itself (times the 1 / B the gradient carries) --
    the floor decides only where the whole gradient is that small (the target at a maximum that stands alone)."""
    return max(rtol * float(np.abs(np.asarray(ref)).max()), 2 * float(np.spacing(np.float32(np.abs(x).max()))) / x.shape[0])


# ------------------------------------------------------------------ the committed case tables
# Every row: the case, then the float32 restatement's measured error against float64 (fractions of the reference tensor's maximum, as
# close() measures) and the defining property on the float64 reference, both at the GPU test's full shape.  tests/test_ranges_host.py
# asserts the bounds and the properties (the decoder shapes with H >= 512 on the first four rows of the same draws: rows are independent).
#
# Where a ladder as first planned ended below the family's own condition, rungs were added ABOVE it (marked +): the condition -- underflow of
# exp(s - max), a logit range of 200, |z| >= 44 -- is what the case is for.
ENC_LADDER = (3.0, 4.0, 6.0, 8.0, 10.0, 12.0, 16.0, 32.0, 48.0)      # + from 8 on: at x6 no H >= 512 shape has every step-0 score range above 88
OUT_LADDER = (16.0, 128.0, 384.0)                              # + 128, 384: x16 gives step-0 logit ranges of 14-47, the condition is 200
OUT_GAIN = 384.0
DEC_BIAS_GAINS = (20.0, 80.0)                                  # + 80: x20 (bias sigma 4) reaches |z| = 13-19, x80 reaches 51-63
LSTM_LADDER = ((5.0, 2.0), (10.0, 4.0), (20.0, 6.0), (40.0, 12.0))      # (bias_gain, x_gain); + (40, 12): at (20, 6) 5-11 % saturated, max |z| 36-43
X_OFFSET_LADDER = (8.0, 32.0, 64.0)
LEVEL_LADDER = (200.0, 1000.0, 5000.0)

# Decoder loops over wide attention scores: (shape (B, L, T, H, E, A, V, nl, masks), seed offset, enc_gain, loop, worst gradient tensor, step-0
# score range over the rows).  Budget 1.25e-4.  Peaked attention makes the gradients ill-conditioned in float32 itself and not monotonically
# in the gain: at most (seed, gain) pairs of the one-layer H >= 512 shapes the float32 restatement is 1e-3 to 1e-2 off (the seeds were searched).
DEC_ENC_CASES = [
    ((19, 8, 37, 128, 32, 64, 130, 3, True), 0, 16.0, "persist", 8.3e-5, "67-123"),            # generic scan
    ((32, 7, 50, 512, 128, 512, 1098, 1, True), 250, 12.0, "persist", 8.2e-5, "115-217"),    # resident H = 512
    ((32, 7, 50, 512, 128, 512, 1098, 3, True), 0, 12.0, "persist", 8.7e-5, "105-185"),      # ... with 3 layers
    ((32, 5, 300, 512, 128, 512, 1098, 1, False), 10, 12.0, "persist", 6.3e-5, "135-185"),   # streamed
    ((32, 4, 420, 512, 128, 512, 1098, 3, True), 0, 10.0, "persist", 2.5e-5, "138-210"),     # streamed, 3 layers
    ((37, 5, 50, 512, 128, 512, 300, 1, False), 330, 12.0, "persist", 1.2e-4, "92-169"),     # row split
    ((32, 7, 40, 1024, 128, 1024, 1098, 1, True), 60, 12.0, "persist", 1.1e-4, "130-256"),   # wide
    ((5, 9, 23, 32, 12, 24, 57, 3, True), 1, 32.0, "per_launch", 8.7e-5, "40-87"),           # per-launch loop
    ((32, 9, 50, 512, 128, 512, 1098, 1, True), 150, 10.0, "per_launch", 4.2e-5, "96-178"),
]
DEC_ENC_KNOB_CASE = ((32, 7, 50, 512, 128, 512, 1098, 1, True), 2, 10.0)      # worst 8.9e-5, step-0 score range 98-158; the older role layouts
# CE roles over wide logits: (shape, seed offset, loop); out_gain = OUT_GAIN.  Worst gradient tensor 1.0e-6 / 1.9e-5 / 6.1e-6 / 6.5e-6, step-0 logit
# ranges 245-415 / 456-846 / 333-656 / 586-969.
DEC_OUT_CASES = [((5, 9, 23, 32, 12, 24, 57, 3, True), 1, "per_launch"), ((32, 7, 50, 512, 128, 512, 1098, 1, True), 0, "persist"),
                 ((19, 8, 37, 128, 32, 64, 130, 3, True), 0, "persist"), ((9, 6, 30, 1024, 128, 1024, 8004, 1, False), 0, "persist")]
# Saturated decoder gates: (shape, seed offset), each under both DEC_BIAS_GAINS.  Worst gradient tensor at x20 / x80: 2.2e-6 / 2.4e-6, 8.2e-7 / 1.0e-6,
# 8.0e-6 / 5.2e-6; at x80 38-40 % of the step-0 i / f / o gates lie within 1e-6 of 0 or 1 and max |z| is 52 / 62 / 53.
DEC_BIAS_CASES = [((32, 7, 50, 512, 128, 512, 1098, 1, True), 0), ((19, 8, 37, 128, 32, 64, 130, 3, True), 0), ((32, 7, 40, 1024, 128, 1024, 1098, 1, True), 0)]
# (x20 is the gain first planned: it reaches |z| = 13-19 and saturates nothing to 1e-6 -- its rows pin the loops on large biases, no more;
#  the family's condition, a tenth of the gates saturated and |z| >= 44, is carried by x80)
DEC_SATURATED = {20.0: (0.0, 12.0), 80.0: (0.10, 44.0)}         # bias_gain -> (least saturated share, least max |z|) asserted on the reference's step 0

# Encoder stacks with saturated gates: ((T, B, in, h, nl, masks), (bias_gain, x_gain), (forward, gradient) error, (saturated share, max |z|)).
# Budgets 5e-5 / 1.25e-4.
LSTM_CASES = [((9, 5, 24, 20, 3, True), (40.0, 12.0), (8.7e-7, 1.2e-6), (0.33, 72.2)),
              ((12, 5, 24, 64, 3, True), (40.0, 12.0), (1.9e-6, 1.7e-6), (0.31, 71.8)),
              ((6, 16, 32, 256, 3, True), (40.0, 12.0), (2.2e-6, 2.6e-6), (0.30, 83.5)),
              ((3, 4, 16, 512, 1, False), (40.0, 12.0), (2.1e-6, 3.5e-6), (0.43, 84.9)),
              ((3, 4, 16, 1024, 2, False), (40.0, 12.0), (2.2e-6, 1.9e-6), (0.33, 78.6))]
LSTM_ROWS32_CASE = ((6, 32, 32, 256, 3, True), (40.0, 12.0))     # the two 32-row forms

# BatchNorm statistics with offset channels: ((B, T, D, c0, c1), with_noise, x_offset, seed, centre, one_pass_fails) with r = the largest layer-0
# |channel mean| / std asserted >= x_offset / 2 on every row.  centre = False: X = N(0, 1) + x_offset (0.5 + d / D) on the drawn weights.  There
# the ramp over the frequency blocks and the zero padding in time put the offset into each channel's VARIANCE as well (r = 3.2-6.3 at
# every rung; six blocks of 80 bins cap it at 3.5), so only the lowest rung, on the 13- and 26-bin shapes, has the property (seeds searched
# over 0..11).  centre = True (cnn_draws: ramp = False, centre_taps = True): the same offset on every bin and layer-0 weights with the centre
# time tap only -- no output step loses taps to the padding, every output of a channel carries x_offset * (tap sum), the spread is the
# noise's: r = 98 / 148 / 154 / 51 at x_offset = 64.  Two-pass float32 against float64 there: output <= 6.7e-6, statistics <= 4.1e-6,
# gradients <= 1.6e-5 (budget: half the tolerance, 1e-4 / 2.5e-4).  one_pass_fails: E[y^2] - E[y]^2 in float32 misses the GPU test's bounds on
# that row (output 2.6e-4 / 3.4e-4 / 3.5e-4 against 2e-4; on the 16-row shape it stays at 2.1e-5) -- asserted by the host module.
CNN_CASES = [((2, 170, 26, 16, 8), False, 8.0, 1, False, False), ((2, 16, 13, 4, 4), False, 8.0, 1, False, False),
             ((2, 16, 13, 4, 4), True, 8.0, 1, False, False),
             ((2, 50, 80, 8, 12), False, 64.0, 0, True, True), ((2, 170, 26, 16, 8), False, 64.0, 0, True, True),
             ((3, 331, 80, 128, 32), False, 64.0, 0, True, True), ((2, 16, 13, 4, 4), False, 64.0, 0, True, False),
             ((2, 50, 80, 8, 12), True, 8.0, 0, True, False)]


# CNN front-end geometries (tests/test_gpu_cnn_geometry.py): (id, B, T, D, layers [(C, kt, kf, st, sf, pt), ...], seed without noise, seed with noise).
# Every other CNN case of the suite runs the shipped geometry (kernel (9, 13) stride (2, 13) pad 4, then (9, 1) (2, 1) 4, two layers), where
# sf == kf, st = 2, kt = 9, pt = 4 -- a frequency offset f * kf for f * sf, or stride-phase arithmetic right for two phases only, would pass.
# The seeds: cnn_draws' convention; the smallest at which the float64 reference has NO post-BatchNorm pre-activation within 2e-5 of the
# ReLU's kink in any layer (searched on the CPU, asserted by the GPU test and by tests/test_ranges_host.py), so that every gradient is held
# to the tight 5e-4.  What each row reaches:
#   kt5-kf8-l1s1     direct kernel with kt * JP = 100, even kf (JG = 8), F' = 10; layer 1 with stride 1 (one phase)
#   kf14-sf7-pt0     kf = the direct kernel's maximum (no pad column in XF), overlapping frequency windows, no time padding, even kt above
#   gaps-pt6-l1s3    sf > kf (input bins no window covers), pt = kt - 1, an uncovered trailing input row; three stride phases above
#   kt2-st2          kt == st at both layers (one tap per phase), F' = 1
#   kf1              kf = 1 (JG = 2)
#   two-tiles        three direct-kernel tiles per (b, f) (167 output steps, ragged last), C0 = 48 (the second wave holds half its channels)
#   kt11-st3-kf16    im2col under every scheme: kt > 9, kf > 14, odd stride
#   st1-l1s13        layer-0 stride 1; 13 stride phases over 12 phase-weight buffers (the flush); 5 uncovered input rows
#   one-layer        layer 0 is the last layer
#   three-layers     a middle layer (consumes and produces padded buffers)
#   four-layers      ASTK_MAX_CNN_LAYERS
#   one-layer-c64    layer 0 is the last layer AND has the 64 channels the tiled sequence re-layout / its fused BatchNorm backward need
#   f10-c64-last     those tiled kernels at F' = 10 (6 (t, b) pairs per 64-slot block iteration, 4 slots idle)
#   f20-kf4          F' = 20 > 16: the un-tiled re-layout and the row-layout BatchNorm backward behind a direct layer 0 with kf = 4
CNN_GEOMETRY_CASES = [
    ("kt5-kf8-l1s1", 3, 45, 80, [(16, 5, 8, 2, 8, 2), (8, 3, 1, 1, 1, 1)], 0, 0),
    ("kf14-sf7-pt0", 2, 51, 40, [(32, 9, 14, 2, 7, 0), (12, 4, 1, 2, 1, 0)], 0, 0),
    ("gaps-pt6-l1s3", 2, 64, 26, [(16, 7, 5, 2, 9, 6), (8, 6, 1, 3, 1, 2)], 0, 0),
    ("kt2-st2", 3, 37, 13, [(16, 2, 13, 2, 13, 0), (8, 2, 1, 2, 1, 0)], 0, 0),
    ("kf1", 2, 40, 6, [(16, 9, 1, 2, 1, 4), (4, 9, 1, 2, 1, 4)], 0, 0),
    ("two-tiles", 2, 333, 26, [(48, 7, 12, 2, 12, 3), (8, 5, 1, 2, 1, 2)], 2, 4),
    ("kt11-st3-kf16", 2, 70, 80, [(8, 11, 16, 3, 16, 5), (8, 5, 1, 3, 1, 1)], 0, 0),
    ("st1-l1s13", 2, 60, 20, [(4, 4, 5, 1, 3, 0), (4, 13, 1, 13, 1, 0)], 1, 0),
    ("one-layer", 3, 50, 80, [(16, 9, 13, 2, 13, 4)], 0, 4),
    ("three-layers", 2, 90, 80, [(16, 9, 13, 2, 13, 4), (12, 9, 1, 2, 1, 4), (8, 3, 1, 1, 1, 1)], 0, 0),
    ("four-layers", 2, 120, 26, [(16, 9, 13, 2, 13, 4), (8, 9, 1, 2, 1, 4), (8, 4, 1, 3, 1, 0), (4, 5, 1, 2, 1, 2)], 0, 0),
    ("one-layer-c64", 2, 50, 80, [(64, 9, 13, 2, 13, 4)], 0, 0),
    ("f10-c64-last", 2, 45, 80, [(16, 5, 8, 2, 8, 2), (64, 3, 1, 1, 1, 1)], 1, 1),
    ("f20-kf4", 2, 30, 80, [(16, 5, 4, 2, 4, 2), (8, 3, 1, 2, 1, 1)], 0, 0),
]
# Max-pooling on a layer 0 that is otherwise eligible for the direct kernel (the shipped geometry with 16 channels): (B, T, D, c0, c1, pool).
# A pooled layer's BatchNorm sees the POOLED rows; the direct kernel's fused statistics are sums over the un-pooled ones.
CNN_POOL_DIRECT_CASES = [(2, 30, 26, 16, 8, [[-1, 1], [1, 1]]), (2, 42, 80, 16, 8, [[1, -1], [1, 1]]), (3, 42, 80, 16, 8, [[2, 1], [1, 1]])]


def conv0_direct_shape(layers, pool=None):
    """conv.hip's conv0_direct_shape restated: the layer-0 shapes the direct convolution takes (under the default arithmetic, bf16x3) --
    the LDS window of an 80-step tile fits 4096 elements (stride 2 only, with the even-stride rule), the f32 weights fit 64 KiB, kt rows
    of 20 columns fit six 32-wide MFMA steps (kt <= 9), kf <= 14, up to 128 channels in multiples of 16, and the layer does not pool."""
    C, kt, kf, st, sf, pt = layers[0]
    win = st * 20 * 79 + 32 * 6 + 40
    pooled = pool is not None and any(w not in (0, 1) for w in pool[0])
    return (win <= 512 * 8 and C * kt * kf * 4 <= 64 * 1024 and kt * 20 <= 32 * 6 and kf <= 14 and st % 2 == 0 and C <= 128
            and C % 16 == 0 and not pooled)


def cnn_case_kw(centre):
    return dict(ramp=False, centre_taps=True) if centre else {}


# Attention score level per shape (B, T, H): the largest rung of LEVEL_LADDER at which float32 scores still resolve alpha to a quarter of 2e-4
# (one ulp of a float32 score at 5000 is 4.9e-4: the level enters alpha through the rounding of the score itself).
# Measured (worse sign): (3,6,8) 8.5e-6 / 3.9e-5 / 2.8e-4 at 200 / 1000 / 5000; (32,50,512) 2.2e-5 / 1.3e-4 / 5.3e-4; (5,201,260) 1.2e-5 / 7.7e-5 / 7.9e-4;
# (2,9,1024) 4.4e-7 / 5.6e-6 / 2.5e-5.  Budget 5e-5.
ATTN_LEVEL = {(3, 6, 8): 1000.0, (32, 50, 512): 200.0, (5, 201, 260): 200.0, (2, 9, 1024): 5000.0}


def dec_rows(s, n):
    """The first n batch rows of a dec_draws() case (rows are independent; the loss then averages over n)."""
    out = dict(s, enc=s["enc"][:n], c0=s["c0"][:, :n], h0=s["h0"][:, :n], y=s["y"][:n])
    out["em"] = None if s["em"] is None else s["em"][:, :n]
    out["rm"] = None if s["rm"] is None else s["rm"][:, :, :n]
    return out


# ------------------------------------------------------------------ defining properties, on float64 restatements of the cases' first steps
def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def dec_step0(s, nl):
    """Step 0 of the decoder loop on a dec_draws() case, float64 NumPy: -> (scores (B, T), logits (B, V), gate pre-activations (nl, B, H, 4))."""
    P = s["P"]
    B = s["enc"].shape[0]
    A = P["context/W"].shape[0]
    e = P["embed_dec/W"][s["y"][:, 0]]
    if s["em"] is not None:
        e = e * s["em"][0]
    x = np.concatenate([e, np.zeros((B, A))], 1)
    zs = []
    for k in range(nl):
        z = (x @ P[f"L{k}_dec/upward/W"].T + P[f"L{k}_dec/upward/b"] + s["h0"][k] @ P[f"L{k}_dec/lateral/W"].T).reshape(B, -1, 4)
        zs.append(z)
        c = np.tanh(z[..., 0]) * _sig(z[..., 1]) + _sig(z[..., 2]) * s["c0"][k]
        x = _sig(z[..., 3]) * np.tanh(c)
        if s["rm"] is not None:
            x = x * s["rm"][k][0]
    q = x @ P["attn_Wa/W"].T + P["attn_Wa/b"]
    scores = np.einsum("bth,bh->bt", s["enc"], q)
    al = np.exp(scores - scores.max(1, keepdims=True))
    al /= al.sum(1, keepdims=True)
    cv = np.einsum("bth,bt->bh", s["enc"], al)
    ht = np.tanh(np.concatenate([cv, x], 1) @ P["context/W"].T + P["context/b"])
    return scores, ht @ P["out/W"].T + P["out/b"], np.stack(zs)


def saturation(z):
    """(share of the i / f / o gate values within 1e-6 of 0 or 1, largest |pre-activation|) of gate pre-activations (..., 4), order a, i, f, o."""
    g = _sig(np.asarray(z, np.float64)[..., 1:])
    return float(((g < 1e-6) | (g > 1 - 1e-6)).mean()), float(np.abs(z).max())


def lstm_preacts(c, nl, masks):
    """Every gate pre-activation of an lstm_draws() case, float64 NumPy, both directions (the reverse one in the reference's order
    0, T - 1, ..., 1): -> array (2 nl T, B, h, 4)."""
    P, x, mk = c["P"], c["x"], c["mk"]
    T = x.shape[0]
    out = []
    for d, pat in enumerate(("L{}_enc", "L{}_rev_enc")):
        xs = x if d == 0 else x[[(-i) % T for i in range(T)]]
        for k in range(nl):
            n = pat.format(k)
            Wu, b, Wl = P[n + "/upward/W"], P[n + "/upward/b"], P[n + "/lateral/W"]
            hdim = Wl.shape[1]
            h, cc, ys = None, np.zeros((x.shape[1], hdim)), []
            for t in range(T):
                z = xs[t] @ Wu.T + b + (0 if h is None else h @ Wl.T)
                z = z.reshape(-1, hdim, 4)
                out.append(z)
                cc = np.tanh(z[..., 0]) * _sig(z[..., 1]) + _sig(z[..., 2]) * cc
                h = _sig(z[..., 3]) * np.tanh(cc)
                ys.append(h if not masks else h * mk[d][k][t])
            xs = np.stack(ys)
    return np.stack(out)


def cnn_layer0_ratio(cfg, P, X, noise):
    """Largest |channel mean| / std of the layer-0 convolution's output (float64): the r of the BatchNorm offset cases."""
    import torch
    l = cfg["cnn_config"]["cnn_layers"][0]
    h = torch.tensor(X * (noise if noise is not None else 1.0)).unsqueeze(1)
    y = torch.nn.functional.conv2d(h, torch.tensor(P["CNN_0/W"]), stride=tuple(l["stride"]), padding=tuple(l["pad"]))
    return float((y.mean(dim=(0, 2, 3)).abs() / y.std(dim=(0, 2, 3), unbiased=False)).max())


def cnn_bn_inputs(cfg, P, X, noise):
    """Per layer, on the float64 reference: (what the layer's BatchNorm sees -- its convolution's output, max-pooled where the layer
    pools -- as (B, C, T_i, F_i), the post-BatchNorm pre-activation of the ReLU), batch statistics throughout."""
    import torch
    TF = torch.nn.functional
    out = []
    with torch.no_grad():
        hh = torch.tensor(X * (noise if noise is not None else 1.0)).unsqueeze(1)
        for i, l in enumerate(cfg["cnn_config"]["cnn_layers"]):
            y = TF.conv2d(hh, torch.tensor(P[f"CNN_{i}/W"]), stride=tuple(l["stride"]), padding=tuple(l["pad"]))
            if "cnn_pool" in cfg["cnn_config"]:
                kt, kf = cfg["cnn_config"]["cnn_pool"][i]
                k = (y.shape[2] if kt == -1 else max(kt, 1), y.shape[3] if kf == -1 else max(kf, 1))
                y = TF.max_pool2d(y, k, stride=k, ceil_mode=True)
            z = TF.batch_norm(y, None, None, torch.tensor(P[f"CNN_{i}_bn/gamma"]), torch.tensor(P[f"CNN_{i}_bn/beta"]), training=True, eps=2e-5)
            out.append((y, z))
            hh = torch.relu(z)
    return out


def cnn_near_kink_layers(cfg, P, X, noise):
    """Per layer, the units whose post-BatchNorm pre-activation lies within 2e-5 of the ReLU's kink on the float64 reference (the operator
    test's near-kink rule), each as a bool tensor (B, C, T_i, F_i)."""
    return [z.abs() < 2e-5 for _, z in cnn_bn_inputs(cfg, P, X, noise)]


def seq_layout(a):
    """(B, C, T'', F') -> the output's (T'', B, C F') layout, feature index c F' + f."""
    Bc, Cc, T2, F2 = a.shape
    return a.permute(2, 0, 1, 3).reshape(T2, Bc, Cc * F2)


def cnn_near_kink(cfg, P, X, noise):
    """The near-kink units of layer 0 as (B, C, T', F) and of the last layer in the output's (T'', B, C F') layout."""
    near = cnn_near_kink_layers(cfg, P, X, noise)
    return near[0].numpy(), seq_layout(near[-1]).numpy()


def attn_upstream(B, T, H):
    return np.random.default_rng(B * T + 1).standard_normal((B, H)).astype(np.float32)


def assert_score_ranges(rng, H):
    """The condition of the wide-score decoder cases on the reference's step-0 score ranges (one per row): every row at least 88 (where
    exp(s - max) underflows in float32) on the shapes with H >= 512, some row above 60 on the narrower ones."""
    if H >= 512:
        assert rng.min() >= 88, rng.min()
    else:
        assert rng.max() > 60, rng.max()
