"""Float32-level accuracy gates for the encoder recurrences (ast_amd/csrc/lstm_persist.hip), shared by tests/test_recurrence_accuracy_host.py
(CPU) and tests/test_gpu_recurrence_accuracy.py (MI355X).  A helper, not a test module: nothing here touches a GPU.

lstm_persist.hip multiplies with split-operand MFMA code of its own -- the lateral and upward products of the forward recurrence, the
recurrent and down products of the backward one -- in four arithmetic forms (f32 MFMAs; fp16x2; bf16x3 with hi / mid / lo planes in
registers; bf16x3 with the weights' lo plane in LDS) and three workgroup forms (16 rows; MT 2; DUO).  Every other test that runs them ends
in close() at 2e-4 / 5e-4 of a tensor's largest entry, where float32 arithmetic sits at 3e-7: a kernel may lose everything below the mid
plane of bf16x3 and pass.  This file holds what closes that gap.

CASES: one row per instantiation (width, workgroup form, arithmetic), at the smallest shapes at which it can still go wrong (cases()).

Inputs: range_cases.lstm_draws with every array rounded to float32 first: the reference and the kernels see the same numbers.

Reference: run(), a BiLSTM stack forward and backward in torch autograd, float64; tests/test_recurrence_accuracy_host.py holds it to 1e-12 of
oracle.ast_ref_torch.encoder_torch.  The same function is (a) the plain float32 evaluation (dtype = torch.float32: every operation rounded
to float32, torch's summation order, a weight gradient summed over all steps in one product as the library sums it) and (b, c) the mutants: per product family -- "lateral" and "upward" (layers >= 1; the layer-0 input
projection is gemm.hip's) -- a Pass for the forward product and one for its backward twin (recurrent: dz Wl; down: dz Wu) says which weight
values the product multiplies, what becomes of the activation operand (the previous output, the input from below; dz backward), and which
plane-by-plane term products are missing.  The weight GRADIENTS are batched products behind the recurrence (gemm.hip): always exact.

Error gate, per case and per slice (enc_states per direction half; cT, hT per (direction, layer); dx; every gradient tensor): max |got - ref|
over the slice's largest |ref| <= TOL[kind], kind in state / dx / dW / db.  TOL[kind] is the smallest {1, 2, 5} x 10^k for which the float32
evaluation stays within a QUARTER of it on every case (the standing margin of row_panel_model.TOL and ctc_model.F32_MODEL_ERR: it covers
another summation order and the kernels' fast exp / reciprocal in the gates); the host test asserts that.  Worst figures over all cases:

    kind    float32 model   tolerance
    state   3.30e-7         2e-6
    dx      5.52e-7         5e-6
    dW      5.86e-7         5e-6
    db      2.63e-7         2e-6

(DESIGN.md has them beside what the kernels measured on an MI355X.)
fp16x2: lstm_persist.hip documents 2^-22 per product for that form against 2^-24 (f32) and 2^-26 (bf16x3) for the others, so the fp16x2
cases are held to FP16X2_FACTOR = 4 x TOL.

Projection gates.  The lowest bf16 plane of an operand is worth 2^-17 of it: 2^7 float32 ulps in a product term, but after accumulation over K
and the recurrence it moves the outputs by 2 ... 18 x the float32 evaluation's own error, dx by 2 ... 4 x -- not separated by a margin of 4 on
every tensor.  What separates it is the DIRECTION in which a lost plane moves the outputs: p = model(mutant) - reference in float64, every
slice divided by its largest reference entry and the slices concatenated; for a result `got`, c = <got - ref, p> / <p, p>.  A kernel that
loses the plane has c = 1 by construction, float32 rounding noise is not aligned with p (the host test: |c| <= C_F32_MAX for the float32
evaluation), and the gate is |c| <= C_GATE.  Directions (directions()): bf16x3 -- the lo plane zeroed in one gate's rows of the lateral or of
the upward weights, forward product only (8, seen on the forward outputs), backward product only (8, seen on dx and the gradients), and
the lo plane of the activation operand zeroed per product (4); fp16x2 -- the same with fp16's lo plane (an operand rounded to 11 significant
bits: hi behind the documented power-of-two scales), the four gates together.  At h = 1024 (the hoisted form) the upward and down products
are batched products of gemm.hip between the launches: that case has the lateral family's directions only.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import range_cases

# ------------------------------------------------------------------ what the library names (include/astk.h, lstm_persist.h)
PREC = {"bf16x3": 2, "f32": 3, "fp16x2": 1}                         # ASTK_PREC_*
ROWS_16, ROWS_MT2, ROWS_DUO = 16, 32, 33                           # astk_lstm_stack_form: *rows
XS_F32, XS_FP16X2, XS_BF16X3, XS_BF16X3_LDS = 0, 2, 3, 4           # ... *xs
ROWS32_KNOB = {ROWS_16: 0, ROWS_MT2: 1, ROWS_DUO: 2}               # "lstm.rows32"

KINDS = ("state", "dx", "dW", "db")
# worst error of the plain float32 evaluation over all cases (test_float32_model_error_is_what_the_tolerances_were_taken_from prints them)
F32_MODEL_ERR = {"state": 3.30e-7, "dx": 5.52e-7, "dW": 5.86e-7, "db": 2.63e-7}
TOL = {"state": 2e-6, "dx": 5e-6, "dW": 5e-6, "db": 2e-6}
FP16X2_FACTOR = 4.0           # 2^-22 per product (lstm_persist.hip) against 2^-24
C_GATE = 0.25                 # |c| of a device result on every direction of its scheme
C_F32_MAX = 0.1               # |c| of the float32 evaluation (host test)

Case = namedtuple("Case", "T B in_dim h layers masks form scheme")


def cases():
    """16 rows at every width: h <= 256 with 17 batch rows (a full tile and a one-row ragged one), h >= 512 with 5; 5 steps (step 0 is peeled,
    a steady loop, the last two steps with clamped prefetch indices); 2 layers (a cell without and one with an upward product); dropout
    masks at h = 128 and 512.  MT 2 and DUO (bf16x3 only) at h <= 256 with 33 rows: two workgroup rows for MT 2, the second with one batch
    row; four virtual rows for DUO, the last without batch rows.  One 2-step case (the backward's last step has nothing left to fetch)."""
    out = []
    for scheme in ("bf16x3", "f32", "fp16x2"):
        for h in (64, 128, 256, 512, 1024):
            out.append(Case(5, 17 if h <= 256 else 5, 16, h, 2, h in (128, 512), ROWS_16, scheme))
        for h in (64, 128, 256):
            out.append(Case(5, 33, 16, h, 2, h == 128, ROWS_MT2, scheme))
    for h in (64, 128, 256):
        out.append(Case(5, 33, 16, h, 2, h == 128, ROWS_DUO, "bf16x3"))
    out.append(Case(2, 17, 16, 128, 2, True, ROWS_16, "bf16x3"))
    assert len(out) == 28 and len(set(out)) == 28
    return out


def case_id(c):
    return f"T{c.T}-B{c.B}-h{c.h}{'-masks' if c.masks else ''}-rows{c.form}-{c.scheme}"


def shape_of(c):
    return tuple(c[:6])


def shapes():
    """The distinct (T, B, in_dim, h, layers, masks) of the cases: the reference and the directions depend on nothing else."""
    seen = []
    for c in cases():
        if shape_of(c) not in seen:
            seen.append(shape_of(c))
    return seen


def expected_launch(c):
    """(astk_lstm_stack_path, *rows, *xs of astk_lstm_stack_form) a case must report."""
    xs = {"f32": XS_F32, "fp16x2": XS_FP16X2}.get(c.scheme)
    if xs is None:
        xs = XS_BF16X3_LDS if (c.h >= 512 or c.form == ROWS_DUO) else XS_BF16X3
    return (2 if c.h == 1024 else 1), c.form, xs


@functools.lru_cache(maxsize=None)
def draws(shape):
    """range_cases.lstm_draws of the shape, every array rounded to float32 (kept as float32 arrays)."""
    T, B, in_dim, h, nl, masks = shape
    d = range_cases.lstm_draws(T, B, in_dim, h, nl, masks)
    f = lambda a: None if a is None else np.asarray(a).astype(np.float32)
    return dict(P={k: f(v) for k, v in d["P"].items()}, names=d["names"], x=f(d["x"]), mk=f(d["mk"]),
                g_enc=f(d["g_enc"]), g_c=f(d["g_c"]), g_h=f(d["g_h"]))


# ------------------------------------------------------------------ planes
def bf16_planes(v):
    """(hi, mid, lo) of common.h split2b: three bf16 terms of the float32 value, round-to-nearest-even each; in v's dtype."""
    v32 = v.detach().float()
    hi = v32.bfloat16().float()
    mid = (v32 - hi).bfloat16().float()
    lo = (v32 - hi - mid).bfloat16().float()
    return hi.to(v.dtype), mid.to(v.dtype), lo.to(v.dtype)


def fp16_planes(v):
    """(hi, lo) of the fp16x2 split behind a power-of-two scale: hi = the value rounded to fp16's 11 significant bits (the scales keep
    every operand of these cases inside fp16's normal range, so the scale itself drops out), lo = what is left, rounded likewise."""
    def r11(t):
        m, e = torch.frexp(t)
        return torch.ldexp(torch.round(m * 2048.0) / 2048.0, e)
    v32 = v.detach().float()
    hi = r11(v32)
    return hi.to(v.dtype), r11(v32 - hi).to(v.dtype)


def plane(v, name):
    if name in ("hi", "mid", "lo"):
        return bf16_planes(v)[("hi", "mid", "lo").index(name)]
    return fp16_planes(v)[("hi16", "lo16").index(name)]


def gate_rows(t, g):
    """t with everything but gate g's rows (4 j + g: the interleaved layout) zeroed; g = None: all of t."""
    if g is None:
        return t
    out = torch.zeros_like(t)
    out[g::4] = t[g::4]
    return out


def without(name, g=None):
    """Operand -> the operand with plane `name` removed (in gate g's rows only, for a weight)."""
    return lambda t: t.detach() - gate_rows(plane(t, name), g)


def garbage_lo(t):
    """A weight whose lo plane comes from the row above (another gate's, another thread's slot)."""
    lo = plane(t, "lo")
    return t.detach() - lo + torch.roll(lo, 1, 0)


# ------------------------------------------------------------------ the model
class Pass:
    """One product of a family in one direction of the pass.  W: weights -> the values multiplied; act: the same for the activation
    operand; drop: [(activation plane, weight plane)] term products left out.  (What is derived from a weight is formed once per run().)"""

    def __init__(self, W=None, act=None, drop=()):
        self.W, self.act, self.drop = W, act, tuple(drop)
        self.derived = {}

    def of_weight(self, w, what):
        """The multiplied values (what = "W") or a plane of the weight tensor w, kept for the steps of one run."""
        key = (id(w), what)
        if key not in self.derived:
            self.derived[key] = (w if self.W is None else self.W(w)) if what == "W" else plane(w, what)
        return self.derived[key]


def _apply(a, w, p, fwd):
    """a w^T (fwd) or a w (backward twin: a = the incoming gradient) under Pass p, in a's dtype."""
    if p is None:
        return a @ (w.t() if fwd else w)
    wv = p.of_weight(w, "W")
    av = a if p.act is None else p.act(a)
    y = av @ (wv.t() if fwd else wv)
    for pa, pw in p.drop:
        y = y - plane(a, pa) @ (p.of_weight(w, pw).t() if fwd else p.of_weight(w, pw))
    return y


class Product(torch.autograd.Function):
    """y = x w^T (x: (B, K), w: (N, K)) with one Pass for the forward product and one for the input gradient.  The weight gradient is exact
    and is not formed step by step: the (incoming gradient, x) pairs go on `tape`, and run() multiplies them once per weight, as the
    library does behind the recurrence."""

    @staticmethod
    def forward(ctx, x, w, fam, tape):
        ctx.fam, ctx.tape = fam, tape
        ctx.save_for_backward(x, w)
        return _apply(x, w, fam[0], True)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        ctx.tape.append((g, x))
        return _apply(g, w, ctx.fam[1], False), None, None, None


def _product(x, w, fam, tapes):
    return Product.apply(x, w, fam or (None, None), tapes.setdefault(id(w), (w, []))[1])


def _lstm_run(x_seq, Wu, b, Wl, masks, layer, spec, tapes):
    """One direction's layer, x_seq (n, B, in) in consumption order (oracle.ast_ref_torch._lstm_run with the two product hooks)."""
    n, B, _ = x_seq.shape
    hdim = Wl.shape[1]
    up = spec.get("upward") if layer > 0 else None
    zx = (x_seq @ Wu.t() if up is None else torch.stack([_product(x_seq[t], Wu, up, tapes) for t in range(n)])) + b
    h, c, outs = None, torch.zeros(B, hdim, dtype=x_seq.dtype), []
    for t in range(n):
        z = zx[t] if h is None else zx[t] + _product(h, Wl, spec.get("lateral"), tapes)
        z = z.view(B, hdim, 4)
        a, i, f, o = torch.tanh(z[..., 0]), torch.sigmoid(z[..., 1]), torch.sigmoid(z[..., 2]), torch.sigmoid(z[..., 3])
        c = a * i + f * c
        h = o * torch.tanh(c)
        outs.append(h if masks is None else h * masks[t])
    return torch.stack(outs, 0), c, h


def run(shape, dtype=torch.float64, spec=None):
    """Forward and backward of the stack on draws(shape) -> {enc_states (B, T, 2h), cT, hT (2, layers, B, h), dx (T, B, in), "grad <name>"} as
    float64 arrays.  spec: {"lateral" / "upward": (forward Pass or None, backward Pass or None)}; None: every product as it is."""
    T, B, in_dim, h, nl, masks = shape
    d, spec = draws(shape), (spec or {})
    for fam in spec.values():
        for p in fam:
            if p is not None:
                p.derived = {}
    P = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in d["P"].items()}
    x = torch.tensor(d["x"], dtype=dtype, requires_grad=True)
    mk = torch.tensor(d["mk"], dtype=dtype) if masks else None
    seqs = [x, x[[(-i) % T for i in range(T)]]]                 # quirk Q1: the reverse stack reads frames 0, T - 1, ..., 1
    cT, hT, tapes = [[], []], [[], []], {}
    for k in range(nl):
        for dd, pat in enumerate(("L{}_enc", "L{}_rev_enc")):
            n = pat.format(k)
            seqs[dd], cf, hf = _lstm_run(seqs[dd], P[n + "/upward/W"], P[n + "/upward/b"], P[n + "/lateral/W"],
                                         mk[dd][k] if masks else None, k, spec, tapes)
            cT[dd].append(cf)
            hT[dd].append(hf)
    enc = torch.cat([seqs[0], torch.flip(seqs[1], [0])], 2).transpose(0, 1)
    cT, hT = (torch.stack([torch.stack(s[0]), torch.stack(s[1])]) for s in (cT, hT))
    up = [torch.tensor(d[k], dtype=dtype) for k in ("g_enc", "g_c", "g_h")]
    ((enc * up[0]).sum() + (cT * up[1]).sum() + (hT * up[2]).sum()).backward()
    for w, tape in tapes.values():                               # the taped weight gradients: sum over the steps of g^T x, one product
        dw = torch.cat([g for g, _ in tape]).t() @ torch.cat([xx for _, xx in tape])
        w.grad = dw if w.grad is None else w.grad + dw
    out = {"enc_states": enc, "cT": cT, "hT": hT, "dx": x.grad}
    out.update({"grad " + k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in P.items()})
    return {k: v.detach().double().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(shape):
    return run(shape)


# ------------------------------------------------------------------ slices and the two gates
def slices(out, shape):
    """[(name, kind, array)] of a result of run() (or of the device call, named alike)."""
    h, nl = shape[3], shape[4]
    res = [(f"enc_states[dir {dd}]", "state", out["enc_states"][:, :, dd * h:(dd + 1) * h]) for dd in range(2)]
    for k in ("cT", "hT"):
        res += [(f"{k}[dir {dd}][layer {l}]", "state", out[k][dd, l]) for dd in range(2) for l in range(nl)]
    res.append(("dx", "dx", out["dx"]))
    for k in sorted(out):
        if k.startswith("grad "):
            res.append((k, "dW" if k.endswith("/W") else "db", out[k]))
    return res


def slice_errors(got, shape):
    """[(name, kind, max |got - ref| over the slice's largest |ref|)] against reference(shape)."""
    ref = reference(shape)
    out = []
    for (name, kind, g), (_, _, r) in zip(slices(got, shape), slices(ref, shape)):
        assert g.shape == r.shape, (name, g.shape, r.shape)
        out.append((name, kind, float(np.abs(np.asarray(g, np.float64) - r).max() / np.abs(r).max())))
    return out


def worst_by_kind(errs):
    return {kind: max(e for _, k, e in errs if k == kind) for kind in KINDS}


def tolerance(c, kind):
    return TOL[kind] * (FP16X2_FACTOR if c.scheme == "fp16x2" else 1.0)


def smallest_125(x):
    """The smallest of {1, 2, 5} x 10^k that is >= x."""
    k = int(np.floor(np.log10(x)))
    for m in (1, 2, 5, 10):
        if m * 10.0 ** k >= x * (1 - 1e-12):
            return m * 10.0 ** k


def displacement(out, shape, side):
    """out - reference over the slices of one side ("fwd": the state slices; "bwd": dx and the gradients), each slice over its largest
    reference entry, concatenated.  Formed in float64, kept in float32 (25 M entries on the backward side at h = 1024)."""
    ref = reference(shape)
    parts = []
    for (_, kind, g), (_, _, r) in zip(slices(out, shape), slices(ref, shape)):
        if (kind == "state") == (side == "fwd"):
            parts.append(((np.asarray(g, np.float64) - r) / np.abs(r).max()).astype(np.float32).ravel())
    return np.concatenate(parts)


def _dot(a, b):
    return float(np.dot(a, b))


Direction = namedtuple("Direction", "name side spec")


def directions(scheme, hoisted=False):
    """The mutants whose displacement of the outputs a device result must not contain.  Forward mutants are seen on the forward outputs,
    backward-only ones (the forward pass runs exact) on dx and the gradients.  hoisted (h = 1024): the upward and down products are batched
    products of gemm.hip between the launches there, not the recurrence kernels': the lateral family's directions only."""
    out = []
    fams = (("lateral", "recurrent"), ("upward", "down"))[:1 if hoisted else 2]
    if scheme == "bf16x3":
        for fam, twin in fams:
            for g in range(4):
                out.append(Direction(f"fwd {fam} weights lo, gate {g}", "fwd", {fam: (Pass(W=without("lo", g)), None)}))
                out.append(Direction(f"bwd {twin} weights lo, gate {g}", "bwd", {fam: (None, Pass(W=without("lo", g)))}))
            out.append(Direction(f"fwd {fam} activations lo", "fwd", {fam: (Pass(act=without("lo")), None)}))
            out.append(Direction(f"bwd {twin} dz lo", "bwd", {fam: (None, Pass(act=without("lo")))}))
    elif scheme == "fp16x2":
        for fam, twin in fams:
            out.append(Direction(f"fwd {fam} weights lo16", "fwd", {fam: (Pass(W=without("lo16")), None)}))
            out.append(Direction(f"bwd {twin} weights lo16", "bwd", {fam: (None, Pass(W=without("lo16")))}))
            out.append(Direction(f"fwd {fam} activations lo16", "fwd", {fam: (Pass(act=without("lo16")), None)}))
            out.append(Direction(f"bwd {twin} dz lo16", "bwd", {fam: (None, Pass(act=without("lo16")))}))
    return out


@functools.lru_cache(maxsize=None)
def direction_vectors(shape, scheme):
    """[(Direction, p)]: p = displacement(model(mutant)), the model in float64."""
    return [(d, displacement(run(shape, spec=d.spec), shape, d.side)) for d in directions(scheme, hoisted=shape[3] >= 1024)]


def coefficients(got, shape, scheme):
    """[(direction name, c)] of a result: c = <got - ref, p> / <p, p>."""
    diff = {side: displacement(got, shape, side) for side in ("fwd", "bwd")}
    return [(d.name, _dot(diff[d.side], p) / _dot(p, p)) for d, p in direction_vectors(shape, scheme)]


# ------------------------------------------------------------------ mutants for the error gate's power (host test)
SIX_TERMS = (("lo", "hi"), ("hi", "lo"), ("mid", "mid"), ("mid", "hi"), ("hi", "mid"), ("hi", "hi"))      # (activation, weight): fwd_gate_products


def error_gate_mutants():
    """name -> (spec, exceeds TOL on every state slice of every bf16x3 shape).  Forward lateral product throughout.  The lowest plane's
    mutants move the state slices by 0.2 ... 1.9 x TOL (garbage lo: 0.3 ... 1.9, above 1 on seven shapes of nine): the projection
    gate's, not the error gate's."""
    return {"mid plane of the weights lost": ({"lateral": (Pass(W=without("mid")), None)}, True),
            "term product mid x hi missing": ({"lateral": (Pass(drop=[("mid", "hi")]), None)}, True),
            "garbage lo plane (rolled by one row)": ({"lateral": (Pass(W=garbage_lo), None)}, False),
            "lo plane of the weights lost": ({"lateral": (Pass(W=without("lo")), None)}, False),
            "term product lo x hi missing": ({"lateral": (Pass(drop=[("lo", "hi")]), None)}, False)}
