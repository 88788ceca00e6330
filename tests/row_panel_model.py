"""The three row-panel operations of ast_amd/csrc/rowgemm.hip restated over dense NumPy arrays, from the struct comments of
ast_amd/csrc/common.h (RowGemmArgs, LstmCellFwdArgs, LstmCellBwdArgs).  A helper, not a test module: it imports no GPU code.
tests/test_row_panel_host.py derives the GPU tolerances from it, tests/test_gpu_row_panel.py compares the kernels with it through the
astk_debug_rowgemm / astk_debug_lstm_cell_fwd / astk_debug_lstm_cell_bwd hooks of libastk_test.so.

    rowgemm       v = sum_p A_p W_p^T (+ bias[n]) (+ addend[r][n]);  v = tanh(v) when act = 1;  out = out2 = v;
                  for n >= carry_col0, j = n - carry_col0:  carry[r][j] = (v[r][n] + carry[r][j]) * (1 - aux[r][j]^2)
    forward cell  z = sum_p A_p W_p^T (+ zx) (+ bias), W_p rows interleaved: row 4j + k is gate k of unit j, k = a, i, f, o;
                  a = tanh, i, f, o = sigmoid;  c = a i + f c_prev (c_prev null: zeros);  h = o tanh(c);
                  gates = (a, i, f, o) interleaved;  hd = hd2 = h * mask (the mask touches the dropped outputs only)
    backward cell dh_rec = A_0 W_0^T;  dy = (A_1 W_1^T + dy + dy2) * mask;  dh = dh_rec + dy + dh_add (dh_add NOT masked);
                  tc = tanh(c_cur);  dc = dh o (1 - tc^2) + dc_next;
                  dz = (dc i (1 - a^2), dc a i (1 - i), dc c_prev f (1 - f), dh tc o (1 - o)) written over the gates;  dc_prev = dc f

dtype = float64 is the reference.  dtype = float32 is the plain float32 evaluation: every operation rounded to float32, the K sum
either in index order (`waves` = None) or the way the kernels split it: k-block s (16 consecutive k) goes to wave s mod NW, each wave
sums its blocks in order -- over both pairs where the pairs share an accumulator (rowgemm, the forward cell) -- and the NW partial sums
are added in wave order.  The host test takes the worse of the two.

Tolerances, relative to the largest magnitude of the reference tensor of the case (tests/test_gpu_ops.py close()).  Each is the smallest
{1, 2, 5} x 10^k for which the float32 evaluation stays within a QUARTER of it on every case of cases() (tests/test_row_panel_host.py
asserts that, and that every mutant below misses at least one).  Worst figures over all cases (the last column: the kernels on an
MI355X, tests/test_gpu_row_panel.py, 256 compute units):

    quantity   float32 model   tolerance   MI355X
    out        2.24e-6         1e-5        1.34e-6
    out2       5.05e-7         5e-6        3.28e-7
    carry      4.44e-7         2e-6        1.60e-7
    gates      2.89e-6         2e-5        5.29e-7
    c          1.10e-6         5e-6        2.88e-7
    h          1.19e-6         5e-6        4.00e-7
    hd         1.20e-6         5e-6        4.04e-7
    dz         1.51e-6         1e-5        3.08e-7
    dc_prev    1.40e-6         1e-5        4.21e-7
"""
import zlib

import numpy as np

TOL = {"out": 1e-5, "out2": 5e-6, "carry": 2e-6, "gates": 2e-5, "c": 5e-6, "h": 5e-6, "hd": 5e-6, "dz": 1e-5, "dc_prev": 1e-5}

LONGK_DEFAULT = 2048          # the row.longk knob's default (include/astk.h)
KEEP = 1.0 / 0.7              # scaled keep-mask value at dropout 0.3

MUTANTS = {
    # name: (operation, what a case needs for the mutant to show)
    "carry_from_col0_plus_1": ("rowgemm", lambda s: s["carry_col0"] is not None),
    "carry_without_old": ("rowgemm", lambda s: s["carry_col0"] is not None),
    "bias_after_act": ("rowgemm", lambda s: s["bias"] and s["act"]),
    "out2_before_act": ("rowgemm", lambda s: s["out2"] and s["act"]),
    "gate_order_iafo": ("fwd", lambda s: True),
    "mask_on_h_out": ("fwd", lambda s: s["mask"]),
    "mask_on_dh_rec": ("bwd", lambda s: s["mask"] and s["Ks"][0] > 0),
    "dh_add_masked": ("bwd", lambda s: s["mask"] and s["dh_add"]),
    "dy2_dropped": ("bwd", lambda s: s["dy2"]),
    "dc_prev_without_gf": ("bwd", lambda s: True),
    "pair1_into_dh_rec": ("bwd", lambda s: s["mask"] and len(s["Ks"]) > 1 and s["Ks"][1] > 0),
}


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------ the route (rowgemm.hip row_route, restated)
def route_key(kind, spec):
    """(column tiles, rows, cells, the K the kernel is keyed on): sum over the pairs for rowgemm and the forward cell, maximum for the
    backward cell."""
    ks = [k for k in spec["Ks"]]
    if kind == "rowgemm":
        return cdiv(spec["N"], 16), spec["M"], 1, sum(ks)
    if kind == "fwd":
        return cdiv(spec["h"], 4), spec["B"], spec["ncells"], sum(ks)
    return cdiv(spec["h"], 16), spec["B"], spec["ncells"], max(ks)


def route(kind, spec, cu):
    """What the hook must report: [bit 0 two row tiles | bit 1 eight waves, grid x, y, z]."""
    tiles, rows, cells, k = route_key(kind, spec)
    longk = LONGK_DEFAULT if spec["longk"] is None else spec["longk"]
    two = rows > 16 and tiles * cdiv(rows, 32) * cells >= cu
    eight = longk > 0 and k >= longk
    return [int(two) | int(eight) << 1, tiles, cdiv(rows, 32 if two else 16), cells]


def instantiation(kind, spec, cu):
    bits = route(kind, spec, cu)[0]
    return kind, 2 if bits & 1 else 1, 8 if bits & 2 else 4


# ------------------------------------------------------------------ arithmetic
def _dot(pairs, dtype, waves=None):
    """sum_p A_p W_p^T over the pairs with K > 0 (None: no pair contributes)."""
    pairs = [(A, W) for A, W in pairs if A is not None and A.shape[1] > 0]
    if not pairs:
        return None
    if dtype == np.float64:
        return sum(A.astype(np.float64) @ W.astype(np.float64).T for A, W in pairs)
    M, N = pairs[0][0].shape[0], pairs[0][1].shape[0]
    acc = np.zeros((waves or 1, M, N), np.float32)
    for A, W in pairs:
        A, W = np.asarray(A, np.float32), np.asarray(W, np.float32)
        for k in range(A.shape[1]):
            w = (k // 16) % waves if waves else 0
            acc[w] += A[:, k, None] * W[None, :, k]
    total = acc[0]
    for w in range(1, acc.shape[0]):
        total = total + acc[w]
    assert total.dtype == np.float32
    return total


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _cast(x, dtype):
    return None if x is None else np.asarray(x).astype(dtype)


def rowgemm(inp, dtype=np.float64, waves=None, mutant=None):
    """{out, out2?, carry?} of one launch.  inp: pairs [(A, W)], bias, addend, act, out2 (bool), carry, aux, carry_col0."""
    v = _dot(inp["pairs"], dtype, waves)
    bias, addend = _cast(inp.get("bias"), dtype), _cast(inp.get("addend"), dtype)
    late_bias = mutant == "bias_after_act" and bias is not None
    if bias is not None and not late_bias:
        v = v + bias[None, :]
    if addend is not None:
        v = v + addend
    pre = v
    if inp.get("act"):
        v = np.tanh(v)
    if late_bias:
        v = v + bias[None, :]
    res = {"out": v}
    if inp.get("out2"):
        res["out2"] = pre if mutant == "out2_before_act" else v
    if inp.get("carry") is not None:
        c0 = inp["carry_col0"]
        old, y = _cast(inp["carry"], dtype), _cast(inp["aux"], dtype)
        new = ((v[:, c0:] if mutant == "carry_without_old" else v[:, c0:] + old)) * (1.0 - y * y)
        if mutant == "carry_from_col0_plus_1":
            new[:, 0] = old[:, 0]
        res["carry"] = new
    assert all(a.dtype == dtype for a in res.values())
    return res


def cell_fwd(inp, dtype=np.float64, waves=None, mutant=None):
    """{gates, c, h, hd?} of one cell.  inp: pairs, zx, bias, c_prev, mask, hd (bool: any dropped destination)."""
    B, h = inp["B"], inp["h"]
    z = _dot(inp["pairs"], dtype, waves)
    if z is None:
        z = np.zeros((B, 4 * h), dtype)
    for add in (_cast(inp.get("zx"), dtype), _cast(inp.get("bias"), dtype)):
        if add is not None:
            z = z + (add if add.ndim == 2 else add[None, :])
    r = z.reshape(B, h, 4)
    ka, ki = (1, 0) if mutant == "gate_order_iafo" else (0, 1)
    a, i, f, o = np.tanh(r[:, :, ka]), _sigmoid(r[:, :, ki]), _sigmoid(r[:, :, 2]), _sigmoid(r[:, :, 3])
    cp = _cast(inp.get("c_prev"), dtype)
    c = a * i + (f * cp if cp is not None else 0.0)
    hh = o * np.tanh(c)
    mask = _cast(inp.get("mask"), dtype)
    hd = hh * mask if mask is not None else hh
    res = {"gates": np.stack([a, i, f, o], axis=2).reshape(B, 4 * h), "c": c, "h": hd if mutant == "mask_on_h_out" else hh}
    if inp.get("hd"):
        res["hd"] = hd
    assert all(x.dtype == dtype for x in res.values())
    return res


def cell_bwd(inp, dtype=np.float64, waves=None, mutant=None):
    """{dz, dc_prev} of one cell.  inp: pairs (1 or 2), dy, dy2, dh_add, mask, dc_next, c_prev, c_cur, gates."""
    B, h = inp["B"], inp["h"]
    zero = np.zeros((B, h), dtype)
    v0 = _dot(inp["pairs"][:1], dtype, waves)
    v1 = _dot(inp["pairs"][1:2], dtype, waves)
    v0 = zero if v0 is None else v0
    v1 = zero if v1 is None else v1
    if mutant == "pair1_into_dh_rec":
        v0, v1 = v0 + v1, zero
    dy = v1
    for name in ("dy", "dy2"):
        x = _cast(inp.get(name), dtype)
        if x is not None and not (name == "dy2" and mutant == "dy2_dropped"):
            dy = dy + x
    mask = _cast(inp.get("mask"), dtype)
    if mask is not None:
        dy = dy * mask
        if mutant == "mask_on_dh_rec":
            v0 = v0 * mask
    dh = v0 + dy
    dh_add = _cast(inp.get("dh_add"), dtype)
    if dh_add is not None:
        dh = dh + (dh_add * mask if mutant == "dh_add_masked" and mask is not None else dh_add)
    g = _cast(inp["gates"], dtype).reshape(B, h, 4)
    ga, gi, gf, go = g[:, :, 0], g[:, :, 1], g[:, :, 2], g[:, :, 3]
    tc = np.tanh(_cast(inp["c_cur"], dtype))
    cp = _cast(inp.get("c_prev"), dtype)
    dc = dh * go * (1.0 - tc * tc)
    dc_next = _cast(inp.get("dc_next"), dtype)
    if dc_next is not None:
        dc = dc + dc_next
    dz = np.stack([dc * gi * (1.0 - ga * ga), dc * ga * gi * (1.0 - gi), (dc * cp if cp is not None else zero) * gf * (1.0 - gf),
                   dh * tc * go * (1.0 - go)], axis=2).reshape(B, 4 * h)
    res = {"dz": dz, "dc_prev": dc if mutant == "dc_prev_without_gf" else dc * gf}
    assert all(x.dtype == dtype for x in res.values())
    return res


OPS = {"rowgemm": rowgemm, "fwd": cell_fwd, "bwd": cell_bwd}


def relerr(got, ref):
    """max |got - ref| relative to max |ref| (floored at 1e-6, as close() floors it)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)) if ref.size else 0.0


# ------------------------------------------------------------------ cases
class Case:
    """One launch: `kind`, a unique `name`, the test `group` it runs in and the spec.  inputs(): one dict per cell (one for rowgemm) of dense
    float32 arrays, drawn from a standard normal and scaled by 1 / sqrt(summed K) where they feed a tanh or a sigmoid."""

    def __init__(self, kind, group, name, **spec):
        self.kind, self.group, self.name, self.spec = kind, group, f"{kind}/{name}", spec
        self._inp = self._ref = None

    def __repr__(self):
        return self.name

    def inputs(self):
        if self._inp is None:
            n = self.spec.get("ncells", 1)
            self._inp = [_DRAW[self.kind](self.spec, np.random.default_rng([zlib.crc32(self.name.encode()), i])) for i in range(n)]
        return self._inp

    def run(self, dtype=np.float64, waves=None, mutant=None):
        if dtype == np.float64 and mutant is None:
            if self._ref is None:
                self._ref = [OPS[self.kind](inp) for inp in self.inputs()]
            return self._ref
        return [OPS[self.kind](inp, dtype, waves, mutant) for inp in self.inputs()]

    def waves(self, cu):
        return instantiation(self.kind, self.spec, cu)[2]


def _normal(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _pairs(rng, rows, cols, Ks, scale):
    return [(_normal(rng, rows, K), _normal(rng, cols, K, scale=scale)) if K > 0 else (None, None) for K in Ks]


def _mask(rng, B, h):
    m = np.where(rng.random((B, h)) < 0.7, KEEP, 0.0).astype(np.float32)
    if m.size >= 2:                                  # both values present, so that the mask is never the identity or all zero
        m.flat[0], m.flat[-1] = 0.0, KEEP
    return m


def _draw_rowgemm(s, rng):
    M, N, ktot = s["M"], s["N"], max(sum(s["Ks"]), 1)
    inp = dict(pairs=_pairs(rng, M, N, s["Ks"], 1.0 / np.sqrt(ktot) if s["act"] else 1.0), act=s["act"], out2=s["out2"])
    if s["bias"]:
        inp["bias"] = _normal(rng, N)
    if s["addend"]:
        inp["addend"] = _normal(rng, M, N)
    if s["carry_col0"] is not None:
        w = N - s["carry_col0"]
        inp["carry_col0"] = s["carry_col0"]
        inp["carry"] = _normal(rng, M, w) + np.float32(3.0)                     # an old value that is never near zero
        inp["aux"] = np.clip(np.tanh(_normal(rng, M, w)), -0.9, 0.9).astype(np.float32)
        inp["aux"] = np.where(np.abs(inp["aux"]) < 0.1, np.float32(0.5), inp["aux"])     # a tanh output away from 0
    return inp


def _draw_fwd(s, rng):
    B, h, ktot = s["B"], s["h"], max(sum(s["Ks"]), 1)
    inp = dict(B=B, h=h, pairs=_pairs(rng, B, 4 * h, s["Ks"], 1.0 / np.sqrt(ktot)), hd=s["hd"] or s["hd2"])
    if s["zx"]:
        inp["zx"] = _normal(rng, B, 4 * h)
        if s["saturate"]:                            # pre-activations at +-30 and +-100 (the product adds a unit-variance term)
            inp["zx"] = rng.choice(np.array([-100.0, -30.0, 30.0, 100.0], np.float32), size=(B, 4 * h))
    if s["bias"]:
        inp["bias"] = _normal(rng, 4 * h)
    if s["c_prev"]:
        inp["c_prev"] = _normal(rng, B, h)
    if s["mask"]:
        inp["mask"] = _mask(rng, B, h)
    return inp


def _draw_bwd(s, rng):
    B, h = s["B"], s["h"]
    inp = dict(B=B, h=h, pairs=_pairs(rng, B, h, s["Ks"], 1.0))
    for name in ("dy", "dy2", "dh_add", "dc_next", "c_prev"):
        if s[name]:
            inp[name] = _normal(rng, B, h)
    if s["mask"]:
        inp["mask"] = _mask(rng, B, h)
    inp["c_cur"] = _normal(rng, B, h)
    z = rng.standard_normal((B, h, 4))
    inp["gates"] = np.stack([np.tanh(z[:, :, 0])] + [_sigmoid(z[:, :, k]) for k in (1, 2, 3)], axis=2).reshape(B, 4 * h).astype(np.float32)
    return inp


_DRAW = {"rowgemm": _draw_rowgemm, "fwd": _draw_fwd, "bwd": _draw_bwd}

MS = BS = (1, 5, 16, 17, 33)
NS = (1, 7, 16, 17, 50)
KS = (4, 8, 12, 16, 20, 64, 132, 516, 1028)        # 516 / 1028: the second / third trip of a four-wave workgroup (8 k-blocks per wave and trip)
HS = (1, 3, 4, 6, 20, 36, 64)


def _rg(group, name, M, N, Ks, *, bias=False, addend=False, act=0, out2=False, carry_col0=None, longk=None):
    Ks = tuple(Ks)
    return Case("rowgemm", group, f"{name}-M{M}-N{N}-K{'+'.join(map(str, Ks))}-lk{longk}", M=M, N=N, Ks=Ks, bias=bias, addend=addend, act=act,
                out2=out2, carry_col0=carry_col0, longk=longk)


def _fw(group, name, B, h, Ks, *, zx=True, bias=True, c_prev=True, mask=True, hd=True, hd2=True, alias=False, ncells=1, saturate=False,
        longk=None):
    Ks = tuple(Ks)
    return Case("fwd", group, f"{name}-B{B}-h{h}-K{'+'.join(map(str, Ks))}-n{ncells}-lk{longk}", B=B, h=h, Ks=Ks, zx=zx, bias=bias,
                c_prev=c_prev, mask=mask, hd=hd, hd2=hd2, alias=alias, ncells=ncells, saturate=saturate, longk=longk)


def _bw(group, name, B, h, Ks, *, dy=True, dy2=True, dh_add=True, mask=True, dc_next=True, c_prev=True, ncells=1, longk=None):
    Ks = tuple(Ks)
    return Case("bwd", group, f"{name}-B{B}-h{h}-K{'+'.join(map(str, Ks))}-n{ncells}-lk{longk}", B=B, h=h, Ks=Ks, dy=dy, dy2=dy2,
                dh_add=dh_add, mask=mask, dc_next=dc_next, c_prev=c_prev, ncells=ncells, longk=longk)


RG_EPILOGUES = {                    # the combinations the product issues, then two it does not
    "bias": dict(bias=True),
    "wc": dict(bias=True, act=1, out2=True),
    "bias+addend": dict(bias=True, addend=True),
}
FWD_VARIANTS = {
    "all": dict(),
    "zx-only": dict(bias=False),
    "bias-only": dict(zx=False),
    "no-cprev": dict(c_prev=False),
    "no-mask": dict(mask=False),
    "hd-only": dict(hd2=False),
    "hd2-only": dict(hd=False),
    "no-hd": dict(hd=False, hd2=False, mask=False),
    "alias": dict(alias=True),
}
BWD_FLAGS = ("dy", "dy2", "dh_add", "mask", "dc_next", "c_prev")


def cases(cu=256):
    """The shared case list.  `cu`: the device's compute unit count (the two-row-tile shapes are stated relative to it)."""
    out = []
    # ---- rowgemm, one row tile per workgroup
    for M in MS:
        for N in NS:
            for K in KS:
                out.append(_rg("rg-plain", "plain", M, N, (K,)))
    shapes = ((1, 1), (5, 7), (16, 16), (17, 50), (33, 17))
    for M, N in shapes:
        for Ks in ((20, 132), (516, 12), (64, 0)):
            out.append(_rg("rg-epilogue", "pairs", M, N, Ks))
        for K in (12, 132):
            for nm, kw in RG_EPILOGUES.items():
                out.append(_rg("rg-epilogue", nm, M, N, (K,), **kw))
            out.append(_rg("rg-epilogue", "dh_top", M, N, (K, K + 8), addend=True))
            for c0 in sorted({c for c in (0, 4, 12, 16, N - 1) if 0 <= c < N}):
                out.append(_rg("rg-epilogue", f"d_x0-c{c0}", M, N, (K,), carry_col0=c0))
            out.append(_rg("rg-epilogue", "tanh+carry", M, N, (K,), act=1, carry_col0=min(4, N - 1)))
    # ---- rowgemm, eight waves
    for M, N in ((5, 7), (17, 50), (33, 17)):
        for K in (16, 20, 132, 1028, 2052):
            out.append(_rg("rg-waves", "knob", M, N, (K,), longk=16))
    for M, N in ((5, 7), (33, 50)):
        for Ks in ((2044,), (2048,), (1024, 1028)):
            out.append(_rg("rg-waves", "default", M, N, Ks))
    # ---- rowgemm, two row tiles per workgroup, and the other side of that decision
    for M, N in ((17, 16 * cu), (32, 16 * cu), (33, 8 * cu), (64, 8 * cu), (32, 16 * cu - 16)):
        for K in (4, 20):
            for longk in (None, 4):
                out.append(_rg("rg-two-tiles", "plain", M, N, (K,), longk=longk))
    out.append(_rg("rg-two-tiles", "wc", 17, 16 * cu, (20,), bias=True, act=1, out2=True))
    out.append(_rg("rg-two-tiles", "d_x0-c12", 33, 8 * cu, (20,), carry_col0=12, longk=4))
    # ---- forward cell
    names = list(FWD_VARIANTS)
    for ih, h in enumerate(HS):
        for ib, B in enumerate(BS):
            nm = names[(ih * len(BS) + ib) % len(names)]
            out.append(_fw("fwd-shapes", nm, B, h, (20, 12), **FWD_VARIANTS[nm]))
            out.append(_fw("fwd-shapes", "first-step", B, h, (0,)))
    for B, h in ((17, 6), (5, 20)):
        for nm, kw in FWD_VARIANTS.items():
            out.append(_fw("fwd-variants", nm, B, h, (8, 20), **kw))
        out.append(_fw("fwd-variants", "lateral", B, h, (36,)))
        out.append(_fw("fwd-variants", "saturated", B, h, (20, 12), saturate=True))
        for n in (2, 8):
            out.append(_fw("fwd-variants", "cells", B, h, (20, 12), ncells=n))
            out.append(_fw("fwd-variants", "cells-alias", B, h, (20,), ncells=n, alias=True))
    for B, h in ((17, 3), (5, 6)):
        for Ks in ((516,), (1028, 4)):                       # second and third trip at four waves
            out.append(_fw("fwd-waves", "trips4", B, h, Ks))
        for Ks in ((20, 12), (1028,), (1028, 1028)):         # eight waves through the knob; 1028: the second trip at eight waves
            out.append(_fw("fwd-waves", "knob", B, h, Ks, longk=16))
        out.append(_fw("fwd-waves", "default", B, h, (1024, 1028)))
    ct = cdiv(cu, 8)                                         # column tiles that fill the chip at 8 cells and one 32-row block
    for h in (4 * ct, 4 * (ct - 1)):
        for longk in (None, 16):
            out.append(_fw("fwd-two-tiles", "cells", 17, h, (20, 12), ncells=8, longk=longk))
    # ---- backward cell
    flagsets = [dict()] + [{f: False} for f in BWD_FLAGS] + [{f: False for f in BWD_FLAGS}]
    for ih, h in enumerate(HS):
        for ib, B in enumerate(BS):
            kw = flagsets[(ih * len(BS) + ib) % len(flagsets)]
            out.append(_bw("bwd-shapes", "two-pairs", B, h, (4 * h, 4 * h + 8), **kw))
            out.append(_bw("bwd-shapes", "one-pair", B, h, (4 * h,), **flagsets[(ih + ib) % len(flagsets)]))
    for B, h in ((17, 6), (5, 20)):
        for i, kw in enumerate(flagsets):
            out.append(_bw("bwd-variants", f"flags{i}", B, h, (4 * h, 12), **kw))
        out.append(_bw("bwd-variants", "last-step", B, h, (0,)))
        out.append(_bw("bwd-variants", "last-step", B, h, (0, 4 * h)))
        for n in (2, 8):
            out.append(_bw("bwd-variants", "cells", B, h, (4 * h, 20), ncells=n))
    for B in (5, 17):
        out.append(_bw("bwd-waves", "trip2-4waves", B, 260, (1040, 1028), longk=0))      # K > 1024: the second trip at four waves (CH = 16)
        out.append(_bw("bwd-waves", "trip2-4waves", B, 6, (24, 1040)))
        out.append(_bw("bwd-waves", "trip2-8waves", B, 516, (2064,)))                    # K > 2048: the second trip at eight waves
        out.append(_bw("bwd-waves", "max-not-sum", B, 6, (1024, 1028)))                  # sum >= 2048, maximum below: four waves
        out.append(_bw("bwd-waves", "knob", B, 6, (24, 20), longk=16))
    for h in (16 * ct, 16 * (ct - 1)):
        for longk in (None, 16):
            out.append(_bw("bwd-two-tiles", "cells", 17, h, (20, 36), ncells=8, longk=longk))
    names_seen = set()
    for c in out:
        assert c.name not in names_seen, c.name
        names_seen.add(c.name)
    return out


def case_list_problems(cs, cu=256):
    """Why a case list cannot tell a mutant from the model (empty: it can).  A carry case needs carry_col0 < N, an old carry that is not
    zero and an aux away from 0; a masked case needs a mask with both values; every mutant needs a case with the inputs it mishandles;
    every (kernel, MT, NW) instantiation needs a case."""
    bad = []
    for c in cs:
        s = c.spec
        if c.kind == "rowgemm" and s["carry_col0"] is not None:
            if not 0 <= s["carry_col0"] < s["N"]:
                bad.append(f"{c.name}: carry_col0 {s['carry_col0']} outside [0, N)")
                continue
            inp = c.inputs()[0]
            if np.abs(inp["carry"]).mean() < 1.0 or np.abs(inp["aux"]).min() < 0.05 or np.abs(inp["aux"]).max() > 0.95:
                bad.append(f"{c.name}: old carry near zero or aux near 0 / 1")
        if s.get("mask"):
            for inp in c.inputs():
                if inp["mask"].size >= 2 and not (inp["mask"].min() == 0 and inp["mask"].max() > 1):
                    bad.append(f"{c.name}: mask without both values")
    for m, (kind, needs) in MUTANTS.items():
        if not any(c.kind == kind and needs(c.spec) and (c.spec.get("B", 2) * c.spec.get("h", 2) >= 2) for c in cs):
            bad.append(f"mutant {m}: no case shows it")
    seen = {instantiation(c.kind, c.spec, cu) for c in cs}
    for kind in OPS:
        for mt in (1, 2):
            for nw in (4, 8):
                if (kind, mt, nw) not in seen:
                    bad.append(f"instantiation {kind}<{mt}, {nw}>: no case takes it")
    return bad
