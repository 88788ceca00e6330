"""Float32-level accuracy gates for the batched products of ast_amd/csrc/gemm.hip, shared by tests/test_gemm_accuracy_host.py (CPU) and
tests/test_gpu_gemm_accuracy.py (MI355X).  A helper, not a test module: nothing here touches a GPU.

gemm_launch_kernel instantiates one template nine times (KERNELS) and gemm_dispatch gives each up to five operand forms; indexed rows,
two-level rows and two-level C rows come on top.  CASES has one row per (kernel, operand form) at the smallest shapes at which that
kernel can still go wrong, plus split-tile, batched, bias and view cases per kernel; every row names the plan fields the launch must show.

Arithmetic, as gemm.hip states it (all operands are float32 numbers, the reference is their float64 product):
  bf16x3   hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), round-to-nearest-even; per 16-k block six MFMAs in the order
           lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi (64- and 128-tiles) or hi.hi, mid.hi, hi.mid, mid.mid, lo.hi, hi.lo (256 x 128)
  fp16x2   behind lowp_model.scale_of: hi = fp16(x s), lo = fp16(x s - hi); lo.hi, hi.lo, hi.hi; unscaled in the epilogue
  fp16     one term, lowp_model.round_operand (reference: the float64 product of the ROUNDED operands, as in tests/test_gpu_lowp.py)
  f32      v_mfma_f32_32x32x2_f32: eight MFMAs of k depth 2 per block, MFMA j on k = KROW(j) and KROW(j) + 2
model(): every term product of a block is summed exactly (float64: the terms are 16- or 22-bit products, 16 of them) and the accumulator
is rounded to float32 once per MFMA; the partial sums of a split tile's contributors are added in float32 in workgroup order.

Three gates:
 (a) selection identities: one operand dense, the other with one signed power of two per row -- every result entry is an operand entry
     times 2^e, no partial sum of the kernel's order rounds, and the device result must equal it bit for bit (selection());
 (b) error gate: N(0,1) operands, rows of A over four decades; |got - ref| of every entry over its own sqrt(sum_k a^2 b^2) (+ |c0| + |bias|)
     against TOL[scheme][K] = 4 x the worst figure of model() over the cases of that (scheme, K) (F32_MODEL_ERR: measured on the CPU by
     test_gemm_accuracy_host.py, which asserts that the model stays within a quarter of TOL);
 (c) projection gates (split schemes): for every term product and either operand's lowest plane p = exact(mutant) - ref, entries scaled as
     in (b); c = <got - ref, p> / <p, p> must stay within C_GATE.  A kernel that loses the term has c = 1, rounding noise is not aligned.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import lowp_model

NT, NN, TN = 0, 1, 2
STORE, ACCUM, ATOMIC = 0, 1, 2
PREC_API = {"bf16x3": 2, "fp16x2": 1, "f32": 3, "fp16": 0}       # ASTK_PREC_* a case passes ("fp16": the default + the lowp mark)
P_F32, P_BF16X3, P_F16, P_F16X2 = 0, 1, 2, 3                     # the `prec` field of a plan line (gemm.hip GemmPrec)
PLAN_PREC = {"bf16x3": P_BF16X3, "fp16x2": P_F16X2, "f32": P_F32, "fp16": P_F16}
OPERANDS_FP16 = 2
BK = 16
KS = (19, 96, 100, 531)

# name -> (scheme, TLM, TL, FIX)
KERNELS = {
    "x3-64": ("bf16x3", 64, 64, 0), "x3-128": ("bf16x3", 128, 128, 0), "x3-128-fix": ("bf16x3", 128, 128, 1), "x3-256": ("bf16x3", 256, 128, 0),
    "h2-64": ("fp16x2", 64, 64, 0), "h2-128": ("fp16x2", 128, 128, 0),
    "f32-64": ("f32", 64, 64, 0), "f32-128": ("f32", 128, 128, 0),
    "h1-128": ("fp16", 128, 128, 0),
}
TERMS = {                        # (plane of A, plane of B) per MFMA of a 16-k block, in the multiplying loop's order
    "bf16x3": ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)),
    "bf16x3-256": ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2)),
    "fp16x2": ((1, 0), (0, 1), (0, 0)),
    "fp16": ((0, 0),),
    "f32": ((0, 0),),
}
PLANE_NAMES = {"bf16x3": ("hi", "mid", "lo"), "fp16x2": ("hi", "lo"), "fp16": ("hi",), "f32": ("x",)}
KROW = lambda j: 4 * (j >> 1) + (j & 1)
C_GATE, C_F32_MAX, C_MUTANT_MIN = 0.25, 0.1, 0.8
COS_MAX = 0.3                    # largest |cosine| of two distinct directions of one case (host test)
# an operand's lowest plane enters one term product only: zeroing it and leaving that term out are the SAME direction
SAME_DIRECTION = {"bf16x3": {"A": (2, 0), "B": (0, 2)}, "fp16x2": {"A": (1, 0), "B": (0, 1)}}

# Worst |model - ref| / scale over the cases of a (scheme, K), printed by test_float32_model_error_is_what_the_tolerances_were_taken_from,
# and TOL = 4 x that figure rounded up to two digits (the project's quarter rule: it covers the MFMAs' internal summation, which the
# model takes as exact, and another order of a split tile's atomics).  Not tuned on device results.
F32_MODEL_ERR = {
    "bf16x3": {19: 7.2e-7, 96: 1.1e-6, 100: 1.2e-6, 531: 2.3e-6},
    "fp16x2": {19: 5.3e-7, 96: 6.4e-7, 100: 6.7e-7, 531: 6.4e-7},
    "f32": {19: 4.4e-7, 96: 9.2e-7, 100: 1.2e-6, 531: 8.5e-7},
    "fp16": {19: 2.8e-7, 96: 3.9e-7, 100: 5.1e-7, 531: 5.1e-7},
}
TOL = {s: {k: 4.0 * v for k, v in row.items()} for s, row in F32_MODEL_ERR.items()}


# ------------------------------------------------------------------ the case table
# a_view / b_view: None | ("2l", tn) two-level rows | ("perm",) indexed rows, a permutation | ("tall", extra) indexed rows into a taller array
Case = namedtuple("Case", "name kernel layout M N K batch modes grid bias a_view b_view c_tn")


def kernel_of(c):
    return KERNELS[c.kernel]


def _shape(kernel):
    _, TLM, TL, _ = KERNELS[kernel]
    return TLM + 6, TL + 3


def cdiv(a, b):
    return (a + b - 1) // b


def wg_first_iter(iters_total, unit, w, G, rem_start=0):
    return rem_start + ((iters_total - rem_start) // unit) * w // G * unit


def tile_ranges(M, N, K, batch, TLM, TL, G, unit):
    """Stream-K split of a one-product launch without data-parallel waves: per tile (batch-major, then row-major over the tiles) the
    [k0, k1) k-iteration ranges of its contributors in workgroup order."""
    kt = cdiv(K, BK)
    tiles = cdiv(M, TLM) * cdiv(N, TL) * batch
    total = tiles * kt
    out = [[] for _ in range(tiles)]
    for w in range(G):
        it, end = wg_first_iter(total, unit, w, G), wg_first_iter(total, unit, w + 1, G)
        while it < end:
            t = it // kt
            k0 = it - t * kt
            k1 = min(kt, k0 + end - it)
            out[t].append((k0, k1))
            it += k1 - k0
    return out


def unit_of(scheme, K):
    return 2 if (scheme != "f32" and cdiv(K, BK) % 2 == 0) else 1


def split_grid(kernel, M, N, K):
    """The smallest forced grid (no multiple of 8: no XCD remap, no hybrid schedule) that gives one tile at least three contributors and
    one tile exactly two.  tile_ranges is a second copy of gemm.hip's wg_first_iter: test_gemm_accuracy_host.py holds its contributor counts,
    for every case with split tiles, to the "contrib" line that astk_debug_gemm_views forms with the library's own function."""
    scheme, TLM, TL, _ = KERNELS[kernel]
    for G in range(2, 64):
        if G % 8 == 0:
            continue
        n = [len(r) for r in tile_ranges(M, N, K, 1, TLM, TL, G, unit_of(scheme, K))]
        if max(n) >= 3 and 2 in n:
            return G
    raise AssertionError((kernel, M, N, K))


def _cases():
    out = []
    for kernel, (scheme, TLM, TL, fix) in KERNELS.items():
        M, N = _shape(kernel)
        both = (STORE, ATOMIC)
        # every launch of the FIX kernel is a deterministic launch with a forced grid (that is what selects it)
        g0 = (lambda K: 5 if fix else 0)
        add = lambda name, *a: out.append(Case(f"{kernel}-{name}", kernel, *a))
        # (kernel, operand form) at two K each; every kernel sees all four K.  531 (a tail of 3 under paired loads) goes to the forms with
        # K-contiguous operands, 96 (unit 2) and 100 (unit 1, a tail of 4) to every family
        for layout, lname, ks in ((NT, "nt", (19, 531)), (NN, "nn", (96, 531)), (TN, "tn", (19, 100))):
            for K in ks:
                add(f"{lname}-k{K}", layout, M, N, K, 1, both, g0(K), 0, None, None, 0)
        add("nn2-k100", NN, M, N, 100, 1, both, g0(100), 0, ("perm",), ("2l", 24), 0)          # k-tile [0, 16) inside a group, [16, 32) straddles
        add("tn2-k96", TN, M, N, 96, 1, both, g0(96), 0, ("2l", 24), ("2l", 40), 6)            # ... both operands, two-level C rows
        add("tn2-k19", TN, M, N, 19, 1, both, g0(19), 0, ("2l", 16), ("2l", 5), 0)             # one group per k-tile; a group shorter than a k-tile
        add("mn2-k100", NT, M, N, 100, 1, both, g0(100), 0, ("2l", 5), ("2l", 7), 4)           # two-level M / N rows, two-level C rows
        add("idx-k531", NT, M, N, 531, 1, both, g0(531), 0, ("perm",), ("tall", 9), 0)
        G = split_grid(kernel, M, N, 100)
        for mode, mname in ((STORE, "store"), (ATOMIC, "atomic"), (ACCUM, "accum")):
            add(f"split-{mname}", (NT, NN, TN)[mode], M, N, 100, 1, (mode,), G, 0, None, None, 0)
        add("batch3", NT, M, N, 100, 3, both, g0(100), 0, None, None, 0)
        add("bias", NN, M, N, 19, 1, (STORE,), g0(19), 1, None, None, 0)
    names = [c.name for c in out]
    assert len(names) == len(set(names))
    return out


CASES = _cases()


def by_name(name):
    return next(c for c in CASES if c.name == name)


def is_view(c):
    return bool(c.a_view or c.b_view or c.c_tn) or kernel_of(c)[0] == "fp16"


def knobs(c):
    """The tuning knobs of a case.  "gemm.ticket" 0: the product library has no ticket path, and the instrumented build plans like it."""
    scheme, TLM, TL, fix = kernel_of(c)
    k = {"gemm.tile": TLM, "gemm.ticket": 0, "gemm.deterministic": fix}
    if c.grid:
        k["gemm.grid"] = c.grid
    return k


def grid_of(scheme, TLM, TL, M, N, K, batch, grid):
    """plan_grid of gemm.hip for a one-product launch of these sizes: (G, aligned)."""
    kt = cdiv(K, BK)
    tiles = cdiv(M, TLM) * cdiv(N, TL) * batch
    G, aligned = tiles, True
    assert tiles < 160 and tiles * kt < 256 * 20
    if min(256, tiles * kt // 8) > tiles:      # too few tiles to occupy the chip: the k range is split as well
        G, aligned = min(256, tiles * kt // 8), False
    if grid:
        G, aligned = min(grid, tiles * kt), False
    return G, aligned


def expected_plan(c, mode):
    """The plan fields a case must show for a launch in `mode`."""
    scheme, TLM, TL, fix = kernel_of(c)
    G, aligned = grid_of(scheme, TLM, TL, c.M, c.N, c.K, c.batch, c.grid)
    twolvl = int((c.layout == TN and bool(c.a_view) and c.a_view[0] == "2l") or (c.layout != NT and bool(c.b_view) and c.b_view[0] == "2l"))
    return dict(tile=TLM * 1000 + TL, prec=PLAN_PREC[scheme], fix=int(bool(fix) and not aligned), twolvl=twolvl, unit=unit_of(scheme, c.K), G=G,
                zero=int(not aligned and G > 1 and mode == STORE and not fix), kt=cdiv(c.K, BK), dp_waves=0, cs=0, aligned=int(aligned),
                rem_start=0, M=c.M, N=c.N, K=c.K, batch=c.batch, mode=mode, layout=c.layout)


def ranges_of(c):
    """Per tile the contributors' k-iteration ranges, or None when every workgroup owns whole tiles."""
    scheme, TLM, TL, _ = kernel_of(c)
    G, aligned = grid_of(scheme, TLM, TL, c.M, c.N, c.K, c.batch, c.grid)
    return None if aligned else tile_ranges(c.M, c.N, c.K, c.batch, TLM, TL, G, unit_of(scheme, c.K))


def model_case(c, A, B, bias=None, c0=None, mutant=None, f32=True):
    """product() per batch slice under the case's kernel and split."""
    scheme, TLM, TL, _ = kernel_of(c)
    r = ranges_of(c)
    per = cdiv(c.M, TLM) * cdiv(c.N, TL)
    return np.stack([product(A[b], B[b], scheme, TLM, TL, None if r is None else r[b * per:(b + 1) * per], bias,
                             None if c0 is None else c0[b], mutant, f32, measured_of(c)) for b in range(A.shape[0])])


def reference_case(c, A, B, bias=None, c0=None):
    return np.stack([reference(A[b], B[b], kernel_of(c)[0], bias, None if c0 is None else c0[b], measured_of(c)) for b in range(A.shape[0])])


def scale_case(A, B, bias=None, c0=None):
    return np.stack([entry_scale(A[b], B[b], bias, None if c0 is None else c0[b]) for b in range(A.shape[0])])


def measured_of(c):
    """fp16 operands: is the operand's maximum measured in front of the launch (plain rows), or is it cast as it is (a view)?"""
    return (int(not c.a_view), int(not c.b_view)) if kernel_of(c)[0] == "fp16" else (1, 1)


def arithmetic_key(c):
    """What model() depends on: cases with equal keys share operands, reference, model and mutants."""
    scheme, TLM, TL, _ = kernel_of(c)
    return (scheme, TLM, TL, c.M, c.N, c.K, c.batch, c.grid, c.bias) + measured_of(c)


# ------------------------------------------------------------------ the splits
def bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def planes(x, scheme, measured=True):
    """-> (float64 planes of the f32 array x in the kernel's plane order, scale).  The planes sum to x * scale (fp16: to its rounding)."""
    x = np.asarray(x, np.float32)
    if scheme == "bf16x3":
        hi = bf16(x)
        r = x - hi
        mid = bf16(r)
        lo = bf16(r - mid)
        return [p.astype(np.float64) for p in (hi, mid, lo)], 1.0
    if scheme == "f32":
        return [x.astype(np.float64)], 1.0
    s = lowp_model.scale_of(float(np.abs(x).max())) if (x.size and measured) else 1.0
    with np.errstate(over="ignore"):
        xs = x * np.float32(s)
        hi = xs.astype(np.float16)
        if scheme == "fp16":
            return [hi.astype(np.float64)], s
        lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return [hi.astype(np.float64), lo.astype(np.float64)], s


def term_order(scheme, TLM):
    return TERMS["bf16x3-256" if (scheme == "bf16x3" and TLM == 256) else scheme]


def _blocks(P, kt):
    """(rows, K) -> (rows, kt, 16), zero-padded: the kernel's zeroed K tail."""
    out = np.zeros((P.shape[0], kt * BK))
    out[:, :P.shape[1]] = P
    return out.reshape(P.shape[0], kt, BK)


def _f32(x):
    return x.astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------ mutants
# A mutant is (kind, operand, plane-or-term): what a subtly wrong kernel would multiply.
def mutants(scheme, TLM):
    npl, terms = len(PLANE_NAMES[scheme]), term_order(scheme, TLM)
    out = []
    for op in "AB":
        for p in range(npl):
            out += [("zero", op, p), ("roll-row", op, p), ("roll-k", op, p), ("stale", op, p)]
    out += [("drop", "-", t) for t in range(len(terms))]
    return out


def mutant_name(m, scheme, TLM):
    kind, op, i = m
    if kind == "drop":
        pa, pb = term_order(scheme, TLM)[i]
        return f"drop {PLANE_NAMES[scheme][pa]}.{PLANE_NAMES[scheme][pb]}"
    return f"{kind} {op}.{PLANE_NAMES[scheme][i]}"


def directions(scheme, TLM):
    """Gate (c): every term product left out, and either operand's lowest plane zeroed (split schemes)."""
    if scheme not in ("bf16x3", "fp16x2"):
        return []
    low = len(PLANE_NAMES[scheme]) - 1
    return [("drop", "-", t) for t in range(len(term_order(scheme, TLM)))] + [("zero", "A", low), ("zero", "B", low)]


def _mutate(pa, pb, kt, mutant):
    """pa, pb: lists of (rows, kt, 16) planes -> mutated copies, dropped term index."""
    if mutant is None:
        return pa, pb, None
    kind, op, i = mutant
    if kind == "drop":
        return pa, pb, i
    pl = list(pa if op == "A" else pb)
    P = pl[i]
    if kind == "zero":
        P = np.zeros_like(P)
    elif kind == "roll-row":
        P = np.roll(P, 1, axis=0)
    elif kind == "roll-k":
        P = np.roll(P.reshape(P.shape[0], -1), 1, axis=1).reshape(P.shape)
    elif kind == "stale":              # the block's plane is the one of the previous k-iteration (block 0 keeps its own)
        P = np.concatenate([P[:, :1], P[:, :-1]], axis=1)
    pl[i] = P
    return (pl, pb, None) if op == "A" else (pa, pl, None)


def product(A, B, scheme, TLM, TL, ranges=None, bias=None, c0=None, mutant=None, f32=True, measured=(1, 1)):
    """A (M, K), B (N, K) float32 -> the (M, N) result as float64.  f32: the float32 model (one rounding per MFMA, split tiles' partial sums
    added in float32); else the same terms summed exactly (the projection gates' directions)."""
    M, K = A.shape
    N = B.shape[0]
    kt = cdiv(K, BK)
    (pa, sa), (pb, sb) = planes(A, scheme, measured[0]), planes(B, scheme, measured[1])
    pa, pb = [_blocks(p, kt) for p in pa], [_blocks(p, kt) for p in pb]
    pa, pb, dropped = _mutate(pa, pb, kt, mutant)
    terms = [t for i, t in enumerate(term_order(scheme, TLM)) if i != dropped]
    if scheme == "f32":                # eight MFMAs of k depth 2: the block's k as (8, 2), MFMA j on KROW(j), KROW(j) + 2
        idx = np.array([[KROW(j), KROW(j) + 2] for j in range(BK // 2)])
        steps = [np.einsum("mbjk,nbjk->bjmn", pa[0][:, :, idx], pb[0][:, :, idx])] if terms else []
        T = steps[0].reshape(kt * (BK // 2), M, N) if steps else np.zeros((0, M, N))
        per_block = BK // 2 if terms else 0
    else:
        T = np.stack([np.einsum("mbk,nbk->bmn", pa[i], pb[j]) for i, j in terms], axis=1).reshape(kt * len(terms), M, N) if terms else np.zeros((0, M, N))
        per_block = len(terms)
    rnd = _f32 if f32 else (lambda x: x)
    out = np.zeros((M, N)) if c0 is None else np.array(c0, np.float64)
    tiles_n = cdiv(N, TL)
    if ranges is None:
        ranges = [[(0, kt)]] * (cdiv(M, TLM) * tiles_n)
    for t, contrib in enumerate(ranges):
        m0, n0 = (t // tiles_n) * TLM, (t % tiles_n) * TL
        sl = (slice(m0, min(m0 + TLM, M)), slice(n0, min(n0 + TL, N)))
        for k0, k1 in contrib:
            acc = np.zeros((sl[0].stop - m0, sl[1].stop - n0))
            for s in range(k0 * per_block, k1 * per_block):
                acc = rnd(acc + T[s][sl])
            acc = rnd(rnd(acc / sa) / sb) if (sa != 1.0 or sb != 1.0) else acc       # (powers of two: exact)
            if bias is not None and k0 == 0:
                acc = rnd(acc + np.asarray(bias, np.float64)[None, sl[1]])
            out[sl] = rnd(out[sl] + acc)
    return out


def reference(A, B, scheme, bias=None, c0=None, measured=(1, 1)):
    """float64; fp16: the product of the rounded operands."""
    if scheme == "fp16":
        a, b = lowp_model.round_measured(A, measured[0]), lowp_model.round_measured(B, measured[1])
    else:
        a, b = np.asarray(A, np.float64), np.asarray(B, np.float64)
    r = a @ b.T
    if bias is not None:
        r = r + np.asarray(bias, np.float64)[None, :]
    if c0 is not None:
        r = r + np.asarray(c0, np.float64)
    return r


def entry_scale(A, B, bias=None, c0=None):
    """sqrt(sum_k a^2 b^2) per entry, plus |c0| and |bias| where they enter."""
    s = np.sqrt((np.asarray(A, np.float64) ** 2) @ (np.asarray(B, np.float64) ** 2).T)
    if bias is not None:
        s = s + np.abs(np.asarray(bias, np.float64))[None, :]
    if c0 is not None:
        s = s + np.abs(np.asarray(c0, np.float64))
    return np.where(s > 0, s, 1.0)


def coefficient(got, ref, p, scale):
    d, q = ((got - ref) / scale).ravel(), (p / scale).ravel()
    return float(d @ q) / float(q @ q)


# ------------------------------------------------------------------ operands
def _seed(key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=None)
def dense_operands(key):
    """Gate (b), (c): N(0,1), rows of A over four decades (lowp_model.gemm_operands); a bias and the c0 of an accumulating launch."""
    scheme, TLM, TL, M, N, K, batch, grid, bias, ma, mb = key
    rng = np.random.default_rng(_seed(key))
    A = (rng.standard_normal((batch, M, K)) * (10.0 ** (-(np.arange(M) % 4)))[None, :, None]).astype(np.float32)
    B = rng.standard_normal((batch, N, K)).astype(np.float32)
    bv = rng.standard_normal(N).astype(np.float32) if bias else None
    c0 = (0.5 * rng.standard_normal((batch, M, N))).astype(np.float32)
    return A, B, bv, c0


def _heavy(rng, shape, scheme, with_max=True):
    """heavy() of tests/test_gpu_ops.py with sigma 3 and exponents within 2^+-20; fp16x2: 22-bit mantissas within 2^5 of the maximum;
    fp16: 11-bit mantissas within fp16's normal range behind the scale."""
    if scheme == "fp16x2" or scheme == "fp16":
        bits = 22 if scheme == "fp16x2" else 11
        e = rng.integers(-4, 1, size=shape)
        m = rng.integers(2 ** (bits - 1), 2 ** bits, size=shape).astype(np.float64) / 2.0 ** bits          # [0.5, 1)
        x = m * 2.0 ** e * rng.choice([-1.0, 1.0], size=shape)
        if with_max:
            x.flat[rng.integers(0, x.size)] = (2.0 ** bits - 1) / 2.0 ** bits                                   # the maximum, present
        return x.astype(np.float32)
    mag = np.clip(np.exp(rng.normal(0.0, 3.0, size=shape)), 2.0 ** -20, 2.0 ** 20)
    return (mag * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def exact_under_every_order(x, scheme):
    """Per value: do all orders of adding its planes (times a power of two) stay exact in float32?"""
    import itertools
    pl, s = planes(x, scheme)
    ok = np.ones(np.shape(x), bool)
    for order in itertools.permutations(range(len(pl))):
        acc = np.zeros(np.shape(x))
        exact = np.zeros(np.shape(x))
        for i in order:
            exact = exact + pl[i]
            acc = _f32(acc + pl[i])
            ok &= acc == exact
    return ok & (sum(pl) == np.asarray(x, np.float64) * s)


def sigma_of(K, rows, ranges_kt=(), phase=0):
    """k = sigma(row) of pass `phase`: the passes of a case together cover every k of [0, K); k = 0, K - 1, both sides of every
    k-iteration boundary and of every stream-K range boundary come first."""
    must = [0, K - 1]
    for b in sorted(set(list(range(BK, K, BK)) + [k * BK for k in ranges_kt if 0 < k * BK < K])):
        must += [b - 1, b]
    must = list(dict.fromkeys(must))
    seq = must + [k for k in range(K) if k not in must]
    return np.array([seq[(phase * rows + r) % K] for r in range(rows)])


def phases(key, role):
    """Passes of the selection identity: the selecting operand has one nonzero per row, so K / rows passes reach every k."""
    return cdiv(key[5], key[4] if role == "A" else key[3])


@functools.lru_cache(maxsize=None)
def selection(key, role, phase=0):
    """Gate (a).  role "A": A dense, B selecting -- C[i, j] = A[i, sigma(j)] s_j; role "B": B dense, A selecting.  -> A, B (float32, batch
    leading), the expected result (float32, exact), the share of redrawn values."""
    scheme, TLM, TL, M, N, K, batch, grid, bias, ma, mb = key
    rng = np.random.default_rng(_seed(key + (role, phase)))
    rows_d, rows_s = (M, N) if role == "A" else (N, M)
    D = _heavy(rng, (batch, rows_d, K), scheme)
    drawn, redrawn = D.size, 0
    for _ in range(20):          # a value that is inexact under ANY order of its terms is redrawn
        bad = ~exact_under_every_order(D, scheme)
        if not bad.any():
            break
        redrawn += int(bad.sum())
        D[bad] = _heavy(rng, (int(bad.sum()),), scheme, with_max=False)
    assert exact_under_every_order(D, scheme).all()
    G, aligned = grid_of(scheme, TLM, TL, M, N, K, batch, grid)
    cuts = () if aligned else sorted({k for r in tile_ranges(M, N, K, batch, TLM, TL, G, unit_of(scheme, K)) for k0k1 in r for k in k0k1})
    sig = sigma_of(K, rows_s, tuple(cuts), phase)
    S = np.zeros((batch, rows_s, K), np.float32)
    val = (2.0 ** rng.integers(-3, 4, size=(batch, rows_s)) * rng.choice([-1.0, 1.0], size=(batch, rows_s))).astype(np.float32)
    val[:, 0] = 8.0
    for b in range(batch):
        S[b, np.arange(rows_s), sig] = val[b]
    picked = D[:, :, sig].astype(np.float64) * val[:, None, :].astype(np.float64)       # (batch, rows_d, rows_s)
    expect = picked if role == "A" else picked.transpose(0, 2, 1)
    assert (expect.astype(np.float32).astype(np.float64) == expect).all()
    A, B = (D, S) if role == "A" else (S, D)
    return A, B, expect.astype(np.float32), redrawn / drawn


# ------------------------------------------------------------------ device images and the hook's arguments (no GPU needed to form them)
def pad4(n):
    return (n + 3) // 4 * 4


class Image:
    """One operand (batch, rows, inner) as the flat float32 buffer a launch reads: rows of ld = pad4(inner) + 4 floats, `fill` (NaN)
    wherever no operand value lies, under plain, two-level or indexed row addressing."""

    def __init__(self, X, view, fill=np.nan, seed=0, pad_batch=True):
        X = np.asarray(X, np.float32)
        bt, r, i = X.shape
        self.ld = self.st = pad4(i) + 4
        self.tn = self.sg = self.idx_rows = 0
        self.rowidx = None
        kind = view[0] if view else None
        assert kind is None or bt == 1
        if kind == "2l":
            self.tn = view[1]
            self.sg = self.tn * self.st + 8
            rows = np.arange(r)
            off = (rows // self.tn) * self.sg + (rows % self.tn) * self.st
            size = cdiv(r, self.tn) * self.sg
        else:
            rows_alloc = r + (view[1] if kind == "tall" else 0)
            idx = np.arange(r)
            if kind in ("perm", "tall"):
                idx = np.random.default_rng(seed + r + i).permutation(rows_alloc)[:r]
                self.rowidx = idx.astype(np.int32)
                self.idx_rows = rows_alloc if kind == "tall" else 0
            off = idx * self.ld
            size = rows_alloc * self.ld
        self.stride = size + 8 if (bt > 1 and pad_batch) else size              # padded batch stride
        self.buf = np.full(bt * self.stride, fill, np.float32)
        for b in range(bt):
            for x in range(r):
                self.buf[b * self.stride + off[x]:b * self.stride + off[x] + i] = X[b, x]


class Result:
    """Addressing of C: (batch, M) rows of ldc = pad4(N) + 4, plain or two-level, and a guard band behind the buffer."""
    GUARD = 4096

    def __init__(self, M, N, batch, c_tn):
        self.M, self.N, self.batch, self.tn = M, N, batch, c_tn
        self.ld = self.st = pad4(N) + 4
        self.sg = c_tn * self.st + 8 if c_tn else 0
        rows = np.arange(M)
        self.off = (rows // c_tn) * self.sg + (rows % c_tn) * self.st if c_tn else rows * self.ld
        size = cdiv(M, c_tn) * self.sg if c_tn else M * self.ld
        self.stride = size + 8 if batch > 1 else size
        self.size = batch * self.stride
        self.index = (np.arange(batch)[:, None, None] * self.stride + self.off[None, :, None] + np.arange(N)[None, None, :])     # (batch, M, N)


def operand_images(c, A, B, fill=np.nan):
    """A (batch, M, K), B (batch, N, K) -> the images in the case's layout (K-major operands stored transposed) and addressing."""
    a = np.asarray(A).transpose(0, 2, 1) if c.layout == TN else np.asarray(A)
    b = np.asarray(B).transpose(0, 2, 1) if c.layout != NT else np.asarray(B)
    # (single-term fp16: both operands are measured, and a measured batched operand is measured as one matrix -- its slices follow each
    #  other without a gap; h1-128-batch3 therefore pads the stride of C only)
    dense = kernel_of(c)[0] != "fp16"
    return Image(a, c.a_view, fill, 1, dense), Image(b, c.b_view, fill, 2, dense)


def views_call(tl, c, mode, ia, ib, rc, ptrs, launch, stream=None):
    """astk_debug_gemm_views for one case.  ptrs: (A, B, C, a_rowidx, b_rowidx, bias) addresses (plan only: any non-null numbers; bias: None = none).
    -> (return code, plan text)."""
    import ctypes as C
    I = lambda v: (C.c_int32 * 1)(int(v))
    L = lambda v: (C.c_long * 1)(int(v))
    P = lambda v: (C.c_void_p * 1)(v)
    scheme = kernel_of(c)[0]
    pa, pb, pc, pia, pib, pbias = ptrs
    meas = measured_of(c) if scheme == "fp16" else (0, 0)
    buf = C.create_string_buffer(1 << 12)
    rcode = tl.astk_debug_gemm_views(
        c.layout, 1, I(c.M), I(c.N), I(c.K), I(c.batch), I(mode), I(scheme == "fp16"), I(meas[0] | 2 * meas[1]),
        P(pa), L(ia.ld), L(ia.stride), P(pb), L(ib.ld), L(ib.stride), P(pc), L(rc.ld), L(rc.stride),
        I(ia.tn), L(ia.sg), L(ia.st), P(pia if ia.rowidx is not None else None), L(ia.idx_rows),
        I(ib.tn), L(ib.sg), L(ib.st), P(pib if ib.rowidx is not None else None), L(ib.idx_rows),
        I(rc.tn), L(rc.sg), L(rc.st), P(pbias), PREC_API[scheme], OPERANDS_FP16 if scheme == "fp16" else 0,
        int(launch), buf, len(buf), stream)
    return rcode, buf.value.decode()


def plan_contributors(text):
    """The "contrib" line of the hook's plan text: workgroups per tile, counted by the library."""
    lines = [ln for ln in text.splitlines() if ln.startswith("contrib 0")]
    assert len(lines) == 1, text
    return [int(v) for v in lines[0].split()[2:]]


def plan_fields(text):
    lines = [ln for ln in text.splitlines() if ln.startswith("astk_gemm")]
    assert len(lines) == 1, text
    return {k: int(v.split("/")[0]) for k, v in (tok.split("=", 1) for tok in lines[0].split()[1:])}


class Knobs:
    """The case's tuning knobs, and the fp16x2 scheme on launches of any size, on every library given; restored on exit."""

    def __init__(self, libs, c):
        self.libs, self.knobs, self.undo = libs, knobs(c), []

    def __enter__(self):
        import ctypes as C
        try:
            for lib in self.libs:
                for key, v in self.knobs.items():
                    old = C.c_double()
                    if lib.astk_get_tuning(key.encode(), C.byref(old)) != 0:
                        assert key == "gemm.ticket", key          # (the one knob a library may not have)
                        continue
                    assert lib.astk_set_tuning(key.encode(), float(v)) == 0, key
                    self.undo.append((lib.astk_set_tuning, (key.encode(), old.value)))
                self.undo.append((lib.astk_set_gemm_bf16_split_below, (C.c_double(lib.astk_set_gemm_bf16_split_below(C.c_double(0.0))),)))
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        while self.undo:
            fn, args = self.undo.pop()
            fn(*args)
        return False
