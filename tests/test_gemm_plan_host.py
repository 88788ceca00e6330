"""The GEMM launcher's plan, pinned on the host (no GPU): what gemm_launch_group decides for a grouped launch is a value -- GemmPlan,
computed by the pure gemm_plan (ast_amd/csrc/gemm.hip) -- and astk_debug_gemm_plan (libastk_test.so) prints it without touching a
device.  Every case of CASES is planned and compared, line for line, with tests/golden/gemm_plans.txt, which was recorded from the
launcher BEFORE it was split into plan and execute (scratch/gemm_plan_record.py over scratch/gemm_plan_parent.patch) and is never
re-recorded from the code under test.  test_every_branch_is_reached keeps the table honest: each decision of the launcher is reached
by a named case, checked on the plan's own fields."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_plans.txt")
NT, NN, TN = 0, 1, 2
STORE, ACCUM, ATOMIC = 0, 1, 2
DEFAULT, FP16X2, BF16X3, F32 = 0, 1, 2, 3          # astk.h ASTK_PREC_*
P_F32, P_BF16X3, P_F16, P_F16X2 = 0, 1, 2, 3       # the `prec` field of a plan line: gemm.hip GemmPrec
OPERANDS_FP16 = 2
KNOBS = ["gemm.tile", "gemm.t256_above", "gemm.grid", "gemm.hybrid", "gemm.chunk", "gemm.chunk_div", "gemm.forward_pairs", "gemm.ticket"]


def case(name, layout, prods, forward=0, precision=DEFAULT, operands=0, det=0, cap=0, pad=1, **knobs):
    """prods: (M, N, K[, batch[, mode[, lowp[, given]]]]) per product; knobs: gemm_tile=64 sets "gemm.tile" for the case.  "gemm.ticket"
    is 0 unless a case asks for it: the product library has no ticket path, and the table describes the product's launches."""
    prods = [tuple(p) + (1, STORE, 0, 0)[len(p) - 3:] for p in prods]
    k = {"gemm.ticket": 0}
    k.update({key.replace("_", ".", 1): v for key, v in knobs.items()})
    assert set(k) <= set(KNOBS), k
    return dict(name=name, layout=layout, prods=prods, forward=forward, precision=precision, operands=operands, det=det, cap=cap, pad=pad,
                knobs=k)


def _random_sweep():
    """The 90 draws of test_gemm_random_shapes_against_float64 (tests/test_gpu_ops.py): the same generator, advanced the same way."""
    import numpy as np
    rng = np.random.default_rng(2026)
    shapes = []
    for i in range(90):
        layout = int(rng.integers(0, 3))
        M, N = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        K = int(rng.choice([1, 3, 15, 16, 17, 31, 33, 64, 100, 257, 700]))
        batch = int(rng.choice([1, 1, 3]))
        mode = int(rng.integers(0, 3))
        extra = 4 * int(rng.integers(0, 3))
        rng.standard_normal((batch, M, K))
        rng.standard_normal((batch, N, K))
        rng.standard_normal((batch, M, (N + 3) // 4 * 4 + extra))
        if mode == 0 and i % 2 == 0:
            rng.standard_normal(N)
        shapes.append((layout, M, N, K, batch, mode))
    return shapes


def _cases():
    out = []
    # -- every shape, layout and mode of the GEMM tests in tests/test_gpu_ops.py (their rows are padded to 16 bytes: pad=1), under the
    #    three arithmetic schemes of their gemm_split fixture where they take it (fp16x2 there with the small-launch downgrade off, which
    #    is a process setting no plan argument carries: those cases give both maxima instead, the downgrade's own exception)
    lay3 = (NT, NN, TN)
    schemes = (("bf16x3", BF16X3, 0), ("fp16x2", FP16X2, 1), ("f32", F32, 0))

    def sweep(test, shapes, modes, layouts=lay3, sch=schemes, batch=1, **kw):
        for (M, N, K) in shapes:
            for lay in layouts:
                for sname, prec, given in sch:
                    for mode in modes:
                        out.append(case(f"{test}-{M}x{N}x{K}{'*%d' % batch if batch > 1 else ''}-l{lay}-m{mode}-{sname}", lay,
                                        [(M, N, K, batch, mode, 0, given)], precision=prec, **kw))
    sweep("layouts", [(128, 128, 32), (200, 72, 120), (37, 1098, 512), (6, 8, 44), (300, 260, 1000), (1, 1, 4)], (STORE, ACCUM, ATOMIC))
    sweep("padding", [(70, 45, 37), (130, 129, 16), (5, 3, 1), (129, 70, 531)], (STORE,))
    sweep("hybrid", [(4100, 1150, 330), (2100, 2100, 300), (33000, 200, 200)], (STORE, ACCUM, ATOMIC))
    sweep("hybrid", [(1100, 1200, 330)], (STORE, ACCUM, ATOMIC), batch=4)
    sweep("deepk", [(512, 1152, 38400), (260, 200, 51200)], (ATOMIC,))
    sweep("deepk", [(512, 640, 24000)], (ACCUM,))
    sweep("split", [(4100, 1150, 332), (300, 260, 20000), (130, 70, 5000), (8200, 1930, 1100)], (STORE,), layouts=(NT,))
    sweep("ticket", [(4100, 1150, 332), (300, 260, 20000), (130, 70, 5000), (8200, 1930, 1100)], (STORE,), layouts=(NT,), sch=schemes[:1],
          gemm_ticket=1)
    for (M, N, K, mode) in [(512, 1152, 38400, ATOMIC), (260, 200, 51200, ACCUM), (4100, 1150, 332, STORE), (1100, 3072, 1024, STORE),
                            (300, 260, 20000, STORE)]:
        sweep("det", [(M, N, K)], (mode,), sch=schemes[:1], det=1)
    fwd_groups = [(NT, [(256, 256, 16384)]), (TN, [(384, 128, 40000)]), (NT, [(1248, 512, 512), (1248, 512, 1152), (640, 1024, 3072)]),
                  (NN, [(2000, 640, 256), (700, 384, 2048)]), (NT, [(38400, 512, 1152)])]
    for i, (lay, shapes) in enumerate(fwd_groups):
        for fwd in (1, 0):
            out.append(case(f"fwdgroup{i}-f{fwd}", lay, shapes, forward=fwd, precision=BF16X3, pad=0))
    for (lay, M, N, K) in [(NT, 256, 256, 16384), (TN, 384, 128, 40000), (NN, 1200, 300, 6000), (NT, 38400, 512, 1152)]:
        out.append(case(f"fwdrule-{M}x{N}x{K}-l{lay}", lay, [(M, N, K)], gemm_forward_pairs=2))
    sweep("t256", [(8200, 1930, 1100)], (STORE, ATOMIC, ACCUM), sch=schemes[:1])
    sweep("magnitudes", [(150, 130, 333)], (STORE,))
    sweep("ring", [(1024, 1024, 1536), (2048, 512, 1600), (96, 8192, 2048)], (STORE,), layouts=(NT,), sch=(("fp16x2-own", FP16X2, 0),), pad=0)
    sweep("heavy", [(1024, 1536, 2048), (1024, 6400, 1024)], (STORE,))
    sweep("tail", [(7, 5, 3), (9, 6, 2), (33, 3, 7), (5, 3, 1), (130, 66, 19)], (STORE,))
    for i, (lay, M, N, K, batch, mode) in enumerate(_random_sweep()):
        for sname, prec, given in schemes:
            out.append(case(f"random{i}-{sname}", lay, [(M, N, K, batch, mode, 0, given)], precision=prec))
    for sname, prec, given in schemes:
        out.append(case(f"batched-tn-{sname}", TN, [(22, 40, 9, 5, STORE, 0, given)], precision=prec))
    # -- the distinct grouped launches of one benchmark train step (gemm.log of the step before this change; dense operands here)
    for i, (lay, prods) in enumerate(STEP_LAUNCHES):
        for fwd in (0, 1):
            out.append(case(f"step{i}-f{fwd}", lay, prods, forward=fwd))
    # -- the launcher's branches (test_every_branch_is_reached names them)
    out += [
        case("auto64", NT, [(300, 260, 1000)]), case("auto128", NT, [(4100, 1150, 330)]), case("auto256", NT, [(8200, 1930, 1100)]),
        case("force64", NT, [(300, 260, 100)], gemm_tile=64), case("force128", NT, [(300, 260, 100)], gemm_tile=128),
        case("force256", NT, [(300, 260, 100)], gemm_tile=256),
        case("small-downgrade", NT, [(300, 260, 1000)], precision=FP16X2),
        case("small-given", NT, [(300, 260, 1000, 1, STORE, 0, 1)], precision=FP16X2),
        case("big-fp16x2", NT, [(4100, 1150, 332)], precision=FP16X2),
        case("lowp-taken", NT, [(300, 260, 1000, 1, STORE, 1), (200, 260, 1000, 1, STORE, 1)], operands=OPERANDS_FP16),
        case("lowp-refused", NT, [(300, 260, 1000, 1, STORE, 1), (200, 260, 1000, 1, STORE, 0)], operands=OPERANDS_FP16),
        case("cap-small", NT, [(1024, 512, 512)], cap=128), case("cap-not-small", NT, [(1024, 1024, 512)], cap=64),
        case("cap-fp16x2", NT, [(4100, 1150, 332)], precision=FP16X2, cap=64),
        case("aligned", NT, [(2048, 2048, 256)]),
        case("aligned-mixed-kt", NT, [(2048, 1024, 256), (2048, 1024, 512)]),
        case("forced-grid", NT, [(300, 260, 1000)], gemm_grid=24),
        case("hybrid", NT, [(4100, 1150, 330)]), case("hybrid-forward", NT, [(4100, 1150, 330)], forward=1),
        case("hybrid-off", NT, [(4100, 1150, 330)], gemm_hybrid=0),
        case("hybrid-accum", NT, [(4100, 1150, 330, 1, ACCUM)]),
        case("fwdcap-gmax", NT, [(1248, 512, 512), (1248, 512, 1152), (640, 1024, 3072)], forward=1),
        case("fwdcap-pairs", NT, [(256, 256, 16384)], forward=1),
        case("fwdcap-off", NT, [(256, 256, 16384)], forward=1, gemm_forward_pairs=0),
        case("chunk", NT, [(128, 128, 2048, 1, ACCUM)]), case("chunk-tn", TN, [(128, 128, 2048, 1, ACCUM)]),
        case("chunk-det", NT, [(128, 128, 2048, 1, ACCUM)], det=1), case("chunk-off", NT, [(128, 128, 2048, 1, ACCUM)], gemm_chunk=0),
        case("chunk-div", NT, [(128, 128, 2048, 1, ACCUM)], gemm_chunk_div=32),
        case("det-fix", NT, [(4100, 1150, 332)], det=1),
        case("det-clipped", NT, [(4100, 1150, 332)], det=1, gemm_grid=512), case("det-unclipped", NT, [(4100, 1150, 332)], gemm_grid=512),
        case("det-f32", NT, [(4100, 1150, 332)], det=1, precision=F32),
        case("zero-vec", NT, [(4100, 1152, 332)]), case("zero-scalar", NT, [(4100, 1150, 332)], pad=0),
        case("ticket", NT, [(4100, 1150, 332)], gemm_ticket=1),
        case("skipped", NT, [(0, 128, 128), (128, 128, 0)]), case("skipped-one", NT, [(0, 128, 128), (128, 128, 64)]),
        case("empty", NT, []),
        case("error-ldb", NN, [(128, 130, 64)], pad=0),
        case("t256-above", NT, [(4100, 1150, 330)], gemm_t256_above=1e9),
    ]
    names = [c["name"] for c in out]
    assert len(names) == len(set(names)), [n for n in names if names.count(n) > 1]
    return out


# (layout, products) of the 14 grouped launches of one train step of bench.py's model (B 32, T 800), all distinct: M, N, K, batch, mode,
# from the step's gemm.log (scratch/gemm_step_trace.py run).  The log does not say which scopes were open: each is planned with and
# without the forward scope.
STEP_LAUNCHES = [
    (NT, [(38400, 512, 1152, 1, 0)]),
    (NT, [(6400, 1024, 3072, 1, 0), (6400, 1024, 3072, 1, 0)]),
    (NN, [(6400, 512, 512, 1, 0)]),
    (NT, [(1248, 512, 512, 1, 0)]),
    (TN, [(200, 512, 39, 32, 2), (200, 512, 39, 32, 2)]),
    (NN, [(1248, 128, 2048, 1, 0), (39, 512, 200, 32, 0)]),
    (TN, [(512, 1024, 1248, 1, 2), (512, 512, 1248, 1, 2), (1098, 512, 1248, 1, 2), (2048, 640, 1248, 1, 2), (2048, 512, 1248, 1, 2)]),
    (NN, [(6400, 3072, 1024, 1, 0)]),
    (TN, [(1024, 3072, 6400, 1, 2)]),
    (NN, [(6400, 3072, 1024, 1, 1)]),
    (TN, [(1024, 256, 6368 + 32 * (i % 2), 1, 2) for i in range(9)] + [(1024, 3072, 6400, 1, 2), (1024, 256, 6368, 1, 2)]),
    (TN, [(512, 1152, 38400, 1, 2)]),
    (NT, [(38400, 128, 2560, 1, 0), (38400, 128, 2048, 1, 0)]),
    (TN, [(128, 126, 76800, 1, 2)]),
]

CASES = _cases()


def plan_text(tlib, c):
    """The plan of one case as the golden file holds it: the hook's lines, or "error: <text>" where the launch is refused."""
    n = len(c["prods"])
    col = lambda j: (C.c_int32 * max(n, 1))(*[p[j] for p in c["prods"]])
    prev = {}
    for key, v in c["knobs"].items():
        old = C.c_double()
        assert tlib.astk_get_tuning(key.encode(), C.byref(old)) == 0
        prev[key] = old.value
        assert tlib.astk_set_tuning(key.encode(), float(v)) == 0
    try:
        buf = C.create_string_buffer(1 << 14)
        rc = tlib.astk_debug_gemm_plan(c["layout"], n, col(0), col(1), col(2), col(3), col(4), col(5), col(6), c["forward"], c["precision"],
                                       c["operands"], c["det"], c["cap"], c["pad"], buf, len(buf))
        return buf.value.decode() if rc == 0 else "error: " + tlib.astk_last_error().decode() + "\n"
    finally:
        for key, v in prev.items():
            assert tlib.astk_set_tuning(key.encode(), v) == 0


def read_golden():
    plans, name = {}, None
    for ln in open(GOLDEN).read().splitlines():
        if ln.startswith("# "):
            name = ln[2:]
            plans[name] = []
        elif ln:
            plans[name].append(ln)
    return plans


def fields(line):
    return {k: v for k, v in (tok.split("=", 1) for tok in line.split()[1:])}


@pytest.fixture
def tlib():
    from ast_amd import _lib
    with _lib.load_test_hooks() as t:
        yield t


def test_plans_equal_the_recorded_ones(tlib):
    golden = read_golden()
    assert list(golden) == [c["name"] for c in CASES], "the case table and tests/golden/gemm_plans.txt list other cases"
    bad = []
    for c in CASES:
        got = plan_text(tlib, c).splitlines()
        if got != golden[c["name"]]:
            bad.append((c["name"], got, golden[c["name"]]))
    assert not bad, f"{len(bad)} of {len(CASES)} plans differ from the recorded ones; first: {bad[0]}"


def _cdiv(a, b):
    return (a + b - 1) // b


def test_every_branch_is_reached():
    """Each decision of the launcher, read off the RECORDED plans: a later edit of the table cannot silently drop a branch.  It reads the
    golden file only and says nothing about the code by itself: test_plans_equal_the_recorded_ones ties the code, and the table's case
    names, to that file.  The two tests hold as a pair."""
    g = {name: [fields(ln) for ln in lines if ln.startswith("astk_gemm")] for name, lines in read_golden().items()}
    raw = read_golden()
    one = lambda name: g[name][0]
    I = lambda name, key: int(one(name)[key])
    by = {c["name"]: c for c in CASES}

    def tiles(name):
        t = I(name, "tile")
        return sum(_cdiv(p[0], t // 1000) * _cdiv(p[1], t % 1000) * p[3] for p in by[name]["prods"])
    # tiles: chosen and forced
    assert I("auto64", "tile") == 64064 and I("auto128", "tile") == 128128 and I("auto256", "tile") == 256128
    assert I("force64", "tile") == 64064 and I("force128", "tile") == 128128 and I("force256", "tile") == 256128
    assert I("t256-above", "tile") == 256128
    # operand scheme
    assert I("small-downgrade", "prec") == P_BF16X3 and I("small-given", "prec") == P_F16X2 and I("big-fp16x2", "prec") == P_F16X2
    assert I("lowp-taken", "prec") == P_F16 and I("lowp-refused", "prec") == P_BF16X3
    assert I("cap-fp16x2", "prec") == P_BF16X3
    # capped launches: the same shapes without a cap take 64-tiles
    assert I("cap-small", "tile") == 64064 and I("cap-not-small", "tile") == 128128 and I("cap-not-small", "G") == 64
    # grid
    assert I("aligned", "aligned") == 1 and I("aligned", "G") == tiles("aligned")
    assert I("aligned-mixed-kt", "aligned") == 0 and len({f["kt"] for f in g["aligned-mixed-kt"]}) == 2
    assert I("forced-grid", "G") == 24 and I("forced-grid", "aligned") == 0
    # hybrid schedule
    assert I("hybrid", "dp_waves") >= 1 and I("hybrid-forward", "dp_waves") == I("hybrid", "dp_waves") - 1 and I("hybrid", "bm") >= 1
    assert I("hybrid-off", "dp_waves") == 0 and I("hybrid-accum", "dp_waves") == 0 and I("hybrid-accum", "aligned") == 0
    assert I("hybrid-accum", "G") == I("hybrid", "G")
    # forward cap
    kts = [int(f["kt"]) for f in g["fwdcap-gmax"]]
    t = I("fwdcap-gmax", "tile")
    iters = sum(_cdiv(p[0], t // 1000) * _cdiv(p[1], t % 1000) * k for p, k in zip(by["fwdcap-gmax"]["prods"], kts))
    assert len(set(kts)) == 3 and I("fwdcap-gmax", "G") == iters // max(kts)
    assert I("fwdcap-pairs", "G") == 2 * tiles("fwdcap-pairs") and I("fwdcap-off", "G") > I("fwdcap-pairs", "G")
    # chunk-major order
    for name in ("chunk", "chunk-tn"):
        assert I(name, "tile") == 64064 and I(name, "kt") == 128 and I(name, "G") == 64 and I(name, "cs") == 8 and I(name, "chunk_iters") == 32
    assert I("chunk-det", "cs") == 0 and I("chunk-off", "cs") == 0 and I("chunk-div", "cs") == 0
    # deterministic mode
    assert I("det-fix", "fix") == 1 and I("det-fix", "zero") == 0 and I("det-fix", "dp_waves") == 1
    assert I("det-clipped", "G") == 256 and I("det-clipped", "fix") == 1 and I("det-unclipped", "G") == 512 and I("det-unclipped", "fix") == 0
    assert I("det-f32", "aligned") == 1 and I("det-f32", "fix") == 0 and I("det-f32", "G") == tiles("det-f32")
    # split tiles
    assert I("zero-vec", "zero") == 1 and I("zero-vec", "zero_vec") == 1 and I("zero-scalar", "zero") == 1 and I("zero-scalar", "zero_vec") == 0
    assert I("ticket", "ticket") == tiles("ticket") and I("ticket", "zero") == 0 and I("zero-scalar", "ticket") == 0
    # nothing to launch, and a refused operand
    assert raw["skipped"] == [] and raw["empty"] == [] and len(raw["skipped-one"]) == 1 and one("skipped-one")["group"] == "0/1"
    assert len(raw["error-ldb"]) == 1 and raw["error-ldb"][0].startswith("error: gemm: leading dimensions") and "ldb=130" in raw["error-ldb"][0]
