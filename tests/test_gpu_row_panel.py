"""GPU tests of the row-panel kernels of ast_amd/csrc/rowgemm.hip -- rowgemm_kernel, lstm_cell_fwd_kernel, lstm_cell_bwd_kernel, each
as <MT, NW> in {1, 2} x {4, 8} -- element by element against the float64 models of tests/row_panel_model.py, through the
astk_debug_rowgemm / astk_debug_lstm_cell_fwd / astk_debug_lstm_cell_bwd hooks of libastk_test.so (the real launchers behind mirror
structs).  The cases are row_panel_model.cases(compute units of the device); the tolerances are row_panel_model.TOL, derived on the host
from the float32 evaluation of the same models (tests/test_row_panel_host.py).

Every operand has a row stride larger than its width and every element outside the live ones -- the padding columns, two rows behind
the last, a band on either side -- holds a NaN of one fixed bit pattern: an output with a NaN has read padding (or was not written), and
a changed pattern around an output was written.  Every launch's route (two row tiles, eight waves, grid) is compared with
row_panel_model.route; the last test asserts that the twelve instantiations all ran."""
import ctypes as C

import numpy as np
import pytest
import torch

import row_panel_model as RP
from test_gpu_ops import stream

pytestmark = pytest.mark.gpu

SENT_BITS = 0x7FDA5A5A             # a quiet NaN with a payload no arithmetic produces
BAND, EXTRA_ROWS = 64, 2
SEEN = set()                       # (kernel, MT, NW) reported by the hooks
WORST = {}                         # quantity -> worst error relative to the reference's maximum
GROUPS = sorted({c.group for c in RP.cases()})
HOOK = {"rowgemm": "astk_debug_rowgemm", "fwd": "astk_debug_lstm_cell_fwd", "bwd": "astk_debug_lstm_cell_bwd"}


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    with _lib.load_test_hooks() as tl:
        v = C.c_double()
        assert tl.astk_get_tuning(b"row.longk", C.byref(v)) == 0 and v.value == RP.LONGK_DEFAULT
        yield tl


@pytest.fixture(scope="module")
def case_list(lib):
    return RP.cases(lib.astk_device_cu_count())


class Pad:
    """[rows][width] float32 in device memory, row stride ld >= width, EXTRA_ROWS rows behind and a band of BAND floats on either side;
    everything but the live elements holds SENT_BITS.  values = None: an output, the live elements hold the pattern too."""

    def __init__(self, rows, width, ld, values=None):
        assert ld >= width
        self.rows, self.width, self.ld, self.n = rows, width, ld, (rows + EXTRA_ROWS) * ld
        host = np.full(BAND + self.n + BAND, SENT_BITS, np.uint32)
        if values is not None:
            host.view(np.float32)[BAND:BAND + self.n].reshape(rows + EXTRA_ROWS, ld)[:rows, :width] = np.asarray(values, np.float32).reshape(rows, width)
        self.live = np.zeros(len(host), bool)
        self.live[BAND:BAND + self.n].reshape(rows + EXTRA_ROWS, ld)[:rows, :width] = True
        self.t = torch.from_numpy(host.view(np.int32)).cuda()
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * BAND

    def fetch(self, what=""):
        """The live elements; asserts that every other element kept its pattern."""
        bits = self.t.cpu().numpy().view(np.uint32)
        bad = int((bits[~self.live] != SENT_BITS).sum())
        assert bad == 0, f"{what}: {bad} elements outside the {self.rows} x {self.width} live ones were written"
        return bits.view(np.float32)[BAND:BAND + self.n].reshape(self.rows + EXTRA_ROWS, self.ld)[:self.rows, :self.width].copy()


def compare(c, q, got, ref, cell=0):
    assert np.isfinite(got).all(), f"{c.name} cell {cell} {q}: {int((~np.isfinite(got)).sum())} elements are not finite (padding read, or not written)"
    e = RP.relerr(got, ref)
    WORST[q] = max(WORST.get(q, 0.0), e)
    assert e <= RP.TOL[q], f"{c.name} cell {cell} {q}: max abs err / max |ref| = {e:.3e} > {RP.TOL[q]:.0e}"


def set_pairs(d, inp, spec, rows, cols, keep):
    for p, (A, W) in enumerate(inp["pairs"]):
        K = spec["Ks"][p]
        d.p[p].K = K
        if K > 0:
            a, w = Pad(rows, K, K + 4, A), Pad(cols, K, K + 8, W)
            keep += [a, w]
            d.p[p].A, d.p[p].lda, d.p[p].W, d.p[p].ldw = a.ptr, a.ld, w.ptr, w.ld
    d.npairs = len(spec["Ks"])


def build_rowgemm(c):
    from ast_amd import _lib as L
    s, inp = c.spec, c.inputs()[0]
    M, N = s["M"], s["N"]
    d, keep, outs = L.DebugRowGemmArgs(), [], {}
    set_pairs(d, inp, s, M, N, keep)
    d.M, d.N, d.act = M, N, s["act"]
    if s["bias"]:
        b = Pad(1, N, N + 4, inp["bias"])
        keep.append(b)
        d.bias = b.ptr
    if s["addend"]:
        a = Pad(M, N, N + 1, inp["addend"])
        keep.append(a)
        d.addend, d.ld_add = a.ptr, a.ld
    outs["out"] = Pad(M, N, N + 3)
    d.out, d.ld_out = outs["out"].ptr, N + 3
    if s["out2"]:
        outs["out2"] = Pad(M, N, N + 5)
        d.out2, d.ld_out2 = outs["out2"].ptr, N + 5
    if s["carry_col0"] is not None:
        w = N - s["carry_col0"]
        outs["carry"] = Pad(M, w, w + 2, inp["carry"])
        aux = Pad(M, w, w + 3, inp["aux"])
        keep.append(aux)
        d.carry, d.ld_carry, d.carry_aux, d.ld_carry_aux, d.carry_col0 = outs["carry"].ptr, w + 2, aux.ptr, w + 3, s["carry_col0"]
    return d, [{q: (o, q) for q, o in outs.items()}], keep


def build_fwd(c):
    from ast_amd import _lib as L
    s = c.spec
    B, h, n = s["B"], s["h"], s["ncells"]
    arr, keep, outs = (L.DebugCellFwdArgs * n)(), [], []
    for i, inp in enumerate(c.inputs()):
        d = arr[i]
        d.struct_size = C.sizeof(L.DebugCellFwdArgs)
        set_pairs(d, inp, s, B, 4 * h, keep)
        d.B, d.h = B, h
        o = {}
        if s["zx"]:
            zx = Pad(B, 4 * h, 4 * h + 8, inp["zx"])
            keep.append(zx)
            d.zx, d.ld_zx = zx.ptr, zx.ld
        gates = zx if s["alias"] else Pad(B, 4 * h, 4 * h + 4)
        o["gates"] = (gates, "gates")
        d.gates, d.ld_g = gates.ptr, gates.ld
        for name in ("bias", "c_prev", "mask"):
            if s[name]:
                buf = Pad(1, 4 * h, 4 * h + 4, inp[name]) if name == "bias" else Pad(B, h, h, inp[name])
                keep.append(buf)
                setattr(d, name, buf.ptr)
        for q, field in (("c", "c_out"), ("h", "h_out")):
            o[q] = (Pad(B, h, h), q)
            setattr(d, field, o[q][0].ptr)
        if s["hd"]:
            o["hd_out"] = (Pad(B, h, h + 3), "hd")
            d.hd_out, d.ld_hd = o["hd_out"][0].ptr, h + 3
        if s["hd2"]:
            o["hd_out2"] = (Pad(B, h, h + 5), "hd")
            d.hd_out2, d.ld_hd2 = o["hd_out2"][0].ptr, h + 5
        outs.append(o)
    return arr, outs, keep


def build_bwd(c):
    from ast_amd import _lib as L
    s = c.spec
    B, h, n = s["B"], s["h"], s["ncells"]
    arr, keep, outs = (L.DebugCellBwdArgs * n)(), [], []
    for i, inp in enumerate(c.inputs()):
        d = arr[i]
        d.struct_size = C.sizeof(L.DebugCellBwdArgs)
        set_pairs(d, inp, s, B, h, keep)
        d.B, d.h = B, h
        for name, ld in (("dy", h + 1), ("dy2", h + 2), ("dh_add", h), ("mask", h), ("dc_next", h), ("c_prev", h), ("c_cur", h)):
            if name == "c_cur" or s[name]:
                buf = Pad(B, h, ld, inp[name])
                keep.append(buf)
                setattr(d, name, buf.ptr)
                if name in ("dy", "dy2"):
                    setattr(d, "ld_" + name, ld)
        o = {"dz": (Pad(B, 4 * h, 4 * h + 4, inp["gates"]), "dz"), "dc_prev": (Pad(B, h, h), "dc_prev")}
        d.gates_dz, d.ld_g, d.dc_prev = o["dz"][0].ptr, 4 * h + 4, o["dc_prev"][0].ptr
        outs.append(o)
    return arr, outs, keep


BUILD = {"rowgemm": build_rowgemm, "fwd": build_fwd, "bwd": build_bwd}


def launch(lib, kind, desc, ncells, route):
    fn = getattr(lib, HOOK[kind])
    if kind == "rowgemm":
        return fn(C.byref(desc), route, stream())
    return fn(desc, ncells, route, stream())


def run_case(lib, tune, c, cu):
    desc, outs, keep = BUILD[c.kind](c)
    tune("row.longk", RP.LONGK_DEFAULT if c.spec["longk"] is None else c.spec["longk"], lib)
    route = (C.c_int32 * 4)()
    rc = launch(lib, c.kind, desc, c.spec.get("ncells", 1), route)
    assert rc == 0, (c.name, lib.astk_last_error().decode())
    assert list(route) == RP.route(c.kind, c.spec, cu), (c.name, list(route), RP.route(c.kind, c.spec, cu))
    SEEN.add(RP.instantiation(c.kind, c.spec, cu))
    for cell, (o, ref) in enumerate(zip(outs, c.run())):
        for field, (buf, q) in o.items():
            compare(c, q, buf.fetch(f"{c.name} cell {cell} {field}"), ref[q], cell)
        assert {q for _, q in o.values()} == set(ref), (c.name, set(ref))
    del keep


@pytest.mark.parametrize("group", GROUPS)
def test_row_panel_kernels_match_the_float64_model(lib, tune, case_list, group):
    cu = lib.astk_device_cu_count()
    mine = [c for c in case_list if c.group == group]
    assert mine
    for c in mine:
        run_case(lib, tune, c, cu)
    if group.endswith("two-tiles"):        # both sides of the decision, whatever the chip's size
        assert {RP.instantiation(c.kind, c.spec, cu)[1] for c in mine} == {1, 2}


def _refused(lib, kind, desc, ncells, outs, what):
    """`outs`: the pure outputs of the call (in-place buffers taken out by the caller): all of them keep the pattern everywhere."""
    route = (C.c_int32 * 4)(7, 7, 7, 7)
    rc = launch(lib, kind, desc, ncells, route)
    assert rc != 0, f"{what}: accepted"
    assert lib.astk_last_error(), what
    assert list(route) == [0, 0, 0, 0] or what.endswith("struct_size") or "ncells" in what, (what, list(route))
    torch.cuda.synchronize()
    for o in outs:
        for buf, _ in o.values():
            assert (buf.t.cpu().numpy().view(np.uint32) == SENT_BITS).all(), f"{what}: refused, yet an output was written"


def test_rowgemm_refusals(lib):
    """Each returns nonzero with a message and launches nothing: the outputs keep their pattern."""
    base = RP._rg("refusals", "base", 5, 7, (12, 8))

    def fresh():
        return build_rowgemm(base)
    for what, edit in (
            ("K not a multiple of 4", lambda d: setattr(d.p[0], "K", 10)),
            ("lda not a multiple of 4", lambda d: setattr(d.p[0], "lda", d.p[0].lda + 2)),
            ("ldw not a multiple of 4", lambda d: setattr(d.p[1], "ldw", d.p[1].ldw + 1)),
            ("misaligned A", lambda d: setattr(d.p[0], "A", d.p[0].A + 4)),
            ("misaligned W", lambda d: setattr(d.p[1], "W", d.p[1].W + 8)),
            ("null A", lambda d: setattr(d.p[0], "A", None)),
            ("npairs 0", lambda d: setattr(d, "npairs", 0)),
            ("npairs 3", lambda d: setattr(d, "npairs", 3)),
            ("M = 0", lambda d: setattr(d, "M", 0)),
            ("N = 0", lambda d: setattr(d, "N", 0)),
            ("null out", lambda d: setattr(d, "out", None)),
            ("struct_size", lambda d: setattr(d, "struct_size", d.struct_size - 8))):
        d, outs, keep = fresh()
        edit(d)
        _refused(lib, "rowgemm", d, 1, outs, what)
    d, outs, keep = fresh()
    route = (C.c_int32 * 4)()
    assert lib.astk_debug_rowgemm(C.byref(d), route, stream()) == 0          # the unedited descriptor is accepted
    assert list(route) == RP.route("rowgemm", base.spec, lib.astk_device_cu_count())
    assert np.isfinite(outs[0]["out"][0].fetch()).all()


def test_cell_refusals(lib):
    from ast_amd import _lib as L
    fw, bw = RP._fw("refusals", "base", 5, 6, (8, 12), ncells=2), RP._bw("refusals", "base", 5, 6, (24, 12), ncells=2)
    for kind, base, build, gates in (("fwd", fw, build_fwd, "gates"), ("bwd", bw, build_bwd, "gates_dz")):
        edits = [("ncells 0", 0, None), ("ncells 9", 9, None),
                 ("cells with different B", 2, lambda a: setattr(a[1], "B", 4)),
                 ("cells with different h", 2, lambda a: setattr(a[1], "h", 5)),
                 ("misaligned " + gates, 2, lambda a: setattr(a[1], gates, getattr(a[1], gates) + 4)),
                 ("ld_g not a multiple of 4", 2, lambda a: setattr(a[0], "ld_g", a[0].ld_g + 2)),
                 ("K not a multiple of 4", 2, lambda a: setattr(a[1].p[1], "K", 10)),
                 ("misaligned W", 2, lambda a: setattr(a[0].p[0], "W", a[0].p[0].W + 4)),
                 ("npairs 3", 2, lambda a: setattr(a[0], "npairs", 3)),
                 ("struct_size", 2, lambda a: setattr(a[1], "struct_size", 8))]
        if kind == "fwd":
            edits += [("misaligned zx", 2, lambda a: setattr(a[0], "zx", a[0].zx + 4)),
                      ("ld_zx not a multiple of 4", 2, lambda a: setattr(a[0], "ld_zx", a[0].ld_zx + 1)),
                      ("misaligned bias", 2, lambda a: setattr(a[1], "bias", a[1].bias + 8)),
                      ("null c_out", 2, lambda a: setattr(a[0], "c_out", None))]
        else:
            edits += [("null c_cur", 2, lambda a: setattr(a[0], "c_cur", None)), ("npairs 0", 2, lambda a: setattr(a[1], "npairs", 0))]
        for what, n, edit in edits:
            arr, outs, keep = build(base)
            if n == 9:                                   # nine descriptors, so that even a launcher that read them all would stay in bounds
                big = (type(arr[0]) * 9)()
                for i in range(9):
                    C.memmove(C.byref(big[i]), C.byref(arr[i % 2]), C.sizeof(arr[0]))
                arr = big
            if edit:
                edit(arr)
            for o in outs:                               # the in-place buffers hold inputs: only the pure outputs can show a write
                o.pop("dz", None)
                if kind == "fwd" and base.spec["alias"]:
                    o.pop("gates", None)
            _refused(lib, kind, arr, n, outs, f"{kind}: {what}")
        arr, outs, keep = build(base)
        route = (C.c_int32 * 4)()
        assert launch(lib, kind, arr, 2, route) == 0, lib.astk_last_error().decode()
        assert list(route) == RP.route(kind, base.spec, lib.astk_device_cu_count())
    assert L.load() is lib


def test_every_instantiation_ran(lib):
    """The route coverage summary: each of the twelve (kernel, MT, NW) instantiations was reported by a hook in this module's run."""
    print({q: f"{e:.2e}" for q, e in sorted(WORST.items())})
    want = {(k, mt, nw) for k in RP.OPS for mt in (1, 2) for nw in (4, 8)}
    assert SEEN == want, sorted(want - SEEN)
    assert set(WORST) == set(RP.TOL)
