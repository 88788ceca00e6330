"""Host tests of the resampling operator.  The model of tests/resample_model.py is the contract and neither sox
nor Kaldi exists to pin it to, so it is pinned independently here: against scipy.signal.upfirdn fed the same taps, against what a
resampler must do to a sine and to a constant, its counts against exact Fraction arithmetic, and the identity at 1/1.  Then the
conditions the named cases must meet, the Python layer's and the command line's pieces that need no GPU, and the declarations and
refusals of the three entry points."""
import ctypes as C
import importlib.util
import math
import os
import pickle
import re
from fractions import Fraction

import numpy as np
import pytest
import scipy.signal

import resample_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = ((9, 10), (11, 10), (1, 2), (2, 1), (441, 80), (1, 1), (3, 2))


# ------------------------------------------------------------------ the model, pinned independently
@pytest.mark.parametrize("p,q,Z,rolloff", [(9, 10, 6, 0.99), (11, 10, 6, 0.99), (1, 2, 6, 0.99), (2, 1, 6, 0.99), (441, 80, 6, 0.99),
                                           (80, 441, 6, 0.99), (3, 2, 16, 0.99), (11, 10, 1, 0.99), (9, 10, 6, 0.5), (1, 1, 6, 1.0)])
def test_model_is_upfirdn_with_the_same_taps(p, q, Z, rolloff):
    """The FIR taps are g(j / q) at the up-sampled rate, j = -Kq .. Kq; upfirdn(up = q, down = p) output m p + K q is y[m].  Bound:
    2K products and sums of relative error 2^-53 each, in two different orders: 2K 2^-50 max |x|."""
    P, Q, c, K = RM.constants(p, q, Z, rolloff)
    rng = np.random.default_rng(p * 131 + q)
    x = RM.gauss(rng, 2 * K + 300)
    h = RM.g(np.arange(-K * Q, K * Q + 1, dtype=np.float64) / Q, c, Z)
    full = scipy.signal.upfirdn(h, x, up=Q, down=1)
    want = RM.resample64(x, p, q, Z, rolloff)
    pick = np.arange(len(want), dtype=np.int64) * P + K * Q
    got = np.where(pick < len(full), full[np.minimum(pick, len(full) - 1)], 0.0)
    assert len(want) == RM.n_out(len(x), p, q)
    err = np.abs(got - want).max()
    print(f"{p}/{q}: K = {K}, model against upfirdn {err:.3e} at max |x| {np.abs(x).max():.0f}")
    assert err <= 2 * K * 2.0 ** -50 * np.abs(x).max(), (p, q, err)


@pytest.mark.parametrize("p,q", RATIOS)
def test_interior_sine_and_dc(p, q):
    """A sine up to 0.4 of the narrower Nyquist comes out as the same sine at the new rate, within 1e-3 of its amplitude, and a constant
    as the same constant within 2e-3, on the interior: at least ceil(K q / p) + 1 output samples from each end."""
    P, Q, c, K = RM.constants(p, q)
    n = 40 * K + 400
    edge = -((-K * Q) // P) + 1
    amp = 3000.0
    for frac in (0.05, 0.2, 0.4):
        f_in = frac * 0.5 * min(1.0, Q / P)                              # cycles per INPUT sample: frac of the narrower Nyquist
        x = amp * np.sin(2.0 * np.pi * f_in * np.arange(n) + 0.3)
        y = RM.resample64(x, p, q)
        t = np.arange(len(y), dtype=np.float64) * P / Q                   # output sample m lies at input time m p / q
        err = np.abs(y - amp * np.sin(2.0 * np.pi * f_in * t + 0.3))[edge:len(y) - edge].max() / amp
        print(f"{p}/{q}: sine at {frac} of the narrower Nyquist, interior error {err:.2e} of the amplitude")
        assert len(y) > 4 * edge and err < 1e-3, (p, q, frac, err)
    y = RM.resample64(np.full(n, amp), p, q)
    dc = np.abs(y / amp - 1.0)[edge:len(y) - edge].max()
    print(f"{p}/{q}: interior DC gain deviation {dc:.2e}")
    assert dc < 2e-3, (p, q, dc)


def test_counts_are_the_exact_fraction():
    for p, q in RATIOS + ((80, 441), (1023, 1024), (8000, 16000), (40, 1), (211, 13)):
        for n in list(range(0, 60)) + [255, 256, 257, 7999, 64000, 2 ** 31 - 1]:
            assert RM.n_out(n, p, q) == math.ceil(Fraction(n) * Fraction(q, p)), (p, q, n)
    assert [RM.n_out(n, 9, 10) for n in (0, 1, 9, 10)] == [0, 2, 10, 12]
    assert RM.reduced(8000, 16000) == (1, 2) and RM.reduced(1000, 1024) == (125, 128) and RM.reduced(1023, 1024) == (1023, 1024)
    assert RM.constants(441, 80)[3] == 34 and RM.constants(9, 10)[2:] == (0.99, 7) and RM.constants(2, 1)[3] == 13


@pytest.mark.parametrize("Z", [1, 6, 16])
def test_unit_ratio_with_rolloff_one_is_the_identity_bit_for_bit(Z):
    tab = RM.table(1, 1, Z, 1.0)
    assert tab.shape == (2 * Z, 1) and tab[Z - 1, 0] == 1.0 and np.count_nonzero(tab) == 1        # g is 1 at 0 and 0 at the other integers
    rng = np.random.default_rng(Z)
    x = (rng.standard_normal(500) * np.exp(rng.uniform(-20, 20, 500))).astype(np.float32)
    assert RM.resample(x, 1, 1, Z, 1.0).tobytes() == x.tobytes()
    assert RM.resample(x, 7, 7, Z, 1.0).tobytes() == x.tobytes()


def test_the_table_is_the_kernel_the_sum_uses():
    for p, q, Z, r in ((9, 10, 6, 0.99), (441, 80, 6, 0.99), (11, 10, 1, 0.99), (2, 1, 16, 0.5)):
        P, Q, c, K = RM.constants(p, q, Z, r)
        tab = RM.table(p, q, Z, r)
        assert tab.shape == (2 * K, Q) and K == math.ceil(Z / c) and K <= RM.MAX_HALF_TAPS
        assert tab[K - 1, 0] == c and (Z < 6 or np.abs(tab.sum(axis=0) - 1.0).max() < 2e-3)   # g(0) = c; every phase has unit DC gain (Z >= 6)
        assert tab[2 * K - 1, 0] == 0.0 or c * K < Z                                          # phase 0's last tap, t = -K: outside the support
    assert np.abs(RM.sinpi(np.arange(-9, 10, dtype=np.float64))).max() == 0.0
    u = np.linspace(-20.0, 20.0, 40001)
    assert np.abs(RM.sinpi(u) - np.sin(np.pi * u)).max() < 1e-14


# ------------------------------------------------------------------ conditions on the cases
def test_the_named_cases_cover_what_they_were_chosen_for():
    T = RM.TILE
    c, (out, counts, n_bad) = RM.result("counts-edge")
    assert c["n_samples"].tolist()[:5] == [0, 0, 1, 2, 6] and counts.tolist() == [0, 0, 2, 3, 7, 3 * T + 1] and n_bad == 0
    for name in ("tile-edge-up", "tile-edge-down"):
        assert RM.result(name)[1][1].tolist() == [T - 1, T, T + 1]
    c, (out, counts, n_bad) = RM.result("mmax-above")
    assert c["Mmax"] > counts.max() + 2 * T and all(c["wave"][b, n:].any() for b, n in enumerate(c["n_samples"].tolist()))
    assert not out[0, counts[0]:].any() and out[0, counts[0] - 1] != 0
    c, (out, counts, n_bad) = RM.result("bad-rows")
    assert c["n_samples"].tolist() == [300, -1, c["wave"].shape[1] + 1, 301, 400, 0] and counts.tolist() == [334, -1, -1, 335, -1, 0]
    assert n_bad == 3 and c["Mmax"] == 335 and not out[[1, 2, 4]].any()
    shapes = {name: RM.constants(RM.case(name)["p"], RM.case(name)["q"], RM.case(name)["num_zeros"], RM.case(name)["rolloff"]) for name in RM.ALL_CASES}
    assert shapes["r441-80"][3] == 34 and shapes["r80-441"][1] == 441 and shapes["r1023-1024"][1] == 1024 == RM.MAX_PHASES
    assert shapes["unreduced-8000-16000"][:2] == (1, 2) and RM.case("unreduced-8000-16000")["p"] == 8000
    # the kernel's four paths: table in LDS or not (2K Q <= 2048 doubles), span in LDS or not ((TILE - 1) P / Q + 1 + 2K <= 4096 doubles)
    paths = {(2 * K * Q <= 2048, (T - 1) * P // Q + 1 + 2 * K <= 4096) for P, Q, _, K in shapes.values()}
    assert paths == {(True, True), (True, False), (False, True), (False, False)}
    assert (2 * shapes["steep-211-13"][3] * 13 > 2048) and shapes["steep-40-1"][3] == 243
    assert {RM.case(n)["num_zeros"] for n in RM.ALL_CASES} == {1, 6, 16} and {RM.case(n)["rolloff"] for n in RM.ALL_CASES} == {0.5, 0.99, 1.0}
    for name in RM.RATIO_CASES:
        assert RM.result(name)[1][1][0] > T, name                        # more than one tile
    c = RM.case("int16-extremes")
    assert c["wave"].dtype == np.int16 and c["wave"].min() == -32768 and c["wave"].max() == 32767
    c = RM.case("float32-nan-behind")
    assert c["wave"].dtype == np.float32 and all(np.isnan(c["wave"][b, n:]).all() and n < c["wave"].shape[1] for b, n in enumerate(c["n_samples"]))
    assert np.isfinite(RM.result("float32-nan-behind")[1][0]).all()
    c = RM.case("int16-max-behind")
    assert all((c["wave"][b, n:] == 32767).all() for b, n in enumerate(c["n_samples"]))
    assert not RM.result("zeros")[1][0].any()
    assert RM.case("impulse-first")["wave"][0, 0] == 32767 and RM.case("impulse-last")["wave"][0, 299] == -32768
    out = RM.result("impulse-first")[1][0][0]
    assert out[0] == np.float32(32767 * 0.99) and np.count_nonzero(out) <= 9          # y[0] = x[0] g(0); the filter's support ends


# ------------------------------------------------------------------ the Python layer and the command line without a GPU
def test_speed_ratio():
    from ast_amd.features import speed_ratio
    assert speed_ratio(0.9) == (9, 10) and speed_ratio(1.1) == (11, 10) and speed_ratio(1.0) == (1, 1) and speed_ratio("1.05") == (21, 20)
    assert speed_ratio(2) == (2, 1) and speed_ratio(0.5) == (1, 2)
    for f in (0.9, 1.1, 1.0, 0.75):
        assert speed_ratio(f) == RM.speed_ratio(f)
    with pytest.raises(ValueError):
        speed_ratio(0)
    with pytest.raises(ValueError):
        speed_ratio(-1.1)


def _cli():
    spec = importlib.util.spec_from_file_location("features_cli", os.path.join(ROOT, "features.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_command_line_flags_and_the_rule_of_the_copies(tmp_path):
    from ast_amd.features import FeatureConfig
    cli = _cli()
    base = ["--scp", "w.scp", "--out", "o", "--set", "dev"]
    a = cli.build_parser().parse_args(base)
    assert (a.resample, a.speed, a.num_zeros, a.rolloff, a.map_in, a.map_out) == (False, None, 6, 0.99, None, None)
    a = cli.build_parser().parse_args(base + ["--resample", "--speed", "0.9,1.0,1.1", "--num-zeros", "16", "--rolloff", "0.95", "--map-in", "m.p",
                                              "--map-out", "m2.p"])
    assert (a.resample, a.speed, a.num_zeros, a.rolloff, a.map_in, a.map_out) == (True, "0.9,1.0,1.1", 16, 0.95, "m.p", "m2.p")
    speeds = cli.parse_speeds(a.speed)
    assert speeds == [("1.0", Fraction(1)), ("0.9", Fraction(9, 10)), ("1.1", Fraction(11, 10))]          # 1.0 first, then as listed
    assert cli.parse_speeds("1.1, 0.9") == [("1.1", Fraction(11, 10)), ("0.9", Fraction(9, 10))]
    for bad in ("0.9,0.90", "abc", "0", "-1.1", "1.0,"):
        with pytest.raises(SystemExit):
            cli.parse_speeds(bad)
    assert cli.copy_name("0.9", Fraction(9, 10), "utt1") == "sp0.9-utt1" and cli.copy_name("1.0", Fraction(1), "utt1") == "utt1"
    assert cli.copy_name("1.1", Fraction(11, 10), "spkA") == "sp1.1-spkA"
    scp = [("b_utt", "b.wav"), ("a_utt", "a.wav")]
    lengths, cfg = {"b_utt": 1000, "a_utt": 801}, FeatureConfig()
    rates = {"b_utt": Fraction(8000), "a_utt": Fraction(16000)}
    copies = cli.plan_copies(scp, lengths, rates, cfg, speeds)
    assert [c["name"] for c in copies] == ["b_utt", "a_utt", "sp0.9-b_utt", "sp0.9-a_utt", "sp1.1-b_utt", "sp1.1-a_utt"]
    assert [c["ratio"] for c in copies] == [Fraction(1), Fraction(2), Fraction(9, 10), Fraction(9, 5), Fraction(11, 10), Fraction(11, 5)]
    want_n = [1000, 401, RM.n_out(1000, 9, 10), RM.n_out(801, 9, 5), RM.n_out(1000, 11, 10), RM.n_out(801, 11, 5)]
    assert [c["n"] for c in copies] == want_n and [c["start"] for c in copies] == [int(v) for v in np.cumsum([0] + want_n[:-1])]
    # the 1.0 copies start where they start without --speed
    plain = cli.plan_copies(scp, lengths, rates, cfg, [("1.0", Fraction(1))])
    assert [(c["name"], c["start"], c["n"]) for c in plain] == [(c["name"], c["start"], c["n"]) for c in copies[:2]]


def test_map_in_map_out_on_a_tiny_pickle(tmp_path):
    cli = _cli()
    m = {"dev": {"u1": {"en_w": ["hello"], "es_w": ["hola"]}, "u2": {"en_w": ["bye"], "es_w": ["adios"]}}, "train": {"t1": {"en_w": ["x"]}}}
    copies = [dict(name=n, utt=u) for n, u in (("u1", "u1"), ("u2", "u2"), ("sp0.9-u1", "u1"), ("sp0.9-u2", "u2"))]
    out = cli.map_copies(m, "dev", copies)
    assert list(out["dev"]) == ["u1", "u2", "sp0.9-u1", "sp0.9-u2"] and out["dev"]["sp0.9-u2"] == m["dev"]["u2"] and out["train"] == m["train"]
    assert pickle.loads(pickle.dumps(out)) == out and list(m["dev"]) == ["u1", "u2"]
    with pytest.raises(SystemExit, match="u3"):                            # a missing utterance is an error that names it
        cli.map_copies(m, "dev", copies + [dict(name="sp0.9-u3", utt="u3")])
    with pytest.raises(SystemExit, match="test"):
        cli.map_copies(m, "test", copies)


# ------------------------------------------------------------------ the library without a GPU
ENTRY_POINTS = {"astk_resample_workspace_bytes": 1, "astk_resample_prepare": 4, "astk_resample": 9}


def test_symbols_are_declared_listed_and_exported():
    from ast_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "astk.h")).read()
    for lib_path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        lib = C.CDLL(lib_path)
        for name in ENTRY_POINTS:
            assert isinstance(getattr(lib, name), C._CFuncPtr), (lib_path, name)
    for name, nargs in ENTRY_POINTS.items():
        decl = re.search(r"\b%s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]) == nargs, name
    decl = re.search(r"int astk_resample\(([^;]*)\);", hdr).group(1)
    assert all(w in decl for w in ("const void* wave", "const int32_t* n_samples", "const void* ws"))          # read-only by declaration
    body = re.search(r"typedef struct \{([^}]*)\} astk_resample_desc;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for stmt in body.split(";") if stmt.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())]
    assert names == [f[0] for f in _lib.ResampleDesc._fields_] == ["struct_size", "B", "Nmax", "Mmax", "sample_type", "p", "q", "num_zeros", "rolloff"]
    assert int(re.search(r"#define ASTK_VERSION (\d+)", hdr).group(1)) >= 113 and _lib.load().astk_version() >= 113
    for macro, value in (("MAX_PHASES", _lib.RESAMPLE_MAX_PHASES), ("MAX_HALF_TAPS", _lib.RESAMPLE_MAX_HALF_TAPS), ("TILE", _lib.RESAMPLE_TILE)):
        assert int(re.search(r"#define ASTK_RESAMPLE_%s (\d+)" % macro, hdr).group(1)) == value == getattr(RM, macro)
    build = open(os.path.join(ROOT, "ast_amd", "csrc", "build.sh")).read()
    srcs, hooked = build.split("SRCS=")[1].split("\n")[0], build.split("HOOKED=")[1].split("\n")[0]
    assert " resample" in srcs and "resample" not in hooked


GOOD = dict(B=2, Nmax=1000, Mmax=1112, sample_type=1, p=9, q=10, num_zeros=6, rolloff=0.99)
REFUSALS = (("B", 0, "B"), ("Nmax", 0, "Nmax"), ("Mmax", 0, "Mmax"), ("p", 0, "p ="), ("q", 0, "q ="), ("p", -3, "p ="), ("q", 1025, "phases"),
            ("p", 1000, "half taps"), ("num_zeros", 0, "num_zeros"), ("num_zeros", 300, "half taps"), ("rolloff", 0.0, "rolloff"),
            ("rolloff", 1.5, "rolloff"), ("rolloff", -0.5, "rolloff"), ("sample_type", 2, "sample_type"), ("sample_type", -1, "sample_type"))


def test_descriptor_refusals_need_no_device():
    """Every refusal comes from the descriptor and the pointers alone, before any launch: with a fake non-null pointer for the buffers
    no device is touched."""
    from ast_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)
    err = lambda: lib.astk_last_error().decode()          # noqa: E731

    def call(d, wave=fake, n=fake, out=fake, n_out=fake, ws=fake, ws_bytes=1 << 30):
        return lib.astk_resample(C.byref(d), wave, n, out, n_out, None, ws, ws_bytes, None)
    for field, value, word in REFUSALS:
        d = _lib.ResampleDesc(**{**GOOD, field: value})
        for rc in (call(d), lib.astk_resample_prepare(C.byref(d), fake, 1 << 30, None)):
            assert rc != 0 and word in err() and "ASTK_" not in err(), (field, value, err())
        assert lib.astk_resample_workspace_bytes(C.byref(d)) == 0, (field, value)
    d = _lib.ResampleDesc(**GOOD)
    need = lib.astk_resample_workspace_bytes(C.byref(d))
    assert need == 256 + 256 * math.ceil(10 * 14 * 8 / 256)                 # the head and 10 phases x 14 taps of float64
    d.struct_size -= 4
    assert call(d) != 0 and "struct_size" in err()
    assert lib.astk_resample_prepare(C.byref(d), fake, need, None) != 0 and "struct_size" in err()
    assert lib.astk_resample_workspace_bytes(C.byref(d)) == 0
    d = _lib.ResampleDesc(**GOOD)
    for kw in (dict(wave=None), dict(n=None), dict(out=None), dict(n_out=None), dict(ws=None)):
        assert call(d, **kw) != 0 and "null" in err(), kw
    assert lib.astk_resample_prepare(C.byref(d), None, need, None) != 0 and "null" in err()
    assert call(d, ws_bytes=need - 1) != 0 and "workspace" in err() and str(need) in err()
    assert lib.astk_resample_prepare(C.byref(d), fake, need - 1, None) != 0 and "workspace" in err()
    assert call(d) != 0 and "never prepared" in err()                    # a workspace the library has not filled
    # the widest shapes are descriptors the library accepts; an unreduced pair is reduced before the bound on the phases
    for kw in (dict(p=1023, q=1024), dict(p=8000, q=16000), dict(p=40, q=1), dict(num_zeros=253, rolloff=1.0), dict(p=1, q=1, rolloff=1.0),
               dict(p=2048, q=2046)):
        assert lib.astk_resample_workspace_bytes(C.byref(_lib.ResampleDesc(**{**GOOD, **kw}))) > 0, kw
