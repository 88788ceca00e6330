"""GPU tests of the resampling operator (include/astk.h astk_resample*): the operator through the C ABI on the
named cases of tests/resample_model.py, then the Python layer and the command line.

The bound is derived, not measured: kernel and model round one float64 sum once to float32.  Their float64 values differ by the
contraction of product and sum into a fused multiply-add and by the device's sinpi / cospi against NumPy's sin(pi u): each at most
about 4e-15 absolute per tap (the weights are at most 1), so at most about 2e-12 amax over 512 taps, where amax is the row's largest
|sample|.  The float32 unit at the floor 2^-12 amax is 2.9e-11 amax: every element lies within ONE float32 unit in the last place at
max(|model|, 2^-12 amax_row) of the model rounded to float32, nothing excluded.

Measured on an MI355X: on 27 of the 28 cases every element equals the model bit for bit; on the full-scale tone 19 of 778 elements
differ, where the sum cancels to a residue near 1e-12, by at most 2.9e-19 amax (1e-8 of the unit at the floor).  The floor stays at
the stated 2^-12 amax: how small the residues are depends on NumPy's sin as much as on the kernel."""
import ctypes as C
import importlib.util
import os
import pickle
import wave

import numpy as np
import pytest
import torch

import resample_model as RM
import speech_features_model as SM
from test_gpu_ops import GuardedWS, dev, ok, stream, vp
from test_resample_host import REFUSALS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -7.0


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


def _desc(c, sample_type):
    from ast_amd import _lib
    B, Nmax = c["wave"].shape
    return _lib.ResampleDesc(B=B, Nmax=Nmax, Mmax=c["Mmax"], sample_type=sample_type, p=c["p"], q=c["q"], num_zeros=c["num_zeros"],
                             rolloff=c["rolloff"])


def _prepared(lib, d):
    nbytes = int(lib.astk_resample_workspace_bytes(C.byref(d)))
    assert nbytes > 0, lib.astk_last_error().decode()
    ws = GuardedWS(nbytes)
    ok(lib, lib.astk_resample_prepare(C.byref(d), C.c_void_p(ws.data_ptr()), nbytes, stream()))
    return ws


def _run_op(lib, c, with_n_bad=True, spare_rows=2, as_float32=False):
    """astk_resample on one case's host arrays: the (B + spare_rows, Mmax) buffer, n_out (B + 2) and n_bad as host arrays, and whether
    the inputs came through unchanged."""
    B = len(c["n_samples"])
    host = c["wave"].astype(np.float32) if as_float32 else c["wave"]
    ins = [torch.from_numpy(np.array(host)).to("cuda"), dev(np.array(c["n_samples"]), torch.int32)]
    before = [t.clone() for t in ins]
    d = _desc(c, 1 if host.dtype == np.int16 else 0)
    ws = _prepared(lib, d)
    out = torch.full((B + spare_rows, c["Mmax"]), FILL, dtype=torch.float32, device="cuda")
    n_out = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    n_bad = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    ok(lib, lib.astk_resample(C.byref(d), vp(ins[0]), vp(ins[1]), vp(out), vp(n_out), C.c_void_p(n_bad.data_ptr() + 4) if with_n_bad else None,
                              C.c_void_p(ws.data_ptr()), ws.nbytes, stream()))
    ws.check("resample")
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(before, ins))
    return dict(out=out.cpu().numpy(), n_out=n_out.cpu().numpy(), n_bad=n_bad.cpu().numpy(), inputs_unchanged=same)


def _amax_rows(c):
    """The largest |sample| inside each row's length (0 for an empty or a bad row)."""
    Nmax = c["wave"].shape[1]
    return np.asarray([np.abs(c["wave"][b, :n].astype(np.float64)).max() if 0 < n <= Nmax else 0.0 for b, n in enumerate(c["n_samples"].tolist())])


def _ulps(got, want, amax):
    """|got - want| in float32 units in the last place at max(|want|, 2^-12 amax_row); a row of zeros (amax 0) must be exactly zero."""
    floor = (2.0 ** -12 * amax).astype(np.float32)[:, None]
    at = np.maximum(np.abs(want), floor)
    unit = np.spacing(at.astype(np.float32)).astype(np.float64)
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return np.where(at > 0, diff / np.where(at > 0, unit, 1.0), np.where(diff > 0, np.inf, 0.0))


@pytest.mark.parametrize("name", RM.ALL_CASES)
def test_resample_equals_the_model_to_one_float32_unit(lib, name):
    c, (want, want_n, want_bad) = RM.result(name)
    B = len(want_n)
    r = _run_op(lib, c)
    assert r["n_out"].tolist() == want_n.tolist() + [-7, -7], (name, r["n_out"])
    assert r["n_bad"].tolist() == [-7, want_bad, -7], (name, r["n_bad"])
    got = r["out"][:B]
    assert np.isfinite(got).all(), name
    u = _ulps(got, want, _amax_rows(c))
    amax = _amax_rows(c)
    rel = (np.abs(got.astype(np.float64) - want) / np.where(amax > 0, amax, 1.0)[:, None]).max()
    print(f"{name}: worst {u.max():.6f} units ({int((got != want).sum())} of {got.size} elements differ from the model, by at most "
          f"{rel:.2e} of the row's largest sample)")
    assert u.max() <= 1.0, (name, float(u.max()), np.argwhere(u > 1.0)[:4].tolist())
    for b, M in enumerate(want_n.tolist()):
        assert not got[b, max(M, 0):].any(), (name, b, "samples behind n_out are not zero")
    assert (r["out"][B:] == FILL).all(), "rows behind B were written"
    assert r["inputs_unchanged"], "an input buffer was written"


def test_rows_of_zeros_are_exactly_zero(lib):
    for name in RM.ZERO_ROW_CASES + ("counts-edge", "bad-rows"):
        c, (want, want_n, _) = RM.result(name)
        got = _run_op(lib, c)["out"]
        for b, n in enumerate(c["n_samples"].tolist()):
            if want_n[b] < 0 or not c["wave"][b, :max(n, 0)].any():
                assert got[b].tobytes() == np.zeros_like(got[b]).tobytes(), (name, b)
    assert not _run_op(lib, RM.case("zeros"))["out"][:2].any()


@pytest.mark.parametrize("name", ["counts-edge", "bad-rows", "r441-80", "r1023-1024", "steep-211-13"])
def test_two_runs_give_identical_bytes_and_n_bad_is_optional(lib, name):
    c = RM.case(name)
    a, b = _run_op(lib, c), _run_op(lib, c, with_n_bad=False)
    assert a["out"].tobytes() == b["out"].tobytes() and a["n_out"].tobytes() == b["n_out"].tobytes()
    assert b["n_bad"].tolist() == [-7] * 3


@pytest.mark.parametrize("name", ["counts-edge", "int16-extremes", "bad-rows", "steep-40-1"])
def test_int16_and_float32_input_of_the_same_integers_give_identical_bytes(lib, name):
    c = RM.case(name)
    assert c["wave"].dtype == np.int16
    a, b = _run_op(lib, c), _run_op(lib, c, as_float32=True)
    assert a["out"].tobytes() == b["out"].tobytes() and a["n_out"].tolist() == b["n_out"].tolist()


def test_unit_ratio_with_rolloff_one_is_the_identity_on_the_device(lib):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 700)) * np.exp(rng.uniform(-20, 20, (2, 700)))).astype(np.float32)
    c = dict(wave=x, n_samples=np.asarray([700, 333], np.int32), p=3, q=3, num_zeros=6, rolloff=1.0, Mmax=700)
    r = _run_op(lib, c)
    assert r["out"][0].tobytes() == x[0].tobytes() and r["out"][1, :333].tobytes() == x[1, :333].tobytes() and not r["out"][1, 333:].any()


def test_refusals_launch_nothing_and_a_foreign_workspace_is_refused(lib):
    from ast_amd import _lib
    c, (want, want_n, _) = RM.result("r9-10")
    B = len(want_n)
    wave_t, n = torch.from_numpy(np.array(c["wave"])).to("cuda"), dev(c["n_samples"], torch.int32)
    d = _desc(c, 1)
    ws = _prepared(lib, d)
    out = torch.full((B, c["Mmax"]), FILL, dtype=torch.float32, device="cuda")
    n_out = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    n_bad = torch.full((1,), -7, dtype=torch.int32, device="cuda")

    def call(d, ws=ws):
        return lib.astk_resample(C.byref(d), vp(wave_t), vp(n), vp(out), vp(n_out), vp(n_bad), C.c_void_p(ws.data_ptr()), ws.nbytes, stream())

    def untouched():
        torch.cuda.synchronize()
        assert int((out != FILL).sum()) == 0 and (n_out == -7).all() and int(n_bad[0]) == -7, "the refused call launched something"

    def reset():
        out.fill_(FILL)
        n_out.fill_(-7)
        n_bad.fill_(-7)
    base = {f[0]: getattr(d, f[0]) for f in d._fields_[1:]}
    for field, value, word in REFUSALS:
        bad = _lib.ResampleDesc(**{**base, field: value})
        assert call(bad) != 0 and word in lib.astk_last_error().decode(), (field, lib.astk_last_error().decode())
        untouched()
    # a workspace prepared for other table fields (11/10: as many bytes), and one that was never prepared
    other = _lib.ResampleDesc(**{**base, "p": 11})
    ws_other = _prepared(lib, other)
    assert ws_other.nbytes == ws.nbytes
    assert call(d, ws=ws_other) != 0 and "different descriptor" in lib.astk_last_error().decode()
    untouched()
    # A workspace nobody prepared.  The host's table goes by address, so a fresh buffer is refused by message -- "never prepared", or
    # "different descriptor" when the allocator hands out an address an earlier test prepared -- unless that address was prepared for
    # this very table: then the kernel finds no digest in the head and makes every row a bad row.
    fresh = GuardedWS(ws.nbytes)
    if call(d, ws=fresh) != 0:
        assert any(w in lib.astk_last_error().decode() for w in ("never prepared", "different descriptor"))
        untouched()
    else:
        torch.cuda.synchronize()
        assert (n_out == -1).all() and int(n_bad[0]) == B and not out.any()
        reset()
    fresh.check("resample")
    # the fields the table does not depend on may change between prepare and the call; an unreduced pair names the same table
    assert call(_lib.ResampleDesc(**{**base, "p": 18, "q": 20})) == 0
    torch.cuda.synchronize()
    assert _ulps(out.cpu().numpy(), want, _amax_rows(c)).max() <= 1.0 and n_out.tolist() == want_n.tolist() and int(n_bad[0]) == 0
    # the kernel looks at the head again: a prepared workspace that was overwritten since makes every row a bad row
    ws.t[:64] = 0
    reset()
    assert call(d) == 0
    torch.cuda.synchronize()
    assert (n_out == -1).all() and int(n_bad[0]) == B and not out.any()
    ws.check("resample")


# ------------------------------------------------------------------ the Python layer
def _waves(seed, lens):
    rng = np.random.default_rng(seed)
    return [RM.gauss(rng, n).astype(np.int16) for n in lens]


def _pack(waves, dtype=np.int16):
    host = np.zeros((len(waves), max(1, max(len(w) for w in waves))), dtype)
    for b, w in enumerate(waves):
        host[b, :len(w)] = w
    return torch.from_numpy(host).to("cuda"), torch.tensor([len(w) for w in waves], dtype=torch.int32, device="cuda")


def test_resample_on_a_ragged_batch_equals_per_row_calls():
    from ast_amd import features as F
    waves = _waves(12, (840, 1, 0, 257, 2000, 1234))
    wave, n = _pack(waves)
    for p, q in ((9, 10), (11, 10), (2, 1), (16000, 8000)):
        Y, n_out = F.resample(wave, n, p, q)
        assert Y.shape == (6, RM.n_out(2000, p, q)) and Y.dtype == torch.float32 and n_out.tolist() == [RM.n_out(len(w), p, q) for w in waves]
        for b, w in enumerate(waves):
            Yb, nb = F.resample(*_pack([w]), p, q)
            m = int(nb[0])
            assert m == int(n_out[b]) and torch.equal(Yb[0, :m], Y[b, :m]) and not Y[b, m:].any()
            want = RM.resample(w, p, q)[None]
            assert m == 0 or _ulps(Y[b:b + 1, :m].cpu().numpy(), want, np.asarray([np.abs(w.astype(np.float64)).max() if len(w) else 0.0])).max() <= 1.0
    Y9, _ = F.resample(wave, n, 9, 10)
    assert torch.equal(F.resample(wave.float(), n, 9, 10)[0], Y9)
    assert len({k[:2] for k in F._RESAMPLE_WORKSPACES}) >= 3 and (2, 1) in {k[:2] for k in F._RESAMPLE_WORKSPACES}       # 16000/8000 is 2/1
    Z16, _ = F.resample(wave, n, 9, 10, num_zeros=16, rolloff=0.95)                                  # another table, another cache entry
    assert Z16.shape == Y9.shape and not torch.equal(Z16, Y9)
    want = RM.resample(waves[4], 9, 10, 16, 0.95)[None]
    assert _ulps(Z16[4:5, :len(want[0])].cpu().numpy(), want, np.asarray([np.abs(waves[4].astype(np.float64)).max()])).max() <= 1.0
    with pytest.raises(ValueError):
        F.resample(wave, n, 0, 10)
    with pytest.raises(ValueError):
        F.resample(wave.cpu(), n, 9, 10)
    with pytest.raises(ValueError):
        F.resample(wave, n.long(), 9, 10)


def test_compute_is_compute_device_on_the_packed_list():
    from ast_amd import features as F
    waves = _waves(13, (840, 150, 200, 4000, 1234))
    for cfg in (F.FeatureConfig(), F.FeatureConfig(dither=1.0), F.FeatureConfig(kind="fbank", sample_frequency=16000.0, num_mel_bins=80)):
        offsets = [5, 0, 77, 123456, 9]
        X, nf = F.compute(waves, cfg, "cuda", seed=3, offsets=offsets)
        wave, n = _pack(waves)
        Xd, nd = F.compute_device(wave, n, cfg, seed=3, offsets=offsets)
        assert X.shape == Xd.shape == (5, max(1, cfg.frames(4000)), cfg.dim) and torch.equal(nf, nd)
        assert X.cpu().numpy().tobytes() == Xd.cpu().numpy().tobytes()
        Xt, _ = F.compute_device(wave, n, cfg, seed=3, offsets=torch.tensor(offsets, dtype=torch.int64, device="cuda"))
        assert torch.equal(Xt, Xd)
    X0, nf0 = F.compute(waves, F.FeatureConfig(), "cuda")
    assert nf0.tolist() == [F.FeatureConfig().frames(len(w)) for w in waves]
    want = SM.features(waves[0], SM.config()).astype(np.float32)
    assert np.abs(X0[0, :want.shape[0]].cpu().numpy() - want).max() <= np.spacing(np.float32(np.abs(want).max()))
    # a longer buffer than the longest row: more frames per row of X, the same frames
    wave, n = _pack(waves + [np.zeros(6000, np.int16)])
    Xl, nl = F.compute_device(wave[:5].contiguous(), n[:5].contiguous(), F.FeatureConfig())
    assert Xl.shape[1] == F.FeatureConfig().frames(6000) and torch.equal(Xl[:, :X0.shape[1]], X0) and not Xl[:, X0.shape[1]:].any()


def test_a_slowed_tone_has_the_features_of_the_lower_tone():
    """compute_device(resample(1000 Hz tone, speed 0.9)): read at the original rate the tone is a 900 Hz tone, and on every interior frame
    the largest log mel energy lies in the bin where an analytic 900 Hz tone has it."""
    from ast_amd import features as F
    cfg = F.FeatureConfig(kind="fbank", num_mel_bins=23)
    n = 8000
    x = RM.tone(n, 1000.0, 8000.0, 20000.0).astype(np.int16)
    p, q = F.speed_ratio(0.9)
    Y, n_out = F.resample(*_pack([x]), p, q)
    assert int(n_out[0]) == RM.n_out(n, 9, 10) == 8889
    X, nf = F.compute_device(Y, n_out, cfg)
    ref, nr = F.compute([RM.tone(8889, 900.0, 8000.0, 20000.0).astype(np.int16), x], cfg, "cuda")
    frames = int(nf[0])
    assert frames == int(nr[0]) == cfg.frames(8889) and frames > 100
    got, want, orig = X[0, :frames].argmax(dim=1), ref[0, :frames].argmax(dim=1), ref[1, :cfg.frames(n)].argmax(dim=1)
    assert torch.equal(got[2:-2], want[2:-2]) and len(set(want.tolist())) == 1
    assert int(orig[5]) != int(want[5])                                   # ... and not where the 1000 Hz tone has it


# ------------------------------------------------------------------ the command line
def _write_wav(path, data, rate=8000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(data).astype("<i2").tobytes())


def _cli():
    spec = importlib.util.spec_from_file_location("features_cli", os.path.join(ROOT, "features.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def _load(out_dir, names):
    return {u: np.load(os.path.join(out_dir, "dev", f"{u}.npy")) for u in names}


def test_command_line_resample_equals_the_calls_by_hand(tmp_path):
    from ast_amd import features as F
    cli = _cli()
    lens = {"a16": 4100, "b16": 1700, "c8": 1300, "d16": 2500}
    waves = dict(zip(lens, _waves(22, lens.values())))
    for u, w in waves.items():
        _write_wav(tmp_path / f"{u}.wav", w, rate=8000 if u == "c8" else 16000)
    (tmp_path / "wav.scp").write_text("".join(f"{u} {tmp_path / (u + '.wav')}\n" for u in lens))
    base = ["--scp", str(tmp_path / "wav.scp"), "--set", "dev", "--dither", "1", "--seed", "4"]
    with pytest.raises(ValueError, match=r"a16\.wav.*16000"):             # without the flag the wrong rate stays an error that names the file
        cli.main(base + ["--out", str(tmp_path / "o0")])
    assert cli.main(base + ["--out", str(tmp_path / "o1"), "--resample", "-b", "2", "--info-out", str(tmp_path / "o1.info")]) == 0
    got = _load(tmp_path / "o1", lens)
    cfg = F.FeatureConfig(dither=1.0)
    n8 = {u: (RM.n_out(n, 2, 1) if u != "c8" else n) for u, n in lens.items()}
    starts = dict(zip(lens, np.cumsum([0] + list(n8.values())[:-1]).tolist()))
    for u in ("a16", "b16", "d16"):
        Y, n_out = F.resample(*_pack([waves[u]]), 16000, 8000)
        X, nf = F.compute_device(Y, n_out, cfg, seed=4, offsets=[starts[u]])
        assert int(n_out[0]) == n8[u] and got[u].tobytes() == X[0, :int(nf[0])].cpu().numpy().tobytes(), u
    X, nf = F.compute([waves["c8"]], cfg, "cuda", seed=4, offsets=[starts["c8"]])
    assert got["c8"].tobytes() == X[0, :int(nf[0])].cpu().numpy().tobytes()
    with open(tmp_path / "o1.info", "rb") as f:
        info = pickle.load(f)
    assert list(info["dev"]) == list(lens) and all(info["dev"][u] == {"sp": cfg.frames(n8[u])} == {"sp": got[u].shape[0]} for u in lens)


def test_command_line_speed_copies_follow_the_rule(tmp_path):
    from ast_amd import features as F
    from ast_amd.dataloader import FisherDataLoader
    cli = _cli()
    lens = {"spkA_0001": 2040, "spkB_0001": 840, "spkA_0002": 1400}
    spk = {"spkA_0001": "spkA", "spkB_0001": "spkB", "spkA_0002": "spkA"}
    waves = dict(zip(lens, _waves(23, lens.values())))
    for u, w in waves.items():
        _write_wav(tmp_path / f"{u}.wav", w)
    (tmp_path / "wav.scp").write_text("".join(f"{u} {tmp_path / (u + '.wav')}\n" for u in lens))
    (tmp_path / "utt2spk").write_text("".join(f"{u} {s}\n" for u, s in spk.items()))
    with open(tmp_path / "map.p", "wb") as f:
        pickle.dump({"dev": {u: {"en_w": [u.lower()]} for u in lens}, "train": {"x": {"en_w": ["y"]}}}, f)
    base = ["--scp", str(tmp_path / "wav.scp"), "--set", "dev", "--dither", "1", "--seed", "7", "--cmvn", "utt", "--norm-vars"]
    speed = ["--speed", "0.9,1.0,1.1"]
    names = list(lens) + [f"sp{f}-{u}" for f in ("0.9", "1.1") for u in lens]
    outs = {}
    for b in (2, 1):
        out = tmp_path / f"s{b}"
        assert cli.main(base + speed + ["--out", str(out), "-b", str(b), "--info-out", str(out / "dev.info"), "--map-in", str(tmp_path / "map.p"),
                                        "--map-out", str(out / "map.p")]) == 0
        assert sorted(os.listdir(out / "dev")) == sorted(f"{u}.npy" for u in names)
        outs[b] = _load(out, names)
    for u in names:                                                       # the output does not depend on -b, with dither
        assert outs[1][u].tobytes() == outs[2][u].tobytes() and outs[1][u].dtype == np.float32, u
    assert cli.main(base + ["--out", str(tmp_path / "plain"), "-b", "2"]) == 0
    plain = _load(tmp_path / "plain", lens)
    for u in lens:                                                        # the 1.0 copies are the run without --speed
        assert plain[u].tobytes() == outs[2][u].tobytes(), u
    cfg = F.FeatureConfig()
    with open(tmp_path / "s2" / "dev.info", "rb") as f:
        info = pickle.load(f)
    assert list(info["dev"]) == list(lens) + [f"sp{f}-{u}" for f in ("0.9", "1.1") for u in lens]       # 1.0 first, then as listed
    for f, (p, q) in (("0.9", (9, 10)), ("1.1", (11, 10))):
        for u, n in lens.items():
            name = f"sp{f}-{u}"
            assert info["dev"][name] == {"sp": cfg.frames(RM.n_out(n, p, q))} == {"sp": outs[2][name].shape[0]}, name
    with open(tmp_path / "s2" / "map.p", "rb") as f:
        m = pickle.load(f)
    assert list(m["dev"]) == list(info["dev"]) and m["dev"]["sp1.1-spkB_0001"] == {"en_w": ["spkb_0001"]} and m["train"] == {"x": {"en_w": ["y"]}}
    loader = FisherDataLoader.__new__(FisherDataLoader)                   # the perturbed set loads
    loader.data_cfg = {"speech_path": str(tmp_path / "s2"), "zero_input": 0}
    assert loader._speech("sp0.9-spkA_0002", "dev", 10 ** 6).tobytes() == outs[2]["sp0.9-spkA_0002"].tobytes()
    with open(tmp_path / "short.p", "wb") as f:
        pickle.dump({"dev": {"spkA_0001": {}, "spkB_0001": {}}}, f)
    with pytest.raises(SystemExit, match="spkA_0002"):
        cli.main(base + speed + ["--out", str(tmp_path / "x"), "--map-in", str(tmp_path / "short.p"), "--map-out", str(tmp_path / "x.p")])
    # --cmvn spk: a perturbed speaker is a new speaker.  Without --norm-vars every group's frames sum to zero per coefficient, over
    # sp0.9-spkA's two utterances together and not over either alone; the unperturbed speakers are the run without --speed.
    spk_args = ["--scp", str(tmp_path / "wav.scp"), "--set", "dev", "--cmvn", "spk", "--utt2spk", str(tmp_path / "utt2spk")]
    assert cli.main(spk_args + ["--speed", "1.0,0.9", "--out", str(tmp_path / "k")]) == 0
    assert cli.main(spk_args + ["--out", str(tmp_path / "k0")]) == 0
    k, k0 = _load(tmp_path / "k", list(lens) + [f"sp0.9-{u}" for u in lens]), _load(tmp_path / "k0", lens)
    for u in lens:
        assert k[u].tobytes() == k0[u].tobytes(), u
    for group in (["spkA_0001", "spkA_0002"], ["spkB_0001"], ["sp0.9-spkA_0001", "sp0.9-spkA_0002"], ["sp0.9-spkB_0001"]):
        rows = np.concatenate([k[u].astype(np.float64) for u in group])
        scale = max(np.abs(k[u]).max() for u in group)
        assert np.abs(rows.mean(axis=0)).max() < 1e-5 * scale, group      # float32 rounding of each normalised value: 6e-8 of the scale
    assert np.abs(k["sp0.9-spkA_0001"].astype(np.float64).mean(axis=0)).max() > 1e-3
