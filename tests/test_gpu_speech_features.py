"""GPU tests of the speech features and CMVN (include/astk.h astk_speech_features, astk_cmvn_*): the operators
through the C ABI on the named cases of tests/speech_features_model.py, then the Python layer, the command line and one end-to-end run
into encode_rows.

The feature bound is derived, not measured: kernel and model round the same float64 quantity once to float32; their float64 values
differ by the reordering of sums (1.4e-10 at worst on these signals, measured on the host with a reversed-order DFT) and by the device's
double log / cos / pow (a few units of 2^-53), so the float32 results can differ only where that lands on a rounding boundary: by one
unit in the last place at max(|model|, 1), on every element, nothing excluded."""
import ctypes as C
import importlib.util
import os
import pickle
import wave

import numpy as np
import pytest
import torch

import speech_features_model as SM
from conftest import tiny_cfg
from test_gpu_ops import GuardedWS, dev, ok, stream, vp
from test_speech_features_host import CMVN_GOOD, GOOD, REFUSALS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -7.0


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


def _desc(c, sample_type, offsets=None):
    from ast_amd import _lib
    cfg = c["cfg"]
    B, Nmax = c["wave"].shape
    return _lib.SpeechFeaturesDesc(
        B=B, Nmax=Nmax, Fmax=c["Fmax"], sample_type=sample_type, kind=1 if cfg["kind"] == "fbank" else 0,
        window=_lib.FEAT_WINDOWS[cfg["window_type"]], frame_len=cfg["frame_len"], frame_shift=cfg["frame_shift_samples"],
        num_mel_bins=cfg["num_mel_bins"], num_ceps=cfg["num_ceps"] if cfg["kind"] == "mfcc" else 0, remove_dc_offset=int(cfg["remove_dc_offset"]),
        use_energy=int(cfg["use_energy"]), sample_frequency=cfg["sample_frequency"], low_freq=cfg["low_freq"], high_freq=cfg["high_freq"],
        preemphasis=cfg["preemphasis_coefficient"], cepstral_lifter=cfg["cepstral_lifter"], dither=cfg["dither"], seed=c["seed"],
        offsets=offsets)


def _prepared(lib, d):
    nbytes = int(lib.astk_speech_features_workspace_bytes(C.byref(d)))
    assert nbytes > 0, lib.astk_last_error().decode()
    ws = GuardedWS(nbytes)
    ok(lib, lib.astk_speech_features_prepare(C.byref(d), C.c_void_p(ws.data_ptr()), nbytes, stream()))
    return ws


def _run_op(lib, c, with_n_bad=True, spare_rows=2, as_float32=False):
    """astk_speech_features on one case's host arrays: the (B + spare_rows, Fmax, D) buffer, n_frames (B + 2) and n_bad as host arrays,
    the inputs before and after."""
    B, D = len(c["n_samples"]), SM.dim(c["cfg"])
    host = c["wave"].astype(np.float32) if as_float32 else c["wave"]
    wave_t = torch.from_numpy(np.array(host)).to("cuda")
    ins = [wave_t, dev(np.array(c["n_samples"]), torch.int32), dev(np.array(c["offsets"]), torch.int64)]
    before = [t.clone() for t in ins]
    d = _desc(c, 1 if host.dtype == np.int16 else 0, ins[2].data_ptr() if c["with_offsets"] else None)
    ws = _prepared(lib, d)
    feats = torch.full((B + spare_rows, c["Fmax"], D), FILL, dtype=torch.float32, device="cuda")
    n_frames = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    n_bad = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    ok(lib, lib.astk_speech_features(C.byref(d), vp(ins[0]), vp(ins[1]), vp(feats), vp(n_frames),
                                     C.c_void_p(n_bad.data_ptr() + 4) if with_n_bad else None, C.c_void_p(ws.data_ptr()), ws.nbytes, stream()))
    ws.check("speech_features")
    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(before, ins))
    return dict(feats=feats.cpu().numpy(), n_frames=n_frames.cpu().numpy(), n_bad=n_bad.cpu().numpy(), inputs_unchanged=same)


def _ulps(got, want):
    """|got - want| in float32 units in the last place at max(|want|, 1)."""
    unit = np.spacing(np.maximum(np.abs(want), np.float32(1)).astype(np.float32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / unit


@pytest.mark.parametrize("name", SM.ALL_CASES)
def test_features_equal_the_model_to_one_float32_unit(lib, name):
    c, (want, want_nf, want_bad) = SM.result(name)
    B = len(want_nf)
    r = _run_op(lib, c)
    assert r["n_frames"].tolist() == want_nf.tolist() + [-7, -7], (name, r["n_frames"])
    assert r["n_bad"].tolist() == [-7, want_bad, -7], (name, r["n_bad"])
    got = r["feats"][:B]
    assert np.isfinite(got).all(), name
    u = _ulps(got, want)
    print(f"{name}: worst {u.max():.3f} units ({int((u > 0).sum())} of {u.size} elements differ), largest |model| {np.abs(want).max():.3f}")
    assert u.max() <= 1.0, (name, float(u.max()), np.argwhere(u > 1.0)[:4].tolist())
    for b, F in enumerate(want_nf.tolist()):
        assert not got[b, max(F, 0):].any(), (name, b, "frames behind F_b are not zero")
    assert (r["feats"][B:] == FILL).all(), "rows behind B were written"
    assert r["inputs_unchanged"], "an input buffer was written"


@pytest.mark.parametrize("name", SM.EXACT_ZERO_CASES + ("len2",))
def test_frames_of_exact_zeros_equal_the_model_bit_for_bit(lib, name):
    c, (want, want_nf, _) = SM.result(name)
    got = _run_op(lib, c)["feats"][:len(want_nf)]
    checked = 0
    for b, n in enumerate(c["n_samples"].tolist()):
        if want_nf[b] <= 0:
            continue
        E, _ = SM.mel_energies(c["wave"][b, :n], c["cfg"])
        silent = np.flatnonzero((E == 0.0).all(axis=1))
        checked += silent.size
        assert got[b, silent].tobytes() == want[b, silent].tobytes(), (name, b, np.abs(got[b, silent] - want[b, silent]).max())
    assert checked > 0, name
    if name in ("constant", "zeros", "len2"):                # every frame of row 0 is silent: the whole row equals the model exactly
        assert got[0].tobytes() == want[0].tobytes()


@pytest.mark.parametrize("name", ["counts-workgroup", "bad-rows", "16k-fbank80", "len1200", "dither-seed1"])
def test_two_runs_give_identical_bytes_and_n_bad_is_optional(lib, name):
    c = SM.case(name)
    a, b = _run_op(lib, c), _run_op(lib, c, with_n_bad=False)
    assert a["feats"].tobytes() == b["feats"].tobytes() and a["n_frames"].tobytes() == b["n_frames"].tobytes()
    assert b["n_bad"].tolist() == [-7] * 3


@pytest.mark.parametrize("name", ["counts-edge", "int16-extremes", "bad-rows"])
def test_int16_and_float32_input_of_the_same_integers_give_identical_bytes(lib, name):
    c = SM.case(name)
    assert c["wave"].dtype == np.int16
    a, b = _run_op(lib, c), _run_op(lib, c, as_float32=True)
    assert a["feats"].tobytes() == b["feats"].tobytes() and a["n_frames"].tolist() == b["n_frames"].tolist()


def test_a_sample_carries_the_same_dither_in_every_frame(lib):
    """Zero samples with dither: frame t of a row at offset o is frame 0 of the same row at offset o + t * shift."""
    c = dict(SM.case("dither-seed1"))
    n = SM.n_for(3, c["cfg"])
    first = _run_op(lib, {**c, "wave": np.zeros((1, n), np.int16), "n_samples": np.asarray([n], np.int32), "offsets": np.asarray([7], np.int64),
                          "Fmax": 3})["feats"][0]
    later = _run_op(lib, {**c, "wave": np.zeros((1, n), np.int16), "n_samples": np.asarray([n - 80], np.int32),
                          "offsets": np.asarray([87], np.int64), "Fmax": 3})["feats"][0]
    assert first[1:3].tobytes() == later[0:2].tobytes() and first[0].tobytes() != first[1].tobytes() and not later[2].any()


def test_refusals_launch_nothing_and_a_foreign_workspace_is_refused(lib):
    from ast_amd import _lib
    c = SM.case("gauss")
    B, D = 1, 13
    wave_t, n = torch.from_numpy(np.array(c["wave"])).to("cuda"), dev(c["n_samples"], torch.int32)
    d = _desc(c, 1)
    ws = _prepared(lib, d)
    feats = torch.full((B, c["Fmax"], D), FILL, dtype=torch.float32, device="cuda")
    n_frames = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    n_bad = torch.full((1,), -7, dtype=torch.int32, device="cuda")

    def call(d, ws=ws):
        return lib.astk_speech_features(C.byref(d), vp(wave_t), vp(n), vp(feats), vp(n_frames), vp(n_bad), C.c_void_p(ws.data_ptr()), ws.nbytes, stream())

    def untouched():
        torch.cuda.synchronize()
        assert int((feats != FILL).sum()) == 0 and int(n_frames[0]) == -7 and int(n_bad[0]) == -7, "the refused call launched something"
    base = {f[0]: getattr(d, f[0]) for f in d._fields_[1:]}
    for field, value, word in REFUSALS:
        bad = _lib.SpeechFeaturesDesc(**{**base, field: value})
        assert call(bad) != 0 and word in lib.astk_last_error().decode(), (field, lib.astk_last_error().decode())
        untouched()
    # a workspace prepared for another descriptor (other tables), and one that was never prepared
    other = _desc(SM.case("hamming"), 1)
    other.B, other.Nmax, other.Fmax = d.B, d.Nmax, d.Fmax
    ws_other = _prepared(lib, other)
    assert ws_other.nbytes == ws.nbytes
    assert call(d, ws=ws_other) != 0 and "different descriptor" in lib.astk_last_error().decode()
    untouched()
    # A workspace nobody prepared.  The host's table goes by address, so a fresh buffer is refused by message -- "never prepared", or
    # "different descriptor" when the allocator hands out an address an earlier test prepared -- unless that address was prepared
    # for these very tables: then the kernel finds no digest in the head and makes every row a bad row.  (The message alone, with
    # an address that cannot have been prepared: tests/test_speech_features_host.py.)
    fresh = GuardedWS(ws.nbytes)
    if call(d, ws=fresh) != 0:
        assert any(w in lib.astk_last_error().decode() for w in ("never prepared", "different descriptor"))
        untouched()
    else:
        torch.cuda.synchronize()
        assert int(n_frames[0]) == -1 and int(n_bad[0]) == 1 and not feats.any()
        feats.fill_(FILL)
        n_frames.fill_(-7)
        n_bad.fill_(-7)
    fresh.check("speech_features")
    # the fields the tables do not depend on may change between prepare and the call
    assert call(d) == 0
    torch.cuda.synchronize()
    want = SM.result("gauss")[1][0]
    assert _ulps(feats.cpu().numpy(), want).max() <= 1.0 and int(n_frames[0]) == 9 and int(n_bad[0]) == 0
    # the kernel looks at the head again: a prepared workspace that was overwritten since makes every row a bad row
    ws.t[:64] = 0
    feats.fill_(FILL)
    assert call(d) == 0
    torch.cuda.synchronize()
    assert int(n_frames[0]) == -1 and int(n_bad[0]) == 1 and not feats.any()
    ws.check("speech_features")


# ------------------------------------------------------------------ CMVN
def _cmvn_run(lib, c, stats0=None, rows=None, out_of_place=False):
    from ast_amd import _lib
    rows = slice(None) if rows is None else rows
    X, nf, gr = dev(np.array(c["X"][rows])), dev(c["n_frames"][rows], torch.int32), dev(c["group"][rows], torch.int32)
    B, Fmax, D = X.shape
    before = [t.clone() for t in (X, nf, gr)]
    stats = torch.full((c["G"] + 1, 2, D + 1), FILL, dtype=torch.float64, device="cuda")
    stats[:c["G"]] = 0 if stats0 is None else torch.from_numpy(stats0).to("cuda")
    n_bad = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    d = _lib.CmvnDesc(B=B, Fmax=Fmax, D=D, G=c["G"], norm_vars=int(c["norm_vars"]))
    ok(lib, lib.astk_cmvn_accumulate(C.byref(d), vp(X), vp(nf), vp(gr), vp(stats), C.c_void_p(n_bad.data_ptr() + 4), stream()))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (X, nf, gr))), "accumulate wrote an input"
    assert (stats[c["G"]] == FILL).all(), "statistics behind G were written"
    out = torch.full((B + 1, Fmax, D), FILL, dtype=torch.float32, device="cuda") if out_of_place else X
    ok(lib, lib.astk_cmvn_apply(C.byref(d), vp(X), vp(out), vp(nf), vp(gr), vp(stats), stream()))
    torch.cuda.synchronize()
    if out_of_place:
        assert torch.equal(X, before[0]) and (out[B:] == FILL).all()
    return dict(stats=stats[:c["G"]].cpu().numpy(), n_bad=n_bad.cpu().numpy(), Y=out[:B].cpu().numpy())


def _stats_close(got, want, c, rows=slice(None)):
    """Sums within 2^-40 sum |x| (sums of squares: 2^-40 sum x^2) of the model's -- fewer than 2^13 float64 additions, each at most
    2^-53 of the running sum of magnitudes -- and the counts exact."""
    D = c["X"].shape[2]
    mag, _ = SM.cmvn_stats(np.abs(c["X"]), c["n_frames"], c["group"], c["G"])
    assert int(np.maximum(c["n_frames"], 0).sum()) < 2 ** 13
    assert (np.abs(got[:, 0, :D] - want[:, 0, :D]) <= 2.0 ** -40 * mag[:, 0, :D]).all()
    assert (np.abs(got[:, 1, :D] - want[:, 1, :D]) <= 2.0 ** -40 * mag[:, 1, :D]).all()
    assert np.array_equal(got[:, 0, D], want[:, 0, D]) and (got[:, 1, D] == 0).all()


@pytest.mark.parametrize("name", SM.CMVN_CASES)
@pytest.mark.parametrize("out_of_place", [False, True])
def test_cmvn_equals_the_model(lib, name, out_of_place):
    c = SM.cmvn_case(name)
    want_stats, want_bad = SM.cmvn_stats(c["X"], c["n_frames"], c["group"], c["G"])
    r = _cmvn_run(lib, c, out_of_place=out_of_place)
    _stats_close(r["stats"], want_stats, c)
    assert r["n_bad"].tolist() == [-7, want_bad, -7]
    want = SM.cmvn_apply(c["X"], c["n_frames"], c["group"], r["stats"], c["norm_vars"])      # applied with the statistics the device holds
    u = _ulps(r["Y"], want)
    print(f"{name}: applied output worst {u.max():.3f} units")
    assert u.max() <= 1.0, (name, float(u.max()))
    want_m = SM.cmvn_apply(c["X"], c["n_frames"], c["group"], want_stats, c["norm_vars"])    # ... and with the model's own
    for b, (g, nf) in enumerate(zip(c["group"].tolist(), c["n_frames"].tolist())):
        skipped = g < 0 or g >= c["G"] or nf < 0 or want_stats[g, 0, -1] == 0
        lo = 0 if skipped else min(nf, c["X"].shape[1])
        assert r["Y"][b, lo:].tobytes() == c["X"][b, lo:].tobytes(), (name, b, "frames that are not normalised must come out as they went in")
    if name == "per-utterance":                              # x - mean is exactly 0 (the float32 inputs sum exactly); one frame: the same
        assert not r["Y"][3, :5].any() and not r["Y"][1, :1].any() and r["Y"][3].tobytes() == want_m[3].tobytes()
    if name == "empty-group":
        assert r["Y"][1].tobytes() == c["X"][1].tobytes() and r["Y"][3].tobytes() == c["X"][3].tobytes() and not r["stats"][1].any()
    again = _cmvn_run(lib, c, out_of_place=out_of_place)
    assert again["stats"].tobytes() == r["stats"].tobytes() and again["Y"].tobytes() == r["Y"].tobytes()


def test_cmvn_statistics_accumulate_across_calls(lib):
    c = SM.cmvn_case("two-speakers")
    want, _ = SM.cmvn_stats(c["X"], c["n_frames"], c["group"], c["G"])
    first = _cmvn_run(lib, c, rows=slice(0, 2))
    both = _cmvn_run(lib, c, stats0=first["stats"], rows=slice(2, 5))
    _stats_close(both["stats"], want, c)
    _stats_close(_cmvn_run(lib, c)["stats"], want, c)


# ------------------------------------------------------------------ the Python layer and the command line
def _waves(seed, lens):
    rng = np.random.default_rng(seed)
    return [SM.gauss(rng, n).astype(np.int16) for n in lens]


def test_compute_on_a_ragged_list_equals_per_utterance_calls():
    from ast_amd import features as F
    cfg = F.FeatureConfig()
    waves = _waves(11, (840, 150, 200, 4000, 1234))
    X, nf = F.compute(waves, cfg, "cuda")
    assert X.shape == (5, cfg.frames(4000), 13) and nf.tolist() == [cfg.frames(len(w)) for w in waves] and X.dtype == torch.float32
    for b, w in enumerate(waves):
        Xb, nb = F.compute([w], cfg, "cuda")
        n = int(nb[0])
        assert n == int(nf[b]) and torch.equal(Xb[0, :n], X[b, :n]) and not X[b, n:].any()
        if n:
            assert _ulps(X[b, :n].cpu().numpy(), SM.features(w, SM.config()).astype(np.float32)).max() <= 1.0
    Xf, _ = F.compute([w.astype(np.float32) for w in waves], cfg, "cuda")
    assert torch.equal(Xf, X)
    fb = F.FeatureConfig(kind="fbank", sample_frequency=16000.0, num_mel_bins=80)
    Xb, nb = F.compute(waves[:2], fb, "cuda")
    assert Xb.shape == (2, fb.frames(840), 80) and len(F._WORKSPACES) >= 2
    with pytest.raises(ValueError):
        F.compute([], cfg, "cuda")
    Y = F.cmvn(X.clone(), nf)
    st, _ = SM.cmvn_stats(X.cpu().numpy(), nf.cpu().numpy(), np.arange(5), 5)
    assert _ulps(Y.cpu().numpy(), SM.cmvn_apply(X.cpu().numpy(), nf.cpu().numpy(), np.arange(5), st, True)).max() <= 1.0


def _write_wav(path, data, rate=8000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(data).astype("<i2").tobytes())


def test_command_line_writes_the_tree_the_loaders_read(tmp_path):
    from ast_amd.dataloader import FisherDataLoader
    spec = importlib.util.spec_from_file_location("features_cli", os.path.join(ROOT, "features.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    utts = {"spkA_0001": 2040, "spkB_0001": 840, "spkA_0002": 1400}
    spk = {"spkA_0001": "spkA", "spkB_0001": "spkB", "spkA_0002": "spkA"}
    waves = dict(zip(utts, _waves(21, utts.values())))
    for u, w in waves.items():
        _write_wav(tmp_path / f"{u}.wav", w)
    (tmp_path / "wav.scp").write_text("".join(f"{u} {tmp_path / (u + '.wav')}\n" for u in utts))
    (tmp_path / "utt2spk").write_text("".join(f"{u} {s}\n" for u, s in spk.items()))
    outs = {}
    for b in (2, 1):
        out = tmp_path / f"out{b}"
        assert cli.main(["--scp", str(tmp_path / "wav.scp"), "--out", str(out), "--set", "dev", "--utt2spk", str(tmp_path / "utt2spk"),
                         "--cmvn", "spk", "--norm-vars", "-b", str(b), "--info-out", str(out / "dev.info"),
                         "--conf", os.path.join(ROOT, "tests", "golden", "kaldi_conf", "mfcc.conf")]) == 0
        outs[b] = {u: np.load(out / "dev" / f"{u}.npy") for u in utts}
    for u in utts:
        assert outs[1][u].tobytes() == outs[2][u].tobytes() and outs[1][u].dtype == np.float32, u
    # the model: float64 features rounded to float32, per-speaker statistics over them, applied
    cfg = SM.config()
    feats = {u: SM.features(w, cfg).astype(np.float32) for u, w in waves.items()}
    Fmax = max(f.shape[0] for f in feats.values())
    X = np.zeros((3, Fmax, 13), np.float32)
    for b, u in enumerate(utts):
        X[b, :feats[u].shape[0]] = feats[u]
    nf = np.asarray([feats[u].shape[0] for u in utts], np.int32)
    group = np.asarray([0, 1, 0], np.int32)
    st, _ = SM.cmvn_stats(X, nf, group, 2)
    Y = SM.cmvn_apply(X, nf, group, st, True)
    # derived bound: the device's features are within u = one float32 unit at max |x| of the model's, so x - mean moves by at most 2 u
    # and sigma by at most 2 u: |dy| <= 2 u s (1 + |y|), plus the rounding of y itself
    count = st[:, 0, 13]
    mean = st[:, 0, :13] / count[:, None]
    s_max = float((1.0 / np.sqrt(st[:, 1, :13] / count[:, None] - mean * mean)).max())
    unit = float(np.spacing(np.float32(np.abs(X).max())))
    for b, u in enumerate(utts):
        got, want = outs[2][u], Y[b, :nf[b]]
        assert got.shape == want.shape, u
        bound = 2.0 * unit * s_max * (1.0 + np.abs(want)) + np.spacing(np.maximum(np.abs(want), np.float32(1)))
        assert (np.abs(got.astype(np.float64) - want) <= bound).all(), (u, float(np.abs(got - want).max()))
    loader = FisherDataLoader.__new__(FisherDataLoader)
    loader.data_cfg = {"speech_path": str(tmp_path / "out2"), "zero_input": 0}
    with open(tmp_path / "out2" / "dev.info", "rb") as f:
        info = pickle.load(f)
    assert list(info) == ["dev"] and list(info["dev"]) == list(utts)
    for u in utts:
        x = loader._speech(u, "dev", 10 ** 6)
        assert x.tobytes() == outs[2][u].tobytes() and info["dev"][u] == {"sp": x.shape[0]} and x.shape == (SM.frames(utts[u], 200, 80), 13)


def test_features_feed_the_batched_encoder():
    """compute then cmvn on two synthetic waves gives the (X, n_frames) pair the model takes: encode_rows(batch_encode=True) on a small
    D = 13 model accepts the rows, and its lengths are the CNN's time formula of the frame counts."""
    import copy
    from oracle import ast_ref as R
    from ast_amd import features as F
    from ast_amd.seq2seq import SpeechEncoderDecoder
    from test_gpu_encode_rows import SMALL
    cfg = tiny_cfg(**SMALL)
    P = R.init_params(cfg, 13, SMALL["V"], seed=0, dtype=np.float32)
    m = SpeechEncoderDecoder(0, copy.deepcopy(cfg)).materialize(13, values=P)
    waves = _waves(31, (8000, 5200))
    X, nf = F.compute(waves, F.FeatureConfig(), "cuda")
    F.cmvn(X, nf)
    assert nf.tolist() == [98, 63] and torch.isfinite(X).all()
    Xs = [X[b, :int(n)] for b, n in enumerate(nf.tolist())]
    rb = m.encode_rows(Xs, batch_encode=True)
    alone = m.encode_rows(Xs, batch_encode=False)
    t2 = lambda t: ((t + 1) // 2 + 1) // 2          # noqa: E731   two CNN layers of time stride 2, kernel 9, pad 4
    assert list(rb.lens) == [t2(98), t2(63)] == list(alone.lens)
    assert torch.isfinite(rb.enc).all() and rb.enc.shape == alone.enc.shape and float(rb.enc.abs().max()) > 0
