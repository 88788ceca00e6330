"""Host tests of the speech features.  The model of tests/speech_features_model.py is the contract and no Kaldi
output exists to pin it to, so it is pinned independently here: its spectrum against a direct DFT summed in reversed order, Parseval,
the frame count against a loop, the DCT rows, the shape of the mel filters, an impulse's flat spectrum, and a float32 restatement of the
same steps.  Then the condition the named cases must meet, the Python layer's pieces that need no GPU, the command line's parser, and
the declarations and refusals of the five entry points."""
import ctypes as C
import importlib.util
import os
import re
import wave

import numpy as np
import pytest
import scipy.fft

import speech_features_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECTRUM_CASES = ("gauss", "tone", "loud-quiet", "impulse", "16k-fbank80", "len100", "len256", "rectangular", "dither-seed1")


def _rows(name):
    c = SM.case(name)
    for b, n in enumerate(c["n_samples"].tolist()):
        if 0 <= n <= c["wave"].shape[1]:
            yield c, b, c["wave"][b, :n]


# ------------------------------------------------------------------ the model, pinned independently
@pytest.mark.parametrize("name", SPECTRUM_CASES)
def test_spectrum_is_the_direct_dft_and_obeys_parseval(name):
    for c, b, x in _rows(name):
        cfg = c["cfg"]
        wf, _ = SM.windowed_frames(x, cfg, c["seed"], c["offsets"][b])
        if wf.shape[0] == 0:
            continue
        N = SM.fft_size(cfg)
        P = SM.power_spectrum(wf, cfg)
        pad = np.zeros((wf.shape[0], N))
        pad[:, :wf.shape[1]] = wf
        kn = (np.arange(N // 2 + 1)[:, None] * np.arange(N)[None, :]) % N
        Wm = np.exp(-2j * np.pi * kn / N)
        direct = np.zeros((wf.shape[0], N // 2 + 1), np.complex128)
        for n in range(N - 1, -1, -1):                                  # O(N^2), summed in reversed order
            direct += pad[:, n, None] * Wm[None, :, n]
        Pd = direct.real ** 2 + direct.imag ** 2
        scale = P.max(axis=1, keepdims=True) + 1e-300
        assert (np.abs(P - Pd) / scale).max() < 1e-12, name
        # Parseval: sum x^2 = (P_0 + 2 sum_{0<k<N/2} P_k + P_{N/2}) / N
        lhs = (pad * pad).sum(axis=1)
        rhs = (P[:, 0] + 2.0 * P[:, 1:-1].sum(axis=1) + P[:, -1]) / N
        assert np.allclose(lhs, rhs, rtol=1e-12, atol=1e-9), name


def test_frame_count_formula_against_a_loop():
    for L, S in ((200, 80), (400, 160), (256, 80), (2, 1), (100, 40), (1200, 480)):
        for n in list(range(0, 3 * L + 5)) + [10 * L + 3]:
            count, start = 0, 0
            while start + L <= n:
                count += 1
                start += S
            assert SM.frames(n, L, S) == count, (L, S, n)
    assert [SM.frames(n, 200, 80) for n in (0, 199, 200, 279, 280)] == [0, 0, 1, 1, 2]


def test_deterministic_cosine_is_a_cosine():
    t = np.concatenate([np.linspace(0.0, 9.0, 20001), np.arange(0, 40) / 4.0, np.arange(0, 127) / 22.0])
    assert np.abs(SM.det_cospi(t) - np.cos(np.pi * t)).max() < 4e-15
    assert np.abs(SM.det_sinpi(t) - np.sin(np.pi * t)).max() < 4e-15
    assert SM.det_cospi(0.0) == 1.0 and SM.det_cospi(0.5) == 0.0 and SM.det_cospi(1.0) == -1.0 and SM.det_sinpi(0.0) == 0.0


@pytest.mark.parametrize("M,K", [(23, 13), (40, 40), (80, 80), (3, 3)])
def test_dct_rows_are_orthonormal(M, K):
    d = SM.dct_rows(SM.config(num_mel_bins=M, num_ceps=K))
    assert np.abs(d @ d.T - np.eye(K)).max() < 1e-14
    lift = SM.lifter(SM.config(num_mel_bins=M, num_ceps=K))
    assert lift[0] == 1.0 and np.allclose(lift, 1.0 + 11.0 * np.sin(np.pi * np.arange(K) / 22.0), rtol=0, atol=1e-13)
    assert (SM.lifter(SM.config(num_mel_bins=M, num_ceps=K, cepstral_lifter=0.0)) == 1.0).all()


@pytest.mark.parametrize("kw", [dict(), dict(sample_frequency=16000.0, num_mel_bins=80), dict(sample_frequency=16000.0, num_mel_bins=40),
                                dict(low_freq=0.0, high_freq=-200.0), dict(frame_len=1200), dict(frame_len=100)])
def test_mel_filters_are_triangles_that_partition_the_band(kw):
    cfg = SM.config(**kw)
    W = SM.mel_banks(cfg)
    N = SM.fft_size(cfg)
    assert W.shape == (cfg["num_mel_bins"], N // 2) and (W >= 0).all() and (W <= 1).all()
    f = np.arange(N // 2) * cfg["sample_frequency"] / N
    for j in range(W.shape[0]):
        nz = np.flatnonzero(W[j])
        if nz.size == 0:
            continue
        assert (np.diff(nz) == 1).all()                                  # one run of bins
        peak = int(W[j].argmax())
        assert (np.diff(W[j, nz[0]:peak + 1]) >= 0).all() and (np.diff(W[j, peak:nz[-1] + 1]) <= 0).all()      # one peak
    # a bin between the first centre and the last centre lies on the falling side of one triangle and the rising side of the next: total 1
    lo, hi = SM.mel(cfg["low_freq"]), SM.mel(SM.resolved_high(cfg))
    delta = (hi - lo) / (cfg["num_mel_bins"] + 1)
    m = SM.mel(f)
    interior = (m > lo + delta) & (m < hi - delta)
    assert interior.sum() > 10 and np.abs(W[:, interior].sum(axis=0) - 1.0).max() < 1e-12
    outside = (m <= lo) | (m >= hi)
    assert (W[:, outside] == 0).all()
    assert (np.count_nonzero(W, axis=0) <= 2).all()                      # what bounds the kernel's packed weights by N


def test_an_impulse_has_a_flat_spectrum():
    cfg = SM.config(window_type="rectangular", preemphasis_coefficient=0.0, remove_dc_offset=False)
    x = np.zeros(200)
    x[37] = 250.0
    wf, energy = SM.windowed_frames(x, cfg)
    P = SM.power_spectrum(wf, cfg)
    assert np.abs(P - 62500.0).max() < 1e-7 and abs(energy[0] - np.log(62500.0)) < 1e-12
    E, _ = SM.mel_energies(x, cfg)
    assert np.allclose(E[0], 62500.0 * SM.mel_banks(cfg).sum(axis=1), rtol=1e-12)


def _float32_restatement(x, cfg, seed, offset):
    """The same steps in float32 arithmetic (scipy.fft in complex64): what a float32 kernel would compute."""
    f = np.float32
    wf64, _ = SM.windowed_frames(x, SM.config(**{**cfg, "window_type": "rectangular", "preemphasis_coefficient": 0.0, "remove_dc_offset": False,
                                                 "frame_len": cfg["frame_len"], "frame_shift_samples": cfg["frame_shift_samples"]}), seed, offset)
    fr = wf64.astype(f)
    if cfg["remove_dc_offset"]:
        fr = fr - fr.mean(axis=1, keepdims=True, dtype=f)
    c = f(cfg["preemphasis_coefficient"])
    prev = np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = (fr - c * prev) * SM.window(cfg).astype(f)[None, :]
    pad = np.zeros((fr.shape[0], SM.fft_size(cfg)), f)
    pad[:, :fr.shape[1]] = fr
    S = scipy.fft.rfft(pad, axis=1)
    assert S.dtype == np.complex64
    P = (S.real ** 2 + S.imag ** 2).astype(f)
    E = (P[:, :-1] @ SM.mel_banks(cfg).T.astype(f)).astype(f)
    Lg = np.log(np.maximum(E, f(SM.EPS)))
    if cfg["kind"] == "fbank":
        return Lg
    T = (SM.lifter(cfg)[:, None] * SM.dct_rows(cfg)).astype(f)
    return (Lg @ T.T).astype(f)


def test_float32_restatement_agrees_on_noise_and_not_on_the_clean_tone():
    """Why the arithmetic is float64: a float32 restatement stays within 1e-4 of the model on noise-like input, and leaves it on a clean
    tone, where rounding leaks from the loud bins into the quiet ones."""
    worst = 0.0
    for name in SM.NOISE_LIKE_CASES:
        for c, b, x in _rows(name):
            if SM.frames(len(x), c["cfg"]["frame_len"], c["cfg"]["frame_shift_samples"]) == 0:
                continue
            d = np.abs(_float32_restatement(x, c["cfg"], c["seed"], c["offsets"][b]) - SM.features(x, c["cfg"], c["seed"], c["offsets"][b])).max()
            worst = max(worst, float(d))
            assert d < 1e-4, (name, b, d)
    c = SM.case("tone")
    x = c["wave"][0, :c["n_samples"][0]]
    d_tone = np.abs(_float32_restatement(x, c["cfg"], 0, 0) - SM.features(x, c["cfg"])).max()
    assert d_tone > 10 * max(worst, 1e-5), (d_tone, worst)


# ------------------------------------------------------------------ a condition on the cases
def test_no_case_sits_on_the_energy_floor():
    """Every mel energy of every case is exactly 0 or at least 1e-4, three decades above the floor 2^-23 = 1.19e-7: no case sits on the
    kink of max(E, eps), where reordered float64 sums could fall on either side."""
    smallest, zeros = np.inf, 0
    for name in SM.ALL_CASES:
        for c, b, x in _rows(name):
            E, _ = SM.mel_energies(x, c["cfg"], c["seed"], c["offsets"][b])
            pos = E[E != 0.0]
            zeros += int((E == 0.0).sum())
            assert (E >= 0).all() and (pos.size == 0 or pos.min() >= 1e-4), (name, b, pos.min())
            if pos.size:
                smallest = min(smallest, float(pos.min()))
    assert zeros > 0 and smallest >= 1e-4
    for name in SM.EXACT_ZERO_CASES:                                     # ... and the exact-zero cases do hold frames of exact zeros
        assert any((SM.mel_energies(x, c["cfg"])[0] == 0.0).all(axis=1).any() for c, b, x in _rows(name) if len(x) >= c["cfg"]["frame_len"]), name


def test_the_named_cases_cover_what_they_were_chosen_for():
    fr = lambda name: SM.result(name)[1][1].tolist()          # noqa: E731
    assert fr("counts-edge") == [0, 0, 1, 1, 2, 9] and fr("counts-workgroup") == [3, 4, 5, 9, 130]
    c, (feats, nf, n_bad) = SM.result("fmax-above")
    assert c["Fmax"] == 1700 > max(nf) and len(nf) * c["Fmax"] > 4 * 2048 and nf[5] == 130 and not feats[5, 130:].any() and feats[5, 129].any()
    c, (feats, nf, n_bad) = SM.result("bad-rows")
    assert nf.tolist() == [5, -1, -1, -1, 4, 0] and n_bad == 3 and not feats[[1, 2, 3]].any()
    c = SM.case("int16-extremes")
    assert c["wave"].dtype == np.int16 and c["wave"].min() == -32768 and c["wave"].max() == 32767
    c = SM.case("float32-nan-behind")
    assert c["wave"].dtype == np.float32 and all(np.isnan(c["wave"][b, n:]).all() and n < c["wave"].shape[1] for b, n in enumerate(c["n_samples"]))
    assert np.isfinite(SM.result("float32-nan-behind")[1][0]).all()
    c = SM.case("int16-max-behind")
    assert all((c["wave"][b, n:] == 32767).all() for b, n in enumerate(c["n_samples"]))
    sizes = {(SM.case(n)["cfg"]["frame_len"], SM.fft_size(SM.case(n)["cfg"])) for n in SM.ALL_CASES}
    assert {(200, 256), (400, 512), (256, 256), (100, 128), (1200, 2048), (2, 2)} <= sizes
    assert SM.case("16k-fbank80")["cfg"]["num_mel_bins"] == 80 and SM.dim(SM.case("16k-mfcc40")["cfg"]) == 40
    assert {SM.case(n)["cfg"]["window_type"] for n in SM.ALL_CASES} == set(SM.WINDOWS)
    a, b = SM.result("dither-seed1"), SM.result("dither-seed2")
    assert (a[0]["wave"] == b[0]["wave"]).all() and a[0]["offsets"].tolist() == [12345, 7, 0] and not np.array_equal(a[1][0], b[1][0])
    # the dither is a function of the sample index: sample n of a row carries z(seed, offset + n) whatever frame holds it
    z = SM.dither_stream(1, 12345, 300)
    assert np.array_equal(z[80:], SM.dither_stream(1, 12345 + 80, 220)) and abs(z.std() - 1.0) < 0.15
    const = SM.result("constant")[1][0][0]
    assert (const == const[0, :]).all() and const[0, 0] == np.float32(SM.features(np.zeros(200), SM.config())[0, 0])


def test_cmvn_model_known_answers():
    X = np.zeros((2, 3, 2), np.float32)
    X[0] = [[1, 10], [3, 10], [9, 9]]
    X[1, :1] = [[5, 6]]
    st, n_bad = SM.cmvn_stats(X, [2, 1], [0, 0], 1)
    assert st.tolist() == [[[9.0, 26.0, 3.0], [35.0, 236.0, 0.0]]] and n_bad == 0
    Y = SM.cmvn_apply(X, [2, 1], [0, 0], st, False)
    assert Y[0, :2].tolist() == [[-2.0, 10 - 26 / 3], [0.0, 10 - 26 / 3]] or np.allclose(Y[0, :2], [[-2, 10 - 26 / 3], [0, 10 - 26 / 3]])
    assert (Y[0, 2] == X[0, 2]).all() and (Y[1, 1:] == 0).all()
    st2, _ = SM.cmvn_stats(X[:1], [2], [0], 1)
    st2, _ = SM.cmvn_stats(X[1:], [1], [0], 1, st2)
    assert np.array_equal(st, st2)
    assert SM.cmvn_stats(X, [2, 1], [0, 5], 1)[1] == 1
    c = SM.cmvn_case("per-utterance")
    st, _ = SM.cmvn_stats(c["X"], c["n_frames"], c["group"], c["G"])
    Y = SM.cmvn_apply(c["X"], c["n_frames"], c["group"], st, True)
    assert (Y[3, :5] == 0).all() and (Y[1, 0] == 0).all() and (Y[4] == c["X"][4]).all()      # constant features; one frame; no frames
    assert np.abs(Y[2, :70].astype(np.float64).std(axis=0) - 1).max() < 1e-5


# ------------------------------------------------------------------ the Python layer without a GPU
def test_feature_config_defaults_and_frames():
    from ast_amd.features import FeatureConfig
    c = FeatureConfig()
    assert (c.kind, c.sample_frequency, c.frame_length, c.frame_shift, c.dither, c.preemphasis_coefficient, c.remove_dc_offset, c.window_type,
            c.num_mel_bins, c.low_freq, c.high_freq, c.num_ceps, c.cepstral_lifter, c.use_energy) == \
        ("mfcc", 8000.0, 25.0, 10.0, 0.0, 0.97, True, "povey", 23, 20.0, 0.0, 13, 22.0, False)
    assert (c.frame_len, c.frame_shift_samples, c.dim) == (200, 80, 13)
    c16 = FeatureConfig(kind="fbank", sample_frequency=16000.0, num_mel_bins=80)
    assert (c16.frame_len, c16.frame_shift_samples, c16.dim) == (400, 160, 80)
    assert [c.frames(n) for n in (0, 199, 200, 279, 280, 840)] == [0, 0, 1, 1, 2, 9]
    m = SM.config()
    for k in ("sample_frequency", "num_mel_bins", "num_ceps", "low_freq", "high_freq", "preemphasis_coefficient", "cepstral_lifter",
              "window_type", "kind", "remove_dc_offset", "use_energy", "dither"):
        assert getattr(c, k) == m[k], k                                  # the layer's defaults are the model's
    assert hash(c) == hash(FeatureConfig())                              # (the workspace cache keys on it)


def test_from_kaldi_conf_reads_the_fixture_and_refuses_what_it_cannot_honour(tmp_path):
    from ast_amd.features import FeatureConfig
    c = FeatureConfig.from_kaldi_conf(os.path.join(ROOT, "tests", "golden", "kaldi_conf", "mfcc.conf"))
    assert (c.use_energy, c.sample_frequency, c.num_ceps) == (False, 8000.0, 13) and c == FeatureConfig()

    def conf(text):
        p = tmp_path / "x.conf"
        p.write_text(text)
        return str(p)
    c = FeatureConfig.from_kaldi_conf(conf("# a comment\n--num-mel-bins=40   # more bins\n\n--window-type=hamming\n--snip-edges=true\n--htk-compat=false\n"
                                           "--use-energy=true\n--low-freq=0\n"), kind="mfcc")
    assert (c.num_mel_bins, c.window_type, c.use_energy, c.low_freq) == (40, "hamming", True, 0.0)
    for text, word in (("--snip-edges=false\n", "snip-edges"), ("--htk-compat=true\n", "htk-compat"), ("--vtln-warp=1.1\n", "vtln-warp"),
                       ("--kind=fbank\n", "kind"), ("num-ceps=13\n", "--key=value"), ("--use-energy=maybe\n", "use-energy")):
        with pytest.raises(ValueError, match=word):
            FeatureConfig.from_kaldi_conf(conf(text))


def _write_wav(path, data, rate=8000, width=2):
    data = np.asarray(data)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if data.ndim == 1 else data.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(data.astype("<i2" if width == 2 else np.uint8).tobytes())


def _cli():
    spec = importlib.util.spec_from_file_location("features_cli", os.path.join(ROOT, "features.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                         # (no main: nothing runs)
    return mod


def test_read_wav_round_trips_and_refusals(tmp_path):
    from ast_amd.features import FeatureConfig, read_wav
    rng = np.random.default_rng(3)
    mono = rng.integers(-32768, 32768, 500).astype(np.int16)
    mono[:2] = [-32768, 32767]
    _write_wav(tmp_path / "m.wav", mono)
    x, rate = read_wav(str(tmp_path / "m.wav"))
    assert x.dtype == np.int16 and rate == 8000 and np.array_equal(x, mono)
    stereo = rng.integers(-32768, 32768, (300, 2)).astype(np.int16)
    _write_wav(tmp_path / "s.wav", stereo, rate=16000)
    for ch in (0, 1):
        x, rate = read_wav(str(tmp_path / "s.wav"), channel=ch)
        assert rate == 16000 and np.array_equal(x, stereo[:, ch]) and x.flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError, match="channels"):
        read_wav(str(tmp_path / "s.wav"))
    with pytest.raises(ValueError, match="channel 2"):
        read_wav(str(tmp_path / "s.wav"), channel=2)
    _write_wav(tmp_path / "b.wav", rng.integers(0, 255, 100), width=1)
    with pytest.raises(ValueError, match="8-bit"):
        read_wav(str(tmp_path / "b.wav"))
    (tmp_path / "junk.wav").write_bytes(b"not a wave file at all")
    with pytest.raises(ValueError, match="junk.wav"):
        read_wav(str(tmp_path / "junk.wav"))
    cli = _cli()
    assert np.array_equal(cli.load_wave(str(tmp_path / "m.wav"), FeatureConfig()), mono)
    _write_wav(tmp_path / "wide.wav", mono, rate=16000)
    with pytest.raises(ValueError, match=r"wide\.wav.*16000"):            # the wrong rate is an error that names the file
        cli.load_wave(str(tmp_path / "wide.wav"), FeatureConfig())


def test_command_line_parses_and_reads_its_lists(tmp_path):
    cli = _cli()
    a = vars(cli.build_parser().parse_args(["--scp", "w.scp", "--out", "o", "--set", "dev"]))
    assert (a["scp"], a["out"], a["set_key"], a["conf"], a["kind"], a["cmvn"], a["norm_vars"], a["batch"], a["seed"], a["info_out"], a["utt2spk"],
            a["dither"]) == ("w.scp", "o", "dev", None, "mfcc", "none", False, 32, 0, None, None, None)
    a = cli.build_parser().parse_args(["--scp", "w.scp", "--out", "o", "--set", "dev", "--kind", "fbank", "--num-mel-bins", "80",
                                       "--sample-frequency", "16000", "--cmvn", "spk", "--utt2spk", "u2s", "--norm-vars", "-b", "2", "--dither", "1",
                                       "--seed", "9", "--info-out", "i.p"])
    assert (a.cmvn, a.norm_vars, a.batch, a.seed, a.info_out, a.utt2spk) == ("spk", True, 2, 9, "i.p", "u2s")
    cfg = cli.config_from_args(a)
    assert (cfg.kind, cfg.num_mel_bins, cfg.sample_frequency, cfg.dither, cfg.dim) == ("fbank", 80, 16000.0, 1.0, 80)
    a = cli.build_parser().parse_args(["--scp", "w", "--out", "o", "--set", "s", "--conf", os.path.join(ROOT, "tests", "golden", "kaldi_conf", "mfcc.conf")])
    assert cli.config_from_args(a).num_ceps == 13
    with pytest.raises(SystemExit):
        cli.config_from_args(cli.build_parser().parse_args(["--scp", "w", "--out", "o", "--set", "s", "--conf", "c", "--num-ceps", "5"]))
    scp = tmp_path / "wav.scp"
    scp.write_text("utt_b /data/b.wav\n\nutt_a  /data/with space/a.wav\n")
    assert cli.read_scp(str(scp)) == [("utt_b", "/data/b.wav"), ("utt_a", "/data/with space/a.wav")]
    scp.write_text("utt_a sph2pipe -f wav a.sph |\n")
    with pytest.raises(ValueError, match="pipe"):
        cli.read_scp(str(scp))
    scp.write_text("utt_a a.wav\nutt_a b.wav\n")
    with pytest.raises(ValueError, match="twice"):
        cli.read_scp(str(scp))
    (tmp_path / "u2s").write_text("utt_a spk1\nutt_b spk2\n")
    assert cli.read_utt2spk(str(tmp_path / "u2s")) == {"utt_a": "spk1", "utt_b": "spk2"}


# ------------------------------------------------------------------ the library without a GPU
ENTRY_POINTS = {"astk_speech_features_workspace_bytes": 1, "astk_speech_features_prepare": 4, "astk_speech_features": 9,
                "astk_cmvn_accumulate": 7, "astk_cmvn_apply": 7}


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
    decl = re.search(r"int astk_speech_features\(([^;]*)\);", hdr).group(1)
    assert "const void* wave" in decl and "const int32_t* n_samples" in decl                     # read-only by declaration
    decl = re.search(r"int astk_cmvn_accumulate\(([^;]*)\);", hdr).group(1)
    assert all("const " + n in decl for n in ("float* feats", "int32_t* n_frames", "int32_t* group"))
    for struct, cls in (("astk_speech_features_desc", _lib.SpeechFeaturesDesc), ("astk_cmvn_desc", _lib.CmvnDesc)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for stmt in body.split(";") if stmt.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())]
        assert names == [f[0] for f in cls._fields_], (struct, names)
    assert int(re.search(r"#define ASTK_VERSION (\d+)", hdr).group(1)) >= 112 and _lib.load().astk_version() >= 112
    assert int(re.search(r"#define ASTK_FEAT_MAX_FRAME_LEN (\d+)", hdr).group(1)) == _lib.FEAT_MAX_FRAME_LEN == 2048
    assert int(re.search(r"#define ASTK_FEAT_MAX_MEL_BINS (\d+)", hdr).group(1)) == _lib.FEAT_MAX_MEL_BINS == 128
    for name, value in _lib.FEAT_WINDOWS.items():
        assert int(re.search(r"#define ASTK_FEAT_WINDOW_%s (\d+)" % name.upper(), hdr).group(1)) == value
    srcs = open(os.path.join(ROOT, "ast_amd", "csrc", "build.sh")).read().split("SRCS=")[1].split("\n")[0]
    hooked = open(os.path.join(ROOT, "ast_amd", "csrc", "build.sh")).read().split("HOOKED=")[1].split("\n")[0]
    assert " features" in srcs and "features" not in hooked


GOOD = dict(B=2, Nmax=1000, Fmax=11, sample_type=1, kind=0, window=0, frame_len=200, frame_shift=80, num_mel_bins=23, num_ceps=13,
            remove_dc_offset=1, use_energy=0, sample_frequency=8000.0, low_freq=20.0, high_freq=0.0, preemphasis=0.97, cepstral_lifter=22.0,
            dither=0.0, seed=0)
REFUSALS = (("B", 0, "B"), ("Nmax", 0, "Nmax"), ("Fmax", 0, "Fmax"), ("frame_len", 1, "frame_len"), ("frame_len", 2049, "frame_len"),
            ("frame_shift", 0, "frame_shift"), ("num_mel_bins", 2, "num_mel_bins"), ("num_mel_bins", 129, "num_mel_bins"),
            ("num_ceps", 0, "num_ceps"), ("num_ceps", 24, "num_ceps"), ("low_freq", -1.0, "low_freq"), ("high_freq", 10.0, "high_freq"),
            ("high_freq", 4000.5, "high_freq"), ("high_freq", -3990.0, "high_freq"), ("kind", 2, "kind"), ("window", 4, "window"),
            ("window", -1, "window"), ("sample_type", 2, "sample_type"))
CMVN_GOOD = dict(B=2, Fmax=5, D=13, G=2, norm_vars=1)
CMVN_REFUSALS = (("B", 0, "B"), ("Fmax", 0, "Fmax"), ("D", 0, "D"), ("G", 0, "G"))


def test_descriptor_refusals_need_no_device():
    """Every refusal comes from the descriptor and the pointers alone, before any launch: with a fake non-null pointer for the buffers
    no device is touched."""
    from ast_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)
    err = lambda: lib.astk_last_error().decode()          # noqa: E731

    def call(d, wave=fake, n=fake, feats=fake, nf=fake, ws=fake, ws_bytes=1 << 30):
        return lib.astk_speech_features(C.byref(d), wave, n, feats, nf, None, ws, ws_bytes, None)
    for field, value, word in REFUSALS + (("use_energy", 1, "use_energy"),):
        d = _lib.SpeechFeaturesDesc(**{**GOOD, field: value, **({"kind": 1} if field == "use_energy" else {})})
        for rc in (call(d), lib.astk_speech_features_prepare(C.byref(d), fake, 1 << 30, None)):
            assert rc != 0 and word in err() and "ASTK_" not in err(), (field, value, err())
        assert lib.astk_speech_features_workspace_bytes(C.byref(d)) == 0, (field, value)
    d = _lib.SpeechFeaturesDesc(**GOOD)
    need = lib.astk_speech_features_workspace_bytes(C.byref(d))
    assert need > 0 and need % 256 == 0
    d.struct_size -= 4
    assert call(d) != 0 and "struct_size" in err()
    assert lib.astk_speech_features_prepare(C.byref(d), fake, need, None) != 0 and "struct_size" in err()
    d = _lib.SpeechFeaturesDesc(**GOOD)
    for kw in (dict(wave=None), dict(n=None), dict(feats=None), dict(nf=None), dict(ws=None)):
        assert call(d, **kw) != 0 and "null" in err(), kw
    assert lib.astk_speech_features_prepare(C.byref(d), None, need, None) != 0 and "null" in err()
    assert call(d, ws_bytes=need - 1) != 0 and "workspace" in err() and str(need) in err()
    assert lib.astk_speech_features_prepare(C.byref(d), fake, need - 1, None) != 0 and "workspace" in err()
    assert call(d) != 0 and "never prepared" in err()                    # a workspace the library has not filled
    # fbank takes no num_ceps; the widest and the narrowest shapes are descriptors the library accepts
    for kw in (dict(kind=1, num_ceps=0, num_mel_bins=128), dict(frame_len=2048, num_mel_bins=128, num_ceps=128), dict(frame_len=2, num_mel_bins=3, num_ceps=1),
               dict(high_freq=4000.0), dict(high_freq=-3979.0)):
        assert lib.astk_speech_features_workspace_bytes(C.byref(_lib.SpeechFeaturesDesc(**{**GOOD, **kw}))) > 0, kw

    def acc(d, feats=fake, nf=fake, group=fake, stats=fake):
        return lib.astk_cmvn_accumulate(C.byref(d), feats, nf, group, stats, None, None)

    def app(d, fin=fake, fout=fake, nf=fake, group=fake, stats=fake):
        return lib.astk_cmvn_apply(C.byref(d), fin, fout, nf, group, stats, None)
    for field, value, word in CMVN_REFUSALS:
        d = _lib.CmvnDesc(**{**CMVN_GOOD, field: value})
        for rc in (acc(d), app(d)):
            assert rc != 0 and word in err() and "ASTK_" not in err(), (field, err())
    d = _lib.CmvnDesc(**CMVN_GOOD)
    d.struct_size += 8
    assert acc(d) != 0 and "struct_size" in err() and app(d) != 0 and "struct_size" in err()
    d = _lib.CmvnDesc(**CMVN_GOOD)
    for kw in (dict(feats=None), dict(nf=None), dict(group=None), dict(stats=None)):
        assert acc(d, **kw) != 0 and "null" in err(), kw
    for kw in (dict(fin=None), dict(fout=None), dict(nf=None), dict(group=None), dict(stats=None)):
        assert app(d, **kw) != 0 and "null" in err(), kw
