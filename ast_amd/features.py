"""Speech features from waveforms on the device (include/astk.h astk_speech_features, astk_cmvn_*): MFCC / log mel
filterbank rows in the sense of Kaldi's compute-mfcc-feats / compute-fbank-feats, and cepstral mean and variance normalisation.  The
definition is tests/speech_features_model.py; parity with Kaldi's binaries is not pinned.  In front of them, resampling by a rational
ratio and with it speed perturbation (astk_resample; the definition is tests/resample_model.py, parity with sox /
Kaldi unpinned).  There is no host fall-back: the compute path is the HIP library."""
import ctypes as C
import dataclasses
import fractions
import wave as _wave

import numpy as np

from . import _lib

_BOOL = {"true": True, "false": False}


@dataclasses.dataclass(frozen=True)
class FeatureConfig:
    """Kaldi's option names as fields (dashes as underscores), Kaldi's defaults -- but dither defaults to 0 here (deterministic output;
    Kaldi's default is 1.0).  `kind` is "mfcc" or "fbank"."""
    kind: str = "mfcc"
    sample_frequency: float = 8000.0
    frame_length: float = 25.0              # milliseconds
    frame_shift: float = 10.0               # milliseconds
    dither: float = 0.0
    preemphasis_coefficient: float = 0.97
    remove_dc_offset: bool = True
    window_type: str = "povey"
    num_mel_bins: int = 23
    low_freq: float = 20.0
    high_freq: float = 0.0
    num_ceps: int = 13
    cepstral_lifter: float = 22.0
    use_energy: bool = False

    @property
    def frame_len(self):
        return int(round(self.sample_frequency * self.frame_length / 1000.0))

    @property
    def frame_shift_samples(self):
        return int(round(self.sample_frequency * self.frame_shift / 1000.0))

    @property
    def dim(self):
        return self.num_mel_bins if self.kind == "fbank" else self.num_ceps

    def frames(self, n_samples):
        """Frames of a waveform of n_samples (snip-edges=true)."""
        L, S = self.frame_len, self.frame_shift_samples
        return 0 if n_samples < L else 1 + (n_samples - L) // S

    @classmethod
    def from_kaldi_conf(cls, path, kind="mfcc"):
        """Reads a Kaldi configuration file: one --key=value per line, # starts a comment.  Unknown keys, snip-edges=false and
        htk-compat=true are refused by name."""
        fields = {f.name: f for f in dataclasses.fields(cls)}
        kw = {"kind": kind}
        with open(path) as f:
            for ln, line in enumerate(f, 1):
                line = line.split("#", 1)[0].strip()
                if not line:
                    continue
                if not line.startswith("--") or "=" not in line:
                    raise ValueError(f"{path}:{ln}: expected --key=value, got {line!r}")
                key, value = line[2:].split("=", 1)
                key, value = key.strip(), value.strip()
                if key == "snip-edges":
                    if _parse_bool(path, ln, key, value) is False:
                        raise ValueError(f"{path}:{ln}: snip-edges=false is not supported (snip-edges=true is the only mode)")
                    continue
                if key == "htk-compat":
                    if _parse_bool(path, ln, key, value) is True:
                        raise ValueError(f"{path}:{ln}: htk-compat=true is not supported")
                    continue
                name = key.replace("-", "_")
                if name not in fields or name == "kind":
                    raise ValueError(f"{path}:{ln}: unknown option --{key}")
                t = fields[name].type
                if t in (bool, "bool"):
                    kw[name] = _parse_bool(path, ln, key, value)
                elif t in (int, "int"):
                    kw[name] = int(value)
                elif t in (float, "float"):
                    kw[name] = float(value)
                else:
                    kw[name] = value
        return cls(**kw)

    def descriptor(self, B, Nmax, Fmax, sample_type, seed=0, offsets=None):
        if self.kind not in ("mfcc", "fbank"):
            raise ValueError(f"unknown kind {self.kind!r} (mfcc or fbank)")
        if self.window_type not in _lib.FEAT_WINDOWS:
            raise ValueError(f"unknown window_type {self.window_type!r} ({', '.join(_lib.FEAT_WINDOWS)})")
        return _lib.SpeechFeaturesDesc(
            B=B, Nmax=Nmax, Fmax=Fmax, sample_type=sample_type, kind=_lib.FEAT_FBANK if self.kind == "fbank" else _lib.FEAT_MFCC,
            window=_lib.FEAT_WINDOWS[self.window_type], frame_len=self.frame_len, frame_shift=self.frame_shift_samples,
            num_mel_bins=self.num_mel_bins, num_ceps=self.num_ceps if self.kind == "mfcc" else 0, remove_dc_offset=int(self.remove_dc_offset),
            use_energy=int(self.use_energy), sample_frequency=self.sample_frequency, low_freq=self.low_freq, high_freq=self.high_freq,
            preemphasis=self.preemphasis_coefficient, cepstral_lifter=self.cepstral_lifter, dither=self.dither, seed=seed & (2 ** 64 - 1),
            offsets=offsets)


def _parse_bool(path, ln, key, value):
    if value.lower() not in _BOOL:
        raise ValueError(f"{path}:{ln}: --{key} takes true or false, got {value!r}")
    return _BOOL[value.lower()]


def read_wav(path, channel=None):
    """(int16 array, sample rate) of a RIFF file of 16-bit PCM: mono, or one chosen channel of several.  Everything else is refused."""
    try:
        w = _wave.open(path, "rb")
    except _wave.Error as e:
        raise ValueError(f"{path}: not a PCM wave file the standard library reads ({e})") from None
    with w:
        nch, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        if width != 2:
            raise ValueError(f"{path}: {8 * width}-bit samples, only 16-bit PCM is read")
        if nch != 1 and channel is None:
            raise ValueError(f"{path}: {nch} channels, choose one (channel=0..{nch - 1})")
        if channel is not None and not 0 <= channel < nch:
            raise ValueError(f"{path}: channel {channel} of a file with {nch}")
        x = np.frombuffer(w.readframes(n), dtype="<i2").reshape(-1, nch)
    return np.ascontiguousarray(x[:, channel or 0]).astype(np.int16), rate


_WORKSPACES = {}        # (cfg, device) -> the prepared table workspace


def _stream(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _workspace(cfg, device, desc):
    import torch
    key = (cfg, str(device))
    ws = _WORKSPACES.get(key)
    if ws is None:
        lib = _lib.load()
        nbytes = int(lib.astk_speech_features_workspace_bytes(C.byref(desc)))
        if nbytes == 0:
            _lib.check(-1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(lib.astk_speech_features_prepare(C.byref(desc), C.c_void_p(ws.data_ptr()), nbytes, _stream(device)))
        _WORKSPACES[key] = ws
    return ws


def _sample_type(wave, what):
    import torch
    if wave.dim() != 2 or not wave.is_contiguous() or wave.dtype not in (torch.int16, torch.float32) or not wave.is_cuda:
        raise ValueError(f"{what}: wave must be a contiguous (B, Nmax) int16 or float32 tensor on the device")
    if wave.shape[0] < 1 or wave.shape[1] < 1:
        raise ValueError(f"{what}: wave of shape {tuple(wave.shape)}, there must be at least one row and one sample")
    return _lib.FEAT_SAMPLE_I16 if wave.dtype == torch.int16 else _lib.FEAT_SAMPLE_F32


def _lengths(n_samples, wave, what):
    import torch
    if not isinstance(n_samples, torch.Tensor) or n_samples.dtype != torch.int32 or n_samples.device != wave.device or \
            tuple(n_samples.shape) != (wave.shape[0],) or not n_samples.is_contiguous():
        raise ValueError(f"{what}: n_samples must be a contiguous int32 tensor of {wave.shape[0]} lengths on the wave's device")
    return n_samples


def compute_device(wave, n_samples, cfg, seed=0, offsets=None):
    """The device-tensor half of compute: features of the rows of wave (B, Nmax) int16 or float32 with the int32 lengths n_samples (B),
    both on the device -- (X (B, Fmax, D) float32, n_frames (B) int32) with Fmax = max(1, cfg.frames(Nmax)).  No host trip: the output
    of resample goes straight in (a row it refused, n_out = -1, comes out with n_frames = -1).  offsets: the dither stream offset of
    each row, a list of ints or an int64 device tensor (default 0)."""
    import torch
    stype = _sample_type(wave, "features.compute_device")
    n_samples = _lengths(n_samples, wave, "features.compute_device")
    device = wave.device
    B, Nmax = wave.shape
    Fmax = max(1, cfg.frames(Nmax))
    off = None
    if offsets is not None:
        if len(offsets) != B:
            raise ValueError(f"features.compute: {len(offsets)} offsets for {B} waveforms")
        if isinstance(offsets, torch.Tensor):
            off = offsets.to(device=device, dtype=torch.int64).contiguous()
        else:
            off = torch.tensor([int(o) for o in offsets], dtype=torch.int64, device=device)
    desc = cfg.descriptor(B, Nmax, Fmax, stype, seed, off.data_ptr() if off is not None else None)
    ws = _workspace(cfg, device, desc)
    X = torch.empty(B, Fmax, cfg.dim, dtype=torch.float32, device=device)
    n_frames = torch.empty(B, dtype=torch.int32, device=device)
    _lib.check(_lib.load().astk_speech_features(C.byref(desc), C.c_void_p(wave.data_ptr()), C.c_void_p(n_samples.data_ptr()),
                                                C.c_void_p(X.data_ptr()), C.c_void_p(n_frames.data_ptr()), None,
                                                C.c_void_p(ws.data_ptr()), ws.numel(), _stream(device)))
    return X, n_frames


def speed_ratio(factor):
    """(p, q) of a speed factor, p / q = Fraction(str(factor)): 0.9 is (9, 10) -- a longer, slower copy --, 1.1 is (11, 10)."""
    f = fractions.Fraction(str(factor))
    if f <= 0:
        raise ValueError(f"speed factor {factor!r} must be positive")
    return f.numerator, f.denominator


_RESAMPLE_WORKSPACES = {}        # (reduced p, reduced q, num_zeros, rolloff, device) -> the prepared table workspace


def resample(wave, n_samples, p, q, num_zeros=6, rolloff=0.99):
    """Band-limited resampling of the rows of wave (B, Nmax) int16 or float32, lengths n_samples (B) int32, both on the device, by
    out_rate / in_rate = q / p (astk_resample; the definition is tests/resample_model.py, parity with sox / Kaldi unpinned): (Y (B,
    Mmax) float32, n_out (B) int32) with Mmax = ceil(Nmax q / p) and Y zero behind each row's n_out = ceil(n q / p).  Read at the
    input's own rate, Y is the input at speed p / q (speed_ratio).  The prepared table is cached per (p, q, num_zeros, rolloff, device)."""
    import math
    import torch
    stype = _sample_type(wave, "features.resample")
    n_samples = _lengths(n_samples, wave, "features.resample")
    p, q = int(p), int(q)
    if p < 1 or q < 1:
        raise ValueError(f"features.resample: p = {p}, q = {q}: both must be at least 1")
    g = math.gcd(p, q)
    p, q = p // g, q // g
    device = wave.device
    B, Nmax = wave.shape
    Mmax = max(1, -((-Nmax * q) // p))
    desc = _lib.ResampleDesc(B=B, Nmax=Nmax, Mmax=Mmax, sample_type=stype, p=p, q=q, num_zeros=int(num_zeros), rolloff=float(rolloff))
    lib = _lib.load()
    key = (p, q, int(num_zeros), float(rolloff), str(device))
    ws = _RESAMPLE_WORKSPACES.get(key)
    if ws is None:
        nbytes = int(lib.astk_resample_workspace_bytes(C.byref(desc)))
        if nbytes == 0:
            _lib.check(-1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _lib.check(lib.astk_resample_prepare(C.byref(desc), C.c_void_p(ws.data_ptr()), nbytes, _stream(device)))
        _RESAMPLE_WORKSPACES[key] = ws
    Y = torch.empty(B, Mmax, dtype=torch.float32, device=device)
    n_out = torch.empty(B, dtype=torch.int32, device=device)
    _lib.check(lib.astk_resample(C.byref(desc), C.c_void_p(wave.data_ptr()), C.c_void_p(n_samples.data_ptr()), C.c_void_p(Y.data_ptr()),
                                 C.c_void_p(n_out.data_ptr()), None, C.c_void_p(ws.data_ptr()), ws.numel(), _stream(device)))
    return Y, n_out


def compute(waves, cfg, device, seed=0, offsets=None):
    """Features of a list of 1-D int16 (or float32) waveforms in one launch: (X (B, Fmax, D) float32, n_frames (B) int32), both on
    `device`, X zero behind each row's frames -- the (X, x_len) pair encode_rows and the CTC paths take.  offsets: the dither stream
    offset of each row (default 0).  Packs the host list and calls compute_device."""
    import torch
    device = torch.device(device)
    if len(waves) == 0:
        raise ValueError("features.compute: no waveforms")
    arrs = [np.asarray(w) for w in waves]
    if any(a.ndim != 1 for a in arrs):
        raise ValueError("features.compute: every waveform must be 1-D")
    if all(a.dtype == np.int16 for a in arrs):
        dtype, stype = np.int16, _lib.FEAT_SAMPLE_I16
    elif all(a.dtype in (np.int16, np.float32) for a in arrs):
        dtype, stype = np.float32, _lib.FEAT_SAMPLE_F32
    else:
        raise ValueError("features.compute: waveforms must be int16 or float32 arrays")
    B = len(arrs)
    Nmax = max(1, max(len(a) for a in arrs))                 # frames() is monotone: Fmax = frames(Nmax) is the longest row's count
    host = np.zeros((B, Nmax), dtype)
    for b, a in enumerate(arrs):
        host[b, :len(a)] = a
    if offsets is not None and len(offsets) != B:
        raise ValueError(f"features.compute: {len(offsets)} offsets for {B} waveforms")
    wave = torch.from_numpy(host).to(device)
    n_samples = torch.tensor([len(a) for a in arrs], dtype=torch.int32, device=device)
    return compute_device(wave, n_samples, cfg, seed, offsets)


def _cmvn_desc(X, G, norm_vars):
    if X.dim() != 3 or str(X.dtype) != "torch.float32" or not X.is_contiguous():
        raise ValueError("cmvn: X must be a contiguous float32 (B, Fmax, D) tensor")
    return _lib.CmvnDesc(B=X.shape[0], Fmax=X.shape[1], D=X.shape[2], G=G, norm_vars=int(bool(norm_vars)))


def _i32(t, device, n, what):
    import torch
    t = torch.as_tensor(t, dtype=torch.int32).to(device).contiguous()
    if t.shape != (n,):
        raise ValueError(f"cmvn: {what} must hold one int32 per row ({n}), got shape {tuple(t.shape)}")
    return t


def cmvn_accumulate(X, n_frames, groups, stats):
    """Adds the frames of X to stats (G, 2, D + 1) float64 on X's device (Kaldi's layout; zero it before the first call); returns the
    device int32 count of rows whose group id lies outside [0, G)."""
    import torch
    G = stats.shape[0]
    if stats.dtype != torch.float64 or tuple(stats.shape) != (G, 2, X.shape[2] + 1) or not stats.is_contiguous():
        raise ValueError("cmvn_accumulate: stats must be a contiguous float64 (G, 2, D + 1) tensor")
    d = _cmvn_desc(X, G, False)
    nf, gr = _i32(n_frames, X.device, X.shape[0], "n_frames"), _i32(groups, X.device, X.shape[0], "groups")
    n_bad = torch.zeros(1, dtype=torch.int32, device=X.device)
    _lib.check(_lib.load().astk_cmvn_accumulate(C.byref(d), C.c_void_p(X.data_ptr()), C.c_void_p(nf.data_ptr()), C.c_void_p(gr.data_ptr()),
                                                C.c_void_p(stats.data_ptr()), C.c_void_p(n_bad.data_ptr()), _stream(X.device)))
    return n_bad


def cmvn_apply(X, n_frames, groups, stats, norm_vars=True, out=None):
    """y = (x - mean_g) * s_g on the frames of every row, in place (out=None) or into `out`; returns the result tensor."""
    out = X if out is None else out
    if out.shape != X.shape or out.dtype != X.dtype or not out.is_contiguous():
        raise ValueError("cmvn_apply: out must match X")
    d = _cmvn_desc(X, stats.shape[0], norm_vars)
    nf, gr = _i32(n_frames, X.device, X.shape[0], "n_frames"), _i32(groups, X.device, X.shape[0], "groups")
    _lib.check(_lib.load().astk_cmvn_apply(C.byref(d), C.c_void_p(X.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(nf.data_ptr()),
                                           C.c_void_p(gr.data_ptr()), C.c_void_p(stats.data_ptr()), _stream(X.device)))
    return out


def cmvn(X, n_frames, groups=None, norm_vars=True):
    """Accumulate and apply in place: per utterance when groups is None (group[b] = b), else per group id (a utt2spk map)."""
    import torch
    B = X.shape[0]
    if groups is None:
        groups, G = torch.arange(B, dtype=torch.int32, device=X.device), B
    else:
        groups = _i32(groups, X.device, B, "groups")
        G = int(groups.max().item()) + 1 if B else 1
        if G < 1:
            raise ValueError("cmvn: no valid group id")
    stats = torch.zeros(G, 2, X.shape[2] + 1, dtype=torch.float64, device=X.device)
    cmvn_accumulate(X, n_frames, groups, stats)
    return cmvn_apply(X, n_frames, groups, stats, norm_vars)
