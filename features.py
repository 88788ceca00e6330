"""Waveforms to feature files: the stage in front of every other command line here.

    python features.py --scp wav.scp --out DIR --set NAME [--conf mfcc.conf | --kind mfcc|fbank ...] [--utt2spk F] [--cmvn none|utt|spk]
                       [--norm-vars] [-b U] [--dither X --seed S] [--info-out P]
                       [--resample] [--speed 0.9,1.0,1.1] [--num-zeros Z] [--rolloff R] [--map-in P --map-out P2]

wav.scp holds `utt path` lines (16-bit PCM RIFF files; lines that end in | -- Kaldi pipe commands -- are refused).  U utterances go into
each launch, length-sorted so that the padding stays small.  Writes DIR/NAME/<utt>.npy, float32 (F, D): the files FisherDataLoader reads
as <speech_path>/<set>/<utt>.npy.  With --cmvn spk all statistics are accumulated in a first pass and applied in a second.  --info-out
writes a pickle {NAME: {utt: {"sp": F}}} in the schema of the .info files.

Resampling and speed perturbation (astk_resample, parity with sox / Kaldi unpinned).  --resample converts a file
whose rate is not sample_frequency (p / q = file rate / sample_frequency); without it such a file is an error.  --speed writes one
copy of every utterance per factor: factor 1.0 under the utterance's own name, with the bytes of a run without --speed; every other
factor f as sp<f>-<utt>, a new utterance of the new speaker sp<f>-<spk> (--cmvn spk).  The copies are ordered 1.0 first, then the
factors as listed, under each the utterances in wav.scp order; a copy's dither stream starts at the sum of the lengths (in samples
at sample_frequency, ceil(n q / p)) of the copies before it, so the output does not depend on -b.  Copies of one ratio go into
launches of their own.  --info-out lists every copy; --map-in / --map-out copy map[SET][utt] to every written copy, which with
--info-out makes the perturbed set loadable by FisherDataLoader."""
import argparse
import os
import pickle
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--scp", required=True, help="wav.scp: lines `utt path`")
    p.add_argument("--out", required=True, help="output directory (the loaders' speech_path)")
    p.add_argument("--set", required=True, dest="set_key", help="set name: files go to OUT/SET/<utt>.npy")
    p.add_argument("--conf", default=None, help="Kaldi configuration file (--key=value lines); excludes the option flags below")
    p.add_argument("--kind", choices=("mfcc", "fbank"), default="mfcc")
    p.add_argument("--sample-frequency", type=float, default=None)
    p.add_argument("--frame-length", type=float, default=None, help="milliseconds")
    p.add_argument("--frame-shift", type=float, default=None, help="milliseconds")
    p.add_argument("--num-mel-bins", type=int, default=None)
    p.add_argument("--num-ceps", type=int, default=None)
    p.add_argument("--low-freq", type=float, default=None)
    p.add_argument("--high-freq", type=float, default=None)
    p.add_argument("--window-type", choices=("povey", "hamming", "hanning", "rectangular"), default=None)
    p.add_argument("--use-energy", action="store_true", default=None)
    p.add_argument("--dither", type=float, default=None, help="default 0: deterministic output (Kaldi's default is 1.0)")
    p.add_argument("--seed", type=int, default=0, help="seed of the dither stream")
    p.add_argument("--utt2spk", default=None, help="lines `utt speaker` (needed by --cmvn spk)")
    p.add_argument("--cmvn", choices=("none", "utt", "spk"), default="none")
    p.add_argument("--norm-vars", action="store_true", help="normalise the variances too (apply-cmvn --norm-vars=true)")
    p.add_argument("-b", "--batch", type=int, default=32, help="utterances per launch")
    p.add_argument("--info-out", default=None, help="pickle {SET: {utt: {'sp': frames}}}")
    p.add_argument("-g", "--gpuid", type=int, default=0)
    p.add_argument("--resample", action="store_true", help="convert files whose rate is not sample_frequency (without it they are an error)")
    p.add_argument("--speed", default=None, help="comma-separated speed factors, e.g. 0.9,1.0,1.1: one copy of every utterance per factor")
    p.add_argument("--num-zeros", type=int, default=6, help="zero crossings of the resampling filter on each side")
    p.add_argument("--rolloff", type=float, default=0.99, help="cut-off of the resampling filter as a fraction of the narrower Nyquist")
    p.add_argument("--map-in", default=None, help="pickle map[SET][utt]: the text of the utterances")
    p.add_argument("--map-out", default=None, help="pickle with map[SET] re-keyed by every written copy (sp<f>-<utt>)")
    return p


OPTION_FLAGS = ("sample_frequency", "frame_length", "frame_shift", "num_mel_bins", "num_ceps", "low_freq", "high_freq", "window_type",
                "use_energy", "dither")


def config_from_args(args):
    import dataclasses
    from ast_amd.features import FeatureConfig
    given = {k: getattr(args, k) for k in OPTION_FLAGS if getattr(args, k) is not None}
    if args.conf is not None:
        extra = sorted(set(given) - {"dither"})
        if extra:
            raise SystemExit(f"--conf excludes the option flags: {', '.join('--' + k.replace('_', '-') for k in extra)}")
        cfg = FeatureConfig.from_kaldi_conf(args.conf, kind=args.kind)
        return dataclasses.replace(cfg, **given)
    return FeatureConfig(kind=args.kind, **given)


def read_scp(path):
    """[(utt, wav path)] of a wav.scp; pipe commands are refused."""
    out, seen = [], set()
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            if line.endswith("|"):
                raise ValueError(f"{path}:{ln}: pipe commands are not supported (convert to RIFF files first)")
            parts = line.split(None, 1)
            if len(parts) != 2:
                raise ValueError(f"{path}:{ln}: expected `utt path`")
            if parts[0] in seen:
                raise ValueError(f"{path}:{ln}: utterance {parts[0]} is listed twice")
            seen.add(parts[0])
            out.append((parts[0], parts[1]))
    return out


def read_utt2spk(path):
    m = {}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 2:
                raise ValueError(f"{path}:{ln}: expected `utt speaker`")
            m[parts[0]] = parts[1]
    return m


def load_wave(path, cfg):
    """The int16 samples of a file whose rate is the configuration's; a different rate is an error that names the file."""
    from ast_amd.features import read_wav
    x, rate = read_wav(path)
    if float(rate) != float(cfg.sample_frequency):
        raise ValueError(f"{path}: sample rate {rate} Hz, the configuration's sample_frequency is {cfg.sample_frequency:g} Hz (no resampling)")
    return x


def parse_speeds(text):
    """[(label, Fraction)] of --speed: the factors as typed (the labels of sp<f>-<utt>), 1.0 first, the others in the order listed."""
    out = []
    for tok in text.split(","):
        tok = tok.strip()
        try:
            f = Fraction(tok)
        except (ValueError, ZeroDivisionError):
            raise SystemExit(f"--speed: {tok!r} is not a factor") from None
        if f <= 0:
            raise SystemExit(f"--speed: the factor {tok} must be positive")
        if any(f == g for _, g in out):
            raise SystemExit(f"--speed: the factor {tok} is listed twice")
        out.append((tok, f))
    return [s for s in out if s[1] == 1] + [s for s in out if s[1] != 1]


def copy_name(label, factor, name):
    """The name of a copy of an utterance -- or of a speaker: factor 1 keeps the name, every other factor is a new utterance of a
    new speaker, sp<f>-<name> (Kaldi's convention)."""
    return name if factor == 1 else f"sp{label}-{name}"


def plan_copies(scp, lengths, rates, cfg, speeds):
    """The copies a run writes, in their order: the factors as parse_speeds orders them, under each the utterances in scp order.  A
    copy is a dict: name, utt, label, factor, ratio (p / q = input rate / output rate as a Fraction; 1: the samples go in as they
    are), n (samples at the configuration's rate, ceil(n_in q / p)) and start, the offset of its dither stream: the sum of n over the
    copies before it.  Nothing here depends on -b, and with the factor 1.0 first its copies start where they start without --speed."""
    target = Fraction(cfg.sample_frequency)
    copies, pos = [], 0
    for label, f in speeds:
        for u, _ in scp:
            ratio = Fraction(rates[u]) / target * f
            n = -((-lengths[u] * ratio.denominator) // ratio.numerator)
            copies.append(dict(name=copy_name(label, f, u), utt=u, label=label, factor=f, ratio=ratio, n=n, start=pos))
            pos += n
    return copies


def map_copies(map_in, set_key, copies):
    """The text map of a perturbed set: map[SET][utt] under the name of every written copy; the other sets stay as they are."""
    if set_key not in map_in:
        raise SystemExit(f"--map-in has no set {set_key}")
    src, out = map_in[set_key], {}
    for c in copies:
        if c["utt"] not in src:
            raise SystemExit(f"--map-in has no entry for {c['utt']} in {set_key}")
        out[c["name"]] = src[c["utt"]]
    return {**map_in, set_key: out}


def main(argv=None):
    import torch
    from ast_amd import features as F
    args = build_parser().parse_args(argv)
    cfg = config_from_args(args)
    if args.batch < 1:
        raise SystemExit("-b must be at least 1")
    if args.cmvn == "spk" and args.utt2spk is None:
        raise SystemExit("--cmvn spk needs --utt2spk")
    if (args.map_in is None) != (args.map_out is None):
        raise SystemExit("--map-in and --map-out go together")
    device = torch.device(f"cuda:{args.gpuid}")
    scp = read_scp(args.scp)
    speeds = parse_speeds(args.speed) if args.speed else [("1.0", Fraction(1))]
    if args.resample:
        read = {u: F.read_wav(p) for u, p in scp}
        waves, rates = {u: x for u, (x, _) in read.items()}, {u: Fraction(r) for u, (_, r) in read.items()}
    else:
        waves = {u: load_wave(p, cfg) for u, p in scp}
        rates = {u: Fraction(cfg.sample_frequency) for u in waves}
    copies = plan_copies(scp, {u: len(w) for u, w in waves.items()}, rates, cfg, speeds)
    if args.map_in:
        with open(args.map_in, "rb") as f:
            map_out = map_copies(pickle.load(f), args.set_key, copies)
    spk_of = read_utt2spk(args.utt2spk) if args.utt2spk else {}
    if args.cmvn == "spk":
        missing = [u for u, _ in scp if u not in spk_of]
        if missing:
            raise SystemExit(f"--utt2spk has no speaker for {missing[0]} ({len(missing)} utterances)")
        for c in copies:
            c["spk"] = copy_name(c["label"], c["factor"], spk_of[c["utt"]])
    speakers = {s: k for k, s in enumerate(sorted({c["spk"] for c in copies}))} if args.cmvn == "spk" else {}
    # launches: factor by factor; under a factor the copies of one ratio together (every rate gets its own launches), sorted by length
    batches = []
    for label, _ in speeds:
        mine = [c for c in copies if c["label"] == label]
        for ratio in sorted({c["ratio"] for c in mine}):
            order = sorted((c for c in mine if c["ratio"] == ratio), key=lambda c: (len(waves[c["utt"]]), c["name"]))
            batches += [order[i:i + args.batch] for i in range(0, len(order), args.batch)]
    out_dir = os.path.join(args.out, args.set_key)
    os.makedirs(out_dir, exist_ok=True)
    D = cfg.dim
    stats = torch.zeros(max(1, len(speakers)), 2, D + 1, dtype=torch.float64, device=device)
    kept, info = [], {}
    for batch in batches:
        utts, ratio = [c["name"] for c in batch], batch[0]["ratio"]
        if ratio == 1:
            X, nf = F.compute([waves[c["utt"]] for c in batch], cfg, device, seed=args.seed, offsets=[c["start"] for c in batch])
        else:
            host = np.zeros((len(batch), max(1, max(len(waves[c["utt"]]) for c in batch))), np.int16)
            for b, c in enumerate(batch):
                host[b, :len(waves[c["utt"]])] = waves[c["utt"]]
            n_in = torch.tensor([len(waves[c["utt"]]) for c in batch], dtype=torch.int32, device=device)
            Y, n_out = F.resample(torch.from_numpy(host).to(device), n_in, ratio.numerator, ratio.denominator, args.num_zeros, args.rolloff)
            X, nf = F.compute_device(Y, n_out, cfg, seed=args.seed, offsets=[c["start"] for c in batch])
        if args.cmvn == "utt":
            F.cmvn(X, nf, None, args.norm_vars)
        elif args.cmvn == "spk":
            groups = torch.tensor([speakers[c["spk"]] for c in batch], dtype=torch.int32, device=device)
            F.cmvn_accumulate(X, nf, groups, stats)
            kept.append((utts, X, nf, groups))
            continue
        _write(out_dir, utts, X, nf, info)
    for utts, X, nf, groups in kept:                             # second pass: every speaker's statistics are complete
        F.cmvn_apply(X, nf, groups, stats, args.norm_vars)
        _write(out_dir, utts, X, nf, info)
    if args.info_out:
        with open(args.info_out, "wb") as f:
            pickle.dump({args.set_key: {c["name"]: info[c["name"]] for c in copies}}, f)
    if args.map_out:
        with open(args.map_out, "wb") as f:
            pickle.dump(map_out, f)
    print(f"wrote {len(info)} feature files ({cfg.kind}, D = {D}) to {out_dir}")
    return 0


def _write(out_dir, utts, X, nf, info):
    Xh, nh = X.cpu().numpy(), nf.cpu().numpy()
    for b, u in enumerate(utts):
        n = int(nh[b])
        if n < 0:
            raise RuntimeError(f"{u}: the device refused the row")
        np.save(os.path.join(out_dir, f"{u}.npy"), np.ascontiguousarray(Xh[b, :n]))
        info[u] = {"sp": n}


if __name__ == "__main__":
    sys.exit(main())
