"""Waveforms to feature files: the stage in front of every other command line here.

    python features.py --scp wav.scp --out DIR --set NAME [--conf mfcc.conf | --kind mfcc|fbank ...] [--utt2spk F] [--cmvn none|utt|spk]
                       [--norm-vars] [-b U] [--dither X --seed S] [--info-out P]

wav.scp holds `utt path` lines (16-bit PCM RIFF files; lines that end in | -- Kaldi pipe commands -- are refused).  U utterances go into
each launch, length-sorted so that the padding stays small.  Writes DIR/NAME/<utt>.npy, float32 (F, D): the files FisherDataLoader reads
as <speech_path>/<set>/<utt>.npy.  With --cmvn spk all statistics are accumulated in a first pass and applied in a second.  --info-out
writes a pickle {NAME: {utt: {"sp": F}}} in the schema of the .info files."""
import argparse
import os
import pickle
import sys

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


def main(argv=None):
    import torch
    from ast_amd import features as F
    args = build_parser().parse_args(argv)
    cfg = config_from_args(args)
    if args.batch < 1:
        raise SystemExit("-b must be at least 1")
    if args.cmvn == "spk" and args.utt2spk is None:
        raise SystemExit("--cmvn spk needs --utt2spk")
    device = torch.device(f"cuda:{args.gpuid}")
    scp = read_scp(args.scp)
    waves = {u: load_wave(p, cfg) for u, p in scp}
    spk_of = read_utt2spk(args.utt2spk) if args.utt2spk else {}
    if args.cmvn == "spk":
        missing = [u for u, _ in scp if u not in spk_of]
        if missing:
            raise SystemExit(f"--utt2spk has no speaker for {missing[0]} ({len(missing)} utterances)")
    speakers = {s: k for k, s in enumerate(sorted({spk_of[u] for u, _ in scp})) } if args.cmvn == "spk" else {}
    order = sorted((u for u, _ in scp), key=lambda u: (len(waves[u]), u))
    batches = [order[i:i + args.batch] for i in range(0, len(order), args.batch)]
    # the dither stream of an utterance starts at its first sample's position in the scp's concatenation: independent of -b
    starts, pos = {}, 0
    for u, _ in scp:
        starts[u] = pos
        pos += len(waves[u])
    out_dir = os.path.join(args.out, args.set_key)
    os.makedirs(out_dir, exist_ok=True)
    D = cfg.dim
    stats = torch.zeros(max(1, len(speakers)), 2, D + 1, dtype=torch.float64, device=device)
    kept, info = [], {}
    for utts in batches:
        X, nf = F.compute([waves[u] for u in utts], cfg, device, seed=args.seed, offsets=[starts[u] for u in utts])
        if args.cmvn == "utt":
            F.cmvn(X, nf, None, args.norm_vars)
        elif args.cmvn == "spk":
            groups = torch.tensor([speakers[spk_of[u]] for u in utts], dtype=torch.int32, device=device)
            F.cmvn_accumulate(X, nf, groups, stats)
            kept.append((utts, X, nf, groups))
            continue
        _write(out_dir, utts, X, nf, info)
    for utts, X, nf, groups in kept:                             # second pass: every speaker's statistics are complete
        F.cmvn_apply(X, nf, groups, stats, args.norm_vars)
        _write(out_dir, utts, X, nf, info)
    if args.info_out:
        with open(args.info_out, "wb") as f:
            pickle.dump({args.set_key: {u: info[u] for u, _ in scp}}, f)
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
