"""Forced decoding from the command line:
    python score.py -m <cfg_dir> -s <set key> [--nbest <beam pickle> [-b U]] [--alignments <out.npz>] [the option of ast_amd.nn.add_alignment_arguments]
Scores the set's references with the newest checkpoint of the experiment (NN.score_set): log-probability and token count per utterance
in <cfg_dir>/<set>_scores.txt, the teacher-forced dev loss and the perplexity on the terminal.  --nbest scores every hypothesis of a
beam.py pickle instead -- each utterance on its own, its X repeated over its hypotheses' rows and the hypotheses PAD-padded, the
encoding the search itself saw -- writes the model score beside the beam score to <pickle>.scores.txt and prints the largest
difference; -b U packs the hypotheses of up to U utterances into one call (ast_amd.nn.score_hypotheses_packed: every row attends over
its own utterance's length, so the scores are those of -b 1).  --alignments also saves the attention rows, one (steps, T'') array per utterance (or per hypothesis: key utt#rank).
The CTC head's forced alignments (ast_amd.nn.write_alignment_file: Viterbi segments per token in encoder and input frames, confidences, the
best-path and the full-sum score; keys utt/segments, utt/segments_input, utt/labels, utt/confidence, utt/score, utt/total_logp, with
--nbest utt#rank/...) go to a file of their own; without that flag nothing else happens."""
import argparse
import itertools
import os
import pickle

import numpy as np
from tqdm import tqdm

from ast_amd.nn import NN, add_alignment_arguments, score_hypotheses, score_hypotheses_packed, write_alignment_file
from ast_amd.seq2seq import using_config


def score_references(nn, set_key, with_alpha):
    """(rows, dev_loss, ppl, alignments): NN.score_set, or the same pass batch by batch when the attention rows are wanted."""
    if not with_alpha:
        scores, dev_loss, ppl = nn.score_set(set_key)
        return scores, dev_loss, ppl, {}
    rows, losses, align = [], [], {}
    for batch in nn.data_loader.get_batch(nn.cfg.train["batch_size"], set_key, train=False, labels=True):
        with using_config("train", False):
            r = nn.model.score(batch["X"], batch["y"], return_alpha=True)
        rows.extend(zip(batch["utts"], r.score.tolist(), r.n_tokens.tolist()))
        losses.append(r.loss / int(batch["y"].shape[1]))
        for i, u in enumerate(batch["utts"]):
            align[u] = r.alpha[i]
    n_tok = sum(n for _, _, n in rows)
    ppl = float(np.exp(-sum(lp for _, lp, _ in rows) / n_tok)) if n_tok else float("nan")
    return rows, (sum(losses) / len(losses) if losses else 0.0), ppl, align


def score_nbest(nn, set_key, beam, with_alpha, utts_per_call=1):
    """rows of (utt, rank, beam score, model score, n tokens) for every hypothesis of `beam` (utt -> [(hyp, score, attn_history)]);
    utts_per_call = U > 1: up to U utterances per call."""
    rows, align = [], {}
    with tqdm(total=len(beam), ncols=80) as pbar:
        if utts_per_call > 1:
            group = []
            for utt in itertools.chain(nn.data_loader.get_batch(1, set_key, train=False, labels=False), [None]):
                if utt is not None and utt["utts"][0] in beam:
                    group.append(utt)
                if group and (utt is None or len(group) == utts_per_call):
                    names = [g["utts"][0] for g in group]
                    with using_config("train", False):
                        res = score_hypotheses_packed(nn.model, [g["X"] for g in group], [[list(h[0]) for h in beam[u]] for u in names],
                                                      return_alpha=with_alpha, max_utts=utts_per_call)
                    for u, (scores, r) in zip(names, res):
                        for k, (h, sc) in enumerate(zip(beam[u], scores)):
                            rows.append((u, k, float(h[1]), sc, len(h[0]) - 1))
                            if with_alpha:
                                align["{0:s}#{1:d}".format(u, k)] = r.alpha[k, :len(h[0]) - 1]
                    pbar.update(len(group))
                    group = []
            return rows, align
        for utt in nn.data_loader.get_batch(1, set_key, train=False, labels=False):
            u = utt["utts"][0]
            if u not in beam:
                continue
            hyps = [list(h[0]) for h in beam[u]]
            with using_config("train", False):
                scores, r = score_hypotheses(nn.model, utt["X"], hyps, return_alpha=with_alpha)
            for k, (h, sc) in enumerate(zip(beam[u], scores)):
                rows.append((u, k, float(h[1]), sc, len(h[0]) - 1))
                if with_alpha:
                    align["{0:s}#{1:d}".format(u, k)] = r.alpha[k, :len(h[0]) - 1]
            pbar.update(1)
    return rows, align


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="Score given translations with the NN model (forced decoding)")
    parser.add_argument("-m", "--cfg_path", help="path for model config", required=True)
    parser.add_argument("-s", "--S", help="dev/dev2/test", required=True)
    parser.add_argument("--nbest", help="a beam.py pickle: score its hypotheses instead of the references")
    parser.add_argument("--alignments", help="write the attention rows to this .npz")
    parser.add_argument("-b", "--batch", type=int, default=1, help="with --nbest: pack the hypotheses of U utterances into one call (default 1)")
    parser.add_argument("--batch-encode", dest="batch_encode", action="store_true",
                        help="encode the utterances of a call in one padded batch with per-row lengths instead of one by one (same encodings; effective with -b U)")
    add_alignment_arguments(parser)
    args = vars(parser.parse_args())
    cfg_path, set_key = args["cfg_path"], args["S"]
    nn = NN(cfg_path)
    nn.model.batch_encode = bool(args["batch_encode"])
    print("-" * 80)
    print("Scoring: {0:s} set: {1:s} gpu: {2:d}".format(cfg_path, set_key, nn.gpuid))
    print("-" * 80)
    if args["nbest"]:
        with open(args["nbest"], "rb") as f:
            beam = pickle.load(f)
        rows, align = score_nbest(nn, set_key, beam, bool(args["alignments"]), max(1, args["batch"]))
        out_fname = args["nbest"] + ".scores.txt"
        with open(out_fname, "w") as f:
            for u, k, bs, ms, n in rows:
                f.write("{0:s} {1:d} {2:.6f} {3:.6f} {4:d}\n".format(u, k, bs, ms, n))
        diff = max((abs(bs - ms) for _, _, bs, ms, _ in rows), default=0.0)
        print("hypotheses scored = {0:d}, largest |beam score - model score| = {1:.3e}".format(len(rows), diff))
    else:
        rows, dev_loss, ppl, align = score_references(nn, set_key, bool(args["alignments"]))
        out_fname = os.path.join(cfg_path, "{0:s}_scores.txt".format(set_key))
        with open(out_fname, "w") as f:
            for u, lp, n in rows:
                f.write("{0:s} {1:.6f} {2:d}\n".format(u, lp, n))
        print("forced dev loss = {0:.4f}, perplexity = {1:.4f}".format(dev_loss, ppl))
    print("Scores written to: {0:s} (path: {1})".format(out_fname, nn.model.last_score_path))
    if args["alignments"]:
        np.savez_compressed(args["alignments"], **align)
        print("Alignments written to: {0:s}".format(args["alignments"]))
    write_alignment_file(nn, set_key, args, beam if args["nbest"] else None)
