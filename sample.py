"""Ancestral sampling from the command line:
    python sample.py -m <cfg_dir> -s <set key> -n <N samples> [-t <temperature>] [-k <top_k>] [-p <top_p>] [--seed <S>] [--mbr]
                     [--utility bleu|edit] [-w <out pickle>] [-b U]
Draws N scored samples of every utterance of the set with the newest checkpoint of the experiment (NN.sample_set) and pickles them
to <cfg_dir>/<set>_sample_N-<N>_T-<T>.p (or -w) in the format of beam.py's n-best pickle, so `score.py --nbest` reads it unchanged.
-k / -p truncate every draw (SpeechEncoderDecoder.sample: the top_k <= 16 largest tempered logits, cut to the nucleus of mass top_p and
renormalised; -p needs -k); the default name then ends _K-<k>_P-<p>.p, and the scores are log-probabilities under the truncated distribution.
-b U packs the rows of up to U utterances into one call (every row attends over its own utterance's length): the same samples.
--mbr also picks one sample per utterance by minimum Bayes risk (ast_amd.nn.mbr_select: the highest mean sentence BLEU against the
other samples), scores the choice with corpus BLEU (ast_amd.eval) and writes it beside the pickle as <pickle>.mbr.en.
--utility bleu|edit implies --mbr and makes the choice through ast_amd.nn.mbr_select_lists instead (the pair
statistics of the lists of U utterances in one astk_pair_stats launch; edit: the sample with the least summed edit distance to the
others); it prints the word error rate of the choice beside its BLEU."""
import argparse
import os
import pickle

from ast_amd.eval import Eval
from ast_amd.nn import NN, mbr_select, mbr_select_set
from ast_amd.seq2seq import checked_truncation


def build_parser():
    parser = argparse.ArgumentParser(description="Sample translations from the NN model")
    parser.add_argument("-m", "--cfg_path", help="path for model config", required=True)
    parser.add_argument("-s", "--S", help="dev/dev2/test", required=True)
    parser.add_argument("-n", "--N", help="number of samples per utterance", type=int, required=True)
    parser.add_argument("-t", "--temperature", type=float, default=1.0, help="softmax temperature (default 1)")
    parser.add_argument("--seed", type=int, default=0, help="seed of the draws (default 0)")
    parser.add_argument("--mbr", action="store_true", help="also choose one sample per utterance by minimum Bayes risk")
    parser.add_argument("--utility", choices=("bleu", "edit"), default=None,
                        help="implies --mbr: choose on the GPU by mean sentence BLEU or by summed edit distance (ast_amd.nn.mbr_select_lists)")
    parser.add_argument("-w", "--out", help="pickle to write (default <cfg_dir>/<set>_sample_N-<N>_T-<T>.p)")
    parser.add_argument("-b", "--batch", type=int, default=1, help="pack the rows of U utterances into one call (default 1)")
    parser.add_argument("--batch-encode", dest="batch_encode", action="store_true",
                        help="encode the utterances of a call in one padded batch with per-row lengths instead of one by one (same encodings; effective with -b U)")
    parser.add_argument("-k", "--top-k", dest="top_k", type=int, default=None, help="draw among the top_k (1..16) best tokens only")
    parser.add_argument("-p", "--top-p", dest="top_p", type=float, default=1.0,
                        help="... cut to the smallest set of them holding a mass top_p in (0, 1] (needs -k; default 1: no cut)")
    return parser


def default_name(set_key, N, T, top_k=None, top_p=1.0):
    """The default pickle name: a suffix for the truncation only when it is on."""
    trunc = "" if top_k is None else "_K-{0:d}_P-{1:.2f}".format(top_k, top_p)
    return "{0:s}_sample_N-{1:d}_T-{2:.2f}{3:s}.p".format(set_key, N, T, trunc)


if __name__ == "__main__":
    parser = build_parser()
    args = vars(parser.parse_args())
    cfg_path, set_key, N, T = args["cfg_path"], args["S"], args["N"], args["temperature"]
    if N < 1:
        parser.error("-n must be at least 1")
    try:
        top_k, top_p = checked_truncation(args["top_k"], args["top_p"])
    except ValueError as e:
        parser.error(str(e))
    nn = NN(cfg_path)
    nn.model.batch_encode = bool(args["batch_encode"])
    print("-" * 80)
    print("Sampling for: {0:s} set: {1:s} gpu: {2:d}".format(cfg_path, set_key, nn.gpuid))
    print("-" * 80)
    samples = nn.sample_set(set_key, N, args["seed"], temperature=T, utts_per_call=max(1, args["batch"]), top_k=top_k, top_p=top_p)
    out_fname = args["out"] or os.path.join(cfg_path, default_name(set_key, N, T, top_k, top_p))
    with open(out_fname, "wb") as f:
        pickle.dump(samples, f)
    print("Samples written to: {0:s} (utterances: {1:d}, path: {2})".format(out_fname, len(samples), nn.model.last_predict_path))
    if args["utility"] is not None:
        metrics = Eval(os.path.join(nn.cfg.train["data"]["refs_path"], set_key), nn.cfg.train["data"]["n_evals"])
        hyps = nn.data_loader.get_hyps(mbr_select_set(samples, args["utility"], utts_per_call=max(1, args["batch"])).items())
        wer = metrics.calc_wer(hyps)
        print("MBR BLEU = {0:.2f}".format(metrics.calc_bleu(hyps) * 100))
        print("MBR WER = {0:.2f} (S {1:d}, D {2:d}, I {3:d}, N {4:d})".format(wer["rate"] * 100, wer["S"], wer["D"], wer["I"], wer["N"]))
        metrics.write_to_file(hyps, out_fname + ".mbr.en")
        print("Predictions written to: {0:s}".format(out_fname + ".mbr.en"))
    elif args["mbr"]:
        metrics = Eval(os.path.join(nn.cfg.train["data"]["refs_path"], set_key), nn.cfg.train["data"]["n_evals"])
        chosen = {u: list(lst[mbr_select([{"hyp": h, "score": sc} for h, sc, _ in lst])][0]) for u, lst in samples.items()}
        hyps = nn.data_loader.get_hyps(chosen.items())
        print("MBR BLEU = {0:.2f}".format(metrics.calc_bleu(hyps) * 100))
        metrics.write_to_file(hyps, out_fname + ".mbr.en")
        print("Predictions written to: {0:s}".format(out_fname + ".mbr.en"))
