"""CTC prefix beam search from the command line:
    python ctc_decode.py -m <cfg_dir> -s <set key> -n <N> -c <C> [-w <out pickle>] [--rescore <W> [-b U] [--batch-encode]] [--wer]
Decodes every utterance of the set with the CTC head of the newest checkpoint alone (NN.ctc_beam_set: the N most probable label
strings, C labels proposed per frame) and pickles the n-best lists to <cfg_dir>/<set>_ctc_N-<N>_C-<C>.p (or -w)
in the format of beam.py's n-best pickle, so `score.py --nbest` reads it unchanged.  --rescore W adds the second pass: the attention
decoder scores every hypothesis (ast_amd.nn.rescore_ctc_nbest; -b U packs the hypotheses of up to U utterances into one call) and the
lists are ranked by (1 - W) * attention + W * CTC; the tuples then end with the two terms, as beam.py's do after a joint search.
--wer prints the word error rate of every list's first hypothesis against the set's references (ast_amd.eval.error_rate, DESIGN.md
section 34).  Needs rnn_config.ctc in model_cfg.json."""
import argparse
import itertools
import os
import pickle

from ast_amd.eval import Eval
from ast_amd.nn import NN, joint_entry_scores, rescore_ctc_nbest


def build_parser():
    parser = argparse.ArgumentParser(description="N-best lists from the CTC head (prefix beam search)")
    parser.add_argument("-m", "--cfg_path", help="path for model config", required=True)
    parser.add_argument("-s", "--S", help="dev/dev2/test", required=True)
    parser.add_argument("-n", "--N", help="beam width (1..16)", type=int, required=True)
    parser.add_argument("-c", "--C", help="labels proposed per frame (1..16)", type=int, required=True)
    parser.add_argument("-w", "--out", help="pickle to write (default <cfg_dir>/<set>_ctc_N-<N>_C-<C>.p)")
    parser.add_argument("--rescore", type=float, default=None, metavar="W",
                        help="second pass: rank by (1 - W) * attention score + W * CTC score, W in [0, 1]")
    parser.add_argument("-b", "--batch", type=int, default=1, help="with --rescore: pack the hypotheses of U utterances into one call (default 1)")
    parser.add_argument("--batch-encode", dest="batch_encode", action="store_true",
                        help="encode the utterances of a call in one padded batch with per-row lengths instead of one by one (same encodings; effective with -b U)")
    parser.add_argument("--wer", action="store_true", help="print the word error rate of the 1-best against the set's references")
    return parser


def wer_of_best(nn, set_key, nbest):
    """Eval.calc_wer of every list's first hypothesis against the references under data.refs_path."""
    metrics = Eval(os.path.join(nn.cfg.train["data"]["refs_path"], set_key), nn.cfg.train["data"]["n_evals"])
    return metrics.calc_wer(nn.data_loader.get_hyps((u, list(lst[0][0])) for u, lst in nbest.items()))


def default_name(set_key, N, C, weight=None):
    """The default pickle name: a suffix for the second pass only when it is on."""
    return "{0:s}_ctc_N-{1:d}_C-{2:d}{3:s}.p".format(set_key, N, C, "" if weight is None else "_W-{0:.2f}".format(weight))


def rescore_set(nn, set_key, nbest, weight, utts_per_call):
    """The pickle's lists after the second pass, U utterances per call."""
    out, group = {}, []
    for utt in itertools.chain(nn.data_loader.get_batch(1, set_key, train=False, labels=False), [None]):
        if utt is not None and utt["utts"][0] in nbest:
            group.append(utt)
        if group and (utt is None or len(group) == utts_per_call):
            names = [g["utts"][0] for g in group]
            lists = rescore_ctc_nbest(nn.model, [g["X"] for g in group], [[{"hyp": h, "score": sc} for h, sc, _ in nbest[u]] for u in names],
                                      weight, max_utts=utts_per_call)
            for u, lst in zip(names, lists):
                out[u] = [(e["hyp"], e["score"], []) + joint_entry_scores(e) for e in lst]
            group = []
    return out


if __name__ == "__main__":
    parser = build_parser()
    args = vars(parser.parse_args())
    cfg_path, set_key, N, C, W = args["cfg_path"], args["S"], args["N"], args["C"], args["rescore"]
    if W is not None and not 0.0 <= W <= 1.0:
        parser.error("--rescore must lie in [0, 1]")
    nn = NN(cfg_path)
    if not nn.model.ctc_head:
        parser.error("ctc_decode.py needs the CTC head: set rnn_config.ctc = true in model_cfg.json")
    nn.model.batch_encode = bool(args["batch_encode"])
    print("-" * 80)
    print("CTC beam for: {0:s} set: {1:s} gpu: {2:d}".format(cfg_path, set_key, nn.gpuid))
    print("-" * 80)
    try:
        nbest = nn.ctc_beam_set(set_key, N, C)
    except ValueError as e:
        parser.error(str(e))
    if W is not None:
        nbest = rescore_set(nn, set_key, nbest, W, max(1, args["batch"]))
    out_fname = args["out"] or os.path.join(cfg_path, default_name(set_key, N, C, W))
    with open(out_fname, "wb") as f:
        pickle.dump(nbest, f)
    print("Hypotheses written to: {0:s} (utterances: {1:d}, path: {2})".format(out_fname, len(nbest), "ctc_beam" if W is None else "ctc_beam + rescore"))
    if args["wer"]:
        wer = wer_of_best(nn, set_key, nbest)
        print("WER = {0:.2f} (S {1:d}, D {2:d}, I {3:d}, N {4:d})".format(wer["rate"] * 100, wer["S"], wer["D"], wer["I"], wer["N"]))
