"""Minimum-Bayes-risk choice in n-best lists from the command line:
    python mbr.py -m <cfg_dir> -s <set key> --nbest <pickle> [--utility bleu|edit] [--posterior-scale A] [-b U] [-w <out>]
Reads an n-best pickle of beam.py, ctc_decode.py or sample.py ({utt: [(hyp, score, ..), ..]}) and chooses one hypothesis per utterance
with ast_amd.nn.mbr_select_lists: the member with the highest mean sentence BLEU against the other members of
its list (--utility bleu, the default) or with the least summed edit distance to them (--utility edit); the pair statistics of the
lists of U utterances (-b U) come from one astk_pair_stats launch.  --posterior-scale A weighs the members of a list by
softmax(A * score) instead of equally.  Prints corpus BLEU and the word error rate of the choice against the set's references and
writes it to <out>.mbr.en (default <pickle>.mbr.en)."""
import argparse
import os
import pickle

from ast_amd.eval import Eval
from ast_amd.nn import NN, mbr_select_set


def build_parser():
    parser = argparse.ArgumentParser(description="Minimum-Bayes-risk choice in n-best lists")
    parser.add_argument("-m", "--cfg_path", help="path for model config", required=True)
    parser.add_argument("-s", "--S", help="dev/dev2/test", required=True)
    parser.add_argument("--nbest", help="n-best pickle of beam.py, ctc_decode.py or sample.py", required=True)
    parser.add_argument("--utility", choices=("bleu", "edit"), default="bleu", help="what a member gains against another (default bleu)")
    parser.add_argument("--posterior-scale", dest="posterior_scale", type=float, default=None, metavar="A",
                        help="weigh the members of a list by softmax(A * score) (default: equally)")
    parser.add_argument("-b", "--batch", type=int, default=1, help="the lists of U utterances per launch (default 1)")
    parser.add_argument("-w", "--out", help="write the choice to <out>.mbr.en (default <pickle>.mbr.en)")
    return parser


def report(nn, set_key, chosen, out_fname):
    """BLEU and WER of one hypothesis per utterance against the set's references; the hypotheses to out_fname."""
    metrics = Eval(os.path.join(nn.cfg.train["data"]["refs_path"], set_key), nn.cfg.train["data"]["n_evals"])
    hyps = nn.data_loader.get_hyps(chosen.items())
    print("MBR BLEU = {0:.2f}".format(metrics.calc_bleu(hyps) * 100))
    wer = metrics.calc_wer(hyps)
    print("MBR WER = {0:.2f} (S {1:d}, D {2:d}, I {3:d}, N {4:d})".format(wer["rate"] * 100, wer["S"], wer["D"], wer["I"], wer["N"]))
    metrics.write_to_file(hyps, out_fname)
    print("Predictions written to: {0:s}".format(out_fname))


if __name__ == "__main__":
    args = vars(build_parser().parse_args())
    nn = NN(args["cfg_path"])
    with open(args["nbest"], "rb") as f:
        nbest = pickle.load(f)
    print("-" * 80)
    print("MBR for: {0:s} set: {1:s} lists: {2:d} utility: {3:s}".format(args["cfg_path"], args["S"], len(nbest), args["utility"]))
    print("-" * 80)
    chosen = mbr_select_set(nbest, args["utility"], args["posterior_scale"], max(1, args["batch"]))
    report(nn, args["S"], chosen, (args["out"] or args["nbest"]) + ".mbr.en")
