"""beam.py drop-in (beam.py:46-146 of the reference):
    python beam.py -m <cfg_dir> -n <N hyps kept> -k <K candidates per step> -s <set key> -w <length weight> [--resume] [-b U] [--device] [--batch-encode] [joint decoding options]
Beam search over one set with the newest checkpoint of the experiment, n-best lists pickled to
<cfg_dir>/<set>_beam_N-<N>_K-<K>.p, the length-normalised best hypothesis of each utterance scored with corpus BLEU
(ast_amd.eval) and written to <cfg_dir>/<set>_beam_N-<N>_K-<K>_W-<W>.en.  -b U decodes U utterances per batched search on the
GPU (ast_amd.nn.decode_beam_batch): the same utterances and hypotheses, the same files.  --device runs the whole search of a group
of utterances (-b U of them, default 32) in persistent launches on the GPU (ast_amd.nn.decode_beam_device): the same files again.
The joint decoding options are the library's (ast_amd.nn.add_joint_decoding_arguments; `python beam.py -h` lists them, DESIGN.md
section 30): with -b U they rank every candidate by the attention decoder and the encoder's second head together; the pickled score
is then that joint score and every entry carries the two separate scores behind its three fields."""
import argparse
import itertools
import math
import os
import pickle
import random

from tqdm import tqdm

from ast_amd._lib import BEAM_MAX_K, BEAM_MAX_N
from ast_amd.eval import Eval
from ast_amd.nn import NN, add_joint_decoding_arguments, joint_decoding_kwargs, joint_entry_scores


def rerank_hypothesis(beam_hyps, weight):
    """score / (len - 2)^weight, best first (beam.py:32-34).  A hypothesis of just [GO, EOS] has len - 2 = 0, which divides by
    zero in the reference; it is ranked with a length of 1 here."""
    return sorted([(h[0], h[1] / math.pow(max(len(h[0]) - 2, 1), weight), len(h[0])) for h in beam_hyps], reverse=True, key=lambda t: t[1])


def get_best_hyps(utts_beam, W):
    return {u: list(rerank_hypothesis(hyps, weight=W)[0][0]) for u, hyps in utts_beam.items()}


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="Beam search to find best predictions for NN model")
    parser.add_argument("-m", "--cfg_path", help="path for model config", required=True)
    parser.add_argument("-n", "--N", help="number of hyps", required=True)
    parser.add_argument("-k", "--K", help="softmax selection", required=True)
    parser.add_argument("-s", "--S", help="dev/dev2/test", required=True)
    parser.add_argument("-w", "--W", help="len normalization weight", required=True)
    parser.add_argument("--resume", action="store_true", help="re-score the saved beam results instead of decoding again")
    parser.add_argument("-b", "--batch", type=int, default=0, help="decode U utterances at once on the GPU (same hypotheses)")
    parser.add_argument("--device", action="store_true", help="the whole search in persistent launches on the GPU (same hypotheses)")
    parser.add_argument("--batch-encode", dest="batch_encode", action="store_true",
                        help="encode the utterances of a call in one padded batch with per-row lengths instead of one by one (same encodings; effective with -b U / --device)")
    add_joint_decoding_arguments(parser)
    args = vars(parser.parse_args())
    cfg_path, N, K, W, set_key = args["cfg_path"], int(args["N"]), int(args["K"]), float(args["W"]), args["S"]
    U = args["batch"]
    if args["device"] and U < 1:
        U = 32
    if U >= 1 and not (N <= BEAM_MAX_N and K <= BEAM_MAX_K):
        print("-b {0:d}: N and K above {1:d} / {2:d} are decoded one utterance at a time".format(U, BEAM_MAX_N, BEAM_MAX_K))
        U = 0
    joint = joint_decoding_kwargs(args, batched=U >= 1, device=args["device"])          # (exits with a message where the search cannot rank jointly)
    nn = NN(cfg_path)
    nn.model.batch_encode = bool(args["batch_encode"])
    metrics = Eval(os.path.join(nn.cfg.train["data"]["refs_path"], set_key), nn.cfg.train["data"]["n_evals"])
    random.seed("meh")
    print("-" * 80)
    print("Beam for: {0:s} gpu: {1:d}".format(cfg_path, nn.gpuid))
    print("-" * 80)
    beam_fname = os.path.join(cfg_path, "{0:s}_beam_N-{1:d}_K-{2:d}.p".format(set_key, N, K))
    if args["resume"]:
        print("Loading saved beam results")
        with open(beam_fname, "rb") as f:
            beam = pickle.load(f)
    else:
        print("Computing beam results")
        stop_limit = nn.cfg.train["data"]["max_pred"]
        beam = {}
        with tqdm(total=nn.data_loader.n_utts[set_key], ncols=80) as pbar:
            if U >= 1:
                # the same utterances, order and truncation as below, U of them per batched search
                group = []
                for utt in itertools.chain(nn.data_loader.get_batch(1, set_key, train=False, labels=False), [None]):
                    if utt is not None:
                        group.append(utt)
                    if group and (utt is None or len(group) == U):
                        search = nn.decode_beam_device if args["device"] else nn.decode_beam_batch
                        lists = search([g["X"] for g in group], stop_limit=stop_limit, N=N, K=K, **joint)
                        for g, n_best in zip(group, lists):
                            beam[g["utts"][0]] = [(e["hyp"], e["score"], e["attn_history"]) + joint_entry_scores(e) for e in n_best]
                        pbar.update(len(group))
                        group = []
            else:
                for utt in nn.data_loader.get_batch(1, set_key, train=False, labels=False):
                    n_best = nn.decode_beam(utt["X"], stop_limit=stop_limit, N=N, K=K)
                    beam[utt["utts"][0]] = [(e["hyp"], e["score"], e["attn_history"]) for e in n_best]
                    pbar.update(len(utt["X"]))
        if args["device"] and U >= 1:
            print("search path: {0:s}".format(str(nn.model.last_beam_path)))
        print("saving hyps")
        with open(beam_fname, "wb") as f:
            pickle.dump(beam, f)
    hyps = nn.data_loader.get_hyps(get_best_hyps(beam, W).items())
    print("BLEU = {0:.2f}".format(metrics.calc_bleu(hyps) * 100))
    out_fname = os.path.join(cfg_path, "{0:s}_beam_N-{1:d}_K-{2:d}_W-{3:.2f}.en".format(set_key, N, K, W))
    metrics.write_to_file(hyps, out_fname)
    print("Predictions written to: {0:s}".format(out_fname))
