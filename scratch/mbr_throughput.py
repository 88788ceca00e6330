"""What minimum-Bayes-risk selection costs, in one process:

    python scratch/mbr_throughput.py

(a) ms per utterance of mbr_select (the host loop: N (N - 1) calls of corpus_bleu per utterance; unchanged code, the baseline) against
    mbr_select_lists with U = 1 and U = 32 utterances per astk_pair_stats launch and both utilities, for N = 8 and N = 32 on 64
    utterances of about 40 tokens (N near-duplicates of one string each).  Wall clock around whole calls, read-back included;
    ALTERNATING block by block (5 blocks behind one warm-up pass each), the median over the blocks and their spread.  The choices of
    the "bleu" paths are asserted equal to mbr_select's.
(b) The operator alone with device events at P = 32 * 496 pairs (32 lists of 32, the pairs i < j), strings of about 40 tokens and of
    512 tokens: us per launch, the DP cells of a launch (sum of La * Lb) and cells per second."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UTTS, LENGTH, BLOCKS = 64, 40, 5
OP_BLOCKS, OP_CALLS, OP_WARMUP = 10, 10, 5


def report(tag, v, unit):
    v = sorted(v)
    med = v[len(v) // 2]
    print(f"{tag:44s} median {med:10.3f} {unit}  spread {(v[-1] - v[0]) / med * 100:5.1f} %  blocks {[round(x, 3) for x in v]}")
    return med


def make_lists(n_lists, N, length, seed):
    """n_lists lists of N near-duplicates of one random string each (a few substitutions, deletions and insertions), scored at random."""
    import random
    rng = random.Random(seed)
    lists = []
    for _ in range(n_lists):
        base = [rng.randrange(4, 1000) for _ in range(length)]
        lst = []
        for _ in range(N):
            h = list(base)
            for _ in range(rng.randrange(0, max(2, length // 5))):
                k, op = rng.randrange(len(h)), rng.randrange(3)
                if op == 0:
                    h[k] = rng.randrange(4, 1000)
                elif op == 1 and len(h) > 2:
                    del h[k]
                else:
                    h.insert(k, rng.randrange(4, 1000))
            lst.append({"hyp": [1] + h[:510] + [2], "score": -rng.random() * 20})
        lists.append(lst)
    return lists


def selection():
    from ast_amd.nn import mbr_select, mbr_select_lists
    for N in (8, 32):
        lists = make_lists(UTTS, N, LENGTH, N)
        got = {}

        def host():
            got["host"] = [mbr_select(l) for l in lists]

        def device(utility, U):
            def f():
                got[utility, U] = [k for lo in range(0, UTTS, U) for k in mbr_select_lists(lists[lo:lo + U], utility)]
            return f
        paths = {"mbr_select (host)": host}
        for utility in ("bleu", "edit"):
            for U in (1, 32):
                paths[f"mbr_select_lists {utility} U {U}"] = device(utility, U)
        for f in paths.values():
            f()
        ms = {k: [] for k in paths}
        for r in range(BLOCKS):
            for k in (list(paths) if r % 2 == 0 else list(paths)[::-1]):
                t0 = time.perf_counter()
                paths[k]()
                ms[k].append((time.perf_counter() - t0) / UTTS * 1e3)
        assert got["bleu", 1] == got["bleu", 32] == got["host"] and got["edit", 1] == got["edit", 32]
        print(f"(a) N {N}, {UTTS} utterances of about {LENGTH} tokens; the edit choice differs from the bleu choice in "
              f"{sum(a != b for a, b in zip(got['edit', 1], got['host']))} of {UTTS} lists")
        med = {k: report(k, v, "ms/utt") for k, v in ms.items()}
        for k, v in med.items():
            if k != "mbr_select (host)":
                print(f"    host / {k} = {med['mbr_select (host)'] / v:.1f} x")


def operator_alone():
    import numpy as np
    import torch
    from ast_amd import _lib
    lib = _lib.load()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for length in (LENGTH, 510):
        lists = make_lists(32, 32, length, 100 + length)
        pool = [h["hyp"] for l in lists for h in l]
        pairs = [(32 * u + i, 32 * u + j) for u in range(32) for i in range(32) for j in range(i + 1, 32)]
        lens = np.asarray([len(p) for p in pool], np.int32)
        tokens = np.zeros((len(pool), int(lens.max())), np.int32)
        for i, p in enumerate(pool):
            tokens[i, :len(p)] = p
        cells = int(sum(int(lens[a]) * int(lens[b]) for a, b in pairs))
        t, l, p = torch.from_numpy(tokens).cuda(), torch.from_numpy(lens).cuda(), torch.tensor(pairs, dtype=torch.int32).cuda()
        out = torch.empty(len(pairs), 8, dtype=torch.int32, device="cuda")
        n_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        d = _lib.PairStatsDesc(len(pool), tokens.shape[1], len(pairs))

        def call(count):
            _lib.check(lib.astk_pair_stats(C.byref(d), t.data_ptr(), l.data_ptr(), p.data_ptr(), out.data_ptr(), n_bad.data_ptr() if count else None, s))
        us = {"astk_pair_stats": [], "astk_pair_stats with n_bad": []}
        for k in us:
            for _ in range(OP_WARMUP):
                call(k.endswith("n_bad"))
        torch.cuda.synchronize()
        for r in range(OP_BLOCKS):
            for k in (list(us) if r % 2 == 0 else list(us)[::-1]):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(OP_CALLS):
                    call(k.endswith("n_bad"))
                b.record()
                b.synchronize()
                us[k].append(a.elapsed_time(b) / OP_CALLS * 1e3)
        assert int(n_bad[0]) == 0 and int(out[:, 0].min()) >= 0
        print(f"(b) P {len(pairs)} pairs, lengths {int(lens.min())}..{int(lens.max())}: {cells / 1e6:.2f} M DP cells per launch, mean distance {float(out[:, 0].float().mean()):.1f}")
        for k, v in us.items():
            med = report(k, v, "us/launch")
            print(f"    {cells / med / 1e3:.2f} G cells/s")


if __name__ == "__main__":
    import torch
    assert torch.cuda.is_available(), "a timing needs the GPU"
    selection()
    operator_alone()
