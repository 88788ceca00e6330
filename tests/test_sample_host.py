"""Sampled decoding, host side: the noise contract of include/astk.h ("sampled decoding on the device") restated in NumPy and pinned to
its known answers, the distribution of Gumbel-max draws from that noise, minimum-Bayes-risk selection and hypothesis cutting.  No GPU.
Every test prints its figures before it asserts."""
import numpy as np

from sample_noise_model import mix64 as _mix64, noise as _noise, row_key as _row_key


KNOWN = [((2024, 0), 0, 0, 10316691, 0.614922702, 0.721014479),
         ((2024, 0), 7, 1097, 7877032, 0.469507724, 0.279620615),
         ((2024, 0), 511, 8003, 1257711, 0.0749654695, -0.951938793),
         ((2024, 31), 0, 0, 3220600, 0.191962764, -0.501050320),
         (((1 << 64) - 1, 5), 7, 1097, 11843045, 0.70590049, 1.054745654)]


def test_known_answers_of_the_noise_contract():
    from ast_amd.seq2seq import gumbel_noise, mix64, sample_row_key
    keys = {"mix64(0)": (mix64(0), _mix64(0), 0xE220A8397B1DCDAF),
            "row_key(2024, 0)": (sample_row_key(2024, 0), _row_key(2024, 0), 0xEE8C6C05E85E6BD6),
            "row_key(2024, 31)": (sample_row_key(2024, 31), _row_key(2024, 31), 0xFBBF30B376932227),
            "row_key(2^64-1, 5)": (sample_row_key((1 << 64) - 1, 5), _row_key((1 << 64) - 1, 5), 0xB6C39F51AF8B94F6)}
    for name, (pkg, mine, want) in keys.items():
        print(f"{name}: package {pkg:#018X}, restatement {mine:#018X}, expected {want:#018X}")
        assert pkg == want and mine == want, name
    for (seed, stream), s, n, top_w, u_w, g_w in KNOWN:
        key = sample_row_key(seed, stream)
        top, u, g = _noise(key, s, n)
        pu, pg = gumbel_noise(key, s, n + 1)
        print(f"({seed}, {stream}) s {s} n {n}: word >> 40 {int(top)}, u {u:.9g} (bits {u.view(np.uint32):#010x}), g {g:.9f}; "
              f"package u {pu[n]:.9g}, g {pg[n]:.9f}")
        assert int(top) == top_w
        assert u.view(np.uint32) == np.float32(u_w).view(np.uint32)          # to the bit as float32
        assert abs(g - g_w) <= 1e-9
        assert pu.dtype == np.float32 and pu[n].view(np.uint32) == u.view(np.uint32) and pg[n] == g
    # u stays inside (0, 1) at both ends of the 24-bit range: the multiplier is the float32 next to 1 / 16777217, below 2^-24
    c = np.float32(1.0 / 16777217.0)
    lo, hi = np.float32(1) * c, np.float32(1 << 24) * c
    print(f"multiplier {float(c).hex()}, u range [{lo:.9g}, {hi:.9g}]")
    assert float(c).hex() == "0x1.fffffe0000000p-25" and 0.0 < lo and hi < 1.0


def test_gumbel_max_draws_follow_the_softmax():
    """20000 streams' draws at one step against softmax(x), chi-square with the classes of expected count below 5 pooled into one.  The
    bound dof + 6 sqrt(2 dof) is a far tail of the chi-square law (mean dof, variance 2 dof): the test is deterministic, so it only has
    to separate a working hash from a broken one."""
    x = np.random.default_rng(1).standard_normal(57) * 2
    p = np.exp(x - x.max())
    p /= p.sum()
    n_draws = 20000
    for seed in (2024, 7):
        keys = np.array([_row_key(seed, st) for st in range(n_draws)], dtype=np.uint64)
        _, u, g = _noise(keys[:, None], 3, np.arange(57)[None, :])
        assert u.min() > 0 and u.max() < 1
        counts = np.bincount((x[None, :] + g).argmax(axis=1), minlength=57).astype(np.float64)
        expect = p * n_draws
        small = expect < 5
        obs, exp_ = counts[~small], expect[~small]
        if small.any():
            obs, exp_ = np.append(obs, counts[small].sum()), np.append(exp_, expect[small].sum())
        dof = len(exp_) - 1
        chi2 = float(((obs - exp_) ** 2 / exp_).sum())
        bound = dof + 6 * np.sqrt(2 * dof)
        unpooled = float(((counts - expect) ** 2 / expect).sum())
        print(f"seed {seed}: chi-square {chi2:.1f} with {dof} degrees of freedom ({int(small.sum())} classes pooled), bound {bound:.1f}; "
              f"unpooled {unpooled:.1f} with 56")
        assert chi2 <= bound, (seed, chi2, bound)
    # rows are independent streams: two seeds, and two steps of one seed, draw different noise
    _, _, g0 = _noise(_row_key(2024, 0), 3, np.arange(57))
    _, _, g1 = _noise(_row_key(7, 0), 3, np.arange(57))
    _, _, g2 = _noise(_row_key(2024, 0), 4, np.arange(57))
    assert np.abs(g0 - g1).max() > 1 and np.abs(g0 - g2).max() > 1


def test_mbr_select_known_answers():
    from ast_amd.nn import mbr_select
    GO, EOS = 1, 2
    base = [GO, 10, 11, 12, 13, 14, 15, EOS]
    hyps = [{"hyp": [GO, 30, 31, 32, 33, 34, EOS], "score": -1.0},          # the outlier, with the best score
            {"hyp": base[:4] + [20] + base[5:], "score": -4.0},             # near-duplicates: one token off the consensus each
            {"hyp": list(base), "score": -5.0},                             # the consensus
            {"hyp": base[:6] + [21, EOS], "score": -4.5}]
    got = mbr_select(hyps)
    print("consensus among near-duplicates plus an outlier:", got)
    assert got == 2
    # ties: two identical candidates are tied in BLEU against the others -> the higher score, then the lower index
    tie = [{"hyp": list(base), "score": -3.0}, {"hyp": list(base), "score": -2.0}, {"hyp": base[:6] + [21, EOS], "score": -1.0}]
    print("tie on BLEU, scores -3 / -2:", mbr_select(tie))
    assert mbr_select(tie) == 1
    tie[0]["score"] = -2.0
    print("tie on BLEU and on the score:", mbr_select(tie))
    assert mbr_select(tie) == 0
    assert mbr_select([{"hyp": [GO, 5, EOS], "score": -0.5}]) == 0


def test_hypotheses_are_cut_behind_the_first_eos():
    from ast_amd.nn import cut_at_eos
    from ast_amd.seq2seq import ScoredPrediction
    EOS = 2
    tokens = np.array([[EOS, 7, 8, 9], [5, 6, 7, 8], [5, EOS, 9, EOS]], dtype=np.int32)
    logp = np.array([[-1.0, -2.0, -4.0, -8.0]] * 3, dtype=np.float32)
    cuts = [cut_at_eos(row, EOS) for row in tokens]
    r = ScoredPrediction(tokens, logp, None, EOS)
    print("cuts:", cuts, "scores:", r.score.tolist())
    assert cuts == [[EOS], [5, 6, 7, 8], [5, EOS]]
    assert all(isinstance(t, int) for c in cuts for t in c)
    assert r.score.tolist() == [-1.0, -15.0, -3.0] and r.nll is None and r.loss is None
