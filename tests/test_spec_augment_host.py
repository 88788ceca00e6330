"""CPU tests of SpecAugment in the training loader (include/astk.h astk_spec_augment): the draw contract's known
answers, ast_amd.spec_augment against the independent model of tests/spec_augment_model.py, the uniformity of the drawn widths, the
config checks, and the CPU loader's batches -- counters across batches, epochs and ranks, padding, targets and evaluation batches."""
import random

import numpy as np
import pytest

import spec_augment_model as SM


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


# ------------------------------------------------------------------ 1. the contract
KNOWN = [  # counter, D, len, config, frequency spans, time spans -- (start, width), seed 2024
    (0, 80, 800, SM.cfg(), [(56, 10), (51, 11)], [(680, 34), (211, 9)]),
    (1, 80, 800, SM.cfg(), [(33, 4), (30, 2)], [(349, 31), (286, 8)]),
    (2**32 - 1, 13, 37, SM.cfg(freq_width=27), [(1, 8), (1, 11)], [(34, 3), (14, 3)]),
    (2**32, 13, 1, SM.cfg(freq_width=27, time_ratio=1.0), [(3, 10), (7, 5)], [(0, 1), (0, 0)]),
]


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: "n{0}_D{1}_len{2}".format(*c[:3]))
def test_known_answers(case):
    from ast_amd import spec_augment as SA
    n, D, length, c, freq, time = case
    assert SM.key(2024, 0) == 0xEE8C6C05E85E6BD6
    assert SM.spans(2024, n, D, length, c) == (freq, time)
    assert SA.spec_spans(2024, n, D, length, SA.checked_spec_augment(c)) == (freq, time)


def test_spec_spans_agree_with_the_model():
    from ast_amd import spec_augment as SA
    rng = random.Random(5)
    edges = [0, 1, 2**32 - 1, 2**32, 2**32 + 1, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 1]
    for k in range(200):
        seed = rng.getrandbits(64) if k % 3 else rng.randrange(5000)
        n = edges[k % len(edges)] if k % 2 else rng.getrandbits(64)
        D, length = rng.choice([1, 13, 40, 80, 257]), rng.choice([1, 2, 5, 37, 799, 800, 2000])
        c = {"freq_masks": rng.randrange(9), "freq_width": rng.choice([0, 1, 15, 27, 300]), "time_masks": rng.randrange(9),
             "time_width": rng.choice([0, 1, 40, 5000]), "time_ratio": rng.choice([0.0, 0.001, 0.2, 0.5, 1.0]), "fill": "zero", "seed": seed}
        got = SA.spec_spans(seed, n, D, length, c)
        assert got == SM.spans(seed, n, D, length, c), (seed, n, D, length, c)
        for f0, f in got[0]:
            assert 0 <= f <= min(c["freq_width"], D) and 0 <= f0 and f0 + f <= D
        for t0, t in got[1]:
            assert 0 <= t <= min(c["time_width"], int(c["time_ratio"] * length)) and 0 <= t0 and t0 + t <= length


def test_widths_are_uniform():
    """Seed 7, D = 80, len = 800, the table's config, counters 0..4095: 8192 draws of each kind.  Every frequency width 0..15 is expected
    512 times, every time width 0..40 close to 200 times (8192 / 41); the windows are 5 sigma of the binomial."""
    c = SM.cfg(seed=7)
    fw, tw = np.zeros(16, int), np.zeros(41, int)
    for n in range(4096):
        fs, ts = SM.spans(7, n, 80, 800, c)
        for _, f in fs:
            fw[f] += 1
        for _, t in ts:
            tw[t] += 1
    print("frequency widths", fw.min(), "..", fw.max(), " time widths", tw.min(), "..", tw.max())
    assert fw.sum() == 8192 and tw.sum() == 8192
    assert (np.abs(fw - 512) <= 110).all(), fw
    assert (np.abs(tw - 200) <= 70).all(), tw


# ------------------------------------------------------------------ 2. the config
def test_checked_spec_augment():
    from ast_amd.spec_augment import checked_spec_augment as chk
    assert chk(None) is None and chk({}) is None
    d = chk({"fill": "mean"})
    assert d == {"freq_masks": 2, "freq_width": 15, "time_masks": 2, "time_width": 40, "time_ratio": 0.2, "fill": "mean", "seed": 2024}
    assert chk({"freq_masks": 0, "time_masks": 0})["freq_masks"] == 0
    assert chk({"time_ratio": 1})["time_ratio"] == 1.0 and chk({"freq_masks": 8, "time_masks": 8, "seed": 2**64 - 1})["seed"] == 2**64 - 1
    bad = [("freq_masks", -1), ("freq_masks", 9), ("freq_masks", 1.5), ("freq_masks", True), ("time_masks", -1), ("time_masks", 9),
           ("time_masks", "2"), ("freq_width", -1), ("freq_width", 2**31), ("time_width", -1), ("time_width", None), ("time_ratio", -0.1),
           ("time_ratio", 1.5), ("time_ratio", float("nan")), ("time_ratio", float("inf")), ("time_ratio", "0.2"), ("time_ratio", True),
           ("fill", "median"), ("fill", 0), ("seed", -1), ("seed", 2**64), ("seed", 1.0)]
    for key, value in bad:
        with pytest.raises(ValueError, match="extras.spec_augment.*" + key):
            chk({key: value})
    with pytest.raises(ValueError, match="freq_mask"):
        chk({"freq_mask": 2})                        # a misspelt key is not silently a default
    with pytest.raises(ValueError, match="train.aug"):
        chk([2, 15], what="train.aug")


# ------------------------------------------------------------------ 3. the CPU loader
def _data(n_train=37, zero_input=0.0):
    return {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": n_train, "syn_dev": 5},
            "frames": [20, 400], "targets": [1, 30], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
            "zero_input": zero_input, "train_scale": 1, "dec_key": "bpe_w"}


def _epochs(tmp_path, spec, n_epochs, rank=0, world=1, n_train=37, dev_between=True, start=0):
    from ast_amd.dataloader import SyntheticDataLoader
    from ast_amd.spec_augment import checked_spec_augment
    dl = SyntheticDataLoader(_data(n_train), str(tmp_path), -1)
    dl.rank, dl.world = rank, world
    dl.spec_augment, dl.spec_counter = checked_spec_augment(spec), start
    random.seed("seed-ast-20h")
    out, dev = [], []
    for _ in range(n_epochs):
        out.append([(b["utts"], b["X"].numpy().copy(), b["y"].numpy().copy()) for b in dl.get_batch(8, "syn_train", train=True, labels=True)])
        if dev_between:
            dev.append([(b["utts"], b["X"].numpy().copy()) for b in dl.get_batch(8, "syn_dev", train=False, labels=False)])
            dev.append([(b["utts"], b["X"].numpy().copy()) for b in dl.get_batch(8, "syn_train", train=False, labels=False)])
    return dl, out, dev


def _lens(dl, utts, set_key="syn_train"):
    return [min(int(dl.info[set_key][u]["sp"]), 400) for u in utts]


@pytest.mark.parametrize("fill", ["zero", "mean"])
def test_cpu_loader_masks_training_batches_only(tmp_path, fill):
    spec = SM.cfg(fill=fill, time_ratio=0.3)
    dl, got, dev = _epochs(tmp_path, spec, 2)
    _, plain, dev_plain = _epochs(tmp_path, None, 2)
    assert dl.spec_counter == 2 * 37
    base, n_masked = 0, 0
    for e in range(2):
        assert len(got[e]) == len(plain[e])
        for (utts, X, y), (utts0, X0, y0) in zip(got[e], plain[e]):
            assert utts == utts0 and X.shape == X0.shape and (y == y0).all()
            lens = _lens(dl, utts)
            want, mask = SM.masked(X0, lens, spec["seed"], base, 1, spec)
            base += len(utts)
            n_masked += int(mask.sum())
            for b, n in enumerate(lens):
                assert (bits(X[b, n:]) == 0).all()                                  # the padding is +0.0, as before
            assert (bits(X)[~mask] == bits(X0)[~mask]).all()
            if fill == "zero":
                assert (bits(X) == bits(want)).all()
            else:
                bound = SM.mean_bound(X0, lens)[:, None, :]
                assert (np.abs(X - want) <= bound + 0 * want)[mask].all()
    assert n_masked > 0
    # evaluation batches -- of the dev set and of the train set -- are never masked, and move no counter
    assert len(dev) == len(dev_plain) == 4
    for a, b in zip(dev, dev_plain):
        assert len(a) == len(b)
        for (u1, x1), (u0, x0) in zip(a, b):
            assert u1 == u0 and (bits(x1) == bits(x0)).all()


def test_counters_under_data_parallelism(tmp_path):
    """World 2: row b of rank r is presented as number base + 2 b + r, its position in the batch's unsharded list, and base advances by
    the cut whole-batch size on every rank.  The first batch of a world-1 loader on the same seeded plan shows the same utterances at
    the same positions: they carry the same masks."""
    spec = SM.cfg(time_ratio=0.3)
    shards, plains = [], []
    for r in range(2):
        dl, got, _ = _epochs(tmp_path, spec, 2, rank=r, world=2, n_train=64, dev_between=(r == 0))
        _, plain, _ = _epochs(tmp_path, None, 2, rank=r, world=2, n_train=64, dev_between=False)
        base = 0
        for e in range(2):
            assert len(got[e]) == len(plain[e])
            for (utts, X, _), (utts0, X0, _) in zip(got[e], plain[e]):
                assert utts == utts0
                want, mask = SM.masked(X0, _lens(dl, utts), spec["seed"], base + r, 2, spec)
                assert (bits(X) == bits(want)).all()
                base += 2 * len(utts)
        assert dl.spec_counter == base and 2 * (64 - 4) <= base <= 2 * 64
        shards.append(got)
    assert [len(u) for u, _, _ in shards[0][0]] == [len(u) for u, _, _ in shards[1][0]]
    # One process walks the same plan uncut: its batch k is the world-2 batch j(k) plus at most one utterance that world 2 leaves out.
    # Started so that the first batch both plans hold begins at the same position, that batch shows the same utterances at the same
    # positions, and therefore the same masks.
    _, plan1, _ = _epochs(tmp_path, None, 1, n_train=64, dev_between=False)
    k = next(i for i, (u, _, _) in enumerate(plan1[0]) if len(u) >= 2)
    assert plan1[0][k][0][0] == shards[0][0][0][0][0]                     # the first batch of the cut plan
    dl1, whole, _ = _epochs(tmp_path, spec, 1, n_train=64, dev_between=False, start=-sum(len(u) for u, _, _ in plan1[0][:k]) % 2**64)
    utts, X, _ = whole[0][k]
    seen = 0
    for g, u in enumerate(utts[:2 * len(shards[0][0][0][0])]):
        r, b = g % 2, g // 2
        assert shards[r][0][0][0][b] == u
        n = _lens(dl1, [u])[0]
        assert (bits(X[g, :n]) == bits(shards[r][0][0][1][b, :n])).all()
        seen += int((X[g, :n] == 0).sum())
    assert seen > 0


def test_apply_host_leaves_its_input_alone():
    from ast_amd import spec_augment as SA
    x = np.random.default_rng(0).standard_normal((50, 13)).astype(np.float32) + 3
    keep = x.copy()
    for fill in ("zero", "mean"):
        c = SA.checked_spec_augment(SM.cfg(fill=fill, freq_width=27, time_ratio=0.5))
        y = SA.apply_host(x, 5, c)
        want, mask = SM.masked(x[None], [50], c["seed"], 5, 1, c)
        assert (x == keep).all() and mask.any() and y.dtype == np.float32
        assert (bits(y)[~mask[0]] == bits(x)[~mask[0]]).all()
        assert np.allclose(y, want[0], rtol=0, atol=1e-6)
    assert SA.apply_host(np.zeros((0, 13), np.float32), 0, c).shape == (0, 13)
