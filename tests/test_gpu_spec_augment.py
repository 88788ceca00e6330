"""GPU tests of SpecAugment in the training loader (include/astk.h astk_spec_augment) against the independent
model of tests/spec_augment_model.py: the operator under both fills, bit for bit where the contract says so, the mean fill inside the
worst-case bound of a float32 sum, means taken from the data on entry, a row alone against the same row inside a padded batch, the
refusals, the device loader against an unmasked twin and against the CPU loader, and train.py."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import spec_augment_model as SM
from conftest import tiny_cfg

pytestmark = pytest.mark.gpu

SEED = 2024
SHAPES = [((3, 37, 13), [37, 1, 0]), ((4, 50, 80), [50, 23, 1, 0]), ((2, 800, 80), [800, 411])]
CONFIGS = {"table": SM.cfg(), "F>=D": SM.cfg(freq_width=200), "W>len": SM.cfg(time_width=5000, time_ratio=1.0),
           "cap0": SM.cfg(time_ratio=1e-4), "eight": SM.cfg(freq_masks=8, time_masks=8, freq_width=5, time_ratio=0.5),
           "freq_only": SM.cfg(time_masks=0), "time_only": SM.cfg(freq_masks=0, time_ratio=0.5)}
COUNTERS = [(2**32 - 1, 1), (5, 2)]
NAN_BITS, NEG0_BITS = 0x7FC00123, -0x80000000


@pytest.fixture(scope="module")
def lib():
    from ast_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def from_bits(b):
    return np.ascontiguousarray(b, dtype=np.int32).view(np.float32)


def batch(shape, lens, seed, ramp=False):
    """N(3, 1) in the true frames (plus a quadratic ramp from 0 to 10 over the utterance if asked), 7 + N(0, 1) in the padding: a mean over T frames, or
    one that reads the padding, misses the bound by orders of magnitude."""
    B, T, D = shape
    rng = np.random.default_rng(seed)
    X = (7.0 + rng.standard_normal(shape)).astype(np.float32)
    for b, n in enumerate(lens):
        X[b, :n] = (3.0 + rng.standard_normal((n, D)) + (10.0 * (np.arange(n)[:, None] / max(n, 1)) ** 2 if ramp else 0.0)).astype(np.float32)
    return X


def desc_of(c):
    from ast_amd import _lib
    return _lib.SpecAugmentDesc(c["freq_masks"], c["freq_width"], c["time_masks"], c["time_width"], c["time_ratio"], {"zero": 0, "mean": 1}[c["fill"]])


def run(lib, X, lens, c, counter0, stride, seed=SEED):
    Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    ld = torch.tensor(list(lens), dtype=torch.int32, device="cuda")
    d = desc_of(c)
    rc = lib.astk_spec_augment(C.c_void_p(Xd.data_ptr()), X.shape[0], X.shape[1], X.shape[2], C.c_void_p(ld.data_ptr()), C.byref(d), seed,
                               counter0, stride, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.astk_last_error().decode()
    torch.cuda.synchronize()
    return Xd.cpu().numpy()


def seeded(X, lens, mask, unmasked_nan):
    """X with a -0.0 in an unmasked true cell and a NaN and a -0.0 in the padding of every row that has such cells; unmasked_nan: a NaN in
    a second unmasked true cell as well (the zero fill reads nothing; under the mean fill a NaN would be its bin's mean)."""
    xb = bits(X).copy()
    B, T, D = X.shape
    for b, n in enumerate(lens):
        free = np.argwhere(~mask[b, :n])
        if len(free) >= 1:
            xb[b, free[0][0], free[0][1]] = NEG0_BITS
        if unmasked_nan and len(free) >= 2:
            xb[b, free[-1][0], free[-1][1]] = NAN_BITS
        if n < T:
            xb[b, n, 0] = NAN_BITS
            xb[b, T - 1, D - 1] = NEG0_BITS
    return from_bits(xb)


def check_mean(got, X, lens, want, mask):
    """The mean fill's result against the float64 model: everything outside the mask keeps its bits; the masked cells of a bin hold ONE
    value, within len 2^-24 mean|x| of the float64 mean.  Returns the largest share of the bound used."""
    assert (bits(got)[~mask] == bits(X)[~mask]).all()
    bound = SM.mean_bound(X, lens)
    share = 0.0
    for b in range(X.shape[0]):
        for d in range(X.shape[2]):
            cells = got[b, :, d][mask[b, :, d]]
            if cells.size:
                assert (bits(cells) == bits(cells[:1])).all(), (b, d)
                err = abs(float(cells[0]) - want[b, mask[b, :, d], d][0])
                assert err <= bound[b, d], (b, d, err, bound[b, d])
                share = max(share, err / bound[b, d] if bound[b, d] > 0 else 0.0)
    return share


# ------------------------------------------------------------------ 1. operator, zero fill
@pytest.mark.parametrize("shape,lens", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_zero_fill_bit_for_bit(lib, shape, lens):
    n_masked = 0
    for name, c in CONFIGS.items():
        for counter0, stride in COUNTERS:
            X = batch(shape, lens, 1)
            _, mask = SM.masked(X, lens, SEED, counter0, stride, c)
            X = seeded(X, lens, mask, unmasked_nan=True)
            want, mask = SM.masked(X, lens, SEED, counter0, stride, c)
            assert (want[mask] == 0).all()
            got = run(lib, X, lens, c, counter0, stride)
            assert (bits(got) == np.where(mask, 0, bits(X))).all(), (name, counter0)
            n_masked += int(mask.sum())
    assert n_masked > 0
    # a fully masked utterance is the definition, not an error: the first counter whose frequency draw is the whole width D
    c, D = CONFIGS["F>=D"], shape[2]
    n = next(n for n in range(10000) if any(f == D for _, f in SM.spans(SEED, n, D, lens[0], c)[0]))
    X = batch(shape, lens, 1)
    got = run(lib, X, lens, c, n, 1)
    _, mask = SM.masked(X, lens, SEED, n, 1, c)
    assert mask[0, :lens[0]].all() and (bits(got) == np.where(mask, 0, bits(X))).all() and (bits(got[0, :lens[0]]) == 0).all()


# ------------------------------------------------------------------ 2. operator, mean fill
@pytest.mark.parametrize("shape,lens", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_mean_fill_within_the_float32_bound(lib, shape, lens):
    worst = 0.0
    for name, c in CONFIGS.items():
        c = dict(c, fill="mean")
        for counter0, stride in COUNTERS:
            X = batch(shape, lens, 2)
            _, mask = SM.masked(X, lens, SEED, counter0, stride, c)
            X = seeded(X, lens, mask, unmasked_nan=False)
            want, mask = SM.masked(X, lens, SEED, counter0, stride, c)
            got = run(lib, X, lens, c, counter0, stride)
            worst = max(worst, check_mean(got, X, lens, want, mask))
            again = run(lib, X, lens, c, counter0, stride)
            assert (bits(again) == bits(got)).all(), (name, counter0)
    print("largest share of the bound used, shape", shape, ":", worst)


# ------------------------------------------------------------------ 3. means come from the data on entry
def test_means_are_taken_before_any_mask(lib):
    """Counter 0 of the table: frequency spans (56,10) (51,11) and time spans (680,34) (211,9) overlap.  With a ramp over the utterance a
    mean that already saw a filled time span lies far outside the bound around the entry mean."""
    c = SM.cfg(fill="mean")
    assert SM.spans(SEED, 0, 80, 800, c) == ([(56, 10), (51, 11)], [(680, 34), (211, 9)])
    X = batch((1, 800, 80), [800], 3, ramp=True)
    want, mask = SM.masked(X, [800], SEED, 0, 1, c)
    assert mask[0, 680:714, 51:66].all() and mask[0, :, 51:66].all() and not mask[0, 0, :51].any()
    entry, bound = X[0].astype(np.float64).mean(axis=0), SM.mean_bound(X, [800])[0]
    late = X[0].astype(np.float64)
    late[680:714], late[211:220] = entry, entry                          # what a mean taken behind the time masks would read
    assert (np.abs(late.mean(axis=0) - entry) > 100 * bound).all()
    got = run(lib, X, [800], c, 0, 1)
    check_mean(got, X, [800], want, mask)
    assert (np.abs(got[0, 700, :] - entry) <= bound).all() and (np.abs(got[0, 0, 51:66] - entry[51:66]) <= bound[51:66]).all()


# ------------------------------------------------------------------ 4. composition
@pytest.mark.parametrize("fill", ["zero", "mean"])
@pytest.mark.parametrize("D,n", [(13, 37), (80, 411)])
def test_a_row_alone_equals_the_row_in_a_batch(lib, fill, D, n):
    c = SM.cfg(fill=fill, time_ratio=0.5)
    T = n + 29
    lens = [T, 5, n, 1]
    X = batch((4, T, D), lens, 4)
    counter0, stride = 2**40 + 3, 7
    inside = run(lib, X, lens, c, counter0, stride)
    alone = run(lib, np.ascontiguousarray(X[2:3, :n]), [n], c, counter0 + 2 * stride, 1)
    assert (bits(inside[2, :n]) == bits(alone[0])).all()
    assert (bits(inside[2, n:]) == bits(X[2, n:])).all() and (bits(alone) != bits(X[2:3, :n])).any()


# ------------------------------------------------------------------ 5. refusals
def test_refusals_name_the_field_and_launch_nothing(lib):
    from ast_amd import _lib
    X = batch((2, 20, 13), [20, 9], 5)
    Xd = torch.from_numpy(X).cuda()
    ld = torch.tensor([20, 9], dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(x=True, lengths=True, d=True, B=2, T=20, D=13, **fields):
        desc = desc_of(SM.cfg())
        for k, v in fields.items():
            setattr(desc, k, v)
        return lib.astk_spec_augment(C.c_void_p(Xd.data_ptr()) if x else None, B, T, D, C.c_void_p(ld.data_ptr()) if lengths else None,
                                     C.byref(desc) if d else None, SEED, 0, 1, st)
    bad = [(dict(x=False), "X"), (dict(lengths=False), "lengths"), (dict(d=False), "descriptor"), (dict(struct_size=36), "struct_size"),
           (dict(struct_size=0), "struct_size"), (dict(n_freq=-1), "n_freq"), (dict(n_freq=9), "n_freq"), (dict(n_time=-1), "n_time"),
           (dict(n_time=9), "n_time"), (dict(freq_width=-1), "freq_width"), (dict(time_width=-1), "time_width"),
           (dict(time_ratio=-0.1), "time_ratio"), (dict(time_ratio=1.0000001), "time_ratio"), (dict(time_ratio=float("nan")), "time_ratio"),
           (dict(time_ratio=float("inf")), "time_ratio"), (dict(fill=2), "fill"), (dict(fill=-1), "fill"), (dict(B=0), "B"), (dict(T=0), "T"),
           (dict(D=0), "D"), (dict(D=1025), "D")]
    assert C.sizeof(_lib.SpecAugmentDesc) == 40
    for kw, field in bad:
        rc = call(**kw)
        msg = lib.astk_last_error().decode()
        assert rc != 0 and "spec_augment" in msg and field in msg, (kw, rc, msg)
    # no masks asked for: success, and nothing launched
    assert call(n_freq=0, n_time=0) == 0
    torch.cuda.synchronize()
    assert (bits(Xd.cpu().numpy()) == bits(X)).all()
    assert call() == 0                                                    # the same call with nothing wrong does mask
    torch.cuda.synchronize()
    assert (bits(Xd.cpu().numpy()) != bits(X)).any()


# ------------------------------------------------------------------ 6. the device loader
def _data(zero_input):
    return {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 45, "syn_dev": 5},
            "frames": [20, 400], "targets": [1, 30], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
            "zero_input": zero_input, "train_scale": 1, "dec_key": "bpe_w"}


def _epochs(tmp_path, gpuid, zero_input, spec, n_epochs=2):
    from ast_amd.dataloader import SyntheticDataLoader
    from ast_amd.spec_augment import checked_spec_augment
    dl = SyntheticDataLoader(_data(zero_input), str(tmp_path), gpuid)
    dl.zero_seed = 0xABCDEF
    dl.spec_augment = checked_spec_augment(spec)
    random.seed("seed-ast-20h")
    out = []
    for _ in range(n_epochs):
        for b in dl.get_batch(8, "syn_train", train=True, labels=True):
            assert set(b) == {"X", "y", "utts"}                           # `len` does not leave the loader
            out.append((b["utts"], b["X"].cpu().numpy().copy(), b["y"].cpu().numpy().copy()))
        dev = [b["X"].cpu().numpy().copy() for b in dl.get_batch(8, "syn_dev", train=False, labels=False)]
    return dl, out, dev


@pytest.mark.parametrize("fill", ["zero", "mean"])
def test_device_loader_masks_behind_frame_zeroing(tmp_path, fill):
    spec = SM.cfg(fill=fill, time_ratio=0.3)
    dl, got, dev = _epochs(tmp_path, 0, 0.1, spec)
    _, plain, dev_plain = _epochs(tmp_path, 0, 0.1, None)
    assert dl.spec_counter == 2 * 45 and len(got) == len(plain)
    base, zeroed, n_masked = 0, 0, 0
    for (utts, X, y), (utts0, X0, y0) in zip(got, plain):
        assert utts == utts0 and (y == y0).all()
        lens = [min(int(dl.info["syn_train"][u]["sp"]), 400) for u in utts]
        want, mask = SM.masked(X0, lens, SEED, base, 1, spec)
        base += len(utts)
        zeroed += int((X0 == 0).all(axis=2).sum() - sum(X0.shape[1] - n for n in lens))
        n_masked += int(mask.sum())
        if fill == "zero":
            assert (bits(X) == np.where(mask, 0, bits(X0))).all()
        else:
            check_mean(X, X0, lens, want, mask)
    assert zeroed > 0 and n_masked > 0                                  # frame zeroing did run in front of the masks
    assert all((bits(a) == bits(b)).all() for a, b in zip(dev, dev_plain)) and len(dev) == len(dev_plain) > 0


def test_device_loader_equals_cpu_loader_under_zero_fill(tmp_path):
    spec = SM.cfg(time_ratio=0.3)
    _, gpu, _ = _epochs(tmp_path, 0, 0.0, spec)
    _, cpu, _ = _epochs(tmp_path, -1, 0.0, spec)
    assert len(gpu) == len(cpu) > 0
    for (u1, x1, y1), (u0, x0, y0) in zip(gpu, cpu):
        assert u1 == u0 and (y1 == y0).all() and (bits(x1) == bits(x0)).all()
    assert any((x == 0).any() for _, x, _ in gpu)


# ------------------------------------------------------------------ 7. train.py
def test_train_py_reads_extras_spec_augment(tmp_path):
    """One epoch of `python train.py` on the synthetic set: with extras.spec_augment the loss is finite and another one than without the
    key; with no masks asked for ({"freq_masks": 0, "time_masks": 0}) the logged losses are those of the run without the key."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mcfg = tiny_cfg(enc_layers=2, dec_layers=1, H=32, E=16, A=32, c0=8, c1=16, V=31, drop=0.0)
    del mcfg["rnn_config"]["dec_vocab_size"]
    tcfg = {"seed": "seed-ast-20h", "gpuid": 0, "batch_size": 8, "train_set": "syn_train", "dev_set": "syn_dev", "iters_save": 2,
            "optimizer": {"type": 0, "lr": 2e-3, "l2": 1e-4, "grad_clip": 2, "grad_noise_eta": 0, "freeze": []},
            "extras": {"teach_ratio": 1.0, "random_out": 0, "speech_noise": 0},
            "data": {"dataloader": "synthetic", "vocab_size": 31, "feat_dim": 13, "n_utts": {"syn_train": 24, "syn_dev": 6},
                     "frames": [60, 300], "targets": [2, 9], "buckets_num": 4, "buckets_width": 80, "max_pred": 12,
                     "zero_input": 0.0, "train_scale": 1, "dec_key": "bpe_w"}}
    logs = {}
    for name, spec in (("masked", {"fill": "mean", "time_ratio": 0.3}), ("plain", None), ("none", {"freq_masks": 0, "time_masks": 0})):
        d = tmp_path / name
        os.makedirs(d)
        tcfg["extras"].pop("spec_augment", None)
        if spec is not None:
            tcfg["extras"]["spec_augment"] = spec
        json.dump(mcfg, open(d / "model_cfg.json", "w"))
        json.dump(tcfg, open(d / "train_cfg.json", "w"))
        r = subprocess.run([sys.executable, os.path.join(root, "train.py"), "-m", str(d), "-e", "1"], cwd=root, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert ("SpecAugment" in r.stdout) == (spec is not None)
        logs[name] = [l.split(",")[1] for l in open(d / "train.log").read().split("\n") if l.strip()]
    print(logs)
    assert len(logs["masked"]) == 1 and np.isfinite(float(logs["masked"][0]))
    assert logs["masked"] != logs["plain"]
    assert logs["none"] == logs["plain"]
