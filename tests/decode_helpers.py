"""What the GPU tests of the on-device decode modes share (test_gpu_greedy.py, test_gpu_greedy_scored.py, test_gpu_forced.py,
test_gpu_sample.py): the model shapes, the model set-up, targets, the float64 LSE, the argmax guard and the tolerance of
log-probabilities.  Helpers that differ between the modes (the per-step loops, the oracles) stay with their tests."""
import copy

import numpy as np

from conftest import tiny_cfg

GO, EOS = 1, 2
OUT_SCALE = 8.0
ES_EN = dict(enc_layers=3, dec_layers=3, H=512, E=128, A=512, c0=128, c1=512, V=1098)     # es_en_20h
CFG1 = dict(enc_layers=3, dec_layers=1, H=512, E=128, A=512, c0=128, c1=512, V=1098)      # BASELINE configs[1] (bench.py cfg1)
WIDE = dict(enc_layers=1, dec_layers=1, H=1024, E=16, A=1024, c0=8, c1=16, V=57)         # the wide decoder (configs[4]'s H = A = 1024)
MID = dict(enc_layers=2, dec_layers=2, H=64, E=16, A=64, c0=8, c1=16, V=57)

# The largest error of the PER-STEP loop (astk_decoder_step_infer logits in float32, LSE in float64 on the host: the arithmetic the
# project had before the scored mode) against the float64 oracle, over logp and nll at every guarded position of the full-size cases
# of test_gpu_greedy_scored.py (test_scored_matches_oracle_full_size prints it as e_loop): 3.26e-6 on configs[1], 3.68e-6 on es_en_20h,
# one MI355X.  The device loop gets twice that -- its logits are accumulated per tile in another order and its LSE is float32 -- or the
# project's bound for float32 log-probabilities against the oracle (tests/test_gpu_model.py:172), whichever is larger.  Sampled
# decoding scales the first term by max(1, 1 / temperature): logit errors scale with inv_temp.
E_LOOP = 3.7e-6


def tol(value, temperature=1.0):
    return np.maximum(2 * E_LOOP * max(1.0, 1.0 / temperature), 1e-4 * np.maximum(1.0, np.abs(value)))


def setup(shape, B, T, seed=0, eos_bias=0.0, D=80, **cfg_over):
    from oracle import ast_ref as R
    from ast_amd.seq2seq import SpeechEncoderDecoder
    cfg = tiny_cfg(**shape)
    for k, v in cfg_over.items():
        cfg["rnn_config"][k] = v
    V = shape["V"]
    P = R.init_params(cfg, D, V, seed=seed, dtype=np.float32)
    P["out/W"] = (P["out/W"] * OUT_SCALE).astype(np.float32)
    P["out/b"] = P["out/b"].copy()
    P["out/b"][EOS] += eos_bias
    X, _ = R.synth_batch(B, T, D, 3, V, seed=seed + 1, dtype=np.float32)
    c = copy.deepcopy(cfg)
    c["rnn_config"]["dec_vocab_size"] = V
    m = SpeechEncoderDecoder(0, c).materialize(D, values=P)
    return cfg, P, X, m


def targets(B, L, V, seed, go_first=False):
    """(B, L) int32 targets, a quarter of the positions PAD (weight 0); go_first: column 0 = GO."""
    rng = np.random.default_rng(seed)
    y = rng.integers(1, V, size=(B, L)).astype(np.int32)
    y[rng.random((B, L)) < 0.25] = 0
    if go_first:
        y[:, 0] = GO
    return y


def lse64(lg):
    mx = lg.max(axis=1, keepdims=True)
    return (mx + np.log(np.exp(lg - mx).sum(axis=1, keepdims=True)))[:, 0]


def guard(ref_tokens, gaps, thr):
    """(B, n) bool: positions before the row's first step whose top-2 gap is below thr."""
    B, n = ref_tokens.shape
    ok = np.zeros((B, n), dtype=bool)
    for b in range(B):
        low = np.nonzero(gaps[:, b] < thr)[0]
        ok[b, :int(low[0]) if len(low) else n] = True
    return ok


def max_err(name, got, ref, ok, temperature=1.0):
    """Prints and returns the largest error and the largest error / tolerance over the positions `ok`."""
    err = np.abs(got.astype(np.float64) - ref)[ok]
    rel = err / tol(ref[ok], temperature)
    print(f"  {name}: max abs err {err.max():.3e}, max err / tol {rel.max():.3f}, max |value| {np.abs(ref[ok]).max():.3f}, n {ok.sum()}")
    return float(err.max()), float(rel.max())
