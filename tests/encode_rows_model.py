"""Host models of the encoder with per-row source lengths (include/astk.h astk_conv_bn_relu_fwd_rows / astk_lstm_stack_fwd_rows;
DESIGN.md section 24), in NumPy and through the float64 oracle's own primitives (oracle/minichainer.py, oracle/ast_ref.py RefModel --
imported, not edited).  Three things make a zero-padded batch equal to every utterance alone:
  1. every CNN layer's activation of row b is zero from the row's own output length T_i(b) on;
  2. the reverse direction of row b reads frames (n - i) % n, n = row_len[b], at loop step i < n (quirk Q1 per row), and any in-range
     frame at a step i >= n, which no step < n can see;
  3. enc_states[b, p] holds the forward half of step p and the reverse half of step n - 1 - p for p < n and zeros behind, and the final
     states are those behind step n - 1.
tests/test_encode_rows_host.py checks the models against each other and the claim itself; tests/test_gpu_encode_rows.py uses the tables."""
import numpy as np

# the frame counts of the issue: T'' = 25, 24, 24, 16, 9, 9, 3, 3, 1, 1 on the shipped stack
FRAMES = (97, 96, 95, 61, 34, 33, 10, 9, 2, 1)
SHIPPED = [(16, 9, 13, 2, 13, 4), (16, 9, 1, 2, 1, 4)]      # (C, kt, kf, st, sf, pt) per layer, as range_cases.cnn_geometry_cfg takes them


def out_lens(layers, n):
    """[T_0, .., T''] of an utterance of n frames: floor((t + 2 pt - kt) / st) + 1 per layer, 0 from the first layer on whose padded
    input is shorter than its kernel (what the library refuses)."""
    out, t = [], int(n)
    for _, kt, _, st, _, pt in layers:
        t = 0 if (t < 1 or t + 2 * pt < kt) else (t + 2 * pt - kt) // st + 1
        out.append(t)
    return out


def out_lens_by_counting(layers, n):
    """The same by counting window positions: output step t exists when its window [t st - pt, t st - pt + kt) ends inside the padded
    input, i.e. t st + kt <= n + 2 pt."""
    out, t = [], int(n)
    for _, kt, _, st, _, pt in layers:
        t = sum(1 for k in range(t + 2 * pt + 1) if k * st + kt <= t + 2 * pt) if t >= 1 else 0
        out.append(t)
    return out


def perm_rows_table(T, B, lens):
    """k_perm_rows_len: rows[i * B + b] = frame * B + b of the row of x (T, B, in) that loop step i of the reverse direction reads for
    batch row b: frame (n - i) % n for i < n = lens[b], frame i behind."""
    rows = np.zeros(T * B, dtype=np.int64)
    for i in range(T):
        for b in range(B):
            n = int(lens[b])
            rows[i * B + b] = ((n - i) % n if i < n else i) * B + b
    return rows


def place_enc(h_fwd, h_rev, lens):
    """k_rows_place_enc: h_fwd / h_rev (T, B, h) in loop-step order -> enc_states (B, T, 2h)."""
    T, B, h = h_fwd.shape
    enc = np.zeros((B, T, 2 * h), dtype=h_fwd.dtype)
    for b in range(B):
        n = int(lens[b])
        enc[b, :n, :h] = h_fwd[:n, b]
        enc[b, :n, h:] = h_rev[:n, b][::-1]      # step i sits at position n - 1 - i: the batch's flip shifted by T - n
    return enc


def final_states(per_step, lens):
    """k_rows_final_states: per_step (T, B, h) of one cell -> (B, h), row b at loop step lens[b] - 1."""
    return np.stack([per_step[int(n) - 1, b] for b, n in enumerate(lens)], 0)


# ------------------------------------------------------------------ the float64 claim, through the oracle's primitives
def ref_model(cfg, D, V=11, seed=0):
    """A float64 RefModel in eval mode with non-trivial BatchNorm running statistics and affine (so that relu(shift) is not 0)."""
    from oracle import ast_ref as R
    P = R.init_params(cfg, D, V, seed=seed, dtype=np.float64)
    rng = np.random.default_rng(seed + 7)
    for i in range(len(cfg["cnn_config"]["cnn_layers"])):
        C = P[f"CNN_{i}_bn/gamma"].shape
        P[f"CNN_{i}_bn/gamma"] = 1 + 0.3 * rng.standard_normal(C)
        P[f"CNN_{i}_bn/beta"] = 0.5 + 0.2 * rng.standard_normal(C)
        P[f"CNN_{i}_bn/avg_mean"] = 0.1 * rng.standard_normal(C)
        P[f"CNN_{i}_bn/avg_var"] = 0.5 + rng.random(C)
    o = R.RefModel(cfg, P, V)
    o.train = False
    return o


def encode_alone(o, X):
    """One utterance X (T, D) through the oracle as it stands: enc (T'', H), c and h per encoder layer (H,) as init_decoder_state
    concatenates them."""
    o.encode(X[None])
    enc = np.asarray(o.enc_states.data)[0]
    c = [np.concatenate([np.asarray(e.c.data)[0], np.asarray(r.c.data)[0]]) for e, r in zip(o.enc, o.rev)]
    h = [np.concatenate([np.asarray(e.h.data)[0], np.asarray(r.h.data)[0]]) for e, r in zip(o.enc, o.rev)]
    return enc, c, h


def encode_batch(o, Xs, layers, cnn_masks=True, per_row=True):
    """The utterances Xs ((T_u, D) each) as ONE zero-padded batch through the oracle's primitives with the three devices above.
    cnn_masks = False: the CNN as the reference runs a padded batch; per_row = False: the batch's own permutation, flip and last step.
    -> enc (B, T''max, H), c, h per encoder layer (B, H), lens2."""
    from oracle import minichainer as F
    lens = [len(X) for X in Xs]
    B, T, D = len(Xs), max(lens), Xs[0].shape[1]
    Xp = np.zeros((B, T, D))
    for b, X in enumerate(Xs):
        Xp[b, :len(X)] = X
    h = F.swapaxes(F.expand_dims(F.as_variable(Xp), 2), 1, 2)               # RefModel.forward_cnn, with the mask behind every ReLU
    per_layer = [out_lens(layers, n) for n in lens]
    for i, l in enumerate(o.cnn_layers):
        h = F.relu(o.bn[f"CNN_{i}_bn"](F.convolution_2d(h, o.p[f"CNN_{i}/W"], tuple(l["stride"]), tuple(l["pad"]), None), train=False))
        if cnn_masks:
            keep = np.zeros(h.shape)
            for b in range(B):
                keep[b, :, :per_layer[b][i]] = 1.0
            h = F.mul(h, F.as_variable(keep))
    h = F.swapaxes(h, 1, 2)
    x = np.asarray(F.rollaxis(F.reshape(h, h.shape[:2] + (-1,)), 1).data)      # (T'', B, C F')
    T2 = x.shape[0]
    lens2 = [p[-1] for p in per_layer] if per_row else [T2] * B
    table = perm_rows_table(T2, B, lens2).reshape(T2, B) // B               # frame per (step, row)
    o.reset_rnn_state()
    steps = {"f": [], "r": []}
    for i in range(T2):
        o.feed_rnn(F.as_variable(x[i]), o.enc, "enc", i)
        o.feed_rnn(F.as_variable(x[table[i], np.arange(B)]), o.rev, "rev", i)
        for k, links in (("f", o.enc), ("r", o.rev)):
            steps[k].append([(np.asarray(l.c.data).copy(), np.asarray(l.h.data).copy()) for l in links])
    top = len(o.enc) - 1
    enc = place_enc(np.stack([s[top][1] for s in steps["f"]]), np.stack([s[top][1] for s in steps["r"]]), lens2)
    c, hh = [], []
    for k in range(len(o.enc)):
        c.append(np.concatenate([final_states(np.stack([s[k][0] for s in steps[d]]), lens2) for d in "fr"], 1))
        hh.append(np.concatenate([final_states(np.stack([s[k][1] for s in steps[d]]), lens2) for d in "fr"], 1))
    return enc, c, hh, lens2
