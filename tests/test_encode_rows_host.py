"""Host-side tests of the encoder with per-row source lengths (no GPU): the NumPy models of tests/encode_rows_model.py against each
other and against ast_amd.seq2seq, the exactness claim in float64 through the oracle's primitives, the exported symbols, the batch
plan of encode_rows(batch_encode=True) on a stub model, and the refusals that happen before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import encode_rows_model as M
import range_cases as RC
from conftest import tiny_cfg

STACKS = [(c[0], c[4]) for c in RC.CNN_GEOMETRY_CASES] + [("shipped", M.SHIPPED)]


# ------------------------------------------------------------------ the index table, the shift, the lengths
@pytest.mark.parametrize("lens", [[24, 23, 17, 16, 15, 2, 1], [1], [5, 5, 5], [1, 2, 3, 40]])
def test_index_table_is_the_lone_permutation_per_row(lens):
    T, B = max(lens), len(lens)
    rows = M.perm_rows_table(T, B, lens)
    assert rows.shape == (T * B,) and rows.min() >= 0 and rows.max() < T * B, "a step reads outside x"
    frame, row = rows.reshape(T, B) // B, rows.reshape(T, B) % B
    assert (row == np.arange(B)[None, :]).all(), "a row reads another row's frames"
    for b, n in enumerate(lens):
        lone = M.perm_rows_table(n, 1, [n])              # the utterance alone: (n - i) % n = 0, n-1, .., 1
        assert lone.tolist() == [(n - i) % n for i in range(n)] == ([0] + list(range(n - 1, 0, -1)))
        assert frame[:n, b].tolist() == lone.tolist()
        assert sorted(frame[:n, b].tolist()) == list(range(n)), "steps < n must read the row's own frames, each once"
    # all lengths equal T: the batch-wide table of k_perm_rows, rows[i B + b] = ((T - i) % T) B + b
    full = M.perm_rows_table(T, B, [T] * B)
    assert full.tolist() == [((T - i // B) % T) * B + i % B for i in range(T * B)]


def test_output_shift_and_final_states():
    rng = np.random.default_rng(0)
    T, B, h = 9, 4, 3
    lens = [9, 4, 1, 7]
    hf, hr = rng.standard_normal((T, B, h)), rng.standard_normal((T, B, h))
    enc = M.place_enc(hf, hr, lens)
    batch = np.concatenate([hf, hr[::-1]], 2).swapaxes(0, 1)         # what the batch's own flip gives: step i at position T - 1 - i
    for b, n in enumerate(lens):
        assert (enc[b, n:] == 0).all()
        assert (enc[b, :n, :h] == batch[b, :n, :h]).all()
        assert (enc[b, :n, h:] == batch[b, T - n:, h:]).all(), "the reverse half is the batch's, shifted by T - n"
        assert (enc[b, 0, h:] == hr[n - 1, b]).all() and (enc[b, n - 1, h:] == hr[0, b]).all()
    fin = M.final_states(hf, lens)
    assert all((fin[b] == hf[n - 1, b]).all() for b, n in enumerate(lens))
    assert (M.place_enc(hf, hr, [T] * B) == batch).all()


@pytest.mark.parametrize("cid,layers", STACKS, ids=[s[0] for s in STACKS])
def test_per_layer_lengths_follow_the_out_dims_arithmetic(cid, layers):
    from ast_amd.seq2seq import cnn_out_lens
    cfg_layers = RC.cnn_geometry_cfg(layers)["cnn_config"]["cnn_layers"]
    for n in list(range(1, 140)) + [333, 1169]:
        want = M.out_lens_by_counting(layers, n)
        assert M.out_lens(layers, n) == want, (n, M.out_lens(layers, n), want)
        if min(want) >= 1:
            assert cnn_out_lens(cfg_layers, n) == want
        else:
            with pytest.raises(ValueError, match="too short"):
                cnn_out_lens(cfg_layers, n)
    if cid == "shipped":
        assert [M.out_lens(layers, n)[-1] for n in M.FRAMES] == [25, 24, 24, 16, 9, 9, 3, 3, 1, 1]


# ------------------------------------------------------------------ the claim, in float64
def _claim_case():
    cfg = RC.cnn_geometry_cfg(M.SHIPPED)
    cfg["rnn_config"].update(enc_layers=2, dec_layers=2, hidden_units=12)
    D = 80
    o = M.ref_model(cfg, D)
    rng = np.random.default_rng(5)
    Xs = [rng.standard_normal((n, D)) for n in M.FRAMES]
    return o, Xs


def _worst(o, Xs, got):
    enc, c, h, lens2 = got
    worst = beyond = 0.0
    for b, X in enumerate(Xs):
        e1, c1, h1 = M.encode_alone(o, X)
        n = e1.shape[0]
        worst = max(worst, float(np.abs(enc[b, :n] - e1).max()))
        worst = max(worst, max(float(np.abs(c[k][b] - c1[k]).max()) for k in range(len(c1))),
                    max(float(np.abs(h[k][b] - h1[k]).max()) for k in range(len(h1))))
        beyond = max(beyond, float(np.abs(enc[b, n:]).max()) if n < enc.shape[1] else 0.0)
    return worst, beyond


def test_masked_padded_batch_equals_every_utterance_alone_in_float64():
    o, Xs = _claim_case()
    got = M.encode_batch(o, Xs, M.SHIPPED)
    assert got[3] == [25, 24, 24, 16, 9, 9, 3, 3, 1, 1]
    worst, beyond = _worst(o, Xs, got)
    print(f"\nmasked batch against alone: enc / c / h max abs diff {worst:.3e}, beyond the lengths {beyond!r}")
    assert worst <= 1e-12 and beyond == 0.0
    # without the CNN masks, and without the per-row tables, the same run is NOT the utterances alone: the test tests the masks
    w_cnn, _ = _worst(o, Xs, M.encode_batch(o, Xs, M.SHIPPED, cnn_masks=False))
    w_row, _ = _worst(o, Xs, M.encode_batch(o, Xs, M.SHIPPED, per_row=False))
    print(f"without the CNN masks {w_cnn:.3e}, without the per-row tables {w_row:.3e}")
    assert w_cnn > 1e-3 and w_row > 1e-3


# ------------------------------------------------------------------ the library's boundary
def test_library_exports_the_three_new_symbols():
    from ast_amd import _lib
    lib = _lib.load()
    for name in ("astk_conv_bn_relu_fwd_rows", "astk_lstm_stack_rows_workspace_bytes", "astk_lstm_stack_fwd_rows"):
        assert name in _lib.SIGNATURES and isinstance(getattr(lib, name), C._CFuncPtr)


def test_entry_points_refuse_bad_descriptors_before_any_launch():
    """What is refused from the descriptor alone never reaches the device (so it runs here): a wrong struct_size, pooled layers, more than
    32 rows.  The pointers are never read."""
    from ast_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(4096)
    cfg = RC.cnn_geometry_cfg(M.SHIPPED)

    def cd(B=4, T=64, pool=None, size=None):
        d = _lib.CnnDesc()
        cc = cfg["cnn_config"]["cnn_layers"]
        d.B, d.T, d.D, d.n_layers = B, T, 80, len(cc)
        for i, l in enumerate(cc):
            d.C[i], (d.kt[i], d.kf[i]), (d.st[i], d.sf[i]), d.pt[i] = l["out_channels"], l["ksize"], l["stride"], l["pad"][0]
        d.bn_eps, d.bn_decay = 2e-5, 0.9
        for i, (wt, wf) in enumerate(pool or []):
            d.pool_t[i], d.pool_f[i] = wt, wf
        if size is not None:
            d.struct_size = size
        return d
    cp = (_lib.CnnLayerParams * 2)()
    for d, cause in ((cd(size=8), "struct_size"), (cd(pool=[[2, 1], [1, 1]]), "pooled layers"), (cd(B=33), "at most 32 rows")):
        rc = lib.astk_conv_bn_relu_fwd_rows(C.byref(d), cp, fake, fake, fake, None, fake, 1 << 30, None)
        assert rc != 0 and cause in lib.astk_last_error().decode(), lib.astk_last_error().decode()
    lp = (_lib.LstmParams * 4)()
    good = _lib.LstmStackDesc(8, 4, 16, 64, 2, 2)
    assert lib.astk_lstm_stack_rows_workspace_bytes(C.byref(good)) == lib.astk_lstm_stack_workspace_bytes(C.byref(good)) > 0
    wide, bad = _lib.LstmStackDesc(8, 33, 16, 64, 2, 2), _lib.LstmStackDesc(8, 4, 16, 64, 2, 2)
    bad.struct_size = 8
    assert lib.astk_lstm_stack_rows_workspace_bytes(C.byref(wide)) == 0 and lib.astk_lstm_stack_rows_workspace_bytes(C.byref(bad)) == 0
    for d, cause in ((bad, "struct_size"), (wide, "1..32 rows")):
        rc = lib.astk_lstm_stack_fwd_rows(C.byref(d), lp, fake, fake, fake, fake, fake, fake, 1 << 30, None)
        assert rc != 0 and cause in lib.astk_last_error().decode(), lib.astk_last_error().decode()


# ------------------------------------------------------------------ the batch plan of encode_rows
def test_plan_encode_batches():
    from ast_amd.seq2seq import plan_encode_batches
    lens = [5, 90, 7, 90, 33, 1] + [10] * 60
    plan = plan_encode_batches(lens)
    assert [len(b) for b in plan] == [32, 32, 2] and sorted(u for b in plan for u in b) == list(range(66))
    flat = [lens[u] for b in plan for u in b]
    assert flat == sorted(lens, reverse=True) and plan[0][:3] == [1, 3, 4], "longest first, ties in index order"
    assert plan_encode_batches([3, 4, 5], max_rows=2) == [[2, 1], [0]] and plan_encode_batches([]) == []
    with pytest.raises(ValueError, match="max_rows"):
        plan_encode_batches([1], max_rows=0)


def _stub(calls, served=True, cfg=None):
    from ast_amd.seq2seq import SpeechEncoderDecoder

    class Stub(SpeechEncoderDecoder):
        """The two device-facing pieces replaced: an utterance's 'encoding' is its frame count and its first value."""

        def _plan_encode_batch(self, Xs):
            return ("plan", len(Xs)) if served else None

        def _encode_batch(self, Xs, plan):
            assert plan == ("plan", len(Xs))
            calls.append([int(X.shape[0]) for X in Xs])
            encs = [torch.full((int(X.shape[0]) // 4 + 1, self.H), float(X[0, 0])) for X in Xs]
            st = [torch.full((2, self.H), float(X[0, 0])) for X in Xs]
            return encs, st, [s + 0.5 for s in st], [{"c": [float(X[0, 0])], "h": []} for X in Xs]

        def _encode_alone(self, Xs, seeds=None):
            calls.append("alone")
            return [torch.zeros(2, self.H)] * len(Xs), [torch.zeros(2, self.H)] * len(Xs), [torch.zeros(2, self.H)] * len(Xs)
    return Stub(-1, cfg or tiny_cfg())


def test_encode_rows_batches_the_distinct_utterances_and_gathers_by_rows_of():
    calls = []
    m = _stub(calls)
    assert m.batch_encode is False and m.last_encode_path is None
    Xs = [torch.full((4 * (u + 1), 3), float(u)) for u in range(40)]
    rows_of = [39, 39, 0, 7, 7, 7, 12]
    rb = m.encode_rows(Xs, rows_of, batch_encode=True)
    assert m.last_encode_path == "batched" and calls == [[160, 52, 32, 4]], calls       # the four distinct utterances, once each, longest first
    assert rb.lens.tolist() == [41, 41, 2, 9, 9, 9, 14] and rb.enc.shape == (7, 41, m.H)
    for b, u in enumerate(rows_of):
        n = 4 * (u + 1) // 4 + 1
        assert (rb.enc[b, :n] == u).all() and (rb.enc[b, n:] == 0).all()
        assert (rb.c0[:, b] == u).all() and (rb.h0[:, b] == u + 0.5).all()
    # more than 32 distinct utterances: two calls of at most 32 (32 rows per RowBatch, so through the shared helper)
    calls[:] = []
    seeds = []
    encs, c0s, h0s = m._encode_utts(Xs, seeds, batch_encode=True)
    assert [len(c) for c in calls] == [32, 8] and calls[0] == sorted(calls[0], reverse=True) and min(calls[0]) >= max(calls[1])
    assert [float(e[0, 0]) for e in encs] == list(range(40)) and [s["c"][0] for s in seeds] == list(range(40))
    # the default, and the model attribute
    calls[:] = []
    m.encode_rows(Xs[:3])
    assert calls == ["alone"] and m.last_encode_path == "alone"
    m.batch_encode = True
    m.encode_rows(Xs[:3])
    assert calls == ["alone", [12, 8, 4]] and m.last_encode_path == "batched"
    m.encode_rows(Xs[:3], batch_encode=False)
    assert calls[-1] == "alone" and m.last_encode_path == "alone"


def test_encode_rows_falls_back_silently_and_refuses_bad_arguments():
    calls = []
    m = _stub(calls, served=False)                       # a workspace query of 0
    m.encode_rows([torch.zeros(8, 3)], batch_encode=True)
    assert calls == ["alone"] and m.last_encode_path == "alone"
    cfg = tiny_cfg()
    cfg["cnn_config"]["cnn_pool"] = [[2, 1], [1, 1]]
    calls[:] = []
    m = _stub(calls, cfg=cfg)
    m.encode_rows([torch.zeros(8, 3)], batch_encode=True)
    assert calls == ["alone"] and m.last_encode_path == "alone"
    calls[:] = []
    m = _stub(calls)
    m.enc_variant = object()                             # rnn_config.ln / linear_proj
    m.encode_rows([torch.zeros(8, 3)], batch_encode=True)
    assert calls == ["alone"] and m.last_encode_path == "alone"
    m = _stub(calls)
    with pytest.raises(ValueError, match="no frames"):
        m.encode_rows([torch.zeros(8, 3), torch.zeros(0, 3)], batch_encode=True)
    with pytest.raises(ValueError, match="1..32 rows"):
        m.encode_rows([torch.zeros(8, 3)], rows_of=[0] * 33, batch_encode=True)
    with pytest.raises(ValueError, match="outside 0..0"):
        m.encode_rows([torch.zeros(8, 3)], rows_of=[1], batch_encode=True)


def test_command_lines_take_the_flag():
    import sample
    a = sample.build_parser().parse_args("-m cfg -s dev -n 6 -b 8 --batch-encode".split())
    assert a.batch_encode is True and sample.build_parser().parse_args("-m cfg -s dev -n 6".split()).batch_encode is False
