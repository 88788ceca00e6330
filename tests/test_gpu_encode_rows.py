"""Per-row source lengths in the encoder (include/astk.h astk_conv_bn_relu_fwd_rows / astk_lstm_stack_fwd_rows; SpeechEncoderDecoder
encode_rows(batch_encode=True)).

In every comparison the reference is THE SAME ROW ALONE on the entry point the project already tests: B = 1, T = the row's length,
train = 0 / no masks.  Bounds: the CNN output under tests/test_gpu_ops.py close() as tests/test_gpu_cnn_geometry.py's operator case applies
it to the forward output (rtol 2e-4 of the reference's scale); the LSTM outputs of BOTH the lone and the batched call against the float64
twin (oracle/ast_ref_torch.py encoder_torch) under the same close(), as test_lstm_stack; what lies beyond a row's length exactly 0; calls
with all lengths = T, or with row_len = NULL, the bits of the existing entry point.  The direct batched-against-alone differences are
printed, not asserted.  Every test prints its figures before it asserts."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import encode_rows_model as M
import range_cases as RC
from conftest import tiny_cfg
from decode_helpers import EOS, OUT_SCALE, targets, tol
from test_gpu_ops import GuardedWS, _cnn_desc, _concurrent_stream, close, dev, gemm_split, lib, ok, stream, vp  # noqa: F401  (the two fixtures)

pytestmark = pytest.mark.gpu


def _status_is_clear():
    from ast_amd import _lib
    mask = C.c_uint(7)
    return _lib.load().astk_persist_status(C.byref(mask), 0) == 0 and mask.value == 0


@pytest.fixture(autouse=True)
def _status_word_stays_clear():
    yield
    torch.cuda.synchronize()
    assert _status_is_clear()


def _i32(a):
    return torch.tensor(list(a), dtype=torch.int32, device="cuda")


def _knobs(lib, knobs):
    class Scope:
        def __enter__(self):
            self.prev = {}
            for k, v in knobs.items():
                self.prev[k] = C.c_double()
                assert lib.astk_get_tuning(k.encode(), C.byref(self.prev[k])) == 0 and lib.astk_set_tuning(k.encode(), float(v)) == 0, k

        def __exit__(self, *exc):
            for k, v in self.prev.items():
                lib.astk_set_tuning(k.encode(), v.value)
            return False
    return Scope()


# ================================================================== CNN operator
GEO = {c[0]: c[4] for c in RC.CNN_GEOMETRY_CASES}
# (id, layers, D, frame counts): the shipped geometry with 16 / 16 channels (the direct layer-0 kernel under bf16x3) on the issue's
# frame counts (T'' = 25, 24, 24, 16, 9, 9, 3, 3, 1, 1); an im2col layer 0 under every scheme (kt 11, kf 16, stride 3: rows of 7+ frames
# only, a shorter one is refused); three layers (a middle layer consumes and produces masked, padded rows); layer-0 stride 1 without any
# time padding (layer 1: kt = st = 13, so rows need 16 frames)
CNN_STACKS = [
    ("shipped-c16", M.SHIPPED, 80, M.FRAMES),
    ("kt11-st3-kf16", GEO["kt11-st3-kf16"], 80, (97, 96, 95, 61, 34, 33, 10, 9, 8, 7)),
    ("three-layers", GEO["three-layers"], 80, M.FRAMES),
    ("st1-l1s13", GEO["st1-l1s13"], 20, (97, 96, 95, 61, 34, 33, 29, 28, 17, 16)),
]


def _cnn_setup(layers, B, T, D, seed=3):
    from ast_amd._lib import CnnLayerGrads, CnnLayerParams
    cfg, P, X, _, rng = RC.cnn_draws(B, T, D, None, None, False, seed=seed, layers=layers)
    n = len(layers)
    for i in range(n):          # running statistics that are not the initial (0, 1): eval mode reads them
        P[f"CNN_{i}_bn/avg_mean"] = 0.1 * rng.standard_normal(P[f"CNN_{i}_bn/avg_mean"].shape)
        P[f"CNN_{i}_bn/avg_var"] = 0.5 + rng.random(P[f"CNN_{i}_bn/avg_var"].shape)
        P[f"CNN_{i}_bn/beta"] = P[f"CNN_{i}_bn/beta"] + 0.3          # relu(shift) > 0 in most channels: what the masks must remove
    prm = {f"CNN_{i}{s}": dev(P[f"CNN_{i}{s}"]) for i in range(n) for s in ("/W", "_bn/gamma", "_bn/beta", "_bn/avg_mean", "_bn/avg_var")}
    grd = {k: torch.zeros_like(v) for k, v in prm.items()}
    cp, cg = (CnnLayerParams * n)(), (CnnLayerGrads * n)()
    for i in range(n):
        k = f"CNN_{i}"
        cp[i].W, cp[i].gamma, cp[i].beta = prm[k + "/W"].data_ptr(), prm[k + "_bn/gamma"].data_ptr(), prm[k + "_bn/beta"].data_ptr()
        cp[i].avg_mean, cp[i].avg_var = prm[k + "_bn/avg_mean"].data_ptr(), prm[k + "_bn/avg_var"].data_ptr()
        cg[i].dW, cg[i].dgamma, cg[i].dbeta = grd[k + "/W"].data_ptr(), grd[k + "_bn/gamma"].data_ptr(), grd[k + "_bn/beta"].data_ptr()
    return cfg, X.astype(np.float32), cp, cg, (prm, grd)


def _cnn_dims(lib, cd):
    t2, f2, feat = C.c_int(), C.c_int(), C.c_int()
    ok(lib, lib.astk_conv_bn_relu_out_dims(C.byref(cd), C.byref(t2), C.byref(f2), C.byref(feat)))
    return t2.value, feat.value


def _cnn_plain(lib, cfg, cp, X):
    """astk_conv_bn_relu_fwd(train = 0) on X (B, T, D): the existing entry point."""
    B, T, D = X.shape
    cd = _cnn_desc(cfg, B, T, D)
    T2, feat = _cnn_dims(lib, cd)
    nbytes = lib.astk_conv_bn_relu_workspace_bytes(C.byref(cd))
    ws = GuardedWS(nbytes)
    out = torch.empty(T2, B, feat, device="cuda")
    xd = dev(X)
    ok(lib, lib.astk_conv_bn_relu_fwd(C.byref(cd), cp, vp(xd), None, vp(out), vp(ws), nbytes, 0, stream()))
    ws.check("cnn fwd eval")
    return out


@pytest.mark.parametrize("cid,layers,D,frames", CNN_STACKS, ids=[s[0] for s in CNN_STACKS])
def test_cnn_rows_against_every_row_alone(lib, cid, layers, D, frames, gemm_split):
    B, T = len(frames), max(frames)
    assert all(min(M.out_lens(layers, n)) >= 1 for n in frames)
    cfg, X, cp, cg, keep = _cnn_setup(layers, B, T, D)
    Xp = X.copy()
    for b, n in enumerate(frames):
        Xp[b, n:] = 0.0                                      # the entry point's contract: zeros behind a row's frames
    cd = _cnn_desc(cfg, B, T, D)
    T2, feat = _cnn_dims(lib, cd)
    nbytes = lib.astk_conv_bn_relu_workspace_bytes(C.byref(cd))
    ws = GuardedWS(nbytes)
    out = torch.full((T2, B, feat), 7.0, device="cuda")
    out_len = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    xd, rl = dev(Xp), _i32(frames)
    ok(lib, lib.astk_conv_bn_relu_fwd_rows(C.byref(cd), cp, vp(xd), vp(rl), vp(out), vp(out_len), vp(ws), nbytes, stream()))
    ws.check("cnn fwd rows")
    want_len = [M.out_lens(layers, n)[-1] for n in frames]
    direct = beyond = 0.0
    lone = {}
    for b, n in enumerate(frames):
        o1 = _cnn_plain(lib, cfg, cp, Xp[b:b + 1, :n])
        lone[b] = o1
        assert o1.shape[0] == want_len[b]
        direct = max(direct, float((out[:want_len[b], b] - o1[:, 0]).abs().max()))
        beyond = max(beyond, float(out[want_len[b]:, b].abs().max()) if want_len[b] < T2 else 0.0)
    print(f"\n{cid} {gemm_split}: T'' {want_len}, out_len {out_len.tolist()}, batched against alone max abs diff {direct:.3e}, "
          f"beyond the lengths {beyond!r}, scale {float(out.abs().max()):.3f}")
    assert out_len.tolist() == want_len
    for b in range(B):
        close(out[:want_len[b], b], lone[b][:, 0], msg=f"row {b} ({frames[b]} frames) against the row alone")
    assert beyond == 0.0
    # the layer-0 path, where the direct kernel is expected: with the knob off the backward call on this workspace is refused before a launch
    if RC.conv0_direct_shape(layers) and gemm_split == "bf16x3":
        g = torch.zeros(T2, B, feat, device="cuda")
        with _knobs(lib, {"conv.direct0": 0}):
            rc = lib.astk_conv_bn_relu_bwd(C.byref(cd), cp, cg, vp(g), vp(ws), nbytes, stream())
        assert rc != 0 and "took the direct-convolution layer-0 path" in lib.astk_last_error().decode(), lib.astk_last_error().decode()
    # all lengths = T, and row_len = NULL: the bits of the existing entry point
    plain = _cnn_plain(lib, cfg, cp, X)
    xf = dev(X)
    for tag, lens in (("all lengths = T", _i32([T] * B)), ("row_len = NULL", None)):
        out.fill_(7.0)
        ok(lib, lib.astk_conv_bn_relu_fwd_rows(C.byref(cd), cp, vp(xf), vp(lens), vp(out), None, vp(ws), nbytes, stream()))
        ws.check("cnn fwd rows, " + tag)
        assert torch.equal(out, plain), f"{tag}: differs from astk_conv_bn_relu_fwd(train = 0) by {float((out - plain).abs().max()):.3e}"


def test_cnn_rows_refusals(lib):
    """Refused with a message before any launch (the output and the workspace keep what they held): a pooled stack, a length of 0 and of
    T + 1 (the call reads the device lengths back and checks them on the host), a row too short for its own geometry, a wrong
    struct_size."""
    layers = GEO["kt11-st3-kf16"]
    B, T, D = 3, 40, 80
    cfg, X, cp, _, keep = _cnn_setup(layers, B, T, D)
    good = _cnn_desc(cfg, B, T, D)
    pooled = _cnn_desc(cfg, B, T, D)
    pooled.pool_t[0], pooled.pool_f[0] = 2, 1
    sized = _cnn_desc(cfg, B, T, D)
    sized.struct_size -= 8
    nbytes = lib.astk_conv_bn_relu_workspace_bytes(C.byref(good))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), 7.0, device="cuda")
    xd = dev(X)
    for tag, cd, lens, cause in (("pooled", pooled, [40, 40, 40], "pooled layers"), ("length 0", good, [40, 0, 9], "outside 1..T"),
                                 ("length T + 1", good, [41, 40, 9], "outside 1..T"), ("too short alone", good, [40, 6, 9], "too short for layer 1"),
                                 ("struct_size", sized, [40, 40, 40], "struct_size")):
        rc = lib.astk_conv_bn_relu_fwd_rows(C.byref(cd), cp, vp(xd), vp(_i32(lens)), vp(out), None, vp(ws), nbytes, stream())
        msg = lib.astk_last_error().decode()
        print(f"{tag}: {msg}")
        assert rc != 0 and cause in msg, (tag, msg)
        torch.cuda.synchronize()
        assert float(out.min()) == 7.0 and float(out.max()) == 7.0 and int(ws.count_nonzero()) == 0, f"{tag}: a refused call wrote"


# ================================================================== LSTM operator
# (id, T, B, in_dim, h, layers, lengths, knobs, side, path): the issue's table -- 17 rows = two batch tiles, one partial; three layers at
# h = 64; the wide recurrence kernel; 32 rows on a stream of their own with four-step side-stream chunks -- then the two routes the issue
# leaves open, which the entry point serves too: the per-step loop ("lstm.persist" 0) and the hoisted form (h = 1024)
LSTM_CASES = [
    ("h256-two-tiles", 24, 17, 32, 256, 2, ([24, 23, 17, 16, 15, 2, 1] * 3)[:17], {}, False, 1),
    ("h64-three-layers", 12, 5, 24, 64, 3, [12, 9, 4, 1, 12], {}, False, 1),
    ("h512-wide", 8, 4, 16, 512, 1, [8, 5, 1, 3], {}, False, 1),
    ("h256-side-stream", 40, 32, 32, 256, 2, [40 - (3 * b) % 40 for b in range(32)], {"lstm.overlap_chunk": 4}, True, 1),
    ("h64-per-step", 12, 5, 24, 64, 3, [12, 9, 4, 1, 12], {"lstm.persist": 0}, False, 0),
    ("h1024-hoisted", 6, 3, 16, 1024, 1, [6, 2, 5], {}, False, 2),
]


@functools.lru_cache(maxsize=None)
def _lstm_twin(cid):
    """The draws of a case and, per row, the float64 twin of the row ALONE: enc (n, 2h), cT, hT (2, nl, h).  Computed once per case."""
    from oracle.ast_ref_torch import encoder_torch
    _, T, B, in_dim, h, nl, lens, _, _, _ = next(c for c in LSTM_CASES if c[0] == cid)
    c = RC.lstm_draws(T, B, in_dim, h, nl, False)
    Pt = {k: torch.tensor(v) for k, v in c["P"].items()}
    twin = []
    with torch.no_grad():
        for b, n in enumerate(lens):
            enc, cT, hT = encoder_torch({"rnn_config": {"enc_layers": nl}}, Pt, torch.tensor(c["x"][:n, b:b + 1]), None)
            twin.append((enc[0].numpy(), cT[:, :, 0].numpy(), hT[:, :, 0].numpy()))
    return c, twin


class _Lstm:
    """One descriptor's buffers and the two calls."""

    def __init__(self, lib, P, names, T, B, in_dim, h, nl, side_stream=None, main=None):
        from ast_amd._lib import LstmParams, LstmStackDesc
        self.lib, self.main = lib, main
        self.d = LstmStackDesc(T, B, in_dim, h, nl, 2)
        if side_stream is not None:
            self.d.side_stream = side_stream.cuda_stream
        self.prm = {k: dev(v) for k, v in P.items()}
        self.lp = (LstmParams * (2 * nl))()
        for i, n in enumerate(names):
            self.lp[i].Wu, self.lp[i].b, self.lp[i].Wl = (self.prm[n + s].data_ptr() for s in ("/upward/W", "/upward/b", "/lateral/W"))
        self.nbytes = lib.astk_lstm_stack_rows_workspace_bytes(C.byref(self.d))
        assert self.nbytes == lib.astk_lstm_stack_workspace_bytes(C.byref(self.d)) > 0
        self.ws = GuardedWS(self.nbytes)
        self.shape = (T, B, h, nl)

    def _stream(self):
        return C.c_void_p(self.main.cuda_stream) if self.main is not None else stream()

    def run(self, x, lens=None, rows=True):
        T, B, h, nl = self.shape
        enc = torch.full((B, T, 2 * h), 7.0, device="cuda")
        cT, hT = torch.full((2, nl, B, h), 7.0, device="cuda"), torch.full((2, nl, B, h), 7.0, device="cuda")
        xd = dev(x)
        rl = None if lens is None else _i32(lens)
        torch.cuda.synchronize()
        if rows:
            ok(self.lib, self.lib.astk_lstm_stack_fwd_rows(C.byref(self.d), self.lp, vp(xd), vp(rl), vp(enc), vp(cT), vp(hT), vp(self.ws), self.nbytes,
                                                           self._stream()))
        else:
            ok(self.lib, self.lib.astk_lstm_stack_fwd(C.byref(self.d), self.lp, vp(xd), None, vp(enc), vp(cT), vp(hT), vp(self.ws), self.nbytes,
                                                      self._stream()))
        torch.cuda.synchronize()
        self.ws.check("lstm fwd" + (" rows" if rows else ""))
        return enc, cT, hT


@pytest.mark.parametrize("cid", [c[0] for c in LSTM_CASES])
def test_lstm_rows_against_every_row_alone(lib, cid, gemm_split):
    _, T, B, in_dim, h, nl, lens, knobs, side, path = next(c for c in LSTM_CASES if c[0] == cid)
    c, twin = _lstm_twin(cid)
    P, names = c["P"], c["names"]
    x = c["x"].astype(np.float32)
    xz = x.copy()
    for b, n in enumerate(lens):
        xz[n:, b] = 0.0
    with _knobs(lib, knobs):
        main = side_s = None
        if side:
            main = torch.cuda.Stream()
            side_s = _concurrent_stream(lib, main)
        call = _Lstm(lib, P, names, T, B, in_dim, h, nl, side_s, main)
        assert lib.astk_lstm_stack_path(C.byref(call.d)) == path, "encoder route"
        if side:
            head, fwd_chunks, bwd_chunks = C.c_int(), C.c_int(), C.c_int()
            ok(lib, lib.astk_lstm_stack_side_plan(C.byref(call.d), C.byref(head), C.byref(fwd_chunks), C.byref(bwd_chunks)))
            print(f"\nside plan: head {head.value} steps, {fwd_chunks.value} forward chunks")
            assert fwd_chunks.value >= 1, "the case must put forward chunks on the side stream"
        enc, cT, hT = call.run(xz, lens)
        # ---- every row alone on the existing entry point, and both against the float64 twin
        direct = beyond = 0.0
        checks = []
        for b, n in enumerate(lens):
            one = _Lstm(lib, P, names, n, 1, in_dim, h, nl)
            e1, c1, h1 = one.run(xz[:n, b:b + 1], rows=False)
            direct = max(direct, float((enc[b, :n] - e1[0]).abs().max()), float((cT[:, :, b] - c1[:, :, 0]).abs().max()),
                         float((hT[:, :, b] - h1[:, :, 0]).abs().max()))
            beyond = max(beyond, float(enc[b, n:].abs().max()) if n < T else 0.0)
            checks.append((b, n, e1[0], c1[:, :, 0], h1[:, :, 0]))
        print(f"\n{cid} {gemm_split}: lengths {lens}, batched against alone max abs diff {direct:.3e}, beyond the lengths {beyond!r}")
        for b, n, e1, c1, h1 in checks:
            te, tc, th = twin[b]
            for what, lone, got, ref in (("enc_states", e1, enc[b, :n], te), ("cT", c1, cT[:, :, b], tc), ("hT", h1, hT[:, :, b], th)):
                close(lone, ref, msg=f"row {b} ({n} steps) ALONE against the float64 twin: {what}")
                close(got, ref, msg=f"row {b} ({n} steps) in the batch against the float64 twin: {what}")
        assert beyond == 0.0
        # ---- what lies behind a row's length is never read into a result: junk of magnitude 1e3 there, every output word the same
        # (bf16x3 and f32 only: fp16x2 scales every operand by its maximum, which sees the junk)
        if gemm_split != "fp16x2":
            rng = np.random.default_rng(11)
            xj = xz.copy()
            for b, n in enumerate(lens):
                xj[n:, b] = (rng.uniform(0.5, 1.0, size=xj[n:, b].shape) * rng.choice([-1.0, 1.0], size=xj[n:, b].shape) * 1e3).astype(np.float32)
            ej, cj, hj = call.run(xj, lens)
            for what, a, z in (("enc_states", ej, enc), ("cT", cj, cT), ("hT", hj, hT)):
                assert torch.equal(a, z), f"{what}: junk behind the lengths changed the result by {float((a - z).abs().max()):.3e}"
        # ---- all lengths = T, and row_len = NULL: the bits of astk_lstm_stack_fwd
        plain = call.run(x, rows=False)
        for tag, ll in (("all lengths = T", [T] * B), ("row_len = NULL", None)):
            got = call.run(x, ll)
            for what, a, z in zip(("enc_states", "cT", "hT"), got, plain):
                assert torch.equal(a, z), f"{tag}: {what} differs from astk_lstm_stack_fwd by {float((a - z).abs().max()):.3e}"


def test_lstm_rows_refusals(lib):
    """A length of 0 or T + 1 is refused on the host before any launch; so are a wrong struct_size and more than 32 rows."""
    T, B, in_dim, h, nl = 6, 3, 16, 64, 1
    c = RC.lstm_draws(T, B, in_dim, h, nl, False)
    call = _Lstm(lib, c["P"], c["names"], T, B, in_dim, h, nl)
    ws = torch.zeros(call.nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((B * T * 2 * h,), 7.0, device="cuda")
    st = torch.full((2 * nl * B * h,), 7.0, device="cuda")
    xd = dev(c["x"])
    from ast_amd._lib import LstmStackDesc
    sized = LstmStackDesc(T, B, in_dim, h, nl, 2)
    sized.struct_size -= 8
    for tag, d, lens, cause in (("length 0", call.d, [6, 0, 2], "outside 1..T"), ("length T + 1", call.d, [7, 6, 2], "outside 1..T"),
                                ("struct_size", sized, [6, 6, 6], "struct_size")):
        rc = lib.astk_lstm_stack_fwd_rows(C.byref(d), call.lp, vp(xd), vp(_i32(lens)), vp(out), vp(st), vp(st), vp(ws), call.nbytes, stream())
        msg = lib.astk_last_error().decode()
        print(f"{tag}: {msg}")
        assert rc != 0 and cause in msg, (tag, msg)
        torch.cuda.synchronize()
        assert float(out.min()) == 7.0 and float(st.min()) == 7.0 and int(ws.count_nonzero()) == 0, f"{tag}: a refused call wrote"
    assert lib.astk_lstm_stack_rows_workspace_bytes(C.byref(LstmStackDesc(T, 33, in_dim, h, nl, 2))) == 0


# ================================================================== model level
# es_en_20h's structure (3 + 3 encoder layers, 3 decoder layers) at h = 64 per direction: the persistent encoder route
SMALL = dict(enc_layers=3, dec_layers=3, H=128, E=16, A=64, c0=16, c1=16, V=57)
UTT_FRAMES = (8, 33, 64, 97, 150, 200)
D_FEAT = 80


def _build(seed=0, eos_bias=0.0, cnn_pool=None, **rnn_over):
    from oracle import ast_ref as R
    from ast_amd.seq2seq import SpeechEncoderDecoder
    cfg = tiny_cfg(**SMALL)
    cfg["rnn_config"].update(rnn_over)
    if cnn_pool is not None:
        cfg["cnn_config"]["cnn_pool"] = cnn_pool
    P = R.init_params(cfg, D_FEAT, SMALL["V"], seed=seed, dtype=np.float32)
    rng = np.random.default_rng(seed + 5)
    for i in range(2):          # eval mode reads the running statistics: not the initial (0, 1), and a shift that the ReLU lets through
        P[f"CNN_{i}_bn/avg_mean"] = (0.1 * rng.standard_normal(P[f"CNN_{i}_bn/avg_mean"].shape)).astype(np.float32)
        P[f"CNN_{i}_bn/avg_var"] = (0.5 + rng.random(P[f"CNN_{i}_bn/avg_var"].shape)).astype(np.float32)
        P[f"CNN_{i}_bn/beta"] = (P[f"CNN_{i}_bn/beta"] + 0.3).astype(np.float32)
    P["out/W"] = (P["out/W"] * OUT_SCALE).astype(np.float32)
    P["out/b"] = P["out/b"].copy()
    P["out/b"][EOS] += eos_bias
    m = SpeechEncoderDecoder(0, copy.deepcopy(cfg)).materialize(D_FEAT, values=P)
    Xs = [torch.from_numpy(R.synth_batch(1, T, D_FEAT, 3, SMALL["V"], seed=60 + i, dtype=np.float32)[0]) for i, T in enumerate(UTT_FRAMES)]
    return cfg, P, m, Xs


@functools.lru_cache(maxsize=None)
def _model_case():
    return _build()


def _bits_equal(a, b):
    return (torch.equal(a.enc, b.enc) and torch.equal(a.c0, b.c0) and torch.equal(a.h0, b.h0) and a.lens.tolist() == b.lens.tolist())


def test_encode_rows_batched_against_the_float64_oracle():
    """enc, c0 and h0 of the batched RowBatch against the float64 oracle encoding every utterance alone: no worse than max(2 e_alone,
    bound), e_alone the default call's own largest error on this case and bound = decode_helpers.tol() of the reference value, the
    tolerance tests/test_gpu_rows.py's model-level case applies to what it reads from a RowBatch."""
    from oracle import ast_ref as R
    cfg, P, m, Xs = _model_case()
    rows_of = [0, 0, 1, 2, 3, 3, 4, 5]
    rb0 = m.encode_rows(Xs, rows_of)
    assert m.last_encode_path == "alone"
    rb1 = m.encode_rows(Xs, rows_of, batch_encode=True)
    assert m.last_encode_path == "batched"
    assert rb1.lens.tolist() == rb0.lens.tolist() and rb1.enc.shape == rb0.enc.shape and rb1.c0.shape == rb0.c0.shape
    ref = {"enc": np.zeros(tuple(rb0.enc.shape)), "c0": np.zeros(tuple(rb0.c0.shape)), "h0": np.zeros(tuple(rb0.h0.shape))}
    for u in sorted(set(rows_of)):
        o = R.RefModel(cfg, {k: v.astype(np.float64) for k, v in P.items()}, SMALL["V"])
        o.train = False
        o.encode(Xs[u].numpy().astype(np.float64))
        o.init_decoder_state()
        e = np.asarray(o.enc_states.data)[0]
        for b in [b for b, v in enumerate(rows_of) if v == u]:
            assert rb0.lens[b] == e.shape[0]
            ref["enc"][b, :e.shape[0]] = e
            for k, link in enumerate(o.dec):
                ref["c0"][k, b], ref["h0"][k, b] = np.asarray(link.c.data)[0], np.asarray(link.h.data)[0]
    worst = {}
    for k in ("enc", "c0", "h0"):
        a0, a1 = getattr(rb0, k).double().cpu().numpy(), getattr(rb1, k).double().cpu().numpy()
        e0, e1 = np.abs(a0 - ref[k]), np.abs(a1 - ref[k])
        worst[k] = (float(e0.max()), float(e1.max()), float(np.abs(a1 - a0).max()), bool((e1 <= np.maximum(2 * e0.max(), tol(ref[k]))).all()))
        print(f"{k}: e_alone {worst[k][0]:.3e}, e_batched {worst[k][1]:.3e}, batched against alone {worst[k][2]:.3e}, scale {np.abs(ref[k]).max():.3f}")
    beyond = max(float(rb1.enc[b, n:].abs().max()) if n < rb1.T else 0.0 for b, n in enumerate(rb1.lens))
    print(f"lengths {rb1.lens.tolist()}, beyond the lengths {beyond!r}")
    assert all(w[3] for w in worst.values()) and beyond == 0.0


def test_forced_scores_through_both_row_batches():
    """score(rows=) of five target rows through the default and the batched RowBatch: log-probabilities under tol() of each other, argmax
    equal at the positions whose top-2 gap on the default path's per-step loop is at least 1e-4, and those are at least 0.95 of all."""
    from ast_amd.seq2seq import using_config
    _, _, m, Xs = _model_case()
    rows_of, L = [0, 0, 2, 3, 5], 10
    y = targets(len(rows_of), L, SMALL["V"], seed=4, go_first=True)
    rb0, rb1 = m.encode_rows(Xs, rows_of), m.encode_rows(Xs, rows_of, batch_encode=True)
    r0, r1 = m.score(None, y, rows=rb0), m.score(None, y, rows=rb1)
    gaps = np.zeros((len(rows_of), L - 1))
    with using_config("train", False):                   # the default path's rows alone on the per-step loop: the top-2 gaps
        for b in range(rb0.B):
            m._adopt_rows(rb0.row(b))
            ht = torch.zeros(1, m.A, dtype=torch.float32, device=m.device)
            for s in range(L - 1):
                logits, ht, _ = m.decode_step(torch.tensor([int(y[b, s])], dtype=torch.int32), ht)
                srt = np.sort(logits.double().cpu().numpy()[0])
                gaps[b, s] = srt[-1] - srt[-2]
    guarded = gaps >= 1e-4
    share = guarded.sum() / guarded.size
    rel = float((np.abs(r1.logp.astype(np.float64) - r0.logp) / tol(r0.logp.astype(np.float64))).max())
    rel_max = float((np.abs(r1.logp_max.astype(np.float64) - r0.logp_max) / tol(r0.logp_max.astype(np.float64))).max())
    wrong = int((r1.pred[guarded] != r0.pred[guarded]).sum())
    print(f"\nguarded {share:.4f} (smallest gap {gaps.min():.2e}), {wrong} argmax differ, logp max diff / tol {rel:.3f}, logp_max {rel_max:.3f}, "
          f"max abs diff {float(np.abs(r1.logp - r0.logp).max()):.3e}")
    assert share >= 0.95 and wrong == 0 and rel <= 1.0 and rel_max <= 1.0


def test_beam_search_takes_the_batched_encodings():
    """decode_beam_batch with model.batch_encode on four utterances: the hypotheses of the default path token for token, scores within
    the summed tol() (at least 1e-4 per token).  The default path's n-best scores are at least 1e-3 apart (asserted), so no ordering
    hangs on the encoder's rounding."""
    from ast_amd import nn as gnn
    _, _, m, Xs = _build(seed=21, eos_bias=2.0)
    Xs = [X[None] if X.dim() == 2 else X for X in Xs[1:5]]
    N = 5
    try:
        base = gnn.decode_beam_batch(m, Xs, 12, N, N)
        assert m.last_encode_path == "alone"
        m.batch_encode = True
        got = gnn.decode_beam_batch(m, Xs, 12, N, N)
        assert m.last_encode_path == "batched"
    finally:
        m.batch_encode = False
    apart = min(abs(a["score"] - b["score"]) for lst in base for a, b in zip(lst, lst[1:]))
    worst = max(abs(a["score"] - b["score"]) / ((len(a["hyp"]) - 1) * 1e-4) for la, lb in zip(base, got) for a, b in zip(la, lb))
    same = all([list(a["hyp"]) for a in la] == [list(b["hyp"]) for b in lb] for la, lb in zip(base, got))
    print(f"\nn-best scores at least {apart:.3e} apart; hypotheses equal: {same}; largest score difference / summed tol {worst:.3f}")
    assert apart >= 1e-3
    assert same and worst <= 1.0 and [len(l) for l in got] == [len(l) for l in base]


@pytest.mark.parametrize("tag,over", [("ln", dict(ln=True)), ("linear_proj", dict(linear_proj=True)), ("cnn_pool", dict(cnn_pool=[[2, 1], [1, 1]]))])
def test_models_the_batched_calls_do_not_serve_fall_back_silently(tag, over):
    _, _, m, Xs = _build(**over)
    rows_of = [0, 2, 2, 4]
    rb0 = m.encode_rows(Xs, rows_of)
    rb1 = m.encode_rows(Xs, rows_of, batch_encode=True)
    assert m.last_encode_path == "alone" and _bits_equal(rb0, rb1)


def test_the_default_call_is_the_utterances_alone_bit_for_bit():
    from ast_amd.seq2seq import RowBatch
    _, _, m, Xs = _model_case()
    rows_of = [0, 0, 1, 2, 3, 3, 4, 5]
    encs, c0s, h0s = m._encode_alone(Xs)
    lens = [int(e.shape[0]) for e in encs]
    enc = torch.zeros(len(rows_of), max(lens), m.H, device=m.device)
    for b, u in enumerate(rows_of):
        enc[b, :lens[u]] = encs[u]
    hand = RowBatch(enc, [lens[u] for u in rows_of], torch.stack([c0s[u] for u in rows_of], 1), torch.stack([h0s[u] for u in rows_of], 1))
    assert m.batch_encode is False
    rb = m.encode_rows(Xs, rows_of)
    assert m.last_encode_path == "alone" and _bits_equal(rb, hand)
