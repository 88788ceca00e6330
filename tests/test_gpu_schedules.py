"""GPU parity tests of the SHIPPED schedule.  NN.train_epoch and bench.py run the train step on a compute stream of their own; there the
model finds a second stream (SpeechEncoderDecoder._side_stream) and (i) the library cuts the layer-0 input projection into flag-gated time
chunks beside the forward recurrence (lstm.hip: plan_side_fwd), (ii) the decoder's parameter gradients run, capped to the free CUs, beside
the encoder's backward recurrence (seq2seq.py: _backward).  Every other whole-step test runs on the legacy default stream, where all of
that is off by design.  Here every test runs under `torch.cuda.stream(torch.cuda.Stream())`, asserts that the side stream was found and
-- through astk_lstm_stack_side_plan -- that chunks were really planned, and that the sticky status word is clean at the end.

Small shapes plan no chunks by themselves (a chunk is sized to fill the free CUs: hundreds of steps at batch 4), so the small cases set
lstm.overlap_chunk = 4 (chunks of 4 steps); the full-size cases of tests/test_golden.py run the plan as shipped, with no knob."""
import numpy as np
import pytest
import torch

from conftest import tiny_cfg
from schedule_helpers import (assert_first_step_against_oracle, gpu_model, make_inputs, oracle_case, require_side, side_plan, status_word,
                              train_step_parity)

pytestmark = pytest.mark.gpu

D = 80
CHUNK4 = {"lstm.overlap_chunk": 4}

# name -> (cfg builder, B, T, L, V, drop, teach): T'' = 70, two layers, one batch tile | T'' = 70, three layers, a ragged second batch tile, masks
# and noise | T'' = 48, the h = 256 recurrence, the decoder's row split 32 + 8
SHAPES = {
    "b4-t70": (lambda d: tiny_cfg(enc_layers=2, dec_layers=1, H=128, E=16, A=64, c0=8, c1=16, V=57, drop=d), 4, 280, 8, 57, 0.0, 0.8),
    "b18-t70-drop": (lambda d: tiny_cfg(enc_layers=3, dec_layers=3, H=128, E=16, A=64, c0=8, c1=16, V=57, drop=d), 18, 280, 8, 57, 0.3, 0.8),
    "b40-t48-h256": (lambda d: tiny_cfg(enc_layers=2, dec_layers=1, H=512, E=64, A=128, c0=8, c1=16, V=300, drop=d), 40, 192, 6, 300, 0.0, 0.8),
}


def _case(shape):
    cfgf, B, T, L, V, drop, teach = SHAPES[shape]
    return (shape, cfgf, B, T, D, L, V, drop, teach)


def _step(m, X, y, teach=1.0):
    """forward_loss / cleargrads / backward on the current stream; returns (loss, enc_states, gradient arena) as host-independent clones."""
    from ast_amd.seq2seq import using_config
    with using_config("train", True):
        loss = m.forward_loss(X=X, y=y, teach_ratio=teach)
        m.cleargrads()
        loss.backward()
    torch.cuda.synchronize()
    return float(loss.data), m.enc_states.clone(), m.arena.grad.clone()


# ------------------------------------------------------------------ (a) the shipped schedule against the float64 oracle
@pytest.mark.parametrize("shape,knobs", [("b4-t70", CHUNK4), ("b18-t70-drop", CHUNK4), ("b40-t48-h256", CHUNK4),
                                         ("b4-t70", {"lstm.overlap_chunk": 4, "lstm.side_bwd": -1})],
                         ids=["b4-t70", "b18-t70-drop", "b40-t48-h256", "b4-t70-side-bwd"])
def test_train_step_parity_on_a_stream_of_its_own(shape, knobs, gemm_scheme):
    """test_train_step_parity's check (tests/schedule_helpers.py: same oracle, same bounds) with the step on its own stream: chunked layer-0
    projection beside the forward recurrence, decoder parameter gradients beside the backward recurrence; `side-bwd`: the input-gradient
    chunks and their wait kernels queue on the same side stream BEHIND those parameter gradients.
    Planned (forward head steps, forward chunks, backward chunks), as astk_lstm_stack_side_plan returned them on an MI355X (256 CUs), the
    same under all three schemes: b4-t70 (34, 9, 0); b18-t70-drop (34, 9, 0); b40-t48-h256 (24, 6, 0); b4-t70-side-bwd (34, 9, 18)."""
    seen = {}

    def inspect(m):
        require_side(m)
        seen["plan"] = side_plan(m._cur["ld"])
    train_step_parity(*_case(shape), gemm_scheme, stream=torch.cuda.Stream(), knobs=knobs, inspect=inspect)
    head, fwd, bwd = seen["plan"]
    print(f"side plan {shape} {gemm_scheme} {knobs}: head {head}, forward chunks {fwd}, backward chunks {bwd}")
    assert fwd >= 2 and head + 4 * fwd == (SHAPES[shape][2] // 4), seen      # (T'' = T / 4 here: the head and the 4-step chunks cover it)
    if knobs.get("lstm.side_bwd"):
        assert bwd >= 2, seen
    assert status_word() == 0


# ------------------------------------------------------------------ (b) late chunks
def _delay_side(main, side):
    """Holds `side` back for 1.5 ms from the moment `main` gets going: main spins 3 ms (time for the host to queue the whole step behind
    it), side waits for the end of that spin and then spins 1.5 ms itself.  The library orders the side stream behind the main one where it
    forks, so the spin sits in front of every chunk product while the step on `main` is already running: layer-0 cells that reach a
    chunk before the spin is over find its flag DOWN and wait (bounded spins far below the hand-off limit of seconds: a delay inside the
    protocol, no time-out)."""
    import ctypes as C
    from ast_amd import _lib
    lib = _lib.load()
    _lib.check(lib.astk_spin(3000, None, C.c_void_p(main.cuda_stream)))
    go = torch.cuda.Event()
    go.record(main)
    side.wait_event(go)
    _lib.check(lib.astk_spin(1500, None, C.c_void_p(side.cuda_stream)))


def test_late_side_stream_chunks_give_the_same_bits(tune):
    """The rate model sizes the in-line head so that no chunk is late: a layer-0 cell normally finds its flag raised.  Here the side stream is
    held back (see _delay_side) so that the cells meet flags that are still down and take the waiting branch -- the acquire and the re-read
    of freshly written gates.  Loss and encoder states must be the bits of the same model's un-delayed step, the gradients agree up to the
    order of float atomics, no time-out.  (Plan: head 34, 9 chunks.)  How much of the 1.5 ms is left when the recurrence reaches its first
    chunk is not controlled at this level -- the main stream runs the input copy and the CNN between the end of its spin and the encoder
    call (some tens of microseconds at this shape) -- so the test does not PROVE that a cell waited; the operator-level case
    test_lstm_stack_late_side_stream_chunks, where the encoder call follows the spin directly, does."""
    tune("lstm.overlap_chunk", 4)
    shape, cfgf, B, T, D_, L, V, drop, teach = _case("b4-t70")
    cfg = cfgf(drop)
    P, X, y = make_inputs(cfg, B, T, D_, L, V)
    main = torch.cuda.Stream()
    with torch.cuda.stream(main):
        m = gpu_model(cfg, P, D_, V)
        m.gemm_precision = "bf16x3"
        m.inject = {"use_truth": [1] * (L - 1)}
        Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
        _step(m, Xd, yd)                                   # warm: the side stream exists, the code objects are loaded
        require_side(m)
        assert side_plan(m._cur["ld"])[1] >= 2, side_plan(m._cur["ld"])
        want = _step(m, Xd, yd)
        _delay_side(main, m._side)
        got = _step(m, Xd, yd)
    assert got[0] == want[0], (got[0], want[0])
    assert torch.equal(got[1], want[1]), float((got[1] - want[1]).abs().max())
    assert float((got[2] - want[2]).abs().max()) <= 1e-5 * float(want[2].abs().max())
    assert status_word() == 0


# ------------------------------------------------------------------ (c) side on against side off
@pytest.mark.parametrize("shape", ["b4-t70", "b40-t48-h256"])
def test_side_stream_step_equals_the_inline_step(shape, gemm_scheme, tune):
    """include/astk.h (astk_lstm_stack_desc.side_stream): forward results are bit-identical to the in-line schedule, backward results equal
    up to the order of float atomics (1e-5 of the largest gradient entry, test_overlapped_backward_equals_inline_backward's bound).  Same
    weights and batch, two fresh models, one on the default stream and one on a stream of its own.  fp16x2 is the header's stated exception
    (capped launches run on bf16x3 operands: the chunked steps use other arithmetic than the head): both runs are held to the float64
    oracle's bounds instead.  (Plans: b4-t70 head 34, 9 chunks; b40-t48-h256 head 24, 6 chunks.  On an MI355X the bits agreed under bf16x3
    and f32 at both shapes.)"""
    tune("lstm.overlap_chunk", 4)
    name, cfgf, B, T, D_, L, V, drop, teach = _case(shape)
    cfg = cfgf(drop)
    P, X, y = make_inputs(cfg, B, T, D_, L, V)
    o = oracle_case(name, cfgf, B, T, D_, L, V, drop, teach) if gemm_scheme == "fp16x2" else None
    flags = o["flags"] if o else [1] * (L - 1)
    res = []
    for own in (False, True):
        torch.cuda.synchronize()
        s = torch.cuda.Stream() if own else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            m = gpu_model(cfg, P, D_, V)
            m.gemm_precision = gemm_scheme
            m.inject = {"use_truth": flags}
            res.append(_step(m, torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda(), teach) + (m.arena.to_numpy(grads=True),))
        if own:
            require_side(m)
            plan = side_plan(m._cur["ld"])
            print(f"side plan {shape} {gemm_scheme}: {plan}")
            assert plan[1] >= 2, plan
        else:
            assert m._side is None
    (l0, e0, g0, n0), (l1, e1, g1, n1) = res
    if gemm_scheme == "fp16x2":
        for lv, enc, named in ((l0, e0, n0), (l1, e1, n1)):
            assert_first_step_against_oracle(name, o, lv, None, enc.cpu().numpy(), named)
    else:
        assert l0 == l1, (l0, l1)
        assert torch.equal(e0, e1), float((e0 - e1).abs().max())
        assert float((g0 - g1).abs().max()) <= 1e-5 * float(g0.abs().max())
    assert status_word() == 0


# ------------------------------------------------------------------ (f) changing shapes under the shipped schedule
def test_changing_shapes_on_a_stream_of_its_own(tune):
    """One model over batches of changing shape, as the bucketed loader delivers them: the pools, the workspaces, the chunk-flag words and the
    side stream are reused from shape to shape (the third shape's recurrence, 20 steps, is shorter than the capped parameter-gradient phase
    beside it).  After each step: the loss is the bits, the gradients (no update: the parameters stay put) the sums up to float-atomics
    order, of a fresh model that has only ever seen that shape.  (Plans, head / chunks: 34 / 9, 18 / 3, 12 / 2, 34 / 9, 34 / 9.)"""
    tune("lstm.overlap_chunk", 4)
    name, cfgf, _, _, D_, _, V, drop, _ = _case("b4-t70")
    cfg = cfgf(drop)
    from oracle import ast_ref as R
    P = R.init_params(cfg, D_, V, seed=0, dtype=np.float32)
    main = torch.cuda.Stream()
    plans = []
    with torch.cuda.stream(main):
        m = gpu_model(cfg, P, D_, V)
        for i, (B, T, L) in enumerate([(4, 280, 8), (18, 120, 5), (4, 80, 3), (18, 280, 8), (4, 280, 8)]):
            X, y = R.synth_batch(B, T, D_, L, V, seed=50 + i, dtype=np.float32)
            Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
            m.inject = {"use_truth": [1] * (L - 1)}
            got = _step(m, Xd, yd)
            require_side(m)
            plans.append(side_plan(m._cur["ld"]))
            fresh = gpu_model(cfg, P, D_, V)
            fresh.inject = {"use_truth": [1] * (L - 1)}
            want = _step(fresh, Xd, yd)
            require_side(fresh)
            assert got[0] == want[0], (i, B, T, L, got[0], want[0])
            assert torch.equal(got[1], want[1]), (i, B, T, L)
            assert float((got[2] - want[2]).abs().max()) <= 1e-5 * float(want[2].abs().max()), (i, B, T, L)
    print("side plans of the five shapes:", plans)
    assert plans[0][1] >= 2 and plans[3][1] >= 2 and plans[4] == plans[0], plans
    assert status_word() == 0


# ------------------------------------------------------------------ deterministic mode as the PROCESS default beside a side stream
@pytest.mark.parametrize("B,T,L", [(4, 80, 3), (4, 280, 8)])
def test_process_wide_deterministic_mode_keeps_the_step_on_one_stream(B, T, L, tune):
    """astk_set_tuning("gemm.deterministic", 1) with model.deterministic left False: the fix-up workspace of the deterministic split tiles is
    process-wide and serves one launch at a time, so the model must not put the decoder's parameter gradients on a second stream beside
    the encoder's weight-gradient products (short buckets: the recurrence between them is over first).  m._side stays None, and every
    evaluation of a batch leaves the same bits in the loss and in the gradient arena."""
    tune("gemm.deterministic", 1)
    tune("lstm.overlap_chunk", 4)
    name, cfgf, _, _, D_, _, V, drop, _ = _case("b4-t70")
    cfg = cfgf(drop)
    P, X, y = make_inputs(cfg, B, T, D_, L, V)
    X2 = np.ascontiguousarray(np.roll(X, 1, axis=0) * 0.9, np.float32)
    main = torch.cuda.Stream()
    with torch.cuda.stream(main):
        m = gpu_model(cfg, P, D_, V)
        assert m.deterministic is False
        m.inject = {"use_truth": [1] * (L - 1)}
        sets = [(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()), (torch.from_numpy(X2).cuda(), torch.from_numpy(y).cuda())]
        from ast_amd.seq2seq import using_config
        with using_config("train", True):                   # (the forward pass alone decides it: asserted in front of the backward call)
            m.forward_loss(X=sets[0][0], y=sets[0][1], teach_ratio=1.0)
        assert m._side is None, "a step under the process-wide deterministic default must not use the side stream"
        ref = [_step(m, *sets[0]), _step(m, *sets[1])]
        assert m._side is None
        assert side_plan(m._cur["ld"])[1:] == (0, 0)
        for it in range(2):
            for which in (1, 0):
                loss, _, grad = _step(m, *sets[which])
                assert loss == ref[which][0], (it, which, loss, ref[which][0])
                assert torch.equal(grad, ref[which][2]), (it, which, float((grad - ref[which][2]).abs().max()))
        assert m._side is None
    assert status_word() == 0
