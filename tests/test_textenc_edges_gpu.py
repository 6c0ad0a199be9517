"""GPU edges of the code beside the episodic path, through the fumi_amd.hip wrappers, against the float64 references of
tests/textenc_ref.py: fumi_hip_clip_step (the loss kernel's loop strides, one pair, the scalar GEMM path in all four layouts, the lane
tail of the row norm, zero-shot at nt != ni), the bi-LSTM entries (a large non-zero PAD row, rows without a real token, an interior
PAD, L = 1, H = 1, R*H just past a block, R > 256) and the linear entries (the staging ring's slab counts, the tile edges, a base
pointer 4 bytes off 16).  Every shape and seed is a row of the tables in tests/textenc_ref.py; tests/test_textenc_ref_cpu.py asserts
the input conditions of every row.  Each test prints its errors before it asserts (DESIGN.md section 27 quotes them)."""
import pytest
import torch

from oracle import fumi_ref as R
from helpers import rel_to_max, RNN_KEYS
import textenc_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _g(t, dev):
    return t.to(dev).contiguous()


# ---- CLIP ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.CLIP_CASES))
def test_clip_step_edges(dev, ws, name):
    """sim, loss and all eight gradients of one table row; the gradient buffers are handed in NaN-filled, so an element the step
    does not write fails too."""
    from fumi_amd import hip
    n = T.CLIP_CASES[name][0]
    w, text, image = T.clip_inputs(name)
    ref = T.clip_case_ref(name)
    wd = [_g(t, dev) for t in w]
    g_w = [torch.full_like(t, float("nan")) for t in wd]
    out = hip.clip_step(ws, _g(text, dev), _g(image, dev), wd, g_w=g_w)
    sim, loss, grads = out["sim"].cpu(), float(out["loss"]), [g.cpu() for g in out["grads"]]
    e_sim, e_loss = rel_to_max(sim, ref["sim"]), abs(loss - float(ref["loss"]))
    if n == 1:                                                # one pair: both soft-maxes are over one entry
        g_abs = [float(g.abs().max()) for g in grads]
        print(f"\ntextenc-edge clip {name}: sim {e_sim:.2e} loss {loss:.2e} max|g| {max(g_abs):.2e} (absolute)")
        assert e_sim <= T.SIM_TOL
        assert loss <= T.ZERO_ABS
        for k, a in zip(R.CLIP_KEYS, g_abs):
            assert a <= T.ZERO_ABS, (k, a)
    else:
        e_g = [rel_to_max(a, b) for a, b in zip(grads, ref["grads"])]
        print(f"\ntextenc-edge clip {name}: sim {e_sim:.2e} loss {e_loss:.2e} grads {max(e_g):.2e}")
        assert e_sim <= T.SIM_TOL
        assert e_loss <= T.LOSS_TOL
        for k, e in zip(R.CLIP_KEYS, e_g):
            assert e <= T.CLIP_GRAD_TOL, (k, e)
    assert ws.read_status() == 0


@pytest.mark.parametrize("nt,ni", T.CLIP_ZERO_SHOT)
def test_clip_zero_shot_edges(dev, ws, nt, ni):
    from fumi_amd import hip
    w, text, image = T.clip_zero_shot_inputs(nt, ni)
    out = hip.clip_step(ws, _g(text, dev), _g(image, dev), [_g(t, dev) for t in w], need_loss=False, need_grad=False)
    assert out["loss"] is None and out["grads"] is None and out["sim"].shape == (nt, ni)
    e = rel_to_max(out["sim"].cpu(), T.clip_zero_shot_ref(nt, ni)["sim"])
    print(f"\ntextenc-edge clip zero-shot {nt} x {ni}: sim {e:.2e}")
    assert e <= T.SIM_TOL
    assert ws.read_status() == 0


def test_clip_loss_refuses_unpaired_rows(dev, ws):
    """The loss pairs text row i with image row i: nt != ni with need_loss raises and leaves the device status clean."""
    from fumi_amd import hip
    w, text, image = T.clip_zero_shot_inputs(3, 130)
    wd = [_g(t, dev) for t in w]
    with pytest.raises(hip.FumiHipError):
        hip.clip_step(ws, _g(text, dev), _g(image, dev), wd, need_loss=True, need_grad=False)
    with pytest.raises(hip.FumiHipError):
        hip.clip_step(ws, _g(text, dev), _g(image, dev), wd)
    assert ws.read_status() == 0


# ---- bi-LSTM -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_cell", [False, True])
@pytest.mark.parametrize("name", list(T.LSTM_CASES))
def test_lstm_edges(dev, ws, name, use_cell):
    """Frozen and taped forward against float64, taped against frozen, all eight gradients against float64.  table[pad_id] is
    50 * randn: a non-zero dgates at a step past a row's length, or a forward step taken there, is scaled by it."""
    from fumi_amd import hip
    c = T.LSTM_CASES[name]
    tok, table, w, pad, d_out = T.lstm_inputs(name)
    ref_out, ref_g = T.lstm_case_ref(name, use_cell)
    tokd, tbd, wd = _g(tok, dev), _g(table, dev), [_g(t, dev) for t in w]
    frozen = hip.lstm_bidir(ws, tokd, tbd, wd, pad, use_cell).cpu()
    out, tape = hip.lstm_bidir_train(ws, tokd, tbd, wd, pad, use_cell)
    out = out.cpu()
    gs = [g.cpu() for g in hip.lstm_bidir_bwd(ws, tokd, tbd, wd, pad, use_cell, tape, _g(d_out, dev))]
    e_f, e_t, e_tf = rel_to_max(frozen, ref_out), rel_to_max(out, ref_out), rel_to_max(out, frozen)
    e_g = [None if i in c["zero_grads"] else rel_to_max(a, b) for i, (a, b) in enumerate(zip(gs, ref_g))]
    print(f"\ntextenc-edge lstm {name} use_cell={use_cell}: frozen {e_f:.2e} taped {e_t:.2e} taped-vs-frozen {e_tf:.2e} "
          f"grads {max(e for e in e_g if e is not None):.2e}")
    assert e_f <= T.LSTM_OUT_TOL
    assert e_t <= T.LSTM_OUT_TOL
    assert e_tf <= T.TAPE_VS_FROZEN_TOL
    empty = (T.lstm_row_lengths(tok, pad) == 0).view(tok.shape[:2])
    assert int(empty.sum()) == c["lens"].count(0)
    assert float(frozen[empty].abs().sum()) == 0.0 and float(out[empty].abs().sum()) == 0.0     # a row without a real token
    for i, (k, a, b, e) in enumerate(zip(RNN_KEYS, gs, ref_g, e_g)):
        if e is None:                                          # analytically zero (h_prev = 0 at a row's only step)
            assert float(b.abs().max()) == 0.0 and float(a.abs().max()) <= T.ZERO_ABS, (k, float(a.abs().max()))
        else:
            assert float(b.abs().max()) > T.GRAD_SCALE_MIN, k
            assert e <= T.LSTM_GRAD_TOL, (k, e)
    assert torch.equal(gs[2], gs[3]) and torch.equal(gs[6], gs[7])                              # the two biases add into the same gates
    assert ws.read_status() == 0


# ---- linear --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", T.LINEAR_SHAPES)
def test_linear_fwd_edges(dev, ws, M, N, K):
    from fumi_amd import hip
    x, W, b, _ = T.linear_inputs(M, N, K)
    xd, Wd, bd = _g(x, dev), _g(W, dev), _g(b, dev)
    errs = []
    for act in (0, 1, 2):
        for bias, bias_d in ((b, bd), (None, None)):
            y = hip.linear_fwd(ws, xd, Wd, bias_d, act).cpu()
            errs.append(rel_to_max(y, T.linear_ref(x, W, bias, act)))
    print(f"\ntextenc-edge linear fwd {M} x {N} x {K}: {max(errs):.2e}")
    assert max(errs) <= T.LINEAR_TOL, errs
    assert ws.read_status() == 0


@pytest.mark.parametrize("M,N,K", list(dict.fromkeys(T.LINEAR_SHAPES + T.LINEAR_BWD_DATA_WALK + T.LINEAR_BWD_WEIGHT_WALK)))
def test_linear_bwd_edges(dev, ws, M, N, K):
    from fumi_amd import hip
    x, W, b, dy = T.linear_inputs(M, N, K)
    _, rx, rW, rb = T.linear_ref(x, W, b, 0, dy)
    dx = hip.linear_bwd_data(ws, _g(dy, dev), _g(W, dev)).cpu()
    dW, db = hip.linear_bwd_weight(ws, _g(dy, dev), _g(x, dev))
    errs = [rel_to_max(dx, rx), rel_to_max(dW.cpu(), rW), rel_to_max(db.cpu(), rb)]
    print(f"\ntextenc-edge linear bwd {M} x {N} x {K}: dx {errs[0]:.2e} dW {errs[1]:.2e} db {errs[2]:.2e}")
    assert max(errs) <= T.LINEAR_TOL, errs
    assert ws.read_status() == 0


def _off16(t, dev):
    """The same values as a contiguous view that starts one element into a larger buffer: every length as before, the pointer 4 bytes
    off a 16-byte boundary (no 16-byte load may use it)."""
    buf = torch.empty(t.numel() + 1, device=dev, dtype=torch.float32)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("which", ["both", "first", "second"])
def test_linear_misaligned_base(dev, ws, which):
    """M, N, K = 40, 36, 64: every length is a multiple of 4, so only the base pointers keep launch_gemm off its 16-byte path -- with
    both operands moved, and with either one alone.  Against float64, and against the same call on aligned copies (the two paths may
    round differently: within the bound, not bit-equal)."""
    from fumi_amd import hip
    M, N, K = T.LINEAR_MISALIGNED
    x, W, b, dy = T.linear_inputs(M, N, K)
    y64, rx, rW, rb = T.linear_ref(x, W, b, 0, dy)
    al = {k: _g(v, dev) for k, v in dict(x=x, W=W, b=b, dy=dy).items()}
    assert all(v.data_ptr() % 16 == 0 for v in al.values())
    a_off, b_off = which in ("both", "first"), which in ("both", "second")
    mv = lambda k, off: _off16(al[k], dev) if off else al[k]
    got = [hip.linear_fwd(ws, mv("x", a_off), mv("W", b_off), mv("b", True), 0),
           hip.linear_bwd_data(ws, mv("dy", a_off), mv("W", b_off)),
           *hip.linear_bwd_weight(ws, mv("dy", a_off), mv("x", b_off))]
    want = [hip.linear_fwd(ws, al["x"], al["W"], al["b"], 0), hip.linear_bwd_data(ws, al["dy"], al["W"]),
            *hip.linear_bwd_weight(ws, al["dy"], al["x"])]
    e64 = [rel_to_max(a.cpu(), r) for a, r in zip(got, [y64, rx, rW, rb])]
    e_al = [rel_to_max(a.cpu(), c.cpu()) for a, c in zip(got, want)]
    print(f"\ntextenc-edge linear misaligned {which}: vs float64 {max(e64):.2e} vs aligned {max(e_al):.2e}")
    assert max(e64) <= T.LINEAR_TOL, e64
    assert max(e_al) <= T.LINEAR_TOL, e_al
    assert ws.read_status() == 0
