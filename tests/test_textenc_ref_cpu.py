"""CPU suite: keeps tests/textenc_ref.py honest (no GPU, no library).

tests/test_textenc_edges_gpu.py holds fumi_hip_clip_step, the bi-LSTM entries and the linear entries to the float64 references of
tests/textenc_ref.py.  That only means something when those references agree with independent ones (torch.nn.LSTM over a packed
sequence; oracle.fumi_ref in float64) and when every row of the shared case table meets the four input conditions listed at the top
of tests/textenc_ref.py.  The fp32-oracle errors of condition (d) are printed (pytest -s) for DESIGN.md section 27."""
import pytest
import torch
import torch.nn.functional as F

from oracle import fumi_ref as R
import textenc_ref as T


def _d(ts):
    return [t.double() for t in ts]


# ---- the references against independent ones ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.LSTM_CASES))
def test_lstm_ref_matches_torch_lstm_and_the_oracle(name):
    """Rows that pack_padded_sequence accepts (length >= 1, no interior PAD) against torch.nn.LSTM's h_n / c_n in float64; the rows it
    refuses against oracle.fumi_ref.lstm_encode in float64; a row without a real token is exactly zero."""
    tok, table, w, pad, _ = T.lstm_inputs(name)
    c = T.LSTM_CASES[name]
    L, E, H = c["L"], c["E"], c["H"]
    flat = tok.reshape(-1, L)
    lens = T.lstm_row_lengths(tok, pad)
    assert lens.tolist() == c["lens"]
    prefix = torch.tensor([bool((flat[r, :int(lens[r])] != pad).all()) for r in range(flat.shape[0])])
    packable = (lens >= 1) & prefix
    assert (~prefix).nonzero().flatten().tolist() == c["interior"]
    rnn = torch.nn.LSTM(E, H, num_layers=1, bidirectional=True, batch_first=True).double()
    with torch.no_grad():
        for k, t in zip(["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
                         "bias_ih_l0_reverse", "bias_hh_l0_reverse"], w):
            getattr(rnn, k).copy_(t.double())
        x = table.double()[flat[packable]]
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, lens[packable], batch_first=True, enforce_sorted=False)
        _, (h_n, c_n) = rnn(packed)
    for use_cell, s_n in ((False, h_n), (True, c_n)):
        mine = T.lstm_ref(tok, table, w, pad, use_cell).reshape(-1, 2 * H)
        assert mine.dtype == torch.float64
        want = torch.cat([s_n[0], s_n[1]], -1)
        assert float((mine[packable] - want).abs().max()) <= 1e-12
        orc = R.lstm_encode(tok, table.double(), _d(w), pad, use_cell).reshape(-1, 2 * H)
        if bool((~packable).any()):
            assert float((mine[~packable] - orc[~packable]).abs().max()) <= 1e-12
        assert float(mine[lens == 0].abs().sum()) == 0.0


@pytest.mark.parametrize("name", list(T.LSTM_CASES))
@pytest.mark.parametrize("use_cell", [False, True])
def test_lstm_ref_grads_match_the_oracle(name, use_cell):
    tok, table, w, pad, d_out = T.lstm_inputs(name)
    out, g = T.lstm_case_ref(name, use_cell)
    ww = [t.double().requires_grad_(True) for t in w]
    o2 = R.lstm_encode(tok, table.double(), ww, pad, use_cell)
    g2 = torch.autograd.grad((o2 * d_out.double()).sum(), ww)
    assert float((out - o2.detach()).abs().max()) <= 1e-12
    for a, b in zip(g, g2):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("name", list(T.CLIP_CASES))
def test_clip_ref_matches_the_oracle(name):
    w, text, image = T.clip_inputs(name)
    mine = T.clip_case_ref(name)
    orc = R.clip_step([t.double().requires_grad_(True) for t in w], text.double(), image.double())
    assert float((mine["sim"] - orc["sim"]).abs().max()) <= 1e-12 and abs(float(mine["loss"]) - float(orc["loss"])) <= 1e-12
    for a, b in zip(mine["grads"], orc["grads"]):
        assert a.dtype == torch.float64 and float((a - b).abs().max()) <= 1e-12


@pytest.mark.parametrize("nt,ni", T.CLIP_ZERO_SHOT)
def test_clip_ref_zero_shot_matches_the_oracle(nt, ni):
    w, text, image = T.clip_zero_shot_inputs(nt, ni)
    mine = T.clip_zero_shot_ref(nt, ni)
    assert mine["loss"] is None and mine["sim"].shape == (nt, ni)
    assert float((mine["sim"] - R.clip_forward(_d(w), text.double(), image.double())).abs().max()) <= 1e-12


def test_linear_ref_matches_autograd():
    x, W, b, dy = T.linear_inputs(33, 65, 97)
    for act in (0, 1, 2):
        xx, WW, bb = [t.double().requires_grad_(True) for t in (x, W, b)]
        y = F.linear(xx, WW, bb)
        y = [y, torch.relu(y), torch.tanh(y)][act]
        assert float((T.linear_ref(x, W, b, act) - y.detach()).abs().max()) <= 1e-12
    xx, WW, bb = [t.double().requires_grad_(True) for t in (x, W, b)]
    gx, gW, gb = torch.autograd.grad((F.linear(xx, WW, bb) * dy.double()).sum(), [xx, WW, bb])
    _, dx, dW, db = T.linear_ref(x, W, b, 0, dy)
    assert max(float((dx - gx).abs().max()), float((dW - gW).abs().max()), float((db - gb).abs().max())) <= 1e-12
    assert float((T.linear_ref(x, W, None, 0) + b.double() - T.linear_ref(x, W, b, 0)).abs().max()) <= 1e-12


# ---- the four input conditions, per row of the case table -----------------------------------------------------------------------
def _check_relu_margin_and_norms(ref):
    for z in ref["pre"]:                                                        # (a)
        assert float(z.abs().min()) >= T.RELU_MARGIN * float(z.abs().max())
        assert z.numel() < 4 or (bool((z > 0).any()) and bool((z < 0).any()))   # (the ReLU is not trivial)
    for nrm in ref["norms"]:                                                    # (c)
        assert float(nrm.min()) >= T.NORM_FRAC_MIN * float(nrm.mean())


@pytest.mark.parametrize("name", list(T.CLIP_CASES))
def test_clip_case_conditions(name):
    w, text, image = T.clip_inputs(name)
    n = T.CLIP_CASES[name][0]
    ref = T.clip_case_ref(name)
    _check_relu_margin_and_norms(ref)
    o32 = R.clip_step([t.clone().requires_grad_(True) for t in w], text, image)          # (d): the fp32 CPU oracle
    e_sim, e_loss = T.rel_err(o32["sim"], ref["sim"]), abs(float(o32["loss"]) - float(ref["loss"]))
    assert e_sim <= T.HEADROOM * T.SIM_TOL
    if n == 1:
        assert abs(float(ref["loss"])) <= 1e-15 and all(float(g.abs().max()) <= 1e-15 for g in ref["grads"])
        assert e_loss <= T.HEADROOM * T.ZERO_ABS and all(float(g.abs().max()) <= T.HEADROOM * T.ZERO_ABS for g in o32["grads"])
        print(f"\nclip {name}: fp32 oracle sim {e_sim:.2e} loss {e_loss:.2e} (gradients exactly 0)")
        return
    assert e_loss <= T.HEADROOM * T.LOSS_TOL
    errs = []
    for k, a, b in zip(R.CLIP_KEYS, o32["grads"], ref["grads"]):
        assert float(b.abs().max()) > T.GRAD_SCALE_MIN, (k, float(b.abs().max()))       # (b)
        errs.append(T.rel_err(a, b))
        assert errs[-1] <= T.HEADROOM * T.CLIP_GRAD_TOL, (k, errs[-1])
    print(f"\nclip {name}: fp32 oracle sim {e_sim:.2e} loss {e_loss:.2e} grads {max(errs):.2e}")


@pytest.mark.parametrize("nt,ni", T.CLIP_ZERO_SHOT)
def test_clip_zero_shot_conditions(nt, ni):
    w, text, image = T.clip_zero_shot_inputs(nt, ni)
    ref = T.clip_zero_shot_ref(nt, ni)
    _check_relu_margin_and_norms(ref)
    e = T.rel_err(R.clip_forward(w, text, image), ref["sim"])
    assert e <= T.HEADROOM * T.SIM_TOL
    print(f"\nclip zero-shot {nt} x {ni}: fp32 oracle sim {e:.2e}")


@pytest.mark.parametrize("name", list(T.LSTM_CASES))
@pytest.mark.parametrize("use_cell", [False, True])
def test_lstm_case_conditions(name, use_cell):
    tok, table, w, pad, d_out = T.lstm_inputs(name)
    c = T.LSTM_CASES[name]
    assert tok.shape == (c["B"], c["S"], c["L"]) and float(table[pad].abs().max()) > 10.0      # the PAD row is large
    assert bool((d_out[:, 1::3] == 0).all()) and float(d_out.abs().max()) > 0
    out, g = T.lstm_case_ref(name, use_cell)
    ww = [t.clone().requires_grad_(True) for t in w]                                           # (d): the fp32 CPU oracle
    o32 = R.lstm_encode(tok, table, ww, pad, use_cell)
    g32 = torch.autograd.grad((o32 * d_out).sum(), ww)
    e_out = T.rel_err(o32.detach(), out)
    assert float(out.abs().max()) > 1e-2 and e_out <= T.HEADROOM * T.LSTM_OUT_TOL, e_out
    errs = []
    for i, (a, b) in enumerate(zip(g32, g)):
        if i in c["zero_grads"]:
            assert float(b.abs().max()) == 0.0 and float(a.abs().max()) <= T.HEADROOM * T.ZERO_ABS
            continue
        assert float(b.abs().max()) > T.GRAD_SCALE_MIN, (i, float(b.abs().max()))               # (b)
        errs.append(T.rel_err(a, b))
        assert errs[-1] <= T.HEADROOM * T.LSTM_GRAD_TOL, (i, errs[-1])
    print(f"\nlstm {name} use_cell={use_cell}: fp32 oracle out {e_out:.2e} grads {max(errs):.2e}")


@pytest.mark.parametrize("M,N,K", T.LINEAR_ALL_SHAPES)
def test_linear_case_conditions(M, N, K):
    x, W, b, dy = T.linear_inputs(M, N, K)
    errs = []
    for act in (0, 1, 2):
        y32 = F.linear(x, W, b)
        errs.append(T.rel_err([y32, torch.relu(y32), torch.tanh(y32)][act], T.linear_ref(x, W, b, act)))
    errs.append(T.rel_err(F.linear(x, W), T.linear_ref(x, W, None, 0)))
    _, dx, dW, db = T.linear_ref(x, W, b, 0, dy)
    errs += [T.rel_err(dy @ W, dx), T.rel_err(dy.t() @ x, dW), T.rel_err(dy.sum(0), db)]
    for r in (dx, dW, db):
        assert float(r.abs().max()) > T.GRAD_SCALE_MIN
    assert max(errs) <= T.HEADROOM * T.LINEAR_TOL, errs
    print(f"\nlinear {M} x {N} x {K}: fp32 torch {max(errs):.2e}")


def test_tables_hold_the_edges_they_are_there_for():
    C = T.CLIP_CASES
    assert [c[:4] for c in C.values()] == [(1, 5, 7, 3), (2, 4, 4, 4), (61, 33, 50, 67), (65, 64, 64, 128), (256, 20, 24, 96),
                                           (257, 36, 40, 64)]
    assert T.CLIP_ZERO_SHOT == [(1, 5), (3, 130), (130, 3)] and T.CLIP_ZERO_SHOT_DIMS[2] == 67
    Lc = T.LSTM_CASES
    assert [(c["B"], c["S"], c["L"], c["E"], c["H"]) for c in Lc.values()] == [(1, 1, 1, 1, 1), (1, 7, 6, 5, 37), (2, 5, 9, 32, 64),
                                                                                (1, 300, 4, 3, 3), (3, 4, 1, 8, 16)]
    assert Lc["rh259"]["S"] * Lc["rh259"]["H"] == 259 and [c["pad"] for c in Lc.values()].count(0) == 1
    assert set(Lc["r300"]["lens"]) == {0, 1, 2, 3, 4} and 0 in Lc["l1_some_empty"]["lens"] and 1 in Lc["l1_some_empty"]["lens"]
    assert [(k + 31) // 32 for k in T.LINEAR_K_WALK] == [1, 1, 1, 2, 3, 4, 5, 7]
    assert len(T.LINEAR_MN_EDGES) == 10 and all(v % 4 == 0 for v in T.LINEAR_MISALIGNED)
