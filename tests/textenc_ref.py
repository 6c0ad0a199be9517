"""Plain float64 references and the shared case table for the code beside the episodic path: fumi_hip_clip_step, the three bi-LSTM
entries (csrc/textenc.hip) and the three linear entries on the GEMM family (csrc/gemm.hip: launch_gemm).

tests/test_textenc_edges_gpu.py takes every shape and seed from the tables below; tests/test_textenc_ref_cpu.py checks the references
against independent ones (torch.nn.LSTM, oracle.fumi_ref in float64) and asserts, per table row, the four input conditions that keep
a float64 comparison of an fp32 kernel meaningful:

  (a) ReLU margin     every tower pre-activation is at least RELU_MARGIN x its tensor's maximum away from 0, so no ReLU decision (and
                      with it no entry of the backward's mask) can differ between fp32 and float64
  (b) gradient scale  every compared gradient tensor has a float64 maximum above GRAD_SCALE_MIN; the analytically zero ones are listed
                      per case and asserted in absolute terms
  (c) norm scale      no latent row norm is below NORM_FRAC_MIN of the mean norm
  (d) fp32 headroom   the fp32 CPU oracle stays within HEADROOM (one quarter) of each GPU bound against float64

The references share no code with oracle/fumi_ref.py: the towers, the cosine, the two cross-entropies and the LSTM recurrence are
written out here; only the gradients come from float64 autograd."""
import functools

import torch

# ---- the bounds of tests/test_textenc_edges_gpu.py (helpers.rel_to_max semantics, all against float64) -------------------------
SIM_TOL = 1e-5
LOSS_TOL = 1e-5            # absolute
CLIP_GRAD_TOL = 1e-4
LSTM_OUT_TOL = 2e-5
LSTM_GRAD_TOL = 1e-4
TAPE_VS_FROZEN_TOL = 1e-6  # tests/test_lstm_finetune_gpu.py: the taped forward against the frozen one
LINEAR_TOL = 1e-5          # tests/test_hip_parity.py: test_linear_fwd / test_linear_bwd
ZERO_ABS = 1e-7            # quantities that are exactly 0 in real arithmetic (n = 1: loss and all gradients; dW_hh at L = 1)

RELU_MARGIN = 1e-4
GRAD_SCALE_MIN = 1e-4
NORM_FRAC_MIN = 1e-2
HEADROOM = 0.25


def rel_err(a, b, floor=1e-5):
    """helpers.rel_to_max without the import (this module is also read by the CPU suite on its own)."""
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


# ==== CLIP ======================================================================================================================
# name -> (n, Dt, D, P, seed)
CLIP_CASES = {
    "n1_one_pair": (1, 5, 7, 3, 1),                 # loss 0, every gradient 0
    "n2_all_vector": (2, 4, 4, 4, 2),               # smallest all-vector case
    "n61_all_scalar": (61, 33, 50, 67, 3),          # nothing a multiple of 4: scalar path in all four layouts, K tails
    "n65_row_past_tile": (65, 64, 64, 128, 4),      # one row past a 64-row tile; two full lane passes in row_norm_kernel
    "n256_one_loss_pass": (256, 20, 24, 96, 5),     # exactly one pass of clip_loss_kernel's loops; P = 64 + a half-lane tail
    "n257_second_loss_pass": (257, 36, 40, 64, 6),  # second pass of every loop; draw has ld = 257: one operand vector-eligible only
}
# zero-shot (need_loss = need_grad = False): (nt, ni) at these widths
CLIP_ZERO_SHOT = [(1, 5), (3, 130), (130, 3)]
CLIP_ZERO_SHOT_DIMS = (33, 50, 67, 7)               # Dt, D, P, seed


def _clear_relu_margin(x, W, b):
    """Move each unit's first-layer bias by the least multiple of the margin that takes every pre-activation of its column out of
    (-2 m, 2 m), m = RELU_MARGIN x max|z|.  A plain draw cannot meet condition (a) at the larger cases: the band holds about
    3e-4 of a Gaussian's mass, so n = 256, P = 96 expects some sixteen pre-activations inside it per draw and no seed passes.  The
    shift is at most a few 1e-3 of the pre-activations' spread, so the signs stay mixed within every row and every column."""
    z = x.double() @ W.double().t()
    m = 2.0 * RELU_MARGIN * float((z + b.double()).abs().max())
    b = b.clone()
    for j in range(W.shape[0]):
        for k in range(400):
            cand = (b[j].double() + (((k + 1) // 2) * (1 if k % 2 else -1)) * 2.0 * m).float()
            if float((z[:, j] + cand.double()).abs().min()) >= m:
                b[j] = cand
                break
        else:
            raise AssertionError("no bias shift clears the ReLU margin")
    return b


def _clip_inputs(nt, ni, Dt, D, P, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    w = []
    for o, i in ((P, Dt), (P, P), (P, D), (P, P)):
        w += [torch.randn(o, i, generator=g) / i ** 0.5, torch.randn(o, generator=g) * 0.1]
    text, image = torch.randn(nt, Dt, generator=g), torch.randn(ni, D, generator=g)
    w[1] = _clear_relu_margin(text, w[0], w[1])
    w[5] = _clear_relu_margin(image, w[4], w[5])
    return w, text, image


@functools.lru_cache(maxsize=None)
def clip_inputs(name):
    """(w: the eight tensors in oracle.fumi_ref.CLIP_KEYS order, text [n, Dt], image [n, D]) in float32.  Shared: do not modify."""
    n, Dt, D, P, seed = CLIP_CASES[name]
    return _clip_inputs(n, n, Dt, D, P, seed)


@functools.lru_cache(maxsize=None)
def clip_zero_shot_inputs(nt, ni):
    Dt, D, P, seed = CLIP_ZERO_SHOT_DIMS
    return _clip_inputs(nt, ni, Dt, D, P, seed + 10 * nt + ni)


def clip_ref(w, text, image, need_grad=True):
    """sim [nt, ni], and for nt == ni the loss and (need_grad) its eight gradients, all float64.  Also returns what the input
    conditions look at: `pre` (the two towers' pre-activations) and `norms` (the latent row norms)."""
    p = [t.detach().double().clone().requires_grad_(need_grad) for t in w]
    W0, b0, W2, b2, V0, c0, V2, c2 = p
    zt = text.double() @ W0.t() + b0
    tl = zt.clamp(min=0) @ W2.t() + b2
    zi = image.double() @ V0.t() + c0
    il = zi.clamp(min=0) @ V2.t() + c2
    na, nb = (tl * tl).sum(1).sqrt(), (il * il).sum(1).sqrt()
    sim = (tl @ il.t()) / (na[:, None] * nb[None, :])
    out = dict(sim=sim.detach(), pre=[zt.detach(), zi.detach()], norms=[na.detach(), nb.detach()], loss=None, grads=None)
    if sim.shape[0] != sim.shape[1]:
        return out
    d = sim.diagonal()
    loss = ((torch.logsumexp(sim, 1) - d).mean() + (torch.logsumexp(sim, 0) - d).mean()) / 2
    out["loss"] = loss.detach()
    if need_grad:
        out["grads"] = list(torch.autograd.grad(loss, p))
    return out


@functools.lru_cache(maxsize=None)
def clip_case_ref(name):
    return clip_ref(*clip_inputs(name))


@functools.lru_cache(maxsize=None)
def clip_zero_shot_ref(nt, ni):
    return clip_ref(*clip_zero_shot_inputs(nt, ni), need_grad=False)


# ==== bi-LSTM ===================================================================================================================
LSTM_V = 12
# name -> dict(B, S, L, E, H, pad: "last" (V - 1) or 0, lens: one length per row, interior: rows laid out [a, PAD, b, PAD, ...], seed,
#              zero_grads: indices (RNN_KEYS order) of the gradients that are exactly 0 in real arithmetic)
LSTM_CASES = {
    "one_token": dict(B=1, S=1, L=1, E=1, H=1, pad="last", lens=[1], interior=[], seed=1, zero_grads=[1, 5]),
    "rh259": dict(B=1, S=7, L=6, E=5, H=37, pad="last", lens=[0, 1, 2, 3, 5, 6, 6], interior=[], seed=2, zero_grads=[]),
    "all_vector_interior_pad": dict(B=2, S=5, L=9, E=32, H=64, pad=0, lens=list(range(10)), interior=[2], seed=3, zero_grads=[]),
    "r300": dict(B=1, S=300, L=4, E=3, H=3, pad="last", lens=[r % 5 for r in range(300)], interior=[], seed=4, zero_grads=[]),
    "l1_some_empty": dict(B=3, S=4, L=1, E=8, H=16, pad="last", lens=[1, 0, 1, 1, 0, 1, 1, 1, 0, 0, 1, 1], interior=[], seed=5,
                          zero_grads=[1, 5]),        # L = 1: h_prev is 0 at the only step, so dW_hh = 0
}
PAD_ROW_SCALE = 50.0


def lstm_weights(g, E, H):
    w = []
    for _ in range(2):
        w += [torch.randn(4 * H, E, generator=g) / E ** 0.5, torch.randn(4 * H, H, generator=g) / H ** 0.5,
              torch.randn(4 * H, generator=g) * 0.1, torch.randn(4 * H, generator=g) * 0.1]
    return w


@functools.lru_cache(maxsize=None)
def lstm_inputs(name):
    """(tokens [B, S, L] int64, table [V, E], the 8 LSTM tensors, pad_id, d_out [B, S, 2H]) -- the PAD row of the table is
    PAD_ROW_SCALE * randn (whatever leaks from a step past a row's length is scaled by it), every third row of d_out is zero.
    Shared: do not modify."""
    c = LSTM_CASES[name]
    B, S, L, E, H = c["B"], c["S"], c["L"], c["E"], c["H"]
    g = torch.Generator().manual_seed(2000 + c["seed"])
    pad = LSTM_V - 1 if c["pad"] == "last" else 0
    table = torch.rand(LSTM_V, E, generator=g) * 2 - 1
    table[pad] = PAD_ROW_SCALE * torch.randn(E, generator=g)
    real = torch.tensor([v for v in range(LSTM_V) if v != pad])
    tok = real[torch.randint(0, LSTM_V - 1, (B * S, L), generator=g)]
    assert len(c["lens"]) == B * S
    for r, n in enumerate(c["lens"]):
        if r in c["interior"]:
            assert 2 * n - 1 <= L
            keep = torch.zeros(L, dtype=torch.bool)
            keep[0:2 * n:2] = True                      # [a, PAD, b, PAD, ...]: n real tokens, a PAD among the first n positions
            tok[r, ~keep] = pad
        else:
            tok[r, n:] = pad
    w = lstm_weights(g, E, H)
    d_out = torch.randn(B, S, 2 * H, generator=g)
    d_out[:, 1::3] = 0
    return tok.view(B, S, L).contiguous(), table, w, pad, d_out


def lstm_row_lengths(tokens, pad_id):
    return (tokens.reshape(-1, tokens.shape[-1]) != pad_id).sum(-1)


def _lstm_forward64(tokens, table, w, pad_id, use_cell):
    """Row by row, step by step: a row of n non-PAD tokens is live at t < n; the forward direction walks its t = 0..n-1, the reverse
    direction t = n-1..0 (of L-1..0, the steps at t >= n are dead); gate order i f g o; the output is each direction's final h (c
    with use_cell); a row without a real token gives zeros."""
    L = tokens.shape[-1]
    flat = tokens.reshape(-1, L)
    H = w[1].shape[1]
    tb = table.double()
    rows = []
    for r in range(flat.shape[0]):
        n = int((flat[r] != pad_id).sum())
        halves = []
        for d in range(2):
            W_ih, W_hh, b_ih, b_hh = w[4 * d:4 * d + 4]
            h, c = tb.new_zeros(H), tb.new_zeros(H)
            for t in (range(n) if d == 0 else range(n - 1, -1, -1)):
                a = W_ih @ tb[flat[r, t]] + b_ih + W_hh @ h + b_hh
                i, f, gg, o = torch.sigmoid(a[:H]), torch.sigmoid(a[H:2 * H]), torch.tanh(a[2 * H:3 * H]), torch.sigmoid(a[3 * H:])
                c = f * c + i * gg
                h = o * torch.tanh(c)
            halves.append(c if use_cell else h)
        rows.append(torch.cat(halves))
    return torch.stack(rows).view(*tokens.shape[:-1], 2 * H)


def lstm_ref(tokens, table, w, pad_id, use_cell):
    with torch.no_grad():
        return _lstm_forward64(tokens, table, [t.double() for t in w], pad_id, use_cell)


def lstm_ref_grads(tokens, table, w, pad_id, use_cell, d_out):
    """(out, the eight gradients of (out * d_out).sum()) by float64 autograd."""
    ww = [t.detach().double().clone().requires_grad_(True) for t in w]
    out = _lstm_forward64(tokens, table, ww, pad_id, use_cell)
    g = torch.autograd.grad((out * d_out.double()).sum(), ww, allow_unused=True)
    return out.detach(), [torch.zeros_like(p) if gi is None else gi for gi, p in zip(g, ww)]


@functools.lru_cache(maxsize=None)
def lstm_case_ref(name, use_cell):
    tok, table, w, pad, d_out = lstm_inputs(name)
    return lstm_ref_grads(tok, table, w, pad, use_cell, d_out)


# ==== linear ====================================================================================================================
# contraction lengths at BK = 32, NST = 3: slab counts 1, 1, 1, 2, 3, 4, 5, 7 (prologue, the three unrolled step slots, the refill)
LINEAR_K_WALK = [1, 31, 32, 33, 96, 97, 129, 200]
LINEAR_K_WALK_MN = (33, 65)
_EDGE = [1, 31, 32, 33, 64, 65]                       # around the 32-wide wave tile and the 64-wide workgroup tile
LINEAR_MN_EDGES = [(v, v) for v in _EDGE] + [(1, 65), (65, 1), (31, 64), (64, 33)]
LINEAR_MN_EDGES_K = 36
LINEAR_MISALIGNED = (40, 36, 64)                      # every length a multiple of 4; only the base pointers differ
# (M, N, K) of every linear case: forward, and the two backward entries on the same tensors.  The K walk also runs with the walked
# length in the place each backward entry contracts over (N for dy W, M for dy^T x), so the ring is walked in three operand layouts.
LINEAR_SHAPES = ([LINEAR_K_WALK_MN + (k,) for k in LINEAR_K_WALK] + [(m, n, LINEAR_MN_EDGES_K) for m, n in LINEAR_MN_EDGES]
                 + [LINEAR_MISALIGNED])
LINEAR_BWD_DATA_WALK = [(33, k, 65) for k in LINEAR_K_WALK]
LINEAR_BWD_WEIGHT_WALK = [(k, 33, 65) for k in LINEAR_K_WALK]
LINEAR_ALL_SHAPES = sorted(set(LINEAR_SHAPES + LINEAR_BWD_DATA_WALK + LINEAR_BWD_WEIGHT_WALK))


@functools.lru_cache(maxsize=None)
def linear_inputs(M, N, K):
    """(x [M, K], W [N, K], b [N], dy [M, N]) in float32.  Shared: do not modify."""
    g = torch.Generator().manual_seed(3000 + M * 1000003 + N * 1009 + K)
    return (torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g),
            torch.randn(M, N, generator=g))


def linear_ref(x, W, b=None, act=0, dy=None):
    """y = act(x W^T + b) with act 0 none / 1 relu / 2 tanh; with dy also dx = dy W, dW = dy^T x, db = colsum(dy).  All float64."""
    y = x.double() @ W.double().t()
    if b is not None:
        y = y + b.double()
    y = [y, y.clamp(min=0), torch.tanh(y)][act]
    if dy is None:
        return y
    dy = dy.double()
    return y, dy @ W.double(), dy.t() @ x.double(), dy.sum(0)
