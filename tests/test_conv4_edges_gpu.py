"""The fp32 Conv4 encoder (csrc/conv_gemm.hip, conv_first.hip, conv_ew.hip, conv4.hip) against the float64 sweep at the shapes its
edge code was written for: odd, non-square, Cin = 2, persistent band chunks and the two-level coefficient sum.  tests/test_conv4_gpu.py
drives the same kernels at square, even shapes with one band per workgroup and one coefficient chunk; this file changes only the shapes.
Tolerances are those of test_conv4_gpu.py for the same quantity (every intermediate 2e-4 of its scale with borders exactly 0, logits
1e-4, predictions outside the 1e-5 margin, meta-gradients 1e-3 with the 2 % floor, features 1e-5); tests/test_conv4_edges_cpu.py
ties the float64 sweep to autograd at these shapes and holds the inputs to the matcher's cap of 6 near-tie decisions.

The cases (tests/conv4_forms.py CASES; shape = Cin, H, W, blocks; alpha = 0.05), the branch each reaches and why:

  A  3 x 9 x 13, 2 blocks, B 2, N 3, K 2, Q 3, T 2.  9 x 13 -> 4 x 6 -> 2 x 3.
     Block 1 odd in both extents and non-square: c1_kernel walks bands_per_img = (9+1)/2 = 5 bands, the fifth a half band
     (two = false, full_row = false: yb = 4 = Ho); Wb = (13+1)/2 = 7 blocks of which the seventh is half a block (vx = false, not
     `full`: xo = 6 = Wo), its dxo load clamped to column min(6, Wo-1) = 5.  Plain path: bwd_apply_kernel's vy / vx / valid[] at
     row 8 and column 12, pixels of no pooling window with du != 0.  Ho = 4 != Wo = 6 at block 1, 2 != 3 at the last block: the
     feature matrix c*Ho*Wo + yo*Wo + xo (F = 64 * 2 * 3 = 384) and load_dxo's `last` branch with Ho != Wo.  T = 2 second order: every
     tangent form (TAN = true) of the kernels above.
  B  2 x 15 x 10, 3 blocks, same episode sizes.  15 x 10 -> 7 x 5 -> 3 x 2 -> 1 x 1.
     Cin = 2: 18 kappa = 9 k-pairs, NO zero-padded kappa (Cin 1: 9 -> 10, Cin 3: 27 -> 28), so conv1_kernel, wgrad1_kernel and
     c1_kernel's load_w1 end on a full pair.  Odd H with even W at block 1 (half band, no half block); block 2 is 7 x 5, odd in both
     extents, through the plain element-wise kernels; the last map is 1 x 1: F = 64, the smallest the entry points accept.
  C  1 x 7 x 22, 2 blocks, same episode sizes.  7 x 22 -> 3 x 11 -> 1 x 5.
     Cin = 1.  Wb = 22/2 = 11 blocks = two 8-block MFMA tiles per band (ntile = 2), the second with 3 of 8 blocks (vb = false for
     xo >= 11, dxo column clamped).  H odd: half band at yb = 3.  Block 2 is 3 x 11, odd and non-square.
  D  3 x 21 x 23, 2 blocks, B 16 on ONE lane (conv4_set_option(1, 1)), N 3, K 2, Q 3, T 1.
     c1_chunks: ceil(1024 / 16) = 64 workgroups per episode; the support pass has 6 images x 11 bands = 66 bands, the query pass
     9 x 11 = 99, so chunk = ceil(66/64) = ceil(99/64) = 2 bands per persistent workgroup (33 and 50 workgroups).  The band loop
     runs twice with the slab of the next band prefetched; bands_per_img = 11 is odd, so for every second image the half band
     (yb = 10) is the FIRST band of a workgroup, which continues with band 0 of the NEXT image (orow and the image pointer change
     inside the loop), and the last query workgroup walks a single band.
  E  3 x 29 x 31, 2 blocks, B 2, N 3, K 3, Q 3, T 1.
     9 images x 31 x 33 padded pixels = 9207 = 72 tiles of 128, so coef_sum_kernel runs two chunks of 64 and 8 slabs: the second
     chunk's t0 = 64, the clamp min(t + 4u, t1 - 1) and a last chunk shorter than one 16-slab round.  Odd and non-square as well.
"""
import pytest
import torch

import conv4_forms as CF
from conv4_forms import LOGIT_TOL, MARGIN, _check_grads, _g, _match_episodes
from oracle import conv4_ref as C
from helpers import rel_to_max, safe_margin_mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


@pytest.fixture(params=["fused-block1", "plain"])
def c1mode(request):
    """Block 1 either recomputed band by band (csrc/conv_first.hip, the default) or through the plain passes."""
    from fumi_amd import hip
    hip.conv4_set_option(0, 1 if request.param == "fused-block1" else 0)
    yield request.param
    hip.conv4_set_option(0, 1)


@pytest.mark.parametrize("name", list(CF.CASES))
def test_every_intermediate_at_the_edges(name, dev, ws, c1mode):
    """Every stored map, pooled map, p, dz, dxo, du and every tangent counterpart of one second-order MAML step against the
    float64 sweep, 2e-4 rel-to-max, borders exactly 0, near-tie decisions taken the way the engine took them."""
    from fumi_amd import hip
    c = CF.CASES[name]
    CF.case_reaches_its_edge(name)
    if name == "D":
        chunk, _, bpi = CF.c1_chunks(c["B"], c["N"] * c["K"], c["shape"][1])
        assert chunk >= 2 and bpi % 2 == 1
    if name == "E":
        assert CF.coef_chunks(c["N"] * c["Q"], c["shape"][1], c["shape"][2]) >= 2
    try:
        if c["lanes"] is not None:
            hip.conv4_set_option(1, c["lanes"])
        CF.check_every_intermediate(hip, ws, dev, c["shape"], c["B"], c["N"], c["K"], c["Q"], c["T"], CF.ALPHA, c["seed"],
                                    c1mode == "fused-block1")
    finally:
        hip.conv4_set_option(1, 0)


def _maml_step(hip, ws, dev, ep, theta, head, T, first_order):
    """maml_conv4_step held as test_maml_conv4_step_matches_the_float64_sweep holds it."""
    B, N = ep["x_s"].shape[0], head.shape[0]
    p = theta + [head[:, :-1].contiguous(), head[:, -1].contiguous()]
    out = hip.maml_conv4_step(ws, _g(ep["x_s"], dev), _g(ep["y_s"], dev), _g(ep["x_q"], dev), _g(ep["y_q"], dev),
                              [_g(t, dev) for t in p], T, CF.ALPHA, first_order)
    assert ws.read_status() == 0
    ms = _match_episodes(hip, ws, dev, out["logits"].cpu(), theta, head[None].expand(B, -1, -1), ep, T, CF.ALPHA, first_order)
    zq = torch.stack([m[0] for m in ms])
    assert rel_to_max(out["loss_b"].cpu(), torch.stack([m[1] for m in ms])) <= LOGIT_TOL
    mask = safe_margin_mask(zq, MARGIN)
    assert torch.equal(out["preds"].cpu()[mask], zq.max(-1)[1][mask]) and float(mask.float().mean()) > 0.9
    if bool(mask.all()):
        assert torch.allclose(out["acc_b"].cpu().double(), zq.max(-1)[1].eq(ep["y_q"]).double().mean(-1), atol=1e-6)
    ref = [sum(m[2][i] for m in ms) / B for i in range(len(theta))]
    hb = sum(m[3] for m in ms) / B
    _check_grads([str(i) for i in range(len(p))], out["g_params"], ref + [hb[:, :-1], hb[:, -1]])
    pl = [t.clone().requires_grad_(True) for t in p]            # fp32 autograd agrees on what no tie can move: the logits
    r32 = C.maml_conv4_meta_step(pl, ep["x_s"], ep["y_s"], ep["x_q"], ep["y_q"], T, CF.ALPHA, first_order, need_grad=False)
    assert rel_to_max(out["logits"].cpu(), r32["logits"]) <= 10 * LOGIT_TOL


def _fumi_step(hip, ws, dev, name, tanh):
    """fumi_conv4_step held as test_fumi_conv4_step_matches_the_float64_sweep holds it."""
    c = CF.CASES[name]
    B, N, T = c["B"], c["N"], c["T"]
    ep, theta, phi = CF.fumi_inputs(name)
    stats = torch.zeros(2, device=dev)
    out = hip.fumi_conv4_step(ws, N, _g(ep["x_s"], dev), _g(ep["y_s"], dev), _g(ep["x_q"], dev), _g(ep["y_q"], dev),
                              [_g(t, dev) for t in theta], [_g(t, dev) for t in phi], T, CF.ALPHA, tanh, text_s=_g(ep["text_s"], dev),
                              stats=stats)
    assert ws.read_status() == 0
    heads, ph = CF.fumi_heads(ep, phi, N, tanh)
    ms = _match_episodes(hip, ws, dev, out["logits"].cpu(), theta, heads.detach(), ep, T, CF.ALPHA, False)
    zq = torch.stack([m[0] for m in ms])
    mask = safe_margin_mask(zq, MARGIN)
    assert torch.equal(out["preds"].cpu()[mask], zq.max(-1)[1][mask])
    loss = float(torch.stack([m[1] for m in ms]).mean())
    assert abs(float(stats[0]) - loss) <= LOGIT_TOL * max(1.0, loss)
    g_theta = [sum(m[2][i] for m in ms) / B for i in range(len(theta))]
    g_phi = torch.autograd.grad(heads, ph, grad_outputs=torch.stack([m[3] for m in ms]) / B)
    _check_grads([f"theta{i}" for i in range(len(theta))] + [f"phi{i}" for i in range(4)], out["g_theta"] + out["g_phi"],
                 g_theta + list(g_phi))


@pytest.mark.parametrize("name", CF.WHOLE_STEP_CASES)
def test_whole_steps_at_the_edges(name, dev, ws, c1mode):
    """maml_conv4_step second and first order at the table's T (and, case A, fumi_conv4_step with tanh): logits and loss 1e-4,
    predictions outside the 1e-5 margin, every meta-gradient 1e-3 of its scale (floor: 2 % of the largest gradient)."""
    from fumi_amd import hip
    c = CF.CASES[name]
    ep, theta, head = CF.maml_inputs(c["shape"], c["B"], c["N"], c["K"], c["Q"], c["seed"])
    for first_order in (False, True):
        _maml_step(hip, ws, dev, ep, theta, head, c["T"], first_order)
    if name == "A":
        _fumi_step(hip, ws, dev, name, True)


def test_features_and_encoder_pair_at_a_non_square_shape(dev, c1mode):
    """conv4_features at 3 x 9 x 13 (2 blocks) and 3 x 15 x 10 (3 blocks) against oracle/conv4_ref.conv4_features at 1e-5 (the bound
    of test_conv4_features_op); then conv4_encode(keep_tape) -> conv4_encode_bwd with random feature gradients at 3 x 9 x 13 against
    float64 autograd of sum <feats, dfeats>: load_dxo's `last` branch with Ho = 2 != Wo = 3.
    Bound per gradient tensor: 1e-3 of its scale.  The tie argument of test_am3_conv4_step_matches_autograd (a ReLU / arg-max
    decision within round-off of a tie re-routes the gradient of its block and of every block before it by up to a percent) raises
    it to 1e-2 ONLY for the tensors of blocks 0 .. l, l being the deepest block at which the float64 forward of these very inputs
    has a decision within TIE_TOL = 3e-6 of a tie -- worked out from the float64 oracle (conv4_forms.deepest_tie_block), never from
    the engine's output; with no such decision every tensor is held to 1e-3."""
    from fumi_amd import hip
    ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
    for (Cin, H, W, nblk), seed in (((3, 9, 13, 2), 51), ((2, 15, 10, 3), 52)):
        ep, theta, Fd = CF._case(seed, 3, 4, 2, 3, Cin, H, W, nblk)
        f = hip.conv4_features(ws, _g(ep["x_q"], dev), [_g(t, dev) for t in theta]).cpu()
        ref = torch.stack([C.conv4_features(ep["x_q"][b], theta) for b in range(3)])
        assert f.shape == (3, 12, Fd) and rel_to_max(f, ref) <= 1e-5
    B, Cin, H, W, nblk = 3, 3, 9, 13, 2
    ep, theta, Fd = CF._case(53, B, 4, 2, 3, Cin, H, W, nblk)
    g = torch.Generator().manual_seed(53)
    dfs, dfq = torch.randn(B, ep["x_s"].shape[1], Fd, generator=g), torch.randn(B, ep["x_q"].shape[1], Fd, generator=g)
    th_d = [_g(t, dev) for t in theta]
    xs, xq = _g(ep["x_s"], dev), _g(ep["x_q"], dev)
    f_s, f_q = hip.conv4_encode(ws_enc, xs, xq, th_d, keep_tape=True)
    g_th = hip.conv4_encode_bwd(ws_enc, xs, xq, _g(dfs, dev), _g(dfq, dev), th_d)
    assert ws_enc.read_status() == 0
    th64 = [t.double().requires_grad_(True) for t in theta]
    r_s = torch.stack([C.conv4_features(ep["x_s"][b].double(), th64) for b in range(B)])
    r_q = torch.stack([C.conv4_features(ep["x_q"][b].double(), th64) for b in range(B)])
    assert rel_to_max(f_s.cpu(), r_s.detach()) <= 1e-5 and rel_to_max(f_q.cpu(), r_q.detach()) <= 1e-5
    ref = torch.autograd.grad((r_s * dfs.double()).sum() + (r_q * dfq.double()).sum(), th64)
    tie = CF.deepest_tie_block([ep["x_s"][b] for b in range(B)] + [ep["x_q"][b] for b in range(B)], theta)
    names = [f"block{i}.{p}" for i in range(nblk) for p in ("W", "g", "b")]
    errs = {n: rel_to_max(a.cpu().double(), r) for n, a, r in zip(names, g_th, ref)}
    print(f"conv4_encode_bwd at 3x9x13: deepest near-tie block {tie}, errors {errs}")
    for i, n in enumerate(names):
        assert errs[n] <= (1e-2 if i // 3 <= tie else 1e-3), (n, errs[n], tie)
