"""GPU tests of AM3 with the bf16 ResNet-12 backbone (--model am3 --im_encoder resnet12) through the C ABI: the first-order encoder
pair fumi_hip_resnet12_encode / fumi_hip_resnet12_encode_bwd in the device's "encoder" workspace, fumi_hip_am3_step_dx on the main one.

"Parity unpinned" (the reference has no ResNet-12; its am3.py:44-46 leaves raw images a TODO).  Checkers:
  * the same kernels on another path: encode features against fumi_hip_resnet12_features bit for bit, and encode_bwd against the
    theta gradient of a T = 0 MAML step (same bf16 rounding points: fp32 noise only);
  * one block tightly against the bf16-rounded sweep oracle/resnet12_manual.py; two blocks and the 64/160/320/640 widths as a whole
    AM3 step against float64 autograd (oracle/resnet12_ref.features under oracle/conv4_ref.am3_conv4_step's AM3 head), with the
    drift bounds of tests/test_resnet12_gpu.py's header (a chain of bf16 roundings decorrelates with depth);
  * the taped and the recompute form, and every chunking of the meta-batch, bit-identical; the tape contract.
"""
import numpy as np
import pytest
import torch

from oracle import casegen as cg
from oracle import conv4_ref as CR
from oracle import resnet12_manual as M
from oracle import resnet12_ref as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wss(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def rel_l2(got, ref):
    num = sum(float(((a.cpu().double() - b.cpu().double()) ** 2).sum()) for a, b in zip(got, ref))
    return (num / sum(float((b.cpu().double() ** 2).sum()) for b in ref)) ** 0.5


def cosine(got, ref):
    dot = sum(float((a.cpu().double() * b.cpu().double()).sum()) for a, b in zip(got, ref))
    na = sum(float((a.cpu().double() ** 2).sum()) for a in got) ** 0.5
    return dot / (na * sum(float((b.cpu().double() ** 2).sum()) for b in ref) ** 0.5)


def case(seed, B, N, K, Q, H, channels, Dt=12):
    ep = CR.make_image_episodes(seed, B, N, K, Q, 3, H, H, Dt)
    return ep, RR.make_params(seed, 3, channels, torch.float32)


def on(dev, ts):
    return [t.to(dev).contiguous() for t in ts]


def encode_pair(wss, dev, ep, theta, dfs=None, dfq=None, scale=1.0, seed=3):
    """encode (tape kept) -> encode_bwd with the given (or seeded random) feature adjoints"""
    from fumi_amd import hip
    ws_enc = wss[1]
    xs, xq, th = ep["x_s"].to(dev), ep["x_q"].to(dev), on(dev, theta)
    fs, fq = hip.resnet12_encode(ws_enc, xs, xq, th, keep_tape=True)
    plan = hip.resnet12_encode_plan()
    if dfs is None:
        g = torch.Generator().manual_seed(seed)
        dfs, dfq = torch.randn(fs.shape, generator=g), torch.randn(fq.shape, generator=g)
    g_th = hip.resnet12_encode_bwd(ws_enc, xs, xq, dfs.to(dev), dfq.to(dev), th, scale=scale)
    assert ws_enc.read_status() == 0
    return fs, fq, [t.clone() for t in g_th], plan, (dfs, dfq)


# ---- the same kernels on the existing paths ------------------------------------------------------------------------------------------
def test_encode_features_equal_the_feature_pass(dev, wss):
    from fumi_amd import hip
    ep, theta = case(31, 3, 3, 2, 3, 16, (32, 64))
    th = on(dev, theta)
    fs, fq = hip.resnet12_encode(wss[1], ep["x_s"].to(dev), ep["x_q"].to(dev), th, keep_tape=False)
    assert wss[1].read_status() == 0
    assert torch.equal(fs, hip.resnet12_features(wss[0], ep["x_s"].to(dev), th))
    assert torch.equal(fq, hip.resnet12_features(wss[0], ep["x_q"].to(dev), th))
    # without a kept tape there is nothing to walk backwards
    with pytest.raises(hip.FumiHipError):
        hip.resnet12_encode_bwd(wss[1], ep["x_s"].to(dev), ep["x_q"].to(dev), torch.zeros_like(fs), torch.zeros_like(fq), th)


def test_encode_bwd_equals_the_maml_step_gradient(dev, wss):
    """MAML with T = 0: query forward -> head -> first-order backward.  Its theta gradient is encode_bwd from
    dfeats_q = dz W_head (dz = (softmax - onehot) / Qn) and dfeats_s = 0 with scale = grad_scale: the same kernels at the same
    roundings (grad_scale = 1/3 applied to dz instead would move every bf16 rounding of the backward: 5.6e-3 rel-L2 measured)."""
    from fumi_amd import hip
    N, B = 3, 3
    ep, theta = case(33, B, N, 2, 3, 16, (32, 64))
    rs = np.random.RandomState(5)
    Wf = torch.from_numpy((rs.standard_normal((N, 64)) * 0.1).astype(np.float32))
    bfin = torch.from_numpy((rs.standard_normal(N) * 0.1).astype(np.float32))
    out = hip.maml_resnet12_step(wss[0], ep["x_s"].to(dev), ep["y_s"].to(dev), ep["x_q"].to(dev), ep["y_q"].to(dev),
                                 on(dev, theta + [Wf, bfin]), 0, 0.05, False)
    assert wss[0].read_status() == 0
    z = out["logits"].cpu().double()
    Qn = z.shape[1]
    dz = (torch.softmax(z, -1) - torch.nn.functional.one_hot(ep["y_q"], N).double()) / Qn
    dfq = (dz @ Wf.double()).float()
    _, _, g, _, _ = encode_pair(wss, dev, ep, theta, torch.zeros(B, ep["x_s"].shape[1], 64), dfq, scale=1.0 / B)
    ref = out["g_params"][:-2]
    assert rel_l2(g, ref) <= 1e-3 and cosine(g, ref) >= 1 - 1e-5, (rel_l2(g, ref), cosine(g, ref))


# ---- against the oracles --------------------------------------------------------------------------------------------------------------
def sweep_encode_bwd(x, th64, df, rnd):
    """features of one image set and d<df, f>/dtheta by the autograd-free sweep (rnd = bf16_round: the engine's roundings)"""
    h, tapes = rnd(x), []
    for i in range(0, len(th64), M.PER_BLOCK):
        h, tp = M.block_fwd(h, th64[i:i + M.PER_BLOCK], rnd)
        tapes.append(tp)
    f = h.mean((2, 3))
    Mi, C, Ho, Wo = h.shape
    d = rnd((df / (Ho * Wo))[:, :, None, None].expand(Mi, C, Ho, Wo))
    g = []
    for i in reversed(range(len(tapes))):
        d, gb = M.block_bwd(d, tapes[i], rnd, need_dx=i > 0)
        g = gb + g
    return f, g


def test_one_block_pair_matches_the_bf16_sweep_tightly(dev, wss):
    ep, theta = case(35, 2, 3, 3, 2, 8, (32,))
    scale = 0.5
    fs, fq, g, _, (dfs, dfq) = encode_pair(wss, dev, ep, theta, scale=scale)
    th64 = [t.double() for t in theta]
    gs = [torch.zeros_like(t) for t in th64]
    for b in range(2):
        for x, f, df in ((ep["x_s"][b], fs[b], dfs[b]), (ep["x_q"][b], fq[b], dfq[b])):
            fr, gr = sweep_encode_bwd(x.double(), th64, df.double(), M.bf16_round)
            assert rel(f.cpu().double(), fr) <= 4e-3
            for a, gi in zip(gs, gr):
                a += scale * gi
    for i, (a, b) in enumerate(zip(g, gs)):        # (the one-block first-order bound of tests/test_resnet12_gpu.py)
        assert float((a.cpu().double() - b).norm() / b.norm()) <= 1e-2, i


# backbone gradient bounds (rel-L2, cosine) = the measured drift of the bf16 chain with a factor ~2 of head room: two blocks 0.13-0.15 /
# 0.989-0.991, the 64/160/320/640 widths 0.27 / 0.965 (the ten AM3 gradients: <= 0.04 / 0.999)
@pytest.mark.parametrize("channels,H,lamda_fixed,tol,cos_min", [
    ((32, 64), 16, None, 0.3, 0.97), ((32, 64), 16, 0, 0.3, 0.97), ((32, 64), 16, 1, 0.3, 0.97), (RR.CHANNELS, 16, None, 0.5, 0.9)])
def test_am3_step_against_float64_autograd(channels, H, lamda_fixed, tol, cos_min, dev, wss, monkeypatch):
    """encode -> am3_step_dx -> encode_bwd against float64 autograd through ResNet-12 + the AM3 head: loss, margin-masked predictions,
    the ten AM3 gradients, the backbone gradients (rel-L2 and cosine within the measured drift of a bf16 chain of this depth)."""
    from fumi_amd import hip
    B, N, K, Q, Dt, Ht, P = 2, 3, 2, 2, 12, 24, 32
    ep, theta = case(37, B, N, K, Q, H, channels, Dt)
    w = cg.make_am3_params(37, channels[-1], Dt, Ht, P)
    wl = [w[k] for k in hip.AM3_KEYS]
    ws_main, ws_enc = wss
    xs, xq, th = ep["x_s"].to(dev), ep["x_q"].to(dev), on(dev, theta)
    f_s, f_q = hip.resnet12_encode(ws_enc, xs, xq, th, keep_tape=True)
    out = hip.am3_step(ws_main, f_s, ep["y_s"].to(dev), f_q, ep["y_q"].to(dev), ep["text_s"].to(dev), on(dev, wl), N, lamda_fixed,
                       want_dx=True)
    g_th = hip.resnet12_encode_bwd(ws_enc, xs, xq, out["dx_s"], out["dx_q"], th)
    assert ws_main.read_status() == 0 and ws_enc.read_status() == 0
    monkeypatch.setattr(CR, "conv4_features", RR.features)          # the AM3 head of the Conv4 oracle in front of ResNet-12
    d64 = lambda t: t.double()
    ref = CR.am3_conv4_step([d64(t) for t in theta], {k: d64(v) for k, v in w.items()}, d64(ep["text_s"]), d64(ep["x_s"]), ep["y_s"],
                            d64(ep["x_q"]), ep["y_q"], N, lamda_fixed)
    nb = len(channels)
    assert rel(f_s.cpu().double(), ref["feats_s"]) <= 2e-2 * nb and rel(f_q.cpu().double(), ref["feats_q"]) <= 2e-2 * nb
    assert abs(float(out["loss"]) - float(ref["loss"])) <= 0.05 * max(1.0, abs(float(ref["loss"])))
    d2 = ref["dist"].transpose(1, 2).topk(2, dim=-1, largest=False)[0]
    mask = (d2[..., 1] - d2[..., 0]) > 5e-2 * d2[..., 1].abs().clamp_min(1.0)
    assert torch.equal(out["preds"].cpu()[mask], ref["preds"][mask])
    got, want = [], []
    for k, g in zip(hip.AM3_KEYS, out["grads"]):
        if float(ref["grads"][k].abs().max()) < 1e-9:      # identically zero (the image bias cancels in every distance when lamda = 1)
            assert float(g.abs().max()) < 1e-6, k
        else:
            got.append(g); want.append(ref["grads"][k])
    assert rel_l2(got, want) <= 0.1 and cosine(got, want) >= 0.995, (rel_l2(got, want), cosine(got, want))
    r, c = rel_l2(g_th, ref["grads_theta"]), cosine(g_th, ref["grads_theta"])
    assert r <= tol and c >= cos_min, (r, c)


# ---- forms and chunks ---------------------------------------------------------------------------------------------------------------
def test_taped_recompute_and_chunkings_are_bit_identical(dev, wss):
    from fumi_amd import hip
    ep, theta = case(39, 5, 3, 2, 3, 16, (32, 64))
    runs = {}
    runs["taped"] = encode_pair(wss, dev, ep, theta)
    hip.resnet12_set_budget(1e-6)                          # nothing fits: the recompute form, one episode per chunk
    try:
        runs["recompute"] = encode_pair(wss, dev, ep, theta)
    finally:
        hip.resnet12_set_budget(0)
    wss[1].set_profiling(True)                            # (phase timing runs one lane: the whole meta-batch is one chunk)
    try:
        runs["single"] = encode_pair(wss, dev, ep, theta)
    finally:
        wss[1].set_profiling(False)
    plans = {k: v[3] for k, v in runs.items()}
    assert plans["taped"][0] and plans["taped"][1] < 5, plans           # several chunks, taped
    assert not plans["recompute"][0] and plans["recompute"][1] == 1, plans
    assert plans["single"][1] == 5 and plans["single"][2] == 1, plans
    a = runs["taped"]
    for k in ("recompute", "single"):
        b = runs[k]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), k
        for i, (x, y) in enumerate(zip(a[2], b[2])):
            assert torch.equal(x, y), (k, i)


# ---- the tape contract --------------------------------------------------------------------------------------------------------------
def test_tape_contract(dev, wss):
    from fumi_amd import hip
    ws_main, ws_enc = wss
    N = 3
    ep, theta = case(41, 3, N, 2, 2, 16, (32, 64))
    xs, xq, th = ep["x_s"].to(dev), ep["x_q"].to(dev), on(dev, theta)
    fs, fq, g1, _, (dfs, dfq) = encode_pair(wss, dev, ep, theta)
    # linear in scale (powers of two: exact)
    _, _, g2, _, _ = encode_pair(wss, dev, ep, theta, dfs, dfq, scale=2.0)
    for a, b in zip(g1, g2):
        assert torch.equal(2 * a, b)
    # an AM3 step on the main workspace between the two calls leaves the tape alone
    hip.resnet12_encode(ws_enc, xs, xq, th, keep_tape=True)
    w = cg.make_am3_params(41, 64, 12, 16, 32)
    out = hip.am3_step(ws_main, fs, ep["y_s"].to(dev), fq, ep["y_q"].to(dev), ep["text_s"].to(dev), on(dev, [w[k] for k in hip.AM3_KEYS]),
                       N, None, want_dx=True)
    assert ws_main.read_status() == 0
    # a backward of another shape is refused and leaves the tape in place ...
    with pytest.raises(hip.FumiHipError):
        hip.resnet12_encode_bwd(ws_enc, xs[:, :4].contiguous(), xq, dfs[:, :4].to(dev).contiguous(), dfq.to(dev), th)
    g3 = hip.resnet12_encode_bwd(ws_enc, xs, xq, dfs.to(dev), dfq.to(dev), th)
    assert ws_enc.read_status() == 0
    for a, b in zip(g1, g3):
        assert torch.equal(a, b)
    # ... which the backward consumes
    with pytest.raises(hip.FumiHipError):
        hip.resnet12_encode_bwd(ws_enc, xs, xq, dfs.to(dev), dfq.to(dev), th)
    assert out["dx_s"].shape == fs.shape and ws_enc.read_status() == 0


# ---- the module and the CLI ---------------------------------------------------------------------------------------------------------
def test_am3_resnet12_evaluate_applies_the_engines_gradient(dev, wss):
    """AM3(im_encoder='resnet12').evaluate: one SGD step moves every parameter (ten AM3 tensors, 48 backbone tensors) by -lr x the
    gradient a direct call of the pair + am3_step returns for the same inputs (same kernels: fp32 round-off)."""
    from fumi_amd import hip
    from fumi_amd.models.am3 import AM3
    N, Dt = 5, 12
    ep = CR.make_image_episodes(8, 3, N, 2, 3, 3, 16, 16, Dt)
    batch = cg.to_batch(ep)
    torch.manual_seed(1)
    m = AM3(im_encoder="resnet12", im_emb_dim=0, text_encoder="BERT", text_emb_dim=Dt, text_hid_dim=16, prototype_dim=32,
            dropout=0.0, image_size=16).to(dev)
    p0 = [p.detach().clone() for p in m._w() + m.conv.theta()]
    xs, xq = ep["x_s"].to(dev), ep["x_q"].to(dev)
    fs, fq = hip.resnet12_encode(wss[1], xs, xq, p0[10:], keep_tape=True)
    out = hip.am3_step(wss[0], fs, ep["y_s"].to(dev), fq, ep["y_q"].to(dev), ep["text_s"].to(dev), p0[:10], N, None,
                       grad_scale=1.0 / 3, want_dx=True)
    g_direct = [g.clone() for g in out["grads"]] + [g.clone() for g in hip.resnet12_encode_bwd(wss[1], xs, xq, out["dx_s"], out["dx_q"],
                                                                                              p0[10:])]
    lr = 0.02
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    tr = m.evaluate(batch, opt, None, N, dev, task="train")
    assert np.isfinite(float(tr[0]))
    assert wss[0].read_status() == 0 and wss[1].read_status() == 0
    p1 = m._w() + m.conv.theta()
    assert len(p1) == 10 + 48
    for i, (a, b, g) in enumerate(zip(p0, p1, g_direct)):
        upd = (b.detach() - a).cpu()
        assert torch.allclose(upd, -lr * g.cpu(), rtol=1e-4, atol=1e-7 + 1e-5 * float(g.abs().max()) * lr), f"parameter {i}"
    te = m.evaluate(batch, None, None, N, dev, task="test")
    assert len(te) == 11 and np.isfinite(float(te[0]))
    emb = m((None, None, xq), im_only=True)
    assert emb.shape == (3, xq.shape[1], 32)


def test_cli_am3_resnet12_end_to_end_on_gpu(dev, tmp_path, monkeypatch):
    """`python -m fumi_amd.main --model am3 --im_encoder resnet12 --dataset synthetic` (shortened): raw images -> bf16 ResNet-12 ->
    AM3 -> training through the encoder pair -> checkpoint -> test."""
    from fumi_amd import main as cli
    monkeypatch.chdir(tmp_path)
    argv = ["--model", "am3", "--dataset", "synthetic", "--im_encoder", "resnet12", "--image_size", "16", "--text_encoder", "BERT",
            "--text_emb_dim", "32", "--batch_size", "8", "--num_shots", "5", "--num_ways", "5", "--num_shots_test", "5",
            "--epochs", "100", "--eval_freq", "50", "--num_ep_test", "16", "--lr", "1e-3", "--dropout", "0.25",
            "--log_dir", str(tmp_path / "res"), "--synthetic_classes", "16", "--wandb_offline"]
    args = cli.parse_args(argv)
    assert args.device.type == "cuda"
    res = cli.main(args)
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    assert res["test_acc"] > 0.25                                       # chance = 0.2 (the FuMI ResNet-12 CLI test's margin)
