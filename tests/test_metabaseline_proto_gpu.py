"""GPU tests of --model metabaseline --fewshot_head proto (fumi_amd/models/metabaseline.py): a training step against
the three engine calls made by hand, the optimizer's move of a learned scale, a fixed scale that no optimizer step moves, the forward form
in few_shot, and short CLI runs in both scale modes.  Conv4 on 16 x 16 images (64 features), B = 2 episodes, 3-way, 2-shot, 2 queries
per class."""
import numpy as np
import pytest
import torch

from helpers import rel_to_max

pytestmark = pytest.mark.gpu
B, N, K, Q, SIZE = 2, 3, 2, 2, 16
SCALE = 0.05


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _batch(seed, dev):
    """An episodic meta-batch in the format of the pixel samplers: batch['train'] = ((_, _, images), labels), batch['test'] likewise."""
    g = torch.Generator().manual_seed(seed)
    y_s = torch.stack([(torch.arange(N * K) % N)[torch.randperm(N * K, generator=g)] for _ in range(B)])
    y_q = torch.stack([(torch.arange(N * Q) % N)[torch.randperm(N * Q, generator=g)] for _ in range(B)])
    x_s, x_q = torch.randn(B, N * K, 3, SIZE, SIZE, generator=g), torch.randn(B, N * Q, 3, SIZE, SIZE, generator=g)
    return {"train": ((None, None, x_s.to(dev)), y_s.to(dev)), "test": ((None, None, x_q.to(dev)), y_q.to(dev))}


def _model(dev, fixed=False):
    from fumi_amd.models.metabaseline import MetaBaseline
    torch.manual_seed(17)
    return MetaBaseline("conv4", image_size=SIZE, image_channels=3, num_ways=N, head="proto", proto_scale=SCALE,
                        proto_scale_fixed=fixed).to(dev)


def _features(model, batch, dev, keep_tape):
    from fumi_amd import hip
    (_, _, x_s), y_s = batch["train"]
    (_, _, x_q), y_q = batch["test"]
    theta = [p.detach() for p in model.conv.theta()]
    f_s, f_q = hip.conv4_encode(hip.Workspace.get(dev, "encoder"), x_s, x_q, theta, keep_tape=keep_tape)
    return x_s, y_s, x_q, y_q, theta, f_s, f_q


@pytest.mark.parametrize("fixed", [False, True])
def test_training_step_equals_the_three_engine_calls_by_hand(fixed, dev):
    from fumi_amd import hip
    model, batch = _model(dev, fixed), _batch(3, dev)
    loss, acc = model.evaluate(batch, None, None, dev, task="train")
    ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
    assert ws.read_status() == 0 and ws_enc.read_status() == 0
    flat = model._flat.flat.clone()
    own = [] if fixed else [model.proto_scale.grad.clone()]
    got = own + [p.grad.clone() for p in model.conv.theta()]
    d_fixed = model._dscale.clone() if fixed else None
    x_s, y_s, x_q, y_q, theta, f_s, f_q = _features(model, batch, dev, True)
    assert f_s.shape[-1] == 64
    out = hip.euclid_proto_step(ws, f_s, y_s, f_q, y_q, model.proto_scale.detach(), need_grad=True, grad_scale=1.0, n_way=N)
    g_th = hip.conv4_encode_bwd(ws_enc, x_s, x_q, out["dfeats_s"], out["dfeats_q"], theta, scale=1.0)
    assert ws.read_status() == 0 and ws_enc.read_status() == 0
    assert float(loss) == float(out["loss"]) and float(acc) == float(out["correct"] / (B * N * Q))
    want = ([] if fixed else [out["dalpha"]]) + list(g_th)
    assert len(got) == len(want)
    for n, g, w in zip(([] if fixed else ["proto_scale"]) + model.conv.theta_names("conv."), got, want):
        assert bool(torch.isfinite(g).all()), n
        assert torch.equal(g, w), n                                               # the same launches on the same inputs: the same bits
    # the flat buffer is [proto_scale | conv.* | loss, acc], without the first where the scale is fixed
    by_hand = torch.cat([w.reshape(-1) for w in want] + [out["loss"], out["correct"] / (B * N * Q)])
    assert torch.equal(flat, by_hand)
    assert float(out["dalpha"].abs()) > 0.0
    if fixed:
        assert torch.equal(d_fixed, out["dalpha"])                                # written beside the buffer
        assert "proto_scale" not in dict(model.named_parameters()) and model.proto_scale.grad is None


def test_adam_moves_a_learned_scale_by_the_rule_for_its_gradient(dev):
    from fumi_amd.optim import Adam
    model = _model(dev)
    kw = dict(lr=1e-2, weight_decay=5e-4)
    opt = Adam(params=model.parameters(), **kw)
    before = model.proto_scale.detach().clone()
    model.evaluate(_batch(7, dev), opt, None, dev, task="train")
    grad, after = model.proto_scale.grad.clone(), model.proto_scale.detach().clone()
    ref = before.clone().requires_grad_(True)
    ref.grad = grad
    torch.optim.Adam([ref], **kw).step()
    print(f"proto_scale {before.tolist()} -> {after.tolist()} (torch's Adam on the same gradient {grad.tolist()}: {ref.detach().tolist()})")
    assert bool((after != before).all())
    assert rel_to_max(after.cpu(), ref.detach().cpu()) <= 2e-7                    # tests/test_optim_fused_gpu.py: the bound on parameters


def test_a_fixed_scale_is_bit_equal_after_three_adamw_steps_with_weight_decay(dev):
    from fumi_amd.optim import AdamW
    model = _model(dev, fixed=True)
    opt = AdamW(params=model.parameters(), lr=1e-2, weight_decay=0.1)
    assert all(p is not model.proto_scale for grp in opt.param_groups for p in grp["params"])
    before = model.proto_scale.clone()
    conv_before = [p.detach().clone() for p in model.conv.theta()]
    for step in range(3):
        loss, _ = model.evaluate(_batch(20 + step, dev), opt, None, dev, task="train")
        assert np.isfinite(float(loss))
    assert torch.equal(model.proto_scale, before) and float(before) == np.float32(SCALE)
    assert torch.equal(model.state_dict()["proto_scale"], before)
    assert all(not torch.equal(p.detach(), q) for p, q in zip(model.conv.theta(), conv_before))    # the backbone moves


@pytest.mark.parametrize("fixed", [False, True])
def test_few_shot_is_the_forward_form(fixed, dev):
    from fumi_amd import hip
    model, batch = _model(dev, fixed).eval(), _batch(9, dev)
    ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
    with torch.no_grad():
        got = model.few_shot(batch, dev)
    x_s, y_s, x_q, y_q, theta, f_s, f_q = _features(model, batch, dev, False)
    alpha = torch.tensor([SCALE], device=dev)
    assert torch.equal(alpha, model.proto_scale.detach())
    out = hip.euclid_proto_step(ws, f_s, y_s, f_q, y_q, alpha, need_grad=False, n_way=N)
    assert out["dfeats_s"] is None and out["dalpha"] is None
    want = torch.cat((out["loss"], out["correct"] / (B * N * Q)))
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    assert ws.read_status() == 0 and ws_enc.read_status() == 0


@pytest.mark.parametrize("fixed", [False, True])
def test_cli_metabaseline_with_the_proto_head_finishes_with_a_finite_loss_and_a_checkpoint(fixed, dev, tmp_path, monkeypatch):
    import glob
    import os
    from fumi_amd import hip
    from fumi_amd import main as cli
    monkeypatch.chdir(tmp_path)
    res = cli.main(cli.parse_args(["--model", "metabaseline", "--fewshot_head", "proto", "--dataset", "synthetic-resident",
                                   "--im_encoder", "conv4", "--image_size", "16", "--synthetic_classes", "8", "--text_emb_dim", "32",
                                   "--batch_size", "2", "--num_ways", "3", "--num_shots", "2", "--num_shots_test", "2",
                                   "--num_ep_test", "4", "--epochs", "3", "--eval_freq", "2", "--lr", "1e-2", "--proto_scale", "0.05",
                                   "--log_dir", str(tmp_path / "res"), "--wandb_offline"] + (["--proto_scale_fixed"] if fixed else [])))
    print(f"cli metabaseline proto{' fixed' if fixed else ''}: test loss {res['test_loss']:.4f}, acc {res['test_acc']:.4f}")
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
    ckpts = glob.glob(os.path.join(str(tmp_path), "**", "*.pth.tar"), recursive=True)
    assert ckpts
    for path in ckpts:
        sd = torch.load(path, map_location="cpu", weights_only=False)["state_dict"]
        assert tuple(sd["proto_scale"].shape) == (1,) and any(k.startswith("conv.") for k in sd)
        if fixed:
            assert float(sd["proto_scale"]) == np.float32(0.05)
