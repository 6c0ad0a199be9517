"""GPU tests of --model metabaseline --fewshot_head ridge (fumi_amd/models/metabaseline.py): a training step
against the three engine calls made by hand, the optimizer's move of the ridge parameters, the forward form in few_shot,
--pretrain_metric ridge in Pretrain.few_shot, and a short CLI run.  Conv4 on 32 x 32 images, B = 2 episodes, 5-way, 2-shot, 2 queries
per class."""
import math

import numpy as np
import pytest
import torch

from helpers import rel_to_max

pytestmark = pytest.mark.gpu
B, N, K, Q, SIZE = 2, 5, 2, 2, 32
LAM, SCALE = 2.0, 3.0


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


def _model(dev):
    from fumi_amd.models.metabaseline import MetaBaseline
    torch.manual_seed(17)
    return MetaBaseline("conv4", image_size=SIZE, image_channels=3, num_ways=N, head="ridge", ridge_lambda=LAM, ridge_scale=SCALE).to(dev)


def _features(model, batch, dev, keep_tape):
    from fumi_amd import hip
    (_, _, x_s), y_s = batch["train"]
    (_, _, x_q), y_q = batch["test"]
    theta = [p.detach() for p in model.conv.theta()]
    f_s, f_q = hip.conv4_encode(hip.Workspace.get(dev, "encoder"), x_s, x_q, theta, keep_tape=keep_tape)
    return x_s, y_s, x_q, y_q, theta, f_s, f_q


def test_training_step_equals_the_three_engine_calls_by_hand(dev):
    from fumi_amd import hip
    model, batch = _model(dev), _batch(3, dev)
    loss, acc = model.evaluate(batch, None, None, dev, task="train")
    ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
    assert ws.read_status() == 0 and ws_enc.read_status() == 0
    flat = model._flat.flat.clone()
    got = [model.ridge.grad.clone()] + [p.grad.clone() for p in model.conv.theta()]
    x_s, y_s, x_q, y_q, theta, f_s, f_q = _features(model, batch, dev, True)
    out = hip.ridge_head_step(ws, f_s, y_s, f_q, y_q, model.ridge.detach(), need_grad=True, grad_scale=1.0, n_way=N)
    g_th = hip.conv4_encode_bwd(ws_enc, x_s, x_q, out["dfeats_s"], out["dfeats_q"], theta, scale=1.0)
    assert ws.read_status() == 0 and ws_enc.read_status() == 0
    assert float(loss) == float(out["loss"]) and float(acc) == float(out["correct"] / (B * N * Q))
    want = [out["dparams"]] + list(g_th)
    assert len(got) == len(want)
    for n, g, w in zip(["ridge"] + model.conv.theta_names("conv."), got, want):
        assert bool(torch.isfinite(g).all()), n
        assert torch.equal(g, w), n                                               # the same launches on the same inputs: the same bits
    # the flat buffer is [ridge | conv.* | loss, acc]
    by_hand = torch.cat([w.reshape(-1) for w in want] + [out["loss"], out["correct"] / (B * N * Q)])
    assert torch.equal(flat, by_hand)
    assert float(got[0].abs().min()) > 0.0


def test_adam_moves_the_ridge_parameters_by_the_rule_for_their_gradient(dev):
    from fumi_amd.optim import Adam
    model = _model(dev)
    kw = dict(lr=1e-2, weight_decay=5e-4)
    opt = Adam(params=model.parameters(), **kw)
    before = model.ridge.detach().clone()
    model.evaluate(_batch(7, dev), opt, None, dev, task="train")
    grad, after = model.ridge.grad.clone(), model.ridge.detach().clone()
    ref = before.clone().requires_grad_(True)
    ref.grad = grad
    torch.optim.Adam([ref], **kw).step()
    print(f"ridge {before.tolist()} -> {after.tolist()} (torch's Adam on the same gradient {grad.tolist()}: {ref.detach().tolist()})")
    assert bool((after != before).all())
    assert rel_to_max(after.cpu(), ref.detach().cpu()) <= 2e-7                    # tests/test_optim_fused_gpu.py: the bound on parameters


def test_few_shot_is_the_forward_form_and_pretrain_metric_ridge_is_one_forward_call(dev):
    from fumi_amd import hip
    from fumi_amd.models.pretrain import Pretrain
    model, batch = _model(dev).eval(), _batch(9, dev)
    ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
    with torch.no_grad():
        got = model.few_shot(batch, dev)
    x_s, y_s, x_q, y_q, theta, f_s, f_q = _features(model, batch, dev, False)
    params = torch.tensor([math.log(LAM), SCALE], device=dev)
    assert torch.equal(params, model.ridge.detach())
    out = hip.ridge_head_step(ws, f_s, y_s, f_q, y_q, params, need_grad=False, n_way=N)
    want = torch.cat((out["loss"], out["correct"] / (B * N * Q)))
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    torch.manual_seed(17)
    pre = Pretrain("conv4", image_size=SIZE, image_channels=3, n_classes=6, num_ways=N, metric="ridge", ridge_lambda=LAM,
                   ridge_scale=SCALE).to(dev).eval()
    pre.conv.load_state_dict(model.conv.state_dict())
    with torch.no_grad():
        got_p = pre.few_shot(batch, dev)
    assert torch.equal(got_p, want)
    assert ws.read_status() == 0 and ws_enc.read_status() == 0


def test_cli_metabaseline_with_the_ridge_head_finishes_with_a_finite_loss(dev, tmp_path, monkeypatch):
    from fumi_amd import hip
    from fumi_amd import main as cli
    monkeypatch.chdir(tmp_path)
    res = cli.main(cli.parse_args(["--model", "metabaseline", "--fewshot_head", "ridge", "--dataset", "synthetic-resident",
                                   "--im_encoder", "conv4", "--image_size", "32", "--synthetic_classes", "8", "--text_emb_dim", "32",
                                   "--batch_size", "2", "--num_ways", "5", "--num_shots", "2", "--num_shots_test", "2",
                                   "--num_ep_test", "4", "--epochs", "3", "--eval_freq", "2", "--lr", "1e-2",
                                   "--log_dir", str(tmp_path / "res"), "--wandb_offline"]))
    print(f"cli metabaseline ridge: test loss {res['test_loss']:.4f}, acc {res['test_acc']:.4f}")
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
