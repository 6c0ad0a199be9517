"""GPU tests of the Meta-Baseline stage (--model metabaseline, fumi_amd/models/metabaseline.py): a training step
against the three engine calls made by hand, the optimizer's move of the temperature, --pretrain_metric in Pretrain.few_shot, and the
CLI from a classifier pre-training to the episodic stage (--encoder_checkpoint).  16 x 16 images, B = 2 episodes, 3-way, 2-shot,
4 queries per class."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_to_max

pytestmark = pytest.mark.gpu
B, N, K, Q, SIZE = 2, 3, 2, 4, 16


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


def _model(backbone, conv, dev, temp=10.0):
    """MetaBaseline with a shallower backbone than the CLI builds (the step reads the depth from the module)."""
    from fumi_amd.models.metabaseline import MetaBaseline
    torch.manual_seed(17)
    model = MetaBaseline(backbone, image_size=SIZE, image_channels=3, num_ways=N, init_temp=temp)
    model.conv = conv
    return model.to(dev)


def _by_hand(model, batch, encode, encode_bwd, dev):
    """encode -> cos_proto_step -> encode_bwd on the same batch: (head output, [dtau] + g_theta, the encoder plans seen)."""
    from fumi_amd import hip
    ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
    (_, _, x_s), y_s = batch["train"]
    (_, _, x_q), y_q = batch["test"]
    theta = [p.detach() for p in model.conv.theta()]
    f_s, f_q = encode(ws_enc, x_s, x_q, theta, keep_tape=True)
    out = hip.cos_proto_step(ws, f_s, y_s, f_q, y_q, model.temp.detach(), need_grad=True, grad_scale=1.0, n_way=N)
    g_th = encode_bwd(ws_enc, x_s, x_q, out["dfeats_s"], out["dfeats_q"], theta, scale=1.0)
    assert ws.read_status() == 0 and ws_enc.read_status() == 0
    return out, [out["dtau"]] + list(g_th)


def _check_step(model, batch, encode, encode_bwd, dev, plan=None):
    from fumi_amd import hip
    loss, acc = model.evaluate(batch, None, None, dev, task="train")
    plan_a = plan() if plan else None
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
    got = [model.temp.grad.clone()] + [p.grad.clone() for p in model.conv.theta()]
    out, want = _by_hand(model, batch, encode, encode_bwd, dev)
    plan_b = plan() if plan else None
    assert float(loss) == float(out["loss"]) and float(acc) == float(out["correct"] / (B * N * Q))
    names = ["temp"] + model.conv.theta_names("conv.")
    assert len(names) == len(got) == len(want)
    for n, g, w in zip(names, got, want):
        assert bool(torch.isfinite(g).all()), n
        if plan_a == plan_b:
            assert torch.equal(g, w), n                                           # the same launches on the same inputs: the same bits
        else:                                                                     # another encoder plan: the composition, 1e-2 of the
            e = rel_to_max(g.cpu(), w.cpu())                                      # tensor's scale (test_am3_conv4_step_matches_autograd)
            print(f"{n}: plans {plan_a} / {plan_b}, rel-to-max difference {e:.3e}")
            assert e <= 1e-2, (n, e)
    assert float(got[0].abs()) > 0.0
    return out


def test_conv4_training_step_equals_the_three_engine_calls_by_hand(dev):
    from fumi_amd import hip
    from fumi_amd.models.conv4 import Conv4
    model = _model("conv4", Conv4(3, 64, 2, SIZE), dev)
    _check_step(model, _batch(3, dev), hip.conv4_encode, hip.conv4_encode_bwd, dev)


def test_resnet12_training_step_equals_the_three_engine_calls_by_hand(dev):
    from fumi_amd import hip
    from fumi_amd.models.resnet12 import ResNet12
    model = _model("resnet12", ResNet12(3, (32, 32), SIZE), dev)
    _check_step(model, _batch(5, dev), hip.resnet12_encode, hip.resnet12_encode_bwd, dev, plan=hip.resnet12_encode_plan)


def test_adam_moves_the_temperature_by_the_rule_for_its_gradient(dev):
    from fumi_amd.models.conv4 import Conv4
    from fumi_amd.optim import Adam
    model = _model("conv4", Conv4(3, 64, 2, SIZE), dev, temp=8.0)
    kw = dict(lr=1e-2, weight_decay=5e-4)
    opt = Adam(params=model.parameters(), **kw)
    model.evaluate(_batch(7, dev), opt, None, dev, task="train")
    grad, after = model.temp.grad.clone(), model.temp.detach().clone()
    ref = torch.tensor([8.0], device=dev, requires_grad=True)
    ref.grad = grad
    torch.optim.Adam([ref], **kw).step()
    print(f"temp 8 -> {float(after):.8f} (torch's Adam on the same gradient {float(grad):.4e}: {float(ref.detach()):.8f})")
    assert float(after) != 8.0
    assert rel_to_max(after.cpu(), ref.detach().cpu()) <= 2e-7                    # tests/test_optim_fused_gpu.py: the bound on parameters


def test_pretrain_few_shot_metric_cosine_is_the_head_and_euclidean_is_unchanged(dev):
    from fumi_amd import hip
    from fumi_amd.models.conv4 import Conv4
    from fumi_amd.models.pretrain import Pretrain
    batch = _batch(9, dev)
    (_, _, x_s), y_s = batch["train"]
    (_, _, x_q), y_q = batch["test"]
    models = {}
    for metric in ("euclidean", "cosine"):
        torch.manual_seed(17)
        m = Pretrain("conv4", image_size=SIZE, image_channels=3, n_classes=6, num_ways=N, metric=metric, metric_temp=12.0)
        m.conv = Conv4(3, 64, 2, SIZE)
        models[metric] = m.to(dev).eval()
    models["cosine"].load_state_dict(models["euclidean"].state_dict())
    ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
    theta = [p.detach() for p in models["euclidean"].conv.theta()]
    f_s, f_q = hip.conv4_encode(ws_enc, x_s, x_q, theta, keep_tape=False)
    with torch.no_grad():
        got_e, got_c = models["euclidean"].few_shot(batch, dev), models["cosine"].few_shot(batch, dev)
    # euclidean: the torch expression few_shot has evaluated so far
    protos = hip.proto_reduce(ws, f_s, y_s, N)
    d2 = ((f_q[:, :, None, :] - protos[:, None, :, :]) ** 2).sum(-1)
    want_e = torch.stack((F.cross_entropy(-d2.reshape(-1, N), y_q.reshape(-1)), (d2.argmin(-1) == y_q).float().mean()))
    assert torch.equal(got_e, want_e)
    # cosine: the forward values of the head on the same features
    out = hip.cos_proto_step(ws, f_s, y_s, f_q, y_q, torch.tensor([12.0], device=dev), need_grad=False, n_way=N)
    assert torch.equal(got_c, torch.cat((out["loss"], out["correct"] / (B * N * Q))))
    assert ws.read_status() == 0 and ws_enc.read_status() == 0


def test_cli_pretrain_with_the_cosine_metric_then_metabaseline_from_its_checkpoint(dev, tmp_path, monkeypatch):
    from fumi_amd import hip
    from fumi_amd import main as cli
    from fumi_amd.models import metabaseline
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "synthetic-resident", "--im_encoder", "conv4", "--image_size", "16", "--synthetic_classes", "8",
              "--text_emb_dim", "32", "--batch_size", "2", "--num_ways", "3", "--num_shots", "2", "--num_shots_test", "4",
              "--num_ep_test", "4", "--lr", "1e-2", "--log_dir", str(tmp_path / "res"), "--wandb_offline"]
    res = cli.main(cli.parse_args(["--model", "pretrain", "--pretrain_batch", "16", "--pretrain_bn_group", "4", "--epochs", "3",
                                   "--eval_freq", "2", "--pretrain_metric", "cosine", "--metric_temp", "12"] + common))
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    run, = glob.glob(str(tmp_path / "res" / "runs" / "train-*"))
    best = os.path.join(run, "best.pth.tar")
    if not os.path.exists(best):                                                  # (no validation of the three steps beat the untrained one)
        best = os.path.join(run, "ckpt.pth.tar")
    seen = {}
    loop = metabaseline.test_loop

    def spy(a, model, *rest, **kw):
        seen["model"] = model
        return loop(a, model, *rest, **kw)
    monkeypatch.setattr(metabaseline, "test_loop", spy)
    res2 = cli.main(cli.parse_args(["--model", "metabaseline", "--encoder_checkpoint", best, "--epochs", "3", "--eval_freq", "2",
                                    "--metric_temp", "12"] + common))
    assert np.isfinite(res2["test_loss"]) and 0.0 <= res2["test_acc"] <= 1.0
    temp = float(seen["model"].temp.detach())
    print(f"cli metabaseline: test loss {res2['test_loss']:.4f}, acc {res2['test_acc']:.4f}, temp 12 -> {temp:.6f}")
    assert np.isfinite(temp) and temp != 12.0
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
    assert os.path.exists(best)
