"""GPU tests of --model pretrain with the cosine classifier (Pretrain(head="cosine")) on Conv4, 16 x 16 images,
C = 8 classes, M = 16 images in groups of R = 4: one training step against the kernels it is made of, a short descent, the fixed
scale, the checkpoint and its hand-over to the Meta-Baseline stage, and the linear head left as it was."""
import pytest
import torch

from helpers import rel_to_max

pytestmark = pytest.mark.gpu
M, R, C, SIZE = 16, 4, 8, 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _batch(seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, 3, SIZE, SIZE, generator=g).to(dev), torch.randint(0, C, (M,), generator=g).to(dev)


def _model(dev, seed=17, **kw):
    from fumi_amd.models.pretrain import Pretrain
    torch.manual_seed(seed)
    return Pretrain("conv4", image_size=SIZE, image_channels=3, n_classes=C, bn_group=R, **kw).to(dev)


@pytest.mark.parametrize("soft", [False, True])
def test_training_step_attaches_the_gradients_of_the_cosine_head(soft, dev):
    """classifier.weight.grad and cls_scale.grad are the gW and dtau of cos_cls_head_step on the features conv4_encode returns (the
    same kernel on the same inputs: the same bits); the backbone gradient is conv4_encode_bwd of its dfeats, compared at 1e-5 of each
    tensor's largest entry, which leaves room only for the order of a sum inside the encoder's backward."""
    from fumi_amd import hip
    model = _model(dev, head="cosine", head_scale=12.0, label_smoothing=0.1 if soft else 0.0)
    x, y = _batch(3, dev)
    kw = dict(y_b=y.flip(0), lam=0.3) if soft else {}
    out = model.train_step(x, y, **kw)
    ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
    assert ws.read_status() == 0 and ws_enc.read_status() == 0
    got_w, got_s = model.classifier.weight.grad.clone(), model.cls_scale.grad.clone()
    got_th = [p.grad.clone() for p in model.conv.theta()]
    loss = out["loss"].clone()
    B, half = M // (2 * R), M // 2
    theta = [p.detach() for p in model.conv.theta()]
    x_s, x_q = x[:half].view(B, R, 3, SIZE, SIZE), x[half:].view(B, R, 3, SIZE, SIZE)
    f_s, f_q = hip.conv4_encode(ws_enc, x_s, x_q, theta, keep_tape=True)
    feats = torch.cat((f_s.view(half, -1), f_q.view(half, -1)))
    head = hip.cos_cls_head_step(ws, feats, y, model.classifier.weight.detach(), model.cls_scale.detach(), need_grad=True,
                                 smoothing=0.1 if soft else 0.0, **kw)
    dfe = head["dfeats"]
    g_th = hip.conv4_encode_bwd(ws_enc, x_s, x_q, dfe[:half].view(B, R, -1).contiguous(), dfe[half:].view(B, R, -1).contiguous(), theta)
    assert ws.read_status() == 0 and ws_enc.read_status() == 0
    assert torch.equal(loss, head["loss"]) and torch.equal(got_w, head["gW"]) and torch.equal(got_s, head["dtau"])
    assert float(got_w.abs().max()) > 0 and float(got_s.abs().max()) > 0
    assert model.classifier.bias is None and float(model.cls_scale.detach()) == 12.0
    for n, g, r in zip(model.conv.theta_names("conv."), got_th, g_th):
        e = rel_to_max(g.cpu(), r.cpu())
        print(f"{n}: rel-to-max difference {e:.3e}")
        assert e <= 1e-5, (n, e)


def test_ten_sgd_steps_lower_the_loss_and_move_the_scale(dev):
    model = _model(dev, head="cosine")
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    assert any(p is model.cls_scale for g in opt.param_groups for p in g["params"])
    x, y = _batch(5, dev)
    losses = [float(model.train_step(x, y, opt)["loss"]) for _ in range(10)]
    print("cosine head, ten SGD steps:", [round(v, 4) for v in losses], "cls_scale", float(model.cls_scale.detach()))
    assert all(v == v for v in losses) and losses[-1] < losses[0]
    assert float(model.cls_scale.detach()) != 10.0


def test_a_fixed_scale_is_no_parameter_and_stays_where_it_is(dev):
    model = _model(dev, head="cosine", head_scale=16.0, head_scale_fixed=True)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    assert not any(p is model.cls_scale for g in opt.param_groups for p in g["params"])
    assert "cls_scale" in model.state_dict() and "cls_scale" not in dict(model.named_parameters())
    x, y = _batch(5, dev)
    w0 = model.classifier.weight.detach().clone()
    first = float(model.train_step(x, y, opt)["loss"])
    assert model.cls_scale.tolist() == [16.0] and not torch.equal(model.classifier.weight.detach(), w0)
    learned = _model(dev, head="cosine", head_scale=16.0)
    assert float(learned.train_step(x, y)["loss"]) == first                      # the same step, the scale from a buffer
    assert torch.equal(learned.classifier.weight.grad, model.classifier.weight.grad)


def test_checkpoint_round_trip_and_hand_over_to_the_meta_baseline_stage(dev, tmp_path):
    from fumi_amd.models.metabaseline import MetaBaseline
    from fumi_amd.utils import utils
    model = _model(dev, head="cosine")
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    x, y = _batch(7, dev)
    model.train_step(x, y, opt)
    path = str(tmp_path / "cosine.pth.tar")
    torch.save({"batch_idx": 0, "state_dict": model.state_dict(), "best_loss": 0.0, "optimizer": opt.state_dict()}, path)
    fresh = _model(dev, seed=99, head="cosine")
    fresh, _ = utils.load_checkpoint(fresh, torch.optim.SGD(fresh.parameters(), lr=0.05), dev, path)
    assert list(fresh.state_dict()) == list(model.state_dict())
    for k, v in model.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v), k
    assert float(fresh.train_step(x, y)["loss"]) == float(model.train_step(x, y)["loss"])
    # --encoder_checkpoint reads conv.* alone: the classifier without a bias and cls_scale are ignored
    torch.manual_seed(1)
    meta = MetaBaseline("conv4", image_size=SIZE).to(dev)
    temp = meta.temp.detach().clone()
    utils.load_encoder_checkpoint(meta, dev, path)
    sd = model.state_dict()
    mine = meta.conv.state_dict()
    assert set("conv." + k for k in mine) == {k for k in sd if k.startswith("conv.")}
    for k, v in mine.items():
        assert torch.equal(v, sd["conv." + k]), k
    assert torch.equal(meta.temp.detach(), temp) and "cls_scale" not in meta.state_dict()


def test_the_linear_head_is_the_model_it_was(dev):
    """head="linear" against Pretrain built without the argument, the same seed: the same state_dict and, after two steps with the
    soft target in the second, the same bits in the loss and in every gradient."""
    a, b = _model(dev), _model(dev, head="linear")
    assert list(a.state_dict()) == list(b.state_dict())
    for k, v in a.state_dict().items():
        assert torch.equal(b.state_dict()[k], v), k
    x, y = _batch(11, dev)
    for kw in ({}, dict(y_b=y.flip(0), lam=0.7)):
        la, lb = a.train_step(x, y, **kw)["loss"].clone(), b.train_step(x, y, **kw)["loss"].clone()
        assert torch.equal(la, lb)
        for (n, p), q in zip(a.named_parameters(), b.parameters()):
            assert torch.equal(p.grad, q.grad), n
