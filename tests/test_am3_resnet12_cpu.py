"""CPU suite: AM3 with the ResNet-12 backbone (--model am3 --im_encoder resnet12) -- module surface, evaluate(), checkpoints and the
CLI, with an oracle engine whose ResNet-12 encoder pair is oracle/resnet12_ref.features under autograd (the GPU engine's pair is
fumi_hip_resnet12_encode / _encode_bwd: tests/test_am3_resnet12_gpu.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import casegen as cg
from oracle import conv4_ref as CR
from oracle import resnet12_ref as RR
from oracle_engine import OracleEngine


class Rn12OracleEngine(OracleEngine):
    """OracleEngine + the ResNet-12 encoder pair (mirrors its Conv4 pair)."""

    def resnet12_encode(self, x_s, x_q, theta, keep_tape=False):
        with torch.no_grad():
            f_s = torch.stack([RR.features(x_s[b], theta) for b in range(x_s.shape[0])])
            f_q = torch.stack([RR.features(x_q[b], theta) for b in range(x_q.shape[0])])
        self._rn_tape = keep_tape
        self.encodes = getattr(self, "encodes", 0) + 1
        return f_s, f_q

    def resnet12_encode_bwd(self, x_s, x_q, dfeats_s, dfeats_q, theta_like, scale=1.0, g_theta=None):
        assert getattr(self, "_rn_tape", False), "resnet12_encode_bwd without a kept tape"
        self._rn_tape = False
        th = [t.detach().clone().requires_grad_(True) for t in theta_like]
        tot = 0.0
        for b in range(x_s.shape[0]):
            tot = tot + (RR.features(x_s[b], th) * dfeats_s[b]).sum() + (RR.features(x_q[b], th) * dfeats_q[b]).sum()
        gs = torch.autograd.grad(tot, th)
        if g_theta is None:
            g_theta = [torch.empty_like(t) for t in theta_like]
        for dst, g in zip(g_theta, gs):
            dst.copy_(g * scale)
        self.backwards = getattr(self, "backwards", 0) + 1
        return g_theta


@pytest.fixture
def rn_engine():
    from fumi_amd import engine
    eng = Rn12OracleEngine()
    old = engine.set_engine(eng)
    yield eng
    engine.set_engine(old)


def _model(**kw):
    from fumi_amd.models.am3 import AM3
    torch.manual_seed(0)
    return AM3(im_encoder="resnet12", im_emb_dim=0, text_encoder="BERT", text_emb_dim=12, text_hid_dim=8, prototype_dim=6,
               dropout=0.0, image_size=16, image_channels=3, **kw)


def test_am3_resnet12_builds_the_backbone(rn_engine):
    m = _model()
    assert m.conv.feature_dim == 640 and m.im_emb_dim == 640 and m.image_encoder.weight.shape == (6, 640)
    assert m.conv.channels == RR.CHANNELS and len(m.conv.theta()) == 48
    keys = set(m.state_dict())
    want = {f"conv.{k}" for k in m.conv.theta_names()} | {"image_encoder.weight", "image_encoder.bias", "g.0.weight", "g.3.bias",
                                                          "h.0.weight", "h.3.bias"}
    assert want <= keys
    assert {k for k in keys if k.startswith("conv.")} == {f"conv.{k}" for k in m.conv.theta_names()}


def test_am3_resnet12_trains_through_evaluate(rn_engine):
    """evaluate(train) runs encode (tape kept) -> AM3 step -> encode_bwd and gives every tensor a gradient: the ten AM3 tensors and
    the 48 backbone tensors all move; test returns the 11-tuple without a tape; forward(im_only=True) maps raw images."""
    m = _model()
    ep = CR.make_image_episodes(4, 2, 3, 2, 2, 3, 16, 16, 12)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    before = [p.detach().clone() for p in m.parameters()]
    out = m.evaluate(cg.to_batch(ep), opt, None, 3, torch.device("cpu"), "train")
    assert len(out) == 6 and np.isfinite(float(out[0]))
    assert rn_engine.encodes == 1 and rn_engine.backwards == 1
    changed = [not torch.equal(a, b.detach()) for a, b in zip(before, m.parameters())]
    assert all(changed), "every parameter receives a gradient (image encoder, g, h and the ResNet-12 backbone)"
    with torch.no_grad():
        r = m.evaluate(cg.to_batch(ep), None, None, 3, torch.device("cpu"), "test")
    assert len(r) == 11 and r[6].shape == (2, 6)
    assert rn_engine.encodes == 2 and rn_engine.backwards == 1 and not rn_engine._rn_tape
    im_emb = m([ep["idx_q"], None, ep["x_q"]], im_only=True)
    assert im_emb.shape == (2, 6, 6)
    th = [t.detach() for t in m.conv.theta()]
    ref = torch.nn.functional.linear(RR.features(ep["x_q"][1], th), m.image_encoder.weight.detach(), m.image_encoder.bias.detach())
    assert torch.allclose(im_emb[1], ref, atol=1e-5)


def test_am3_resnet12_checkpoint_round_trip(rn_engine, tmp_path):
    from fumi_amd.utils import utils
    m = _model()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    ep = CR.make_image_episodes(5, 2, 3, 2, 2, 3, 16, 16, 12)
    m.evaluate(cg.to_batch(ep), opt, None, 3, torch.device("cpu"), "train")
    f = str(tmp_path / "best.pth.tar")
    torch.save({"batch_idx": 0, "state_dict": m.state_dict(), "best_loss": 1.0, "optimizer": opt.state_dict()}, f)
    m2 = _model()
    opt2 = torch.optim.Adam(m2.parameters(), lr=1e-3)
    m2, opt2 = utils.load_checkpoint(m2, opt2, torch.device("cpu"), f)
    for (k, a), (k2, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    with torch.no_grad():
        r1 = m.evaluate(cg.to_batch(ep), None, None, 3, torch.device("cpu"), "test")
        r2 = m2.evaluate(cg.to_batch(ep), None, None, 3, torch.device("cpu"), "test")
    assert float(r1[0]) == float(r2[0])


def test_init_model_builds_am3_resnet12_from_flags(rn_engine):
    from fumi_amd import main as cli
    from fumi_amd.models.am3 import AM3
    from fumi_amd.utils import utils
    args = cli.parse_args(["--model", "am3", "--im_encoder", "resnet12", "--image_size", "16", "--image_channels", "1",
                           "--text_encoder", "BERT", "--text_emb_dim", "12", "--disable_cuda"])
    m = utils.init_model(args, None, watch=False)
    assert isinstance(m, AM3) and m.backbone == "resnet12"
    assert m.conv.image_size == 16 and m.conv.in_channels == 1 and m.image_encoder.in_features == 640
    help_ = [a.help for a in utils.parser()._actions if "--im_encoder" in a.option_strings][0]
    assert "resnet12" in help_ and "am3" in help_


def test_cli_am3_resnet12_plumbing_on_cpu(rn_engine, tmp_path, monkeypatch):
    """`main.py --model am3 --im_encoder resnet12` on CPU: flags -> image loader -> ResNet-12 -> AM3 training through the encoder
    pair -> checkpoint (backbone keys under conv.) -> best-checkpoint reload -> test."""
    from fumi_amd import main as cli
    monkeypatch.chdir(tmp_path)
    argv = ["--model", "am3", "--dataset", "synthetic", "--disable_cuda", "--im_encoder", "resnet12", "--image_size", "16",
            "--text_encoder", "BERT", "--text_emb_dim", "12", "--num_shots", "1", "--num_shots_test", "2", "--batch_size", "2",
            "--epochs", "1", "--eval_freq", "1", "--num_ep_test", "2", "--log_dir", str(tmp_path / "res"),
            "--synthetic_classes", "10"]
    args = cli.parse_args(argv)
    res = cli.main(args)
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    assert rn_engine.backwards >= 1
    runs = os.listdir(tmp_path / "res" / "runs")
    ck = torch.load(tmp_path / "res" / "runs" / runs[0] / "ckpt.pth.tar", weights_only=False)
    sd = ck["state_dict"]
    assert sd["conv.block0.conv1.weight"].shape == (64, 3, 3, 3) and sd["conv.block3.bns.bias"].shape == (640,)
    assert sd["image_encoder.weight"].shape[1] == 640
