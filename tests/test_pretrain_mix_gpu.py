"""GPU tests of --label_smoothing / --mixup_alpha / --cutmix_alpha / --mix_prob for --model pretrain, end to end
on the 16 x 16 synthetic resident pixel table with Conv4 (fp32), M = 16, R = 4: the defaults change no bit, the batch fed to a mixed
step is the reference blend of the unmixed gather, its published loss is the float64 soft-target loss of its features, and a run
through the command line finishes clean."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import image_mix_ref as MR
from cls_head_soft_ref import cls_head_soft_ref

pytestmark = pytest.mark.gpu

COMMON = ["--model", "pretrain", "--dataset", "synthetic-resident", "--im_encoder", "conv4", "--image_size", "16",
          "--synthetic_classes", "8", "--text_emb_dim", "32", "--batch_size", "4", "--num_ways", "5", "--num_shots", "5",
          "--num_ep_test", "8", "--pretrain_batch", "16", "--pretrain_bn_group", "4", "--augment", "--augment_pad", "1",
          "--augment_jitter", "0.1", "--wandb_offline"]
MIX = ["--label_smoothing", "0.1", "--mixup_alpha", "0.4", "--cutmix_alpha", "1.0"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _setup(extra):
    """(args, the supervised train source, the model init_model builds for them)."""
    from fumi_amd import main as cli
    from fumi_amd.utils import utils
    args = cli.parse_args(COMMON + extra)
    cli.check_supported(args)
    train = cli.get_dataset(args)[0]
    args.n_classes = int(train.n_classes)
    torch.manual_seed(args.seed)
    return args, train, utils.init_model(args, None, watch=False)


def test_default_flags_change_no_bit_of_three_steps(dev):
    from fumi_amd import hip
    from fumi_amd.models.pretrain import Pretrain
    from fumi_amd.utils import utils
    args, train, model = _setup([])
    assert train.mix is None and model.label_smoothing == 0.0
    torch.manual_seed(args.seed)
    plain = Pretrain(im_encoder="conv4", image_size=16, image_channels=3, n_classes=args.n_classes, bn_group=4, num_ways=5).to(dev)
    for (n, p), (_, q) in zip(model.named_parameters(), plain.named_parameters()):
        assert torch.equal(p, q), n
    opt_a, opt_b = utils.init_optim(args, model), utils.init_optim(args, plain)
    for step in range(3):
        batch = train.batch(step)
        assert len(batch) == 2
        la = [float(v) for v in model.evaluate(batch, opt_a, None, dev, task="train")]
        lb = [float(v) for v in plain.evaluate(train.batch(step), opt_b, None, dev, task="train")]
        assert la == lb and np.isfinite(la).all()
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
    for (n, p), (_, q) in zip(model.named_parameters(), plain.named_parameters()):
        assert torch.equal(p, q), n


def test_mixed_step_feeds_the_reference_blend_and_publishes_the_soft_loss(dev):
    from fumi_amd import hip
    from fumi_amd.dataset.supervised_pixels import CUTMIX, MIXUP, mix_draw
    args, train, model = _setup(MIX)
    assert train.mix == dict(mixup_alpha=0.4, cutmix_alpha=1.0, prob=1.0) and model.label_smoothing == 0.1
    M, R = 16, 4
    steps = {}
    for step in range(64):                                                 # the first step of each mode
        steps.setdefault(mix_draw(train.seed, step, M, 16, 16, **train.mix)[0], step)
    assert set(steps) == {MIXUP, CUTMIX}
    ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
    theta = [p.detach() for p in model.conv.theta()]
    W, b = model.classifier.weight.detach().cpu().numpy(), model.classifier.bias.detach().cpu().numpy()
    for mode, step in sorted(steps.items()):
        _, lam, box, partner = mix_draw(train.seed, step, M, 16, 16, **train.mix)
        plain, y = train.gather(step)
        x, y_a, y_b, lam_fed = train.batch(step)
        assert lam_fed == lam and torch.equal(y_a, y) and torch.equal(y_b, y[torch.from_numpy(partner).to(dev)])
        ref = MR.mix_images(plain.cpu().numpy(), partner, mode, lam=lam, box=box)
        if mode == CUTMIX:
            assert np.array_equal(x.cpu().numpy(), ref.astype(np.float32))
        else:
            a = np.abs(plain.cpu().numpy())
            assert bool((np.abs(x.cpu().numpy() - ref) <= 4 * 2.0 ** -24 * np.maximum(a, a[partner])).all())
        B, half = M // (2 * R), M // 2
        f_s, f_q = hip.conv4_encode(ws_enc, x[:half].view(B, R, 3, 16, 16), x[half:].view(B, R, 3, 16, 16), theta, keep_tape=False)
        feats = torch.cat((f_s.view(half, -1), f_q.view(half, -1))).cpu().numpy()
        want = cls_head_soft_ref(feats, y_a.cpu().numpy(), W, b, y_b=y_b.cpu().numpy(), lam=lam, smoothing=0.1)
        out = model.train_step(x, y_a, y_b=y_b, lam=lam_fed)               # no optimizer: the parameters stay
        assert ws.read_status() == 0 and ws_enc.read_status() == 0
        got = float(out["loss"])
        print(f"mode {mode} step {step} lam {lam:.4f} box {box}: loss {got:.6f}, float64 {want['loss']:.6f}")
        assert abs(got - want["loss"]) <= 1e-4 * max(abs(want["loss"]), 1e-5)
        assert abs(float(out["correct"]) - want["correct"]) <= int((want["margin"] <= 1e-5).sum())
        for n, p in model.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n


def test_cli_run_with_the_three_options_finishes_clean(dev, tmp_path, monkeypatch):
    from fumi_amd import hip
    from fumi_amd import main as cli
    monkeypatch.chdir(tmp_path)
    res = cli.main(cli.parse_args(COMMON + MIX + ["--epochs", "23", "--eval_freq", "12", "--lr", "2e-3", "--max_grad_norm", "1",
                                                  "--log_dir", str(tmp_path / "res")]))
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    run, = glob.glob(str(tmp_path / "res" / "runs" / "train-*"))
    recs = [json.loads(l) for l in open(os.path.join(run, "metrics.jsonl"))]
    train = [r["train/loss"] for r in recs if "train/loss" in r]
    print(f"cli pretrain with smoothing, mixup and CutMix: {len(train)} steps, train/loss first {train[0]:.4f} last {train[-1]:.4f}")
    assert len(train) >= 24 and bool(np.isfinite(train).all())
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
