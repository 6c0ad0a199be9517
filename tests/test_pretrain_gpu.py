"""GPU tests of supervised backbone pre-training (--model pretrain, fumi_amd/models/pretrain.py): one training
step against the composition of the existing ops, the same step on the bf16 ResNet-12, and the CLI end to end including the
hand-over of the backbone to AM3 (--encoder_checkpoint)."""
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from cls_head_ref import cls_head_ref
from helpers import rel_to_max

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _batch(seed, M, C, size, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, 3, size, size, generator=g).to(dev), torch.randint(0, C, (M,), generator=g).to(dev)


def _model(backbone, conv, C, R, dev):
    """Pretrain with a shallower backbone than the CLI builds (the step reads the depth from the module)."""
    from fumi_amd.models.pretrain import Pretrain
    torch.manual_seed(17)
    model = Pretrain(backbone, image_size=16, image_channels=3, n_classes=C, bn_group=R)
    model.conv = conv
    model.classifier = nn.Linear(conv.feature_dim, C)
    return model.to(dev)


def test_conv4_training_step_equals_the_composition_of_the_unit_ops(dev):
    """Encoder gradients, gW and gb of one step (16 x 16 images, 2 blocks, M = 16, R = 4, C = 6) against conv4_encode -> linear_fwd /
    ce_fwd_bwd / linear_bwd_data / linear_bwd_weight -> conv4_encode_bwd on the same batch, at the tolerance tests/test_conv4_gpu.py
    applies to parameter gradients (1e-2 of the tensor's scale, test_am3_conv4_step_matches_autograd there)."""
    from fumi_amd import hip
    from fumi_amd.models.conv4 import Conv4
    M, R, C = 16, 4, 6
    model = _model("conv4", Conv4(3, 64, 2, 16), C, R, dev)
    x, y = _batch(3, M, C, 16, dev)
    out = model.train_step(x, y)
    ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
    assert ws.read_status() == 0 and ws_enc.read_status() == 0
    got = [model.classifier.weight.grad.clone(), model.classifier.bias.grad.clone()] + [p.grad.clone() for p in model.conv.theta()]
    # the composition
    B, half = M // (2 * R), M // 2
    theta = [p.detach() for p in model.conv.theta()]
    W, b = model.classifier.weight.detach(), model.classifier.bias.detach()
    x_s, x_q = x[:half].view(B, R, 3, 16, 16), x[half:].view(B, R, 3, 16, 16)
    f_s, f_q = hip.conv4_encode(ws_enc, x_s, x_q, theta, keep_tape=True)
    feats = torch.cat((f_s.view(half, -1), f_q.view(half, -1)))
    loss, dz, _ = hip.ce_fwd_bwd(ws, hip.linear_fwd(ws, feats, W, b), y)
    dfe = hip.linear_bwd_data(ws, dz, W)
    gW, gb = hip.linear_bwd_weight(ws, dz, feats)
    g_th = hip.conv4_encode_bwd(ws_enc, x_s, x_q, dfe[:half].view(B, R, -1).contiguous(), dfe[half:].view(B, R, -1).contiguous(), theta)
    assert ws.read_status() == 0 and ws_enc.read_status() == 0
    assert abs(float(out["loss"]) - float(loss)) <= 1e-4 * max(1.0, abs(float(loss)))
    names = ["classifier.weight", "classifier.bias"] + model.conv.theta_names("conv.")
    for n, g, r in zip(names, got, [gW, gb] + list(g_th)):
        e = rel_to_max(g.cpu(), r.cpu())
        print(f"{n}: rel-to-max difference {e:.3e}")
        assert e <= 1e-2, (n, e)


def test_resnet12_training_step_runs_and_its_loss_is_the_head_loss_of_its_features(dev):
    """The same step with the bf16 ResNet-12 (16 x 16 images, channels 32/32, M = 16): status 0, finite gradients, and the loss is the
    float64 head loss of the features resnet12_encode returns (1e-4, tests/test_hip_parity.py:18)."""
    from fumi_amd import hip
    from fumi_amd.models.resnet12 import ResNet12
    M, R, C = 16, 4, 6
    model = _model("resnet12", ResNet12(3, (32, 32), 16), C, R, dev)
    x, y = _batch(5, M, C, 16, dev)
    ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
    B, half = M // (2 * R), M // 2
    f_s, f_q = hip.resnet12_encode(ws_enc, x[:half].view(B, R, 3, 16, 16), x[half:].view(B, R, 3, 16, 16),
                                   [p.detach() for p in model.conv.theta()], keep_tape=False)
    feats = torch.cat((f_s.view(half, -1), f_q.view(half, -1))).cpu()
    out = model.train_step(x, y)
    assert ws.read_status() == 0 and ws_enc.read_status() == 0
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    ref = cls_head_ref(feats.numpy(), y.cpu().numpy(), model.classifier.weight.detach().cpu().numpy(),
                       model.classifier.bias.detach().cpu().numpy())
    assert abs(float(out["loss"]) - ref["loss"]) <= 1e-4 * max(abs(ref["loss"]), 1e-5)


def _held_out_train_class_episodes(args, shots, queries, n_batches):
    """Episodic meta-batches over FRESH images of the training classes: the train split's class prototypes (synthetic.py: a function of
    the seed and the split) with noise the run never saw, normalised by the train table's statistics like every split of the run."""
    from fumi_amd.dataset.gpu_sampler import GpuEpisodeSampler
    from fumi_amd.dataset.synthetic import SyntheticEpisodes, image_normalization, synthetic_pixel_table
    shape = (args.image_channels, args.image_size, args.image_size)
    base = SyntheticEpisodes(args.synthetic_classes, args.im_emb_dim, args.text_emb_dim, args.num_ways, args.num_shots, 1,
                             args.batch_size, args.seed, "train", None, image_shape=shape)
    per = max(48, args.num_shots + max(args.num_shots_test, int(100 / args.num_ways)))          # get_synthetic_resident's table
    seen, _ = synthetic_pixel_table(base, per, np.random.RandomState(args.seed * 13 + len("train")))
    norm = image_normalization(args, torch.from_numpy(seen).to(args.device))
    fresh, coi = synthetic_pixel_table(base, shots + queries, np.random.RandomState(991))
    assert not np.array_equal(fresh[:8], seen[:8])
    sampler = GpuEpisodeSampler(torch.from_numpy(fresh).to(args.device), coi, torch.from_numpy(base.text), args.num_ways, shots,
                                queries, args.batch_size, seed=77, normalize=norm)
    return [sampler.batch(i) for i in range(n_batches)]


def _few_shot_accuracy(model, batches, device):
    model.eval()
    with torch.no_grad():
        return float(torch.stack([model.few_shot(b, device) for b in batches]).mean(0)[1])


def test_cli_pretrain_then_am3_with_the_pretrained_backbone(dev, tmp_path, monkeypatch):
    """`--model pretrain` on the synthetic resident pixel table with --augment and --max_grad_norm 1, six dozen steps:
      * the training loss at the end is below the loss at step 0;
      * the few-shot validation accuracy is above chance + 10 points at EVERY validation point, the last included;
      * training raises the few-shot accuracy on held-out images of the training classes, the thing pre-training can help here: the
        validation classes are other white-noise patterns than the training classes, so fitting the training patterns does not
        carry over to them (their accuracy falls during the run, see the log below) -- the trained backbone (ckpt.pth.tar, the last
        step) must beat an untrained one by more than 0.05 on 20 episodes x 100 queries of fresh images: a binomial standard error of
        at most 0.0112 per figure, 0.016 for the difference, three of them;
      * then `--model am3 --encoder_checkpoint best.pth.tar --evaluate` runs with exactly the checkpoint's backbone.
    The synthetic prototypes are white-noise patterns of 0.14 pixel-scale standard deviation: the default colour jitter (0.4: a brightness
    shift of up to 1.4 standard deviations per image) buries them, so the run uses --augment_jitter 0.1 and a one-pixel crop; 25 shots keep
    the centroid noise of the 64-dimensional 16 x 16 features below the class distances.  The figures of a run are printed and kept in
    profiles/pretrain/gpu_tests.log."""
    from fumi_amd import main as cli
    from fumi_amd.models import am3
    from fumi_amd.utils import utils
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "synthetic-resident", "--im_encoder", "conv4", "--image_size", "16", "--synthetic_classes", "8",
              "--text_emb_dim", "32", "--batch_size", "4", "--num_ways", "5", "--num_shots", "25", "--num_ep_test", "32",
              "--log_dir", str(tmp_path / "res"), "--wandb_offline"]
    args = cli.parse_args(["--model", "pretrain", "--pretrain_batch", "16", "--pretrain_bn_group", "4", "--epochs", "71",
                           "--eval_freq", "35", "--lr", "2e-3", "--augment", "--augment_pad", "1", "--augment_jitter", "0.1",
                           "--max_grad_norm", "1"] + common)
    assert args.device.type == "cuda"
    res = cli.main(args)
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    run, = glob.glob(str(tmp_path / "res" / "runs" / "train-*"))
    recs = [json.loads(l) for l in open(os.path.join(run, "metrics.jsonl"))]
    train = [r["train/loss"] for r in recs if "train/loss" in r]
    val = [(r["_step"], r["val/loss"], r["val/acc"]) for r in recs if "val/acc" in r]
    print(f"cli pretrain: train/loss first {train[0]:.4f} last {train[-1]:.4f} over {len(train)} steps; "
          f"val (step, loss, acc) {[(s, round(l, 4), round(a, 4)) for s, l, a in val]}")
    assert len(train) >= 24 and train[-1] < train[0]
    assert len(val) == 3 and val[-1][0] == 70
    for step, _, acc in val:
        assert acc > 1.0 / 5 + 0.10, (step, acc)
    # what the training is good for: few-shot episodes over fresh images of the training classes
    episodes = _held_out_train_class_episodes(args, 25, 20, 5)
    torch.manual_seed(args.seed)
    untrained = utils.init_model(args, None, watch=False)
    trained = utils.init_model(args, None, watch=False)
    last = torch.load(os.path.join(run, "ckpt.pth.tar"), map_location=dev, weights_only=False)
    assert last["batch_idx"] == 70
    trained.load_state_dict(last["state_dict"])
    a0, a1 = _few_shot_accuracy(untrained, episodes, dev), _few_shot_accuracy(trained, episodes, dev)
    print(f"cli pretrain: few-shot accuracy on held-out images of the training classes: untrained {a0:.4f}, after 71 steps {a1:.4f}")
    assert a1 > a0 + 0.05
    best = os.path.join(run, "best.pth.tar")
    assert os.path.exists(best)
    # the backbone carried into AM3
    seen = {}
    loop = am3.test_loop

    def spy(a, model, *rest, **kw):
        seen["model"] = model
        return loop(a, model, *rest, **kw)
    monkeypatch.setattr(am3, "test_loop", spy)
    res2 = cli.main(cli.parse_args(["--model", "am3", "--encoder_checkpoint", best, "--evaluate", "--dropout", "0"] + common))
    assert np.isfinite(res2["test_loss"]) and 0.0 <= res2["test_acc"] <= 1.0
    sd = torch.load(best, map_location="cpu", weights_only=False)["state_dict"]
    mine = seen["model"].conv.state_dict()
    assert len(mine) == 12 and set("conv." + k for k in mine) == {k for k in sd if k.startswith("conv.")}
    for k, v in mine.items():
        assert torch.equal(v.cpu(), sd["conv." + k]), k
