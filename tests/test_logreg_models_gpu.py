"""GPU tests of the logistic-regression head in the models: Pretrain(metric="logreg").few_shot and
MetaBaseline(eval_head="logreg").few_shot against the encode call and the head call made by hand, a training step of MetaBaseline that
does not depend on the evaluation head, and a short CLI run.  Conv4 on 16 x 16 images, B = 2 episodes, 3-way, 2-shot, Qn = 5."""
import glob
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
B, N, K, QN, SIZE = 2, 3, 2, 5, 16
CFG = dict(steps=40, lr=0.5, momentum=0.8, C=2.0, normalize=True)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _batch(seed, dev):
    """An episodic meta-batch in the format of the pixel samplers: batch['train'] = ((_, _, images), labels), batch['test'] likewise."""
    g = torch.Generator().manual_seed(seed)
    y_s = torch.stack([(torch.arange(N * K) % N)[torch.randperm(N * K, generator=g)] for _ in range(B)])
    y_q = torch.randint(0, N, (B, QN), generator=g)
    x_s, x_q = torch.randn(B, N * K, 3, SIZE, SIZE, generator=g), torch.randn(B, QN, 3, SIZE, SIZE, generator=g)
    return {"train": ((None, None, x_s.to(dev)), y_s.to(dev)), "test": ((None, None, x_q.to(dev)), y_q.to(dev))}


def _meta(dev, eval_head):
    from fumi_amd.models.metabaseline import MetaBaseline
    torch.manual_seed(17)
    return MetaBaseline("conv4", image_size=SIZE, image_channels=3, num_ways=N, eval_head=eval_head, logreg=CFG).to(dev)


def _by_hand(model, batch, dev):
    from fumi_amd import hip
    (_, _, x_s), y_s = batch["train"]
    (_, _, x_q), y_q = batch["test"]
    theta = [p.detach() for p in model.conv.theta()]
    f_s, f_q = hip.conv4_encode(hip.Workspace.get(dev, "encoder"), x_s, x_q, theta, keep_tape=False)
    out = hip.logreg_head_step(hip.Workspace.get(dev), f_s, y_s, f_q, y_q, n_way=N, **CFG)
    return torch.cat((out["loss"], out["correct"] / (B * QN)))


def test_few_shot_of_both_models_is_the_encode_call_and_the_head_call(dev):
    from fumi_amd import hip
    from fumi_amd.models.pretrain import Pretrain
    batch = _batch(9, dev)
    meta = _meta(dev, "logreg").eval()
    with torch.no_grad():
        got = meta.few_shot(batch, dev)
    want = _by_hand(meta, batch, dev)
    print(f"metabaseline few_shot with the logreg head: {got.tolist()}")
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    # the model's own head gives another loss on the same features
    with torch.no_grad():
        own = _meta(dev, "train").eval().few_shot(batch, dev)
    assert float(own[0]) != float(got[0])
    torch.manual_seed(17)
    pre = Pretrain("conv4", image_size=SIZE, image_channels=3, n_classes=6, num_ways=N, metric="logreg", logreg=CFG).to(dev).eval()
    pre.conv.load_state_dict(meta.conv.state_dict())
    with torch.no_grad():
        got_p = pre.few_shot(batch, dev)
    assert torch.equal(got_p, want)
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0


def test_training_step_does_not_depend_on_the_evaluation_head(dev):
    from fumi_amd import hip
    batch = _batch(3, dev)
    flats = []
    for eval_head in ("train", "logreg"):
        model = _meta(dev, eval_head)
        model.evaluate(batch, None, None, dev, task="train")
        flats.append(model._flat.flat.clone())
        assert model.temp.grad is not None
    assert torch.equal(flats[0], flats[1]) and bool(torch.isfinite(flats[0]).all())
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0


def test_cli_pretrain_with_the_logreg_metric_finishes_with_a_finite_validation_accuracy(dev, tmp_path, monkeypatch):
    from fumi_amd import hip
    from fumi_amd import main as cli
    monkeypatch.chdir(tmp_path)
    res = cli.main(cli.parse_args(["--model", "pretrain", "--pretrain_metric", "logreg", "--logreg_steps", "50", "--dataset",
                                   "synthetic-resident", "--im_encoder", "conv4", "--image_size", "16", "--synthetic_classes", "8",
                                   "--text_emb_dim", "32", "--batch_size", "2", "--num_ways", "5", "--num_shots", "2",
                                   "--num_shots_test", "2", "--num_ep_test", "4", "--pretrain_batch", "16", "--pretrain_bn_group", "4",
                                   "--epochs", "3", "--eval_freq", "2", "--lr", "1e-2", "--log_dir", str(tmp_path / "res"),
                                   "--wandb_offline"]))
    run, = glob.glob(str(tmp_path / "res" / "runs" / "train-*"))
    recs = [json.loads(l) for l in open(os.path.join(run, "metrics.jsonl"))]
    val = [(r["_step"], r["val/loss"], r["val/acc"]) for r in recs if "val/acc" in r]
    print(f"cli pretrain logreg: val (step, loss, acc) {val}; test loss {res['test_loss']:.4f}, acc {res['test_acc']:.4f}")
    assert val and all(np.isfinite(l) and 0.0 <= a <= 1.0 for _, l, a in val)
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
