"""GPU tests of born-again distillation for --model pretrain (--distill_checkpoint), end to end on the 16 x 16
synthetic resident pixel table with M = 16, R = 4, Conv4 (fp32) and ResNet-12 (bf16): the head outputs of a step are the float64
distillation loss of the features the engine returns, a teacher that carries no weight changes no bit of three steps, the default weights
lower the distillation loss, a teacher of another backbone is refused, and the student's checkpoint is a plain --model pretrain one."""
import numpy as np
import pytest
import torch

from cls_head_distill_ref import cls_head_distill_ref

pytestmark = pytest.mark.gpu

BACKBONES = ["conv4", "resnet12"]
TOL = 1e-4                                                                  # the head's bound (tests/test_cls_head_distill_gpu.py)


def _common(backbone):
    return ["--model", "pretrain", "--dataset", "synthetic-resident", "--im_encoder", backbone, "--image_size", "16",
            "--synthetic_classes", "8", "--text_emb_dim", "32", "--batch_size", "4", "--num_ways", "5", "--num_shots", "5",
            "--num_ep_test", "8", "--pretrain_batch", "16", "--pretrain_bn_group", "4", "--lr", "2e-3", "--wandb_offline"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _setup(backbone, extra=(), seed=None):
    """(args, the supervised train source, the model main builds for them, teacher included)."""
    from fumi_amd import main as cli
    from fumi_amd.utils import utils
    args = cli.parse_args(_common(backbone) + list(extra))
    cli.check_supported(args)
    train = cli.get_dataset(args)[0]
    args.n_classes = int(train.n_classes)
    torch.manual_seed(args.seed if seed is None else seed)
    model = utils.init_model(args, None, watch=False)
    if args.distill_checkpoint:
        model = utils.load_distill_checkpoint(model, args, args.distill_checkpoint)
    return args, train, model


@pytest.fixture(scope="module")
def teachers(dev, tmp_path_factory):
    """Per backbone the checkpoint file of a teacher trained for four steps, in the dictionary training_run saves."""
    from fumi_amd.utils import utils
    out = {}
    for backbone in BACKBONES:
        args, train, model = _setup(backbone, seed=991)
        opt = utils.init_optim(args, model)
        for step in range(4):
            model.evaluate(train.batch(step), opt, None, dev, task="train")
        path = str(tmp_path_factory.mktemp("teacher") / f"{backbone}.pth.tar")
        torch.save({"batch_idx": 3, "state_dict": model.state_dict(), "best_loss": 0.0, "optimizer": opt.state_dict(),
                    "args": vars(args)}, path)
        out[backbone] = path
    return out


def _features(model, theta, x, dev):
    from fumi_amd import hip
    enc = hip.conv4_encode if model.backbone == "conv4" else hip.resnet12_encode
    M, R = x.shape[0], model.bn_group
    B, half = M // (2 * R), M // 2
    f_s, f_q = enc(hip.Workspace.get(dev, "encoder"), x[:half].view(B, R, *x.shape[1:]), x[half:].view(B, R, *x.shape[1:]), theta,
                   keep_tape=False)
    return torch.cat((f_s.view(half, -1), f_q.view(half, -1))).cpu().numpy()


@pytest.mark.parametrize("backbone", BACKBONES)
def test_first_step_publishes_the_float64_distillation_loss_of_its_features(backbone, teachers, dev):
    from fumi_amd import hip
    args, train, model = _setup(backbone, ["--distill_checkpoint", teachers[backbone], "--distill_temp", "2", "--distill_alpha", "0.9",
                                           "--distill_ce_weight", "0.1", "--label_smoothing", "0.1"])
    assert model.distill == dict(temp=2.0, alpha=0.9, ce_weight=0.1)
    sd = torch.load(teachers[backbone], map_location=dev, weights_only=False)["state_dict"]
    conv_t, w_t = model._teacher
    for k, v in conv_t.state_dict().items():
        assert v.device.type == "cuda" and torch.equal(v, sd["conv." + k]), k
    assert torch.equal(w_t[0], sd["classifier.weight"]) and torch.equal(w_t[1], sd["classifier.bias"])
    x, y = train.batch(0)
    npy = lambda t: t.detach().cpu().numpy()
    ref = cls_head_distill_ref(_features(model, [p.detach() for p in model.conv.theta()], x, dev), npy(y), npy(model.classifier.weight),
                               npy(model.classifier.bias), _features(model, [p.detach() for p in conv_t.theta()], x, dev),
                               npy(w_t[0]), npy(w_t[1]), 2.0, 0.9, 0.1, smoothing=0.1)
    out = model.train_step(x, y)                                            # no optimizer: the parameters stay
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
    for k in ("loss", "loss_ce", "loss_kd"):
        e = abs(float(out[k]) - ref[k]) / max(abs(ref[k]), 1e-5)
        print(f"{backbone} first step {k}: {float(out[k]):.6f}, float64 {ref[k]:.6f}, relative error {e:.3e}")
        assert e <= TOL, (k, e)
    near = int(((ref["margin"] < 2e-4 * abs(ref["logits"]).max()) | (ref["margin_t"] < 2e-4 * abs(ref["logits"]).max())).sum())
    assert abs(float(out["correct"]) - ref["correct"]) <= near and abs(float(out["agree"]) - ref["agree"]) <= near
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert all(p.grad is None for p in conv_t.parameters())


@pytest.mark.parametrize("backbone", BACKBONES)
def test_a_teacher_without_weight_changes_no_bit_of_three_steps(backbone, teachers, dev):
    """alpha = 0, ce_weight = 1: the head returns the bits of the plain head, so every parameter stays bit-equal only if the teacher's
    encode disturbs neither the student's tape, the workspaces nor any random draw."""
    from fumi_amd import hip
    from fumi_amd.utils import utils
    args_a, train_a, student = _setup(backbone, ["--distill_checkpoint", teachers[backbone], "--distill_alpha", "0",
                                                 "--distill_ce_weight", "1", "--augment", "--augment_pad", "1"])
    args_b, train_b, plain = _setup(backbone, ["--augment", "--augment_pad", "1"])
    assert student._teacher is not None and plain.distill is None
    for (n, p), (_, q) in zip(student.named_parameters(), plain.named_parameters()):
        assert torch.equal(p, q), n
    opt_a, opt_b = utils.init_optim(args_a, student), utils.init_optim(args_b, plain)
    for step in range(3):
        la = [float(v) for v in student.evaluate(train_a.batch(step), opt_a, None, dev, task="train")]
        lb = [float(v) for v in plain.evaluate(train_b.batch(step), opt_b, None, dev, task="train")]
        assert la == lb and np.isfinite(la).all()
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
    for (n, p), (_, q) in zip(student.named_parameters(), plain.named_parameters()):
        assert torch.equal(p, q), n


@pytest.mark.parametrize("backbone", BACKBONES)
def test_a_dozen_steps_at_the_default_weights_lower_the_distillation_loss(backbone, teachers, dev, tmp_path):
    """loss_kd of batch 0 before and after twelve optimizer steps (the same images both times: a batch is a function of seed and step);
    then the student's checkpoint loads into a plain Pretrain and through --encoder_checkpoint."""
    from fumi_amd import hip
    from fumi_amd.models.pretrain import Pretrain, distill_log
    from fumi_amd.utils import utils
    args, train, student = _setup(backbone, ["--distill_checkpoint", teachers[backbone]])
    assert student.distill == dict(temp=4.0, alpha=0.5, ce_weight=0.5)
    keys = list(student.state_dict())
    opt = utils.init_optim(args, student)
    assert sum(p.numel() for g in opt.param_groups for p in g["params"]) == sum(p.numel() for p in student.parameters())
    first = float(student.train_step(*train.batch(0))["loss_kd"])
    trace = []
    for step in range(12):
        student.evaluate(train.batch(step), opt, None, dev, task="train")
        trace.append(float(student.last_out["loss_kd"]))
    log = distill_log(student)
    assert set(log) == {"train/loss_ce", "train/loss_kd", "train/teacher_agree"} and 0.0 <= log["train/teacher_agree"] <= 1.0
    last = float(student.train_step(*train.batch(0))["loss_kd"])
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
    print(f"{backbone} loss_kd on batch 0: before {first:.6f}, after 12 steps {last:.6f}; per step {[round(v, 5) for v in trace]}")
    assert np.isfinite(trace).all() and last < first
    # the checkpoint format is unchanged
    assert list(student.state_dict()) == keys and not any("teacher" in k for k in keys)
    path = str(tmp_path / "student.pth.tar")
    torch.save({"batch_idx": 11, "state_dict": student.state_dict(), "best_loss": 0.0, "optimizer": opt.state_dict(),
                "args": vars(args)}, path)
    plain = Pretrain(im_encoder=backbone, image_size=16, image_channels=3, n_classes=args.n_classes, bn_group=4, num_ways=5).to(dev)
    plain, _ = utils.load_checkpoint(plain, utils.init_optim(args, plain), dev, path)
    other = Pretrain(im_encoder=backbone, image_size=16, image_channels=3, n_classes=args.n_classes, bn_group=4, num_ways=5).to(dev)
    utils.load_encoder_checkpoint(other, dev, path)
    for k, v in student.state_dict().items():
        assert torch.equal(plain.state_dict()[k], v), k
        if k.startswith("conv."):
            assert torch.equal(other.state_dict()[k], v), k


def test_a_teacher_of_another_backbone_is_refused(teachers, dev):
    with pytest.raises(ValueError, match="--im_encoder resnet12"):
        _setup("conv4", ["--distill_checkpoint", teachers["resnet12"]])
    with pytest.raises(ValueError, match="--im_encoder conv4"):
        _setup("resnet12", ["--distill_checkpoint", teachers["conv4"]])
