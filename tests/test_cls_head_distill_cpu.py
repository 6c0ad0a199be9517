"""CPU suite of born-again distillation for --model pretrain: the float64 restatement of the distillation head
against autograd and against the soft form, the four flags and the refusals of check_supported, the teacher of ``Pretrain`` (outside
parameters() and state_dict(), moved with the model), the order of the engine calls of a step, and the number of rows the GPU test sets
aside at each of its cases."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cls_head_distill_cases import CONFIGS, GRAD_SCALE, MAX_SET_ASIDE, SHAPES, case, set_aside
from cls_head_distill_ref import cls_head_distill_ref
from cls_head_ref import ST_LABEL_RANGE
from cls_head_soft_ref import cls_head_soft_ref


def _inputs(M=9, Fd=32, C=5, seed=11):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, W, b, x_t, W_t, b_t = r(M, Fd), r(C, Fd) * 0.3, r(C), r(M, Fd), r(C, Fd) * 0.3, r(C)
    y_a = torch.randint(0, C, (M,), generator=g)
    y_b = y_a[torch.randperm(M, generator=g)]
    y_b[:2] = y_a[:2]
    assert bool((y_a != y_b).any())
    return x, W, b, x_t, W_t, b_t, y_a, y_b


def _np(*ts):
    return [t.detach().numpy() for t in ts]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,alpha,cw,eps,lam", [(4.0, 0.5, 0.5, 0.0, 1.0), (1.0, 1.0, 0.0, 0.0, 1.0), (2.0, 0.9, 0.1, 0.1, 0.3)])
def test_distill_restatement_equals_autograd_in_float64(T, alpha, cw, eps, lam):
    gs = 0.25
    x, W, b, x_t, W_t, b_t, y_a, y_b = _inputs()
    x, W, b = (t.requires_grad_(True) for t in (x, W, b))
    z, z_t = x @ W.T + b, x_t @ W_t.T + b_t
    ce = lam * F.cross_entropy(z, y_a, label_smoothing=eps) + (1 - lam) * F.cross_entropy(z, y_b, label_smoothing=eps)
    kd = T * T * F.kl_div(F.log_softmax(z / T, dim=1), F.softmax(z_t / T, dim=1), reduction="batchmean")
    loss = cw * ce + alpha * kd
    dx, dW, db = torch.autograd.grad(gs * loss, [x, W, b])
    ref = cls_head_distill_ref(*_np(x, y_a, W, b, x_t, W_t, b_t), T, alpha, cw, gs, y_b=y_b.numpy(), lam=lam, smoothing=eps)
    assert ref["status"] == 0
    for k, want in (("loss", loss), ("loss_ce", ce), ("loss_kd", kd)):
        assert abs(ref[k] - float(want.detach())) <= 1e-12, k
    assert np.array_equal(ref["preds"], z.argmax(1).numpy()) and ref["correct"] == float((z.argmax(1) == y_a).sum())
    assert ref["agree"] == float((z.argmax(1) == z_t.argmax(1)).sum())
    assert np.abs(ref["probs_t"] - F.softmax(z_t / T, dim=1).numpy()).max() <= 1e-12
    for got, want in ((ref["dfeats"], dx), (ref["gW"], dW), (ref["gb"], db)):
        assert np.abs(got - want.numpy()).max() <= 1e-12


def test_distill_restatement_without_a_distillation_weight_is_the_soft_one():
    x, W, b, x_t, W_t, b_t, y_a, y_b = _inputs()
    a = _np(x, y_a, W, b)
    soft = cls_head_soft_ref(*a, 0.25, y_b=y_b.numpy(), lam=0.3, smoothing=0.1)
    kd = cls_head_distill_ref(*a, *_np(x_t, W_t, b_t), 4.0, 0.0, 1.0, 0.25, y_b=y_b.numpy(), lam=0.3, smoothing=0.1)
    assert set(kd) >= set(soft) | {"loss_ce", "loss_kd", "agree", "probs_t"}
    for k, v in soft.items():
        assert np.array_equal(np.asarray(kd[k]), np.asarray(v)), k


def test_distill_restatement_drops_a_row_whose_label_is_out_of_range():
    x, W, b, x_t, W_t, b_t, y_a, y_b = _inputs()
    M, C = x.shape[0], W.shape[0]
    bad = y_b.clone(); bad[4] = C
    keep = np.arange(M) != 4
    xs, ya, Wn, bn, xt, Wt, bt = _np(x, y_a, W, b, x_t, W_t, b_t)
    kw = dict(lam=0.3, smoothing=0.1)
    full = cls_head_distill_ref(xs, ya, Wn, bn, xt, Wt, bt, 2.0, 0.9, 0.1, y_b=bad.numpy(), **kw)
    sub = cls_head_distill_ref(xs[keep], ya[keep], Wn, bn, xt[keep], Wt, bt, 2.0, 0.9, 0.1, y_b=y_b.numpy()[keep], **kw)
    assert full["status"] == ST_LABEL_RANGE and sub["status"] == 0
    for k in ("loss", "loss_ce", "loss_kd"):
        assert abs(full[k] * M - sub[k] * (M - 1)) <= 1e-12, k
    assert not full["dfeats"][4].any()
    assert np.abs(full["dfeats"][keep] * M - sub["dfeats"] * (M - 1)).max() <= 1e-12
    assert np.abs(full["gW"] * M - sub["gW"] * (M - 1)).max() <= 1e-12 and np.abs(full["gb"] * M - sub["gb"] * (M - 1)).max() <= 1e-12
    assert full["correct"] == sub["correct"] and full["agree"] == sub["agree"]


def test_a_teacher_equal_to_the_student_leaves_the_cross_entropy_gradient():
    x, W, b, _, _, _, y_a, y_b = _inputs()
    a = _np(x, y_a, W, b)
    kd = cls_head_distill_ref(*a, *_np(x, W, b), 4.0, 0.5, 0.5, 0.25, y_b=y_b.numpy(), lam=0.3, smoothing=0.1)
    soft = cls_head_soft_ref(*a, 0.25, y_b=y_b.numpy(), lam=0.3, smoothing=0.1)
    assert abs(kd["loss_kd"]) <= 1e-12 and kd["agree"] == float(x.shape[0])
    for k in ("dfeats", "gW", "gb"):
        assert np.abs(kd[k] - 0.5 * soft[k]).max() <= 1e-12, k


def test_a_peaked_teacher_gives_finite_values():
    x, W, b, x_t, W_t, b_t, y_a, _ = _inputs()
    kd = cls_head_distill_ref(*_np(x, y_a, W, b, x_t), *_np(50.0 * W_t, 50.0 * b_t), 1.0, 1.0, 0.0)
    assert kd["probs_t"].min() == 0.0 or kd["probs_t"].min() < 1e-30            # a logarithm of it would not be finite
    for k in ("loss", "loss_ce", "loss_kd", "dfeats", "gW", "gb", "probs_t"):
        assert np.isfinite(np.asarray(kd[k])).all(), k
    assert kd["loss_kd"] > 0.0


@pytest.mark.parametrize("M,Fd,C", SHAPES)
def test_the_gpu_cases_set_aside_at_most_two_rows(M, Fd, C):
    """Checked here so that the set-aside of tests/test_cls_head_distill_gpu.py cannot hide a failure: at every shape, and with the
    teacher's logits scaled by 50 as well, at most two rows have a top-two gap in z or z_t below 2e-4 max|z|."""
    c = case(M, Fd, C)
    a = _np(c["x"], c["y"], c["W"], c["b"], c["x_t"])
    for scale in (1.0, 50.0):
        ref = cls_head_distill_ref(*a, *_np(scale * c["W_t"], scale * c["b_t"]), 4.0, 0.5, 0.5, GRAD_SCALE)
        n = int(set_aside(ref).sum())
        print(f"({M},{Fd},{C}) teacher x{scale:g}: {n} rows set aside, agree {ref['agree']:.0f} of {M}")
        assert n <= MAX_SET_ASIDE
    assert len(CONFIGS) == 3 and bool((c["y_b"] == c["y"]).any())


# ---- flags and refusals ---------------------------------------------------------------------------------------------------------
class StubEngine:
    """Records the engine calls of Pretrain.train_step; runs on the host with made-up features."""
    runs_on_host = True

    def __init__(self):
        self.calls = []

    def _encode(self, x_s, x_q, theta, keep_tape=False):
        self.calls.append(("encode", bool(keep_tape), theta[0].data_ptr()))
        f = lambda x: x.reshape(x.shape[0], x.shape[1], -1)[..., :self.F] * float(theta[0].reshape(-1)[0])
        return f(x_s), f(x_q)

    def _encode_bwd(self, x_s, x_q, df_s, df_q, theta, scale=1.0, g_theta=None):
        self.calls.append(("encode_bwd",))

    conv4_encode = resnet12_encode = _encode
    conv4_encode_bwd = resnet12_encode_bwd = _encode_bwd

    def _head(self, name, feats, **kw):
        self.calls.append((name, kw))
        M = feats.shape[0]
        one = torch.ones(1)
        return dict(loss=one, correct=one, preds=torch.zeros(M, dtype=torch.int64), dfeats=torch.zeros_like(feats), loss_ce=one,
                    loss_kd=one, agree=one)

    def cls_head_step(self, feats, y, W, b, **kw):
        return self._head("cls_head_step", feats, **kw)

    def cls_head_step_soft(self, feats, y, W, b, **kw):
        return self._head("cls_head_step_soft", feats, **kw)

    def cls_head_step_distill(self, feats, y, W, b, feats_t, W_t, b_t, **kw):
        return self._head("cls_head_step_distill", feats, feats_t=feats_t, W_t=W_t, b_t=b_t, **kw)


@pytest.fixture()
def stub_engine():
    from fumi_amd import engine
    eng = StubEngine()
    old = engine.set_engine(eng)
    yield eng
    engine.set_engine(old)


_PRETRAIN = ["--model", "pretrain", "--disable_cuda", "--dataset", "synthetic-resident", "--im_encoder", "conv4"]


def test_distill_flags_parse_with_their_defaults_at_the_tail_of_the_reference_list():
    from fumi_amd.utils import utils
    d = utils.parser().parse_args([])
    assert (d.distill_checkpoint, d.distill_temp, d.distill_alpha, d.distill_ce_weight) == (None, 4.0, 0.5, 0.5)
    a = utils.parser().parse_args(["--distill_checkpoint", "t.pth.tar", "--distill_temp", "2", "--distill_alpha", "0.9",
                                   "--distill_ce_weight", "0.1"])
    assert (a.distill_checkpoint, a.distill_temp, a.distill_alpha, a.distill_ce_weight) == ("t.pth.tar", 2.0, 0.9, 0.1)
    names = ["--distill_checkpoint", "--distill_temp", "--distill_alpha", "--distill_ce_weight"]
    assert [f for f, _ in utils._DISTILL_FLAGS] == names
    assert len(utils._REFERENCE_FLAGS) == 50 and utils._FLAGS == utils._REFERENCE_FLAGS + utils._DISTILL_FLAGS
    flags = [act.option_strings[0] for act in utils.parser()._actions if act.option_strings and act.dest != "help"]
    assert flags[50:54] == names and flags[54] == utils._RIDGE_FLAGS[0][0]
    assert not [f for f in flags if f.startswith("--distill") and f not in names]


@pytest.mark.parametrize("flag,value", [("--distill_checkpoint", "CKPT"), ("--distill_temp", "2"), ("--distill_alpha", "0.9"),
                                        ("--distill_ce_weight", "0.1")])
def test_check_supported_refuses_a_distill_flag_without_model_pretrain(flag, value, stub_engine, tmp_path):
    from fumi_amd import main as cli
    ckpt = tmp_path / "teacher.pth.tar"
    ckpt.write_bytes(b"")
    value = str(ckpt) if value == "CKPT" else value
    with pytest.raises(ValueError, match="--model pretrain"):
        cli.check_supported(cli.parse_args(["--model", "am3", "--disable_cuda", "--dropout", "0", flag, value]))


@pytest.mark.parametrize("flag,value", [("--distill_temp", "2"), ("--distill_alpha", "0.9"), ("--distill_ce_weight", "0.1")])
def test_check_supported_refuses_a_weight_without_a_teacher(flag, value, stub_engine, tmp_path):
    from fumi_amd import main as cli
    with pytest.raises(ValueError, match="--distill_checkpoint"):
        cli.check_supported(cli.parse_args(_PRETRAIN + [flag, value]))
    ckpt = tmp_path / "teacher.pth.tar"
    ckpt.write_bytes(b"")
    cli.check_supported(cli.parse_args(_PRETRAIN + [flag, value, "--distill_checkpoint", str(ckpt)]))
    cli.check_supported(cli.parse_args(_PRETRAIN))


@pytest.mark.parametrize("flag,value", [("--distill_temp", "0"), ("--distill_temp", "-1"), ("--distill_temp", "nan"),
                                        ("--distill_alpha", "-0.1"), ("--distill_ce_weight", "-0.5")])
def test_check_supported_refuses_values_out_of_range(flag, value, stub_engine, tmp_path):
    from fumi_amd import main as cli
    ckpt = tmp_path / "teacher.pth.tar"
    ckpt.write_bytes(b"")
    with pytest.raises(ValueError, match=flag):
        cli.check_supported(cli.parse_args(_PRETRAIN + ["--distill_checkpoint", str(ckpt), flag, value]))


def test_check_supported_refuses_a_teacher_file_that_does_not_exist(stub_engine, tmp_path):
    from fumi_amd import main as cli
    with pytest.raises(ValueError, match="does not exist"):
        cli.check_supported(cli.parse_args(_PRETRAIN + ["--distill_checkpoint", str(tmp_path / "missing.pth.tar")]))


def test_a_teacher_of_another_backbone_or_image_shape_is_refused_by_name(stub_engine, tmp_path):
    from fumi_amd import main as cli
    from fumi_amd.models.pretrain import Pretrain
    from fumi_amd.utils import utils
    teacher = Pretrain("conv4", image_size=16, n_classes=4)
    args = cli.parse_args(_PRETRAIN + ["--image_size", "16"])
    for key, other in (("im_encoder", "resnet12"), ("image_size", 32), ("image_channels", 1)):
        saved = dict(vars(args)); saved[key] = other
        path = tmp_path / f"{key}.pth.tar"
        torch.save({"state_dict": teacher.state_dict(), "args": saved, "batch_idx": 0}, path)
        student = Pretrain("conv4", image_size=16, n_classes=4, distill={})
        with pytest.raises(ValueError, match=f"--{key}"):
            utils.load_distill_checkpoint(student, args, str(path))
    path = tmp_path / "same.pth.tar"
    torch.save({"state_dict": teacher.state_dict(), "args": dict(vars(args)), "batch_idx": 0}, path)
    student = utils.load_distill_checkpoint(Pretrain("conv4", image_size=16, n_classes=4, distill={}), args, str(path))
    assert student._teacher is not None


# ---- the model ------------------------------------------------------------------------------------------------------------------
def test_distill_config_is_checked():
    from fumi_amd.models.pretrain import Pretrain
    assert Pretrain("conv4", image_size=16, n_classes=4).distill is None
    assert Pretrain("conv4", image_size=16, n_classes=4, distill={}).distill == dict(temp=4.0, alpha=0.5, ce_weight=0.5)
    for bad in (dict(temp=0.0), dict(temp=float("nan")), dict(alpha=-1.0), dict(ce_weight=-0.5), dict(alpha=float("inf"))):
        with pytest.raises(ValueError, match="distillation"):
            Pretrain("conv4", image_size=16, n_classes=4, distill=bad)


@pytest.mark.parametrize("backbone", ["conv4", "resnet12"])
def test_the_teacher_is_outside_parameters_and_state_dict_and_moves_with_the_model(backbone):
    from fumi_amd.models.pretrain import Pretrain
    torch.manual_seed(3)
    teacher = Pretrain(backbone, image_size=16, n_classes=4)
    plain = Pretrain(backbone, image_size=16, n_classes=4)
    student = Pretrain(backbone, image_size=16, n_classes=4, distill=dict(temp=2.0, alpha=0.9, ce_weight=0.1))
    student.load_state_dict(plain.state_dict())
    keys, n_par = list(student.state_dict()), len(list(student.parameters()))
    student.load_teacher(teacher.state_dict())
    assert list(student.state_dict()) == keys == list(plain.state_dict())
    assert len(list(student.parameters())) == n_par == len(list(plain.parameters()))
    assert len(list(student.modules())) == len(list(plain.modules()))
    for k, v in plain.state_dict().items():
        assert torch.equal(student.state_dict()[k], v), k
    conv_t, w_t = student._teacher
    for k, v in conv_t.state_dict().items():
        assert torch.equal(v, teacher.state_dict()["conv." + k]), k
    assert torch.equal(w_t[0], teacher.classifier.weight) and torch.equal(w_t[1], teacher.classifier.bias)
    assert not any(p.requires_grad for p in conv_t.parameters()) and not w_t[0].requires_grad
    student.to(torch.float64)                                                    # (_apply: what .to(device) goes through)
    conv_t, w_t = student._teacher
    assert all(p.dtype == torch.float64 for p in conv_t.parameters()) and w_t[0].dtype == w_t[1].dtype == torch.float64
    assert student._tcache is None


def test_load_teacher_names_a_missing_or_misshapen_tensor():
    from fumi_amd.models.pretrain import Pretrain
    teacher = Pretrain("conv4", image_size=16, n_classes=4)
    student = Pretrain("conv4", image_size=16, n_classes=4, distill={})
    for name in ("conv.block2.conv.weight", "classifier.weight", "classifier.bias"):
        sd = dict(teacher.state_dict()); del sd[name]
        with pytest.raises(ValueError, match=name):
            student.load_teacher(sd)
        sd = dict(teacher.state_dict()); sd[name] = torch.zeros(3, 1, 2)
        with pytest.raises(ValueError, match=name):
            student.load_teacher(sd)
    with pytest.raises(ValueError, match="classifier.weight"):
        student.load_teacher(Pretrain("conv4", image_size=16, n_classes=5).state_dict())
    assert student._teacher is None
    with pytest.raises(ValueError, match="distill"):
        Pretrain("conv4", image_size=16, n_classes=4).load_teacher(teacher.state_dict())


def test_a_step_encodes_with_the_teacher_first_and_without_a_tape(stub_engine):
    from fumi_amd.models.pretrain import Pretrain
    torch.manual_seed(5)
    teacher = Pretrain("conv4", image_size=16, n_classes=4)
    student = Pretrain("conv4", image_size=16, n_classes=4, bn_group=2, distill=dict(temp=2.0, alpha=0.9, ce_weight=0.1),
                       label_smoothing=0.1)
    stub_engine.F = student.conv.feature_dim
    x, y = torch.randn(8, 3, 16, 16), torch.randint(0, 4, (8,))
    with pytest.raises(RuntimeError, match="load_teacher"):
        student.train_step(x, y)
    assert stub_engine.calls == []
    student.load_teacher(teacher.state_dict())
    y_b = y.flip(0)
    out = student.train_step(x, y, y_b=y_b, lam=0.3)
    conv_t, w_t = student._teacher
    names = [c[0] for c in stub_engine.calls]
    assert names == ["encode", "encode", "cls_head_step_distill", "encode_bwd"]
    assert stub_engine.calls[0][1:] == (False, conv_t.theta()[0].data_ptr())          # the teacher, untaped
    assert stub_engine.calls[1][1:] == (True, student.conv.theta()[0].data_ptr())     # the student, taped
    kw = stub_engine.calls[2][1]
    assert (kw["temp"], kw["alpha"], kw["ce_weight"], kw["smoothing"], kw["lam"]) == (2.0, 0.9, 0.1, 0.1, 0.3)
    assert kw["y_b"] is y_b and kw["W_t"] is w_t[0] and kw["b_t"] is w_t[1] and kw["need_grad"]
    scale_t = float(conv_t.theta()[0].reshape(-1)[0])
    assert torch.equal(kw["feats_t"], x.reshape(8, -1)[:, :stub_engine.F] * scale_t)  # the student's x, in the images' order
    assert student.last_out is out
    # without distill the calls are the ones they were
    stub_engine.calls.clear()
    plain = Pretrain("conv4", image_size=16, n_classes=4, bn_group=2)
    plain.train_step(x, y)
    assert [c[0] for c in stub_engine.calls] == ["encode", "cls_head_step", "encode_bwd"]


def test_distill_log_reports_the_last_step(stub_engine):
    from fumi_amd.models.pretrain import Pretrain, distill_log
    plain = Pretrain("conv4", image_size=16, n_classes=4, bn_group=2)
    assert distill_log(plain) == {}
    plain.last_out = dict(loss_ce=torch.tensor([1.5]), loss_kd=torch.tensor([0.25]), agree=torch.tensor([6.0]), preds=torch.zeros(8))
    assert distill_log(plain) == {"train/loss_ce": 1.5, "train/loss_kd": 0.25, "train/teacher_agree": 0.75}
