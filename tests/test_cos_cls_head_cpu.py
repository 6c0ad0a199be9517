"""CPU suite of the cosine classifier head: the float64 restatement tests/cos_cls_head_ref.py against central
finite differences of its own loss, the conditions tests/test_cos_cls_head_gpu.py relies on (how many rows of each case it sets aside,
what an out-of-range label and a zero row do), and the flags, refusals and state_dict of --pretrain_head cosine."""
import numpy as np
import pytest
import torch

from cls_head_ref import ST_LABEL_RANGE
from cos_cls_head_cases import INPUTS, MARGIN, MAX_SET_ASIDE, SHAPES, TARGETS, case, second_labels, target_kw
from cos_cls_head_ref import cos_cls_head_ref


# ---- the reference --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,F,C,kw", [(3, 5, 4, dict()), (4, 6, 3, dict(lam=0.3, smoothing=0.1, mixed=True))])
def test_reference_gradients_match_central_finite_differences(M, F, C, kw):
    """The closed forms of dfeats, gW and dtau against (loss(p + h) - loss(p - h)) / 2h in float64, h = 1e-6: the difference
    quotient's own error is h^2 |loss'''| / 6 ~ 1e-12 plus rounding 1e-16 / h = 1e-10, held to 1e-7 of the largest entry."""
    rng = np.random.default_rng(17 * M + F)
    x, W, tau, gs = rng.standard_normal((M, F)) + 0.5, rng.standard_normal((C, F)), 2.5, 0.25
    y = rng.integers(0, C, M)
    kw = dict(kw)
    y_b = np.roll(y, 1) if kw.pop("mixed", False) else None
    ref = cos_cls_head_ref(x, y, W, tau, gs, y_b=y_b, **kw)
    loss = lambda x_, W_, t_: gs * cos_cls_head_ref(x_, y, W_, t_, y_b=y_b, **kw)["loss"]
    h = 1e-6

    def fd(arr, f):
        out = np.zeros_like(arr)
        for i in np.ndindex(arr.shape):
            p, m = arr.copy(), arr.copy()
            p[i] += h; m[i] -= h
            out[i] = (f(p) - f(m)) / (2 * h)
        return out
    for name, got, want in (("dfeats", ref["dfeats"], fd(x, lambda v: loss(v, W, tau))), ("gW", ref["gW"], fd(W, lambda v: loss(x, v, tau))),
                            ("dtau", np.array([ref["dtau"]]), fd(np.array([tau]), lambda v: loss(x, W, v[0])))):
        e = np.abs(got - want).max() / np.abs(want).max()
        print(f"{name}: {e:.3e}")
        assert e <= 1e-7, (name, e)
    # the gradients are tangential: no step along a row changes its direction
    assert np.abs((ref["dfeats"] * x).sum(axis=1)).max() <= 1e-12 and np.abs((ref["gW"] * W).sum(axis=1)).max() <= 1e-12


def test_reference_equals_torch_autograd_on_normalised_rows():
    import torch.nn.functional as Fn
    M, F, C = 9, 16, 7
    x, y, W, tau = case(M, F, C)
    y_b = second_labels(y, M, F, C)
    ref = cos_cls_head_ref(x.numpy(), y.numpy(), W.numpy(), tau.numpy(), 0.25, y_b=y_b.numpy(), lam=0.3, smoothing=0.1)
    xt, Wt, tt = (t.double().requires_grad_(True) for t in (x, W, tau))
    z = tt * Fn.normalize(xt, dim=1) @ Fn.normalize(Wt, dim=1).T
    t = 0.9 * (0.3 * Fn.one_hot(y, C).double() + 0.7 * Fn.one_hot(y_b, C).double()) + 0.1 / C
    loss = Fn.cross_entropy(z, t)
    (0.25 * loss).backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12
    for got, want in ((ref["dfeats"], xt.grad), (ref["gW"], Wt.grad), (np.array([ref["dtau"]]), tt.grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-12


@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("M,F,C", SHAPES)
def test_the_gpu_cases_set_aside_at_most_one_row_in_a_hundred(M, F, C, inputs):
    """Checked here so that the set-aside of tests/test_cos_cls_head_gpu.py cannot hide a failure."""
    x, y, W, tau = case(M, F, C, inputs)
    ref = cos_cls_head_ref(x.numpy(), y.numpy(), W.numpy(), tau.numpy())
    under = int((ref["margin"] <= MARGIN).sum())
    print(f"({M},{F},{C}) {inputs}: {under} of {M} rows under the margin, smallest {ref['margin'].min():.3e}")
    assert under <= MAX_SET_ASIDE * M
    assert np.isfinite(ref["dfeats"]).all() and np.isfinite(ref["gW"]).all()


def test_reference_drops_a_row_with_a_label_out_of_range():
    M, F, C = 17, 96, 5
    x, y, W, tau = case(M, F, C)
    kw = target_kw("soft", y, M, F, C)
    y_b = kw.pop("y_b").clone()
    y_b[7] = C
    keep = np.arange(M) != 7
    a = (x.numpy(), y.numpy(), W.numpy(), tau.numpy())
    full = cos_cls_head_ref(*a, 0.25, y_b=y_b.numpy(), **kw)
    sub = cos_cls_head_ref(a[0][keep], a[1][keep], a[2], a[3], 0.25, y_b=y_b.numpy()[keep], **kw)
    assert full["status"] == ST_LABEL_RANGE and sub["status"] == 0 and not full["dfeats"][7].any()
    s = (M - 1) / M                                                               # the divisor stays M
    assert abs(full["loss"] - s * sub["loss"]) <= 1e-14 and abs(full["dtau"] - s * sub["dtau"]) <= 1e-14
    assert np.abs(full["gW"] - s * sub["gW"]).max() <= 1e-14 and np.abs(full["dfeats"][keep] - s * sub["dfeats"]).max() <= 1e-14
    assert full["correct"] == sub["correct"]


def test_reference_treats_a_zero_row_as_the_zero_direction():
    M, F, C = 17, 96, 5
    x, y, W, tau = case(M, F, C)
    x[3] = 0.0
    W[2] = 0.0
    x[5] = 1e-20                                                                   # a norm below eps, not zero
    ref = cos_cls_head_ref(x.numpy(), y.numpy(), W.numpy(), tau.numpy(), 0.25)
    assert all(np.isfinite(np.asarray(ref[k])).all() for k in ("loss", "dfeats", "gW", "dtau", "logits"))
    assert not ref["dfeats"][3].any() and not ref["dfeats"][5].any() and not ref["gW"][2].any()
    assert not ref["logits"][3].any() and not ref["logits"][:, 2].any()
    assert ref["dfeats"][4].any() and ref["gW"][1].any()


# ---- flags and refusals ---------------------------------------------------------------------------------------------------------
class StubEngine:
    """Records the engine calls of Pretrain.train_step; runs on the host with made-up features."""
    runs_on_host = True

    def __init__(self):
        self.calls = []

    def _encode(self, x_s, x_q, theta, keep_tape=False):
        self.calls.append(("encode", {}))
        f = lambda x: x.reshape(x.shape[0], x.shape[1], -1)[..., :self.F]
        return f(x_s), f(x_q)

    def _encode_bwd(self, x_s, x_q, df_s, df_q, theta, scale=1.0, g_theta=None):
        self.calls.append(("encode_bwd", {}))

    conv4_encode = resnet12_encode = _encode
    conv4_encode_bwd = resnet12_encode_bwd = _encode_bwd

    def _head(self, name, feats, **kw):
        self.calls.append((name, kw))
        one = torch.ones(1)
        return dict(loss=one, correct=one, preds=torch.zeros(feats.shape[0], dtype=torch.int64), dfeats=torch.zeros_like(feats))

    def cls_head_step(self, feats, y, W, b, **kw):
        return self._head("cls_head_step", feats, W=W, b=b, **kw)

    def cls_head_step_soft(self, feats, y, W, b, **kw):
        return self._head("cls_head_step_soft", feats, W=W, b=b, **kw)

    def cos_cls_head_step(self, feats, y, W, tau, **kw):
        return self._head("cos_cls_head_step", feats, W=W, tau=tau, **kw)


@pytest.fixture()
def stub_engine():
    from fumi_amd import engine
    eng = StubEngine()
    old = engine.set_engine(eng)
    yield eng
    engine.set_engine(old)


_PRETRAIN = ["--model", "pretrain", "--disable_cuda", "--dataset", "synthetic-resident", "--im_encoder", "conv4"]
_NAMES = ["--pretrain_head", "--pretrain_head_scale", "--pretrain_head_scale_fixed"]


def test_the_flags_parse_with_their_defaults_after_every_earlier_flag():
    from fumi_amd import main as cli
    from fumi_amd.utils import utils
    d = cli.parse_args(["--disable_cuda"])
    assert (d.pretrain_head, d.pretrain_head_scale, d.pretrain_head_scale_fixed) == ("linear", 10.0, False)
    a = cli.parse_args(["--disable_cuda", "--pretrain_head", "cosine", "--pretrain_head_scale", "16", "--pretrain_head_scale_fixed"])
    assert (a.pretrain_head, a.pretrain_head_scale, a.pretrain_head_scale_fixed) == ("cosine", 16.0, True)
    with pytest.raises(SystemExit):
        cli.parse_args(["--disable_cuda", "--pretrain_head", "arcface"])
    assert [f for f, _ in utils._PRETRAIN_HEAD_FLAGS] == _NAMES
    flags = lambda p: [act.option_strings[0] for act in p._actions if act.option_strings and act.dest != "help"]
    assert flags(utils.run_parser()) == flags(utils.cli_parser()) + _NAMES
    assert not [f for f in flags(utils.cli_parser()) if f.startswith("--pretrain_head")]          # cli_parser() is what it was


def test_check_supported_takes_the_cosine_head_and_refuses_what_does_not_go_with_it(stub_engine, tmp_path):
    from fumi_amd import main as cli
    cli.check_supported(cli.parse_args(_PRETRAIN))
    cli.check_supported(cli.parse_args(_PRETRAIN + ["--pretrain_head", "linear"]))
    cli.check_supported(cli.parse_args(_PRETRAIN + ["--pretrain_head", "cosine"]))
    cli.check_supported(cli.parse_args(_PRETRAIN + ["--pretrain_head", "cosine", "--pretrain_head_scale", "16", "--pretrain_head_scale_fixed",
                                                    "--pretrain_metric", "cosine", "--label_smoothing", "0.1", "--mixup_alpha", "0.4"]))
    for extra in (["--pretrain_head", "cosine"], ["--pretrain_head_scale", "5"], ["--pretrain_head_scale_fixed"]):
        for other in (["--model", "am3", "--dropout", "0"], ["--model", "metabaseline", "--dataset", "synthetic-resident", "--im_encoder", "conv4"]):
            with pytest.raises(ValueError, match="--model pretrain"):
                cli.check_supported(cli.parse_args(other + ["--disable_cuda"] + extra))
    for bad in ("0", "-2", "nan", "inf"):
        with pytest.raises(ValueError, match="--pretrain_head_scale"):
            cli.check_supported(cli.parse_args(_PRETRAIN + ["--pretrain_head", "cosine", "--pretrain_head_scale", bad]))
    for extra in (["--pretrain_head_scale", "5"], ["--pretrain_head_scale_fixed"]):
        with pytest.raises(ValueError, match="--pretrain_head cosine"):
            cli.check_supported(cli.parse_args(_PRETRAIN + extra))
    ckpt = tmp_path / "teacher.pth.tar"
    ckpt.write_bytes(b"")
    cli.check_supported(cli.parse_args(_PRETRAIN + ["--distill_checkpoint", str(ckpt)]))
    with pytest.raises(NotImplementedError, match="--pretrain_head cosine"):
        cli.check_supported(cli.parse_args(_PRETRAIN + ["--pretrain_head", "cosine", "--distill_checkpoint", str(ckpt)]))


def test_pretrain_refuses_what_the_cosine_head_cannot_be():
    from fumi_amd.models.pretrain import Pretrain
    mk = lambda **kw: Pretrain("conv4", image_size=16, n_classes=4, **kw)
    with pytest.raises(ValueError, match="linear or cosine"):
        mk(head="arcface")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="positive"):
            mk(head="cosine", head_scale=bad)
    with pytest.raises(ValueError, match="cosine head"):
        mk(head_scale_fixed=True)
    with pytest.raises(ValueError, match="cosine head"):
        mk(head="linear", head_scale=5.0)
    with pytest.raises(NotImplementedError, match="cosine student or teacher"):
        mk(head="cosine", distill={})
    student = mk(distill={})
    with pytest.raises(ValueError, match="cls_scale"):
        student.load_teacher(mk(head="cosine").state_dict())
    assert student._teacher is None
    student.load_teacher(mk().state_dict())                                       # a linear teacher loads as before


def test_state_dict_keys_of_both_heads_and_of_the_fixed_scale():
    from fumi_amd.models.pretrain import Pretrain, head_log
    mk = lambda **kw: Pretrain("conv4", image_size=16, n_classes=4, **kw)
    plain, linear = mk(), mk(head="linear")
    conv = [k for k in plain.state_dict() if k.startswith("conv.")]
    assert list(plain.state_dict()) == list(linear.state_dict()) == conv + ["classifier.weight", "classifier.bias"]
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in linear.named_parameters()]
    assert head_log(plain) == {}
    cos = mk(head="cosine", head_scale=16.0)
    assert sorted(cos.state_dict()) == sorted(conv + ["classifier.weight", "cls_scale"])
    assert cos.classifier.bias is None and isinstance(cos.cls_scale, torch.nn.Parameter) and cos.cls_scale.tolist() == [16.0]
    assert cos._head_params()[0] is cos.classifier.weight and cos._head_params()[1] is cos.cls_scale and len(cos._head_params()) == 2
    assert head_log(cos) == {"cls_scale": 16.0}
    fixed = mk(head="cosine", head_scale_fixed=True)
    assert sorted(fixed.state_dict()) == sorted(cos.state_dict())                  # a persistent buffer: the same checkpoint keys
    assert "cls_scale" not in dict(fixed.named_parameters()) and fixed.cls_scale.tolist() == [10.0]
    assert len(fixed._head_params()) == 1
    fixed.load_state_dict(cos.state_dict())
    assert fixed.cls_scale.tolist() == [16.0]
    with pytest.raises(RuntimeError, match="classifier.bias"):
        cos.load_state_dict(plain.state_dict())


def test_init_model_builds_the_head_the_flags_name():
    from fumi_amd import main as cli
    from fumi_amd.utils import utils
    def build(extra):
        a = cli.parse_args(_PRETRAIN + ["--image_size", "16"] + extra)
        a.n_classes = 8                                                            # (set by the dataset in a run)
        return utils.init_model(a, None, watch=False)
    m = build([])
    assert m.head == "linear" and "cls_scale" not in m.state_dict() and m.classifier.bias is not None
    m = build(["--pretrain_head", "cosine", "--pretrain_head_scale", "12"])
    assert m.head == "cosine" and m.cls_scale.tolist() == [12.0] and isinstance(m.cls_scale, torch.nn.Parameter)
    m = build(["--pretrain_head", "cosine", "--pretrain_head_scale_fixed"])
    assert m.head_scale_fixed and "cls_scale" in m._buffers


@pytest.mark.parametrize("fixed", [False, True])
def test_a_cosine_step_always_calls_the_cosine_head(fixed, stub_engine):
    from fumi_amd.models.pretrain import Pretrain
    torch.manual_seed(5)
    model = Pretrain("conv4", image_size=16, n_classes=4, bn_group=2, head="cosine", head_scale_fixed=fixed, label_smoothing=0.1)
    stub_engine.F = model.conv.feature_dim
    x, y = torch.randn(8, 3, 16, 16), torch.randint(0, 4, (8,))
    model.train_step(x, y)
    y_b = y.flip(0)
    model.train_step(x, y, y_b=y_b, lam=0.3)
    assert [c[0] for c in stub_engine.calls] == ["encode", "cos_cls_head_step", "encode_bwd"] * 2
    kw = stub_engine.calls[4][1]
    assert (kw["smoothing"], kw["lam"], kw["need_grad"]) == (0.1, 0.3, True) and kw["y_b"] is y_b
    assert kw["W"].data_ptr() == model.classifier.weight.data_ptr() and kw["tau"].data_ptr() == model.cls_scale.data_ptr()
    flat = model._flat
    assert [p is q for p, q in zip(flat.params, model._head_params() + model.conv.theta())] == [True] * len(flat.params)
    assert kw["gW"] is flat.views[0]
    if fixed:
        assert kw["dtau"] is model._dscale and flat.params[1] is model.conv.theta()[0]
    else:
        assert kw["dtau"] is flat.views[1] and model.cls_scale.grad is flat.views[1]
    # the linear head's calls are the ones they were
    stub_engine.calls.clear()
    plain = Pretrain("conv4", image_size=16, n_classes=4, bn_group=2)
    plain.train_step(x, y)
    plain.train_step(x, y, y_b=y_b, lam=0.3)
    assert [c[0] for c in stub_engine.calls] == ["encode", "cls_head_step", "encode_bwd", "encode", "cls_head_step_soft", "encode_bwd"]


def test_the_binding_and_the_engine_carry_the_entry():
    from fumi_amd import engine, hip
    assert "fumi_hip_cos_cls_head_step" in hip.SYMBOLS
    assert callable(hip.cos_cls_head_step) and callable(engine.HipEngine.cos_cls_head_step)
