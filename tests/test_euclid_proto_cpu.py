"""CPU suite of the prototypical-network head and --fewshot_head proto: the float64 restatement
tests/euclid_proto_ref.py against torch.autograd on the direct-difference form, its invariance under a common shift of the features, the
margins of the GPU parity inputs (plain and shifted), the flags and refusals, the state_dict contract of MetaBaseline in both scale
modes, and a training step on a host-running oracle engine (as tests/test_logreg_head_cpu.py does it)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from euclid_proto_ref import (GRAD_SCALE, SHAPES, SHIFT, SHIFTED, ST_CLASS_MISSING, ST_LABEL_RANGE, case_inputs, euclid_proto_ref)
from oracle_engine import OracleEngine


# ---- the restatement of the head ------------------------------------------------------------------------------------------------
def _torch_head(f_s, y_s, f_q, y_q, alpha, N, gs):
    """The head in torch float64 ops with autograd, distances from the [B,Qn,N,F] differences; rows whose label is out of range are
    masked the way the kernel drops them."""
    xs = torch.tensor(f_s, dtype=torch.float64, requires_grad=True)
    xq = torch.tensor(f_q, dtype=torch.float64, requires_grad=True)
    a = torch.tensor([alpha], dtype=torch.float64, requires_grad=True)
    ys, yq = torch.as_tensor(y_s), torch.as_tensor(y_q)
    ok_s, ok_q = (ys >= 0) & (ys < N), (yq >= 0) & (yq < N)
    onehot = F.one_hot(ys.clamp(0, N - 1), N).to(torch.float64) * ok_s[..., None]
    protos = torch.bmm(onehot.transpose(1, 2), xs) / onehot.sum(1).clamp(min=1)[:, :, None]
    z = -a * ((xq[:, :, None, :] - protos[:, None, :, :]) ** 2).sum(-1)
    nll = F.cross_entropy(z.reshape(-1, N), yq.clamp(0, N - 1).reshape(-1), reduction="none")
    loss = (nll * ok_q.reshape(-1)).sum() / yq.numel()
    return xs, xq, a, z, loss, gs * loss


def _unequal_case(seed=5, B=2, S=9, Qn=6, N=4, Fd=32):
    rs = np.random.RandomState(seed)
    f_s, f_q = rs.standard_normal((B, S, Fd)), rs.standard_normal((B, Qn, Fd))
    y_s = np.tile(np.arange(S) % N, (B, 1)); y_s[:, -1] = 0                      # class 0 has three rows, classes 1..3 two
    y_q = rs.randint(0, N, (B, Qn))
    return f_s, y_s, f_q, y_q, N


def _rel(got, want):
    want = np.asarray(want)
    return float(np.abs(np.asarray(got) - want).max() / max(np.abs(want).max(), 1e-300))


def _compare(f_s, y_s, f_q, y_q, N, status, alpha=0.07, gs=0.25):
    ref = euclid_proto_ref(f_s, y_s, f_q, y_q, alpha, N, gs)
    xs, xq, a, z, loss, obj = _torch_head(f_s, y_s, f_q, y_q, alpha, N, gs)
    assert ref["status"] == status
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    assert _rel(ref["logits"], z.detach().numpy()) <= 1e-12
    dxs, dxq, da = torch.autograd.grad(obj, [xs, xq, a])
    for k, want in (("dfeats_s", dxs), ("dfeats_q", dxq), ("dalpha", da)):
        assert _rel(ref[k], want.numpy()) <= 1e-12, k
    return ref


def test_restatement_equals_autograd_with_unequal_class_counts():
    f_s, y_s, f_q, y_q, N = _unequal_case()
    ref = _compare(f_s, y_s, f_q, y_q, N, 0)
    z = ref["logits"]
    assert np.array_equal(ref["preds"], z.argmax(-1)) and ref["correct"] == float((z.argmax(-1) == y_q).sum())
    top = np.sort(z, -1)
    assert np.array_equal(ref["margin"], top[..., -1] - top[..., -2])
    assert ref["dalpha_abs"] >= abs(ref["dalpha"]) * (1 - 1e-12)


def test_restatement_equals_autograd_with_labels_out_of_range():
    f_s, y_s, f_q, y_q, N = _unequal_case(seed=6)
    y_q[1, 2] = N
    y_s[0, 3] = -1
    ref = _compare(f_s, y_s, f_q, y_q, N, ST_LABEL_RANGE)
    assert not ref["dfeats_q"][1, 2].any() and not ref["dfeats_s"][0, 3].any()
    # the support row is left out: the same numbers as the episode without it
    keep = np.arange(f_s.shape[1]) != 3
    sub = euclid_proto_ref(f_s[:1][:, keep], y_s[:1][:, keep], f_q[:1], y_q[:1], 0.07, N, 0.25)
    assert np.abs(sub["logits"] - ref["logits"][:1]).max() <= 1e-13


def test_restatement_equals_autograd_with_a_class_without_support():
    f_s, y_s, f_q, y_q, N = _unequal_case(seed=7)
    y_s[0][y_s[0] == 2] = 1                                                        # episode 0 has no row of class 2
    ref = _compare(f_s, y_s, f_q, y_q, N, ST_CLASS_MISSING)
    assert not ref["protos"][0, 2].any()
    assert np.abs(ref["logits"][0, :, 2] + 0.07 * (f_q[0] ** 2).sum(-1)).max() <= 1e-12    # a zero prototype: -alpha |f_q|^2


@pytest.mark.parametrize("case", ["unequal", "labels"])
def test_restatement_is_invariant_under_a_common_shift_of_the_features(case):
    f_s, y_s, f_q, y_q, N = _unequal_case(seed=9)
    if case == "labels":
        y_q[0, 1], y_s[1, 2] = -3, N + 1
    a = euclid_proto_ref(f_s, y_s, f_q, y_q, 0.07, N, 0.25)
    b = euclid_proto_ref(f_s + SHIFT, y_s, f_q + SHIFT, y_q, 0.07, N, 0.25)
    for k in ("logits", "dfeats_s", "dfeats_q", "dalpha"):
        assert _rel(b[k], a[k]) < 1e-10, k
    assert abs(b["loss"] - a["loss"]) < 1e-10 * a["loss"] and np.array_equal(a["preds"], b["preds"])


def _parity_inputs(shape, shifted):
    f_s, y_s, f_q, y_q = case_inputs(*shape)
    return (f_s + np.float32(SHIFT), y_s, f_q + np.float32(SHIFT), y_q) if shifted else (f_s, y_s, f_q, y_q)


@pytest.mark.parametrize("shape,shifted", [(s, False) for s in SHAPES] + [(s, True) for s in SHIFTED])
def test_margins_of_the_gpu_parity_inputs_leave_no_query_row_aside(shape, shifted):
    """With alpha = 1 / F every query row of every GPU parity input has a top-two margin above 1e-5, the softmax is not saturated and
    dalpha is not a difference of much larger parts: nothing is set aside, every gradient is exercised."""
    B, S, Qn, N, Fd = shape
    f_s, y_s, f_q, y_q = _parity_inputs(shape, shifted)
    ref = euclid_proto_ref(f_s, y_s, f_q, y_q, 1.0 / Fd, N, GRAD_SCALE)
    print(f"{shape}{' shifted' if shifted else ''}: smallest top-two margin {ref['margin'].min():.4g}, largest probability "
          f"{ref['pmax']:.3f}, |dalpha| / dalpha_abs {abs(ref['dalpha']) / ref['dalpha_abs']:.3f}")
    assert ref["status"] == 0 and ref["margin"].min() > 1e-5
    assert ref["margin"].min() >= 3.4e-3 * 0.99                                    # (the smallest over all shapes is 3.4e-3)
    assert ref["pmax"] <= 0.62
    assert abs(ref["dalpha"]) / ref["dalpha_abs"] >= 0.09
    if S > N:
        counts = np.stack([(y_s == n).sum(1) for n in range(N)], 1)
        assert (counts.max(1) > counts.min(1)).all()                               # unequal class counts


# ---- bindings, flags, refusals --------------------------------------------------------------------------------------------------
def test_the_binding_exists_in_every_layer():
    from fumi_amd import engine, hip
    assert callable(hip.euclid_proto_step) and "fumi_hip_euclid_proto_step" in hip.SYMBOLS
    assert callable(engine.HipEngine.euclid_proto_step)
    assert (hip.ST_LABEL_RANGE, hip.ST_CLASS_MISSING) == (ST_LABEL_RANGE, ST_CLASS_MISSING)


def test_proto_flags_parse_with_their_defaults_sit_after_the_logreg_flags_and_reach_the_model():
    from fumi_amd.utils import utils
    d = utils.parser().parse_args([])
    assert (d.fewshot_head, d.proto_scale, d.proto_scale_fixed, d.pretrain_metric) == ("cosine", 1.0, False, "euclidean")
    a = utils.parser().parse_args(["--model", "metabaseline", "--fewshot_head", "proto", "--proto_scale", "0.5", "--im_encoder", "conv4",
                                   "--image_size", "16", "--num_ways", "3"])
    assert (a.fewshot_head, a.proto_scale, a.proto_scale_fixed) == ("proto", 0.5, False)
    with pytest.raises(SystemExit):
        utils.parser().parse_args(["--fewshot_head", "svm"])
    with pytest.raises(SystemExit):
        utils.parser().parse_args(["--pretrain_metric", "proto"])                  # --pretrain_metric gains nothing
    assert [f for f, _ in utils._PROTO_FLAGS] == ["--proto_scale", "--proto_scale_fixed"]
    flags = [act.option_strings[0] for act in utils.parser()._actions if act.option_strings and act.dest != "help"]
    n_f, n_r, n_l, n_p = len(utils._FLAGS), len(utils._RIDGE_FLAGS), len(utils._LOGREG_FLAGS), len(utils._PROTO_FLAGS)
    at = n_f + n_r + n_l
    assert flags[n_f + n_r:at] == [f for f, _ in utils._LOGREG_FLAGS]
    assert flags[at:at + n_p] == [f for f, _ in utils._PROTO_FLAGS]                # directly after _LOGREG_FLAGS
    assert flags[at + n_p:at + n_p + len(utils._ENGINE_FLAGS)] == [f for f, _ in utils._ENGINE_FLAGS]
    a.device = "cpu"
    model = utils.init_model(a, None, watch=False)
    assert model.head == "proto" and not model.proto_scale_fixed and isinstance(model.proto_scale, torch.nn.Parameter)
    assert tuple(model.proto_scale.shape) == (1,) and float(model.proto_scale) == 0.5
    a.proto_scale_fixed = True
    fixed = utils.init_model(a, None, watch=False)
    assert fixed.proto_scale_fixed and not isinstance(fixed.proto_scale, torch.nn.Parameter) and float(fixed.proto_scale) == 0.5


def test_check_supported_refuses_what_the_proto_head_cannot_run():
    from fumi_amd import engine
    from fumi_amd import main as cli
    old = engine.set_engine(OracleEngine())
    try:
        base = ["--disable_cuda", "--dataset", "synthetic-resident", "--im_encoder", "conv4"]
        meta = ["--model", "metabaseline", "--fewshot_head", "proto"] + base
        cli.check_supported(cli.parse_args(meta))
        cli.check_supported(cli.parse_args(meta + ["--proto_scale_fixed"]))
        cli.check_supported(cli.parse_args(meta + ["--num_ways", "64", "--num_shots", "5", "--eval_head", "train"]))
        cli.check_supported(cli.parse_args(meta + ["--eval_head", "logreg"]))
        cli.check_supported(cli.parse_args(meta + ["--im_encoder", "resnet12", "--encoder_checkpoint", "x.pth.tar"]))
        with pytest.raises(ValueError, match="--fewshot_head"):
            cli.check_supported(cli.parse_args(["--model", "pretrain", "--fewshot_head", "proto"] + base))
        with pytest.raises(ValueError, match="--fewshot_head"):
            cli.check_supported(cli.parse_args(["--model", "am3", "--disable_cuda", "--dropout", "0", "--fewshot_head", "proto"]))
        for bad in ("0", "-1"):
            with pytest.raises(ValueError, match="--proto_scale"):
                cli.check_supported(cli.parse_args(meta + ["--proto_scale", bad]))
        for head in ([], ["--fewshot_head", "cosine"], ["--fewshot_head", "ridge"]):
            with pytest.raises(ValueError, match="--proto_scale_fixed"):
                cli.check_supported(cli.parse_args(["--model", "metabaseline", "--proto_scale_fixed"] + head + base))
        for ways in ("1", "65"):
            with pytest.raises(NotImplementedError, match="--num_ways"):
                cli.check_supported(cli.parse_args(meta + ["--num_ways", ways]))
        # the cosine head is asked nothing new
        cli.check_supported(cli.parse_args(["--model", "metabaseline"] + base))
    finally:
        engine.set_engine(old)


# ---- MetaBaseline ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("im_encoder", ["conv4", "resnet12"])
def test_metabaseline_state_dict_is_proto_scale_plus_the_backbone_of_pretrain_in_both_scale_modes(im_encoder):
    from fumi_amd.models.metabaseline import MetaBaseline, head_log
    from fumi_amd.models.pretrain import Pretrain
    from fumi_amd.utils import utils
    torch.manual_seed(5)
    kw = dict(image_size=16, image_channels=3, num_ways=3, head="proto")
    pre = Pretrain(im_encoder, image_size=16, image_channels=3, n_classes=6)
    conv = {k for k in pre.state_dict() if k.startswith("conv.")}
    learned = MetaBaseline(im_encoder, proto_scale=0.25, **kw)
    fixed = MetaBaseline(im_encoder, proto_scale_fixed=True, **kw)
    assert conv and set(learned.state_dict()) == set(fixed.state_dict()) == {"proto_scale"} | conv
    assert tuple(learned.state_dict()["proto_scale"].shape) == tuple(fixed.state_dict()["proto_scale"].shape) == (1,)
    # learned: the head parameter, in front of the backbone; fixed: a buffer no optimizer is handed
    assert learned.head_param() is learned.proto_scale and [n for n, _ in learned.named_parameters()][0] == "proto_scale"
    assert fixed.head_param() is None and all(n.startswith("conv.") for n, _ in fixed.named_parameters())
    assert "proto_scale" in dict(fixed.named_buffers()) and float(fixed.proto_scale) == 1.0
    assert head_log(learned) == {"proto_scale": 0.25} and head_log(fixed) == {"proto_scale": 1.0}
    # a fixed-scale checkpoint loads into a learned-scale model and back
    learned.load_state_dict(fixed.state_dict())
    assert float(learned.proto_scale) == 1.0 and isinstance(learned.proto_scale, torch.nn.Parameter)
    with torch.no_grad():
        learned.proto_scale.fill_(0.75)
    fixed.load_state_dict(learned.state_dict())
    assert float(fixed.proto_scale) == 0.75 and not isinstance(fixed.proto_scale, torch.nn.Parameter)
    # the backbone of a --model pretrain checkpoint
    names = utils.load_backbone_state(fixed, pre.state_dict())
    assert names == sorted(conv) and float(fixed.proto_scale) == 0.75
    # the other heads keep their keys
    assert set(MetaBaseline(im_encoder, image_size=16).state_dict()) == {"temp"} | conv
    assert set(MetaBaseline(im_encoder, image_size=16, head="ridge").state_dict()) == {"ridge"} | conv
    for bad in (dict(head="proto", proto_scale=0.0), dict(head="proto", proto_scale=-1.0), dict(head="cosine", proto_scale_fixed=True),
                dict(head="svm")):
        with pytest.raises(ValueError):
            MetaBaseline(im_encoder, image_size=16, **bad)


class ProtoOracleEngine(OracleEngine):
    """OracleEngine plus the prototypical head from the numpy restatement; records the forms it was asked for."""

    def __init__(self):
        self.forms = []

    def euclid_proto_step(self, feats_s, y_s, feats_q, y_q, alpha, need_grad=True, grad_scale=1.0, want_logits=False, dfeats_s=None,
                          dfeats_q=None, dalpha=None, n_way=None):
        self.forms.append("train" if need_grad else "forward")
        r = euclid_proto_ref(feats_s.numpy(), y_s.numpy(), feats_q.numpy(), y_q.numpy(), alpha.numpy(), n_way, grad_scale)
        f32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32))
        out = dict(loss=f32(r["loss"]).reshape(1), correct=f32(r["correct"]).reshape(1), preds=torch.as_tensor(r["preds"]),
                   logits=f32(r["logits"]) if want_logits else None, dfeats_s=None, dfeats_q=None, dalpha=None)
        if need_grad:
            out.update(dfeats_s=f32(r["dfeats_s"]), dfeats_q=f32(r["dfeats_q"]), dalpha=f32(r["dalpha"]).reshape(1))
            if dalpha is not None:
                dalpha.copy_(out["dalpha"]); out["dalpha"] = dalpha
        return out


def _episodic_batch(seed, B=2, N=3, K=2, Q=2, size=16):
    g = torch.Generator().manual_seed(seed)
    y_s = (torch.arange(N * K) % N).repeat(B, 1)
    y_q = (torch.arange(N * Q) % N).repeat(B, 1)
    x_s, x_q = torch.randn(B, N * K, 3, size, size, generator=g), torch.randn(B, N * Q, 3, size, size, generator=g)
    return {"train": ((None, None, x_s), y_s), "test": ((None, None, x_q), y_q)}


@pytest.mark.parametrize("fixed", [False, True])
def test_metabaseline_proto_step_on_a_host_engine_attaches_gradients_and_returns_the_head_loss(fixed):
    """The plumbing of evaluate() on the host: encode -> euclid_proto_step -> encode_bwd, one flat gradient buffer [proto_scale | conv.*
    | loss, acc] (learned scale) or [conv.* | loss, acc] (fixed scale), and the forward form for validation."""
    from fumi_amd import engine
    from fumi_amd.models.metabaseline import MetaBaseline
    eng = ProtoOracleEngine()
    old = engine.set_engine(eng)
    try:
        torch.manual_seed(9)
        model = MetaBaseline("conv4", image_size=16, image_channels=3, num_ways=3, head="proto", proto_scale=0.02, proto_scale_fixed=fixed)
        batch = _episodic_batch(13)
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        loss, acc = model.evaluate(batch, opt, None, "cpu", task="train")
        theta = [p.detach() for p in model.conv.theta()]
        f_s, f_q = eng.conv4_encode(batch["train"][0][2], batch["test"][0][2], theta)
        ref = euclid_proto_ref(f_s.numpy(), batch["train"][1].numpy(), f_q.numpy(), batch["test"][1].numpy(), np.float32(0.02), 3)
        assert eng.forms == ["train"]
        assert abs(float(loss) - ref["loss"]) <= 1e-6 * max(1.0, ref["loss"]) and abs(float(acc) - ref["correct"] / 12) <= 1e-7
        held = [p for grp in opt.param_groups for p in grp["params"]]
        if fixed:
            assert all(p is not model.proto_scale for p in held) and len(held) == len(model.conv.theta())
            assert model._flat.flat.numel() == sum(p.numel() for p in model.conv.theta()) + 2
            assert model.conv.theta()[0].grad.data_ptr() == model._flat.flat.data_ptr()
            assert abs(float(model._dscale) - ref["dalpha"]) <= 1e-6 * max(1.0, abs(ref["dalpha"]))
            assert getattr(model.proto_scale, "grad", None) is None and float(model.proto_scale) == np.float32(0.02)
        else:
            assert any(p is model.proto_scale for p in held)
            assert abs(float(model.proto_scale.grad) - ref["dalpha"]) <= 1e-6 * max(1.0, abs(ref["dalpha"]))
            assert model.proto_scale.grad.data_ptr() == model._flat.flat.data_ptr()          # in front, where temp sits
        for n, p in model.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        assert any(bool(p.grad.abs().max() > 0) for p in model.conv.theta())
        v_loss, v_acc = model.evaluate(batch, None, None, "cpu", task="val")
        assert eng.forms == ["train", "forward"] and not model.training
        assert abs(float(v_loss) - ref["loss"]) <= 1e-6 * max(1.0, ref["loss"]) and abs(float(v_acc) - ref["correct"] / 12) <= 1e-7
    finally:
        engine.set_engine(old)
