"""CPU suite of the ridge-regression head and --fewshot_head ridge: the float64 restatement
tests/ridge_head_ref.py against torch.autograd through torch.linalg.cholesky / cholesky_solve, the conditioning and the margins of the
GPU parity inputs, the support row that is left out, the flags and refusals, and the state_dict contract of MetaBaseline."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ridge_head_ref import (ALPHA, GRAD_SCALE, RHO, SHAPES, ST_CLASS_MISSING, ST_LABEL_RANGE, ST_NOT_POSDEF, case_inputs,
                            ridge_head_ref)

SMALL = (2, 7, 33, 3, 96)


# ---- the restatement of the head ------------------------------------------------------------------------------------------------
def _torch_head(f_s, y_s, f_q, y_q, rho, alpha, N, gs):
    """The head in torch float64 ops with autograd; rows whose label is out of range are masked the way the kernel drops them."""
    ys, yq = torch.as_tensor(y_s), torch.as_tensor(y_q)
    ok_s, ok_q = (ys >= 0) & (ys < N), (yq >= 0) & (yq < N)
    xs = torch.tensor(f_s, dtype=torch.float64, requires_grad=True)
    xq = torch.tensor(f_q, dtype=torch.float64, requires_grad=True)
    p = torch.tensor([rho, alpha], dtype=torch.float64, requires_grad=True)
    x = xs * ok_s[..., None]
    Y = F.one_hot(ys.clamp(0, N - 1), N).to(torch.float64) * ok_s[..., None]
    M = torch.bmm(x, x.transpose(1, 2)) + torch.exp(p[0]) * torch.eye(x.shape[1], dtype=torch.float64)
    A = torch.cholesky_solve(Y, torch.linalg.cholesky(M))
    z = p[1] * torch.bmm(xq, torch.bmm(x.transpose(1, 2), A))
    nll = F.cross_entropy(z.reshape(-1, N), yq.clamp(0, N - 1).reshape(-1), reduction="none")
    loss = (nll * ok_q.reshape(-1)).sum() / yq.numel()
    return xs, xq, p, z, loss, gs * loss


def _compare(f_s, y_s, f_q, y_q, N, status, tol=1e-10):
    ref = ridge_head_ref(f_s, y_s, f_q, y_q, (RHO, ALPHA), N, GRAD_SCALE)
    xs, xq, p, z, loss, obj = _torch_head(f_s, y_s, f_q, y_q, RHO, ALPHA, N, GRAD_SCALE)
    assert ref["status"] == status
    assert abs(ref["loss"] - float(loss.detach())) <= tol
    assert np.abs(ref["logits"] - z.detach().numpy()).max() <= tol
    dxs, dxq, dp = torch.autograd.grad(obj, [xs, xq, p])
    for k, want in (("dfeats_s", dxs), ("dfeats_q", dxq), ("dparams", dp)):
        e = np.abs(ref[k] - want.numpy()).max()
        print(f"{k}: largest difference to autograd {e:.3e}")
        assert e <= tol, k
    zz = ref["logits"]
    ok = (np.asarray(y_q) >= 0) & (np.asarray(y_q) < N)
    assert np.array_equal(ref["preds"], zz.argmax(-1)) and ref["correct"] == float(((zz.argmax(-1) == y_q) & ok).sum())
    return ref


@pytest.mark.parametrize("B,S,Qn,N,Fd", SHAPES)
def test_restatement_equals_autograd_and_the_inputs_are_well_conditioned(B, S, Qn, N, Fd):
    f_s, y_s, f_q, y_q = case_inputs(B, S, Qn, N, Fd)
    ref = _compare(f_s, y_s, f_q, y_q, N, 0)
    print(f"({B},{S},{Qn},{N},{Fd}): cond {ref['cond']:.3g}, smallest top-two margin {ref['margin'].min():.3g}")
    assert ref["cond"] <= 10.0                                                     # conditions on the inputs: a row that breaks one
    assert ref["margin"].min() > 1e-5                                              # gets another seed, not another bound
    if S > N:
        counts = np.stack([(y_s == n).sum(1) for n in range(N)], 1)
        assert (counts.max(1) > counts.min(1)).all()                               # unequal class counts


def test_restatement_equals_autograd_with_a_query_label_out_of_range():
    f_s, y_s, f_q, y_q = case_inputs(*SMALL)
    y_q[1, 20] = SMALL[3]
    ref = _compare(f_s, y_s, f_q, y_q, SMALL[3], ST_LABEL_RANGE)
    assert not ref["dfeats_q"][1, 20].any()


def test_restatement_equals_autograd_with_a_support_label_out_of_range():
    f_s, y_s, f_q, y_q = case_inputs(*SMALL)
    y_s[0, 6] = -1
    ref = _compare(f_s, y_s, f_q, y_q, SMALL[3], ST_LABEL_RANGE)
    assert not ref["dfeats_s"][0, 6].any() and not ref["A"][0, 6].any()


def test_restatement_equals_autograd_with_a_class_without_support():
    f_s, y_s, f_q, y_q = case_inputs(*SMALL)
    y_s[1][y_s[1] == 2] = 1                                                        # episode 1 has no row of class 2
    ref = _compare(f_s, y_s, f_q, y_q, SMALL[3], ST_CLASS_MISSING)
    assert not ref["logits"][1, :, 2].any() and not ref["W"][1, :, 2].any()


def test_a_support_row_left_out_gives_the_episode_with_that_row_deleted():
    B, S, Qn, N, Fd = 1, 7, 33, 3, 96
    f_s, y_s, f_q, y_q = case_inputs(B, S, Qn, N, Fd)
    y_s[0, 6] = N + 3
    full = ridge_head_ref(f_s, y_s, f_q, y_q, (RHO, ALPHA), N, GRAD_SCALE)
    sub = ridge_head_ref(f_s[:, :6], y_s[:, :6], f_q, y_q, (RHO, ALPHA), N, GRAD_SCALE)
    assert full["status"] == ST_LABEL_RANGE and sub["status"] == 0
    assert abs(full["loss"] - sub["loss"]) <= 1e-14
    for k in ("logits", "dfeats_q", "dparams"):
        assert np.abs(full[k] - sub[k]).max() <= 1e-14, k
    assert np.abs(full["dfeats_s"][:, :6] - sub["dfeats_s"]).max() <= 1e-14 and not full["dfeats_s"][0, 6].any()


def test_restatement_reports_a_matrix_that_is_not_positive_definite():
    f_s, y_s, f_q, y_q = case_inputs(*SMALL)
    f_s[1, 2, 5] = np.nan
    with np.errstate(all="ignore"):
        ref = ridge_head_ref(f_s, y_s, f_q, y_q, (RHO, ALPHA), SMALL[3], GRAD_SCALE)
    assert ref["status"] == ST_NOT_POSDEF


# ---- bindings, flags, refusals --------------------------------------------------------------------------------------------------
def test_the_binding_and_the_status_bit_exist():
    from fumi_amd import engine, hip
    assert callable(hip.ridge_head_step) and "fumi_hip_ridge_head_step" in hip.SYMBOLS
    assert hip.ST_NOT_POSDEF == ST_NOT_POSDEF == 8
    assert callable(engine.HipEngine.ridge_head_step)
    with pytest.raises(FloatingPointError):
        hip.raise_on_status(hip.ST_NOT_POSDEF)
    hip.raise_on_status(0)


def test_ridge_flags_parse_with_their_defaults_and_reach_the_model():
    from fumi_amd.utils import utils
    d = utils.parser().parse_args([])
    assert (d.fewshot_head, d.ridge_lambda, d.ridge_scale, d.pretrain_metric) == ("cosine", 50.0, 1.0, "euclidean")
    a = utils.parser().parse_args(["--model", "metabaseline", "--fewshot_head", "ridge", "--ridge_lambda", "20", "--ridge_scale", "3",
                                   "--im_encoder", "conv4", "--image_size", "16", "--num_ways", "3"])
    assert (a.fewshot_head, a.ridge_lambda, a.ridge_scale) == ("ridge", 20.0, 3.0)
    assert utils.parser().parse_args(["--pretrain_metric", "ridge"]).pretrain_metric == "ridge"
    with pytest.raises(SystemExit):
        utils.parser().parse_args(["--fewshot_head", "svm"])
    a.device = "cpu"
    model = utils.init_model(a, None, watch=False)
    assert model.head == "ridge" and tuple(model.ridge.shape) == (2,)
    assert abs(float(model.ridge[0]) - math.log(20.0)) <= 1e-6 and float(model.ridge[1]) == 3.0
    a.model, a.pretrain_metric, a.n_classes = "pretrain", "ridge", 6
    pre = utils.init_model(a, None, watch=False)
    assert (pre.metric, pre.ridge_lambda, pre.ridge_scale) == ("ridge", 20.0, 3.0)


def test_check_supported_refuses_what_the_ridge_head_cannot_run():
    from fumi_amd import engine
    from fumi_amd import main as cli
    from oracle_engine import OracleEngine
    old = engine.set_engine(OracleEngine())
    try:
        base = ["--disable_cuda", "--dataset", "synthetic-resident", "--im_encoder", "conv4"]
        meta = ["--model", "metabaseline", "--fewshot_head", "ridge"] + base
        cli.check_supported(cli.parse_args(meta))
        cli.check_supported(cli.parse_args(meta + ["--num_ways", "20", "--num_shots", "5"]))
        cli.check_supported(cli.parse_args(["--model", "pretrain", "--pretrain_metric", "ridge"] + base))
        with pytest.raises(ValueError, match="--fewshot_head"):
            cli.check_supported(cli.parse_args(["--model", "pretrain", "--fewshot_head", "ridge"] + base))
        with pytest.raises(ValueError, match="--fewshot_head"):
            cli.check_supported(cli.parse_args(["--model", "am3", "--disable_cuda", "--dropout", "0", "--fewshot_head", "ridge"]))
        for bad in ("0", "-1"):
            with pytest.raises(ValueError, match="--ridge_lambda"):
                cli.check_supported(cli.parse_args(meta + ["--ridge_lambda", bad]))
            with pytest.raises(ValueError, match="--ridge_scale"):
                cli.check_supported(cli.parse_args(meta + ["--ridge_scale", bad]))
        with pytest.raises(NotImplementedError, match="128"):
            cli.check_supported(cli.parse_args(meta + ["--num_ways", "26", "--num_shots", "5"]))
        with pytest.raises(NotImplementedError, match="128"):
            cli.check_supported(cli.parse_args(["--model", "pretrain", "--pretrain_metric", "ridge", "--num_ways", "43",
                                                "--num_shots", "3"] + base))
        # the cosine head takes the larger support set as before
        cli.check_supported(cli.parse_args(["--model", "metabaseline", "--num_ways", "26", "--num_shots", "5"] + base))
    finally:
        engine.set_engine(old)


@pytest.mark.parametrize("im_encoder", ["conv4", "resnet12"])
def test_metabaseline_state_dict_is_ridge_plus_the_backbone_and_cosine_keeps_temp(im_encoder):
    from fumi_amd.models.metabaseline import MetaBaseline, head_log
    torch.manual_seed(5)
    ridge = MetaBaseline(im_encoder, image_size=16, image_channels=3, num_ways=3, head="ridge", ridge_lambda=20.0, ridge_scale=2.0)
    cosine = MetaBaseline(im_encoder, image_size=16, image_channels=3, num_ways=3)
    conv = {k for k in cosine.state_dict() if k.startswith("conv.")}
    assert conv and set(cosine.state_dict()) == {"temp"} | conv and cosine.head == "cosine"
    assert set(ridge.state_dict()) == {"ridge"} | conv
    assert ridge.head_param() is ridge.ridge and cosine.head_param() is cosine.temp
    log = head_log(ridge)
    assert set(log) == {"ridge_lambda", "ridge_scale"} and abs(log["ridge_lambda"] - 20.0) <= 1e-5 and log["ridge_scale"] == 2.0
    assert head_log(cosine) == {"temp": 10.0}
    for kw in (dict(ridge_lambda=0.0), dict(ridge_scale=-1.0)):
        with pytest.raises(ValueError):
            MetaBaseline(im_encoder, image_size=16, head="ridge", **kw)
    with pytest.raises(ValueError):
        MetaBaseline(im_encoder, image_size=16, head="svm")


def test_metabaseline_ridge_step_on_a_host_engine_fills_the_flat_buffer(monkeypatch):
    """The plumbing of evaluate() on the host: encode -> ridge_head_step -> encode_bwd, one flat gradient buffer [ridge | conv.* | loss,
    acc], and the forward form for validation."""
    from fumi_amd import engine
    from fumi_amd.models.metabaseline import MetaBaseline
    from oracle_engine import OracleEngine

    class RidgeOracleEngine(OracleEngine):
        def ridge_head_step(self, feats_s, y_s, feats_q, y_q, params, need_grad=True, grad_scale=1.0, want_logits=False, dfeats_s=None,
                            dfeats_q=None, dparams=None, n_way=None):
            r = ridge_head_ref(feats_s.numpy(), y_s.numpy(), feats_q.numpy(), y_q.numpy(), params.numpy(), n_way, grad_scale)
            f32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32))
            out = dict(loss=f32(r["loss"]).reshape(1), correct=f32(r["correct"]).reshape(1), preds=torch.as_tensor(r["preds"]),
                       logits=None, dfeats_s=None, dfeats_q=None, dparams=None)
            if need_grad:
                out.update(dfeats_s=f32(r["dfeats_s"]), dfeats_q=f32(r["dfeats_q"]), dparams=f32(r["dparams"]))
                if dparams is not None:
                    dparams.copy_(out["dparams"]); out["dparams"] = dparams
            return out

    eng = RidgeOracleEngine()
    old = engine.set_engine(eng)
    try:
        torch.manual_seed(9)
        model = MetaBaseline("conv4", image_size=16, image_channels=3, num_ways=3, head="ridge", ridge_lambda=2.0, ridge_scale=3.0)
        g = torch.Generator().manual_seed(13)
        y_s, y_q = (torch.arange(6) % 3).repeat(2, 1), (torch.arange(6) % 3).repeat(2, 1)
        x_s, x_q = torch.randn(2, 6, 3, 16, 16, generator=g), torch.randn(2, 6, 3, 16, 16, generator=g)
        batch = {"train": ((None, None, x_s), y_s), "test": ((None, None, x_q), y_q)}
        loss, acc = model.evaluate(batch, None, None, "cpu", task="train")
        theta = [p.detach() for p in model.conv.theta()]
        f_s, f_q = eng.conv4_encode(x_s, x_q, theta)
        ref = ridge_head_ref(f_s.numpy(), y_s.numpy(), f_q.numpy(), y_q.numpy(), (math.log(2.0), 3.0), 3)
        assert abs(float(loss) - ref["loss"]) <= 1e-6 and abs(float(acc) - ref["correct"] / 12) <= 1e-7
        assert np.abs(model.ridge.grad.numpy() - ref["dparams"]).max() <= 1e-6 * max(1.0, np.abs(ref["dparams"]).max())
        assert model.ridge.grad.data_ptr() == model._flat.flat.data_ptr()
        for n, p in model.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        v_loss, v_acc = model.evaluate(batch, None, None, "cpu", task="val")
        assert abs(float(v_loss) - ref["loss"]) <= 1e-6 and abs(float(v_acc) - ref["correct"] / 12) <= 1e-7
    finally:
        engine.set_engine(old)
