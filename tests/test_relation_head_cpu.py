"""CPU suite of the Relation Network head (--fewshot_head relation): the float64 restatement
tests/relation_head_ref.py against torch.autograd on the plain expression, the conditions on the case table that
tests/test_relation_head_gpu.py relies on, the label rules, the parser layering, the model's parameters and every refusal."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle_engine import OracleEngine
from relation_head_ref import (GRAD_SCALE, LIMITS, LOSSES, ONE_SHOT, SHAPES, ST_CLASS_MISSING, ST_LABEL_RANGE, UNCERTAIN, case,
                               case_weights, relation_head_ref)

GRADS = ("dfeats_s", "dfeats_q", "dw1", "db1", "dw2", "db2")
_REFS = {}


def _ref(shape, loss):
    if (shape, loss) not in _REFS:
        inputs, w = case(shape)
        _REFS[(shape, loss)] = relation_head_ref(*inputs, *w, shape[3], loss, GRAD_SCALE)
    return _REFS[(shape, loss)]


def _autograd(inputs, w, N, loss, grad_scale):
    """The plain expression in float64: class means by a one-hot product, the concatenation (class mean, query) of every pair,
    Linear(2F, H), relu, Linear(H, 1), nn.MSELoss() of the sigmoid against the one-hot labels or cross_entropy."""
    f_s, y_s, f_q, y_q = (torch.as_tensor(a) for a in inputs)
    f_s, f_q = f_s.double().requires_grad_(True), f_q.double().requires_grad_(True)
    w1, b1, w2, b2 = (torch.as_tensor(t).double().requires_grad_(True) for t in w)
    B, S, F = f_s.shape
    Qn, H = f_q.shape[1], w1.shape[1]
    oh = Fn.one_hot(y_s, N).double()                                               # [B, S, N]
    c = torch.bmm(oh.transpose(1, 2), f_s) / oh.sum(1).clamp(min=1.0)[:, :, None]  # [B, N, F]
    pairs = torch.cat((c[:, None, :, :].expand(B, Qn, N, F), f_q[:, :, None, :].expand(B, Qn, N, F)), dim=-1)
    W = torch.cat((w1[0], w1[1]), dim=1)                                           # [H, 2F]
    z = Fn.linear(torch.relu(Fn.linear(pairs, W, b1)), w2[None, :], b2)[..., 0]    # [B, Qn, N]
    if loss == "mse":
        val = torch.nn.MSELoss()(torch.sigmoid(z), Fn.one_hot(y_q, N).double())
    else:
        val = Fn.cross_entropy(z.reshape(B * Qn, N), y_q.reshape(-1))
    (grad_scale * val).backward()
    return dict(loss=float(val.detach()), logits=z.detach().numpy(), preds=z.argmax(-1).numpy(), dfeats_s=f_s.grad.numpy(),
                dfeats_q=f_q.grad.numpy(), dw1=w1.grad.numpy(), db1=b1.grad.numpy(), dw2=w2.grad.numpy(), db2=b2.grad.numpy())


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape", SHAPES[:4], ids=str)
def test_reference_agrees_with_autograd_on_the_plain_expression(shape, loss):
    inputs, w = case(shape)
    ref, ag = _ref(shape, loss), _autograd(inputs, w, shape[3], loss, GRAD_SCALE)
    assert abs(ref["loss"] - ag["loss"]) <= 1e-10 * max(1.0, abs(ag["loss"]))
    assert np.array_equal(ref["preds"], ag["preds"])
    assert ref["correct"] == float((ag["preds"] == inputs[3]).sum())
    for k in ("logits",) + GRADS:
        e = float(np.abs(ref[k] - ag[k]).max())
        assert e <= 1e-10 * max(1.0, float(np.abs(ag[k]).max())), (k, e)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_case_table_meets_the_conditions_the_gpu_file_relies_on(shape):
    """Status 0, every prediction decided by more than 1e-5, few hidden units near the ReLU's kink, no saturated sigmoid."""
    (f_s, y_s, f_q, y_q), (w1, b1, w2, b2) = case(shape)
    B, S, Qn, N, F, H = shape
    assert f_s.shape == (B, S, F) and f_q.shape == (B, Qn, F) and w1.shape == (2, H, F) and w2.shape == (H,) and b2.tolist() == [np.float32(0.1)]
    k1 = 1.0 / math.sqrt(2.0 * F)
    assert np.abs(w1).max() <= k1 and np.abs(b1).max() <= k1 and np.abs(w2).max() <= 4.0 / math.sqrt(H)
    for loss in LOSSES:
        ref = _ref(shape, loss)
        assert ref["status"] == 0
        assert ref["margin"].min() > 1e-5, ref["margin"].min()
        pre = ref["pre"]
        assert float((np.abs(pre) <= UNCERTAIN * np.abs(pre).max()).mean()) <= 1e-3
        assert np.abs(ref["logits"]).max() <= 8.0
        assert np.array_equal(ref["pre"], ref["hid_q"][:, :, None, :] + ref["hid_s"][:, None, :, :])
    assert _ref(shape, "mse")["logits"] is not _ref(shape, "ce")["logits"] and np.array_equal(_ref(shape, "mse")["logits"], _ref(shape, "ce")["logits"])


def test_the_table_holds_the_cases_of_the_issue():
    assert SHAPES == [(2, 7, 33, 3, 96, 96), (4, 5, 1, 5, 64, 32), (1, 25, 75, 5, 640, 256), (3, 100, 17, 20, 160, 64),
                      (2, 129, 16, 64, 32, 1024), (1, 130, 5, 2, 2048, 32)]
    assert LIMITS == (2, 1024, 32768, 2, 32, 32) and LIMITS[0] * LIMITS[2] == 65536 and ONE_SHOT in SHAPES and GRAD_SCALE == 0.25
    w = case_weights(64, 32)
    rs = np.random.RandomState(31 * 32 + 64)
    assert np.array_equal(w[0], rs.uniform(-1.0 / math.sqrt(128.0), 1.0 / math.sqrt(128.0), (2, 32, 64)).astype(np.float32))


SMALL = SHAPES[0]


def _small():
    inputs, w = case(SMALL)
    return [a.copy() for a in inputs], w


@pytest.mark.parametrize("loss", LOSSES)
def test_label_rules(loss):
    N = SMALL[3]
    plain = _ref(SMALL, loss)
    # a query label out of range: the row adds nothing, the divisor stays
    (f_s, y_s, f_q, y_q), w = _small()
    y_q[1, 20] = N
    ref = relation_head_ref(f_s, y_s, f_q, y_q, *w, N, loss, GRAD_SCALE)
    assert ref["status"] == ST_LABEL_RANGE and not ref["dfeats_q"][1, 20].any()
    assert np.array_equal(ref["logits"], plain["logits"]) and ref["loss"] < plain["loss"]
    assert np.array_equal(ref["dfeats_q"][0], plain["dfeats_q"][0])
    # a support label out of range: left out of the count and the sum, a zero row of dfeats_s
    (f_s, y_s, f_q, y_q), w = _small()
    i0 = int(np.nonzero(y_s[0] == 0)[0][-1])
    y_s[0, i0] = -1
    ref = relation_head_ref(f_s, y_s, f_q, y_q, *w, N, loss, GRAD_SCALE)
    assert ref["status"] == ST_LABEL_RANGE and not ref["dfeats_s"][0, i0].any()
    keep = np.arange(SMALL[1]) != i0
    sub = relation_head_ref(f_s[:1, keep], y_s[:1, keep], f_q[:1], y_q[:1], *w, N, loss, GRAD_SCALE)
    assert np.allclose(sub["logits"][0], ref["logits"][0], rtol=0, atol=1e-13)
    assert np.array_equal(ref["logits"][1], plain["logits"][1])
    # a class without support: a zero prototype, U = b1
    (f_s, y_s, f_q, y_q), w = _small()
    y_s[1][y_s[1] == 2] = 1
    ref = relation_head_ref(f_s, y_s, f_q, y_q, *w, N, loss, GRAD_SCALE)
    assert ref["status"] == ST_CLASS_MISSING
    assert np.array_equal(ref["hid_s"][1, 2], w[1].astype(np.float64)) and np.isfinite(ref["logits"]).all()
    assert np.array_equal(ref["logits"][0], plain["logits"][0])


@pytest.mark.parametrize("loss", LOSSES)
def test_the_mask_argument_reproduces_the_default_and_only_moves_the_backward(loss):
    inputs, w = case(SMALL)
    plain = _ref(SMALL, loss)
    forced = relation_head_ref(*inputs, *w, SMALL[3], loss, GRAD_SCALE, mask=plain["pre"] > 0.0)
    for k in ("loss", "correct", "logits", "preds") + GRADS:
        assert np.array_equal(np.asarray(forced[k]), np.asarray(plain[k])), k
    other = relation_head_ref(*inputs, *w, SMALL[3], loss, GRAD_SCALE, mask=np.ones_like(plain["pre"], dtype=bool))
    assert np.array_equal(other["logits"], plain["logits"]) and other["loss"] == plain["loss"]
    assert not np.array_equal(other["dfeats_q"], plain["dfeats_q"])


# ---- flags, the model's parameters, refusals ---------------------------------------------------------------------------------------
def test_relation_parser_layers_on_match_parser():
    from fumi_amd import main as cli
    from fumi_amd.utils import utils
    flags = lambda p: [act.option_strings[0] for act in p._actions if act.option_strings and act.dest != "help"]
    assert flags(utils.relation_parser()) == flags(utils.match_parser()) + ["--relation_hidden", "--relation_loss"]
    choices = lambda p, dest: list(next(a for a in p._actions if a.dest == dest).choices)
    assert "relation" not in choices(utils.match_parser(), "fewshot_head")        # match_parser() is what it was
    assert choices(utils.relation_parser(), "fewshot_head") == choices(utils.match_parser(), "fewshot_head") + ["relation"]
    assert choices(utils.relation_parser(), "pretrain_metric") == choices(utils.match_parser(), "pretrain_metric")
    with pytest.raises(SystemExit):
        utils.match_parser().parse_args(["--fewshot_head", "relation"])
    with pytest.raises(SystemExit):
        cli.parse_args(["--pretrain_metric", "relation"])
    with pytest.raises(SystemExit):
        cli.parse_args(["--relation_loss", "hinge"])
    d = cli.parse_args([])
    assert d.fewshot_head == "cosine" and d.relation_hidden == 256 and d.relation_loss == "mse"
    assert utils.relation_config(d) is None
    a = cli.parse_args(["--fewshot_head", "relation", "--relation_hidden", "64", "--relation_loss", "ce"])
    assert utils.relation_config(a) == dict(hidden=64, loss="ce")


def test_the_model_owns_the_relation_module():
    from fumi_amd import main as cli
    from fumi_amd.models.metabaseline import MetaBaseline, head_log
    from fumi_amd.utils import utils
    torch.manual_seed(5)
    model = MetaBaseline("conv4", image_size=16, num_ways=3, head="relation", relation=dict(hidden=64, loss="ce"))
    F = model.conv.feature_dim
    keys = [k for k in model.state_dict() if not k.startswith("conv.")]
    assert keys == ["relation.w1", "relation.b1", "relation.w2", "relation.b2"] and not hasattr(model, "temp")
    assert model.head_param() is None and model.relation_loss == "ce"
    r = model.relation
    assert [tuple(t.shape) for t in r.tensors()] == [(2, 64, F), (64,), (64,), (1,)]
    assert [t is u for t, u in zip(r.tensors(), (r.w1, r.b1, r.w2, r.b2))] == [True] * 4
    k1, k2 = 1.0 / math.sqrt(2.0 * F), 1.0 / math.sqrt(64.0)
    assert 0.5 * k1 < float(r.w1.abs().max()) <= k1 and float(r.b1.abs().max()) <= k1
    assert 0.5 * k2 < float(r.w2.abs().max()) <= k2 and float(r.b2.abs().max()) <= k2
    assert abs(float(r.w1.mean())) < 0.05 * k1                                    # uniform about zero
    assert head_log(model) == {"relation_w2_norm": float(r.w2.detach().norm())}
    dflt = MetaBaseline("conv4", image_size=16, head="relation")
    assert dflt.relation.w1.shape == (2, 256, F) and dflt.relation_loss == "mse"
    a = cli.parse_args(["--model", "metabaseline", "--fewshot_head", "relation", "--relation_hidden", "96", "--im_encoder", "conv4",
                        "--image_size", "16", "--num_ways", "3"])
    a.device = "cpu"
    built = utils.init_model(a, None, watch=False)
    assert built.head == "relation" and built.relation.w2.shape == (96,) and built.relation_loss == "mse"
    assert MetaBaseline("conv4", image_size=16, head="relation", eval_head="logreg").eval_head == "logreg"
    plain = MetaBaseline("conv4", image_size=16)
    assert "temp" in plain.state_dict() and not any(k.startswith("relation.") for k in plain.state_dict())


def test_the_model_refuses_what_the_head_cannot_run():
    from fumi_amd.models.metabaseline import MetaBaseline
    with pytest.raises(ValueError, match="adapt=feat"):
        MetaBaseline("conv4", image_size=16, head="relation", adapt="feat")
    with pytest.raises(ValueError, match="transductive_steps"):
        MetaBaseline("conv4", image_size=16, head="relation", transductive_steps=2)
    for hidden in (0, 48, 1056):
        with pytest.raises(ValueError, match="hidden"):
            MetaBaseline("conv4", image_size=16, head="relation", relation=dict(hidden=hidden))
    with pytest.raises(ValueError, match="loss"):
        MetaBaseline("conv4", image_size=16, head="relation", relation=dict(loss="hinge"))
    with pytest.raises(ValueError, match="relation"):
        MetaBaseline("conv4", image_size=16, head="cosine", relation=dict(hidden=64))
    with pytest.raises(ValueError, match="feature width"):
        MetaBaseline("conv4", image_size=96, head="relation")                     # Conv4 at 96 x 96: F = 64 * 6 * 6 = 2304 > 2048
    assert MetaBaseline("conv4", image_size=84, head="relation").relation.w1.shape[2] == 1600


def test_check_supported_refuses_what_the_relation_head_cannot_run():
    from fumi_amd import engine
    from fumi_amd import main as cli
    old = engine.set_engine(OracleEngine())
    try:
        base = ["--disable_cuda", "--dataset", "synthetic-resident", "--im_encoder", "conv4"]
        meta = ["--model", "metabaseline", "--fewshot_head", "relation"] + base
        cli.check_supported(cli.parse_args(meta))
        cli.check_supported(cli.parse_args(meta + ["--relation_loss", "ce", "--relation_hidden", "1024"]))
        cli.check_supported(cli.parse_args(meta + ["--eval_head", "logreg"]))
        cli.check_supported(cli.parse_args(meta + ["--num_ways", "64", "--num_shots", "16"]))               # S = 1024
        cli.check_supported(cli.parse_args(["--model", "metabaseline", "--fewshot_head", "relation", "--disable_cuda", "--dataset",
                                            "synthetic-resident", "--im_encoder", "resnet12", "--drop_rate", "0.1"]))
        with pytest.raises(ValueError, match="--fewshot_head"):
            cli.check_supported(cli.parse_args(["--model", "pretrain", "--fewshot_head", "relation"] + base))
        with pytest.raises(ValueError, match="--fewshot_adapt"):
            cli.check_supported(cli.parse_args(meta + ["--fewshot_adapt", "feat"]))
        with pytest.raises(ValueError, match="--transductive_steps"):
            cli.check_supported(cli.parse_args(meta + ["--transductive_steps", "3"]))
        for hidden in ("0", "48", "1056"):
            with pytest.raises(NotImplementedError, match="--relation_hidden"):
                cli.check_supported(cli.parse_args(meta + ["--relation_hidden", hidden]))
        for ways in ("1", "65"):
            with pytest.raises(NotImplementedError, match="--num_ways"):
                cli.check_supported(cli.parse_args(meta + ["--num_ways", ways, "--num_shots", "1"]))
        with pytest.raises(NotImplementedError, match="1024"):
            cli.check_supported(cli.parse_args(meta + ["--num_ways", "41", "--num_shots", "25"]))           # S = 1025
        other = ["--model", "metabaseline"] + base
        with pytest.raises(ValueError, match="--relation_hidden"):
            cli.check_supported(cli.parse_args(other + ["--relation_hidden", "64"]))
        with pytest.raises(ValueError, match="--relation_loss"):
            cli.check_supported(cli.parse_args(other + ["--fewshot_head", "proto", "--relation_loss", "ce"]))
        cli.check_supported(cli.parse_args(other))                                    # the cosine head is asked nothing new
        cli.check_supported(cli.parse_args(other + ["--fewshot_head", "matching"]))
    finally:
        engine.set_engine(old)


def test_bindings_hold_the_symbol_and_the_engine_method():
    from fumi_amd import engine, hip
    assert "fumi_hip_relation_head_step" in hip.SYMBOLS
    assert callable(engine.HipEngine.relation_head_step) and callable(hip.relation_head_step)
    assert hip.RELATION_PARAMS == ("w1", "b1", "w2", "b2") and hip.RELATION_LOSSES == {"ce": 0, "mse": 1}
