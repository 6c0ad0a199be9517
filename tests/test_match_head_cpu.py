"""CPU suite of the Matching Networks head: the float64 reference tests/match_head_ref.py against torch.autograd
on the plain expression (log_softmax over the support rows, then logsumexp per class) at 1e-10; against tests/cos_proto_ref.py at one
valid row per class at 1e-12; the rows of da sum to zero; the conditions tests/test_match_head_gpu.py relies on (status 0 and margins
above 1e-5 at every parity shape, a class more than 110 below the row's largest in the saturated case); the flags, the model and the
refusals.  No GPU is needed."""
import numpy as np
import pytest
import torch

from cos_proto_ref import cos_proto_ref
from match_head_ref import (GRAD_SCALE, LIMITS, ONE_SHOT, SATURATED, SHAPES, ST_CLASS_MISSING, ST_LABEL_RANGE, TAU, TAU_SATURATED,
                            case_inputs, match_head_ref, saturated_inputs)
from oracle_engine import OracleEngine


def _autograd(f_s, y_s, f_q, y_q, tau, N, grad_scale):
    """The plain expression in float64: -log sum_{i: y_i = y_q} softmax_i(tau cos) as log_softmax over rows, logsumexp per class."""
    xs = torch.tensor(f_s, dtype=torch.float64, requires_grad=True)
    xq = torch.tensor(f_q, dtype=torch.float64, requires_grad=True)
    t = torch.tensor([tau], dtype=torch.float64, requires_grad=True)
    ys, yq = torch.as_tensor(y_s), torch.as_tensor(y_q)
    a = t * torch.einsum("bqf,bsf->bqs", torch.nn.functional.normalize(xq, dim=-1), torch.nn.functional.normalize(xs, dim=-1))
    logp = torch.log_softmax(a, dim=-1)                                           # [B, Qn, S]
    mask = torch.nn.functional.one_hot(ys, N).bool()                              # [B, S, N]
    per = logp[:, :, :, None].masked_fill(~mask[:, None, :, :], float("-inf"))
    logmass = torch.logsumexp(per, dim=2)                                         # [B, Qn, N] = z - logsumexp_n z
    loss = -logmass.gather(-1, yq[..., None]).mean()
    (grad_scale * loss).backward()
    return dict(loss=float(loss.detach()), logmass=logmass.detach().numpy(), dfeats_s=xs.grad.numpy(), dfeats_q=xq.grad.numpy(),
                dtau=float(t.grad))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_reference_equals_autograd_on_the_plain_expression(shape):
    f_s, y_s, f_q, y_q = case_inputs(*shape)
    ref = match_head_ref(f_s, y_s, f_q, y_q, TAU, shape[3], GRAD_SCALE)
    ag = _autograd(f_s, y_s, f_q, y_q, TAU, shape[3], GRAD_SCALE)
    assert abs(ref["loss"] - ag["loss"]) <= 1e-10
    z = ref["logits"]
    mx = z.max(-1, keepdims=True)
    logmass = z - (mx + np.log(np.exp(z - mx).sum(-1, keepdims=True)))
    assert np.abs(logmass - ag["logmass"]).max() <= 1e-10
    assert np.array_equal(ref["preds"], ag["logmass"].argmax(-1))
    for k in ("dfeats_s", "dfeats_q"):
        assert np.abs(ref[k] - ag[k]).max() <= 1e-10, k
    assert abs(ref["dtau"] - ag["dtau"]) <= 1e-10
    assert ref["da_rowsum_max"] <= 1e-15                                          # every row of da sums to zero


def test_one_valid_row_per_class_is_the_cosine_head():
    B, S, Qn, N, F = ONE_SHOT
    f_s, y_s, f_q, y_q = case_inputs(*ONE_SHOT)
    assert all(sorted(r) == list(range(N)) for r in y_s.tolist())
    ref = match_head_ref(f_s, y_s, f_q, y_q, TAU, N, GRAD_SCALE)
    cos = cos_proto_ref(f_s, y_s, f_q, y_q, TAU, N, GRAD_SCALE)
    assert abs(ref["loss"] - cos["loss"]) <= 1e-12 and abs(ref["dtau"] - cos["dtau"]) <= 1e-12
    for k in ("logits", "dfeats_s", "dfeats_q"):
        assert np.abs(ref[k] - cos[k]).max() <= 1e-12, k
    assert np.array_equal(ref["preds"], cos["preds"]) and ref["correct"] == cos["correct"]
    # ... and with further rows whose labels are out of range: still one VALID row per class
    f_s2 = np.concatenate([f_s, f_s[:, :2] + 1.0], axis=1)
    y_s2 = np.concatenate([y_s, np.full((B, 2), -1)], axis=1)
    y_s2[:, -1] = N + 2
    ref2 = match_head_ref(f_s2, y_s2, f_q, y_q, TAU, N, GRAD_SCALE)
    assert ref2["status"] == ST_LABEL_RANGE and not ref2["dfeats_s"][:, S:].any()
    assert np.abs(ref2["logits"] - cos["logits"]).max() <= 1e-12 and np.abs(ref2["dfeats_s"][:, :S] - cos["dfeats_s"]).max() <= 1e-12


def test_rows_of_da_sum_to_zero_and_left_out_rows_have_none():
    shape = SHAPES[0]
    f_s, y_s, f_q, y_q = (a.copy() for a in case_inputs(*shape))
    y_q[1, 20] = shape[3]
    y_s[0, 6] = -1
    ref = match_head_ref(f_s, y_s, f_q, y_q, TAU, shape[3], GRAD_SCALE, want_da=True)
    assert ref["status"] == ST_LABEL_RANGE
    assert np.abs(ref["da"].sum(-1)).max() <= 1e-15
    assert not ref["da"][1, 20].any() and not ref["da"][0, :, 6].any() and not ref["dfeats_q"][1, 20].any()
    assert abs(ref["dtau"] - (ref["da"] * ref["cos"]).sum()) <= 1e-15 and ref["dtau_abs"] >= abs(ref["dtau"])


def test_class_without_a_row_has_no_mass_and_its_queries_are_left_out():
    shape = SHAPES[0]
    f_s, y_s, f_q, y_q = (a.copy() for a in case_inputs(*shape))
    y_s[1][y_s[1] == 2] = 1
    ref = match_head_ref(f_s, y_s, f_q, y_q, TAU, shape[3], GRAD_SCALE)
    assert ref["status"] == ST_CLASS_MISSING and (y_q[1] == 2).any()
    assert np.isneginf(ref["logits"][1, :, 2]).all() and np.isfinite(ref["logits"][0]).all() and np.isfinite(ref["logits"][1, :, :2]).all()
    assert (ref["preds"][1] != 2).all() and not ref["dfeats_q"][1][y_q[1] == 2].any() and np.isfinite(ref["loss"])
    # the loss is that of the same episodes with those query rows' labels out of range
    y_q2 = y_q.copy(); y_q2[1][y_q[1] == 2] = -1
    ref2 = match_head_ref(f_s, y_s, f_q, y_q2, TAU, shape[3], GRAD_SCALE)
    assert ref2["loss"] == ref["loss"] and np.array_equal(ref2["dfeats_s"], ref["dfeats_s"])
    plain = match_head_ref(*case_inputs(*shape), TAU, shape[3], GRAD_SCALE)
    assert np.array_equal(plain["logits"][0], ref["logits"][0])                   # the other episode is untouched


def test_conditions_the_gpu_file_relies_on():
    for shape in SHAPES:
        f_s, y_s, f_q, y_q = case_inputs(*shape)
        ref = match_head_ref(f_s, y_s, f_q, y_q, TAU, shape[3], GRAD_SCALE)
        assert ref["status"] == 0 and ref["margin"].min() > 1e-5, shape          # no prediction is set aside
        counts = np.stack([np.bincount(r, minlength=shape[3]) for r in y_s])
        if shape[1] % shape[3]:
            assert counts.min() != counts.max(), shape                            # unequal shots
        if counts.max() > 1:
            assert any((np.diff(np.nonzero(r == r[0])[0]) > 1).any() for r in y_s), shape   # a class's rows are not contiguous
        # attention is neither uniform nor one-hot: the loss lies strictly between 0 and log S
        assert 1e-6 < ref["loss"] < np.log(shape[1]) or shape[2] == 1, shape
    # case C: for at least one query row a class lies more than 110 below the row's largest, finite -- beyond what fp32 exp can
    # represent relative to the maximum (exp(-104) underflows): log of a sum of globally normalised probabilities would give -inf
    f_s, y_s, f_q, y_q = saturated_inputs()
    assert f_s.shape == SATURATED[:2] + SATURATED[4:] and f_q.shape == (SATURATED[0], SATURATED[2], SATURATED[4])
    ref = match_head_ref(f_s, y_s, f_q, y_q, TAU_SATURATED, SATURATED[3], GRAD_SCALE)
    z = ref["logits"]
    assert ref["status"] == 0 and np.isfinite(z).all()
    assert ((z.max(-1) - z.min(-1)) > 110.0).any()
    assert LIMITS[1] == 512 and LIMITS[0] * LIMITS[2] == 65536


# ---- flags, the model's parameter, refusals -------------------------------------------------------------------------------------------
def test_matching_parses_and_reaches_the_model():
    from fumi_amd import main as cli
    from fumi_amd.utils import utils
    def parse(argv):
        a = cli.parse_args(argv)
        a.device = "cpu"
        return a
    d = cli.parse_args([])
    assert d.fewshot_head == "cosine" and d.pretrain_metric == "euclidean" and d.metric_temp == 10.0      # defaults unchanged
    flags = lambda p: [act.option_strings[0] for act in p._actions if act.option_strings and act.dest != "help"]
    assert flags(utils.match_parser()) == flags(utils.drop_parser())                                      # a choice, no flag
    for dest in ("fewshot_head", "pretrain_metric"):
        old = next(a for a in utils.drop_parser()._actions if a.dest == dest).choices
        new = next(a for a in utils.match_parser()._actions if a.dest == dest).choices
        assert "matching" not in old and list(new) == list(old) + ["matching"]                            # drop_parser() is what it was
    with pytest.raises(SystemExit):
        utils.drop_parser().parse_args(["--fewshot_head", "matching"])
    with pytest.raises(SystemExit):
        cli.parse_args(["--fewshot_head", "knn"])
    a = parse(["--model", "metabaseline", "--fewshot_head", "matching", "--metric_temp", "12.5", "--im_encoder", "conv4",
               "--image_size", "16", "--num_ways", "3"])
    model = utils.init_model(a, None, watch=False)
    assert model.head == "matching" and isinstance(model.temp, torch.nn.Parameter) and model.temp.tolist() == [12.5]
    assert model.head_param() is model.temp and "temp" in model.state_dict()
    plain = utils.init_model(parse(["--model", "metabaseline", "--im_encoder", "conv4", "--image_size", "16"]), None, watch=False)
    assert plain.head == "cosine" and sorted(plain.state_dict()) == sorted(model.state_dict())            # the same keys
    plain.load_state_dict(model.state_dict())
    assert plain.temp.tolist() == [12.5]
    from fumi_amd.models.metabaseline import MetaBaseline, head_log
    assert head_log(model) == {"temp": 12.5}
    with pytest.raises(ValueError, match="adapt=feat"):
        MetaBaseline("conv4", image_size=16, head="matching", adapt="feat")
    with pytest.raises(ValueError, match="transductive_steps"):
        MetaBaseline("conv4", image_size=16, head="matching", transductive_steps=2)
    assert MetaBaseline("conv4", image_size=16, head="matching", eval_head="logreg").eval_head == "logreg"
    p = parse(["--model", "pretrain", "--pretrain_metric", "matching", "--metric_temp", "7", "--im_encoder", "conv4", "--image_size", "16"])
    p.n_classes = 8                                                               # (set by the dataset in a run)
    pre = utils.init_model(p, None, watch=False)
    assert pre.metric == "matching" and pre.metric_temp == 7.0
    from fumi_amd.models.pretrain import Pretrain
    with pytest.raises(ValueError, match="matching"):
        Pretrain("conv4", image_size=16, n_classes=8, metric="matching", transductive_steps=2)
    from fumi_amd import engine, hip
    assert callable(engine.HipEngine.match_head_step) and callable(hip.match_head_step)
    assert "fumi_hip_match_head_step" in hip.SYMBOLS


def test_check_supported_refuses_what_the_matching_head_cannot_run():
    from fumi_amd import engine
    from fumi_amd import main as cli
    old = engine.set_engine(OracleEngine())
    try:
        base = ["--disable_cuda", "--dataset", "synthetic-resident", "--im_encoder", "conv4"]
        meta = ["--model", "metabaseline", "--fewshot_head", "matching"] + base
        cli.check_supported(cli.parse_args(meta))
        cli.check_supported(cli.parse_args(meta + ["--eval_head", "logreg"]))         # as the other heads: the logreg head evaluates
        cli.check_supported(cli.parse_args(meta + ["--num_ways", "64", "--num_shots", "8"]))                # S = 512
        cli.check_supported(cli.parse_args(["--model", "metabaseline", "--fewshot_head", "matching", "--disable_cuda", "--dataset",
                                            "synthetic-resident", "--im_encoder", "resnet12", "--drop_rate", "0.1"]))
        cli.check_supported(cli.parse_args(["--model", "pretrain", "--pretrain_metric", "matching", "--metric_temp", "5"] + base))
        with pytest.raises(ValueError, match="--fewshot_head"):
            cli.check_supported(cli.parse_args(["--model", "pretrain", "--fewshot_head", "matching"] + base))
        with pytest.raises(ValueError, match="--pretrain_metric"):
            cli.check_supported(cli.parse_args(["--model", "metabaseline", "--pretrain_metric", "matching"] + base))
        with pytest.raises(ValueError, match="--fewshot_adapt"):
            cli.check_supported(cli.parse_args(meta + ["--fewshot_adapt", "feat"]))
        with pytest.raises(ValueError, match="--transductive_steps"):
            cli.check_supported(cli.parse_args(meta + ["--transductive_steps", "3"]))
        with pytest.raises(ValueError, match="--transductive_steps"):
            cli.check_supported(cli.parse_args(["--model", "pretrain", "--pretrain_metric", "matching", "--transductive_steps", "3"] + base))
        with pytest.raises(ValueError, match="--metric_temp"):
            cli.check_supported(cli.parse_args(meta + ["--metric_temp", "0"]))
        with pytest.raises(NotImplementedError, match="512"):
            cli.check_supported(cli.parse_args(meta + ["--num_ways", "57", "--num_shots", "9"]))            # S = 513
        for ways in ("1", "65"):
            with pytest.raises(NotImplementedError, match="--num_ways"):
                cli.check_supported(cli.parse_args(meta + ["--num_ways", ways, "--num_shots", "1"]))
        cli.check_supported(cli.parse_args(["--model", "metabaseline"] + base))       # the cosine head is asked nothing new
    finally:
        engine.set_engine(old)
