"""CPU tests of the transductive prototype refinement: the float64 restatement tests/trans_proto_ref.py against
a plain torch float64 loop in the primal and, at steps = 0, against cos_proto_ref / euclid_proto_ref; its label rules; what the
parity inputs must fulfil for the GPU test to mean something (the refinement moves the logits, float32 can reach the bound, few rows
sit on a decision boundary); the flag, its refusals, and the models' plumbing on a host engine."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cos_proto_ref import cos_proto_ref
from euclid_proto_ref import euclid_proto_ref
from ridge_head_ref import SHAPES, case_inputs
from trans_proto_ref import (LIMIT_SHAPES, METRICS, SCALES, SHIFT, SHIFTED, ST_CLASS_MISSING, ST_LABEL_RANGE, STEPS, trans_proto_ref)

_REFS = {}


def _case(shape, metric, steps):
    key = (shape, metric, steps)
    if key not in _REFS:
        inputs = case_inputs(*shape)
        _REFS[key] = (inputs, trans_proto_ref(*inputs, shape[3], SCALES[metric], metric, steps))
    return _REFS[key]


def _torch_primal(f_s, y_s, f_q, n_way, scale, metric, steps):
    """The same iteration in torch float64 ops on the prototypes themselves: one-hot bmm sums, cdist / normalised bmm logits."""
    xs, xq = torch.as_tensor(f_s, dtype=torch.float64), torch.as_tensor(f_q, dtype=torch.float64)
    onehot = F.one_hot(torch.as_tensor(y_s), n_way).double()
    sums, count = torch.bmm(onehot.transpose(1, 2), xs), onehot.sum(1)

    def logits(protos):
        if metric == "cosine":
            return scale * torch.bmm(F.normalize(xq, dim=-1, eps=1e-12), F.normalize(protos, dim=-1, eps=1e-12).transpose(1, 2))
        return -scale * torch.cdist(xq, protos, compute_mode="donot_use_mm_for_euclid_dist") ** 2

    protos = sums / count.clamp(min=1.0)[..., None]
    for _ in range(steps):
        w = torch.softmax(logits(protos), dim=-1)
        protos = (sums + torch.bmm(w.transpose(1, 2), xq)) / (count + w.sum(1))[..., None]
    return logits(protos).numpy()


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_reference_is_the_torch_float64_loop_and_its_inputs_are_fit_for_the_gpu_test(shape, metric, steps):
    (f_s, y_s, f_q, y_q), ref = _case(shape, metric, steps)
    zmax = np.abs(ref["logits"]).max()
    z = _torch_primal(f_s, y_s, f_q, shape[3], SCALES[metric], metric, steps)
    assert np.abs(z - ref["logits"]).max() <= 1e-12 * zmax
    loss = float(F.cross_entropy(torch.as_tensor(z).reshape(-1, shape[3]), torch.as_tensor(y_q).reshape(-1)))
    assert abs(loss - ref["loss"]) <= 1e-12 * zmax
    assert np.array_equal(ref["preds"], z.argmax(-1)) and ref["correct"] == float((z.argmax(-1) == y_q).sum()) and ref["status"] == 0
    # the refinement does work on these inputs ...
    if steps >= 1:
        work = np.abs(ref["logits"] - ref["logits0"]).max() / zmax
        print(f"{shape} {metric} steps={steps}: max|z^T - z^0| = {work:.3f} max|z^T|")
        assert work >= 0.05
    # ... and the same iteration in plain float32 stays far inside the GPU test's bound of 1e-4
    r32 = trans_proto_ref(f_s, y_s, f_q, y_q, shape[3], SCALES[metric], metric, steps, dtype=np.float32)
    assert r32["logits"].dtype == np.float32
    e32 = np.abs(r32["logits"].astype(np.float64) - ref["logits"]).max() / zmax
    print(f"{shape} {metric} steps={steps}: float32 numpy within {e32:.2e} of float64")
    assert e32 <= 1e-5


def test_few_query_rows_of_the_gpu_table_sit_on_a_decision_boundary():
    """The GPU test sets aside rows whose float64 top-two gap is below 2e-4 max|z|: at most 2 per case, at most 1 % of all rows."""
    rows = near = 0
    for shape in SHAPES + LIMIT_SHAPES:
        for metric in METRICS:
            for steps in STEPS:
                _, ref = _case(shape, metric, steps)
                n = int((ref["margin"] < 2e-4 * np.abs(ref["logits"]).max()).sum())
                assert n <= 2, (shape, metric, steps, n)
                near += n; rows += ref["margin"].size
    print(f"{near} of {rows} rows within 2e-4 max|z| of a tie")
    assert near <= 0.01 * rows
    for shape in SHIFTED:                                                          # the offset cases compare every prediction
        f_s, y_s, f_q, y_q = case_inputs(*shape)
        ref = trans_proto_ref(f_s + np.float32(SHIFT), y_s, f_q + np.float32(SHIFT), y_q, shape[3], SCALES["euclid"], "euclid", 10)
        plain = _case(shape, "euclid", 10)[1]
        zmax = np.abs(ref["logits"]).max()
        assert ref["margin"].min() >= 2e-4 * zmax
        assert np.abs(ref["logits"] - plain["logits"]).max() <= 1e-5 * zmax        # (fp32 inputs plus 8.0 round: not 1e-10 as in float64)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_zero_steps_are_the_cosine_and_the_prototypical_head(shape):
    f_s, y_s, f_q, y_q = case_inputs(*shape)
    for metric, head in (("cosine", cos_proto_ref), ("euclid", euclid_proto_ref)):
        ref = _case(shape, metric, 0)[1]
        ind = head(f_s, y_s, f_q, y_q, SCALES[metric], shape[3])
        zmax = np.abs(ind["logits"]).max()
        assert np.abs(ref["logits"] - ind["logits"]).max() <= 1e-12 * zmax and abs(ref["loss"] - ind["loss"]) <= 1e-12 * zmax
        assert np.array_equal(ref["preds"], ind["preds"]) and ref["status"] == ind["status"] and ref["correct"] == ind["correct"]
        assert np.array_equal(ref["logits"], ref["logits0"])


SMALL = (2, 7, 33, 3, 96)


@pytest.mark.parametrize("metric", METRICS)
def test_query_label_out_of_range_drops_its_own_term_and_still_moves_the_prototypes(metric):
    f_s, y_s, f_q, y_q = (a.copy() for a in case_inputs(*SMALL))
    n, scale, rows = SMALL[3], SCALES[metric], SMALL[0] * SMALL[2]
    good = trans_proto_ref(f_s, y_s, f_q, y_q, n, scale, metric, 3)
    y_bad = y_q.copy(); y_bad[1, 20] = n
    bad = trans_proto_ref(f_s, y_s, f_q, y_bad, n, scale, metric, 3)
    assert bad["status"] == ST_LABEL_RANGE and good["status"] == 0
    assert np.array_equal(bad["logits"], good["logits"]) and np.array_equal(bad["preds"], good["preds"])     # no query label is read
    z = good["logits"][1, 20]
    term = np.log(np.exp(z - z.max()).sum()) + z.max() - z[y_q[1, 20]]
    assert abs((good["loss"] - bad["loss"]) * rows - term) <= 1e-12 * max(term, 1.0)                       # the divisor stays B * Qn
    assert bad["correct"] == good["correct"] - float(good["preds"][1, 20] == y_q[1, 20])
    # the row takes part in the refinement: without it the other rows of its episode get other logits
    keep = np.arange(SMALL[2]) != 20
    without = trans_proto_ref(f_s[1:], y_s[1:], f_q[1:, keep], y_q[1:, keep], n, scale, metric, 3)
    moved = np.abs(without["logits"][0] - bad["logits"][1, keep]).max() / np.abs(bad["logits"]).max()
    print(f"{metric}: the row with the bad label moves the other rows' logits by {moved:.2e} of max|z|")
    assert moved > 1e-6
    zero = trans_proto_ref(f_s[1:], y_s[1:], f_q[1:, keep], y_q[1:, keep], n, scale, metric, 0)
    assert np.abs(zero["logits"][0] - good["logits0"][1, keep]).max() <= 1e-12     # (at steps = 0 it moves nothing)


@pytest.mark.parametrize("metric", METRICS)
def test_support_label_out_of_range_gives_the_episode_without_that_row(metric):
    f_s, y_s, f_q, y_q = (a.copy() for a in case_inputs(*SMALL))
    y_s[0, 6], y_s[1, 6] = -1, SMALL[3] + 2                                       # (the extra row of class 0: every class keeps support)
    for steps in (0, 3):
        ref = trans_proto_ref(f_s, y_s, f_q, y_q, SMALL[3], SCALES[metric], metric, steps)
        sub = trans_proto_ref(f_s[:, :6], y_s[:, :6], f_q, y_q, SMALL[3], SCALES[metric], metric, steps)
        assert ref["status"] == ST_LABEL_RANGE and sub["status"] == 0
        assert np.abs(ref["logits"] - sub["logits"]).max() <= 1e-12 and abs(ref["loss"] - sub["loss"]) <= 1e-12
        assert np.array_equal(ref["preds"], sub["preds"])


@pytest.mark.parametrize("metric", METRICS)
def test_class_without_support_sets_the_bit_and_is_refined(metric):
    f_s, y_s, f_q, y_q = (a.copy() for a in case_inputs(*SMALL))
    y_s[1][y_s[1] == 2] = 1                                                       # episode 1 has no row of class 2
    zero = trans_proto_ref(f_s, y_s, f_q, y_q, SMALL[3], SCALES[metric], metric, 0)
    assert zero["status"] == ST_CLASS_MISSING and not zero["protos"][1, 2].any()
    want = 0.0 if metric == "cosine" else -SCALES[metric] * (f_q[1].astype(np.float64) ** 2).sum(-1)
    assert np.abs(zero["logits"][1, :, 2] - want).max() <= 1e-12
    ref = trans_proto_ref(f_s, y_s, f_q, y_q, SMALL[3], SCALES[metric], metric, 3)
    assert ref["status"] == ST_CLASS_MISSING and np.isfinite(ref["logits"]).all()
    w = np.exp(zero["logits"][1] - zero["logits"][1].max(-1, keepdims=True))
    w = (w / w.sum(-1, keepdims=True))[:, 2]
    one = trans_proto_ref(f_s, y_s, f_q, y_q, SMALL[3], SCALES[metric], metric, 1)
    assert np.abs(one["protos"][1, 2] - (w[:, None] * f_q[1]).sum(0) / w.sum()).max() <= 1e-12    # a mean of query rows alone
    assert np.abs(ref["protos"][1, 2]).max() > 0


def test_reference_refuses_an_unknown_metric():
    with pytest.raises(ValueError):
        trans_proto_ref(*case_inputs(*SHAPES[0]), 2, 1.0, "euclidean", 1)


# ---- flags and refusals ---------------------------------------------------------------------------------------------------------
def test_the_flag_parses_with_its_default_and_is_the_last_ridge_flag():
    from fumi_amd import main as cli
    from fumi_amd.utils import utils
    assert cli.parse_args([]).transductive_steps == 0
    assert utils.parser().parse_args(["--transductive_steps", "7"]).transductive_steps == 7
    assert utils._RIDGE_FLAGS[-1][0] == "--transductive_steps"
    assert [f for f, _ in utils._RIDGE_FLAGS[:-1]] == ["--fewshot_head", "--ridge_lambda", "--ridge_scale"]
    help_text = " ".join(utils.parser().format_help().split())
    assert "soft k-means refinement of the class prototypes on each validation / test episode's queries" in help_text
    with pytest.raises(SystemExit):
        utils.parser().parse_args(["--transductive_steps", "many"])
    a = utils.parser().parse_args(["--model", "metabaseline", "--transductive_steps", "4", "--im_encoder", "conv4", "--image_size", "16",
                                   "--num_ways", "3"])
    a.device = "cpu"
    assert utils.init_model(a, None, watch=False).transductive_steps == 4
    a.model, a.n_classes = "pretrain", 6
    assert utils.init_model(a, None, watch=False).transductive_steps == 4
    a.transductive_steps = 0
    assert utils.init_model(a, None, watch=False).transductive_steps == 0


def test_check_supported_refuses_what_the_transductive_head_cannot_run():
    from fumi_amd import engine
    from fumi_amd import main as cli
    from oracle_engine import OracleEngine
    old = engine.set_engine(OracleEngine())
    try:
        base = ["--disable_cuda", "--dataset", "synthetic-resident", "--im_encoder", "conv4"]
        meta, pre = ["--model", "metabaseline"] + base, ["--model", "pretrain"] + base
        on = ["--transductive_steps", "5"]
        for args in (meta, pre, meta + ["--fewshot_head", "proto"], meta + ["--fewshot_head", "proto", "--proto_scale_fixed"],
                     pre + ["--pretrain_metric", "cosine"]):
            cli.check_supported(cli.parse_args(args + on))
            cli.check_supported(cli.parse_args(args + ["--transductive_steps", "100"]))
            cli.check_supported(cli.parse_args(args + on + ["--num_ways", "20", "--num_shots", "5", "--num_shots_test", "15"]))
            for bad in ("-1", "101"):
                with pytest.raises(ValueError, match="--transductive_steps"):
                    cli.check_supported(cli.parse_args(args + ["--transductive_steps", bad]))
            # outside the kernel's limits: S + Qn = 20 * 37 > 512; Qn * N = 32 * 17 * 17 > 8192; N = 65
            with pytest.raises(NotImplementedError, match="512"):
                cli.check_supported(cli.parse_args(args + on + ["--num_ways", "20", "--num_shots", "5"]))
            with pytest.raises(NotImplementedError, match="8192"):
                cli.check_supported(cli.parse_args(args + on + ["--num_ways", "17", "--num_shots", "1", "--num_shots_test", "29"]))
            with pytest.raises(NotImplementedError, match="64"):
                cli.check_supported(cli.parse_args(args + on + ["--num_ways", "65", "--num_shots", "1", "--num_shots_test", "1"]))
        for args in (meta + ["--fewshot_head", "ridge"], meta + ["--eval_head", "logreg"], pre + ["--pretrain_metric", "ridge"],
                     pre + ["--pretrain_metric", "logreg"]):
            cli.check_supported(cli.parse_args(args))
            with pytest.raises(ValueError, match="--transductive_steps"):
                cli.check_supported(cli.parse_args(args + on))
        for model in (["--model", "am3", "--dropout", "0"], ["--model", "maml"], ["--model", "fumi"]):
            with pytest.raises(ValueError, match="--transductive_steps"):
                cli.check_supported(cli.parse_args(model + ["--disable_cuda"] + on))
            with pytest.raises(ValueError, match="--transductive_steps"):
                cli.check_supported(cli.parse_args(model + ["--disable_cuda", "--transductive_steps", "-1"]))
        # with the flag at 0 nothing is asked: the inductive heads take the larger episodes as before
        cli.check_supported(cli.parse_args(meta + ["--num_ways", "20", "--num_shots", "5"]))
        cli.check_supported(cli.parse_args(pre + ["--num_ways", "20", "--num_shots", "5"]))
    finally:
        engine.set_engine(old)


def test_models_refuse_the_heads_that_have_no_prototypes_and_keep_their_state_dict():
    from fumi_amd.models.metabaseline import MetaBaseline, head_log
    from fumi_amd.models.pretrain import Pretrain
    kw = dict(image_size=16, image_channels=3, num_ways=3)
    for extra in (dict(head="ridge"), dict(eval_head="logreg")):
        MetaBaseline("conv4", **kw, **extra)
        with pytest.raises(ValueError):
            MetaBaseline("conv4", **kw, **extra, transductive_steps=2)
    for metric in ("ridge", "logreg"):
        Pretrain("conv4", **kw, n_classes=6, metric=metric)
        with pytest.raises(ValueError):
            Pretrain("conv4", **kw, n_classes=6, metric=metric, transductive_steps=2)
    for bad in (-1, 101):
        with pytest.raises(ValueError):
            MetaBaseline("conv4", **kw, transductive_steps=bad)
        with pytest.raises(ValueError):
            Pretrain("conv4", **kw, n_classes=6, transductive_steps=bad)
    for extra in (dict(), dict(head="proto"), dict(head="proto", proto_scale_fixed=True)):
        torch.manual_seed(5)
        a = MetaBaseline("conv4", **kw, **extra)
        torch.manual_seed(5)
        b = MetaBaseline("conv4", **kw, **extra, transductive_steps=4)
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        assert "transductive_steps" not in head_log(a) and head_log(b)["transductive_steps"] == 4
        assert {k: v for k, v in head_log(b).items() if k != "transductive_steps"} == head_log(a)
    for metric in ("euclidean", "cosine"):
        torch.manual_seed(5)
        a = Pretrain("conv4", **kw, n_classes=6, metric=metric)
        torch.manual_seed(5)
        b = Pretrain("conv4", **kw, n_classes=6, metric=metric, transductive_steps=4)
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


class _Reached(Exception):
    pass


def test_few_shot_of_both_models_calls_the_head_on_a_host_engine():
    """The plumbing on the host: encode -> trans_proto_step with the model's metric, its scale tensor and its number of steps; never
    with the flag at 0, never from a training step."""
    from fumi_amd import engine
    from fumi_amd.models.metabaseline import MetaBaseline
    from fumi_amd.models.pretrain import Pretrain
    from oracle_engine import OracleEngine
    calls = []

    class TransOracleEngine(OracleEngine):
        def trans_proto_step(self, feats_s, y_s, feats_q, y_q, scale, metric, steps, want_logits=False, n_way=None):
            calls.append(dict(metric=metric, steps=steps, scale=scale))
            r = trans_proto_ref(feats_s.numpy(), y_s.numpy(), feats_q.numpy(), y_q.numpy(), n_way, scale.numpy(), metric, steps)
            f32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32))
            return dict(loss=f32(r["loss"]).reshape(1), correct=f32(r["correct"]).reshape(1), preds=torch.as_tensor(r["preds"]), logits=None)

        def _inductive(self, name):                  # (the oracle engine has no inductive head: reaching one is what the test asks)
            calls.append(name)
            raise _Reached()

        def cos_proto_step(self, *args, **kw):
            self._inductive("cos_proto_step")

        def euclid_proto_step(self, *args, **kw):
            self._inductive("euclid_proto_step")

        def proto_reduce(self, *args, **kw):
            self._inductive("proto_reduce")

    eng = TransOracleEngine()
    old = engine.set_engine(eng)
    try:
        g = torch.Generator().manual_seed(13)
        y_s, y_q = (torch.arange(6) % 3).repeat(2, 1), (torch.arange(6) % 3).repeat(2, 1)
        x_s, x_q = torch.randn(2, 6, 3, 16, 16, generator=g), torch.randn(2, 6, 3, 16, 16, generator=g)
        batch = {"train": ((None, None, x_s), y_s), "test": ((None, None, x_q), y_q)}
        kw = dict(image_size=16, image_channels=3, num_ways=3)
        torch.manual_seed(9)
        # (model, metric of the call, value of the scale, the model's own tensor the scale must be | None, the inductive call at 0)
        table = [
            (lambda t: MetaBaseline("conv4", **kw, init_temp=7.0, transductive_steps=t), "cosine", 7.0, "temp", "cos_proto_step"),
            (lambda t: MetaBaseline("conv4", **kw, head="proto", proto_scale=0.5, transductive_steps=t), "euclid", 0.5, "proto_scale",
             "euclid_proto_step"),
            (lambda t: MetaBaseline("conv4", **kw, head="proto", proto_scale=0.25, proto_scale_fixed=True, transductive_steps=t), "euclid",
             0.25, "proto_scale", "euclid_proto_step"),
            (lambda t: Pretrain("conv4", **kw, n_classes=6, metric="cosine", metric_temp=12.0, transductive_steps=t), "cosine", 12.0, None,
             "cos_proto_step"),
            (lambda t: Pretrain("conv4", **kw, n_classes=6, metric="euclidean", transductive_steps=t), "euclid", 1.0, None, "proto_reduce"),
        ]
        for make, metric, value, own, inductive in table:
            model = make(3).eval()
            calls.clear()
            v_loss, v_acc = model.evaluate(batch, None, None, "cpu", task="val")
            assert len(calls) == 1 and calls[0]["metric"] == metric and calls[0]["steps"] == 3
            scale = calls[0]["scale"]
            assert scale.shape == (1,) and scale.dtype == torch.float32 and float(scale) == value and not scale.requires_grad
            if own is not None:
                assert scale.data_ptr() == getattr(model, own).data_ptr()          # the parameter / buffer itself, no copy
            model.evaluate(batch, None, None, "cpu", task="test")
            assert len(calls) == 2 and calls[1]["scale"].data_ptr() == scale.data_ptr()   # (a fixed scale is made once)
            theta = [p.detach() for p in model.conv.theta()]
            f_s, f_q = eng.conv4_encode(x_s, x_q, theta)
            ref = trans_proto_ref(f_s.numpy(), y_s.numpy(), f_q.numpy(), y_q.numpy(), 3, value, metric, 3)
            assert abs(float(v_loss) - ref["loss"]) <= 1e-6 * max(1.0, abs(ref["loss"])) and abs(float(v_acc) - ref["correct"] / 12) <= 1e-7
            # with the flag at 0 the model takes today's path and the new head is never called
            calls.clear()
            with pytest.raises(_Reached):
                make(0).eval().evaluate(batch, None, None, "cpu", task="val")
            assert calls == [inductive]
        # training keeps the model's own head, whatever the flag says
        for make, _, _, _, inductive in table[:3]:
            calls.clear()
            with pytest.raises(_Reached):
                make(3).evaluate(batch, None, None, "cpu", task="train")
            assert calls == [inductive]
    finally:
        engine.set_engine(old)
