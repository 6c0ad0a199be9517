"""CPU checks of the logistic-regression head: the float64 restatement tests/logreg_head_ref.py (the dual
iteration the kernel runs) against heavy-ball descent on the primal objective under torch.autograd, the conditions the GPU tests'
inputs must meet, the status semantics, the flags and refusals, and the models' plumbing through the test-only oracle engine."""
import numpy as np
import pytest
import torch

from logreg_head_ref import (C_REG, CASES, LR, MOMENTUM, SHAPES, ST_CLASS_MISSING, ST_LABEL_RANGE, case_inputs, logreg_head_ref)

MARGIN = 1e-5


def _primal_autograd(f_s, y_s, f_q, n_way, steps, lr, momentum, C, normalize):
    """T steps of heavy-ball descent on f(W, b) = (1/n) sum CE(W^T x~ + b, y) + (wd/2) |W|^2 from zero, float64, gradients from
    autograd; returns the query logits [B,Qn,N] and the final (W, b) per episode."""
    xs, xq = torch.as_tensor(f_s, dtype=torch.float64), torch.as_tensor(f_q, dtype=torch.float64)
    ys = torch.as_tensor(y_s)
    if normalize:
        xs = xs / xs.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        xq = xq / xq.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    B, S, F = xs.shape
    out = []
    for e in range(B):
        n = S
        wd = 1.0 / (C * n)
        W = torch.zeros(F, n_way, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(n_way, dtype=torch.float64, requires_grad=True)
        VW, Vb = torch.zeros_like(W), torch.zeros_like(b)
        for _ in range(steps):
            f = torch.nn.functional.cross_entropy(xs[e] @ W + b, ys[e], reduction="sum") / n + 0.5 * wd * (W * W).sum()
            gW, gb = torch.autograd.grad(f, (W, b))
            VW, Vb = momentum * VW + gW, momentum * Vb + gb
            with torch.no_grad():
                W -= lr * VW
                b -= lr * Vb
        out.append((xq[e] @ W + b).detach())
    return torch.stack(out).numpy()


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_the_dual_restatement_is_heavy_ball_descent_on_the_primal_objective(normalize, momentum):
    for shape, steps in (((2, 7, 33, 3, 96), 25), ((1, 25, 17, 5, 1600), 12), ((1, 33, 16, 3, 32), 25)):
        f_s, y_s, f_q, y_q = case_inputs(*shape)
        N = shape[3]
        ref = logreg_head_ref(f_s, y_s, f_q, y_q, N, steps=steps, lr=LR, momentum=momentum, C=C_REG, normalize=normalize)
        z = _primal_autograd(f_s, y_s, f_q, N, steps, LR, momentum, C_REG, normalize)
        err = np.abs(z - ref["logits"]).max()
        zt = torch.as_tensor(z).reshape(-1, N)
        loss = float(torch.nn.functional.cross_entropy(zt, torch.as_tensor(y_q).reshape(-1)))
        print(f"{shape} normalize={normalize} momentum={momentum}: logits {err:.2e}, loss {abs(loss - ref['loss']):.2e}")
        assert err <= 1e-10 and abs(loss - ref["loss"]) <= 1e-10
        assert np.array_equal(ref["preds"], z.argmax(-1)) and ref["status"] == 0


def test_the_gradient_norm_falls_as_the_fit_runs():
    f_s, y_s, f_q, y_q = case_inputs(*SHAPES[3])
    g = [logreg_head_ref(f_s, y_s, f_q, y_q, 5, steps=t)["grad_norm"] for t in (1, 10, 100, 400)]
    print("gradient norms at T = 1, 10, 100, 400:", g)
    assert g[0] > g[1] > g[2] > g[3] and g[3] < 1e-3 * g[0]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-T{c[1]}-m{c[2]}-{'norm' if c[3] else 'raw'}")
def test_the_gpu_cases_meet_their_conditions(case):
    """Every top-two margin of the float64 logits exceeds 1e-5 (no query row of the GPU tests is set aside), and a plain float32 numpy
    evaluation of the same iteration is within 1e-5 of them, relative to their largest magnitude."""
    shape, steps, momentum, normalize = case
    inp = case_inputs(*shape)
    ref = logreg_head_ref(*inp, shape[3], steps=steps, momentum=momentum, normalize=normalize)
    f32 = logreg_head_ref(*inp, shape[3], steps=steps, momentum=momentum, normalize=normalize, dtype=np.float32)
    err = np.abs(f32["logits"] - ref["logits"]).max() / np.abs(ref["logits"]).max()
    print(f"{case}: smallest margin {ref['margin'].min():.3e}, float32 error {err:.3e}, gradient norm {ref['grad_norm']:.3e}")
    assert ref["status"] == 0 and np.isfinite(ref["logits"]).all()
    assert ref["margin"].min() > MARGIN
    assert err <= 1e-5


def test_status_semantics_of_the_restatement():
    shape = (2, 7, 33, 3, 96)
    f_s, y_s, f_q, y_q = case_inputs(*shape)
    clean = logreg_head_ref(f_s, y_s, f_q, y_q, 3, steps=20)
    # a support row left out: the same as the episode without that row, the other episode untouched, n one smaller
    ys = y_s.copy(); ys[0, 6] = -1
    out = logreg_head_ref(f_s, ys, f_q, y_q, 3, steps=20)
    assert out["status"] == ST_LABEL_RANGE and not out["A"][0, 6].any()
    cut = logreg_head_ref(f_s[:1, :6], y_s[:1, :6], f_q[:1], y_q[:1], 3, steps=20)
    assert np.abs(out["logits"][0] - cut["logits"][0]).max() <= 1e-12
    assert np.array_equal(out["logits"][1], clean["logits"][1])
    assert np.abs(out["logits"][0] - clean["logits"][0]).max() > 1e-6
    # a query row dropped: the logits stay, the row leaves the loss and the count, the divisor stays B * Qn
    yq = y_q.copy(); yq[1, 20] = 3
    out = logreg_head_ref(f_s, y_s, f_q, yq, 3, steps=20)
    assert out["status"] == ST_LABEL_RANGE and np.array_equal(out["logits"], clean["logits"])
    z = clean["logits"][1, 20]
    row = np.log(np.exp(z - z.max()).sum()) + z.max() - z[y_q[1, 20]]
    assert abs(out["loss"] - (clean["loss"] - row / 66)) <= 1e-12
    assert out["correct"] == clean["correct"] - float(clean["preds"][1, 20] == y_q[1, 20])
    # a class without support: fitted like any class, its logit pushed down
    ys = y_s.copy(); ys[1][ys[1] == 2] = 1
    out = logreg_head_ref(f_s, ys, f_q, y_q, 3, steps=20)
    assert out["status"] == ST_CLASS_MISSING
    assert (out["logits"][1, :, 2] < out["logits"][1, :, :2].max(-1)).all() and (out["b"][1, 2] < 0)
    assert not (out["preds"][1] == 2).any()


# ---- flags and refusals ---------------------------------------------------------------------------------------------------------
def test_logreg_flags_parse_with_their_defaults_and_sit_beside_the_ridge_flags():
    from fumi_amd.utils import utils
    d = utils.parser().parse_args([])
    assert (d.logreg_steps, d.logreg_lr, d.logreg_momentum, d.logreg_C, d.logreg_raw, d.eval_head) == (100, 1.0, 0.9, 1.0, False, "train")
    assert utils.logreg_config(d) == dict(steps=100, lr=1.0, momentum=0.9, C=1.0, normalize=True) == utils.logreg_config(None)
    a = utils.parser().parse_args(["--model", "metabaseline", "--eval_head", "logreg", "--logreg_steps", "30", "--logreg_lr", "0.5",
                                   "--logreg_momentum", "0.5", "--logreg_C", "10", "--logreg_raw", "--im_encoder", "conv4",
                                   "--image_size", "16", "--num_ways", "3"])
    assert utils.logreg_config(a) == dict(steps=30, lr=0.5, momentum=0.5, C=10.0, normalize=False)
    assert utils.parser().parse_args(["--pretrain_metric", "logreg"]).pretrain_metric == "logreg"
    with pytest.raises(SystemExit):
        utils.parser().parse_args(["--eval_head", "svm"])
    assert [f for f, _ in utils._LOGREG_FLAGS] == ["--logreg_steps", "--logreg_lr", "--logreg_momentum", "--logreg_C", "--logreg_raw",
                                                   "--eval_head"]
    flags = [act.option_strings[0] for act in utils.parser()._actions if act.option_strings and act.dest != "help"]
    n_f, n_r, n_l = len(utils._FLAGS), len(utils._RIDGE_FLAGS), len(utils._LOGREG_FLAGS)
    assert flags[:n_f] == [f for f, _ in utils._FLAGS]                               # the reference's flag surface stays in front
    assert flags[n_f + n_r:n_f + n_r + n_l] == [f for f, _ in utils._LOGREG_FLAGS]
    a.device = "cpu"
    model = utils.init_model(a, None, watch=False)
    assert model.eval_head == "logreg" and model.head == "cosine" and model.logreg == utils.logreg_config(a)
    a.model, a.pretrain_metric, a.n_classes = "pretrain", "logreg", 6
    pre = utils.init_model(a, None, watch=False)
    assert pre.metric == "logreg" and pre.logreg == utils.logreg_config(a)
    help_text = utils.parser().format_help()
    for flag in ("--logreg_steps", "--logreg_lr", "--logreg_momentum", "--logreg_C", "--logreg_raw"):
        assert flag in help_text
    assert "[--model metabaseline] the classifier of validation" in " ".join(help_text.split())


def test_check_supported_refuses_what_the_logreg_head_cannot_run():
    from fumi_amd import engine
    from fumi_amd import main as cli
    from oracle_engine import OracleEngine
    old = engine.set_engine(OracleEngine())
    try:
        base = ["--disable_cuda", "--dataset", "synthetic-resident", "--im_encoder", "conv4"]
        meta = ["--model", "metabaseline", "--eval_head", "logreg"] + base
        pre = ["--model", "pretrain", "--pretrain_metric", "logreg"] + base
        cli.check_supported(cli.parse_args(meta))
        cli.check_supported(cli.parse_args(meta + ["--fewshot_head", "ridge", "--num_ways", "20", "--num_shots", "5"]))
        cli.check_supported(cli.parse_args(pre))
        cli.check_supported(cli.parse_args(pre + ["--logreg_raw", "--logreg_lr", "50"]))          # no bound without the normalisation
        cli.check_supported(cli.parse_args(pre + ["--logreg_lr", "3.1"]))                         # 3.1 * (1 + 1/25) < 3.8
        with pytest.raises(ValueError, match="--eval_head"):
            cli.check_supported(cli.parse_args(["--model", "pretrain", "--eval_head", "logreg"] + base))
        with pytest.raises(ValueError, match="--eval_head"):
            cli.check_supported(cli.parse_args(["--model", "am3", "--disable_cuda", "--dropout", "0", "--eval_head", "logreg"]))
        with pytest.raises(ValueError, match="--pretrain_metric"):
            cli.check_supported(cli.parse_args(["--model", "metabaseline", "--pretrain_metric", "logreg"] + base))
        for args in (meta, pre):
            with pytest.raises(NotImplementedError, match="128"):
                cli.check_supported(cli.parse_args(args + ["--num_ways", "26", "--num_shots", "5"]))
            with pytest.raises(NotImplementedError, match="64"):
                cli.check_supported(cli.parse_args(args + ["--num_ways", "65", "--num_shots", "1"]))
            for flag, bad in (("--logreg_steps", "0"), ("--logreg_steps", "10001"), ("--logreg_lr", "0"), ("--logreg_lr", "-1"),
                              ("--logreg_momentum", "1"), ("--logreg_momentum", "-0.1"), ("--logreg_C", "0"), ("--logreg_C", "-2")):
                with pytest.raises(ValueError, match=flag):
                    cli.check_supported(cli.parse_args(args + [flag, bad]))
            # lr (1 + wd) >= 2 (1 + momentum): 3.8 at the defaults, 2 without momentum; the message names the curvature bound
            with pytest.raises(ValueError, match="curvature.*at most 1"):
                cli.check_supported(cli.parse_args(args + ["--logreg_lr", "3.7"]))                # 3.7 * 1.04 = 3.848
            with pytest.raises(ValueError, match="can diverge"):
                cli.check_supported(cli.parse_args(args + ["--logreg_lr", "2", "--logreg_momentum", "0"]))
        # the cosine head takes the larger support set as before, and nothing is asked of runs without the head
        cli.check_supported(cli.parse_args(["--model", "metabaseline", "--num_ways", "26", "--num_shots", "5"] + base))
        stray = ["--logreg_steps", "0", "--logreg_lr", "-1", "--logreg_momentum", "1", "--logreg_C", "0"]
        cli.check_supported(cli.parse_args(["--model", "metabaseline"] + base + stray))
        cli.check_supported(cli.parse_args(["--model", "pretrain"] + base + stray))
        a = cli.parse_args(["--model", "pretrain", "--image_size", "16"] + base + stray)
        a.device, a.n_classes = "cpu", 6
        from fumi_amd.utils import utils
        assert utils.init_model(a, None, watch=False).logreg == utils.logreg_config(None)
    finally:
        engine.set_engine(old)


def test_metabaseline_state_dict_does_not_depend_on_the_evaluation_head():
    from fumi_amd.models.metabaseline import MetaBaseline
    for head in ("cosine", "ridge"):
        torch.manual_seed(5)
        a = MetaBaseline("conv4", image_size=16, image_channels=3, num_ways=3, head=head, eval_head="train")
        torch.manual_seed(5)
        b = MetaBaseline("conv4", image_size=16, image_channels=3, num_ways=3, head=head, eval_head="logreg",
                         logreg=dict(steps=7, lr=0.5, momentum=0.0, C=2.0, normalize=False))
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        assert b.eval_head == "logreg" and b.logreg["steps"] == 7 and a.logreg["steps"] == 100
    with pytest.raises(ValueError):
        MetaBaseline("conv4", image_size=16, eval_head="svm")
    with pytest.raises(ValueError):
        MetaBaseline("conv4", image_size=16, eval_head="logreg", logreg=dict(steps=0))


class _Reached(Exception):
    pass


def test_few_shot_of_both_models_calls_the_head_on_a_host_engine():
    """The plumbing on the host: encode -> logreg_head_step at the model's fixed hyper-parameters, for Pretrain(metric="logreg") and
    MetaBaseline(eval_head="logreg"); the training step of the latter keeps the model's own head."""
    from fumi_amd import engine
    from fumi_amd.models.metabaseline import MetaBaseline
    from fumi_amd.models.pretrain import Pretrain
    from oracle_engine import OracleEngine
    calls = []

    class LogregOracleEngine(OracleEngine):
        def logreg_head_step(self, feats_s, y_s, feats_q, y_q, steps=100, lr=1.0, momentum=0.9, C=1.0, normalize=True, want_logits=False,
                             n_way=None):
            calls.append(dict(steps=steps, lr=lr, momentum=momentum, C=C, normalize=normalize))
            r = logreg_head_ref(feats_s.numpy(), y_s.numpy(), feats_q.numpy(), y_q.numpy(), n_way, steps=steps, lr=lr, momentum=momentum,
                                C=C, normalize=normalize)
            f32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32))
            return dict(loss=f32(r["loss"]).reshape(1), correct=f32(r["correct"]).reshape(1), preds=torch.as_tensor(r["preds"]), logits=None)

        def cos_proto_step(self, *args, **kw):       # (the oracle engine has no cosine head: reaching it is what the test asks)
            calls.append("cos_proto_step")
            raise _Reached()

    eng = LogregOracleEngine()
    old = engine.set_engine(eng)
    try:
        cfg = dict(steps=15, lr=0.5, momentum=0.8, C=2.0, normalize=True)
        g = torch.Generator().manual_seed(13)
        y_s, y_q = (torch.arange(6) % 3).repeat(2, 1), (torch.arange(6) % 3).repeat(2, 1)
        x_s, x_q = torch.randn(2, 6, 3, 16, 16, generator=g), torch.randn(2, 6, 3, 16, 16, generator=g)
        batch = {"train": ((None, None, x_s), y_s), "test": ((None, None, x_q), y_q)}
        torch.manual_seed(9)
        models = [Pretrain("conv4", image_size=16, image_channels=3, n_classes=6, num_ways=3, metric="logreg", logreg=cfg),
                  MetaBaseline("conv4", image_size=16, image_channels=3, num_ways=3, eval_head="logreg", logreg=cfg)]
        for model in models:
            calls.clear()
            model.eval()
            v_loss, v_acc = model.evaluate(batch, None, None, "cpu", task="val")
            assert calls == [cfg]
            theta = [p.detach() for p in model.conv.theta()]
            f_s, f_q = eng.conv4_encode(x_s, x_q, theta)
            ref = logreg_head_ref(f_s.numpy(), y_s.numpy(), f_q.numpy(), y_q.numpy(), 3, **cfg)
            assert abs(float(v_loss) - ref["loss"]) <= 1e-6 and abs(float(v_acc) - ref["correct"] / 12) <= 1e-7
        calls.clear()
        with pytest.raises(_Reached):                                                # training keeps the model's own head
            models[1].evaluate(batch, None, None, "cpu", task="train")
        assert calls == ["cos_proto_step"]
    finally:
        engine.set_engine(old)
