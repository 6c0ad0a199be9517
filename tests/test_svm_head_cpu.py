"""CPU suite of the MetaOptNet-SVM head: the float64 restatement tests/svm_head_ref.py against independent
witnesses, the conditions tests/test_svm_head_gpu.py relies on, and the flags and refusals of --fewshot_head svm.

Witnesses: at T = 4000 the fit satisfies the KKT conditions of the dual to 1e-12; at T = 4000, Tb = 1000 the implicit gradient equals
central finite differences of the float64 loss to 1e-6 relative (entries sampled among those of at least a tenth of the tensor's largest
magnitude: the differences' own truncation error does not shrink with the entry); the projection meets its constraints and equals a
brute-force search over all free sets.

Conditions of the GPU test, over the whole case table: a plain float32 numpy run of the same iteration is within the GPU tolerances
(worst seen: logits 4.9e-7, alpha 1.8e-6, loss 1.5e-7, dfeats_s 5.6e-6, dfeats_q 6.7e-7, dscale 1.5e-7 of the largest magnitude; the
"offset" case 2.2e-5 on the logits, 2.1e-5 on alpha and 1.1e-3 on dfeats_s, see test_svm_head_gpu.py); its bound mask equals the
float64 mask at every entry whose float64 margin is at least M_FIT = 1e-5, and in fact at every entry: the smallest margin in the table
is 8.2e-8 and the float32 witness agrees there too, so no power of ten is too small for this witness.  M_FIT is 1e-5 by reasoning
instead: the witness's alpha is off by up to 2e-7 absolute, the extrapolation doubles that, the product and tau add as much again, so
a margin below 1e-6 can flip under another summation order (the kernels' orders are not numpy's), and ten times that is kept clear.
At most 0.85 % of an episode's entries are set aside (cap 1 %); no query row is (smallest top-two margin 2.4e-2)."""
import itertools

import numpy as np
import pytest

from oracle_engine import OracleEngine
from svm_head_cases import CASES, C_REG, EPS, IDS, M_FIT, MARGIN, MAX_SET_ASIDE, SCALE_TEST, SHAPES, case_inputs
from svm_head_ref import project_rows, svm_head_ref

TOL, TOL_OFFSET_GRAD = 1e-4, 1e-2      # tests/test_svm_head_gpu.py
WITNESS = [CASES[0], CASES[1], CASES[3]]   # 5-way 1-shot, 5-way 5-shot, 20-way 5-shot


def _rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("case", WITNESS, ids=[c[0] for c in WITNESS])
def test_fit_meets_the_kkt_conditions_and_the_gradient_equals_finite_differences(case):
    f_s, y_s, f_q, y_q = (a[:1] for a in case_inputs(case))
    N = case[1][0]
    kw = dict(scale=SCALE_TEST, C=C_REG, eps=EPS, steps=4000)
    ref = svm_head_ref(f_s, y_s, f_q, y_q, N, bwd_steps=1000, cg_floor=1e-28, **kw)
    print(f"{case[0]}: KKT residual {ref['stats'][0, 0]:.3e}, CG residual {ref['stats'][0, 1]:.3e}")
    assert ref["stats"][0, 0] < 1e-12
    loss = lambda xs, xq, sc: svm_head_ref(xs, y_s, xq, y_q, N, need_grad=False, **{**kw, "scale": sc})["loss"]
    rng = np.random.default_rng(5)
    h = 1e-5
    for name, x, g in (("dfeats_s", f_s.astype(np.float64), ref["gXs"]), ("dfeats_q", f_q.astype(np.float64), ref["gXq"])):
        big = np.argwhere(np.abs(g) >= 0.1 * np.abs(g).max())
        for idx in big[rng.choice(len(big), size=min(4, len(big)), replace=False)]:
            xp, xm = x.copy(), x.copy()
            xp[tuple(idx)] += h; xm[tuple(idx)] -= h
            args = (lambda v: (v, f_q, SCALE_TEST)) if name == "dfeats_s" else (lambda v: (f_s, v, SCALE_TEST))
            fd = (loss(*args(xp)) - loss(*args(xm))) / (2 * h)
            print(f"{case[0]} {name}{tuple(idx)}: {g[tuple(idx)]:.10e} against {fd:.10e}")
            assert abs(fd - g[tuple(idx)]) <= 1e-6 * abs(g[tuple(idx)])
    fd = (loss(f_s, f_q, SCALE_TEST + h) - loss(f_s, f_q, SCALE_TEST - h)) / (2 * h)
    assert abs(fd - ref["gscale"]) <= 1e-6 * abs(ref["gscale"])


def _brute_force(v, u):
    """The projection of v on {a <= u, sum a = 0}: the feasible stationary point of every free set, the nearest one kept."""
    best, n = None, len(v)
    for k in range(1, n + 1):
        for free in itertools.combinations(range(n), k):
            fr = np.zeros(n, dtype=bool); fr[list(free)] = True
            tau = (v[fr].sum() + u[~fr].sum()) / k
            a = np.where(fr, v - tau, u)
            if (a <= u + 1e-15).all():
                d = ((a - v) ** 2).sum()
                if best is None or d < best[0]:
                    best = (d, a)
    return best[1]


def test_projection_meets_its_constraints_and_equals_the_brute_force_search():
    rng = np.random.default_rng(11)
    for N in (2, 3, 5, 6):
        V = rng.standard_normal((40, N)) * rng.choice([0.01, 0.3, 3.0], size=(40, 1))
        U = np.zeros((40, N)); U[np.arange(40), rng.integers(0, N, 40)] = 0.1
        V[::7, 1] = V[::7, 0]                                                   # ties
        a, bound, margin = project_rows(V, U)
        assert (a <= U).all() and np.abs(a.sum(1)).max() < 1e-14
        assert np.array_equal(bound, margin >= 0)
        for r in range(40):
            assert np.abs(a[r] - _brute_force(V[r], U[r])).max() < 1e-12
    a, bound, _ = project_rows(rng.standard_normal((3, 4)), np.zeros((3, 4)), np.array([True, False, True]))
    assert (a[1] == 0).all() and bound[1].all()
    for dtype in (np.float32, np.float64):                                      # the constraints hold in the format's own arithmetic
        V = rng.standard_normal((200, 20)).astype(dtype)
        U = np.zeros((200, 20), dtype=dtype); U[np.arange(200), rng.integers(0, 20, 200)] = dtype(0.1)
        a, _, _ = project_rows(V, U)
        assert a.dtype == dtype and (a <= U).all() and np.abs(a.sum(1)).max() <= 64 * np.finfo(dtype).eps


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_witness_is_within_the_gpu_tolerances_and_the_margins_hold(case):
    name, (N, shots, Qn, Fd), B, T, Tb, variant, _ = case
    inp = case_inputs(case)
    kw = dict(scale=SCALE_TEST, C=C_REG, eps=EPS, steps=T, bwd_steps=Tb)
    ref = svm_head_ref(*inp, N, **kw)
    wit = svm_head_ref(*inp, N, dtype=np.float32, **kw)
    # the margins of the float64 reference alone
    aside = ref["fit_margin"] < M_FIT
    frac = aside.reshape(B, -1).mean(axis=1).max()
    print(f"{name}: {frac:.4f} of an episode set aside, smallest fit margin {ref['fit_margin'].min():.3e}, "
          f"smallest query margin {ref['margin'].min():.3e}")
    assert frac <= MAX_SET_ASIDE
    assert (ref["margin"] > MARGIN).all()
    # the float32 witness: the mask outside the set-aside entries, then everything the GPU test bounds
    assert np.array_equal(wit["bound"][~aside], ref["bound"][~aside])
    assert np.array_equal(wit["preds"], ref["preds"]) and wit["correct"] == ref["correct"] and wit["status"] == ref["status"]
    tf = svm_head_ref(*inp, N, mask=wit["bound"], **kw)
    errs = dict(logits=_rel(wit["logits"], ref["logits"]), alpha=_rel(wit["alpha"], ref["alpha"]),
                loss=abs(wit["loss"] - ref["loss"]) / abs(ref["loss"]), dfeats_s=_rel(wit["gXs"], tf["gXs"]),
                dfeats_q=_rel(wit["gXq"], tf["gXq"]), dscale=abs(wit["gscale"] - tf["gscale"]) / abs(tf["gscale"]))
    print(f"{name}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= (TOL_OFFSET_GRAD if variant == "offset" and k.startswith("d") else TOL), k
    assert np.allclose(wit["stats"], tf["stats"], rtol=1e-3, atol=1e-6)
    U = np.zeros_like(wit["alpha"])
    ok_s = (inp[1] >= 0) & (inp[1] < N)
    bi, si = np.nonzero(ok_s)
    U[bi, si, inp[1][bi, si]] = np.float32(C_REG)
    assert (wit["alpha"] <= U).all() and np.abs(wit["alpha"].sum(-1)).max() <= 1e-6


def test_case_table_covers_what_the_issue_names():
    assert {c[1] for c in CASES} == set(SHAPES) and {c[2] for c in CASES} == {1, 3}
    assert {c[3] for c in CASES} == {1, 2, 37, 120} and {c[4] for c in CASES} == {1, 40}
    assert {c[5] for c in CASES} == {None, "unbalanced", "status", "offset"}
    st = next(c for c in CASES if c[5] == "status")
    ref = svm_head_ref(*case_inputs(st), st[1][0], steps=5, need_grad=False)
    assert ref["status"] == 3 and (ref["alpha"][1, 0] == 0).all() and ref["bound"][1, 0].all()


# ---- flags, the model's parameter, refusals -------------------------------------------------------------------------------------------
def test_svm_flags_parse_with_their_defaults_and_reach_the_model():
    import torch
    from fumi_amd.utils import utils
    def parse(argv):
        a = utils.cli_parser().parse_args(argv)
        a.device = "cpu"
        return a
    d = utils.cli_parser().parse_args([])
    assert (d.svm_C, d.svm_eps, d.svm_scale, d.svm_steps, d.svm_bwd_steps) == (0.1, 1.0, 1.0, 120, 40)
    assert [f for f, _ in utils._SVM_FLAGS] == ["--svm_C", "--svm_eps", "--svm_scale", "--svm_steps", "--svm_bwd_steps"]
    flags = lambda p: [act.option_strings[0] for act in p._actions if act.option_strings and act.dest != "help"]
    assert flags(utils.cli_parser()) == flags(utils.parser()) + [f for f, _ in utils._SVM_FLAGS]   # appended after every earlier flag
    assert "svm" not in next(a for a in utils.parser()._actions if a.dest == "fewshot_head").choices   # parser() is what it was
    assert utils.svm_config(utils.parser().parse_args([])) == utils.svm_config(None)              # a namespace without the flags
    from fumi_amd.models.metabaseline import MetaBaseline
    with pytest.raises(ValueError, match="svm="):                                                 # no silent hyper-parameters
        MetaBaseline("conv4", image_size=16, head="svm")
    assert MetaBaseline("conv4", image_size=16, head="svm", svm=utils.svm_config(None)).svm.tolist() == [1.0]
    with pytest.raises(SystemExit):
        utils.cli_parser().parse_args(["--fewshot_head", "knn"])
    a = parse(["--model", "metabaseline", "--fewshot_head", "svm", "--svm_scale", "2.5", "--svm_C", "0.2", "--svm_steps", "60",
               "--im_encoder", "conv4", "--image_size", "16", "--num_ways", "3"])
    model = utils.init_model(a, None, watch=False)
    assert model.head == "svm" and isinstance(model.svm, torch.nn.Parameter) and model.svm.tolist() == [2.5]
    assert model.head_param() is model.svm and "svm" in model.state_dict() and "temp" not in model.state_dict()
    assert model.svm_cfg == dict(C=0.2, eps=1.0, scale=2.5, steps=60, bwd_steps=40)
    fresh = utils.init_model(parse(["--model", "metabaseline", "--fewshot_head", "svm", "--im_encoder", "conv4", "--image_size", "16",
                                    "--num_ways", "3"]), None, watch=False)
    fresh.load_state_dict(model.state_dict())
    assert fresh.svm.tolist() == [2.5]
    p = parse(["--model", "pretrain", "--pretrain_metric", "svm", "--svm_C", "0.3", "--im_encoder", "conv4", "--image_size", "16"])
    p.n_classes = 8                                                               # (set by the dataset in a run)
    pre = utils.init_model(p, None, watch=False)
    assert pre.metric == "svm" and pre.svm_cfg["C"] == 0.3
    from fumi_amd import engine, hip
    assert callable(engine.HipEngine.svm_head_step) and callable(hip.svm_set_form) and callable(hip.svm_get_fit)
    # the default head builds what it built before
    plain = utils.init_model(parse(["--model", "metabaseline", "--im_encoder", "conv4", "--image_size", "16"]), None, watch=False)
    assert plain.head == "cosine" and "temp" in plain.state_dict() and "svm" not in plain.state_dict()


def test_check_supported_refuses_what_the_svm_head_cannot_run():
    from fumi_amd import engine
    from fumi_amd import main as cli
    old = engine.set_engine(OracleEngine())
    try:
        base = ["--disable_cuda", "--dataset", "synthetic-resident", "--im_encoder", "conv4"]
        meta = ["--model", "metabaseline", "--fewshot_head", "svm"] + base
        cli.check_supported(cli.parse_args(meta))
        cli.check_supported(cli.parse_args(meta + ["--svm_C", "1", "--svm_eps", "0.5", "--svm_scale", "7", "--svm_steps", "30",
                                                   "--svm_bwd_steps", "10"]))
        cli.check_supported(cli.parse_args(meta + ["--eval_head", "logreg"]))         # as the other heads: the logreg head evaluates
        cli.check_supported(cli.parse_args(["--model", "pretrain", "--pretrain_metric", "svm", "--svm_steps", "60"] + base))
        for flag, val in (("--svm_C", "0.2"), ("--svm_eps", "2"), ("--svm_scale", "3"), ("--svm_steps", "10"), ("--svm_bwd_steps", "5")):
            for other in (["--model", "metabaseline"], ["--model", "metabaseline", "--fewshot_head", "ridge"], ["--model", "pretrain"]):
                with pytest.raises(ValueError, match=flag):
                    cli.check_supported(cli.parse_args(other + base + [flag, val]))   # the flags without their head
        with pytest.raises(ValueError, match="--svm_bwd_steps"):
            cli.check_supported(cli.parse_args(["--model", "pretrain", "--pretrain_metric", "svm", "--svm_bwd_steps", "5"] + base))
        with pytest.raises(ValueError, match="--fewshot_head"):
            cli.check_supported(cli.parse_args(["--model", "pretrain", "--fewshot_head", "svm"] + base))
        with pytest.raises(ValueError, match="--pretrain_metric"):
            cli.check_supported(cli.parse_args(["--model", "metabaseline", "--pretrain_metric", "svm"] + base))
        with pytest.raises(ValueError, match="--transductive_steps"):
            cli.check_supported(cli.parse_args(meta + ["--transductive_steps", "3"]))
        with pytest.raises(ValueError, match="--transductive_steps"):
            cli.check_supported(cli.parse_args(["--model", "pretrain", "--pretrain_metric", "svm", "--transductive_steps", "3"] + base))
        with pytest.raises(ValueError, match="--logreg_lr"):                          # --eval_head logreg keeps its own refusals
            cli.check_supported(cli.parse_args(meta + ["--eval_head", "logreg", "--logreg_lr", "9"]))
        for flag in ("--svm_C", "--svm_eps", "--svm_scale"):
            for bad in ("0", "-1"):
                with pytest.raises(ValueError, match=flag):
                    cli.check_supported(cli.parse_args(meta + [flag, bad]))
        for flag, bad in (("--svm_steps", "0"), ("--svm_steps", "10001"), ("--svm_bwd_steps", "0"), ("--svm_bwd_steps", "1001")):
            with pytest.raises(ValueError, match=flag):
                cli.check_supported(cli.parse_args(meta + [flag, bad]))
        with pytest.raises(NotImplementedError, match="128"):
            cli.check_supported(cli.parse_args(meta + ["--num_ways", "30", "--num_shots", "5"]))
        for ways in ("1", "65"):
            with pytest.raises(NotImplementedError, match="--num_ways"):
                cli.check_supported(cli.parse_args(meta + ["--num_ways", ways, "--num_shots", "1"]))
        cli.check_supported(cli.parse_args(["--model", "metabaseline"] + base))       # the cosine head is asked nothing new
    finally:
        engine.set_engine(old)
