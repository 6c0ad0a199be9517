"""CPU suite that pins the oracle of tests/test_optim_edges_gpu.py (tests/optim_ref.py) without a GPU: rule64 is torch.optim's
rule, the table E32 behind the device bound is what rule32 measures against rule64, and a comparison at that bound notices a
dropped tail element, a wrong tensor at a boundary and a missing weight decay.

What "applies" means for the three corruptions (`test_the_comparison_has_teeth`):
  tail     every tensor of every case, except where the tensor's last element is the one whose gradient the cold variant sets to 0
           (a one-element tensor): with zero moments and a zero gradient the true update is the identity, or lr wd p.
  wrong    every case of two tensors or more.
  no decay weight_decay != 0 and a rule whose decayed gradient enters a state stream (adam, both sgd_momentum forms): there the loss
           is first order in wd.  For sgd and adamw the decay reaches the parameter alone, scaled by lr: the loss is lr wd = 1.5e-6 of
           the tensor's old maximum WHATEVER the values, and 100 x the smallest possible bound is 100 * 4 * 2^-24 = 2.4e-5.  No choice
           of values can give those two rules the 100 x margin; `test_decay_that_reaches_the_parameter_alone_costs_lr_times_wd`
           holds what arithmetic allows: the loss is exactly lr wd of the largest parameter, which is outside the bound wherever the
           step does not grow that maximum much (lr wd is 2.9 x the bound for adamw, 6.3 x for sgd), and nothing else moves.  The device
           comparison alone does not promise to notice a lost decay in those two rules; the torch-class comparisons over five
           steps (tests/test_optim_fused_gpu.py) do."""
import numpy as np
import pytest
import torch

import optim_ref as R

EPS64 = float(np.finfo(np.float64).eps)
# individually rounded float64 operations of one step of the rule, coefficient folding included (bias corrections, lr / bc1,
# 1 / sqrt(bc2), 1 - lr wd, 1 - beta)
OPS = {"adam": 17, "adamw": 16, "sgd_momentum": 6, "sgd": 4}
STEPS = 3
TORCH_CASES = ["quad_tails", "boundaries_in_one_workgroup", "all_misaligned"]


def _torch_chain(rule, hyper, p, grads):
    """STEPS steps of the torch class on float64 CPU tensors, fed the ABI-rounded scalars -> (p, s0, s1) lists."""
    h = R.abi(rule, hyper)
    params = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in p]
    if rule == "adam":
        opt = torch.optim.Adam(params, lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"], foreach=False)
    elif rule == "adamw":
        opt = torch.optim.AdamW(params, lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"], foreach=False)
    else:
        opt = torch.optim.SGD(params, lr=h["lr"], momentum=h["momentum"] if rule == "sgd_momentum" else 0.0, weight_decay=h["wd"],
                              foreach=False)
    for gs in grads:
        for x, g in zip(params, gs):
            x.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
    keys = {"adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq"), "sgd_momentum": ("momentum_buffer",), "sgd": ()}[rule]
    state = [[opt.state[x][k].numpy() for x in params] for k in keys] + [None, None]
    return [x.detach().numpy() for x in params], state[0], state[1]


@pytest.mark.parametrize("hyper", range(len(R.HYPERS)))
@pytest.mark.parametrize("rule", sorted(OPS))
def test_rule64_is_torchs_rule(rule, hyper):
    """Three chained steps (step = 1, 2, 3, a new gradient each; sgd_momentum's first step is sgd_momentum_first) against the torch
    class in float64 with the same ABI-rounded scalars.  Measured: at most 0.91 eps (adam), 1.16 eps (adamw), 0.60 eps (sgd_momentum), 0.41 eps (sgd) --
    the two differ in association only (torch divides by sqrt(bc2), the kernel multiplies by its inverse)."""
    worst = 0.0
    for name in TORCH_CASES:
        x = R.case_inputs(name, "adam")
        n = len(x["p"])
        rng = np.random.default_rng([7, sorted(R.CASES).index(name)])
        grads = [[g * rng.uniform(0.5, 2.0) + 0.1 * rng.standard_normal(g.shape) for g in x["g"]] for _ in range(STEPS)]
        p = [np.asarray(a, dtype=np.float64) for a in x["p"]]
        s0, s1 = [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p]
        for it in range(STEPS):
            r = "sgd_momentum_first" if rule == "sgd_momentum" and it == 0 else rule
            out = [R.rule64(r, p[i], grads[it][i], s0[i], s1[i], dict(R.HYPERS[hyper], step=it + 1)) for i in range(n)]
            p = [o[0] for o in out]
            s0 = [o[1] for o in out] if R.NSTATE[rule] >= 1 else s0
            s1 = [o[2] for o in out] if R.NSTATE[rule] >= 2 else s1
        tp, ts0, ts1 = _torch_chain(rule, R.HYPERS[hyper], x["p"], grads)
        for mine, theirs in ((p, tp), (s0, ts0), (s1, ts1)):
            if theirs is not None:
                worst = max(worst, max(R.rel_to_max(a, b) for a, b in zip(mine, theirs)))
    print(f"{rule} hyper {hyper}: rule64 against torch float64 over {STEPS} steps: {worst / EPS64:.2f} eps")
    assert worst <= 0.5 * EPS64 * OPS[rule]            # half an ulp per operation, none of them amplified


def test_adam_beta_rounding_is_the_documented_deviation():
    """The Adam ABI's float betas against torch.optim.Adam fed the doubles 0.9 and 0.999 (float64, one step from zero moments):
    exp_avg_sq = (1 - b2) gr^2 is smaller by ADAM_BETA2_DEVIATION = 1.2875e-5 of itself, element by element; exp_avg by 2.1e-7 of
    itself (the rounding of 0.9f against 0.1)."""
    x = R.case_inputs("boundaries_in_one_workgroup", "adam", "cold")
    hyper = dict(R.HYPERS[0], step=1)
    for i in range(len(x["p"])):
        _, m, v = R.rule64("adam", x["p"][i], x["g"][i], x["s0"][i], x["s1"][i], hyper)
        gr = np.asarray(x["g"][i], np.float64) + float(np.float32(hyper["wd"])) * np.asarray(x["p"][i], np.float64)
        dv = R.rel_to_max(v, (1.0 - 0.999) * gr * gr)
        dm = R.rel_to_max(m, (1.0 - 0.9) * gr)
        print(f"tensor {i}: exp_avg_sq off by {dv:.6e}, exp_avg by {dm:.3e}")
        assert dv == pytest.approx(R.ADAM_BETA2_DEVIATION, rel=1e-6) and R.ADAM_BETA2_DEVIATION == pytest.approx(1.2875e-5, rel=1e-4)
        assert dm == pytest.approx(2.384e-7, rel=1e-3)
    # and the AdamW ABI (double betas) shows none of it
    _, m, v = R.rule64("adamw", x["p"][0], x["g"][0], x["s0"][0], x["s1"][0], hyper)
    g = np.asarray(x["g"][0], np.float64)
    assert R.rel_to_max(v, (1.0 - 0.999) * g * g) <= 2 * EPS64


@pytest.mark.parametrize("rule", R.RULES)
def test_e32_is_the_table_this_measures(rule):
    got = R.measure_e32(rule)
    print(f"{rule}: measured {got}, recorded {R.E32[rule]}")
    assert got.keys() == R.E32[rule].keys()
    for k, v in got.items():
        assert R.E32[rule][k] / 2 <= v <= R.E32[rule][k], (k, v, R.E32[rule][k])


def test_the_case_table_is_the_one_the_kernel_needs():
    assert R.CASES["grid_stride_wraps"][0][0] == (2048 * 1024 + 5,) and [s for s, _ in R.CASES["grid_stride_wraps"][1:]] == [(6,), (1025,)]
    assert R.CASES["wrap_then_misaligned"] == [((2048 * 1024 + 1,), {}), ((130,), {"p": 1})]
    assert len(R.CASES["thirty_two"]) == R.MAXT == 32
    for s in R.STREAMS:
        offs = [o for _, o in R.CASES[f"one_stream_misaligned_{s}"]]
        assert offs == [{s: 1}, {}, {s: 1}]
    assert all(o == dict.fromkeys(R.STREAMS, 1) for _, o in R.CASES["all_misaligned"])
    for name in R.CASES:
        for rule in ("adam", "sgd_momentum"):
            warm, cold = R.case_inputs(name, rule, "warm"), R.case_inputs(name, rule, "cold")
            for i, (shape, _) in enumerate(R.CASES[name]):
                assert warm["g"][i].shape == shape and warm["g"][i].dtype == np.float32
                assert int((cold["g"][i] == 0).sum()) == 1 and not (warm["g"][i] == 0).any()
                assert not cold["s0"][i].any() and warm["s0"][i].all()
                if rule == "adam":
                    assert not cold["s1"][i].any() and (warm["s1"][i] > 0).all()


def _margin(rule, ref, bad):
    """max over tensors and streams of (rel_to_max of the corrupted output against the true one) / the stream's device bound"""
    worst = 0.0
    for r, b in zip(ref, bad):
        for k, x, y in zip(R.OUT_STREAMS, r, b):
            if x is not None:
                worst = max(worst, R.rel_to_max(y, x) / R.bound(rule, k))
    return worst


def _tail(rule, x, ref, k):
    """tensor k's last element keeps the values it came with"""
    bad = [tuple(None if a is None else a.copy() for a in r) for r in ref]
    for stream, a in zip(R.OUT_STREAMS, bad[k]):
        if a is not None:
            a.flat[-1] = x[stream][k].flat[-1]
    return bad


def _wrong_tensor(rule, x, ref, hyper):
    """the last tensor's first quad is the rule applied to the previous tensor's first quad"""
    bad = [tuple(None if a is None else a.copy() for a in r) for r in ref]
    q = min(4, x["p"][-1].size, x["p"][-2].size)
    arg = lambda s: None if x[s] is None else x[s][-2].reshape(-1)[:q]
    for a, w in zip(bad[-1], R.rule64(rule, arg("p"), arg("g"), arg("s0"), arg("s1"), hyper)):
        if a is not None:
            a.reshape(-1)[:q] = w
    return bad


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("name", sorted(R.CASES))
@pytest.mark.parametrize("rule", R.RULES)
def test_the_comparison_has_teeth(rule, name, variant):
    x = R.case_inputs(name, rule, variant)
    n = len(x["p"])
    for hi, hyper in enumerate(R.HYPERS):
        ref = R.reference(name, rule, hyper, variant)
        for k in sorted({0, n - 1}):
            if x["g"][k].flat[-1] != 0:
                m = _margin(rule, ref, _tail(rule, x, ref, k))
                print(f"hyper {hi}: tail of tensor {k} left alone: {m:.3g} x the bound")
                assert m >= 100
        if n >= 2:
            m = _margin(rule, ref, _wrong_tensor(rule, x, ref, R.cold_hyper(hyper, variant)))
            print(f"hyper {hi}: wrong tensor at the last boundary: {m:.3g} x the bound")
            assert m >= 100
        if hyper["wd"] != 0 and rule in ("adam", "sgd_momentum_first", "sgd_momentum"):
            m = _margin(rule, ref, R.reference(name, rule, dict(hyper, wd=0.0), variant))
            print(f"hyper {hi}: no weight decay: {m:.3g} x the bound")
            assert m >= 100


@pytest.mark.parametrize("rule", ["adamw", "sgd"])
def test_decay_that_reaches_the_parameter_alone_costs_lr_times_wd(rule):
    """See the module docstring: in every case, losing the decay moves a tensor by exactly lr wd of the largest parameter it had, no
    state stream at all, and lr wd is below 100 x the smallest bound any stream can have."""
    hyper = R.HYPERS[0]
    h = R.abi(rule, hyper)
    worst = 0.0
    for name in sorted(R.CASES):
        for variant in R.VARIANTS:
            ref = R.reference(name, rule, hyper, variant)
            bad = R.reference(name, rule, dict(hyper, wd=0.0), variant)
            for r, b, p in zip(ref, bad, R.case_inputs(name, rule, variant)["p"]):
                assert np.abs(b[0] - r[0]).max() == pytest.approx(h["lr"] * h["wd"] * float(np.abs(p).max()), rel=1e-6)
                assert all(x is None or np.array_equal(x, y) for x, y in zip(r[1:], b[1:]))
                worst = max(worst, R.rel_to_max(b[0], r[0]) / R.bound(rule, "p"))
    print(f"{rule}: lr wd = {h['lr'] * h['wd']:.3e}; the lost decay is at most {worst:.2f} x the bound {R.bound(rule, 'p'):.3e}")
    assert h["lr"] * h["wd"] < 100 * 4 * 2.0 ** -24
    assert worst > 1
