"""GPU suite of the clipped optimizer step (csrc/adam.hip: grad_sumsq_kernel, clip_finish_kernel, optim_clipped_kernel;
fumi_amd/optim.py: max_grad_norm; --max_grad_norm).

The norm and the coefficient are held to the float64 restatement of tests/clip_ref.py within its derived bounds (norm 2^-22, coef
2^-21 relative).  Everything behind the coefficient is held BIT FOR BIT to the existing unclipped entry point run on gradients that
were multiplied on the device by the coefficient the clipped call wrote: an fp32 multiply is the same everywhere."""
import functools
import glob
import json
import math
import os

import numpy as np
import pytest
import torch

import clip_ref as R
from helpers import rel_to_max
from test_optim_fused_gpu import SHAPES, STATE_TOL, STEPS, _forbid_torch_step

pytestmark = pytest.mark.gpu

RULES = ["adam", "adamw", "sgd_momentum_first", "sgd_momentum", "sgd"]
HYPER = dict(lr=3e-3, b1=0.9, b2=0.999, eps=1e-8, wd=5e-4, step=3, momentum=0.9)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _place(arr, offset, dev):
    """The array on the device; offset 1: as a view starting one element into a larger buffer."""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    if not offset:
        return t.to(dev)
    buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device=dev)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def _case(name):
    """(gradients on the device, their float64 norm): computed once per case and left unchanged."""
    dev = torch.device("cuda:0")
    arrays = R.case_arrays(name)
    grads = [_place(a, off, dev) for a, (_, off) in zip(arrays, R.CASES[name])]
    return grads, R.norm64(arrays)


def _state(name, rule, dev):
    """Fresh parameters and state tensors for `rule` (same values on every call), laid out like the case's gradients."""
    arrays = R.case_arrays(name, seed=1)
    offs = [off for _, off in R.CASES[name]]
    p = [_place(a, off, dev) for a, off in zip(arrays, offs)]
    s0 = s1 = None
    if rule in ("adam", "adamw"):
        s0 = [_place(a * np.float32(0.1), off, dev) for a, off in zip(R.case_arrays(name, seed=2), offs)]
        s1 = [_place(a * a, off, dev) for a, off in zip(R.case_arrays(name, seed=3), offs)]
    elif rule == "sgd_momentum":
        s0 = [_place(a, off, dev) for a, off in zip(R.case_arrays(name, seed=2), offs)]
    elif rule == "sgd_momentum_first":
        s0 = [_place(np.full_like(a, np.float32(7.0)), off, dev) for a, off in zip(arrays, offs)]      # written, never read
    return p, s0, s1


def _step(rule, p, g, s0, s1, dev, clip=None):
    """One call of the rule's entry point: clipped (clip = (max_norm, clip_out)) or the existing unclipped one, which takes at most
    32 tensors and none without elements (torch gives those a NULL pointer) -- it is called per chunk of 32 on the others."""
    from fumi_amd import hip
    ws = hip.Workspace.get(dev)
    h = HYPER

    def call(idx):
        sel = lambda xs: None if xs is None else [xs[i] for i in idx]
        if rule in ("adam", "adamw"):
            args = hip.AdamArgs(sel(p), sel(g), sel(s0), sel(s1))
            if clip is None:
                (hip.adam_step if rule == "adam" else hip.adamw_step)(ws, args, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"], dev)
            else:
                (hip.adam_step_clipped if rule == "adam" else hip.adamw_step_clipped)(
                    ws, args, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"], clip[0], clip[1], dev)
        else:
            args = hip.SgdArgs(sel(p), sel(g), sel(s0))
            mom = h["momentum"] if s0 is not None else 0.0
            first = rule == "sgd_momentum_first"
            if clip is None:
                hip.sgd_step(ws, args, h["lr"], mom, h["wd"], first, dev)
            else:
                hip.sgd_step_clipped(ws, args, h["lr"], mom, h["wd"], first, clip[0], clip[1], dev)

    if clip is not None:
        call(range(len(p)))
    else:
        idx = [i for i in range(len(p)) if p[i].numel() > 0]
        for k0 in range(0, len(idx), 32):
            call(idx[k0:k0 + 32])


def _all(p, s0, s1):
    return list(p) + list(s0 or []) + list(s1 or [])


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_norm_and_coef_match_the_float64_restatement(name, dev):
    from fumi_amd import hip
    grads, ref = _case(name)
    ws = hip.Workspace.get(dev)
    max_norm = ref / 2
    alone = hip.grad_norm(ws, grads)
    p, s0, s1 = _state(name, "sgd", dev)
    clip_out = torch.full((2,), -1.0, device=dev)
    _step("sgd", p, grads, s0, s1, dev, clip=(max_norm, clip_out))
    norm, coef = clip_out.tolist()
    want = R.coef32(ref, max_norm)
    print(f"{name}: norm {norm!r} (float64 {ref!r}, rel {abs(norm - ref) / ref:.3e}), coef {coef!r} (want {want!r}, rel {abs(coef - want) / want:.3e})")
    assert abs(norm - ref) <= R.NORM_RTOL * ref
    assert abs(float(alone) - ref) <= R.NORM_RTOL * ref
    assert abs(coef - want) <= R.COEF_RTOL * want
    assert torch.equal(alone, clip_out[:1])                                   # the two entry points: the same bits


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_clipped_step_is_bit_identical_to_the_existing_kernel_on_scaled_gradients(name, rule, dev):
    grads, ref = _case(name)
    keep = [g.clone() for g in grads]
    max_norm = ref / 2
    p, s0, s1 = _state(name, rule, dev)
    clip_out = torch.full((2,), -1.0, device=dev)
    _step(rule, p, grads, s0, s1, dev, clip=(max_norm, clip_out))
    assert 0.0 < float(clip_out[1]) < 1.0
    for g, k in zip(grads, keep):
        assert torch.equal(g, k)                                              # the gradients are read only
    # the existing entry point on clones whose gradients were multiplied on the device by the coef the call wrote
    q, t0, t1 = _state(name, rule, dev)
    scaled = [g * clip_out[1] for g in grads]
    _step(rule, q, scaled, t0, t1, dev)
    for x, y in zip(_all(p, s0, s1), _all(q, t0, t1)):
        assert torch.equal(x, y)
    # and once more on equal inputs: equal bits
    r, u0, u1 = _state(name, rule, dev)
    again = torch.full((2,), -1.0, device=dev)
    _step(rule, r, grads, u0, u1, dev, clip=(max_norm, again))
    assert torch.equal(again, clip_out)
    for x, y in zip(_all(p, s0, s1), _all(r, u0, u1)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_a_norm_below_max_norm_clips_nothing(name, rule, dev):
    grads, ref = _case(name)
    p, s0, s1 = _state(name, rule, dev)
    clip_out = torch.full((2,), -1.0, device=dev)
    _step(rule, p, grads, s0, s1, dev, clip=(ref * 2, clip_out))
    assert float(clip_out[1]) == 1.0
    q, t0, t1 = _state(name, rule, dev)
    _step(rule, q, grads, t0, t1, dev)
    for x, y in zip(_all(p, s0, s1), _all(q, t0, t1)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("bad,check", [(float("inf"), lambda n, c: n == math.inf and c == 0.0),
                                       (float("nan"), lambda n, c: math.isnan(n) and math.isnan(c))])
def test_non_finite_gradients_are_ordinary_inputs(bad, check, dev):
    grads = [g.clone() for g in _case("boundaries_in_one_workgroup")[0]]
    grads[1][700] = bad
    p, s0, s1 = _state("boundaries_in_one_workgroup", "adam", dev)
    clip_out = torch.full((2,), -1.0, device=dev)
    _step("adam", p, grads, s0, s1, dev, clip=(1.0, clip_out))
    norm, coef = clip_out.tolist()
    assert check(norm, coef), (norm, coef)


def test_argument_checks(dev):
    from fumi_amd import hip
    ws = hip.Workspace.get(dev)
    p = [torch.zeros(5, device=dev)]
    g = [torch.ones(5, device=dev)]
    clip_out = torch.zeros(2, device=dev)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(hip.FumiHipError, match=r"\(-1\)"):               # FUMI_EINVAL
            hip.sgd_step_clipped(ws, hip.SgdArgs(p, g, None), 0.1, 0.0, 0.0, False, bad, clip_out, dev)
    many_p = list(torch.zeros(257, 5, device=dev).unbind(0))
    many_g = list(torch.ones(257, 5, device=dev).unbind(0))
    with pytest.raises(hip.FumiHipError, match=r"\(-4\)"):                   # FUMI_ENOTSUP
        hip.sgd_step_clipped(ws, hip.SgdArgs(many_p, many_g, None), 0.1, 0.0, 0.0, False, 1.0, clip_out, dev)
    with pytest.raises(hip.FumiHipError, match=r"\(-4\)"):
        hip.grad_norm(ws, many_g)
    hip.sgd_step_clipped(ws, hip.SgdArgs(many_p[:256], many_g[:256], None), 0.1, 0.0, 0.0, False, 1.0, clip_out, dev)
    torch.cuda.synchronize()
    assert all(bool((x == 0).all()) for x in p) and float(clip_out[0]) == pytest.approx(math.sqrt(256 * 5), rel=1e-6)


# ---- the optimizer classes ------------------------------------------------------------------------------------------------------
CLASSES = [("Adam", dict(lr=3e-3, weight_decay=5e-4)), ("AdamW", dict(lr=3e-3, weight_decay=1e-2)),
           ("SGD", dict(lr=3e-3, momentum=0.9, weight_decay=5e-4)), ("SGD", dict(lr=3e-3, momentum=0.0, weight_decay=5e-4))]


def _classes(name):
    from fumi_amd import optim
    return getattr(optim, name), getattr(torch.optim, name)


@pytest.mark.parametrize("shapes", [SHAPES, [(5, 3)] * 50 + [(300,), (2,)]], ids=["production", "52_tensors"])
@pytest.mark.parametrize("name,kw", CLASSES)
def test_clipping_class_matches_torchs_clip_and_step(name, kw, shapes, dev, monkeypatch):
    """Five steps, every one clipped; bounds of tests/test_optim_fused_gpu.py (2e-7 rel-to-max on parameters, STATE_TOL on state:
    the norm path adds at most 2^-21 relative to each gradient, below both at five steps).  torch's own step never runs for ours."""
    cls, tcls = _classes(name)
    max_norm = 0.05
    g = torch.Generator().manual_seed(0)
    pa = [torch.randn(*s, generator=g).to(dev).requires_grad_(True) for s in shapes]
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    oa, ob = cls(pa, max_grad_norm=max_norm, **kw), tcls(pb, **kw)
    torch_step = _forbid_torch_step(monkeypatch, tcls)
    coefs = []
    for it in range(STEPS):
        for x, y in zip(pa, pb):
            gr = torch.randn(x.shape, generator=g).to(dev)
            x.grad, y.grad = gr.clone(), gr.clone()
        keep = [x.grad.clone() for x in pa]
        total = torch.nn.utils.clip_grad_norm_(pb, max_norm)
        if it % 2:
            oa.step_fused()
        else:
            oa.step()
        torch_step(ob)
        norm, coef = oa.clip_stats.tolist()
        coefs.append(coef)
        assert norm == pytest.approx(float(total), rel=1e-6)
        assert all(torch.equal(x.grad, k) for x, k in zip(pa, keep))          # p.grad is left unscaled
    assert all(0.0 < c < 1.0 for c in coefs), coefs
    errs = [rel_to_max(x.detach().cpu(), y.detach().cpu()) for x, y in zip(pa, pb)]
    print(f"{name} {kw}: max rel-to-max over parameters {max(errs):.3e}")
    assert max(errs) <= 2e-7, errs
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert set(sa["state"][k]) == set(sb["state"][k])
        for key in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
            if key in sa["state"][k]:
                err = rel_to_max(sa["state"][k][key].cpu(), sb["state"][k][key].cpu())
                assert err <= STATE_TOL, (key, err)


def test_a_clipping_optimizer_never_defers(dev):
    from fumi_amd import hip, optim
    p = [torch.randn(64, 8, device=dev).requires_grad_(True)]
    o = optim.Adam(p, lr=1e-3, max_grad_norm=0.5)
    for _ in range(2):                                                        # (an unclipped optimizer would defer from its second step on)
        p[0].grad = torch.ones_like(p[0])
        o.step_fused()
    assert o.defer_step(dev) is False
    assert hip.adam_flush(hip.Workspace.get(dev), dev) is False                # nothing was left pending
    plain = optim.Adam([p[0]], lr=1e-3)
    for _ in range(2):
        plain.step_fused()
    assert plain.defer_step(dev) is True and plain.finish_deferred(dev) is True


# ---- the command line -------------------------------------------------------------------------------------------------------------
CLI = {"fumi": (["--num_train_adapt_steps", "1", "--num_test_adapt_steps", "1", "--step_size", "0.05"], 2),
       "maml": (["--num_train_adapt_steps", "1", "--num_test_adapt_steps", "1"], 0),
       "am3": ([], 0)}


def _cli(model, max_grad_norm, log_dir, epochs=None, eval_freq=1000):
    """One CLI run; --epochs E processes E + 1 meta-batches (default: the model's count in CLI) and validates every eval_freq-th
    (default: never).  Returns the parameters before and after and the optimizer."""
    from fumi_amd import main as cli
    from fumi_amd.utils import utils as U
    made = {}
    init_model, init_optim = U.init_model, U.init_optim

    def capture_model(args, dictionary, *a, **k):
        m = init_model(args, dictionary, *a, **k)
        made["model"], made["before"] = m, [p.detach().clone() for p in m.parameters()]
        return m

    def capture_optim(args, m):
        made["optim"] = init_optim(args, m)
        return made["optim"]
    extra = CLI[model][0]
    epochs = CLI[model][1] if epochs is None else epochs
    argv = ["--model", model, "--dataset", "synthetic-resident", "--text_encoder", "BERT", "--image_embedding_model", "resnet-34",
            "--im_emb_dim", "512", "--text_emb_dim", "32", "--batch_size", "4", "--num_shots", "2", "--num_ways", "5",
            "--num_shots_test", "3", "--epochs", str(epochs), "--eval_freq", str(eval_freq), "--num_ep_test", "4", "--lr", "1e-3",
            "--dropout", "0", "--log_dir", log_dir, "--synthetic_classes", "16", "--wandb_offline"] + extra
    if max_grad_norm is not None:
        argv += ["--max_grad_norm", max_grad_norm]
    U.init_model, U.init_optim = capture_model, capture_optim
    try:
        args = cli.parse_args(argv)
        assert args.device.type == "cuda"
        cli.main(args)
    finally:
        U.init_model, U.init_optim = init_model, init_optim
    torch.cuda.synchronize()
    opt = made["optim"][0] if type(made["optim"]) is tuple else made["optim"]
    return made["before"], [p.detach().clone() for p in made["model"].parameters()], opt


@pytest.mark.parametrize("model", sorted(CLI))
def test_cli_with_the_flag(model, tmp_path_factory, monkeypatch):
    root = tmp_path_factory.mktemp(f"clip_{model}")
    monkeypatch.chdir(root)
    _, off, opt_off = _cli(model, None, str(root / "off"))
    _, huge, opt_huge = _cli(model, "1e30", str(root / "huge"))
    before, tight, opt_tight = _cli(model, "1e-3", str(root / "tight"))
    assert opt_off.max_grad_norm is None and opt_off.clip_stats is None
    # a bound no gradient reaches: coef is exactly 1 and the separate launches leave the bits the run without the flag leaves
    assert opt_huge.max_grad_norm == 1e30 and float(opt_huge.clip_stats[1]) == 1.0
    for x, y in zip(off, huge):
        assert torch.equal(x, y)
    norm, coef = opt_tight.clip_stats.tolist()
    assert math.isfinite(norm) and math.isfinite(coef) and 0.0 < coef < 1.0, (norm, coef)
    assert all(bool(torch.isfinite(p).all()) for p in tight)
    assert any(not torch.equal(x, y) for x, y in zip(before, tight)), "no parameter moved"
    assert any(not torch.equal(x, y) for x, y in zip(off, tight))


def _validation_records(log_dir):
    """The records of the run's validation points (the run directory's metrics.jsonl; `_step` is the meta-batch index)."""
    files = glob.glob(os.path.join(log_dir, "runs", "*", "metrics.jsonl"))
    assert len(files) == 1, files
    with open(files[0]) as fh:
        return [r for r in map(json.loads, fh) if "val/loss" in r]


@pytest.mark.parametrize("model", sorted(CLI))
def test_cli_logs_the_clip_at_its_validation_points(model, tmp_path_factory, monkeypatch):
    """Two meta-batches with a validation point after each (fumi and maml skip the one at batch 0): with the flag the record of every
    validation point carries train/grad_norm and train/clip_coef, the last one the optimizer's clip_stats; without it neither."""
    root = tmp_path_factory.mktemp(f"clip_log_{model}")
    monkeypatch.chdir(root)
    _, _, opt = _cli(model, "1e-3", str(root / "tight"), epochs=1, eval_freq=1)
    recs = _validation_records(str(root / "tight"))
    assert [r["_step"] for r in recs] == ([0, 1] if model == "am3" else [1])
    for r in recs:
        assert math.isfinite(r["train/grad_norm"]) and r["train/grad_norm"] > 0.0 and 0.0 < r["train/clip_coef"] < 1.0
    norm, coef = opt.clip_stats.tolist()
    assert (recs[-1]["train/grad_norm"], recs[-1]["train/clip_coef"]) == (norm, coef)
    _cli(model, None, str(root / "off"), epochs=1, eval_freq=1)
    recs = _validation_records(str(root / "off"))
    assert recs and all("train/grad_norm" not in r and "train/clip_coef" not in r for r in recs)
