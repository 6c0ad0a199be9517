"""GPU suite of the fused SGD / AdamW optimizers (fumi_amd/optim.py, csrc/adam.hip, csrc/gemm.hip: launch_reduce_multi_final).

Each rule against its torch class (the project's Adam bound: rel-to-max <= 2e-7 on the parameters -- the element rules restated in
fp32 differ from torch's single-tensor code by 5e-8 of the tensor maximum over five steps), checkpoint interchange and resume, the
fold of the update into the FuMI meta-step's last launch against the separate launches (BIT FOR BIT, as tests/test_folded_step_gpu.py
asks of Adam), the statistics publication riding on the stand-alone optimizer launch, and the command line with each --optim."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import rel_to_max
from oracle import casegen as cg

pytestmark = pytest.mark.gpu

STEPS = 5
# State tensors (momentum_buffer, exp_avg, exp_avg_sq) are compared as well; the issue's 2e-7 is a bound on the PARAMETERS.  One
# step of a moment is four individually rounded fp32 operations here (contraction is off: common.h) and three in torch's GPU
# kernels (lerp / add-with-alpha use a fused multiply-add), each off by at most half an ulp (2^-24) of a quantity of the tensor's
# scale, and a moment carries its error from step to step (decay 0.9 .. 0.999): the two can differ by STEPS * 7 * 2^-24 of the
# tensor maximum.  (This comparison is what found 1 - beta2 formed from a beta2 that had been rounded to fp32 in a draft of
# the AdamW rule: exp_avg_sq was off by 1.3e-5 of its maximum, the rounding error of 0.999f relative to 0.001, with the parameters
# inside 2e-7 all the same; the entry points now take the betas as doubles and fold 1 - beta in double, as torch does.)
STATE_TOL = STEPS * 7 * 2.0 ** -24
SHAPES = [(256, 2048), (256,), (64, 256), (65,), (7, 3), (1,)]
RULES = [("SGD", dict(lr=3e-3, momentum=0.9, weight_decay=5e-4)), ("SGD", dict(lr=3e-3, momentum=0.0, weight_decay=5e-4)),
         ("AdamW", dict(lr=3e-3, weight_decay=0.0)), ("AdamW", dict(lr=3e-3, weight_decay=1e-2))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _classes(name):
    from fumi_amd import optim
    return getattr(optim, name), getattr(torch.optim, name)


def _forbid_torch_step(monkeypatch, tcls):
    """The fused path must be the one that runs: torch's own step raises for the rest of the test.  Returns the original, for
    the reference optimizer."""
    orig = tcls.step

    def refuse(self, *a, **k):
        raise AssertionError(f"{tcls.__name__}.step of torch ran: the fused launch did not take the step")
    monkeypatch.setattr(tcls, "step", refuse)
    return orig


@pytest.mark.parametrize("name,kw", RULES)
def test_fused_rule_matches_its_torch_class(name, kw, dev, monkeypatch):
    cls, tcls = _classes(name)
    g = torch.Generator().manual_seed(0)
    pa = [torch.randn(*s, generator=g).to(dev).requires_grad_(True) for s in SHAPES]
    pb = [p.detach().clone().requires_grad_(True) for p in pa]
    oa, ob = cls(pa, **kw), tcls(pb, **kw)
    torch_step = _forbid_torch_step(monkeypatch, tcls)
    steps = STEPS
    for it in range(steps):
        for grp in oa.param_groups + ob.param_groups:
            grp["lr"] = kw["lr"] * (it + 1) / steps                          # a new Python float every step, as a schedule sets it
        for x, y in zip(pa, pb):
            gr = torch.randn(x.shape, generator=g).to(dev)
            x.grad, y.grad = gr.clone(), gr.clone()
        if it % 2:
            oa.step_fused()
        else:
            oa.step()
        torch_step(ob)
    torch.cuda.synchronize()
    errs = [rel_to_max(x.detach().cpu(), y.detach().cpu()) for x, y in zip(pa, pb)]
    print(f"{name} {kw}: rel-to-max per tensor {errs}")
    assert max(errs) <= 2e-7, errs
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert set(sa["state"][k]) == set(sb["state"][k])
        if "step" in sa["state"][k]:
            assert float(sa["state"][k]["step"]) == float(sb["state"][k]["step"]) == float(steps)
        for key in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
            if key in sa["state"][k]:
                err = rel_to_max(sa["state"][k][key].cpu(), sb["state"][k][key].cpu())
                print(f"  state[{k}][{key}]: rel-to-max {err:.3e}")
                assert err <= STATE_TOL, (key, err)
    if name == "SGD":
        assert (len(sa["state"]) > 0) == (kw["momentum"] != 0)
    ob.load_state_dict(sa)                                                   # checkpoints interchange, both directions
    oa.load_state_dict(sb)
    for x, y in zip(pa, pb):
        x.grad, y.grad = torch.ones_like(x), torch.ones_like(y)
    oa.step(); torch_step(ob)                                                # ... and the fused launch goes on from torch's state
    for x, y in zip(pa, pb):
        assert rel_to_max(x.detach().cpu(), y.detach().cpu()) <= 2e-7


def test_sgd_resumed_from_a_state_dict_equals_an_uninterrupted_run(dev, monkeypatch):
    """First step (no momentum buffer: the kernel writes it) and a resumed run (buffer present: not a first step) both fused."""
    from fumi_amd.optim import SGD
    _forbid_torch_step(monkeypatch, torch.optim.SGD)
    kw = dict(lr=3e-3, momentum=0.9, weight_decay=5e-4)
    g0 = torch.Generator().manual_seed(7)
    P = [torch.randn(*s, generator=g0).to(dev) for s in SHAPES]
    G = [[torch.randn(*s, generator=g0).to(dev) for s in SHAPES] for _ in range(4)]

    def go(params, opt, its):
        for it in its:
            for p, gr in zip(params, G[it]):
                p.grad = gr.clone()
            opt.step()

    pa = [p.clone().requires_grad_(True) for p in P]
    oa = SGD(pa, **kw)
    go(pa, oa, range(4))
    pb = [p.clone().requires_grad_(True) for p in P]
    ob = SGD(pb, **kw)
    go(pb, ob, range(2))
    ckpt = ob.state_dict()
    pc = [p.detach().clone().requires_grad_(True) for p in pb]
    oc = SGD(pc, **kw)
    oc.load_state_dict(ckpt)
    go(pc, oc, range(2, 4))
    torch.cuda.synchronize()
    for x, y in zip(pa, pc):
        assert torch.equal(x, y)
    for k, st in oa.state_dict()["state"].items():
        assert torch.equal(st["momentum_buffer"], oc.state_dict()["state"][k]["momentum_buffer"])


# ---- the fold into the meta-step's last launch ----------------------------------------------------------------------------------
FOLD_RULES = ["SGD", "adamw", "adamw_lin_schedule"]


@functools.lru_cache(maxsize=None)
def _run(rule, fold, T, steps=6):
    from fumi_amd import optim
    from fumi_amd.models.fumi import FUMI
    from fumi_amd.utils import utils as U
    dev = torch.device("cuda:0")
    c = dict(B=8, N=5, K=5, Q=8, D=512, hid=[256, 64], Dt=48, Ht=64)
    torch.manual_seed(3)
    m = FUMI(n_way=c["N"], im_emb_dim=c["D"], im_hid_dim=c["hid"], text_encoder="BERT", text_emb_dim=c["Dt"], text_hid_dim=c["Ht"],
             dropout_rate=0.0, norm_hypernet=True).to(dev)
    sched = None
    if rule == "SGD":
        opt = optim.SGD(m.parameters(), lr=1e-2, momentum=0.9, weight_decay=5e-4)
    else:
        opt = optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)
        if rule == "adamw_lin_schedule":
            sched = U._linear_warmup_schedule(opt, 3, 20)
    folded = []
    if not fold:
        opt.defer_step = lambda device: False                           # the ordinary path: gradient launch, then the optimizer's launch
    else:
        fin = opt.finish_deferred
        opt.finish_deferred = lambda device: folded.append(not fin(device))   # (True: the step had folded the update)
    args = SimpleNamespace(device=dev, num_train_adapt_steps=T, num_test_adapt_steps=T, step_size=0.05, first_order=False, num_ways=c["N"],
                           batch_size=c["B"])
    losses, lrs = [], []
    for i in range(steps):
        ep = cg.make_episodes(100 + i, c["B"], c["N"], c["K"], c["Q"], c["D"], c["Dt"])
        lrs.append(opt.param_groups[0]["lr"])
        loss, acc, _, _ = m.evaluate(args, cg.to_batch(ep), opt, "train")
        if sched is not None:
            sched.step()
        losses.append((float(loss), float(acc)))
    torch.cuda.synchronize()
    st = opt.state_dict()["state"]
    state = [st[i][k].clone() if torch.is_tensor(st[i][k]) else st[i][k] for i in sorted(st) for k in sorted(st[i])]
    keys = [k for i in sorted(st) for k in sorted(st[i])]
    return dict(losses=losses, params=[p.detach().clone() for p in m.parameters()], grads=[p.grad.detach().clone() for p in m.parameters()],
                state=state, keys=keys, folded=folded, lrs=lrs)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("rule", FOLD_RULES)
def test_folded_step_is_bit_identical_to_the_separate_launches(rule, T, recwarn):
    a, b = _run(rule, True, T), _run(rule, False, T)
    assert len(a["folded"]) == 5 and all(a["folded"]), a["folded"]          # steps 2..6 registered AND were folded by the meta-step
    assert a["losses"] == b["losses"] and a["keys"] == b["keys"] and a["lrs"] == b["lrs"]
    assert len(a["state"]) > 0
    for x, y in zip(a["params"] + a["grads"] + a["state"], b["params"] + b["grads"] + b["state"]):
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))
    assert all(np.isfinite(v) for t in a["losses"] for v in t)
    if rule == "adamw_lin_schedule":
        assert len(set(a["lrs"])) == len(a["lrs"]), a["lrs"]                 # group["lr"] really differed from step to step
        assert not [w for w in recwarn.list if "lr_scheduler.step()" in str(w.message)]
    if "step" in a["keys"]:
        assert all(float(s) == 6.0 for s, k in zip(a["state"], a["keys"]) if k == "step")


@pytest.mark.parametrize("rule", FOLD_RULES)
def test_statistics_ride_on_the_stand_alone_optimizer_launch(rule):
    """Fold disabled (`defer_step` returns False): `lazy.scalars(defer=True)` waits for "the next optimizer launch of this
    workspace", whichever rule's it is.  The losses read through `lazy` are those of the folded run, and they move."""
    a, b = _run(rule, True, 1), _run(rule, False, 1)
    assert b["folded"] == []
    assert [t[0] for t in b["losses"]] == [t[0] for t in a["losses"]]
    assert len({t[0] for t in b["losses"]}) == len(b["losses"])


# ---- the command line -------------------------------------------------------------------------------------------------------------
CLI = [("fumi", "SGD", ["--num_train_adapt_steps", "1", "--num_test_adapt_steps", "1", "--step_size", "0.05"]),
       ("fumi", "adamw", ["--num_train_adapt_steps", "1", "--num_test_adapt_steps", "1", "--step_size", "0.05"]),
       ("am3", "adamw_lin_schedule", []),
       ("maml", "SGD", ["--num_train_adapt_steps", "1", "--num_test_adapt_steps", "1"])]


@pytest.mark.parametrize("model,optim_name,extra", CLI)
def test_cli_trains_with_each_optimizer_on_the_fused_launch(model, optim_name, extra, dev, tmp_path, monkeypatch):
    from fumi_amd import main as cli
    from fumi_amd.utils import utils as U
    monkeypatch.chdir(tmp_path)
    tcls = torch.optim.SGD if optim_name == "SGD" else torch.optim.AdamW
    _forbid_torch_step(monkeypatch, tcls)
    made = {}
    init_model = U.init_model

    def capture(args, dictionary, *a, **k):
        m = init_model(args, dictionary, *a, **k)
        made["model"], made["before"] = m, [p.detach().clone() for p in m.parameters()]
        return m
    monkeypatch.setattr(U, "init_model", capture)
    argv = ["--model", model, "--optim", optim_name, "--dataset", "synthetic", "--text_encoder", "BERT", "--image_embedding_model", "resnet-34", "--im_emb_dim", "512",
            "--text_emb_dim", "32", "--batch_size", "4", "--num_shots", "2", "--num_ways", "5", "--num_shots_test", "3",
            "--epochs", "12", "--eval_freq", "6", "--num_ep_test", "8", "--lr", "1e-3", "--dropout", "0",
            "--log_dir", str(tmp_path / "res"), "--synthetic_classes", "16", "--wandb_offline"] + extra
    args = cli.parse_args(argv)
    assert args.device.type == "cuda"
    res = cli.main(args)
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    after = list(made["model"].parameters())
    assert all(bool(torch.isfinite(p).all()) for p in after)
    moved = [not torch.equal(x, y.detach()) for x, y in zip(made["before"], after) if y.requires_grad]
    assert moved and any(moved), "no parameter moved"
