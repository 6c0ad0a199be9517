"""CPU suite of the fused SGD / AdamW optimizers (fumi_amd/optim.py, csrc/adam.hip): what `init_optim` hands out for --optim SGD,
adamw and adamw_lin_schedule, the fall-back to torch's own step on CPU tensors, checkpoint interchange with the torch classes, and
the compiled kernels' resources (every rule's stand-alone and folded kernel: no scratch memory, no register spills)."""
import copy
import os
import pickle
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT
from fumi_amd.optim import SGD, AdamW


def _args(optim):
    return SimpleNamespace(optim=optim, lr=3e-4, weight_decay=5e-4, momentum=0.8, num_warmup_steps=3, epochs=20)


def test_init_optim_returns_the_fused_classes_with_the_reference_constructor_values():
    from fumi_amd.utils import utils as U
    model = torch.nn.Linear(4, 3)
    o = U.init_optim(_args("SGD"), model)
    assert type(o) is SGD and isinstance(o, torch.optim.SGD)
    g = o.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["dampening"], g["nesterov"]) == (3e-4, 0.8, 5e-4, 0, False)
    o = U.init_optim(_args("adamw"), model)
    assert type(o) is AdamW and isinstance(o, torch.optim.AdamW)
    g = o.param_groups[0]
    assert (g["lr"], g["weight_decay"], tuple(g["betas"]), g["eps"]) == (3e-4, 0.0, (0.9, 0.999), 1e-8)
    pair = U.init_optim(_args("adamw_lin_schedule"), model)
    assert type(pair) is tuple and len(pair) == 2
    o, sched = pair
    assert type(o) is AdamW and isinstance(sched, torch.optim.lr_scheduler.LambdaLR) and sched.optimizer is o
    assert o.param_groups[0]["weight_decay"] == 0.0 and o.param_groups[0]["initial_lr"] == 3e-4
    assert o.param_groups[0]["lr"] == 0.0                                     # warm-up starts at 0 (3 warm-up steps)


CASES = [(SGD, torch.optim.SGD, dict(lr=0.1, momentum=0.9, weight_decay=5e-4)),
         (SGD, torch.optim.SGD, dict(lr=0.1, momentum=0.0, weight_decay=5e-4)),
         (AdamW, torch.optim.AdamW, dict(lr=1e-2, weight_decay=0.0)),
         (AdamW, torch.optim.AdamW, dict(lr=1e-2, weight_decay=1e-2))]


def _pair(cls, tcls, kw, steps):
    g = torch.Generator().manual_seed(1)
    P = [torch.randn(s, generator=g) for s in ((6, 5), (7,), (1,))]
    pa = [p.clone().requires_grad_(True) for p in P]
    pb = [p.clone().requires_grad_(True) for p in P]
    oa, ob = cls(pa, **kw), tcls(pb, **kw)
    for it in range(steps):
        for grp in oa.param_groups + ob.param_groups:
            grp["lr"] = kw["lr"] * (it + 1) / steps
        for x, y in zip(pa, pb):
            gr = torch.randn(x.shape, generator=g)
            x.grad, y.grad = gr.clone(), gr.clone()
        if it % 2:
            oa.step_fused()
        else:
            oa.step()
        ob.step()
    return pa, pb, oa, ob


@pytest.mark.parametrize("cls,tcls,kw", CASES)
def test_cpu_tensors_fall_back_to_torchs_own_step(cls, tcls, kw):
    pa, pb, oa, ob = _pair(cls, tcls, kw, 5)
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    assert oa._fused_args == {}                                               # nothing was planned for the fused launch
    assert oa.defer_step(torch.device("cpu")) is False


@pytest.mark.parametrize("cls,tcls,kw", CASES)
def test_state_dict_interchanges_with_the_torch_class(cls, tcls, kw):
    pa, pb, oa, ob = _pair(cls, tcls, kw, 3)
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert set(sa["state"][k]) == set(sb["state"][k])
        for name in sa["state"][k]:
            assert torch.equal(torch.as_tensor(sa["state"][k][name]), torch.as_tensor(sb["state"][k][name])), name
    ob.load_state_dict(sa)                                                    # ours -> torch's
    oa.load_state_dict(sb)                                                    # torch's -> ours
    for o in (pickle.loads(pickle.dumps(oa)), copy.deepcopy(oa)):
        assert type(o) is cls and o._fused_args == {}
        assert o.state_dict()["state"].keys() == sa["state"].keys()
    # both go on from the exchanged state in step
    for x, y in zip(pa, pb):
        x.grad, y.grad = torch.ones_like(x), torch.ones_like(y)
    oa.step(); ob.step()
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)


def test_scheduler_sees_the_wrapped_step_and_raises_no_order_warning(recwarn):
    from fumi_amd.utils import utils as U
    model = torch.nn.Linear(4, 3)
    o, sched = U.init_optim(_args("adamw_lin_schedule"), model)
    lrs = []
    for it in range(4):
        for p in model.parameters():
            p.grad = torch.ones_like(p)
        o.step_fused()
        sched.step()
        lrs.append(o.param_groups[0]["lr"])
    assert lrs[0] == pytest.approx(1e-4) and lrs[2] == pytest.approx(3e-4) and lrs[3] < lrs[2]
    assert not [w for w in recwarn.list if "lr_scheduler.step()" in str(w.message)]


def _resources(src, opt):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", opt, "-std=c++17", "-fPIC", "-c", src, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        m = re.search(r"(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\d+)", line)
        if m and name:
            seen[name][m.group(1)] = int(m.group(2))
    return seen


@pytest.mark.parametrize("src,opt,kernel", [("adam.hip", "-Os", "optim_kernel"), ("gemm.hip", "-O3", "reduce_multi_optim_kernel")])
def test_every_rules_kernel_compiles_without_scratch_or_spills(src, opt, kernel):
    """One instance per rule (Adam, AdamW, SGD with momentum, SGD without), compiled as build() compiles the file."""
    seen = _resources(os.path.join(ROOT, "fumi_amd", "csrc", src), opt)
    hot = {k: v for k, v in seen.items() if kernel in k}
    assert len(hot) == 4, sorted(seen)
    for k, v in hot.items():
        assert v == {"ScratchSize [bytes/lane]": 0, "SGPRs Spill": 0, "VGPRs Spill": 0}, (k, v)
