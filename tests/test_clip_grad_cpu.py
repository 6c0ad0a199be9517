"""CPU suite of --max_grad_norm (fumi_amd/optim.py, fumi_amd/utils/utils.py, csrc/adam.hip): the flag and what `init_optim` does
with it, the optimizer classes' bookkeeping around the value (state_dict layout, pickling), the route CPU tensors take (torch's
own clip, then torch's own step), the fairness of the clip tests' inputs, and the compiled kernels' resources."""
import copy
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import clip_ref as R
from conftest import ROOT
from fumi_amd.optim import SGD, Adam, AdamW, clip_log
from test_optim_fused_cpu import _resources

CLASSES = [(Adam, torch.optim.Adam, dict(lr=1e-2, weight_decay=5e-4)),
           (AdamW, torch.optim.AdamW, dict(lr=1e-2, weight_decay=1e-2)),
           (SGD, torch.optim.SGD, dict(lr=0.1, momentum=0.9, weight_decay=5e-4)),
           (SGD, torch.optim.SGD, dict(lr=0.1, momentum=0.0, weight_decay=5e-4))]


def test_parser_has_the_flag_and_clip_still_abbreviates_clip_latent_dim():
    from fumi_amd.utils import utils as U
    assert U.parser().parse_args([]).max_grad_norm is None
    a = U.parser().parse_args(["--max_grad_norm", "0.5", "--clip", "64"])
    assert a.max_grad_norm == 0.5 and a.clip_latent_dim == 64
    assert "--max_grad_norm" in [f for f, _ in U._ENGINE_FLAGS]


@pytest.mark.parametrize("optim", ["adam", "SGD", "adamw", "adamw_lin_schedule"])
@pytest.mark.parametrize("value", [None, 0.25])
def test_init_optim_hands_the_value_to_every_choice(optim, value):
    from fumi_amd.utils import utils as U
    args = SimpleNamespace(optim=optim, lr=3e-4, weight_decay=5e-4, momentum=0.8, num_warmup_steps=3, epochs=20, max_grad_norm=value)
    o = U.init_optim(args, torch.nn.Linear(4, 3))
    o = o[0] if type(o) is tuple else o
    assert o.max_grad_norm == value and o.clip_stats is None
    assert "max_grad_norm" not in o.param_groups[0] and "max_grad_norm" not in o.defaults


@pytest.mark.parametrize("bad", [0.0, -1.0, float("inf"), float("nan")])
def test_the_value_must_be_finite_and_positive(bad):
    with pytest.raises(ValueError):
        Adam([torch.zeros(3, requires_grad=True)], max_grad_norm=bad)


def _pair(cls, tcls, kw, max_norm, steps=4):
    g = torch.Generator().manual_seed(2)
    P = [torch.randn(s, generator=g) for s in ((6, 5), (7,), (1,))]
    pa = [p.clone().requires_grad_(True) for p in P]
    pb = [p.clone().requires_grad_(True) for p in P]
    oa, ob = cls(pa, max_grad_norm=max_norm, **kw), tcls(pb, **kw)
    stats = []
    for it in range(steps):
        for x, y in zip(pa, pb):
            gr = torch.randn(x.shape, generator=g) * (10.0 if it % 2 else 0.01)      # clipped and unclipped steps alternate
            x.grad, y.grad = gr.clone(), gr.clone()
        if max_norm is not None:
            stats.append(float(torch.nn.utils.clip_grad_norm_(pb, max_norm)))
        if it % 2:
            oa.step_fused()
        else:
            oa.step()
        ob.step()
    return pa, pb, oa, ob, stats


@pytest.mark.parametrize("cls,tcls,kw", CLASSES)
def test_cpu_step_equals_torchs_clip_followed_by_torchs_step(cls, tcls, kw):
    pa, pb, oa, ob, norms = _pair(cls, tcls, kw, 1.0)
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
        assert torch.equal(x.grad, y.grad)                                    # torch's clip scales p.grad in place on this route
    assert oa._fused_args == {} and oa.defer_step(torch.device("cpu")) is False
    norm, coef = oa.clip_stats.tolist()
    assert norm == pytest.approx(norms[-1], rel=1e-6) and coef < 1.0
    assert clip_log(oa) == {"train/grad_norm": norm, "train/clip_coef": coef}
    assert clip_log(ob) == {} and clip_log(cls(pa, **kw)) == {}


@pytest.mark.parametrize("cls,tcls,kw", CLASSES)
@pytest.mark.parametrize("value", [None, 0.5])
def test_state_dict_keys_are_the_torch_classes(cls, tcls, kw, value):
    pa, pb, oa, ob, _ = _pair(cls, tcls, kw, value, steps=2)
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa.keys() == sb.keys() and sa["state"].keys() == sb["state"].keys()
    assert [set(g) for g in sa["param_groups"]] == [set(g) for g in sb["param_groups"]]
    for k in sa["state"]:
        assert set(sa["state"][k]) == set(sb["state"][k])
    ob.load_state_dict(sa)
    oa.load_state_dict(sb)
    assert oa.max_grad_norm == value


@pytest.mark.parametrize("cls,tcls,kw", CLASSES)
@pytest.mark.parametrize("value", [None, 0.5])
def test_pickle_and_deepcopy_keep_the_value(cls, tcls, kw, value):
    pa, pb, oa, ob, _ = _pair(cls, tcls, kw, value, steps=2)
    for o in (pickle.loads(pickle.dumps(oa)), copy.deepcopy(oa)):
        assert type(o) is cls and o.max_grad_norm == value and o._fused_args == {}
        assert o.state_dict()["state"].keys() == oa.state_dict()["state"].keys()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_float32_numpy_stays_within_half_the_norm_bound_on_every_case(name):
    arrays = R.case_arrays(name)
    ref, got = R.norm64(arrays), R.norm32_numpy(arrays)
    err = abs(got - ref) / ref
    print(f"{name}: float64 norm {ref:.9g}, float32 numpy {got:.9g}, relative error {err:.3e}")
    assert err <= R.NORM_RTOL / 2
    assert R.coef32(ref, ref / 2) == pytest.approx(ref / 2 / (ref + 1e-6), rel=1e-6) and R.coef32(ref, ref * 2) == 1.0
    assert R.coef32(float("inf"), 1.0) == 0.0 and np.isnan(R.coef32(float("nan"), 1.0))


def test_the_new_kernels_compile_without_scratch_or_spills():
    """The four clipped instances, the sum-of-squares kernel and the finish kernel, compiled as build() compiles the file."""
    seen = _resources(os.path.join(ROOT, "fumi_amd", "csrc", "adam.hip"), "-Os")
    hot = {k: v for k, v in seen.items() if "optim_clipped_kernel" in k or "grad_sumsq_kernel" in k or "clip_finish_kernel" in k}
    assert len(hot) == 6, sorted(seen)
    for k, v in hot.items():
        assert v == {"ScratchSize [bytes/lane]": 0, "SGPRs Spill": 0, "VGPRs Spill": 0}, (k, v)
