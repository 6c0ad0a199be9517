"""GPU parity of the fused cosine classifier head (fumi_hip_cos_cls_head_step, csrc/coshead.hip) against the
float64 restatement tests/cos_cls_head_ref.py (held to finite differences and torch.autograd by tests/test_cos_cls_head_cpu.py), over
the cases of tests/cos_cls_head_cases.py.

Tolerances are the linear head's (tests/test_cls_head_gpu.py): 1e-4 of the largest magnitude of dfeats and gW, 1e-4 relative for the
loss and for dtau -- dtau relative to sum |dz k| of the reference, since its sum cancels -- and predictions compared only where the
float64 top-two logit margin exceeds 1e-5; tests/test_cos_cls_head_cpu.py asserts that at most one row in a hundred of each case lies
under it.  torch's fp32 autograd on the device (F.normalize, F.cross_entropy) is held to the same float64 values as a second
witness."""
import numpy as np
import pytest
import torch

from cls_head_ref import ST_LABEL_RANGE
from cos_cls_head_cases import GRAD_SCALE, INPUTS, MARGIN, SHAPES, TARGETS, TOL, case, target_kw
from cos_cls_head_ref import cos_cls_head_ref
from helpers import rel_to_max

pytestmark = pytest.mark.gpu
KEYS = ("loss", "correct", "preds", "dfeats", "gW", "dtau")
_REFS = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _ref(M, F, C, inputs, target):
    """(host inputs, host keyword arguments, float64 reference), computed once per case."""
    key = (M, F, C, inputs, target)
    if key not in _REFS:
        x, y, W, tau = case(M, F, C, inputs)
        kw = target_kw(target, y, M, F, C)
        ref = cos_cls_head_ref(x.numpy(), y.numpy(), W.numpy(), tau.numpy(), GRAD_SCALE,
                               **{**kw, "y_b": None if kw["y_b"] is None else kw["y_b"].numpy()})
        _REFS[key] = ((x, y, W, tau), kw, ref)
    return _REFS[key]


def _check(got, ref, what):
    e = abs(float(got["loss"]) - ref["loss"]) / max(abs(ref["loss"]), 1e-5)
    print(f"{what} loss: relative error {e:.3e}")
    assert e <= TOL, (what, "loss", e)
    safe = ref["margin"] > MARGIN
    assert np.array_equal(got["preds"].cpu().numpy()[safe], ref["preds"][safe]), what
    if "correct" in got:
        assert abs(float(got["correct"]) - ref["correct"]) <= int((~safe).sum()), what
    e = abs(float(got["dtau"]) - ref["dtau"]) / max(ref["dtau_abs"], 1e-30)
    print(f"{what} dtau: error relative to sum |dz k| {e:.3e}")
    assert e <= TOL, (what, "dtau", e)
    for k in ("dfeats", "gW"):
        e = rel_to_max(got[k].cpu(), ref[k])
        print(f"{what} {k}: rel-to-max error {e:.3e}")
        assert e <= TOL, (what, k, e)


def _torch_witness(x, y, W, tau, y_b, lam, smoothing):
    """The same quantities from torch's fp32 autograd on the device."""
    import torch.nn.functional as Fn
    C = W.shape[0]
    xt, Wt, tt = (t.clone().requires_grad_(True) for t in (x, W, tau))
    z = tt * (Fn.normalize(xt, dim=1) @ Fn.normalize(Wt, dim=1).T)
    t = (1.0 - smoothing) * (lam * Fn.one_hot(y, C).float() + (1.0 - lam) * Fn.one_hot(y if y_b is None else y_b, C).float()) + smoothing / C
    loss = Fn.cross_entropy(z, t)
    (GRAD_SCALE * loss).backward()
    return dict(loss=loss.detach(), preds=z.detach().argmax(dim=1), dfeats=xt.grad, gW=Wt.grad, dtau=tt.grad)


@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("inputs", INPUTS)
@pytest.mark.parametrize("M,F,C", SHAPES)
def test_head_step_matches_float64_and_is_reproducible(M, F, C, inputs, target, dev, ws):
    from fumi_amd import hip
    (x, y, W, tau), kw, ref = _ref(M, F, C, inputs, target)
    xd, yd, Wd, td = (t.to(dev) for t in (x, y, W, tau))
    kw = {**kw, "y_b": None if kw["y_b"] is None else kw["y_b"].to(dev)}
    what = f"({M},{F},{C}) {inputs} {target}"
    out = hip.cos_cls_head_step(ws, xd, yd, Wd, td, need_grad=True, grad_scale=GRAD_SCALE, **kw)
    assert ws.read_status() == 0
    _check(out, ref, "fused " + what)
    # the forward form and a second call: the same bits
    fwd = hip.cos_cls_head_step(ws, xd, yd, Wd, td, need_grad=False, **kw)
    assert fwd["dfeats"] is None and fwd["gW"] is None and fwd["dtau"] is None
    for k in ("loss", "correct", "preds"):
        assert torch.equal(fwd[k], out[k]), k
    again = hip.cos_cls_head_step(ws, xd, yd, Wd, td, need_grad=True, grad_scale=GRAD_SCALE, **kw)
    for k in KEYS:
        assert torch.equal(again[k], out[k]), k
    assert ws.read_status() == 0
    # second witness: torch's fp32 autograd, against the same float64 values
    _check(_torch_witness(xd, yd, Wd, td, **kw), ref, "torch fp32 " + what)


def test_label_out_of_range_sets_the_status_bit_and_drops_the_row(dev, ws):
    """The reference leaves the row out exactly (tests/test_cos_cls_head_cpu.py: it equals the reference of the other rows)."""
    from fumi_amd import hip
    M, F, C = 17, 96, 5
    x, y, W, tau = case(M, F, C)
    kw = target_kw("soft", y, M, F, C)
    y_b = kw.pop("y_b").clone()
    y_b[7] = C
    ref = cos_cls_head_ref(x.numpy(), y.numpy(), W.numpy(), tau.numpy(), GRAD_SCALE, y_b=y_b.numpy(), **kw)
    assert ref["status"] == ST_LABEL_RANGE and not ref["dfeats"][7].any()
    out = hip.cos_cls_head_step(ws, *(t.to(dev) for t in (x, y, W, tau)), y_b=y_b.to(dev), need_grad=True, grad_scale=GRAD_SCALE, **kw)
    assert ws.read_status() & hip.ST_LABEL_RANGE
    assert ws.read_status() == 0                                                  # (reading clears the word)
    assert float(out["dfeats"][7].abs().max()) == 0.0
    _check(out, ref, "out-of-range label")
    y = y.clone()
    y[16] = -1                                                                    # in y_a, in the ragged tile, the hard target
    ref = cos_cls_head_ref(x.numpy(), y.numpy(), W.numpy(), tau.numpy(), GRAD_SCALE)
    out = hip.cos_cls_head_step(ws, *(t.to(dev) for t in (x, y, W, tau)), need_grad=True, grad_scale=GRAD_SCALE)
    assert ws.read_status() & hip.ST_LABEL_RANGE
    assert float(out["dfeats"][16].abs().max()) == 0.0
    _check(out, ref, "out-of-range first label")


def test_zero_rows_are_the_zero_direction_and_harm_nothing_else(dev, ws):
    from fumi_amd import hip
    M, F, C = 17, 96, 5
    x, y, W, tau = case(M, F, C)
    x[3] = 0.0
    W[2] = 0.0
    x[16] = 1e-20                                                                 # a norm below eps, not zero
    ref = cos_cls_head_ref(x.numpy(), y.numpy(), W.numpy(), tau.numpy(), GRAD_SCALE, smoothing=0.1)
    out = hip.cos_cls_head_step(ws, *(t.to(dev) for t in (x, y, W, tau)), smoothing=0.1, need_grad=True, grad_scale=GRAD_SCALE)
    assert ws.read_status() == 0
    for k in ("loss", "dfeats", "gW", "dtau"):
        assert bool(torch.isfinite(out[k]).all()), k
    assert float(out["dfeats"][3].abs().max()) == 0.0 and float(out["dfeats"][16].abs().max()) == 0.0
    assert float(out["gW"][2].abs().max()) == 0.0
    _check(out, ref, "zero rows")


@pytest.mark.parametrize("M,F,C,kw,why", [(8, 48, 5, {}, "not supported"), (8, 64, 1025, {}, "not supported"), (0, 64, 5, {}, "invalid argument"),
                                          (8, 32, 5, dict(lam=0.5), "invalid argument")])
def test_what_the_entry_cannot_run_is_refused_before_any_launch(M, F, C, kw, why, dev, ws):
    from fumi_amd import hip
    x = torch.zeros(M, F, device=dev)
    y = torch.full((M,), C, dtype=torch.int64, device=dev)                       # a launch would set the status bit
    W, tau = torch.zeros(C, F, device=dev), torch.ones(1, device=dev)
    for need_grad in (False, True):
        with pytest.raises(hip.FumiHipError, match="fumi_hip_cos_cls_head_step"):
            hip.cos_cls_head_step(ws, x, y, W, tau, need_grad=need_grad, **kw)
    rc = hip.lib().fumi_hip_cos_cls_head_step(ws.handle, hip._stream(dev), M, F, C, x.data_ptr(), y.data_ptr(), None, kw.get("lam", 1.0),
                                              0.0, W.data_ptr(), tau.data_ptr(), 1.0, tau.data_ptr(), tau.data_ptr(), None, None, None,
                                              None)
    assert why in hip.lib().fumi_hip_strerror(rc).decode()
    assert ws.read_status() == 0
