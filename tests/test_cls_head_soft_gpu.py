"""GPU parity of the soft-target form of the fused classification head (fumi_hip_cls_head_step_soft, csrc/clshead.hip; DESIGN.md
section 25) against the float64 restatement tests/cls_head_soft_ref.py (tied to torch.autograd at 1e-12 by
tests/test_pretrain_mix_cpu.py), on the inputs of the hard form's test.

Tolerances are the hard form's (tests/test_cls_head_gpu.py): 1e-4 of the largest magnitude of the compared tensor, predictions compared
only where the float64 top-two logit margin exceeds 1e-5.  The measured errors of a run are kept in profiles/pretrain_mix/gpu_tests.log."""
import numpy as np
import pytest
import torch

from cls_head_ref import ST_LABEL_RANGE
from cls_head_soft_ref import cls_head_soft_ref
from helpers import rel_to_max
from test_cls_head_gpu import GRAD_SCALE, MARGIN, TOL, _case

pytestmark = pytest.mark.gpu

# the hard form's tile edges (tests/test_cls_head_gpu.py), without its two largest shapes
SHAPES = [(1, 32, 2), (33, 96, 5), (130, 640, 64), (257, 64, 1024)]
CASES = [(0.1, 1.0, False), (0.0, 0.3, True), (0.1, 0.7, True)]          # (eps, lam, with y_b)
KEYS = ("loss", "correct", "preds", "dfeats", "gW", "gb")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _second_labels(y, M, F, C):
    """A permutation of y that leaves at least one row with y_a == y_b (row 0 keeps its place)."""
    g = torch.Generator().manual_seed(7919 * M + 31 * F + C)
    perm = torch.cat((torch.zeros(1, dtype=torch.int64), 1 + torch.randperm(M - 1, generator=g)))
    y_b = y[perm]
    assert sorted(y_b.tolist()) == sorted(y.tolist()) and bool((y_b == y).any())
    return y_b


def _check(got, ref, what):
    e = abs(float(got["loss"]) - ref["loss"]) / max(abs(ref["loss"]), 1e-5)
    print(f"{what} loss: relative error {e:.3e}")
    assert e <= TOL, (what, "loss", e)
    safe = ref["margin"] > MARGIN
    assert np.array_equal(got["preds"].cpu().numpy()[safe], ref["preds"][safe]), what
    assert abs(float(got["correct"]) - ref["correct"]) <= int((~safe).sum()), what
    for k in ("dfeats", "gW", "gb"):
        e = rel_to_max(got[k].cpu(), ref[k])
        print(f"{what} {k}: rel-to-max error {e:.3e}")
        assert e <= TOL, (what, k, e)


@pytest.mark.parametrize("eps,lam,mixed", CASES)
@pytest.mark.parametrize("M,F,C", SHAPES)
def test_soft_head_matches_float64_and_is_reproducible(M, F, C, eps, lam, mixed, dev, ws):
    from fumi_amd import hip
    x, y, W, b = _case(M, F, C)
    y_b = _second_labels(y, M, F, C) if mixed else None
    ref = cls_head_soft_ref(x.numpy(), y.numpy(), W.numpy(), b.numpy(), GRAD_SCALE, y_b=None if y_b is None else y_b.numpy(),
                            lam=lam, smoothing=eps)
    xd, yd, Wd, bd = (t.to(dev) for t in (x, y, W, b))
    kw = dict(y_b=None if y_b is None else y_b.to(dev), lam=lam, smoothing=eps)
    out = hip.cls_head_step_soft(ws, xd, yd, Wd, bd, need_grad=True, grad_scale=GRAD_SCALE, **kw)
    assert ws.read_status() == 0
    _check(out, ref, f"soft ({M},{F},{C}) eps {eps} lam {lam}")
    fwd = hip.cls_head_step_soft(ws, xd, yd, Wd, bd, need_grad=False, **kw)
    assert fwd["dfeats"] is None and fwd["gW"] is None and fwd["gb"] is None
    for k in ("loss", "correct", "preds"):
        assert torch.equal(fwd[k], out[k]), k
    again = hip.cls_head_step_soft(ws, xd, yd, Wd, bd, need_grad=True, grad_scale=GRAD_SCALE, **kw)
    for k in KEYS:
        assert torch.equal(again[k], out[k]), k


@pytest.mark.parametrize("M,F,C", SHAPES)
def test_soft_head_without_smoothing_or_mix_returns_the_bits_of_the_hard_head(M, F, C, dev, ws):
    from fumi_amd import hip
    x, y, W, b = (t.to(dev) for t in _case(M, F, C))
    hard = hip.cls_head_step(ws, x, y, W, b, need_grad=True, grad_scale=GRAD_SCALE)
    soft = hip.cls_head_step_soft(ws, x, y, W, b, y_b=None, lam=1.0, smoothing=0.0, need_grad=True, grad_scale=GRAD_SCALE)
    assert ws.read_status() == 0
    for k in KEYS:
        assert torch.equal(soft[k], hard[k]), k
    fwd = hip.cls_head_step_soft(ws, x, y, W, b, need_grad=False)
    for k in ("loss", "correct", "preds"):
        assert torch.equal(fwd[k], hard[k]), k


def test_second_label_out_of_range_sets_the_status_bit_and_drops_the_row(dev, ws):
    from fumi_amd import hip
    M, F, C = 33, 96, 5
    x, y, W, b = _case(M, F, C)
    y_b = _second_labels(y, M, F, C)
    y_b[7] = C
    y_b[20] = -1
    ref = cls_head_soft_ref(x.numpy(), y.numpy(), W.numpy(), b.numpy(), GRAD_SCALE, y_b=y_b.numpy(), lam=0.7, smoothing=0.1)
    assert ref["status"] == ST_LABEL_RANGE and not ref["dfeats"][7].any() and not ref["dfeats"][20].any()
    out = hip.cls_head_step_soft(ws, *(t.to(dev) for t in (x, y, W, b)), y_b=y_b.to(dev), lam=0.7, smoothing=0.1, need_grad=True,
                                 grad_scale=GRAD_SCALE)
    assert ws.read_status() & hip.ST_LABEL_RANGE
    assert ws.read_status() == 0
    assert float(out["dfeats"][7].abs().max()) == 0.0 and float(out["dfeats"][20].abs().max()) == 0.0
    _check(out, ref, "out-of-range second label")


@pytest.mark.parametrize("kw", [dict(smoothing=1.0), dict(smoothing=-0.1), dict(smoothing=float("nan")), dict(lam=1.5, mixed=True),
                                dict(lam=-0.1, mixed=True), dict(lam=float("nan"), mixed=True), dict(lam=0.5)])
def test_invalid_arguments_are_refused_before_any_launch(kw, dev, ws):
    from fumi_amd import hip
    M, F, C = 8, 32, 5
    x = torch.zeros(M, F, device=dev)
    y = torch.full((M,), C, dtype=torch.int64, device=dev)                       # a launch would set the status bit
    W, b = torch.zeros(C, F, device=dev), torch.zeros(C, device=dev)
    kw = dict(kw)
    y_b = y if kw.pop("mixed", False) else None
    for need_grad in (False, True):
        with pytest.raises(hip.FumiHipError, match="fumi_hip_cls_head_step_soft.*invalid argument"):
            hip.cls_head_step_soft(ws, x, y, W, b, y_b=y_b, need_grad=need_grad, **kw)
    assert ws.read_status() == 0
