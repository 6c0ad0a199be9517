"""GPU parity of the fused classification head (fumi_hip_cls_head_step, csrc/clshead.hip) against the float64 restatement
tests/cls_head_ref.py (tied to torch.autograd at 1e-12 by tests/test_pretrain_cpu.py).

Tolerances are the ones the fp32 MLP paths are held to against float64: 1e-4 of the largest magnitude of the compared tensor
(LOGIT_TOL / GRAD_TOL, tests/test_hip_parity.py:18-19) and predictions compared only where the float64 top-two logit margin
exceeds 1e-5 (MARGIN, tests/test_hip_parity.py:20).  The four unit ops (linear_fwd, ce_fwd_bwd, linear_bwd_data, linear_bwd_weight)
are held to the same float64 values as a second witness."""
import numpy as np
import pytest
import torch

from cls_head_ref import ST_LABEL_RANGE, cls_head_ref
from helpers import rel_to_max

pytestmark = pytest.mark.gpu
TOL, MARGIN = 1e-4, 1e-5          # tests/test_hip_parity.py:18-20
GRAD_SCALE = 0.25

# (M, F, C): one row and the smallest head; rows and classes off every tile edge; the ResNet-12 width, more than two row tiles plus a
# tail of two rows; the Conv4 width (13 feature blocks, the last a short one); the class limit (8 class blocks per tile); the row limit
SHAPES = [(1, 32, 2), (33, 96, 5), (130, 640, 64), (64, 1600, 100), (257, 64, 1024), (4096, 32, 3)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _case(M, F, C):
    """Inputs seeded per case; logits of standard deviation ~2: a softmax that is neither flat nor saturated."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * F + C)
    x = torch.randn(M, F, generator=g)
    W = torch.randn(C, F, generator=g) * (2.0 / F ** 0.5)
    b = 0.5 * torch.randn(C, generator=g)
    y = torch.randint(0, C, (M,), generator=g)
    return x, y, W, b


def _check(got, ref, what):
    """loss, correct, preds, dfeats, gW, gb of one route against the float64 values."""
    assert abs(float(got["loss"]) - ref["loss"]) <= TOL * max(abs(ref["loss"]), 1e-5), what
    safe = ref["margin"] > MARGIN
    preds = got["preds"].cpu().numpy()
    assert np.array_equal(preds[safe], ref["preds"][safe]), what
    if "correct" in got:
        assert abs(float(got["correct"]) - ref["correct"]) <= int((~safe).sum()), what
    for k in ("dfeats", "gW", "gb"):
        e = rel_to_max(got[k].cpu(), ref[k])
        print(f"{what} {k}: rel-to-max error {e:.3e}")
        assert e <= TOL, (what, k, e)


@pytest.mark.parametrize("M,F,C", SHAPES)
def test_head_step_matches_float64_and_is_reproducible(M, F, C, dev, ws):
    from fumi_amd import hip
    x, y, W, b = _case(M, F, C)
    ref = cls_head_ref(x.numpy(), y.numpy(), W.numpy(), b.numpy(), GRAD_SCALE)
    xd, yd, Wd, bd = (t.to(dev) for t in (x, y, W, b))
    out = hip.cls_head_step(ws, xd, yd, Wd, bd, need_grad=True, grad_scale=GRAD_SCALE)
    assert ws.read_status() == 0
    _check(out, ref, f"fused ({M},{F},{C})")
    # the forward form and a second call: the same bits
    fwd = hip.cls_head_step(ws, xd, yd, Wd, bd, need_grad=False)
    assert fwd["dfeats"] is None and fwd["gW"] is None and fwd["gb"] is None
    for k in ("loss", "correct", "preds"):
        assert torch.equal(fwd[k], out[k]), k
    again = hip.cls_head_step(ws, xd, yd, Wd, bd, need_grad=True, grad_scale=GRAD_SCALE)
    for k in ("loss", "correct", "preds", "dfeats", "gW", "gb"):
        assert torch.equal(again[k], out[k]), k
    # second witness: the four unit ops, against the same float64 values
    z = hip.linear_fwd(ws, xd, Wd, bd)
    loss, dz, preds = hip.ce_fwd_bwd(ws, z, yd)
    dz = dz * GRAD_SCALE
    gW, gb = hip.linear_bwd_weight(ws, dz, xd)
    unit = dict(loss=loss, preds=preds, dfeats=hip.linear_bwd_data(ws, dz, Wd), gW=gW, gb=gb)
    assert ws.read_status() == 0
    _check(unit, ref, f"unit ops ({M},{F},{C})")


def test_label_out_of_range_sets_the_status_bit_and_drops_the_row(dev, ws):
    from fumi_amd import hip
    M, F, C = 33, 96, 5
    x, y, W, b = _case(M, F, C)
    y[7] = C
    ref = cls_head_ref(x.numpy(), y.numpy(), W.numpy(), b.numpy(), GRAD_SCALE)
    assert ref["status"] == ST_LABEL_RANGE and not ref["dfeats"][7].any()
    out = hip.cls_head_step(ws, *(t.to(dev) for t in (x, y, W, b)), need_grad=True, grad_scale=GRAD_SCALE)
    assert ws.read_status() & hip.ST_LABEL_RANGE
    assert ws.read_status() == 0                                                  # (reading clears the word)
    assert float(out["dfeats"][7].abs().max()) == 0.0
    _check(out, ref, "out-of-range label")


@pytest.mark.parametrize("M,F,C", [(8, 48, 5), (8, 64, 1025), (0, 64, 5)])
def test_unsupported_shapes_are_refused(M, F, C, dev, ws):
    from fumi_amd import hip
    x = torch.zeros(M, F, device=dev)
    y = torch.zeros(M, dtype=torch.int64, device=dev)
    W, b = torch.zeros(C, F, device=dev), torch.zeros(C, device=dev)
    with pytest.raises(hip.FumiHipError, match="fumi_hip_cls_head_step"):
        hip.cls_head_step(ws, x, y, W, b, need_grad=False)
    with pytest.raises(hip.FumiHipError, match="fumi_hip_cls_head_step"):
        hip.cls_head_step(ws, x, y, W, b, need_grad=True)
    assert ws.read_status() == 0
