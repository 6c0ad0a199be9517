"""GPU parity of the distillation form of the fused classification head (fumi_hip_cls_head_step_distill, csrc/clshead.hip; DESIGN.md
section 37) against the float64 restatement tests/cls_head_distill_ref.py (tied to torch.autograd at 1e-12 by
tests/test_cls_head_distill_cpu.py), on the inputs of tests/cls_head_distill_cases.py.

Tolerances are the existing head's (tests/test_cls_head_gpu.py): 1e-4 of the largest magnitude of the compared tensor.  preds, correct
and agree are compared outside the rows whose float64 top-two gap in z or z_t is below 2e-4 max|z|; the CPU suite holds that set to at
most two rows per case.  The measured errors of a run are kept in profiles/distill/gpu_tests.log."""
import numpy as np
import pytest
import torch

from cls_head_distill_cases import CONFIGS, GRAD_SCALE, MAX_SET_ASIDE, SHAPES, TOL, case, set_aside
from cls_head_distill_ref import cls_head_distill_ref
from cls_head_ref import ST_LABEL_RANGE
from helpers import rel_to_max

pytestmark = pytest.mark.gpu
KEYS = ("loss", "loss_parts", "correct", "agree", "preds", "dfeats", "gW", "gb")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _args(c, dev, teacher_scale=1.0):
    """(positional device tensors of hip.cls_head_step_distill, the same as float32 numpy arrays for the restatement)."""
    ts = [c["x"], c["y"], c["W"], c["b"], c["x_t"], teacher_scale * c["W_t"], teacher_scale * c["b_t"]]
    return [t.to(dev) for t in ts], [t.numpy() for t in ts]


def _check(got, ref, what, grads=True):
    for k in ("loss", "loss_ce", "loss_kd"):
        e = abs(float(got[k]) - ref[k]) / max(abs(ref[k]), 1e-5)
        print(f"{what} {k}: relative error {e:.3e}")
        assert e <= TOL, (what, k, e, float(got[k]), ref[k])
    aside = set_aside(ref)
    assert int(aside.sum()) <= MAX_SET_ASIDE
    assert np.array_equal(got["preds"].cpu().numpy()[~aside], ref["preds"][~aside]), what
    assert abs(float(got["correct"]) - ref["correct"]) <= int(aside.sum()), what
    assert abs(float(got["agree"]) - ref["agree"]) <= int(aside.sum()), what
    if not int(aside.sum()):
        assert float(got["correct"]) == ref["correct"] and float(got["agree"]) == ref["agree"], what
    for k in ("dfeats", "gW", "gb") if grads else ():
        e = rel_to_max(got[k].cpu(), ref[k])
        print(f"{what} {k}: rel-to-max error {e:.3e}")
        assert e <= TOL, (what, k, e)


@pytest.mark.parametrize("T,alpha,cw,eps,lam,mixed", CONFIGS)
@pytest.mark.parametrize("M,F,C", SHAPES)
def test_distill_head_matches_float64_and_is_reproducible(M, F, C, T, alpha, cw, eps, lam, mixed, dev, ws):
    from fumi_amd import hip
    c = case(M, F, C)
    y_b = c["y_b"] if mixed else None
    d, h = _args(c, dev)
    ref = cls_head_distill_ref(*h, T, alpha, cw, GRAD_SCALE, y_b=None if y_b is None else y_b.numpy(), lam=lam, smoothing=eps)
    kw = dict(temp=T, alpha=alpha, ce_weight=cw, y_b=None if y_b is None else y_b.to(dev), lam=lam, smoothing=eps)
    out = hip.cls_head_step_distill(ws, *d, need_grad=True, grad_scale=GRAD_SCALE, **kw)
    assert ws.read_status() == 0
    _check(out, ref, f"distill ({M},{F},{C}) T {T} alpha {alpha} ce {cw} eps {eps} lam {lam}")
    assert torch.equal(out["loss_parts"], torch.cat((out["loss_ce"], out["loss_kd"])))
    fwd = hip.cls_head_step_distill(ws, *d, need_grad=False, **kw)
    assert fwd["dfeats"] is None and fwd["gW"] is None and fwd["gb"] is None
    for k in ("loss", "loss_parts", "correct", "agree", "preds"):
        assert torch.equal(fwd[k], out[k]), k
    again = hip.cls_head_step_distill(ws, *d, need_grad=True, grad_scale=GRAD_SCALE, **kw)
    for k in KEYS:
        assert torch.equal(again[k], out[k]), k


@pytest.mark.parametrize("eps,lam,mixed", [(0.0, 1.0, False), (0.1, 0.3, True)])
@pytest.mark.parametrize("M,F,C", SHAPES)
def test_without_a_distillation_weight_the_head_returns_the_bits_of_the_soft_head(M, F, C, eps, lam, mixed, dev, ws):
    from fumi_amd import hip
    c = case(M, F, C)
    d, _ = _args(c, dev)
    soft_kw = dict(y_b=c["y_b"].to(dev) if mixed else None, lam=lam, smoothing=eps)
    soft = hip.cls_head_step_soft(ws, *d[:4], need_grad=True, grad_scale=GRAD_SCALE, **soft_kw)
    kd = hip.cls_head_step_distill(ws, *d, temp=4.0, alpha=0.0, ce_weight=1.0, need_grad=True, grad_scale=GRAD_SCALE, **soft_kw)
    assert ws.read_status() == 0
    for k in ("loss", "correct", "preds", "dfeats", "gW", "gb"):
        assert np.array_equal(kd[k].cpu().numpy(), soft[k].cpu().numpy()), k
    assert torch.equal(kd["loss_ce"], soft["loss"])


@pytest.mark.parametrize("M,F,C", SHAPES)
def test_a_teacher_equal_to_the_student_has_no_distillation_loss(M, F, C, dev, ws):
    """loss_kd is 0 in float64; the bound is the loss tolerance at the scale of the cross-entropy the same sums produce."""
    from fumi_amd import hip
    c = case(M, F, C)
    d, h = _args(c, dev)
    d[4:], h[4:] = d[:1] + d[2:4], h[:1] + h[2:4]
    ref = cls_head_distill_ref(*h, 4.0, 0.5, 0.5, GRAD_SCALE)
    out = hip.cls_head_step_distill(ws, *d, temp=4.0, alpha=0.5, ce_weight=0.5, need_grad=True, grad_scale=GRAD_SCALE)
    assert ws.read_status() == 0
    print(f"teacher = student ({M},{F},{C}): loss_kd {float(out['loss_kd']):.3e}, loss_ce {ref['loss_ce']:.4f}")
    assert abs(ref["loss_kd"]) <= 1e-12 and abs(float(out["loss_kd"])) <= TOL * max(abs(ref["loss_ce"]), 1e-5)
    assert float(out["agree"]) == float(M) == ref["agree"]
    for k in ("dfeats", "gW", "gb"):
        assert rel_to_max(out[k].cpu(), ref[k]) <= TOL, k


@pytest.mark.parametrize("M,F,C", SHAPES)
def test_a_peaked_teacher_gives_finite_outputs_within_the_bound(M, F, C, dev, ws):
    from fumi_amd import hip
    c = case(M, F, C)
    d, h = _args(c, dev, teacher_scale=50.0)
    ref = cls_head_distill_ref(*h, 1.0, 1.0, 0.0, GRAD_SCALE)
    out = hip.cls_head_step_distill(ws, *d, temp=1.0, alpha=1.0, ce_weight=0.0, need_grad=True, grad_scale=GRAD_SCALE)
    assert ws.read_status() == 0
    for k in ("loss", "loss_parts", "correct", "agree", "dfeats", "gW", "gb"):
        assert bool(torch.isfinite(out[k]).all()), k
    _check(out, ref, f"peaked teacher ({M},{F},{C})")


def test_label_out_of_range_sets_the_status_bit_and_drops_the_row(dev, ws):
    from fumi_amd import hip
    M, F, C = 33, 96, 5
    c = case(M, F, C)
    c["y"][7] = C
    d, h = _args(c, dev)
    ref = cls_head_distill_ref(*h, 2.0, 0.9, 0.1, GRAD_SCALE, y_b=c["y_b"].numpy(), lam=0.3, smoothing=0.1)
    assert ref["status"] == ST_LABEL_RANGE and not ref["dfeats"][7].any()
    out = hip.cls_head_step_distill(ws, *d, temp=2.0, alpha=0.9, ce_weight=0.1, y_b=c["y_b"].to(dev), lam=0.3, smoothing=0.1,
                                    need_grad=True, grad_scale=GRAD_SCALE)
    assert ws.read_status() & hip.ST_LABEL_RANGE
    assert ws.read_status() == 0
    assert float(out["dfeats"][7].abs().max()) == 0.0
    _check(out, ref, "out-of-range label")


def _zeros(M, F, C, dev):
    x = torch.zeros(M, F, device=dev)
    y = torch.full((M,), C, dtype=torch.int64, device=dev)                       # a launch would set the status bit
    W, b = torch.zeros(C, F, device=dev), torch.zeros(C, device=dev)
    return [x, y, W, b, x, W, b]


@pytest.mark.parametrize("kw", [dict(temp=0.0), dict(temp=-1.0), dict(temp=float("nan")), dict(temp=float("inf")), dict(alpha=-0.1),
                                dict(alpha=float("nan")), dict(alpha=float("inf")), dict(ce_weight=-1.0), dict(ce_weight=float("nan")),
                                dict(smoothing=1.0), dict(lam=1.5, mixed=True), dict(lam=0.5)])
def test_invalid_arguments_are_refused_before_any_launch(kw, dev, ws):
    from fumi_amd import hip
    a = _zeros(8, 32, 5, dev)
    kw = dict(dict(temp=4.0, alpha=0.5, ce_weight=0.5), **kw)
    y_b = a[1] if kw.pop("mixed", False) else None
    for need_grad in (False, True):
        with pytest.raises(hip.FumiHipError, match="fumi_hip_cls_head_step_distill.*invalid argument"):
            hip.cls_head_step_distill(ws, *a, y_b=y_b, need_grad=need_grad, **kw)
    assert ws.read_status() == 0


def test_a_null_teacher_pointer_is_refused_before_any_launch(dev, ws):
    import ctypes
    from fumi_amd import hip
    M, F, C = 8, 32, 5
    x, y, W, b = _zeros(M, F, C, dev)[:4]
    o = torch.zeros(4, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for null in range(3):
        teacher = [p(x), p(W), p(b)]
        teacher[null] = None
        rc = hip.lib().fumi_hip_cls_head_step_distill(ws.handle, None, M, F, C, p(x), p(y), None, 1.0, 0.0, p(W), p(b), *teacher, 4.0, 0.5,
                                                      0.5, 1.0, p(o[0:1]), p(o[1:3]), p(o[3:4]), p(o[3:4]), None, None, None, None)
        assert rc == -1 and hip.lib().fumi_hip_strerror(rc) == b"invalid argument"
    assert ws.read_status() == 0


@pytest.mark.parametrize("M,F,C", [(8, 48, 5), (8, 64, 1025), (0, 64, 5)])
def test_unsupported_shapes_are_refused(M, F, C, dev, ws):
    from fumi_amd import hip
    a = _zeros(M, F, C, dev)
    for need_grad in (False, True):
        with pytest.raises(hip.FumiHipError, match="fumi_hip_cls_head_step_distill"):
            hip.cls_head_step_distill(ws, *a, temp=4.0, alpha=0.5, ce_weight=0.5, need_grad=need_grad)
    assert ws.read_status() == 0
