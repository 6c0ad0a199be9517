"""GPU parity of the fused logistic-regression head (fumi_hip_logreg_head_step, csrc/logreghead.hip) against the float64 restatement
tests/logreg_head_ref.py (tied to heavy-ball descent on the primal objective under torch.autograd at 1e-10 by
tests/test_logreg_head_cpu.py).

Tolerances are the ones the fp32 paths are held to against float64 (tests/test_hip_parity.py:18-20): 1e-4 of the largest magnitude on
the logits, 1e-4 relative on the loss, predictions compared where the float64 top-two logit margin exceeds 1e-5 -- and
tests/test_logreg_head_cpu.py asserts that this sets aside no query row of these inputs (smallest margin 1.76e-5) and that a plain
float32 numpy evaluation of the same iteration is within 1e-5 (worst 9.5e-6).  The second witness is the same iteration in torch fp32
ops on the GPU, held to the same float64 logits."""
import numpy as np
import pytest
import torch

from helpers import rel_to_max
from logreg_head_ref import CASES, C_REG, LR, MOMENTUM, ST_CLASS_MISSING, ST_LABEL_RANGE, case_inputs, logreg_head_ref

pytestmark = pytest.mark.gpu
TOL, MARGIN = 1e-4, 1e-5          # tests/test_hip_parity.py:18-20
_REFS = {}


def _ref(case):
    """The inputs and the float64 result of one case, computed once and left unchanged."""
    if case not in _REFS:
        shape, steps, momentum, normalize = case
        inp = case_inputs(*shape)
        _REFS[case] = (inp, logreg_head_ref(*inp, shape[3], steps=steps, lr=LR, momentum=momentum, C=C_REG, normalize=normalize))
    return _REFS[case]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


@pytest.fixture(autouse=True, params=["valu", "mfma"])
def form(request):
    """Every test of this file runs with the fit's K~ A product in both of its forms (the VALU loop, the f32 MFMA)."""
    from fumi_amd import hip
    hip.logreg_set_form(request.param)
    yield request.param
    hip.logreg_set_form(None)


def _gpu(dev, *arrays):
    return [torch.as_tensor(a).to(dev) for a in arrays]


def _check(got, ref, what):
    print(f"{what} loss: {float(got['loss']):.6e} against {ref['loss']:.6e}")
    e = rel_to_max(got["logits"].cpu(), ref["logits"])
    print(f"{what} logits: rel-to-max error {e:.3e}")
    assert e <= TOL, (what, e)
    assert abs(float(got["loss"]) - ref["loss"]) <= TOL * max(abs(ref["loss"]), 1e-5), what
    safe = ref["margin"] > MARGIN
    assert safe.all(), what                                                        # every prediction is compared
    assert np.array_equal(got["preds"].cpu().numpy(), ref["preds"]), what
    assert float(got["correct"]) == ref["correct"], what


def torch_logreg(xs, ys, xq, N, steps, lr, momentum, C, normalize):
    """The same dual iteration in torch fp32 ops (the second witness, and the yardstick of tools/bench_logreg_head.py)."""
    if normalize:
        xs = xs / xs.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        xq = xq / xq.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    B, S, _ = xs.shape
    K = torch.bmm(xs, xs.transpose(1, 2))
    Y = torch.nn.functional.one_hot(ys, N).float()
    wd = 1.0 / (C * S)
    A = torch.zeros(B, S, N, device=xs.device); VA = torch.zeros_like(A)
    b = torch.zeros(B, 1, N, device=xs.device); Vb = torch.zeros_like(b)
    for _ in range(steps):
        R = (torch.softmax(torch.baddbmm(b, K, A), dim=-1) - Y) / S
        VA = momentum * VA + R + wd * A
        Vb = momentum * Vb + R.sum(dim=1, keepdim=True)
        A = A - lr * VA
        b = b - lr * Vb
    return torch.bmm(xq, torch.bmm(xs.transpose(1, 2), A)) + b


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-T{c[1]}-m{c[2]}-{'norm' if c[3] else 'raw'}")
def test_head_step_matches_float64_and_is_reproducible(case, dev, ws):
    from fumi_amd import hip
    (f_s, y_s, f_q, y_q), ref = _ref(case)
    shape, steps, momentum, normalize = case
    N = shape[3]
    xs, ys, xq, yq = _gpu(dev, f_s, y_s, f_q, y_q)
    kw = dict(steps=steps, lr=LR, momentum=momentum, C=C_REG, normalize=normalize, n_way=N)
    out = hip.logreg_head_step(ws, xs, ys, xq, yq, want_logits=True, **kw)
    assert ws.read_status() == 0
    _check(out, ref, f"fused {case}")
    # a second call: the same bits
    again = hip.logreg_head_step(ws, xs, ys, xq, yq, want_logits=True, **kw)
    for k in ("loss", "correct", "preds", "logits"):
        assert torch.equal(again[k], out[k]), k
    # without logits (the binding) and without preds and logits (the C entry): the same loss, count and predictions
    bare = hip.logreg_head_step(ws, xs, ys, xq, yq, want_logits=False, **kw)
    assert bare["logits"] is None
    for k in ("loss", "correct", "preds"):
        assert torch.equal(bare[k], out[k]), k
    from ctypes import c_void_p
    p = lambda t: c_void_p(t.data_ptr())
    loss, correct = torch.full((1,), -1.0, device=dev), torch.full((1,), -1.0, device=dev)
    B, S, Qn, _, Fd = shape
    rc = hip.lib().fumi_hip_logreg_head_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, p(xs), p(ys), p(xq), p(yq), steps, LR,
                                             momentum, C_REG, int(normalize), p(loss), p(correct), None, None)
    assert rc == 0 and torch.equal(loss, out["loss"]) and torch.equal(correct, out["correct"])
    assert ws.read_status() == 0
    # second witness: the same iteration in torch fp32 ops, against the same float64 logits
    z = torch_logreg(xs, ys, xq, N, steps, LR, momentum, C_REG, normalize)
    e = rel_to_max(z.cpu(), ref["logits"])
    print(f"torch fp32 ops {case} logits: rel-to-max error {e:.3e}")
    assert e <= TOL


def test_the_default_form_is_one_of_the_two(dev, ws):
    from fumi_amd import hip
    for case in (CASES[5], CASES[7]):                                              # 20-way 5-shot and 5-way 5-shot at T = 100
        (f_s, y_s, f_q, y_q), ref = _ref(case)
        shape, steps, momentum, normalize = case
        xs, ys, xq, yq = _gpu(dev, f_s, y_s, f_q, y_q)
        kw = dict(steps=steps, lr=LR, momentum=momentum, C=C_REG, normalize=normalize, n_way=shape[3], want_logits=True)
        outs = {}
        for f in ("valu", "mfma", None):
            hip.logreg_set_form(f)
            outs[f] = hip.logreg_head_step(ws, xs, ys, xq, yq, **kw)["logits"]
        assert torch.equal(outs[None], outs["valu"]) or torch.equal(outs[None], outs["mfma"])
        assert hip.lib().fumi_hip_logreg_set_form(2) == -1                         # FUMI_EINVAL, and the form stays
    assert ws.read_status() == 0


# shapes on both sides of the switch between the double-buffered layout (one barrier per step) and the single-buffered one (two): of
# the VALU form (S = 125, N = 64 is its largest LDS request; S >= 126 with N > 32 is single-buffered) and of the MFMA form (S <= 112
# with N > 32 double-buffered); and the three column-tile counts of the MFMA form next to S = 128
@pytest.mark.parametrize("B,S,Qn,N,Fd", [(1, 125, 4, 64, 32), (1, 128, 4, 32, 32), (1, 126, 4, 33, 32), (1, 112, 4, 64, 32),
                                         (1, 113, 4, 33, 32), (2, 128, 4, 16, 32)])
def test_shapes_next_to_the_layout_switch_match_float64(B, S, Qn, N, Fd, dev, ws):
    from fumi_amd import hip
    f_s, y_s, f_q, y_q = case_inputs(B, S, Qn, N, Fd)
    ref = logreg_head_ref(f_s, y_s, f_q, y_q, N, steps=5, lr=LR, momentum=MOMENTUM, C=C_REG)
    xs, ys, xq, yq = _gpu(dev, f_s, y_s, f_q, y_q)
    out = hip.logreg_head_step(ws, xs, ys, xq, yq, steps=5, lr=LR, momentum=MOMENTUM, C=C_REG, want_logits=True, n_way=N)
    assert ws.read_status() == 0
    _check_status_case(out, ref, f"layout switch ({B},{S},{Qn},{N},{Fd})")
    again = hip.logreg_head_step(ws, xs, ys, xq, yq, steps=5, lr=LR, momentum=MOMENTUM, C=C_REG, want_logits=True, n_way=N)
    assert torch.equal(again["logits"], out["logits"]) and torch.equal(again["loss"], out["loss"])


SMALL = CASES[3]                   # (2, 7, 33, 3, 96) at T = 100
KW = dict(steps=SMALL[1], lr=LR, momentum=SMALL[2], C=C_REG, normalize=SMALL[3])


def _small_case():
    assert SMALL[0] == (2, 7, 33, 3, 96) and SMALL[1] == 100
    (f_s, y_s, f_q, y_q), _ = _ref(SMALL)
    return SMALL[0] + (f_s.copy(), y_s.copy(), f_q.copy(), y_q.copy())


def _run(dev, ws, f_s, y_s, f_q, y_q, N):
    from fumi_amd import hip
    xs, ys, xq, yq = _gpu(dev, f_s, y_s, f_q, y_q)
    return hip.logreg_head_step(ws, xs, ys, xq, yq, want_logits=True, n_way=N, **KW)


def _check_status_case(got, ref, what):
    """As _check, for inputs whose margins the CPU test does not cover: predictions compared where the margin allows."""
    e = rel_to_max(got["logits"].cpu(), ref["logits"])
    print(f"{what} logits: rel-to-max error {e:.3e}; loss {float(got['loss']):.6e} against {ref['loss']:.6e}")
    assert e <= TOL, (what, e)
    assert abs(float(got["loss"]) - ref["loss"]) <= TOL * max(abs(ref["loss"]), 1e-5), what
    safe = ref["margin"] > MARGIN
    assert np.array_equal(got["preds"].cpu().numpy()[safe], ref["preds"][safe]), what
    assert abs(float(got["correct"]) - ref["correct"]) <= int((~safe).sum()), what


def test_query_label_out_of_range_sets_the_status_bit_and_drops_the_row(dev, ws):
    from fumi_amd import hip
    B, S, Qn, N, Fd, f_s, y_s, f_q, y_q = _small_case()
    clean = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    assert ws.read_status() == 0
    y_q[1, 20] = N
    ref = logreg_head_ref(f_s, y_s, f_q, y_q, N, **KW)
    assert ref["status"] == ST_LABEL_RANGE
    out = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    assert ws.read_status() == hip.ST_LABEL_RANGE
    assert ws.read_status() == 0                                                  # (reading clears the word)
    assert torch.equal(out["logits"], clean["logits"]) and float(out["loss"]) != float(clean["loss"])
    _check_status_case(out, ref, "query label out of range")


def test_support_label_out_of_range_sets_the_status_bit_and_leaves_the_row_out(dev, ws):
    from fumi_amd import hip
    B, S, Qn, N, Fd, f_s, y_s, f_q, y_q = _small_case()
    clean = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    assert ws.read_status() == 0
    y_s[0, 6] = -1                                                                # (the extra row of class 0: every class keeps support)
    ref = logreg_head_ref(f_s, y_s, f_q, y_q, N, **KW)
    assert ref["status"] == ST_LABEL_RANGE
    out = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    assert ws.read_status() == hip.ST_LABEL_RANGE
    assert ws.read_status() == 0
    _check_status_case(out, ref, "support label out of range")
    assert torch.equal(out["logits"][1], clean["logits"][1])                      # the other episode: the same bits
    assert not torch.equal(out["logits"][0], clean["logits"][0])
    # the episode against a run with that row physically removed
    cut = _run(dev, ws, f_s[:1, :6], y_s[:1, :6], f_q[:1], y_q[:1], N)
    assert ws.read_status() == 0
    e = rel_to_max(out["logits"][0].cpu(), cut["logits"][0].cpu().double())
    print(f"left-out row against the row removed: rel-to-max error {e:.3e}")
    assert e <= TOL


def test_class_without_support_sets_the_status_bit_and_is_fitted_like_any_class(dev, ws):
    from fumi_amd import hip
    B, S, Qn, N, Fd, f_s, y_s, f_q, y_q = _small_case()
    y_s[1][y_s[1] == 2] = 1                                                       # episode 1 has no row of class 2
    ref = logreg_head_ref(f_s, y_s, f_q, y_q, N, **KW)
    assert ref["status"] == ST_CLASS_MISSING
    out = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    assert ws.read_status() == hip.ST_CLASS_MISSING
    assert ws.read_status() == 0
    _check_status_case(out, ref, "class without support")
    assert not bool((out["preds"][1] == 2).any())


def test_a_nan_in_one_episode_leaves_the_other_episode_alone(dev, ws):
    """The fit runs a fixed number of steps whatever the values are: no index and no trip count depends on a float."""
    B, S, Qn, N, Fd, f_s, y_s, f_q, y_q = _small_case()
    clean = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    assert ws.read_status() == 0
    f_s[1, 2, 5] = np.nan
    out = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    assert ws.read_status() == 0
    assert torch.equal(out["logits"][0], clean["logits"][0])
    assert bool(torch.isnan(out["logits"][1]).any())


_OK = dict(steps=3, lr=1.0, momentum=0.9, C=1.0)


# S = 129, N = 1, N = 65, F = 48, Qn = 0, steps = 0, steps = 10001, momentum = 1, C = 0, lr = 0
@pytest.mark.parametrize("B,S,Qn,N,Fd,kw", [(1, 129, 4, 2, 32, {}), (1, 4, 4, 1, 32, {}), (1, 65, 4, 65, 32, {}), (1, 4, 4, 2, 48, {}),
                                            (1, 4, 0, 2, 32, {}), (1, 4, 4, 2, 32, dict(steps=0)), (1, 4, 4, 2, 32, dict(steps=10001)),
                                            (1, 4, 4, 2, 32, dict(momentum=1.0)), (1, 4, 4, 2, 32, dict(C=0.0)),
                                            (1, 4, 4, 2, 32, dict(lr=0.0))])
def test_unsupported_shapes_and_hyper_parameters_are_refused(B, S, Qn, N, Fd, kw, dev, ws):
    from fumi_amd import hip
    xs, xq = torch.zeros(B, S, Fd, device=dev), torch.zeros(B, Qn, Fd, device=dev)
    ys, yq = torch.zeros(B, S, dtype=torch.int64, device=dev), torch.zeros(B, Qn, dtype=torch.int64, device=dev)
    with pytest.raises(hip.FumiHipError, match="fumi_hip_logreg_head_step"):
        hip.logreg_head_step(ws, xs, ys, xq, yq, n_way=N, **{**_OK, **kw})
    assert ws.read_status() == 0


def test_a_null_required_pointer_is_an_invalid_argument(dev, ws):
    from ctypes import c_void_p
    from fumi_amd import hip
    B, S, Qn, N, Fd = 1, 4, 4, 2, 32
    xs, xq = torch.zeros(B, S, Fd, device=dev), torch.zeros(B, Qn, Fd, device=dev)
    ys, yq = torch.zeros(B, S, dtype=torch.int64, device=dev), torch.zeros(B, Qn, dtype=torch.int64, device=dev)
    loss, correct = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    ptrs = [c_void_p(t.data_ptr()) for t in (xs, ys, xq, yq, loss, correct)]
    for missing in range(6):
        a = list(ptrs)
        a[missing] = None
        rc = hip.lib().fumi_hip_logreg_head_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, a[0], a[1], a[2], a[3], 3, 1.0, 0.9, 1.0, 1,
                                                 a[4], a[5], None, None)
        assert rc == -1, missing                                                  # FUMI_EINVAL
    assert ws.read_status() == 0
