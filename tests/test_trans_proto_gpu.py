"""GPU parity of the transductive prototype refinement (fumi_hip_trans_proto_step, csrc/transproto.hip) against the float64 restatement
tests/trans_proto_ref.py (tied to a torch float64 loop and to cos_proto_ref / euclid_proto_ref by tests/test_trans_proto_cpu.py).

The bound is the one every head of this project is held to: logits and loss within 1e-4 of max|z| of the float64 reference.
Predictions are compared on every row whose float64 top-two gap is at least 2e-4 max|z| (a row nearer than that may fall either way
inside the bound); tests/test_trans_proto_cpu.py asserts on the reference alone that at most 2 rows per case and at most 1 % of all
rows are set aside.  ``correct`` must be the count of the kernel's own predictions, which ties it to the reference's on the rows
compared.  Scales: cosine 10, euclid 4; steps 0, 1, 10; the shapes of ridge_head_ref.SHAPES and the two limit shapes.

Measured on one MI355X (profiles/trans_proto/gpu_tests.log), as a fraction of max|z|: logits at most 3.6e-6
over all 54 parity cases (loss 1.6e-7), 2.0e-6 with 8.0 added to every feature; steps = 0 against cos_proto_step / euclid_proto_step
at most 1.3e-6; 8 of 6048 rows set aside."""
import numpy as np
import pytest
import torch

from ridge_head_ref import SHAPES, case_inputs
from trans_proto_ref import (LIMIT_SHAPES, METRICS, SCALES, SHIFT, SHIFTED, ST_CLASS_MISSING, ST_LABEL_RANGE, STEPS, trans_proto_ref)

pytestmark = pytest.mark.gpu
TOL, GAP = 1e-4, 2e-4

_REFS = {}


def _case(shape, metric, steps, shifted=False):
    """(inputs, float64 reference) of a parity case, computed once and shared."""
    key = (shape, metric, steps, shifted)
    if key not in _REFS:
        f_s, y_s, f_q, y_q = case_inputs(*shape)
        if shifted:
            f_s, f_q = f_s + np.float32(SHIFT), f_q + np.float32(SHIFT)
        _REFS[key] = ((f_s, y_s, f_q, y_q), trans_proto_ref(f_s, y_s, f_q, y_q, shape[3], SCALES[metric], metric, steps))
    return _REFS[key]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _gpu(dev, *arrays):
    return [torch.as_tensor(a).to(dev) for a in arrays]


def _step(dev, ws, inputs, n_way, metric, steps):
    from fumi_amd import hip
    xs, ys, xq, yq = _gpu(dev, *inputs)
    scale = torch.tensor([SCALES[metric]], device=dev)
    return hip.trans_proto_step(ws, xs, ys, xq, yq, scale, metric=metric, steps=steps, want_logits=True, n_way=n_way)


def _check(got, ref, y_q, n_way, what):
    zmax = float(np.abs(ref["logits"]).max())
    e_z = float(np.abs(got["logits"].cpu().numpy().astype(np.float64) - ref["logits"]).max()) / zmax
    e_l = abs(float(got["loss"]) - float(ref["loss"])) / zmax
    safe = ref["margin"] >= GAP * zmax
    print(f"{what}: logits {e_z:.3e}, loss {e_l:.3e} of max|z| = {zmax:.4g}; rows set aside {int((~safe).sum())}")
    assert e_z <= TOL and e_l <= TOL, (what, e_z, e_l)
    assert int((~safe).sum()) <= 2, what                                          # (a condition on the inputs)
    preds = got["preds"].cpu().numpy()
    assert np.array_equal(preds[safe], ref["preds"][safe]), what
    ok = (y_q >= 0) & (y_q < n_way)
    assert float(got["correct"]) == float(((preds == y_q) & ok).sum()), what       # the count of its own predictions ...
    assert abs(float(got["correct"]) - ref["correct"]) <= int((~safe).sum()), what  # ... so the reference's on the rows compared
    return e_z


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("shape", SHAPES + LIMIT_SHAPES, ids=str)
def test_step_matches_float64_and_is_reproducible(shape, metric, steps, dev, ws):
    inputs, ref = _case(shape, metric, steps)
    assert ref["status"] == 0
    out = _step(dev, ws, inputs, shape[3], metric, steps)
    assert ws.read_status() == 0
    _check(out, ref, inputs[3], shape[3], f"trans {shape} {metric} steps={steps}")
    again = _step(dev, ws, inputs, shape[3], metric, steps)
    for k in ("loss", "correct", "preds", "logits"):
        assert torch.equal(again[k], out[k]), k


@pytest.mark.parametrize("shape", SHIFTED, ids=str)
def test_euclid_matches_float64_with_an_offset_on_every_feature(shape, dev, ws):
    inputs, ref = _case(shape, "euclid", 10, shifted=True)
    assert ref["status"] == 0 and ref["margin"].min() >= GAP * np.abs(ref["logits"]).max()
    out = _step(dev, ws, inputs, shape[3], "euclid", 10)
    assert ws.read_status() == 0
    _check(out, ref, inputs[3], shape[3], f"trans {shape} + {SHIFT} euclid steps=10")
    assert np.array_equal(out["preds"].cpu().numpy(), ref["preds"]) and float(out["correct"]) == ref["correct"]


@pytest.mark.parametrize("shape", [(2, 7, 33, 3, 96), (2, 100, 130, 20, 640), (1, 128, 18, 64, 64)], ids=str)
def test_zero_steps_agree_with_the_inductive_heads(shape, dev, ws):
    """steps = 0 against the forward forms of cos_proto_step and euclid_proto_step on the same inputs: each within the bound of the
    float64 reference both are held to; their difference is recorded."""
    from fumi_amd import hip
    for metric, head in (("cosine", hip.cos_proto_step), ("euclid", hip.euclid_proto_step)):
        inputs, ref = _case(shape, metric, 0)
        out = _step(dev, ws, inputs, shape[3], metric, 0)
        xs, ys, xq, yq = _gpu(dev, *inputs)
        ind = head(ws, xs, ys, xq, yq, torch.tensor([SCALES[metric]], device=dev), need_grad=False, want_logits=True, n_way=shape[3])
        assert ws.read_status() == 0
        zmax = float(np.abs(ref["logits"]).max())
        e_t = float(np.abs(out["logits"].cpu().numpy() - ref["logits"]).max()) / zmax
        e_i = float(np.abs(ind["logits"].cpu().numpy() - ref["logits"]).max()) / zmax
        diff = float((out["logits"] - ind["logits"]).abs().max()) / zmax
        print(f"steps=0 {shape} {metric}: transductive {e_t:.3e}, inductive {e_i:.3e} of the reference; between them {diff:.3e} of max|z|")
        assert e_t <= TOL and e_i <= TOL
        safe = ref["margin"] >= GAP * zmax
        assert torch.equal(out["preds"].cpu()[torch.as_tensor(safe)], ind["preds"].cpu()[torch.as_tensor(safe)])


SMALL = (2, 7, 33, 3, 96)


def _small_case():
    return tuple(a.copy() for a in case_inputs(*SMALL))


@pytest.mark.parametrize("metric", METRICS)
def test_query_label_out_of_range_sets_the_bit_drops_the_row_and_still_refines(metric, dev, ws):
    from fumi_amd import hip
    f_s, y_s, f_q, y_q = _small_case()
    y_q[1, 20] = SMALL[3]
    ref = trans_proto_ref(f_s, y_s, f_q, y_q, SMALL[3], SCALES[metric], metric, 3)
    assert ref["status"] == ST_LABEL_RANGE
    out = _step(dev, ws, (f_s, y_s, f_q, y_q), SMALL[3], metric, 3)
    assert ws.read_status() == hip.ST_LABEL_RANGE
    assert ws.read_status() == 0                                                  # (reading clears the word)
    _check(out, ref, y_q, SMALL[3], f"query label out of range, {metric}")
    # the refinement reads no query label: the logits are those of the episode with the label in range, bit for bit
    y_q[1, 20] = 0
    plain = _step(dev, ws, (f_s, y_s, f_q, y_q), SMALL[3], metric, 3)
    assert ws.read_status() == 0
    assert torch.equal(plain["logits"], out["logits"]) and torch.equal(plain["preds"], out["preds"])


@pytest.mark.parametrize("metric", METRICS)
def test_support_label_out_of_range_gives_the_episode_without_that_row(metric, dev, ws):
    from fumi_amd import hip
    f_s, y_s, f_q, y_q = _small_case()
    y_s[0, 6], y_s[1, 6] = -1, SMALL[3] + 2                                       # (the extra row of class 0: every class keeps support)
    ref = trans_proto_ref(f_s, y_s, f_q, y_q, SMALL[3], SCALES[metric], metric, 3)
    sub = trans_proto_ref(f_s[:, :6], y_s[:, :6], f_q, y_q, SMALL[3], SCALES[metric], metric, 3)
    assert ref["status"] == ST_LABEL_RANGE and np.abs(ref["logits"] - sub["logits"]).max() <= 1e-12
    out = _step(dev, ws, (f_s, y_s, f_q, y_q), SMALL[3], metric, 3)
    assert ws.read_status() == hip.ST_LABEL_RANGE
    assert ws.read_status() == 0
    _check(out, ref, y_q, SMALL[3], f"support label out of range, {metric}")


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("steps", (0, 3))
def test_class_without_support_sets_the_bit_and_is_refined(metric, steps, dev, ws):
    from fumi_amd import hip
    f_s, y_s, f_q, y_q = _small_case()
    y_s[1][y_s[1] == 2] = 1                                                       # episode 1 has no row of class 2
    ref = trans_proto_ref(f_s, y_s, f_q, y_q, SMALL[3], SCALES[metric], metric, steps)
    assert ref["status"] == ST_CLASS_MISSING
    if steps:
        assert np.abs(ref["protos"][1, 2]).max() > 0                              # (the class has moved off the zero prototype)
    out = _step(dev, ws, (f_s, y_s, f_q, y_q), SMALL[3], metric, steps)
    assert ws.read_status() == hip.ST_CLASS_MISSING
    assert ws.read_status() == 0
    _check(out, ref, y_q, SMALL[3], f"class without support, {metric}, steps={steps}")


# on either side of every limit: B = 0, S = 0, Qn = 0, S + Qn = 513, Qn * N = 8256, B * Qn = 65537, N = 1, N = 65, F = 48 (no multiple of
# 32), F = 0, F = 2080; then steps = -1 and 101 at an accepted shape
REFUSED = [(0, 4, 4, 2, 32, 1), (1, 0, 4, 2, 32, 1), (1, 4, 0, 2, 32, 1), (1, 256, 257, 2, 32, 1), (1, 4, 129, 64, 32, 1),
           (65537, 1, 1, 2, 32, 1), (1, 4, 4, 1, 32, 1), (1, 65, 4, 65, 32, 1), (1, 4, 4, 2, 48, 1), (1, 4, 4, 2, 0, 1), (1, 4, 4, 2, 2080, 1),
           (1, 4, 4, 2, 32, -1), (1, 4, 4, 2, 32, 101)]


@pytest.mark.parametrize("B,S,Qn,N,Fd,steps", REFUSED)
def test_unsupported_shapes_and_step_counts_are_refused_before_any_launch(B, S, Qn, N, Fd, steps, dev, ws):
    from ctypes import c_void_p
    from fumi_amd import hip
    xs, xq = torch.zeros(B, S, Fd, device=dev), torch.zeros(B, Qn, Fd, device=dev)
    ys, yq = torch.zeros(B, S, dtype=torch.int64, device=dev), torch.zeros(B, Qn, dtype=torch.int64, device=dev)
    scale = torch.tensor([1.0], device=dev)
    for metric in METRICS:
        with pytest.raises(hip.FumiHipError, match="fumi_hip_trans_proto_step"):
            hip.trans_proto_step(ws, xs, ys, xq, yq, scale, metric=metric, steps=steps, n_way=N)
    # the documented code, with every pointer given; the outputs are not touched
    loss, correct = torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    preds = torch.full((max(B, 1), max(Qn, 1)), 7, dtype=torch.int64, device=dev)
    logits = torch.full((max(B, 1), max(Qn, 1), N), 7.0, device=dev)
    one = torch.zeros(1, device=dev)
    p = lambda t: c_void_p(t.data_ptr() if t.numel() else one.data_ptr())
    for metric in (0, 1):
        rc = hip.lib().fumi_hip_trans_proto_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, p(xs), p(ys), p(xq), p(yq), p(scale), metric,
                                                 steps, p(loss), p(correct), p(preds), p(logits))
        assert rc == -4                                                           # FUMI_ENOTSUP
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and float(correct) == 7.0 and int(preds.min()) == 7 and float(logits.min()) == 7.0
    assert ws.read_status() == 0


def test_a_missing_pointer_or_an_unknown_metric_is_an_invalid_argument(dev, ws):
    from ctypes import c_void_p
    from fumi_amd import hip
    B, S, Qn, N, Fd = 1, 4, 4, 2, 32
    xs, xq = torch.zeros(B, S, Fd, device=dev), torch.zeros(B, Qn, Fd, device=dev)
    ys, yq = (torch.arange(S, device=dev) % N).repeat(B, 1), torch.zeros(B, Qn, dtype=torch.int64, device=dev)      # both classes have support
    scale, loss, correct = torch.tensor([1.0], device=dev), torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    preds, logits = torch.full((B, Qn), 7, dtype=torch.int64, device=dev), torch.full((B, Qn, N), 7.0, device=dev)
    p = lambda t: c_void_p(t.data_ptr()) if t is not None else None
    call = lambda req, metric, opt: hip.lib().fumi_hip_trans_proto_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, *(p(t) for t in req[:5]),
                                                                        metric, 2, p(req[5]), p(req[6]), *(p(t) for t in opt))
    required = [xs, ys, xq, yq, scale, loss, correct]
    for i in range(len(required)):                                                # feats_s, y_s, feats_q, y_q, scale, loss, correct
        req = list(required); req[i] = None
        assert call(req, 0, (preds, logits)) == -1 and call(req, 1, (None, None)) == -1, i          # FUMI_EINVAL
    for metric in (-1, 2):
        assert call(required, metric, (preds, logits)) == -1
    assert hip.lib().fumi_hip_trans_proto_step(None, hip._stream(dev), B, S, Qn, N, Fd, *(p(t) for t in required[:5]), 0, 2, p(loss),
                                               p(correct), None, None) == -1
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and float(correct) == 7.0 and int(preds.min()) == 7 and float(logits.min()) == 7.0   # nothing was launched
    with pytest.raises(hip.FumiHipError, match="metric"):
        hip.trans_proto_step(ws, xs, ys, xq, yq, scale, metric="euclidean", steps=2, n_way=N)
    # preds and logits are optional
    assert call(required, 0, (None, None)) == 0 and call(required, 1, (preds, logits)) == 0
    torch.cuda.synchronize()
    assert float(loss) != 7.0 and int(preds.max()) < N
    assert ws.read_status() == 0
