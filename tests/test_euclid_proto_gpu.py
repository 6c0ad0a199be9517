"""GPU parity of the fused prototypical-network head (fumi_hip_euclid_proto_step, csrc/euclidproto.hip) against the float64 restatement
tests/euclid_proto_ref.py (tied to torch.autograd at 1e-12 by tests/test_euclid_proto_cpu.py).

Tolerances are the ones the fp32 paths are held to against float64 (tests/test_hip_parity.py:18-20, as tests/test_cos_proto_gpu.py uses
them): 1e-4 of the largest magnitude of the compared tensor, 1e-4 relative on the loss, predictions compared where the float64 top-two
logit margin exceeds 1e-5 -- tests/test_euclid_proto_cpu.py asserts that this sets aside no query row of these inputs.  dalpha is held
to 1e-4 of dalpha_abs = sum |dz (d2 - min_n d2)|, the magnitude its round-off scales with (sum_n dz = 0, so the part of d2 common to a
row does not reach it).  alpha = 1 / F, grad_scale = 0.25.  Two of the shapes run a second time with 8.0 added to every feature, at the
same tolerances: the distances do not change, an uncentred |f|^2 - 2 f.c + |c|^2 would lose them.  The second witness is proto_reduce
plus the torch fp32 expression of Pretrain.few_shot on the GPU, held to the same float64 logits.

Measured on one MI355X (profiles/euclid_proto/gpu_tests.log), each in the unit of its own bound of 1e-4: at most
3.4e-7 over the six plain shapes, at most 1.5e-6 (dfeats_s) with 8.0 added to every feature."""
import numpy as np
import pytest
import torch

from euclid_proto_ref import (GRAD_SCALE, SHAPES, SHIFT, SHIFTED, ST_CLASS_MISSING, ST_LABEL_RANGE, case_inputs, euclid_proto_ref)
from helpers import rel_to_max

pytestmark = pytest.mark.gpu
TOL, MARGIN = 1e-4, 1e-5          # tests/test_hip_parity.py:18-20

_REFS = {}


def _case(shape, shifted=False):
    """(inputs, float64 reference) of a parity shape, computed once and shared."""
    key = (shape, shifted)
    if key not in _REFS:
        f_s, y_s, f_q, y_q = case_inputs(*shape)
        if shifted:
            f_s, f_q = f_s + np.float32(SHIFT), f_q + np.float32(SHIFT)
        _REFS[key] = ((f_s, y_s, f_q, y_q), euclid_proto_ref(f_s, y_s, f_q, y_q, 1.0 / shape[4], shape[3], GRAD_SCALE))
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


def _check(got, ref, what, grads=True):
    e = abs(float(got["loss"]) - ref["loss"]) / max(abs(ref["loss"]), 1e-5)
    print(f"{what} loss: relative error {e:.3e}")
    assert e <= TOL, what
    safe = ref["margin"] > MARGIN
    preds = got["preds"].cpu().numpy()
    assert np.array_equal(preds[safe], ref["preds"][safe]), what
    assert abs(float(got["correct"]) - ref["correct"]) <= int((~safe).sum()), what
    keys = ("logits",) + (("dfeats_s", "dfeats_q") if grads else ())
    for k in keys:
        e = rel_to_max(got[k].cpu(), ref[k])
        print(f"{what} {k}: rel-to-max error {e:.3e}")
        assert e <= TOL, (what, k, e)
    if grads:
        e = abs(float(got["dalpha"]) - ref["dalpha"]) / ref["dalpha_abs"]
        print(f"{what} dalpha: {float(got['dalpha']):.6e} against {ref['dalpha']:.6e}, error {e:.3e} of dalpha_abs {ref['dalpha_abs']:.3e}")
        assert e <= TOL, (what, e)


def _step(dev, ws, inputs, shape, need_grad=True):
    from fumi_amd import hip
    xs, ys, xq, yq = _gpu(dev, *inputs)
    alpha = torch.tensor([1.0 / shape[4]], device=dev)
    return hip.euclid_proto_step(ws, xs, ys, xq, yq, alpha, need_grad=need_grad, grad_scale=GRAD_SCALE, want_logits=True, n_way=shape[3])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_head_step_matches_float64_and_is_reproducible(shape, dev, ws):
    from fumi_amd import hip
    B, S, Qn, N, Fd = shape
    inputs, ref = _case(shape)
    assert ref["status"] == 0 and ref["margin"].min() > MARGIN                    # every prediction is compared, here: equal
    out = _step(dev, ws, inputs, shape)
    assert ws.read_status() == 0
    _check(out, ref, f"fused {shape}")
    assert np.array_equal(out["preds"].cpu().numpy(), ref["preds"]) and float(out["correct"]) == ref["correct"]
    # the forward form and a second call: the same bits
    fwd = _step(dev, ws, inputs, shape, need_grad=False)
    assert fwd["dfeats_s"] is None and fwd["dfeats_q"] is None and fwd["dalpha"] is None
    for k in ("loss", "correct", "preds", "logits"):
        assert torch.equal(fwd[k], out[k]), k
    again = _step(dev, ws, inputs, shape)
    for k in ("loss", "correct", "preds", "logits", "dfeats_s", "dfeats_q", "dalpha"):
        assert torch.equal(again[k], out[k]), k
    # second witness: proto_reduce and the torch fp32 expression of Pretrain.few_shot on the GPU, against the same float64 logits
    xs, ys, xq, yq = _gpu(dev, *inputs)
    protos = hip.proto_reduce(ws, xs, ys, N)
    d2 = ((xq[:, :, None, :] - protos[:, None, :, :]) ** 2).sum(-1)
    assert ws.read_status() == 0
    e = rel_to_max((-d2 / Fd).cpu(), ref["logits"])
    print(f"proto_reduce + torch {shape} logits: rel-to-max error {e:.3e}")
    assert e <= TOL


@pytest.mark.parametrize("shape", SHIFTED, ids=str)
def test_head_step_matches_float64_with_an_offset_on_every_feature(shape, dev, ws):
    inputs, ref = _case(shape, shifted=True)
    plain = _case(shape)[1]
    assert rel_to_max(ref["logits"], plain["logits"]) < 1e-5                       # (fp32 inputs plus 8.0 round: not 1e-10 as in float64)
    assert ref["status"] == 0 and ref["margin"].min() > MARGIN
    out = _step(dev, ws, inputs, shape)
    assert ws.read_status() == 0
    _check(out, ref, f"fused {shape} + {SHIFT}")
    assert np.array_equal(out["preds"].cpu().numpy(), ref["preds"]) and float(out["correct"]) == ref["correct"]
    fwd = _step(dev, ws, inputs, shape, need_grad=False)
    for k in ("loss", "correct", "preds", "logits"):
        assert torch.equal(fwd[k], out[k]), k


SMALL = (2, 7, 33, 3, 96)


def _small_case():
    return tuple(a.copy() for a in case_inputs(*SMALL))


def test_query_label_out_of_range_sets_the_status_bit_and_drops_the_row(dev, ws):
    from fumi_amd import hip
    f_s, y_s, f_q, y_q = _small_case()
    y_q[1, 20] = SMALL[3]
    ref = euclid_proto_ref(f_s, y_s, f_q, y_q, 1.0 / SMALL[4], SMALL[3], GRAD_SCALE)
    assert ref["status"] == ST_LABEL_RANGE and not ref["dfeats_q"][1, 20].any()
    out = _step(dev, ws, (f_s, y_s, f_q, y_q), SMALL)
    assert ws.read_status() == hip.ST_LABEL_RANGE
    assert ws.read_status() == 0                                                  # (reading clears the word)
    assert float(out["dfeats_q"][1, 20].abs().max()) == 0.0
    _check(out, ref, "query label out of range")


def test_support_label_out_of_range_gives_the_episode_without_that_row(dev, ws):
    from fumi_amd import hip
    f_s, y_s, f_q, y_q = _small_case()
    y_s[0, 6], y_s[1, 6] = -1, SMALL[3] + 2                                       # (the extra row of class 0: every class keeps support)
    ref = euclid_proto_ref(f_s, y_s, f_q, y_q, 1.0 / SMALL[4], SMALL[3], GRAD_SCALE)
    assert ref["status"] == ST_LABEL_RANGE and not ref["dfeats_s"][:, 6].any()
    out = _step(dev, ws, (f_s, y_s, f_q, y_q), SMALL)
    assert ws.read_status() == hip.ST_LABEL_RANGE
    assert ws.read_status() == 0
    assert float(out["dfeats_s"][:, 6].abs().max()) == 0.0
    _check(out, ref, "support label out of range")
    # the same sums in the same order as the episode of the six other rows: the same bits
    sub = _step(dev, ws, (f_s[:, :6], y_s[:, :6], f_q, y_q), (2, 6, 33, 3, 96))
    assert ws.read_status() == 0
    for k in ("loss", "correct", "preds", "logits", "dfeats_q", "dalpha"):
        assert torch.equal(sub[k], out[k]), k
    assert torch.equal(sub["dfeats_s"], out["dfeats_s"][:, :6])


def test_class_without_support_sets_the_status_bit_and_has_the_logits_of_a_zero_prototype(dev, ws):
    from fumi_amd import hip
    f_s, y_s, f_q, y_q = _small_case()
    y_s[1][y_s[1] == 2] = 1                                                       # episode 1 has no row of class 2
    ref = euclid_proto_ref(f_s, y_s, f_q, y_q, 1.0 / SMALL[4], SMALL[3], GRAD_SCALE)
    assert ref["status"] == ST_CLASS_MISSING
    out = _step(dev, ws, (f_s, y_s, f_q, y_q), SMALL)
    assert ws.read_status() == hip.ST_CLASS_MISSING
    assert ws.read_status() == 0
    want = -(f_q[1].astype(np.float64) ** 2).sum(-1) / SMALL[4]                    # -alpha |f_q|^2
    assert np.abs(ref["logits"][1, :, 2] - want).max() <= 1e-12
    e = float(np.abs(out["logits"][1, :, 2].cpu().numpy() - want).max() / np.abs(ref["logits"]).max())
    print(f"class without support: logits against -alpha |f_q|^2, rel-to-max error {e:.3e}")
    assert e <= TOL
    _check(out, ref, "class without support")


def test_the_shapes_at_the_limits_run(dev, ws):
    """S = 1024 and B * Qn = 65536 with N = 2, F = 32 (N = 64 and F = 2048 are among the parity shapes)."""
    shape = (2, 1024, 32768, 2, 32)
    inputs, ref = _case(shape)
    out = _step(dev, ws, inputs, shape)
    assert ws.read_status() == 0
    _check(out, ref, f"fused {shape}")


# on either side of every limit: F = 48 (no multiple of 32), F = 0, F = 2080, N = 1, N = 65, S = 0, S = 1025, Qn = 0, B * Qn = 65537, B = 0
REFUSED = [(1, 4, 4, 2, 48), (1, 4, 4, 2, 0), (1, 4, 4, 2, 2080), (1, 4, 4, 1, 32), (1, 65, 4, 65, 32), (1, 0, 4, 2, 32), (1, 1025, 4, 2, 32),
           (1, 4, 0, 2, 32), (1, 4, 65537, 2, 32), (0, 4, 4, 2, 32)]


@pytest.mark.parametrize("B,S,Qn,N,Fd", REFUSED)
def test_unsupported_shapes_are_refused_before_any_launch(B, S, Qn, N, Fd, dev, ws):
    from ctypes import c_void_p
    from fumi_amd import hip
    xs, xq = torch.zeros(B, S, Fd, device=dev), torch.zeros(B, Qn, Fd, device=dev)
    ys, yq = torch.zeros(B, S, dtype=torch.int64, device=dev), torch.zeros(B, Qn, dtype=torch.int64, device=dev)
    alpha = torch.tensor([1.0], device=dev)
    for need_grad in (False, True):
        with pytest.raises(hip.FumiHipError, match="fumi_hip_euclid_proto_step"):
            hip.euclid_proto_step(ws, xs, ys, xq, yq, alpha, need_grad=need_grad, n_way=N)
    # the documented code, with every pointer given; the outputs are not touched
    loss, correct = torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    dfs, dfq, da = torch.ones(max(B, 1), max(S, 1), max(Fd, 1), device=dev), torch.ones(max(B, 1), max(Qn, 1), max(Fd, 1), device=dev), \
        torch.full((1,), 7.0, device=dev)
    one = torch.zeros(1, device=dev)
    p = lambda t: c_void_p(t.data_ptr() if t.numel() else one.data_ptr())
    for grads in ((None, None, None), (p(dfs), p(dfq), p(da))):
        rc = hip.lib().fumi_hip_euclid_proto_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, p(xs), p(ys), p(xq), p(yq), p(alpha), 1.0,
                                                  p(loss), p(correct), None, None, *grads)
        assert rc == -4                                                           # FUMI_ENOTSUP
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and float(correct) == 7.0 and float(da) == 7.0 and float(dfs.min()) == 1.0 and float(dfq.min()) == 1.0
    assert ws.read_status() == 0


def test_a_missing_pointer_or_part_of_the_gradient_pointers_is_an_invalid_argument(dev, ws):
    from ctypes import c_void_p
    from fumi_amd import hip
    B, S, Qn, N, Fd = 1, 4, 4, 2, 32
    xs, xq = torch.zeros(B, S, Fd, device=dev), torch.zeros(B, Qn, Fd, device=dev)
    ys, yq = (torch.arange(S, device=dev) % N).repeat(B, 1), torch.zeros(B, Qn, dtype=torch.int64, device=dev)      # both classes have support
    alpha, loss, correct = torch.tensor([1.0], device=dev), torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    dfs, dfq, da = torch.zeros_like(xs), torch.zeros_like(xq), torch.zeros(1, device=dev)
    p = lambda t: c_void_p(t.data_ptr()) if t is not None else None
    call = lambda req, grads: hip.lib().fumi_hip_euclid_proto_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, *(p(t) for t in req[:5]),
                                                                   1.0, p(req[5]), p(req[6]), None, None, *(p(g) for g in grads))
    required = [xs, ys, xq, yq, alpha, loss, correct]
    for grads in ((dfs, None, None), (None, dfq, None), (None, None, da), (dfs, dfq, None), (dfs, None, da), (None, dfq, da)):
        assert call(required, grads) == -1, grads                                 # FUMI_EINVAL
    for i in range(len(required)):                                                # feats_s, y_s, feats_q, y_q, alpha, loss, correct
        req = list(required); req[i] = None
        assert call(req, (None, None, None)) == -1, i
        assert call(req, (dfs, dfq, da)) == -1, i
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and float(correct) == 7.0                           # nothing was launched
    assert call(required, (dfs, dfq, da)) == 0 and call(required, (None, None, None)) == 0
    assert ws.read_status() == 0
