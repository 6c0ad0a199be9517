"""GPU parity of the fused cosine nearest-centroid head (fumi_hip_cos_proto_step, csrc/cosproto.hip) against the float64 restatement
tests/cos_proto_ref.py (tied to torch.autograd at 1e-12 by tests/test_cos_proto_cpu.py).

Tolerances are the ones the fp32 paths are held to against float64 (tests/test_hip_parity.py:18-20, as tests/test_cls_head_gpu.py uses
them): 1e-4 of the largest magnitude of the compared tensor, 1e-4 relative on loss and dtau, predictions compared where the float64
top-two logit margin exceeds 1e-5 -- and tests/test_cos_proto_cpu.py asserts that this sets aside no query row of these inputs.  The
second witness is proto_reduce plus torch fp32 ops on the GPU, held to the same float64 logits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cos_proto_ref import ST_CLASS_MISSING, ST_LABEL_RANGE, case_inputs, cos_proto_ref
from helpers import rel_to_max

pytestmark = pytest.mark.gpu
TOL, MARGIN = 1e-4, 1e-5          # tests/test_hip_parity.py:18-20
GRAD_SCALE, TAU = 0.25, 10.0

# (B, S, Qn, N, F): the smallest of everything; rows, classes and features off every tile edge with unequal counts; 20-way at the
# ResNet-12 width, more than eight row tiles plus a tail of two; the Conv4 width, a short last feature block; the class limit; the
# feature limit
SHAPES = [(1, 2, 1, 2, 32), (2, 7, 33, 3, 96), (2, 100, 130, 20, 640), (1, 25, 17, 5, 1600), (1, 64, 18, 64, 64), (3, 10, 16, 5, 2048)]


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
    assert abs(float(got["loss"]) - ref["loss"]) <= TOL * max(abs(ref["loss"]), 1e-5), what
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
        e = abs(float(got["dtau"]) - ref["dtau"])
        print(f"{what} dtau: {float(got['dtau']):.6e} against {ref['dtau']:.6e}")
        assert e <= TOL * max(abs(ref["dtau"]), 1e-5), (what, e)


@pytest.mark.parametrize("B,S,Qn,N,Fd", SHAPES)
def test_head_step_matches_float64_and_is_reproducible(B, S, Qn, N, Fd, dev, ws):
    from fumi_amd import hip
    f_s, y_s, f_q, y_q = case_inputs(B, S, Qn, N, Fd)
    ref = cos_proto_ref(f_s, y_s, f_q, y_q, TAU, N, GRAD_SCALE)
    assert ref["margin"].min() > MARGIN                                           # every prediction is compared
    xs, ys, xq, yq = _gpu(dev, f_s, y_s, f_q, y_q)
    tau = torch.tensor([TAU], device=dev)
    out = hip.cos_proto_step(ws, xs, ys, xq, yq, tau, need_grad=True, grad_scale=GRAD_SCALE, want_logits=True, n_way=N)
    assert ws.read_status() == 0
    _check(out, ref, f"fused ({B},{S},{Qn},{N},{Fd})")
    # the forward form and a second call: the same bits
    fwd = hip.cos_proto_step(ws, xs, ys, xq, yq, tau, need_grad=False, want_logits=True, n_way=N)
    assert fwd["dfeats_s"] is None and fwd["dfeats_q"] is None and fwd["dtau"] is None
    for k in ("loss", "correct", "preds", "logits"):
        assert torch.equal(fwd[k], out[k]), k
    again = hip.cos_proto_step(ws, xs, ys, xq, yq, tau, need_grad=True, grad_scale=GRAD_SCALE, want_logits=True, n_way=N)
    for k in ("loss", "correct", "preds", "logits", "dfeats_s", "dfeats_q", "dtau"):
        assert torch.equal(again[k], out[k]), k
    # second witness: proto_reduce and torch fp32 ops on the GPU, against the same float64 logits
    protos = hip.proto_reduce(ws, xs, ys, N)
    z = TAU * torch.bmm(F.normalize(xq, dim=-1), F.normalize(protos, dim=-1).transpose(1, 2))
    assert ws.read_status() == 0
    e = rel_to_max(z.cpu(), ref["logits"])
    print(f"proto_reduce + torch ({B},{S},{Qn},{N},{Fd}) logits: rel-to-max error {e:.3e}")
    assert e <= TOL


def _small_case():
    B, S, Qn, N, Fd = 2, 7, 33, 3, 96
    return (B, S, Qn, N, Fd) + tuple(case_inputs(B, S, Qn, N, Fd))


def _run(dev, ws, f_s, y_s, f_q, y_q, N):
    from fumi_amd import hip
    xs, ys, xq, yq = _gpu(dev, f_s, y_s, f_q, y_q)
    return hip.cos_proto_step(ws, xs, ys, xq, yq, torch.tensor([TAU], device=dev), need_grad=True, grad_scale=GRAD_SCALE,
                              want_logits=True, n_way=N)


def test_query_label_out_of_range_sets_the_status_bit_and_drops_the_row(dev, ws):
    from fumi_amd import hip
    B, S, Qn, N, Fd, f_s, y_s, f_q, y_q = _small_case()
    y_q[1, 20] = N
    ref = cos_proto_ref(f_s, y_s, f_q, y_q, TAU, N, GRAD_SCALE)
    assert ref["status"] == ST_LABEL_RANGE and not ref["dfeats_q"][1, 20].any()
    out = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    assert ws.read_status() == hip.ST_LABEL_RANGE
    assert ws.read_status() == 0                                                  # (reading clears the word)
    assert float(out["dfeats_q"][1, 20].abs().max()) == 0.0
    _check(out, ref, "query label out of range")


def test_support_label_out_of_range_sets_the_status_bit_and_leaves_the_row_out(dev, ws):
    from fumi_amd import hip
    B, S, Qn, N, Fd, f_s, y_s, f_q, y_q = _small_case()
    y_s[0, 6] = -1                                                                # (the extra row of class 0: every class keeps support)
    ref = cos_proto_ref(f_s, y_s, f_q, y_q, TAU, N, GRAD_SCALE)
    assert ref["status"] == ST_LABEL_RANGE and not ref["dfeats_s"][0, 6].any()
    out = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    assert ws.read_status() == hip.ST_LABEL_RANGE
    assert ws.read_status() == 0
    assert float(out["dfeats_s"][0, 6].abs().max()) == 0.0
    _check(out, ref, "support label out of range")


def test_class_without_support_sets_the_status_bit_and_has_zero_logits(dev, ws):
    from fumi_amd import hip
    B, S, Qn, N, Fd, f_s, y_s, f_q, y_q = _small_case()
    y_s[1][y_s[1] == 2] = 1                                                       # episode 1 has no row of class 2
    ref = cos_proto_ref(f_s, y_s, f_q, y_q, TAU, N, GRAD_SCALE)
    assert ref["status"] == ST_CLASS_MISSING
    out = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    assert ws.read_status() == hip.ST_CLASS_MISSING
    assert ws.read_status() == 0
    assert float(out["logits"][1, :, 2].abs().max()) == 0.0
    _check(out, ref, "class without support")


# F = 48, N = 65, N = 1, S = 1025, Qn = 0
@pytest.mark.parametrize("B,S,Qn,N,Fd", [(1, 4, 4, 2, 48), (1, 65, 4, 65, 32), (1, 4, 4, 1, 32), (1, 1025, 4, 2, 32), (1, 4, 0, 2, 32)])
def test_unsupported_shapes_are_refused(B, S, Qn, N, Fd, dev, ws):
    from fumi_amd import hip
    xs, xq = torch.zeros(B, S, Fd, device=dev), torch.zeros(B, Qn, Fd, device=dev)
    ys, yq = torch.zeros(B, S, dtype=torch.int64, device=dev), torch.zeros(B, Qn, dtype=torch.int64, device=dev)
    tau = torch.tensor([TAU], device=dev)
    with pytest.raises(hip.FumiHipError, match="fumi_hip_cos_proto_step"):
        hip.cos_proto_step(ws, xs, ys, xq, yq, tau, need_grad=False, n_way=N)
    with pytest.raises(hip.FumiHipError, match="fumi_hip_cos_proto_step"):
        hip.cos_proto_step(ws, xs, ys, xq, yq, tau, need_grad=True, n_way=N)
    assert ws.read_status() == 0


def test_part_of_the_gradient_pointers_is_an_invalid_argument(dev, ws):
    from ctypes import c_void_p
    from fumi_amd import hip
    B, S, Qn, N, Fd = 1, 4, 4, 2, 32
    xs, xq = torch.zeros(B, S, Fd, device=dev), torch.zeros(B, Qn, Fd, device=dev)
    ys, yq = torch.zeros(B, S, dtype=torch.int64, device=dev), torch.zeros(B, Qn, dtype=torch.int64, device=dev)
    tau, loss, correct = torch.tensor([TAU], device=dev), torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    dfs, dfq, dtau = torch.zeros_like(xs), torch.zeros_like(xq), torch.zeros(1, device=dev)
    p = lambda t: c_void_p(t.data_ptr()) if t is not None else None
    for grads in ((dfs, None, None), (None, dfq, None), (dfs, dfq, None), (None, dfq, dtau)):
        rc = hip.lib().fumi_hip_cos_proto_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, p(xs), p(ys), p(xq), p(yq), p(tau), 1.0,
                                               p(loss), p(correct), None, None, *(p(g) for g in grads))
        assert rc == -1, grads                                                    # FUMI_EINVAL
    rc = hip.lib().fumi_hip_cos_proto_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, p(xs), p(ys), p(xq), p(yq), None, 1.0,
                                           p(loss), p(correct), None, None, None, None, None)
    assert rc == -1                                                               # tau is required
    assert ws.read_status() == 0
