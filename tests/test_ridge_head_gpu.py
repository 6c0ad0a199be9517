"""GPU parity of the fused ridge-regression head (fumi_hip_ridge_head_step, csrc/ridgehead.hip) against the float64 restatement
tests/ridge_head_ref.py (tied to torch.autograd at 1e-10 by tests/test_ridge_head_cpu.py).

Tolerances are the ones the fp32 paths are held to against float64 (tests/test_hip_parity.py:18-20, as tests/test_cos_proto_gpu.py uses
them): 1e-4 of the largest magnitude of the compared tensor, 1e-4 relative on the loss and both entries of dparams, predictions
compared where the float64 top-two logit margin exceeds 1e-5 -- and tests/test_ridge_head_cpu.py asserts that this sets aside no query
row of these inputs and that their Gram matrices have a condition number of at most 10 (a plain fp32 numpy evaluation of the same
formulas is within 9e-7).  The second witness is torch fp32 cholesky_solve on the GPU, held to the same float64 logits."""
import numpy as np
import pytest
import torch

from helpers import rel_to_max
from ridge_head_ref import (ALPHA, GRAD_SCALE, RHO, SHAPES, ST_CLASS_MISSING, ST_LABEL_RANGE, ST_NOT_POSDEF, case_inputs,
                            ridge_head_ref)

pytestmark = pytest.mark.gpu
TOL, MARGIN = 1e-4, 1e-5          # tests/test_hip_parity.py:18-20
_REFS = {}


def _ref(shape):
    """The inputs and the float64 result of one row of the shape table, computed once and left unchanged."""
    if shape not in _REFS:
        N = shape[3]
        inp = case_inputs(*shape)
        _REFS[shape] = (inp, ridge_head_ref(*inp, (RHO, ALPHA), N, GRAD_SCALE))
    return _REFS[shape]


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


def _params(dev):
    return torch.tensor([RHO, ALPHA], device=dev, dtype=torch.float32)


def _check(got, ref, what, grads=True):
    print(f"{what} loss: {float(got['loss']):.6e} against {ref['loss']:.6e}")
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
        dp = got["dparams"].cpu().numpy().astype(np.float64)
        for i, name in enumerate(("drho", "dalpha")):
            print(f"{what} {name}: {dp[i]:.6e} against {ref['dparams'][i]:.6e}")
            assert abs(dp[i] - ref["dparams"][i]) <= TOL * max(abs(ref["dparams"][i]), 1e-5), (what, name)


@pytest.mark.parametrize("B,S,Qn,N,Fd", SHAPES)
def test_head_step_matches_float64_and_is_reproducible(B, S, Qn, N, Fd, dev, ws):
    from fumi_amd import hip
    (f_s, y_s, f_q, y_q), ref = _ref((B, S, Qn, N, Fd))
    assert ref["margin"].min() > MARGIN                                           # every prediction is compared
    xs, ys, xq, yq = _gpu(dev, f_s, y_s, f_q, y_q)
    params = _params(dev)
    out = hip.ridge_head_step(ws, xs, ys, xq, yq, params, need_grad=True, grad_scale=GRAD_SCALE, want_logits=True, n_way=N)
    assert ws.read_status() == 0
    _check(out, ref, f"fused ({B},{S},{Qn},{N},{Fd})")
    # the forward form and a second call: the same bits
    fwd = hip.ridge_head_step(ws, xs, ys, xq, yq, params, need_grad=False, want_logits=True, n_way=N)
    assert fwd["dfeats_s"] is None and fwd["dfeats_q"] is None and fwd["dparams"] is None
    for k in ("loss", "correct", "preds", "logits"):
        assert torch.equal(fwd[k], out[k]), k
    again = hip.ridge_head_step(ws, xs, ys, xq, yq, params, need_grad=True, grad_scale=GRAD_SCALE, want_logits=True, n_way=N)
    for k in ("loss", "correct", "preds", "logits", "dfeats_s", "dfeats_q", "dparams"):
        assert torch.equal(again[k], out[k]), k
    assert ws.read_status() == 0
    # second witness: torch fp32 cholesky_solve on the GPU, against the same float64 logits
    Y = torch.nn.functional.one_hot(ys, N).float()
    M = torch.bmm(xs, xs.transpose(1, 2)) + float(np.exp(RHO)) * torch.eye(S, device=dev)
    z = ALPHA * torch.bmm(xq, torch.bmm(xs.transpose(1, 2), torch.cholesky_solve(Y, torch.linalg.cholesky(M))))
    e = rel_to_max(z.cpu(), ref["logits"])
    print(f"torch cholesky_solve ({B},{S},{Qn},{N},{Fd}) logits: rel-to-max error {e:.3e}")
    assert e <= TOL


SMALL = (2, 7, 33, 3, 96)


def _small_case():
    (f_s, y_s, f_q, y_q), _ = _ref(SMALL)
    return SMALL + (f_s.copy(), y_s.copy(), f_q.copy(), y_q.copy())


def _run(dev, ws, f_s, y_s, f_q, y_q, N):
    from fumi_amd import hip
    xs, ys, xq, yq = _gpu(dev, f_s, y_s, f_q, y_q)
    return hip.ridge_head_step(ws, xs, ys, xq, yq, _params(dev), need_grad=True, grad_scale=GRAD_SCALE, want_logits=True, n_way=N)


def test_query_label_out_of_range_sets_the_status_bit_and_drops_the_row(dev, ws):
    from fumi_amd import hip
    B, S, Qn, N, Fd, f_s, y_s, f_q, y_q = _small_case()
    y_q[1, 20] = N
    ref = ridge_head_ref(f_s, y_s, f_q, y_q, (RHO, ALPHA), N, GRAD_SCALE)
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
    ref = ridge_head_ref(f_s, y_s, f_q, y_q, (RHO, ALPHA), N, GRAD_SCALE)
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
    ref = ridge_head_ref(f_s, y_s, f_q, y_q, (RHO, ALPHA), N, GRAD_SCALE)
    assert ref["status"] == ST_CLASS_MISSING
    out = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    assert ws.read_status() == hip.ST_CLASS_MISSING
    assert ws.read_status() == 0
    assert float(out["logits"][1, :, 2].abs().max()) == 0.0
    _check(out, ref, "class without support")


def test_a_nan_in_one_episode_sets_not_posdef_and_leaves_the_other_episode_alone(dev, ws):
    """A status path on code that runs a fixed number of steps whatever the values are: no index depends on a float."""
    from fumi_amd import hip
    B, S, Qn, N, Fd, f_s, y_s, f_q, y_q = _small_case()
    clean = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    assert ws.read_status() == 0
    f_s[1, 2, 5] = np.nan
    out = _run(dev, ws, f_s, y_s, f_q, y_q, N)
    st = ws.read_status()
    assert st & hip.ST_NOT_POSDEF and not st & ~hip.ST_NOT_POSDEF
    assert ws.read_status() == 0
    assert torch.equal(out["logits"][0], clean["logits"][0])
    assert torch.equal(out["dfeats_q"][0], clean["dfeats_q"][0]) and torch.equal(out["dfeats_s"][0], clean["dfeats_s"][0])
    with pytest.raises(FloatingPointError):
        hip.raise_on_status(st)


# S = 129, N = 1, N = 65, F = 48, Qn = 0
@pytest.mark.parametrize("B,S,Qn,N,Fd", [(1, 129, 4, 2, 32), (1, 4, 4, 1, 32), (1, 65, 4, 65, 32), (1, 4, 4, 2, 48), (1, 4, 0, 2, 32)])
def test_unsupported_shapes_are_refused(B, S, Qn, N, Fd, dev, ws):
    from fumi_amd import hip
    xs, xq = torch.zeros(B, S, Fd, device=dev), torch.zeros(B, Qn, Fd, device=dev)
    ys, yq = torch.zeros(B, S, dtype=torch.int64, device=dev), torch.zeros(B, Qn, dtype=torch.int64, device=dev)
    with pytest.raises(hip.FumiHipError, match="fumi_hip_ridge_head_step"):
        hip.ridge_head_step(ws, xs, ys, xq, yq, _params(dev), need_grad=False, n_way=N)
    with pytest.raises(hip.FumiHipError, match="fumi_hip_ridge_head_step"):
        hip.ridge_head_step(ws, xs, ys, xq, yq, _params(dev), need_grad=True, n_way=N)
    assert ws.read_status() == 0


def test_part_of_the_gradient_pointers_or_no_params_is_an_invalid_argument(dev, ws):
    from ctypes import c_void_p
    from fumi_amd import hip
    B, S, Qn, N, Fd = 1, 4, 4, 2, 32
    xs, xq = torch.zeros(B, S, Fd, device=dev), torch.zeros(B, Qn, Fd, device=dev)
    ys, yq = torch.zeros(B, S, dtype=torch.int64, device=dev), torch.zeros(B, Qn, dtype=torch.int64, device=dev)
    params, loss, correct = _params(dev), torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    dfs, dfq, dpar = torch.zeros_like(xs), torch.zeros_like(xq), torch.zeros(2, device=dev)
    p = lambda t: c_void_p(t.data_ptr()) if t is not None else None
    for grads in ((dfs, None, None), (None, dfq, None), (None, None, dpar), (dfs, dfq, None), (None, dfq, dpar), (dfs, None, dpar)):
        rc = hip.lib().fumi_hip_ridge_head_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, p(xs), p(ys), p(xq), p(yq), p(params), 1.0,
                                                p(loss), p(correct), None, None, *(p(g) for g in grads))
        assert rc == -1, grads                                                    # FUMI_EINVAL
    rc = hip.lib().fumi_hip_ridge_head_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, p(xs), p(ys), p(xq), p(yq), None, 1.0,
                                            p(loss), p(correct), None, None, None, None, None)
    assert rc == -1                                                               # params is required
    assert ws.read_status() == 0
