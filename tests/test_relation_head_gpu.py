"""GPU parity of the fused Relation Network head (fumi_hip_relation_head_step, csrc/relationhead.hip) against the float64 restatement
tests/relation_head_ref.py (tied to torch.autograd at 1e-10 by tests/test_relation_head_cpu.py).

Tolerances are the ones the fp32 paths are held to against float64 (tests/test_hip_parity.py:18-20): 1e-4 of the largest magnitude of
each compared tensor (hid_s and hid_q included), 1e-4 relative on the loss; predictions and ``correct`` are compared exactly on the
parity cases -- tests/test_relation_head_cpu.py asserts that each has status 0 and a top-two margin above 1e-5.  The ReLU's kink is the
one place where fp32 and float64 may legitimately disagree, so the backward is compared TEACHER-FORCED: the kernels' mask is rebuilt
from their hid_s + hid_q in fp32 (one addition, the contract of include/fumi_hip.h), it may differ from the reference's pre > 0 only
where |pre| <= 1e-5 max|pre|, and the reference's backward runs on that mask.  grad_scale = 0.25.

Measured on one MI355X (profiles/relation_head/gpu_tests.log), worst over both losses, each in the unit of its own
bound of 1e-4: on the six parity cases logits 0.0090, hid_s 0.010, hid_q 0.012, loss 0.0013, dfeats_s 0.0090, dfeats_q 0.0095, dw1
0.0040, db1 0.0060, dw2 0.011, db2 0.033; at the limit shape dw2 0.081, dfeats_s and dw1 0.050; no mask entry differs in any case; the
torch-ops witness at one shot at most 0.0070."""
from ctypes import c_void_p

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from helpers import rel_to_max
from relation_head_ref import (GRAD_SCALE, LIMITS, LOSSES, ONE_SHOT, SHAPES, ST_CLASS_MISSING, ST_LABEL_RANGE, UNCERTAIN, case,
                               relation_head_ref)

pytestmark = pytest.mark.gpu
TOL, MARGIN = 1e-4, 1e-5          # tests/test_hip_parity.py:18-20
FWD = ("loss", "correct", "preds", "logits", "hid_s", "hid_q")
GRADS = ("dfeats_s", "dfeats_q", "dw1", "db1", "dw2", "db2")

_REFS = {}


def _case(shape, loss):
    """(inputs, weights, float64 reference) of a parity case, computed once and shared."""
    if (shape, loss) not in _REFS:
        inputs, w = case(shape)
        _REFS[(shape, loss)] = (inputs, w, relation_head_ref(*inputs, *w, shape[3], loss, GRAD_SCALE))
    return _REFS[(shape, loss)]


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


def _step(dev, ws, inputs, w, N, loss, need_grad=True):
    from fumi_amd import hip
    xs, ys, xq, yq = _gpu(dev, *inputs)
    return hip.relation_head_step(ws, xs, ys, xq, yq, _gpu(dev, *w), loss=loss, need_grad=need_grad, grad_scale=GRAD_SCALE,
                                  want_logits=True, want_hidden=True, n_way=N)


def _kernel_mask(out):
    """The mask the kernels used: fl32(hid_s[n,h] + hid_q[q,h]) > 0, one fp32 addition."""
    U, V = out["hid_s"].cpu().numpy(), out["hid_q"].cpu().numpy()
    assert U.dtype == np.float32 and V.dtype == np.float32
    return (V[:, :, None, :] + U[:, None, :, :]) > np.float32(0.0)


def _check_forward(got, ref, what, exact_preds=True):
    e = abs(float(got["loss"]) - ref["loss"]) / max(abs(ref["loss"]), 1e-5)
    print(f"{what} loss: relative error {e:.3e}")
    assert e <= TOL, what
    if exact_preds:
        assert np.array_equal(got["preds"].cpu().numpy(), ref["preds"]) and float(got["correct"]) == ref["correct"], what
    for k in ("logits", "hid_s", "hid_q"):
        e = rel_to_max(got[k].cpu(), ref[k])
        print(f"{what} {k}: rel-to-max error {e:.3e}")
        assert e <= TOL, (what, k, e)


def _check_mask(got, ref, what):
    """The kernels' mask against the reference's: different only inside the uncertain set.  Returns the kernels' mask."""
    mask, pre = _kernel_mask(got), ref["pre"]
    differ = mask != (pre > 0.0)
    uncertain = np.abs(pre) <= UNCERTAIN * np.abs(pre).max()
    print(f"{what} mask: {int(differ.sum())} of {differ.size} entries differ, {int(uncertain.sum())} uncertain")
    assert not (differ & ~uncertain).any(), what
    return mask


def _check_grads(got, forced, what, loss, db1_cancels=False):
    """Each gradient within 1e-4 of its largest magnitude.  db2 = sum dz is one number: with the mse loss it is held to 1e-4 of itself;
    with the ce loss every row of dz = softmax - onehot sums to zero, so db2 is zero in exact arithmetic (the float64 reference returns
    its own round-off, ~1e-18) and no fp32 sum can be within 1e-4 of that: there the error is held to 1e-4 of db2_abs = sum |dz|, the
    scale of the terms that cancel -- the rule tests/test_match_head_gpu.py applies to dtau against dtau_abs.  ``db1_cancels``: the limit
    case forces every hidden unit on or off for ALL pairs, so with the ce loss db1[h] = w2[h] sum_q sum_n dz[q,n] is zero in exact
    arithmetic as well; there it is held to 1e-4 of db1_abs = max_h sum |dU[n,h]| by the same argument."""
    for k in GRADS:
        if k == "db1" and loss == "ce" and db1_cancels:
            e = float(np.abs(got[k].cpu().numpy().astype(np.float64) - forced[k]).max()) / forced["db1_abs"]
            print(f"{what} db1: largest {float(got[k].abs().max()):.3e} against {np.abs(forced[k]).max():.3e}, error {e:.3e} of db1_abs "
                  f"{forced['db1_abs']:.3e}")
            assert e <= TOL, (what, k, e)
            continue
        if k == "db2" and loss == "ce":
            e = abs(float(got[k]) - float(forced[k][0])) / forced["db2_abs"]
            print(f"{what} db2: {float(got[k]):.3e} against {float(forced[k][0]):.3e}, error {e:.3e} of db2_abs {forced['db2_abs']:.3e}")
            assert e <= TOL, (what, k, e)
            continue
        e = rel_to_max(got[k].cpu(), forced[k])
        print(f"{what} {k}: rel-to-max error {e:.3e}")
        assert e <= TOL, (what, k, e)


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_head_step_matches_float64_and_is_reproducible(shape, loss, dev, ws):
    inputs, w, ref = _case(shape, loss)
    assert ref["status"] == 0 and ref["margin"].min() > MARGIN                    # every prediction is compared, here: equal
    what = f"fused {shape} {loss}"
    out = _step(dev, ws, inputs, w, shape[3], loss)
    assert ws.read_status() == 0
    _check_forward(out, ref, what)
    mask = _check_mask(out, ref, what)
    forced = ref if np.array_equal(mask, ref["pre"] > 0.0) else relation_head_ref(*inputs, *w, shape[3], loss, GRAD_SCALE, mask=mask)
    _check_grads(out, forced, what, loss)
    # the forward form and a second call: the same bits
    fwd = _step(dev, ws, inputs, w, shape[3], loss, need_grad=False)
    assert all(fwd[k] is None for k in GRADS)
    for k in FWD:
        assert torch.equal(fwd[k], out[k]), k
    again = _step(dev, ws, inputs, w, shape[3], loss)
    for k in FWD + GRADS:
        assert torch.equal(again[k], out[k]), k


@pytest.mark.parametrize("loss", LOSSES)
def test_one_shot_agrees_with_torch_ops_on_the_device(loss, dev, ws):
    """The second witness: the float32 torch-ops expression with autograd on the device.  Its own mask may differ from the kernels' at
    the kink; the rows and columns such an entry touches are set aside, at most 1e-3 of the entries."""
    shape = ONE_SHOT
    B, S, Qn, N, F, H = shape
    inputs, w, ref = _case(shape, loss)
    out = _step(dev, ws, inputs, w, N, loss)
    assert ws.read_status() == 0
    xs, ys, xq, yq = _gpu(dev, *inputs)
    xs.requires_grad_(True); xq.requires_grad_(True)
    w1, b1, w2, b2 = (t.requires_grad_(True) for t in _gpu(dev, *w))
    oh = Fn.one_hot(ys, N).float()
    c = torch.bmm(oh.transpose(1, 2), xs) / oh.sum(1).clamp(min=1.0)[:, :, None]
    pre = (Fn.linear(c, w1[0], b1)[:, None, :, :] + Fn.linear(xq, w1[1])[:, :, None, :])
    z = torch.relu(pre) @ w2 + b2
    val = torch.nn.MSELoss()(torch.sigmoid(z), Fn.one_hot(yq, N).float()) if loss == "mse" else Fn.cross_entropy(z.reshape(-1, N), yq.reshape(-1))
    (GRAD_SCALE * val).backward()
    differ = torch.as_tensor(_kernel_mask(out)).to(dev) != (pre.detach() > 0)    # [B, Qn, N, H]
    print(f"one shot {loss}: {int(differ.sum())} mask entries differ between the kernels and the torch expression")
    assert float(differ.float().mean()) <= 1e-3
    e = abs(float(out["loss"]) - float(val.detach())) / max(abs(float(val.detach())), 1e-5)
    print(f"one shot {loss} loss: relative error {e:.3e}")
    assert e <= TOL
    e = rel_to_max(out["logits"].cpu(), z.detach().cpu().double().numpy())
    print(f"one shot {loss} logits: rel-to-max error {e:.3e}")
    assert e <= TOL and torch.equal(out["preds"], z.argmax(-1))
    bad_b, bad_h = differ.any(dim=3).any(dim=2).any(dim=1), differ.any(dim=2).any(dim=1).any(dim=0)     # episodes, hidden units
    keep = {"dfeats_s": ~bad_b[:, None, None].expand(B, S, F), "dfeats_q": ~bad_b[:, None, None].expand(B, Qn, F),
            "dw1": ~bad_h[None, :, None].expand(2, H, F), "db1": ~bad_h, "dw2": ~bad_h, "db2": None}
    excluded = 0.0
    for k, t in (("dfeats_s", xs), ("dfeats_q", xq), ("dw1", w1), ("db1", b1), ("dw2", w2), ("db2", b2)):
        if bool(differ.any()) and k == "db2":
            continue                                                               # (db2 sums every entry)
        m = keep[k] if keep[k] is not None else torch.ones_like(t, dtype=torch.bool)
        excluded = max(excluded, 1.0 - float(m.float().mean()))
        if k == "db2" and loss == "ce":                                            # (zero in exact arithmetic: see _check_grads)
            e = abs(float(out[k]) - float(t.grad)) / ref["db2_abs"]
            print(f"one shot {loss} db2: error {e:.3e} of db2_abs")
            assert e <= TOL
            continue
        g, r = out[k] * m, t.grad * m
        e = rel_to_max(g.cpu(), r.cpu().double().numpy())
        print(f"one shot {loss} {k}: rel-to-max error {e:.3e}")
        assert e <= TOL, (k, e)
    assert excluded <= 1e-3


SMALL = SHAPES[0]


def _small(loss):
    inputs, w, _ = _case(SMALL, loss)
    return [a.copy() for a in inputs], w


def _check_case(dev, ws, inputs, w, loss, status, what):
    from fumi_amd import hip
    ref = relation_head_ref(*inputs, *w, SMALL[3], loss, GRAD_SCALE)
    assert ref["status"] == status
    out = _step(dev, ws, inputs, w, SMALL[3], loss)
    assert ws.read_status() == status
    assert ws.read_status() == 0                                                  # (reading clears the word)
    _check_forward(out, ref, what, exact_preds=bool(ref["margin"].min() > MARGIN))
    mask = _check_mask(out, ref, what)
    _check_grads(out, relation_head_ref(*inputs, *w, SMALL[3], loss, GRAD_SCALE, mask=mask), what, loss)
    return out, ref


@pytest.mark.parametrize("loss", LOSSES)
def test_labels_out_of_range_and_a_class_without_support(loss, dev, ws):
    from fumi_amd import hip
    assert (hip.ST_LABEL_RANGE, hip.ST_CLASS_MISSING) == (ST_LABEL_RANGE, ST_CLASS_MISSING)
    inputs0, w = _small(loss)
    plain = _step(dev, ws, inputs0, w, SMALL[3], loss)
    assert ws.read_status() == 0
    # a query label out of range, in episode 1
    inputs, _ = _small(loss)
    inputs[3][1, 20] = SMALL[3]
    out, _ = _check_case(dev, ws, inputs, w, loss, ST_LABEL_RANGE, f"query label out of range {loss}")
    assert float(out["dfeats_q"][1, 20].abs().max()) == 0.0
    for k in ("logits", "preds", "hid_s", "hid_q", "dfeats_s", "dfeats_q"):
        assert torch.equal(out[k][0], plain[k][0]), k                             # the other episode is untouched
    # a support label out of range, in episode 0 (a row of class 0, which has three)
    inputs, _ = _small(loss)
    i0 = int(np.nonzero(inputs[1][0] == 0)[0][-1])
    inputs[1][0, i0] = SMALL[3] + 2
    out, _ = _check_case(dev, ws, inputs, w, loss, ST_LABEL_RANGE, f"support label out of range {loss}")
    assert float(out["dfeats_s"][0, i0].abs().max()) == 0.0
    for k in ("logits", "preds", "hid_s", "hid_q", "dfeats_s", "dfeats_q"):
        assert torch.equal(out[k][1], plain[k][1]), k
    # a class without support, in episode 1: a zero prototype, U = b1
    inputs, _ = _small(loss)
    inputs[1][1][inputs[1][1] == 2] = 1
    out, _ = _check_case(dev, ws, inputs, w, loss, ST_CLASS_MISSING, f"class without support {loss}")
    assert torch.equal(out["hid_s"][1, 2].cpu(), torch.as_tensor(w[1]))
    for k in ("logits", "preds", "hid_s", "hid_q", "dfeats_s", "dfeats_q"):
        assert torch.equal(out[k][0], plain[k][0]), k


def test_the_shapes_at_the_limits_run(dev, ws):
    """S = 1024 and B * Qn = 65536 with N = 2, F = H = 32 (N = 64, F = 2048 and H = 1024 are among the parity cases).  b1 is set to
    +-4 max|U + V - b1| with the sign alternating in h: every hidden unit is firmly on or firmly off, so the case tests indexing only."""
    inputs, (w1, _, w2, b2) = case(LIMITS)
    N, H = LIMITS[3], LIMITS[5]
    zero = relation_head_ref(*inputs, w1, np.zeros(H), w2, b2, N, "mse", GRAD_SCALE)
    amp = 4.0 * float(np.abs(zero["pre"]).max())
    b1 = (amp * np.where(np.arange(H) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    del zero
    w = (w1, b1, w2, b2)
    for loss in LOSSES:
        ref = relation_head_ref(*inputs, *w, N, loss, GRAD_SCALE)
        assert ref["status"] == 0 and np.abs(ref["pre"]).min() > 0.5 * amp         # the uncertain set is empty by construction
        out = _step(dev, ws, inputs, w, N, loss)
        assert ws.read_status() == 0
        what = f"fused {LIMITS} {loss}"
        _check_forward(out, ref, what, exact_preds=False)
        safe = ref["margin"] > MARGIN
        assert np.array_equal(out["preds"].cpu().numpy()[safe], ref["preds"][safe])
        assert abs(float(out["correct"]) - ref["correct"]) <= int((~safe).sum())
        assert np.array_equal(_kernel_mask(out), ref["pre"] > 0.0)
        _check_grads(out, ref, what, loss, db1_cancels=True)


def _raw_call(dev, ws, B, S, Qn, N, Fd, H, kind, req=None, grads=6, fill=7.0):
    """A call of the entry with every pointer given (grads: how many of the six gradient pointers, from the front, or a tuple of
    flags); req: indices of the ten required pointers to pass as NULL.  Returns (rc, the outputs)."""
    from fumi_amd import hip
    m = lambda v: max(v, 1)
    xs, xq = torch.zeros(m(B), m(S), m(Fd), device=dev), torch.zeros(m(B), m(Qn), m(Fd), device=dev)
    ys = (torch.arange(m(S), device=dev) % max(N, 1)).repeat(m(B), 1)
    yq = torch.zeros(m(B), m(Qn), dtype=torch.int64, device=dev)
    w1, b1, w2, b2 = (torch.zeros(2, m(H), m(Fd), device=dev), torch.zeros(m(H), device=dev), torch.zeros(m(H), device=dev),
                      torch.zeros(1, device=dev))
    outs = dict(loss=torch.full((1,), fill, device=dev), correct=torch.full((1,), fill, device=dev),
                preds=torch.full((m(B), m(Qn)), 7, dtype=torch.int64, device=dev), logits=torch.full((m(B), m(Qn), m(N)), fill, device=dev),
                hid_s=torch.full((m(B), m(N), m(H)), fill, device=dev), hid_q=torch.full((m(B), m(Qn), m(H)), fill, device=dev),
                dfeats_s=torch.full_like(xs, fill), dfeats_q=torch.full_like(xq, fill), dw1=torch.full_like(w1, fill),
                db1=torch.full_like(b1, fill), dw2=torch.full_like(w2, fill), db2=torch.full_like(b2, fill))
    p = lambda t: c_void_p(t.data_ptr())
    required = [p(t) for t in (xs, ys, xq, yq, w1, b1, w2, b2, outs["loss"], outs["correct"])]
    for i in (req or ()):
        required[i] = None
    flags = grads if isinstance(grads, tuple) else tuple(i < grads for i in range(6))
    gp = [p(outs[k]) if f else None for k, f in zip(GRADS, flags)]
    rc = hip.lib().fumi_hip_relation_head_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, H, *required[:8], kind, 1.0,
                                               required[8], required[9], p(outs["preds"]), p(outs["logits"]), p(outs["hid_s"]),
                                               p(outs["hid_q"]), *gp)
    return rc, outs


def _untouched(outs, fill=7.0):
    torch.cuda.synchronize()
    return all(float(t.float().min()) == fill and float(t.float().max()) == fill for t in outs.values())


# on either side of every limit: F 48 / 0 / 2080, N 1 / 65, S 0 / 1025, Qn 0, B Qn 65537, B 0, H 0 / 48 / 1056, loss_kind 2
REFUSED = [(1, 4, 4, 2, 48, 32, 1), (1, 4, 4, 2, 0, 32, 1), (1, 4, 4, 2, 2080, 32, 1), (1, 4, 4, 1, 32, 32, 1), (1, 65, 4, 65, 32, 32, 1),
           (1, 0, 4, 2, 32, 32, 1), (1, 1025, 4, 2, 32, 32, 1), (1, 4, 0, 2, 32, 32, 1), (1, 4, 65537, 2, 32, 32, 1), (0, 4, 4, 2, 32, 32, 1),
           (1, 4, 4, 2, 32, 0, 1), (1, 4, 4, 2, 32, 48, 1), (1, 4, 4, 2, 32, 1056, 1), (1, 4, 4, 2, 32, 32, 2)]


@pytest.mark.parametrize("B,S,Qn,N,Fd,H,kind", REFUSED)
def test_unsupported_shapes_are_refused_before_any_launch(B, S, Qn, N, Fd, H, kind, dev, ws):
    for grads in (0, 6):
        rc, outs = _raw_call(dev, ws, B, S, Qn, N, Fd, H, kind, grads=grads)
        assert rc == -4                                                           # FUMI_ENOTSUP
        assert _untouched(outs)
    assert ws.read_status() == 0


def test_the_shapes_just_inside_the_limits_are_accepted(dev, ws):
    from fumi_amd import hip
    for B, S, Qn, N, Fd, H in ((1, 1, 1, 2, 32, 32), (1, 64, 2, 64, 32, 1024), (1, 1024, 1, 2, 32, 32), (2, 2, 32768, 2, 32, 32),
                               (1, 2, 2, 2, 2048, 32)):
        xs, xq = torch.ones(B, S, Fd, device=dev), torch.ones(B, Qn, Fd, device=dev)
        ys = (torch.arange(S, device=dev) % N).repeat(B, 1)
        yq = torch.zeros(B, Qn, dtype=torch.int64, device=dev)
        w = [torch.full((2, H, Fd), 0.01, device=dev), torch.zeros(H, device=dev), torch.full((H,), 0.1, device=dev), torch.zeros(1, device=dev)]
        for loss in LOSSES:
            out = hip.relation_head_step(ws, xs, ys, xq, yq, w, loss=loss, n_way=N, want_logits=True)
            assert all(bool(torch.isfinite(out[k]).all()) for k in ("loss", "logits") + GRADS)
            assert ws.read_status() == (hip.ST_CLASS_MISSING if S < N else 0)


def test_a_missing_pointer_or_part_of_the_gradient_pointers_is_an_invalid_argument(dev, ws):
    import itertools
    B, S, Qn, N, Fd, H = 1, 4, 4, 2, 32, 32
    for flags in itertools.product((False, True), repeat=6):
        if 0 < sum(flags) < 6:
            rc, outs = _raw_call(dev, ws, B, S, Qn, N, Fd, H, 1, grads=flags)
            assert rc == -1 and _untouched(outs), flags                           # FUMI_EINVAL
    for i in range(10):                                                           # feats_s .. b2, loss, correct
        for grads in (0, 6):
            rc, outs = _raw_call(dev, ws, B, S, Qn, N, Fd, H, 1, req=(i,), grads=grads)
            assert rc == -1 and _untouched(outs), i
    for grads in (0, 6):
        rc, outs = _raw_call(dev, ws, B, S, Qn, N, Fd, H, 1, grads=grads)
        assert rc == 0 and not _untouched(outs)
    assert ws.read_status() == 0


# ---- the model ----------------------------------------------------------------------------------------------------------------------
MB, MN, MK, MQ, SIZE = 2, 3, 2, 2, 16


def _batch(seed, dev):
    """An episodic meta-batch in the format of the pixel samplers, resident on the device; unequal shots (class 0 has one row more)."""
    g = torch.Generator().manual_seed(seed)
    S = MN * MK + 1
    y_s = torch.stack([(torch.arange(S) % MN)[torch.randperm(S, generator=g)] for _ in range(MB)])
    y_q = torch.stack([(torch.arange(MN * MQ) % MN)[torch.randperm(MN * MQ, generator=g)] for _ in range(MB)])
    mu = torch.randn(MB, MN, 3, SIZE, SIZE, generator=g)
    bi = torch.arange(MB)[:, None]
    x_s = mu[bi, y_s] + 0.5 * torch.randn(MB, S, 3, SIZE, SIZE, generator=g)
    x_q = mu[bi, y_q] + 0.5 * torch.randn(MB, MN * MQ, 3, SIZE, SIZE, generator=g)
    return {"train": ((None, None, x_s.to(dev)), y_s.to(dev)), "test": ((None, None, x_q.to(dev)), y_q.to(dev))}


def _model(dev, loss="mse"):
    from fumi_amd.models.metabaseline import MetaBaseline
    torch.manual_seed(17)
    return MetaBaseline("conv4", image_size=SIZE, image_channels=3, num_ways=MN, head="relation", relation=dict(hidden=64, loss=loss)).to(dev)


def test_training_step_leaves_finite_gradients_and_the_loss_of_few_shot(dev):
    from fumi_amd import hip
    model, batch = _model(dev), _batch(3, dev)
    loss, acc = model.evaluate(batch, None, None, dev, task="train")
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
    for name, p in model.relation.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), name
    assert any(float(p.grad.abs().max()) > 0.0 for p in model.relation.parameters())
    for name, p in zip(model.conv.theta_names("conv."), model.conv.theta()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert any(float(p.grad.abs().max()) > 0.0 for p in model.conv.theta())
    with torch.no_grad():
        fs_loss, fs_acc = model.few_shot(batch, dev).tolist()
    print(f"train_step loss {float(loss):.7f}, few_shot loss {fs_loss:.7f}")
    assert np.isfinite(float(loss)) and abs(float(loss) - fs_loss) <= 1e-5 and float(acc) == fs_acc


@pytest.mark.parametrize("loss", LOSSES)
def test_twenty_adam_steps_on_one_batch_lower_the_loss(loss, dev):
    from fumi_amd.optim import Adam
    model, batch = _model(dev, loss), _batch(5, dev)
    opt = Adam(params=model.parameters(), lr=1e-3)
    losses = [float(model.evaluate(batch, opt, None, dev, task="train")[0]) for _ in range(20)]
    print(f"{loss} losses:", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_max_grad_norm_on_the_fused_optimizer_sees_the_relation_tensors(dev):
    from fumi_amd.optim import Adam
    model, batch = _model(dev), _batch(7, dev)
    before = [p.detach().clone() for p in model.relation.tensors()]
    opt = Adam(params=model.parameters(), lr=1e-3, max_grad_norm=1e-3)
    losses = [float(model.evaluate(batch, opt, None, dev, task="train")[0]) for _ in range(3)]
    assert all(np.isfinite(losses))
    assert model._flat.views[0].shape == model.relation.w1.shape and model.relation.w1.grad is model._flat.views[0]
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.relation.tensors()))
