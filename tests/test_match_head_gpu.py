"""GPU parity of the fused Matching Networks head (fumi_hip_match_head_step, csrc/matchhead.hip) against the float64 restatement
tests/match_head_ref.py (tied to torch.autograd at 1e-10 and, at one row per class, to tests/cos_proto_ref.py at 1e-12 by
tests/test_match_head_cpu.py).

Tolerances are the ones the fp32 paths are held to against float64 (tests/test_hip_parity.py:18-20): 1e-4 of the largest magnitude of
each compared tensor, 1e-4 relative on the loss, dtau within 1e-4 of dtau_abs = sum |da cos|; predictions and ``correct`` are compared
exactly -- tests/test_match_head_cpu.py asserts that every parity shape has status 0 and a top-two margin above 1e-5, so no row is set
aside.  tau = 10, grad_scale = 0.25.  The second witness at one shot per class is cos_proto_step on the same inputs.  The saturated case
(tau = 100, a class about 200 below the row's largest) holds every finite logit to the same bound and admits no inf or nan.

Measured on one MI355X (profiles/matching_head/gpu_tests.log), worst over the six parity shapes, each in the unit
of its own bound of 1e-4: logits 0.0032, dfeats_s 0.035, dfeats_q 0.037, loss 0.036, dtau 0.041; at the limit shape dfeats_s 0.061; the
saturated case at most 0.011 (dfeats_s); one shot against the cosine head at most 0.0023."""
import numpy as np
import pytest
import torch

from helpers import rel_to_max
from match_head_ref import (GRAD_SCALE, LIMITS, ONE_SHOT, SATURATED, SHAPES, ST_CLASS_MISSING, ST_LABEL_RANGE, TAU, TAU_SATURATED,
                            case_inputs, match_head_ref, saturated_inputs)

pytestmark = pytest.mark.gpu
TOL, MARGIN = 1e-4, 1e-5          # tests/test_hip_parity.py:18-20

_REFS = {}


def _case(shape):
    """(inputs, float64 reference) of a parity shape, computed once and shared."""
    if shape not in _REFS:
        inputs = case_inputs(*shape)
        _REFS[shape] = (inputs, match_head_ref(*inputs, TAU, shape[3], GRAD_SCALE))
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


def _finite_rel(got, ref):
    """Largest error over the entries the reference has finite, relative to the largest finite magnitude; the others must be equal."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin])
    return float(np.abs(got[fin] - ref[fin]).max() / max(np.abs(ref[fin]).max(), 1e-30))


def _check(got, ref, what, grads=True, exact_preds=True):
    e = abs(float(got["loss"]) - ref["loss"]) / max(abs(ref["loss"]), 1e-5)
    print(f"{what} loss: relative error {e:.3e}")
    assert e <= TOL, what
    if exact_preds:
        assert np.array_equal(got["preds"].cpu().numpy(), ref["preds"]) and float(got["correct"]) == ref["correct"], what
    e = _finite_rel(got["logits"].cpu().numpy(), ref["logits"])
    print(f"{what} logits: rel-to-max error {e:.3e}")
    assert e <= TOL, (what, "logits", e)
    if grads:
        for k in ("dfeats_s", "dfeats_q"):
            e = rel_to_max(got[k].cpu(), ref[k])
            print(f"{what} {k}: rel-to-max error {e:.3e}")
            assert e <= TOL, (what, k, e)
        e = abs(float(got["dtau"]) - ref["dtau"]) / ref["dtau_abs"]
        print(f"{what} dtau: {float(got['dtau']):.6e} against {ref['dtau']:.6e}, error {e:.3e} of dtau_abs {ref['dtau_abs']:.3e}")
        assert e <= TOL, (what, e)


def _step(dev, ws, inputs, shape, need_grad=True, tau=TAU):
    from fumi_amd import hip
    xs, ys, xq, yq = _gpu(dev, *inputs)
    t = torch.tensor([tau], device=dev, dtype=torch.float32)
    return hip.match_head_step(ws, xs, ys, xq, yq, t, need_grad=need_grad, grad_scale=GRAD_SCALE, want_logits=True, n_way=shape[3])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_head_step_matches_float64_and_is_reproducible(shape, dev, ws):
    inputs, ref = _case(shape)
    assert ref["status"] == 0 and ref["margin"].min() > MARGIN                    # every prediction is compared, here: equal
    out = _step(dev, ws, inputs, shape)
    assert ws.read_status() == 0
    _check(out, ref, f"fused {shape}")
    # the forward form and a second call: the same bits
    fwd = _step(dev, ws, inputs, shape, need_grad=False)
    assert fwd["dfeats_s"] is None and fwd["dfeats_q"] is None and fwd["dtau"] is None
    for k in ("loss", "correct", "preds", "logits"):
        assert torch.equal(fwd[k], out[k]), k
    again = _step(dev, ws, inputs, shape)
    for k in ("loss", "correct", "preds", "logits", "dfeats_s", "dfeats_q", "dtau"):
        assert torch.equal(again[k], out[k]), k


def test_one_shot_agrees_with_the_cosine_head(dev, ws):
    """The second witness: at one row per class the class log-mass is the row's score, and cos_proto_step computes the same head."""
    from fumi_amd import hip
    inputs, ref = _case(ONE_SHOT)
    out = _step(dev, ws, inputs, ONE_SHOT)
    xs, ys, xq, yq = _gpu(dev, *inputs)
    cos = hip.cos_proto_step(ws, xs, ys, xq, yq, torch.tensor([TAU], device=dev), need_grad=True, grad_scale=GRAD_SCALE,
                             want_logits=True, n_way=ONE_SHOT[3])
    assert ws.read_status() == 0
    for k in ("logits", "dfeats_s", "dfeats_q"):
        e = rel_to_max(out[k].cpu(), cos[k].cpu().double().numpy())
        print(f"one shot, matching against cosine {k}: rel-to-max error {e:.3e}")
        assert e <= TOL, (k, e)
    e = abs(float(out["dtau"]) - float(cos["dtau"])) / ref["dtau_abs"]
    print(f"one shot, matching against cosine dtau: error {e:.3e} of dtau_abs")
    assert e <= TOL
    assert torch.equal(out["preds"], cos["preds"])


def test_saturated_scores_keep_every_class_finite_and_accurate(dev, ws):
    """Case C: tau = 100, the first query rows near-copies of a support row, another class pointing the opposite way."""
    inputs = saturated_inputs()
    ref = match_head_ref(*inputs, TAU_SATURATED, SATURATED[3], GRAD_SCALE)
    z = ref["logits"]
    assert np.isfinite(z).all() and ((z.max(-1) - z.min(-1)) > 110.0).any()
    for need_grad in (True, False):
        out = _step(dev, ws, inputs, SATURATED, need_grad=need_grad, tau=TAU_SATURATED)
        assert ws.read_status() == 0
        for k, v in out.items():
            if v is not None:
                assert bool(torch.isfinite(v.float()).all()), k                   # no inf or nan in any output
        _check(out, ref, f"saturated (training form: {need_grad})", grads=need_grad, exact_preds=bool(ref["margin"].min() > MARGIN))


SMALL = (2, 7, 33, 3, 96)


def _small_case():
    return tuple(a.copy() for a in case_inputs(*SMALL))


def test_query_label_out_of_range_sets_the_status_bit_and_drops_the_row(dev, ws):
    from fumi_amd import hip
    f_s, y_s, f_q, y_q = _small_case()
    y_q[1, 20] = SMALL[3]
    ref = match_head_ref(f_s, y_s, f_q, y_q, TAU, SMALL[3], GRAD_SCALE)
    assert ref["status"] == ST_LABEL_RANGE and not ref["dfeats_q"][1, 20].any()
    out = _step(dev, ws, (f_s, y_s, f_q, y_q), SMALL)
    assert ws.read_status() == hip.ST_LABEL_RANGE
    assert ws.read_status() == 0                                                  # (reading clears the word)
    assert float(out["dfeats_q"][1, 20].abs().max()) == 0.0
    _check(out, ref, "query label out of range")


def test_support_label_out_of_range_gives_the_episode_without_that_row(dev, ws):
    from fumi_amd import hip
    f_s, y_s, f_q, y_q = _small_case()
    i0, i1 = (int(np.nonzero(y_s[b] == 0)[0][-1]) for b in range(2))              # a row of class 0, which has three: every class keeps support
    y_s[0, i0], y_s[1, i1] = -1, SMALL[3] + 2
    ref = match_head_ref(f_s, y_s, f_q, y_q, TAU, SMALL[3], GRAD_SCALE)
    assert ref["status"] == ST_LABEL_RANGE and not ref["dfeats_s"][0, i0].any() and not ref["dfeats_s"][1, i1].any()
    out = _step(dev, ws, (f_s, y_s, f_q, y_q), SMALL)
    assert ws.read_status() == hip.ST_LABEL_RANGE
    assert ws.read_status() == 0
    assert float(out["dfeats_s"][0, i0].abs().max()) == 0.0 and float(out["dfeats_s"][1, i1].abs().max()) == 0.0
    _check(out, ref, "support label out of range")


def test_class_without_support_sets_the_status_bit_and_carries_no_mass(dev, ws):
    from fumi_amd import hip
    f_s, y_s, f_q, y_q = _small_case()
    y_s[1][y_s[1] == 2] = 1                                                       # episode 1 has no row of class 2
    ref = match_head_ref(f_s, y_s, f_q, y_q, TAU, SMALL[3], GRAD_SCALE)
    assert ref["status"] == ST_CLASS_MISSING and (y_q[1] == 2).any()
    out = _step(dev, ws, (f_s, y_s, f_q, y_q), SMALL)
    assert ws.read_status() == hip.ST_CLASS_MISSING
    assert ws.read_status() == 0
    logits = out["logits"].cpu().numpy()
    assert np.isneginf(logits[1, :, 2]).all() and np.isfinite(logits[0]).all() and np.isfinite(logits[1, :, :2]).all()
    lost = torch.as_tensor(y_q[1] == 2)
    assert float(out["dfeats_q"][1][lost.to(dev)].abs().max()) == 0.0             # a query row labelled with the missing class
    _check(out, ref, "class without support")
    # such rows add nothing to the loss: the same call with their labels out of range gives the same bits
    y_q2 = y_q.copy(); y_q2[1][y_q[1] == 2] = -1
    out2 = _step(dev, ws, (f_s, y_s, f_q, y_q2), SMALL)
    assert ws.read_status() == (hip.ST_CLASS_MISSING | hip.ST_LABEL_RANGE)
    for k in ("loss", "logits", "preds", "dfeats_s", "dfeats_q", "dtau"):
        assert torch.equal(out2[k], out[k]), k
    # the other episode is untouched
    plain = _step(dev, ws, _small_case(), SMALL)
    assert ws.read_status() == 0
    assert torch.equal(plain["logits"][0], out["logits"][0]) and torch.equal(plain["dfeats_q"][0], out["dfeats_q"][0])
    assert torch.equal(plain["dfeats_s"][0], out["dfeats_s"][0]) and torch.equal(plain["preds"][0], out["preds"][0])


def test_the_shapes_at_the_limits_run(dev, ws):
    """S = 512 and B * Qn = 65536 with N = 2, F = 32 (N = 64 and F = 2048 are among the parity shapes)."""
    inputs, ref = _case(LIMITS)
    out = _step(dev, ws, inputs, LIMITS)
    assert ws.read_status() == 0
    _check(out, ref, f"fused {LIMITS}", exact_preds=False)
    safe = ref["margin"] > MARGIN
    assert np.array_equal(out["preds"].cpu().numpy()[safe], ref["preds"][safe])
    assert abs(float(out["correct"]) - ref["correct"]) <= int((~safe).sum())


# on either side of every limit: F = 48 (no multiple of 32), F = 0, F = 2080, N = 1, N = 65, S = 0, S = 513, Qn = 0, B * Qn = 65537, B = 0
REFUSED = [(1, 4, 4, 2, 48), (1, 4, 4, 2, 0), (1, 4, 4, 2, 2080), (1, 4, 4, 1, 32), (1, 65, 4, 65, 32), (1, 0, 4, 2, 32), (1, 513, 4, 2, 32),
           (1, 4, 0, 2, 32), (1, 4, 65537, 2, 32), (0, 4, 4, 2, 32)]


@pytest.mark.parametrize("B,S,Qn,N,Fd", REFUSED)
def test_unsupported_shapes_are_refused_before_any_launch(B, S, Qn, N, Fd, dev, ws):
    from ctypes import c_void_p
    from fumi_amd import hip
    xs, xq = torch.zeros(B, S, Fd, device=dev), torch.zeros(B, Qn, Fd, device=dev)
    ys, yq = torch.zeros(B, S, dtype=torch.int64, device=dev), torch.zeros(B, Qn, dtype=torch.int64, device=dev)
    tau = torch.tensor([1.0], device=dev)
    for need_grad in (False, True):
        with pytest.raises(hip.FumiHipError, match="fumi_hip_match_head_step"):
            hip.match_head_step(ws, xs, ys, xq, yq, tau, need_grad=need_grad, n_way=N)
    # the documented code, with every pointer given; the outputs are not touched
    loss, correct = torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    dfs, dfq, dt = torch.ones(max(B, 1), max(S, 1), max(Fd, 1), device=dev), torch.ones(max(B, 1), max(Qn, 1), max(Fd, 1), device=dev), \
        torch.full((1,), 7.0, device=dev)
    preds = torch.full((max(B, 1), max(Qn, 1)), 7, dtype=torch.int64, device=dev)
    logits = torch.full((max(B, 1), max(Qn, 1), max(N, 1)), 7.0, device=dev)
    one = torch.zeros(1, device=dev)
    p = lambda t: c_void_p(t.data_ptr() if t.numel() else one.data_ptr())
    for grads in ((None, None, None), (p(dfs), p(dfq), p(dt))):
        rc = hip.lib().fumi_hip_match_head_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, p(xs), p(ys), p(xq), p(yq), p(tau), 1.0,
                                                p(loss), p(correct), p(preds), p(logits), *grads)
        assert rc == -4                                                           # FUMI_ENOTSUP
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and float(correct) == 7.0 and float(dt) == 7.0 and float(dfs.min()) == 1.0 and float(dfq.min()) == 1.0
    assert int(preds.min()) == 7 and float(logits.min()) == 7.0
    assert ws.read_status() == 0


def test_the_shapes_just_inside_the_limits_are_accepted(dev, ws):
    from fumi_amd import hip
    for B, S, Qn, N, Fd in ((1, 1, 1, 2, 32), (1, 64, 2, 64, 32)):
        xs, xq = torch.ones(B, S, Fd, device=dev), torch.ones(B, Qn, Fd, device=dev)
        ys = (torch.arange(S, device=dev) % N).repeat(B, 1)
        yq = torch.zeros(B, Qn, dtype=torch.int64, device=dev)
        out = hip.match_head_step(ws, xs, ys, xq, yq, torch.tensor([1.0], device=dev), n_way=N, want_logits=True)
        assert bool(torch.isfinite(out["loss"]).all()) and bool(torch.isfinite(out["dfeats_s"]).all())
        assert ws.read_status() == (hip.ST_CLASS_MISSING if S < N else 0)


def test_a_missing_pointer_or_part_of_the_gradient_pointers_is_an_invalid_argument(dev, ws):
    from ctypes import c_void_p
    from fumi_amd import hip
    B, S, Qn, N, Fd = 1, 4, 4, 2, 32
    xs, xq = torch.zeros(B, S, Fd, device=dev), torch.zeros(B, Qn, Fd, device=dev)
    ys, yq = (torch.arange(S, device=dev) % N).repeat(B, 1), torch.zeros(B, Qn, dtype=torch.int64, device=dev)      # both classes have support
    tau, loss, correct = torch.tensor([1.0], device=dev), torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    dfs, dfq, dt = torch.zeros_like(xs), torch.zeros_like(xq), torch.zeros(1, device=dev)
    p = lambda t: c_void_p(t.data_ptr()) if t is not None else None
    call = lambda req, grads: hip.lib().fumi_hip_match_head_step(ws.handle, hip._stream(dev), B, S, Qn, N, Fd, *(p(t) for t in req[:5]),
                                                                 1.0, p(req[5]), p(req[6]), None, None, *(p(g) for g in grads))
    required = [xs, ys, xq, yq, tau, loss, correct]
    for grads in ((dfs, None, None), (None, dfq, None), (None, None, dt), (dfs, dfq, None), (dfs, None, dt), (None, dfq, dt)):
        assert call(required, grads) == -1, grads                                 # FUMI_EINVAL
    for i in range(len(required)):                                                # feats_s, y_s, feats_q, y_q, tau, loss, correct
        req = list(required); req[i] = None
        assert call(req, (None, None, None)) == -1, i
        assert call(req, (dfs, dfq, dt)) == -1, i
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and float(correct) == 7.0                           # nothing was launched
    assert call(required, (dfs, dfq, dt)) == 0 and call(required, (None, None, None)) == 0
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


def _model(dev):
    from fumi_amd.models.metabaseline import MetaBaseline
    torch.manual_seed(17)
    return MetaBaseline("conv4", image_size=SIZE, image_channels=3, num_ways=MN, head="matching").to(dev)


def test_training_step_leaves_finite_gradients_and_the_loss_of_few_shot(dev):
    from fumi_amd import hip
    model, batch = _model(dev), _batch(3, dev)
    loss, acc = model.evaluate(batch, None, None, dev, task="train")
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
    assert model.temp.grad is not None and bool(torch.isfinite(model.temp.grad).all()) and float(model.temp.grad.abs()) > 0.0
    for name, p in zip(model.conv.theta_names("conv."), model.conv.theta()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert any(float(p.grad.abs().max()) > 0.0 for p in model.conv.theta())
    with torch.no_grad():
        fs_loss, fs_acc = model.few_shot(batch, dev).tolist()
    print(f"train_step loss {float(loss):.7f}, few_shot loss {fs_loss:.7f}")
    assert np.isfinite(float(loss)) and abs(float(loss) - fs_loss) <= 1e-5 and float(acc) == fs_acc


def test_twenty_adam_steps_on_one_batch_lower_the_loss(dev):
    from fumi_amd.optim import Adam
    model, batch = _model(dev), _batch(5, dev)
    opt = Adam(params=model.parameters(), lr=1e-3)
    losses = [float(model.evaluate(batch, opt, None, dev, task="train")[0]) for _ in range(20)]
    print("losses:", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


def test_pretrain_reports_by_the_matching_metric(dev):
    from fumi_amd import hip
    from fumi_amd.models.pretrain import Pretrain
    torch.manual_seed(19)
    model = Pretrain("conv4", image_size=SIZE, image_channels=3, n_classes=8, num_ways=MN, metric="matching", metric_temp=10.0).to(dev).eval()
    with torch.no_grad():
        loss, acc = model.few_shot(_batch(9, dev), dev).tolist()
    assert hip.Workspace.get(dev).read_status() == 0
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0
