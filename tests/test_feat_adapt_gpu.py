"""GPU parity of the set-to-set prototype adaptation (fumi_hip_feat_adapt_fwd / _bwd, csrc/featadapt.hip)
against the float64 restatement tests/feat_adapt_ref.py (tied to finite differences by tests/test_feat_adapt_cpu.py), over the case
table tests/feat_adapt_cases.py.

Every compared tensor -- protos_out, dfeats_s and the seven parameter gradients dWq, dWk, dWv, dWo, dbo, dgamma, dbeta -- is measured
as its largest error over its largest float64 magnitude and held to 1e-4, the project's bound for the heads (tests/test_cls_head_gpu.py).
Then: bit identity of the forward form against the taped form and of a second call against the first, outputs pre-filled with NaN, the
status word, the limits on both sides, the composition with the cosine and the prototypical head against the float64 restatement of
the whole chain, and two training steps of MetaBaseline(adapt="feat")."""
import ctypes

import numpy as np
import pytest
import torch

from cos_proto_ref import cos_proto_ref
from euclid_proto_ref import euclid_proto_ref
from feat_adapt_cases import CASES, LEFT_OUT, MARGIN, MISSING, make_case, make_compose
from feat_adapt_ref import GRAD_NAMES, ST_CLASS_MISSING, ST_LABEL_RANGE, feat_adapt_bwd_ref, feat_adapt_fwd_ref, feat_adapt_ref, rel_to_max

pytestmark = pytest.mark.gpu
TOL = 1e-4
EINVAL, ENOTSUP = -1, -4

_REFS = {}


def _case(name):
    """(case, float64 reference) computed once and shared."""
    if name not in _REFS:
        c = make_case(name)
        _REFS[name] = (c, feat_adapt_ref(c["feats_s"], c["y_s"], c["w"], c["N"], c["dprotos"]))
    return _REFS[name]


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


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev, dtype=torch.float32)


def _run(dev, ws, c, keep_tape=True):
    """The two entries through the C ABI with every output pre-filled with NaN: dict(protos, tape, dfeats_s, dwqkv, dwo, dbo, dgamma,
    dbeta) of GPU tensors (the gradients only with keep_tape)."""
    from fumi_amd import hip
    L, st = hip.lib(), hip._stream(dev)
    B, S, N, F = c["B"], c["S"], c["N"], c["F"]
    xs, ys, dpr = _gpu(dev, c["feats_s"], c["y_s"], c["dprotos"])
    w = _gpu(dev, *c["w"])
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    out = dict(protos=_nan(dev, B, N, F), tape=_nan(dev, int(L.fumi_hip_feat_adapt_tape_floats(B, N, F))) if keep_tape else None)
    rc = L.fumi_hip_feat_adapt_fwd(ws.handle, st, B, S, N, F, p(xs), p(ys), *(p(t) for t in w), p(out["protos"]), p(out["tape"]))
    assert rc == 0, rc
    if keep_tape:
        out.update(dfeats_s=_nan(dev, B, S, F), dwqkv=_nan(dev, 3 * F, F), dwo=_nan(dev, F, F), dbo=_nan(dev, F), dgamma=_nan(dev, F),
                   dbeta=_nan(dev, F))
        rc = L.fumi_hip_feat_adapt_bwd(ws.handle, st, B, S, N, F, p(xs), p(ys), *(p(t) for t in w), p(out["tape"]), p(dpr),
                                       *(p(out[k]) for k in ("dfeats_s", "dwqkv", "dwo", "dbo", "dgamma", "dbeta")))
        assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def _split(got, F):
    """The tensors of a run under the reference's names (dWqkv as its three blocks), on the host."""
    h = {k: v.cpu().numpy() for k, v in got.items() if v is not None and k != "tape"}
    if "dwqkv" in h:
        q = h.pop("dwqkv")
        h.update(dwq=q[:F], dwk=q[F:2 * F], dwv=q[2 * F:])
    return h


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_against_float64(name, dev, ws):
    c, ref = _case(name)
    ws.read_status()
    got = _run(dev, ws, c)
    status = ws.read_status()
    h = _split(got, c["F"])
    errs = {}
    for k in ("protos",) + GRAD_NAMES:
        assert np.isfinite(h[k]).all(), (name, k)                                  # the NaN guard: everything was written
        errs[k] = rel_to_max(h[k], ref[k])
        print(f"{name} {k}: rel-to-max error {errs[k]:.3e}")
    assert status == ref["status"], (name, status)
    bad = {k: e for k, e in errs.items() if not e <= TOL}
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", ["n5_f96_unit", "n17_f96_offset", "n64_f640_unit", "n5_f640_saturated"])
def test_forward_form_and_a_second_call_give_the_same_bits(name, dev, ws):
    c, _ = _case(name)
    first, second, fwd = _run(dev, ws, c), _run(dev, ws, c), _run(dev, ws, c, keep_tape=False)
    assert torch.equal(fwd["protos"], first["protos"]), "forward form against taped form"
    for k, v in first.items():
        assert torch.equal(v.view(torch.int32), second[k].view(torch.int32)), k    # bits: the tape's padding floats are never written


def test_status_word_and_the_rows_left_out(dev, ws):
    c, ref = _case("n5_f96_label_range")
    ws.read_status()
    got = _run(dev, ws, c)
    assert ws.read_status() == ST_LABEL_RANGE
    dfs = got["dfeats_s"].cpu().numpy()
    left = [(b, int(np.nonzero((c["y_s"][b] < 0) | (c["y_s"][b] >= c["N"]))[0][0])) for b in LEFT_OUT]
    for b, s in left:
        assert not dfs[b, s].any(), (b, s)                                         # a zero gradient for the row left out
    assert np.count_nonzero(np.abs(dfs).sum(-1) == 0) == len(left)
    c, ref = _case("n5_f96_class_missing")
    got = _run(dev, ws, c)
    assert ws.read_status() == ST_CLASS_MISSING
    tape_p = got["tape"][:c["B"] * c["N"] * c["F"]].view(c["B"], c["N"], c["F"])
    assert not bool(tape_p[MISSING[0], MISSING[1]].any())                          # P_n = 0 ...
    assert rel_to_max(got["protos"].cpu().numpy()[MISSING[0], MISSING[1]], ref["protos"][MISSING[0], MISSING[1]]) <= TOL   # ... and still adapted
    c, _ = _case("n5_f96_unit")
    _run(dev, ws, c)
    assert ws.read_status() == 0


def test_limits_on_both_sides_and_null_pointers(dev, ws):
    """Inside each limit the call succeeds; outside it returns FUMI_ENOTSUP, with a NULL required pointer FUMI_EINVAL, and writes
    nothing (the outputs keep their NaN fill: nothing was launched)."""
    from fumi_amd import hip
    L, st = hip.lib(), hip._stream(dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(B, S, N, F, null=None, bwd=False, alloc=None):
        aB, aS, aN, aF = alloc or (B, S, N, F)
        xs = torch.randn(aB, aS, aF, device=dev)
        ys = (torch.arange(aS, device=dev) % aN).repeat(aB, 1).contiguous()
        w = [torch.randn(3 * aF, aF, device=dev) / aF ** 0.5, torch.randn(aF, aF, device=dev) / aF ** 0.5, torch.zeros(aF, device=dev),
             torch.ones(aF, device=dev), torch.zeros(aF, device=dev)]
        protos = _nan(dev, aB, aN, aF)
        tape = _nan(dev, max(int(L.fumi_hip_feat_adapt_tape_floats(aB, aN, aF)), 1))
        args = [xs, ys, *w, protos, tape]
        if null is not None and not bwd:
            args[null] = None
        rc = L.fumi_hip_feat_adapt_fwd(ws.handle, st, B, S, N, F, *(p(t) for t in args))
        outs = [protos]
        if bwd:
            grads = [_nan(dev, aB, aS, aF), _nan(dev, 3 * aF, aF), _nan(dev, aF, aF), _nan(dev, aF), _nan(dev, aF), _nan(dev, aF)]
            args = [xs, ys, *w, tape, torch.randn(aB, aN, aF, device=dev), *grads]
            if null is not None:
                args[null] = None
            rc = L.fumi_hip_feat_adapt_bwd(ws.handle, st, B, S, N, F, *(p(t) for t in args))
            outs = grads
        torch.cuda.synchronize()
        return rc, outs

    untouched = lambda outs: all(bool(torch.isnan(o).all()) for o in outs)
    small = (1, 4, 2, 32)
    # the inner side of every limit: B = 1, S = 1 and 1024, N = 2 and 64, B N = 65536, F = 32 and 2048
    for ok in (small, (1, 1, 2, 32), (1, 1024, 2, 32), (1, 64, 64, 32), (1024, 64, 64, 32), (1, 4, 2, 2048)):
        for bwd in (False, True):
            rc, outs = call(*ok, bwd=bwd)
            assert rc == 0 and all(bool(torch.isfinite(o).all()) for o in outs), (ok, bwd, rc)
        assert ws.read_status() == (ST_CLASS_MISSING if ok[1] < ok[2] else 0), ok    # one support row cannot fill two classes
    outside = [(0, 4, 2, 32), (1, 0, 2, 32), (1, 1025, 2, 32), (1, 4, 1, 32), (1, 65, 65, 32), (1025, 64, 64, 32), (1, 4, 2, 0),
               (1, 4, 2, 48), (1, 4, 2, 2080)]
    for dims in outside:                                                           # refused from the dimensions alone: small buffers do
        for bwd in (False, True):
            rc, outs = call(*dims, bwd=bwd, alloc=small)
            assert rc == ENOTSUP and untouched(outs), (dims, bwd, rc)
    assert L.fumi_hip_feat_adapt_tape_floats(1, 65, 32) == 0 and L.fumi_hip_feat_adapt_tape_floats(1, 5, 48) == 0
    for null in range(8):                                                          # every pointer of the forward but the tape
        rc, outs = call(*small, null=null)
        assert rc == EINVAL and untouched(outs), null
    for null in range(15):                                                         # every pointer of the backward
        rc, outs = call(*small, null=null, bwd=True)
        assert rc == EINVAL and untouched([o for o in outs if o is not None]), null
    assert L.fumi_hip_feat_adapt_fwd(None, st, *small, *([None] * 9)) == EINVAL
    assert ws.read_status() == 0


@pytest.mark.parametrize("head", ["cosine", "proto"])
def test_composition_with_the_heads_against_the_float64_chain(head, dev, ws):
    """feat_adapt_fwd, the head on (P', arange), feat_adapt_bwd: loss and every gradient against the float64 restatement of the whole
    chain, built from cos_proto_ref / euclid_proto_ref as they are."""
    from fumi_amd import hip
    c = make_compose()
    N, gs = c["N"], 0.5
    B = c["feats_s"].shape[0]
    scale = 10.0 if head == "cosine" else 0.05
    y_p = np.tile(np.arange(N), (B, 1))
    fw = feat_adapt_fwd_ref(c["feats_s"], c["y_s"], *c["w"], N)
    href = (cos_proto_ref if head == "cosine" else euclid_proto_ref)(fw["protos"], y_p, c["feats_q"], c["y_q"], scale, N, gs)
    ref = feat_adapt_bwd_ref(fw, href["dfeats_s"])
    xs, ys, xq, yq, yp = _gpu(dev, c["feats_s"], c["y_s"], c["feats_q"], c["y_q"], y_p)
    w = _gpu(dev, *c["w"])
    sc = torch.tensor([scale], device=dev)
    protos, tape = hip.feat_adapt_fwd(ws, xs, ys, w, n_way=N, keep_tape=True)
    step = hip.cos_proto_step if head == "cosine" else hip.euclid_proto_step
    out = step(ws, protos, yp, xq, yq, sc, need_grad=True, grad_scale=gs, n_way=N)
    dfs, g_w = hip.feat_adapt_bwd(ws, xs, ys, w, tape, out["dfeats_s"], n_way=N)
    assert ws.read_status() == 0
    F = c["feats_s"].shape[-1]
    got = dict(protos=protos, dfeats_s=dfs, dfeats_q=out["dfeats_q"], dwq=g_w[0][:F], dwk=g_w[0][F:2 * F], dwv=g_w[0][2 * F:], dwo=g_w[1],
               dbo=g_w[2], dgamma=g_w[3], dbeta=g_w[4])
    want = dict(ref, protos=fw["protos"], dfeats_q=href["dfeats_q"])
    e = abs(float(out["loss"]) - href["loss"]) / max(abs(href["loss"]), 1e-5)
    print(f"compose {head} loss: relative error {e:.3e}")
    errs = {"loss": e}
    for k, v in got.items():
        errs[k] = rel_to_max(v.cpu().numpy(), want[k])
        print(f"compose {head} {k}: rel-to-max error {errs[k]:.3e}")
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    safe = href["margin"] > MARGIN
    assert np.array_equal(out["preds"].cpu().numpy()[safe], href["preds"][safe])


# ---- the model ------------------------------------------------------------------------------------------------------------------------
MB, MN, MK, MQ, SIZE = 2, 5, 2, 3, 32


def _batch(seed, dev):
    g = torch.Generator().manual_seed(seed)
    y_s = torch.stack([(torch.arange(MN * MK) % MN)[torch.randperm(MN * MK, generator=g)] for _ in range(MB)])
    y_q = torch.stack([(torch.arange(MN * MQ) % MN)[torch.randperm(MN * MQ, generator=g)] for _ in range(MB)])
    x_s, x_q = torch.randn(MB, MN * MK, 3, SIZE, SIZE, generator=g), torch.randn(MB, MN * MQ, 3, SIZE, SIZE, generator=g)
    return {"train": ((None, None, x_s.to(dev)), y_s.to(dev)), "test": ((None, None, x_q.to(dev)), y_q.to(dev))}


def _model(dev, adapt, head="cosine"):
    from fumi_amd.models.metabaseline import MetaBaseline
    torch.manual_seed(23)
    return MetaBaseline("conv4", image_size=SIZE, image_channels=3, num_ways=MN, head=head, proto_scale=0.05, adapt=adapt).to(dev)


@pytest.mark.parametrize("head", ["cosine", "proto"])
def test_model_trains_the_new_parameters(head, dev):
    from fumi_amd import hip
    from fumi_amd.optim import Adam
    model = _model(dev, "feat", head)
    assert model.feat.wqkv.shape == (3 * 256, 256)                                 # Conv4 on 32 x 32 images: 64 * 2 * 2 features
    opt = Adam(params=model.parameters(), lr=1e-3)
    names = ["feat." + n for n, _ in model.feat.named_parameters()]
    assert names == ["feat.wqkv", "feat.wo", "feat.bo", "feat.ln_weight", "feat.ln_bias"]
    for step in range(2):
        before = [p.detach().clone() for p in model.feat.parameters()]
        loss, acc = model.evaluate(_batch(40 + step, dev), opt, None, dev, task="train")
        assert np.isfinite(float(loss)) and 0.0 <= float(acc) <= 1.0
        for n, p, b in zip(names, model.feat.parameters(), before):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, n
            assert not torch.equal(p.detach(), b), n                               # moved by the fused optimizer
    with torch.no_grad():
        val = model.few_shot(_batch(50, dev), dev)
    assert bool(torch.isfinite(val).all())
    assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0


def test_adapt_none_is_the_unchanged_route(dev):
    """adapt="none": the state_dict keys, the engine calls and the bits of the route as it was -- two runs of it in one process, the
    default construction and adapt="none", give the same loss bits and the same gradients on the same batch."""
    runs = []
    for kw in (None, "none"):
        from fumi_amd.models.metabaseline import MetaBaseline
        torch.manual_seed(23)
        model = (MetaBaseline("conv4", image_size=SIZE, image_channels=3, num_ways=MN) if kw is None else
                 MetaBaseline("conv4", image_size=SIZE, image_channels=3, num_ways=MN, adapt=kw)).to(dev)
        assert not any(k.startswith("feat.") for k in model.state_dict())
        model.evaluate(_batch(44, dev), None, None, dev, task="train")
        runs.append(model._flat.flat.clone())
    assert torch.equal(runs[0], runs[1]) and bool(torch.isfinite(runs[0]).all())
