"""CPU suite of the cosine nearest-centroid head and --model metabaseline: the float64 restatement
tests/cos_proto_ref.py against torch.autograd, the margins of the GPU parity inputs, the flags and refusals, and the state_dict
contract of MetaBaseline (host-running oracle engine, as tests/test_pretrain_cpu.py does)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cos_proto_ref import ST_CLASS_MISSING, ST_LABEL_RANGE, case_inputs, cos_proto_ref
from oracle_engine import OracleEngine

# the shapes (B, S, Qn, N, F) of tests/test_cos_proto_gpu.py
GPU_SHAPES = [(1, 2, 1, 2, 32), (2, 7, 33, 3, 96), (2, 100, 130, 20, 640), (1, 25, 17, 5, 1600), (1, 64, 18, 64, 64),
              (3, 10, 16, 5, 2048)]


class CosOracleEngine(OracleEngine):
    """OracleEngine plus the two ops Pretrain.few_shot and MetaBaseline need on the host; counts the calls of each."""

    def __init__(self):
        self.calls = dict(proto_reduce=0, cos_proto_step=0)

    def proto_reduce(self, x, y, n_way):
        self.calls["proto_reduce"] += 1
        onehot = F.one_hot(y, n_way).to(x.dtype)                                   # [B, S, N]
        return torch.einsum("bsn,bsf->bnf", onehot, x) / onehot.sum(1).clamp(min=1)[:, :, None]

    def cos_proto_step(self, feats_s, y_s, feats_q, y_q, tau, need_grad=True, grad_scale=1.0, want_logits=False, dfeats_s=None,
                       dfeats_q=None, dtau=None, n_way=None):
        self.calls["cos_proto_step"] += 1
        r = cos_proto_ref(feats_s.numpy(), y_s.numpy(), feats_q.numpy(), y_q.numpy(), tau.numpy(), n_way, grad_scale)
        f32 = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32))
        out = dict(loss=f32(r["loss"]).reshape(1), correct=f32(r["correct"]).reshape(1), preds=torch.as_tensor(r["preds"]),
                   logits=f32(r["logits"]) if want_logits else None, dfeats_s=None, dfeats_q=None, dtau=None)
        if need_grad:
            out.update(dfeats_s=f32(r["dfeats_s"]), dfeats_q=f32(r["dfeats_q"]), dtau=f32(r["dtau"]).reshape(1))
            if dtau is not None:
                dtau.copy_(out["dtau"]); out["dtau"] = dtau
        return out


@pytest.fixture()
def cos_engine():
    from fumi_amd import engine
    eng = CosOracleEngine()
    old = engine.set_engine(eng)
    yield eng
    engine.set_engine(old)


# ---- the restatement of the head ------------------------------------------------------------------------------------------------
def _torch_head(f_s, y_s, f_q, y_q, tau, N, gs):
    """The head in torch float64 ops with autograd; rows whose label is out of range are masked the way the kernel drops them."""
    xs = torch.tensor(f_s, dtype=torch.float64, requires_grad=True)
    xq = torch.tensor(f_q, dtype=torch.float64, requires_grad=True)
    t = torch.tensor([tau], dtype=torch.float64, requires_grad=True)
    ys, yq = torch.as_tensor(y_s), torch.as_tensor(y_q)
    ok_s, ok_q = (ys >= 0) & (ys < N), (yq >= 0) & (yq < N)
    onehot = F.one_hot(ys.clamp(0, N - 1), N).to(torch.float64) * ok_s[..., None]
    protos = torch.bmm(onehot.transpose(1, 2), xs) / onehot.sum(1).clamp(min=1)[:, :, None]
    z = t * torch.bmm(F.normalize(xq, dim=-1), F.normalize(protos, dim=-1).transpose(1, 2))
    nll = F.cross_entropy(z.reshape(-1, N), yq.clamp(0, N - 1).reshape(-1), reduction="none")
    loss = (nll * ok_q.reshape(-1)).sum() / yq.numel()
    return xs, xq, t, z, loss, gs * loss


def _unequal_case(seed=5, B=2, S=9, Qn=6, N=4, Fd=32):
    rs = np.random.RandomState(seed)
    f_s, f_q = rs.standard_normal((B, S, Fd)), rs.standard_normal((B, Qn, Fd))
    y_s = np.tile(np.arange(S) % N, (B, 1)); y_s[:, -1] = 0                      # class 0 has three rows, classes 1..3 two
    y_q = rs.randint(0, N, (B, Qn))
    return f_s, y_s, f_q, y_q, N


def _compare(f_s, y_s, f_q, y_q, N, status, tau=7.5, gs=0.25, grads=True):
    ref = cos_proto_ref(f_s, y_s, f_q, y_q, tau, N, gs)
    xs, xq, t, z, loss, obj = _torch_head(f_s, y_s, f_q, y_q, tau, N, gs)
    assert ref["status"] == status
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-12
    assert np.abs(ref["logits"] - z.detach().numpy()).max() <= 1e-12
    if grads:
        dxs, dxq, dt = torch.autograd.grad(obj, [xs, xq, t])
        for got, want in ((ref["dfeats_s"], dxs), (ref["dfeats_q"], dxq), (ref["dtau"], dt)):
            assert np.abs(got - want.numpy()).max() <= 1e-12
    return ref


def test_restatement_equals_autograd_with_unequal_class_counts():
    f_s, y_s, f_q, y_q, N = _unequal_case()
    ref = _compare(f_s, y_s, f_q, y_q, N, 0)
    z = ref["logits"]
    assert np.array_equal(ref["preds"], z.argmax(-1)) and ref["correct"] == float((z.argmax(-1) == y_q).sum())


def test_restatement_equals_autograd_with_labels_out_of_range():
    f_s, y_s, f_q, y_q, N = _unequal_case(seed=6)
    y_q[1, 2] = N
    y_s[0, 3] = -1
    ref = _compare(f_s, y_s, f_q, y_q, N, ST_LABEL_RANGE)
    assert not ref["dfeats_q"][1, 2].any() and not ref["dfeats_s"][0, 3].any()


def test_restatement_equals_autograd_with_a_class_without_support():
    f_s, y_s, f_q, y_q, N = _unequal_case(seed=7)
    y_s[0][y_s[0] == 2] = 1                                                        # episode 0 has no row of class 2
    ref = _compare(f_s, y_s, f_q, y_q, N, ST_CLASS_MISSING)
    assert not ref["protos"][0, 2].any() and not ref["logits"][0, :, 2].any()


def test_restatement_of_a_zero_query_row_has_zero_logits_and_a_finite_loss():
    f_s, y_s, f_q, y_q, N = _unequal_case(seed=8)
    f_q[0, 1] = 0.0
    ref = _compare(f_s, y_s, f_q, y_q, N, 0, grads=False)
    assert not ref["logits"][0, 1].any() and np.isfinite(ref["loss"])


@pytest.mark.parametrize("B,S,Qn,N,Fd", GPU_SHAPES)
def test_margins_of_the_gpu_parity_inputs_leave_no_query_row_aside(B, S, Qn, N, Fd):
    f_s, y_s, f_q, y_q = case_inputs(B, S, Qn, N, Fd)
    ref = cos_proto_ref(f_s, y_s, f_q, y_q, 10.0, N, 0.25)
    print(f"({B},{S},{Qn},{N},{Fd}): smallest top-two margin {ref['margin'].min():.4g}")
    assert ref["status"] == 0 and ref["margin"].min() > 1e-5
    if S > N:
        counts = np.stack([(y_s == n).sum(1) for n in range(N)], 1)
        assert (counts.max(1) > counts.min(1)).all()                               # unequal class counts


# ---- flags ----------------------------------------------------------------------------------------------------------------------
def test_metric_flags_parse_with_their_defaults_and_sit_before_the_mix_flags():
    from fumi_amd.utils import utils
    d = utils.parser().parse_args([])
    assert d.metric_temp == 10.0 and d.pretrain_metric == "euclidean"
    a = utils.parser().parse_args(["--model", "metabaseline", "--metric_temp", "12.5", "--pretrain_metric", "cosine"])
    assert (a.model, a.metric_temp, a.pretrain_metric) == ("metabaseline", 12.5, "cosine")
    with pytest.raises(SystemExit):
        utils.parser().parse_args(["--pretrain_metric", "manhattan"])
    assert [f for f, _ in utils._METRIC_FLAGS] == ["--metric_temp", "--pretrain_metric"]
    flags = [act.option_strings[0] for act in utils.parser()._actions if act.option_strings and act.dest != "help"]
    n_e, n_m, n_x = len(utils._ENGINE_FLAGS), len(utils._METRIC_FLAGS), len(utils._PRETRAIN_MIX_FLAGS)
    assert flags[-n_x:] == [f for f, _ in utils._PRETRAIN_MIX_FLAGS]
    assert flags[-n_x - n_m:-n_x] == [f for f, _ in utils._METRIC_FLAGS]
    assert flags[-n_x - n_m - n_e:-n_x - n_m] == [f for f, _ in utils._ENGINE_FLAGS]


def test_check_supported_and_get_dataset_refuse_what_metabaseline_cannot_run(cos_engine, monkeypatch):
    from fumi_amd import main as cli
    base = ["--model", "metabaseline", "--disable_cuda", "--dataset", "synthetic-resident"]
    cli.check_supported(cli.parse_args(base + ["--im_encoder", "conv4"]))
    cli.check_supported(cli.parse_args(base + ["--im_encoder", "resnet12", "--encoder_checkpoint", "x.pth.tar"]))
    assert "metabaseline" in cli._FAMILIES and cli._TEST_METRICS["metabaseline"] == ("loss", "acc")
    with pytest.raises(ValueError, match="--im_encoder"):
        cli.check_supported(cli.parse_args(base))                                              # precomputed embeddings
    with pytest.raises(ValueError, match="--metric_temp"):
        cli.check_supported(cli.parse_args(base + ["--im_encoder", "conv4", "--metric_temp", "0"]))
    with pytest.raises(ValueError, match="--metric_temp"):
        cli.check_supported(cli.parse_args(base + ["--im_encoder", "conv4", "--metric_temp", "-1"]))
    with pytest.raises(ValueError, match="--pretrain_metric"):
        cli.check_supported(cli.parse_args(base + ["--im_encoder", "conv4", "--pretrain_metric", "cosine"]))
    with pytest.raises(ValueError, match="--model pretrain"):                                  # the mix flags stay with pretrain
        cli.check_supported(cli.parse_args(base + ["--im_encoder", "conv4", "--label_smoothing", "0.1"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        cli.check_supported(cli.parse_args(base + ["--im_encoder", "conv4"]))
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="pixel table"):
        cli.get_dataset(cli.parse_args(["--model", "metabaseline", "--disable_cuda", "--dataset", "synthetic", "--im_encoder", "conv4"]))
    # --pretrain_metric belongs to --model pretrain, where both values pass
    pre = ["--model", "pretrain", "--disable_cuda", "--dataset", "synthetic-resident", "--im_encoder", "conv4"]
    cli.check_supported(cli.parse_args(pre + ["--pretrain_metric", "cosine"]))
    cli.check_supported(cli.parse_args(pre + ["--pretrain_metric", "euclidean"]))
    with pytest.raises(ValueError, match="--metric_temp"):
        cli.check_supported(cli.parse_args(pre + ["--pretrain_metric", "cosine", "--metric_temp", "0"]))
    with pytest.raises(ValueError, match="--pretrain_metric"):
        cli.check_supported(cli.parse_args(["--model", "am3", "--disable_cuda", "--dropout", "0", "--pretrain_metric", "cosine"]))


def _episodic_batch(seed, B=2, N=3, K=2, Q=2, size=16):
    g = torch.Generator().manual_seed(seed)
    y_s = (torch.arange(N * K) % N).repeat(B, 1)
    y_q = (torch.arange(N * Q) % N).repeat(B, 1)
    x_s, x_q = torch.randn(B, N * K, 3, size, size, generator=g), torch.randn(B, N * Q, 3, size, size, generator=g)
    return {"train": ((None, None, x_s), y_s), "test": ((None, None, x_q), y_q)}


def test_pretrain_metric_euclidean_keeps_few_shot_on_its_present_path_and_cosine_is_one_head_call(cos_engine):
    from fumi_amd.models.pretrain import Pretrain
    torch.manual_seed(3)
    batch = _episodic_batch(11)
    kw = dict(image_size=16, image_channels=3, n_classes=6, num_ways=3)
    model = Pretrain("conv4", **kw)
    assert model.metric == "euclidean"
    got = model.few_shot(batch, torch.device("cpu"))
    assert cos_engine.calls == dict(proto_reduce=1, cos_proto_step=0)
    # the expression few_shot has evaluated so far
    theta = [p.detach() for p in model.conv.theta()]
    (_, _, x_s), y_s = batch["train"]
    (_, _, x_q), y_q = batch["test"]
    f_s, f_q = cos_engine.conv4_encode(x_s, x_q, theta)
    protos = cos_engine.proto_reduce(f_s, y_s, 3)
    d2 = ((f_q[:, :, None, :] - protos[:, None, :, :]) ** 2).sum(-1)
    want = torch.stack((F.cross_entropy(-d2.reshape(-1, 3), y_q.reshape(-1)), (d2.argmin(-1) == y_q).float().mean()))
    assert torch.equal(got, want)
    # cosine: one forward call of the head at the fixed temperature
    cos_engine.calls.update(proto_reduce=0, cos_proto_step=0)
    cosine = Pretrain("conv4", metric="cosine", metric_temp=8.0, **kw)
    cosine.load_state_dict(model.state_dict())
    got = cosine.few_shot(batch, torch.device("cpu"))
    assert cos_engine.calls == dict(proto_reduce=0, cos_proto_step=1)
    ref = cos_proto_ref(f_s.numpy(), y_s.numpy(), f_q.numpy(), y_q.numpy(), 8.0, 3)
    assert abs(float(got[0]) - ref["loss"]) <= 1e-6 and abs(float(got[1]) - ref["correct"] / y_q.numel()) <= 1e-7
    with pytest.raises(ValueError):
        Pretrain("conv4", metric="cosine", metric_temp=0.0, **kw)
    with pytest.raises(ValueError):
        Pretrain("conv4", metric="manhattan", **kw)


# ---- MetaBaseline ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("im_encoder", ["conv4", "resnet12"])
def test_metabaseline_state_dict_is_temp_plus_the_backbone_of_pretrain(im_encoder, cos_engine):
    from fumi_amd.models.metabaseline import MetaBaseline
    from fumi_amd.models.pretrain import Pretrain
    from fumi_amd.utils import utils
    torch.manual_seed(5)
    pre = Pretrain(im_encoder, image_size=16, image_channels=3, n_classes=6)
    with torch.no_grad():
        for p in pre.parameters():
            p.add_(torch.randn_like(p))
    model = MetaBaseline(im_encoder, image_size=16, image_channels=3, num_ways=3, init_temp=12.0)
    sd, mine = pre.state_dict(), model.state_dict()
    assert set(mine) == {"temp"} | {k for k in sd if k.startswith("conv.")}
    assert model.backbone_module() is model.conv and tuple(model.temp.shape) == (1,) and float(model.temp) == 12.0
    model._pcache = "stale"
    names = utils.load_backbone_state(model, sd)
    assert model._pcache is None and names == sorted(k for k in sd if k.startswith("conv."))
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]) if k != "temp" else float(v) == 12.0, k
    with pytest.raises(ValueError):
        MetaBaseline(im_encoder, image_size=16, init_temp=0.0)


def test_metabaseline_step_on_the_host_engine_attaches_gradients_and_returns_the_head_loss(cos_engine):
    """The plumbing of evaluate() on the host: encode -> cos_proto_step -> encode_bwd, one flat gradient buffer [temp | conv.* | loss,
    acc], and the forward form for validation."""
    from fumi_amd.models.metabaseline import MetaBaseline
    torch.manual_seed(9)
    model = MetaBaseline("conv4", image_size=16, image_channels=3, num_ways=3)
    batch = _episodic_batch(13)
    loss, acc = model.evaluate(batch, None, None, "cpu", task="train")
    theta = [p.detach() for p in model.conv.theta()]
    f_s, f_q = cos_engine.conv4_encode(batch["train"][0][2], batch["test"][0][2], theta)
    ref = cos_proto_ref(f_s.numpy(), batch["train"][1].numpy(), f_q.numpy(), batch["test"][1].numpy(), 10.0, 3)
    assert abs(float(loss) - ref["loss"]) <= 1e-6 and abs(float(acc) - ref["correct"] / 12) <= 1e-7
    assert abs(float(model.temp.grad) - ref["dtau"]) <= 1e-6 * max(1.0, abs(ref["dtau"]))
    assert model.temp.grad.data_ptr() == model._flat.flat.data_ptr()
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    v_loss, v_acc = model.evaluate(batch, None, None, "cpu", task="val")
    assert abs(float(v_loss) - ref["loss"]) <= 1e-6 and abs(float(v_acc) - ref["correct"] / 12) <= 1e-7
    assert not model.training
