"""CPU suite of supervised backbone pre-training (--model pretrain): the float64 restatement of the head
against autograd, the flags, the permutation schedule of the supervised batch source, the --encoder_checkpoint helper and the
refusals of check_supported (host-running oracle engine, as tests/test_host_logic.py does)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cls_head_ref import ST_LABEL_RANGE, cls_head_ref
from helpers import GOLDEN
from oracle_engine import OracleEngine


@pytest.fixture()
def oracle_engine():
    from fumi_amd import engine
    old = engine.set_engine(OracleEngine())
    yield
    engine.set_engine(old)


# ---- the restatement of the head ------------------------------------------------------------------------------------------------
def test_head_restatement_equals_autograd_in_float64():
    M, Fd, C, gs = 7, 32, 5, 0.25
    g = torch.Generator().manual_seed(7)
    x = torch.randn(M, Fd, generator=g, dtype=torch.float64).requires_grad_(True)
    W = torch.randn(C, Fd, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    y = torch.randint(0, C, (M,), generator=g)
    z = x @ W.T + b
    loss = F.cross_entropy(z, y)
    dx, dW, db = torch.autograd.grad(gs * loss, [x, W, b])
    ref = cls_head_ref(x.detach().numpy(), y.numpy(), W.detach().numpy(), b.detach().numpy(), gs)
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-12 and ref["status"] == 0
    assert np.array_equal(ref["preds"], z.argmax(1).numpy()) and ref["correct"] == float((z.argmax(1) == y).sum())
    for got, want in ((ref["dfeats"], dx), (ref["gW"], dW), (ref["gb"], db)):
        assert np.abs(got - want.numpy()).max() <= 1e-12


def test_head_restatement_drops_a_row_whose_label_is_out_of_range():
    M, Fd, C = 7, 32, 5
    rs = np.random.RandomState(3)
    x, W, b = rs.standard_normal((M, Fd)), rs.standard_normal((C, Fd)), rs.standard_normal(C)
    y = rs.randint(0, C, M)
    bad = y.copy(); bad[2] = C
    keep = np.arange(M) != 2
    full, sub = cls_head_ref(x, bad, W, b), cls_head_ref(x[keep], y[keep], W, b)
    assert full["status"] == ST_LABEL_RANGE and sub["status"] == 0
    assert abs(full["loss"] * M - sub["loss"] * (M - 1)) <= 1e-12            # the row adds nothing, the divisor stays M
    assert not full["dfeats"][2].any() and np.abs(full["gW"] * M - sub["gW"] * (M - 1)).max() <= 1e-12
    assert full["correct"] == sub["correct"]


# ---- flags ----------------------------------------------------------------------------------------------------------------------
def test_pretrain_flags_parse_and_every_existing_flag_is_unchanged():
    from fumi_amd.utils import utils
    d = utils.parser().parse_args([])
    assert d.pretrain_batch == 128 and d.pretrain_bn_group == 64 and d.encoder_checkpoint is None
    a = utils.parser().parse_args(["--model", "pretrain", "--pretrain_batch", "16", "--pretrain_bn_group", "4", "--encoder_checkpoint", "x.pth.tar"])
    assert (a.model, a.pretrain_batch, a.pretrain_bn_group, a.encoder_checkpoint) == ("pretrain", 16, 4, "x.pth.tar")
    assert [f for f, _ in utils._ENGINE_FLAGS][-3:] == ["--pretrain_batch", "--pretrain_bn_group", "--encoder_checkpoint"]
    # the reference's flags, as tests/test_host_logic.py::test_every_reference_flag_same_name_default_type compares them
    ref = json.load(open(os.path.join(GOLDEN, "surface.json")))["flags"]
    mine = {act.dest: act for act in utils.parser()._actions if act.option_strings and act.dest != "help"}
    assert len(ref) == 50
    for dest, r in ref.items():
        act = mine[dest]
        assert act.option_strings[0] == r["flag"] and act.default == r["default"], dest
        assert (act.type.__name__ if act.type else None) == r["type"] and act.nargs == r["nargs"], dest
        assert (list(act.choices) if act.choices else None) == r["choices"], dest
        assert (type(act).__name__ == "_StoreTrueAction") == r["store_true"], dest
    # this engine's earlier additive flags: names, order and defaults
    earlier = [("--synthetic_classes", 64), ("--synthetic_vocab", 2000), ("--synthetic_seq_len", 32), ("--image_size", 84),
               ("--image_channels", 3), ("--augment_pad", 8), ("--augment_jitter", 0.4), ("--image_crop_frac", 0.875),
               ("--augment_scale", None), ("--augment_ratio", 4.0 / 3.0), ("--synthetic_table_size", None), ("--image_mean", None),
               ("--image_std", None), ("--max_grad_norm", None)]
    assert [(f, kw.get("default")) for f, kw in utils._ENGINE_FLAGS[:len(earlier)]] == earlier


# ---- the permutation schedule of SupervisedPixelBatches ---------------------------------------------------------------------------
def test_supervised_schedule_covers_every_image_once_per_epoch_and_is_reproducible():
    from fumi_amd.dataset.supervised_pixels import batch_indices, epoch_permutation
    n, batch, seed = 53, 8, 11
    per_epoch = n // batch                                     # 6 whole batches; the 5 images of the short tail are dropped
    for epoch in range(3):
        idx = torch.cat([batch_indices(n, batch, seed, epoch * per_epoch + k) for k in range(per_epoch)])
        perm = epoch_permutation(n, seed, epoch)
        assert sorted(perm.tolist()) == list(range(n))                       # a permutation of the table
        assert torch.equal(idx, perm[:per_epoch * batch])                    # whole batches only, every index at most once
        assert len(set(idx.tolist())) == per_epoch * batch
    assert not torch.equal(epoch_permutation(n, seed, 0), epoch_permutation(n, seed, 1))
    assert not torch.equal(epoch_permutation(n, seed, 0), epoch_permutation(n, seed + 1, 0))
    for step in (0, 5, 6, 17):
        assert torch.equal(batch_indices(n, batch, seed, step), batch_indices(n, batch, seed, step))
        assert batch_indices(n, batch, seed, step).dtype == torch.int64 and batch_indices(n, batch, seed, step).shape == (batch,)
    assert torch.equal(batch_indices(n, batch, seed, per_epoch), epoch_permutation(n, seed, 1)[:batch])
    with pytest.raises(ValueError):
        batch_indices(5, 8, seed, 0)


# ---- --encoder_checkpoint ---------------------------------------------------------------------------------------------------------
def _models(im_encoder, size):
    from fumi_amd.models import am3, fumi, maml
    return [am3.AM3(im_encoder, 0, "BERT", text_emb_dim=8, text_hid_dim=8, prototype_dim=8, image_size=size),
            fumi.FUMI(n_way=3, text_encoder="BERT", text_emb_dim=8, text_hid_dim=8, dropout_rate=0.0, im_encoder=im_encoder, image_size=size),
            maml.PureImageNetwork(n_way=3, im_encoder=im_encoder, image_size=size)]


@pytest.mark.parametrize("im_encoder", ["conv4", "resnet12"])
def test_encoder_checkpoint_helper_copies_the_backbone_only(im_encoder, tmp_path, oracle_engine):
    from fumi_amd.models.pretrain import Pretrain
    from fumi_amd.utils import utils
    torch.manual_seed(5)
    pre = Pretrain(im_encoder, image_size=16, image_channels=3, n_classes=6)
    with torch.no_grad():
        for p in pre.parameters():
            p.add_(torch.randn_like(p))
    sd = pre.state_dict()
    assert {k.split(".")[0] for k in sd} == {"conv", "classifier"}
    path = str(tmp_path / "best.pth.tar")
    torch.save({"batch_idx": 3, "state_dict": sd, "best_loss": 1.0, "optimizer": {}, "args": {}}, path)
    for model in _models(im_encoder, 16):
        before = {k: v.clone() for k, v in model.state_dict().items()}
        bb = model.backbone_module()
        prefix = next(n for n, m in model.named_modules() if m is bb) + "."
        cached = hasattr(model, "_pcache")                                   # (AM3 and FuMI; the MAML model keeps no such cache)
        if cached:
            model._pcache = "stale"
        utils.load_encoder_checkpoint(model, torch.device("cpu"), path)
        assert cached == hasattr(model, "_pcache") and getattr(model, "_pcache", None) is None     # the cached views are dropped
        after = model.state_dict()
        assert len(bb.state_dict()) == len([k for k in sd if k.startswith("conv.")])
        for k, v in after.items():
            if k.startswith(prefix):
                assert torch.equal(v, sd["conv." + k[len(prefix):]]), k
            else:
                assert torch.equal(v, before[k]), k                          # nothing else changes; the classifier is ignored
    # a missing tensor and a mis-shaped one are ValueErrors that name the tensor
    name = "conv.block1.conv.weight" if im_encoder == "conv4" else "conv.block1.conv2.weight"
    model = _models(im_encoder, 16)[0]
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        utils.load_backbone_state(model, {k: v for k, v in sd.items() if k != name})
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        utils.load_backbone_state(model, {**sd, name: sd[name][:, :-1]})
    with pytest.raises(ValueError, match="backbone"):
        from fumi_amd.models import am3
        utils.load_backbone_state(am3.AM3("precomputed", 8, "BERT", text_emb_dim=8), sd)


# ---- check_supported --------------------------------------------------------------------------------------------------------------
def test_check_supported_refuses_what_pretrain_cannot_run(oracle_engine, monkeypatch):
    from fumi_amd import main as cli
    base = ["--model", "pretrain", "--disable_cuda", "--dataset", "synthetic-resident"]
    cli.check_supported(cli.parse_args(base + ["--im_encoder", "conv4"]))
    cli.check_supported(cli.parse_args(base + ["--im_encoder", "resnet12", "--pretrain_batch", "16", "--pretrain_bn_group", "4"]))
    with pytest.raises(ValueError, match="--im_encoder"):
        cli.check_supported(cli.parse_args(base))                                              # precomputed embeddings
    with pytest.raises(ValueError, match="--pretrain_bn_group"):
        cli.check_supported(cli.parse_args(base + ["--im_encoder", "conv4", "--pretrain_batch", "100"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
        cli.check_supported(cli.parse_args(base + ["--im_encoder", "conv4"]))
    monkeypatch.delenv("WORLD_SIZE")
    # --encoder_checkpoint needs a backbone to load into
    with pytest.raises(ValueError, match="--encoder_checkpoint"):
        cli.check_supported(cli.parse_args(["--model", "am3", "--disable_cuda", "--dropout", "0", "--encoder_checkpoint", "x"]))
    cli.check_supported(cli.parse_args(["--model", "am3", "--disable_cuda", "--im_encoder", "conv4", "--encoder_checkpoint", "x"]))
    with pytest.raises(ValueError, match="pixel table"):
        cli.get_dataset(cli.parse_args(["--model", "pretrain", "--disable_cuda", "--dataset", "synthetic", "--im_encoder", "conv4"]))
