"""CPU suite of label smoothing, mixup and CutMix for --model pretrain: the float64 restatement of the soft-target
head against autograd, the host draw ``mix_draw``, the four flags and the refusals of check_supported."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cls_head_ref import ST_LABEL_RANGE, cls_head_ref
from cls_head_soft_ref import cls_head_soft_ref
from oracle_engine import OracleEngine


@pytest.fixture()
def oracle_engine():
    from fumi_amd import engine
    old = engine.set_engine(OracleEngine())
    yield
    engine.set_engine(old)


def _inputs(M=9, Fd=32, C=5, seed=7):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, Fd, generator=g, dtype=torch.float64)
    W = torch.randn(C, Fd, generator=g, dtype=torch.float64)
    b = torch.randn(C, generator=g, dtype=torch.float64)
    y_a = torch.randint(0, C, (M,), generator=g)
    y_b = y_a[torch.randperm(M, generator=g)]
    y_b[:2] = y_a[:2]                                          # rows whose two labels coincide
    assert bool((y_a != y_b).any())
    return x, W, b, y_a, y_b


# ---- the restatement of the soft-target head ------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("lam", [1.0, 0.3])
def test_soft_head_restatement_equals_autograd_in_float64(eps, lam):
    gs = 0.25
    x, W, b, y_a, y_b = _inputs()
    x, W, b = (t.requires_grad_(True) for t in (x, W, b))
    z = x @ W.T + b
    loss = lam * F.cross_entropy(z, y_a, label_smoothing=eps) + (1 - lam) * F.cross_entropy(z, y_b, label_smoothing=eps)
    dx, dW, db = torch.autograd.grad(gs * loss, [x, W, b])
    ref = cls_head_soft_ref(x.detach().numpy(), y_a.numpy(), W.detach().numpy(), b.detach().numpy(), gs, y_b=y_b.numpy(), lam=lam,
                            smoothing=eps)
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-12 and ref["status"] == 0
    assert np.array_equal(ref["preds"], z.argmax(1).numpy()) and ref["correct"] == float((z.argmax(1) == y_a).sum())
    for got, want in ((ref["dfeats"], dx), (ref["gW"], dW), (ref["gb"], db)):
        assert np.abs(got - want.numpy()).max() <= 1e-12


def test_soft_head_restatement_without_smoothing_or_mix_is_the_hard_one():
    x, W, b, y_a, _ = _inputs()
    hard = cls_head_ref(x.numpy(), y_a.numpy(), W.numpy(), b.numpy(), 0.25)
    for y_b in (None, y_a.numpy()):
        soft = cls_head_soft_ref(x.numpy(), y_a.numpy(), W.numpy(), b.numpy(), 0.25, y_b=y_b, lam=1.0, smoothing=0.0)
        assert set(soft) == set(hard)
        for k, v in hard.items():
            assert np.array_equal(np.asarray(soft[k]), np.asarray(v)), k


def test_soft_head_restatement_drops_a_row_whose_second_label_is_out_of_range():
    x, W, b, y_a, y_b = _inputs()
    M, C = x.shape[0], W.shape[0]
    bad = y_b.clone(); bad[4] = C
    keep = np.arange(M) != 4
    a = (x.numpy(), y_a.numpy(), W.numpy(), b.numpy())
    full = cls_head_soft_ref(*a, y_b=bad.numpy(), lam=0.3, smoothing=0.1)
    sub = cls_head_soft_ref(a[0][keep], a[1][keep], a[2], a[3], y_b=y_b.numpy()[keep], lam=0.3, smoothing=0.1)
    assert full["status"] == ST_LABEL_RANGE and sub["status"] == 0
    assert abs(full["loss"] * M - sub["loss"] * (M - 1)) <= 1e-12
    assert not full["dfeats"][4].any() and np.abs(full["gW"] * M - sub["gW"] * (M - 1)).max() <= 1e-12
    assert full["correct"] == sub["correct"]


# ---- mix_draw -------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a[:3] == b[:3] and np.array_equal(a[3], b[3])


def test_mix_draw_is_reproducible_and_its_draws_are_valid():
    from fumi_amd.dataset.supervised_pixels import CUTMIX, MIXUP, mix_draw
    M, H, W = 16, 12, 20
    modes = set()
    for step in range(64):
        d = mix_draw(5, step, M, H, W, 0.4, 1.0, 1.0)
        assert _same(d, mix_draw(5, step, M, H, W, 0.4, 1.0, 1.0))
        mode, lam, box, partner = d
        modes.add(mode)
        assert mode in (MIXUP, CUTMIX) and 0.0 <= lam <= 1.0
        assert partner.dtype == np.int64 and sorted(partner.tolist()) == list(range(M))
        bx0, by0, bx1, by1 = box
        if mode == CUTMIX:
            assert 0 <= bx0 <= bx1 <= W and 0 <= by0 <= by1 <= H
            assert lam == 1.0 - (bx1 - bx0) * (by1 - by0) / float(H * W)
        else:
            assert box == (0, 0, 0, 0)
    assert modes == {MIXUP, CUTMIX}                                                   # both alphas on: both modes within 64 steps
    assert not _same(mix_draw(5, 0, M, H, W, 0.4, 1.0, 1.0), mix_draw(5, 1, M, H, W, 0.4, 1.0, 1.0))
    assert not _same(mix_draw(5, 0, M, H, W, 0.4, 1.0, 1.0), mix_draw(6, 0, M, H, W, 0.4, 1.0, 1.0))
    for step in range(32):                                                            # one alpha on: that mode only
        assert mix_draw(5, step, M, H, W, 0.4, 0.0, 1.0)[0] == MIXUP
        assert mix_draw(5, step, M, H, W, 0.0, 1.0, 1.0)[0] == CUTMIX


def test_mix_draw_with_probability_zero_never_mixes_and_with_one_half_sometimes():
    from fumi_amd.dataset.supervised_pixels import mix_draw
    n = 0
    for step in range(64):
        mode, lam, box, partner = mix_draw(5, step, 8, 6, 6, 0.4, 1.0, 0.0)
        assert mode is None and lam == 1.0 and box == (0, 0, 0, 0) and np.array_equal(partner, np.arange(8))
        assert mix_draw(5, step, 8, 6, 6, 0.0, 0.0, 1.0)[0] is None                   # nothing to mix with
        n += mix_draw(5, step, 8, 6, 6, 0.4, 1.0, 0.5)[0] is not None
    assert 0 < n < 64


def test_mix_stream_is_keyed_apart_from_the_epoch_permutation():
    from fumi_amd.dataset.supervised_pixels import batch_indices, epoch_permutation, mix_draw
    # with mix off nothing about the schedule moves: the values tests/test_pretrain_cpu.py holds it to, once more
    n, batch, seed = 53, 8, 11
    assert torch.equal(batch_indices(n, batch, seed, 6), epoch_permutation(n, seed, 1)[:batch])
    g = torch.Generator(); g.manual_seed((seed * 1000003 + 1) % (2 ** 63 - 1))
    assert torch.equal(epoch_permutation(n, seed, 1), torch.randperm(n, generator=g))
    # and the partner permutation is not the epoch's
    assert not np.array_equal(mix_draw(seed, 1, n, 8, 8, 0.4, 0.0, 1.0)[3], epoch_permutation(n, seed, 1).numpy())


# ---- flags and refusals ---------------------------------------------------------------------------------------------------------
def test_mix_flags_parse_with_their_defaults_and_the_engine_flag_list_is_unchanged():
    from fumi_amd.utils import utils
    d = utils.parser().parse_args([])
    assert (d.label_smoothing, d.mixup_alpha, d.cutmix_alpha, d.mix_prob) == (0.0, 0.0, 0.0, 1.0)
    a = utils.parser().parse_args(["--model", "pretrain", "--label_smoothing", "0.1", "--mixup_alpha", "0.4", "--cutmix_alpha", "1.0",
                                   "--mix_prob", "0.5"])
    assert (a.label_smoothing, a.mixup_alpha, a.cutmix_alpha, a.mix_prob) == (0.1, 0.4, 1.0, 0.5)
    assert [f for f, _ in utils._ENGINE_FLAGS][-3:] == ["--pretrain_batch", "--pretrain_bn_group", "--encoder_checkpoint"]
    assert len(utils._ENGINE_FLAGS) == 17
    assert [f for f, _ in utils._PRETRAIN_MIX_FLAGS] == ["--label_smoothing", "--mixup_alpha", "--cutmix_alpha", "--mix_prob"]
    flags = [act.option_strings[0] for act in utils.parser()._actions if act.option_strings and act.dest != "help"]
    assert flags[-4:] == [f for f, _ in utils._PRETRAIN_MIX_FLAGS]                    # appended after every earlier flag


@pytest.mark.parametrize("flag,value", [("--label_smoothing", "0.1"), ("--mixup_alpha", "0.4"), ("--cutmix_alpha", "1.0"),
                                        ("--mix_prob", "0.5")])
def test_check_supported_refuses_a_mix_flag_without_model_pretrain(flag, value, oracle_engine):
    from fumi_amd import main as cli
    with pytest.raises(ValueError, match="--model pretrain"):
        cli.check_supported(cli.parse_args(["--model", "am3", "--disable_cuda", "--dropout", "0", flag, value]))
    cli.check_supported(cli.parse_args(["--model", "pretrain", "--disable_cuda", "--dataset", "synthetic-resident", "--im_encoder",
                                        "conv4", flag, value]))


@pytest.mark.parametrize("flag,value", [("--label_smoothing", "1.0"), ("--label_smoothing", "-0.1"), ("--mixup_alpha", "-0.5"),
                                        ("--cutmix_alpha", "-1"), ("--mix_prob", "1.5"), ("--mix_prob", "-0.1")])
def test_check_supported_refuses_values_out_of_range(flag, value, oracle_engine):
    from fumi_amd import main as cli
    with pytest.raises(ValueError, match=flag):
        cli.check_supported(cli.parse_args(["--model", "pretrain", "--disable_cuda", "--dataset", "synthetic-resident", "--im_encoder",
                                            "conv4", flag, value]))


def test_pretrain_refuses_a_smoothing_it_cannot_train_with(oracle_engine):
    from fumi_amd.models.pretrain import Pretrain
    assert Pretrain("conv4", image_size=16, n_classes=4).label_smoothing == 0.0
    assert Pretrain("conv4", image_size=16, n_classes=4, label_smoothing=0.1).label_smoothing == 0.1
    with pytest.raises(ValueError, match="label_smoothing"):
        Pretrain("conv4", image_size=16, n_classes=4, label_smoothing=1.0)
