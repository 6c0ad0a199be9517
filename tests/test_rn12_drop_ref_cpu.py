"""CPU suite of DropBlock / dropout in the ResNet-12 (--drop_rate): the reference tests/rn12_drop_ref.py on its
own (dilation against the definition, the kept fraction of a large mask against its binomial expectation, the global indexing of
episodes), the annealing schedule, the flags and the refusals."""
import numpy as np
import pytest

import rn12_drop_ref as R
from oracle_engine import OracleEngine

SEED = 0x5EED0123456789AB


@pytest.mark.parametrize("bs", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("H", [1, 5, 10, 11, 42])
def test_dilation_equals_any_seed_within_reach(bs, H):
    W = max(1, H - 1) if H > 1 else 1                      # (not square where it can be)
    b = min(bs, H, W)                                      # bs > H: clamped, as the kernel's plan does
    rs = np.random.RandomState(100 * bs + H)
    for density in (0.05, 0.3):
        s = rs.random_sample((3, 2, H - b + 1, W - b + 1)) < density
        assert np.array_equal(R.dilate(s, b, H, W), R.dilate_brute(s, b, H, W))
    assert R.plan(H, W, 0.1, bs)[0] == b


@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_kept_fraction_of_element_dropout_within_five_sigma(rate):
    M, C, H, W = 64, 64, 21, 21
    keep = R.keep_mask(SEED, 1, 0, 0, M, C, H, W, rate, 1)
    n = keep.size
    thr = R.plan(H, W, rate, 1)[1]
    p_keep = 1.0 - thr / 4294967296.0
    assert abs(p_keep - (1.0 - rate)) < 1e-6
    sd = (n * p_keep * (1 - p_keep)) ** 0.5
    assert abs(int(keep.sum()) - n * p_keep) <= 5 * sd, (int(keep.sum()), n * p_keep, sd)
    # every plane and every position drops at about the rate too (a stuck key bit would show here): 5 sigma of their own counts
    per_plane = keep.reshape(M * C, -1).sum(1)
    sd_p = (H * W * p_keep * (1 - p_keep)) ** 0.5
    assert abs(per_plane.mean() - H * W * p_keep) <= 5 * sd_p / (M * C) ** 0.5
    per_pos = keep.reshape(M * C, -1).sum(0)
    assert np.all(np.abs(per_pos - M * C * p_keep) <= 5 * (M * C * p_keep * (1 - p_keep)) ** 0.5)


@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_seed_fraction_of_dropblock_within_five_sigma(rate):
    M, C, H, W, bs = 64, 64, 21, 21, 5
    b, thr = R.plan(H, W, rate, bs)
    s = R.seeds(SEED, 2, 1, 3, M, C, H - b + 1, W - b + 1, thr)
    gamma = rate / 25.0 * (H * W) / ((H - 4) * (W - 4))
    assert abs(thr / 4294967296.0 - gamma) < 1e-6
    sd = (s.size * gamma * (1 - gamma)) ** 0.5
    assert abs(int(s.sum()) - s.size * gamma) <= 5 * sd
    keep = ~R.dilate(s, b, H, W)
    kept, scale = R.kept_scale(keep)
    assert kept == int(keep.sum()) and scale == np.float32(keep.size) / np.float32(kept) and scale.dtype == np.float32
    assert R.kept_scale(np.zeros((2, 3), dtype=bool)) == (0, np.float32(0.0))


def test_mask_follows_the_global_episode_not_the_chunk_offset():
    M, H, W, C = 3, 10, 10, 32
    rs = np.random.RandomState(0)
    bits = R.f32_to_bf16_bits(rs.standard_normal((4, M * (H + 2) * (W + 2), C)).astype(np.float32))
    whole, kept, scale = R.apply_map(bits, M, H, W, 0.3, 3, SEED, 2, 1, 0)
    for b0 in (1, 2, 3):                                   # the same episodes reached as the head of a later chunk
        part, k, s = R.apply_map(bits[b0:], M, H, W, 0.3, 3, SEED, 2, 1, b0)
        assert np.array_equal(part, whole[b0:]) and np.array_equal(k, kept[b0:]) and np.array_equal(s, scale[b0:])
    assert len({int(k) for k in kept}) > 1                 # episodes differ from each other
    other = R.apply_map(bits, M, H, W, 0.3, 3, SEED, 2, 0, 0)[0]
    assert not np.array_equal(other, whole)                # and the support set from the query set
    # borders pass through untouched, dropped cells are +0, kept cells are the rounded fp32 product
    x = whole.reshape(4, M, H + 2, W + 2, C)
    src = bits.reshape(4, M, H + 2, W + 2, C)
    assert np.array_equal(x[:, :, 0], src[:, :, 0]) and np.array_equal(x[:, :, :, -1], src[:, :, :, -1])
    assert (x[:, :, 1:-1, 1:-1] == 0).mean() > 0.2


def test_annealing_schedule():
    from fumi_amd.models.resnet12 import DropSchedule, drop_rate_at, drop_step_seed
    assert drop_rate_at(0.1, 0, 40000) == 0.0
    assert drop_rate_at(0.1, 20000, 40000) == 0.1 * 0.5
    assert drop_rate_at(0.1, 40000, 40000) == 0.1
    assert drop_rate_at(0.1, 10 ** 9, 40000) == 0.1
    assert drop_rate_at(0.1, 0, 0) == 0.1 and drop_rate_at(0.1, 7, 0) == 0.1
    s = DropSchedule(0.1, block_size=5, blocks=2, anneal_steps=100, seed=123, n_blocks=4)
    rates, blocks, seed = s.args(50)
    assert rates == [0.05] * 4 and blocks == [1, 1, 5, 5] and seed == drop_step_seed(123, 50)
    assert DropSchedule(0.1, blocks=0, n_blocks=2).block_sizes() == [1, 1]
    assert DropSchedule(0.1, blocks=4, block_size=3).block_sizes() == [3] * 4
    seeds = {drop_step_seed(123, t) for t in range(1000)} | {drop_step_seed(124, t) for t in range(1000)}
    assert len(seeds) == 2000 and all(0 <= v < 2 ** 64 for v in seeds)
    for bad in (dict(rate=1.0), dict(rate=-0.1), dict(rate=0.1, block_size=9), dict(rate=0.1, block_size=0), dict(rate=0.1, blocks=5),
                dict(rate=0.1, anneal_steps=-1)):
        with pytest.raises(ValueError):
            DropSchedule(**bad)


def test_flags_parse_and_reach_the_models():
    from fumi_amd.utils import utils
    d = utils.drop_parser().parse_args([])
    assert (d.drop_rate, d.drop_block_size, d.drop_blocks, d.drop_anneal_steps) == (0.0, 5, 2, 40000)
    assert [f for f, _ in utils._DROP_FLAGS] == ["--drop_rate", "--drop_block_size", "--drop_blocks", "--drop_anneal_steps"]
    flags = lambda p: [a.option_strings[0] for a in p._actions if a.option_strings and a.dest != "help"]
    assert flags(utils.drop_parser()) == flags(utils.main_parser()) + [f for f, _ in utils._DROP_FLAGS]     # the earlier sequence is kept
    with pytest.raises(SystemExit):
        utils.main_parser().parse_args(["--drop_rate", "0.1"])
    argv = ["--im_encoder", "resnet12", "--image_size", "16", "--num_ways", "3", "--drop_rate", "0.1", "--drop_block_size", "3",
            "--drop_blocks", "1", "--drop_anneal_steps", "10", "--seed", "7"]
    for model in ("pretrain", "metabaseline"):
        a = utils.drop_parser().parse_args(["--model", model] + argv)
        a.device, a.n_classes = "cpu", 6                   # (the dataset sets n_classes)
        m = utils.init_model(a, None, watch=False)
        assert (m.drop.rate, m.drop.block_size, m.drop.blocks, m.drop.anneal_steps, m.drop.seed) == (0.1, 3, 1, 10, 7)
        assert m.drop.block_sizes() == [1, 1, 1, 3] and m.drop_step == 0
        a.drop_rate = 0.0
        plain = utils.init_model(a, None, watch=False)
        assert plain.drop is None
        assert list(m.state_dict().keys()) == list(plain.state_dict().keys())              # the checkpoint format does not change


def test_check_supported_refuses_what_the_drop_pass_cannot_run():
    from fumi_amd import engine
    from fumi_amd import main as cli
    old = engine.set_engine(OracleEngine())
    try:
        base = ["--disable_cuda", "--dataset", "synthetic-resident"]
        rn = base + ["--im_encoder", "resnet12", "--drop_rate", "0.1"]
        cli.check_supported(cli.parse_args(["--model", "pretrain"] + rn))
        cli.check_supported(cli.parse_args(["--model", "metabaseline"] + rn))
        cli.check_supported(cli.parse_args(["--model", "metabaseline"] + rn + ["--drop_block_size", "8", "--drop_blocks", "4",
                                                                               "--drop_anneal_steps", "0"]))
        for model in ("pretrain", "metabaseline"):
            with pytest.raises(NotImplementedError, match="--im_encoder resnet12"):
                cli.check_supported(cli.parse_args(["--model", model] + base + ["--im_encoder", "conv4", "--drop_rate", "0.1"]))
        for model in ("fumi", "maml"):
            with pytest.raises(NotImplementedError, match="second-order"):
                cli.check_supported(cli.parse_args(["--model", model] + rn))
        with pytest.raises(NotImplementedError, match="--drop_rate"):
            cli.check_supported(cli.parse_args(["--model", "am3", "--dropout", "0"] + rn))
        for bad in ("1", "-0.1"):
            with pytest.raises(ValueError, match="--drop_rate"):
                cli.check_supported(cli.parse_args(["--model", "pretrain"] + base + ["--im_encoder", "resnet12", "--drop_rate", bad]))
        for flag, bad in (("--drop_block_size", "9"), ("--drop_block_size", "0"), ("--drop_blocks", "5"), ("--drop_anneal_steps", "-1")):
            with pytest.raises(ValueError, match=flag):
                cli.check_supported(cli.parse_args(["--model", "pretrain"] + rn + [flag, bad]))
        with pytest.raises(ValueError, match="--drop_rate > 0"):
            cli.check_supported(cli.parse_args(["--model", "pretrain"] + base + ["--im_encoder", "resnet12", "--drop_blocks", "1"]))
        with pytest.raises(NotImplementedError, match="64"):
            cli.check_supported(cli.parse_args(["--model", "pretrain"] + rn + ["--image_size", "300", "--drop_blocks", "3"]))
        # without the flag nothing new is asked
        cli.check_supported(cli.parse_args(["--model", "pretrain"] + base + ["--im_encoder", "conv4"]))
    finally:
        engine.set_engine(old)
