"""CPU suite of the resident uint8 image path: the numpy restatement of fumi_hip_gather_images (tests/image_gather_ref.py) is held to
its own invariants -- it is what the GPU suite compares the kernel with --, ``load_image_split`` parses and refuses files, the new
flags parse, and the host surface names the new symbol."""
import numpy as np
import pytest

import image_gather_ref as IR

MEAN, STD = (0.45, 0.5, 0.4), (0.25, 0.2, 0.3)


def _table(seed, n, C, H, W):
    t = np.random.RandomState(seed).randint(0, 256, (n, C, H, W)).astype(np.uint8)
    t[0, :, 0, 0], t[0, :, -1, -1] = 0, 255                  # both ends of the byte range in every channel
    return t


# ---- restatement invariants ---------------------------------------------------------------------------------------------------------
def test_no_augmentation_is_plain_normalisation():
    t = _table(0, 7, 3, 6, 8)
    idx = np.array([3, 0, 6, 3])
    out = IR.gather_images(t, idx, MEAN, STD)
    k = np.float32(1) / np.float32(255)
    inv = np.float32(1) / np.asarray(STD, np.float32)
    want = (t[idx].astype(np.float32) * k - np.asarray(MEAN, np.float32).reshape(3, 1, 1)) * inv.reshape(3, 1, 1)
    assert out.dtype == np.float32 and np.array_equal(out, want)
    out64 = IR.gather_images(t, idx, MEAN, STD, dtype=np.float64)
    assert out64.dtype == np.float64 and np.abs(out64 - out).max() < 1e-6 * float(inv.max())
    assert np.array_equal(IR.gather_images(t, [7, -1], MEAN, STD), IR.gather_images(t, [0, 0], MEAN, STD))    # out of range: image 0


def test_crop_and_flip_move_pixels_as_torchvision_orders_them():
    t = _table(1, 2, 1, 5, 6)
    img = t[1]
    padded = np.zeros((1, 5 + 4, 6 + 4), np.uint8)
    padded[:, 2:7, 2:8] = img
    for ox in range(5):
        for oy in range(5):
            crop = padded[:, oy:oy + 5, ox:ox + 6]
            assert np.array_equal(IR.source_window(img, ox, oy, 0, 2), crop)
            assert np.array_equal(IR.source_window(img, ox, oy, 1, 2), crop[:, :, ::-1])


def test_offsets_cover_their_range_and_flips_are_fair():
    pad, n = 2, 2000
    d = np.array([IR.draws(123, 5, 0, i, pad, True) for i in range(n)])
    assert set(d[:, 0]) == set(range(2 * pad + 1)) and set(d[:, 1]) == set(range(2 * pad + 1))
    assert abs(d[:, 2].mean() - 0.5) <= 0.05
    assert IR.draws(123, 5, 0, 17, 0, False) == (0, 0, 0)                       # pad 0: the window is the image


def test_streams_and_steps_draw_differently():
    pad, n = 2, 64
    s0 = [IR.draws(9, 3, 0, i, pad, True) for i in range(n)]
    s1 = [IR.draws(9, 3, 1, i, pad, True) for i in range(n)]
    s0_next = [IR.draws(9, 4, 0, i, pad, True) for i in range(n)]
    assert s0 != s1 and s0 != s0_next and s1 != s0_next
    assert s0 == [IR.draws(9, 3, 0, i, pad, True) for i in range(n)]
    t = _table(2, 5, 3, 8, 8)
    idx = np.arange(40) % 5
    a = IR.gather_images(t, idx, MEAN, STD, seed=9, step=3, stream_id=0, pad=pad, flip=True)
    assert not np.array_equal(a, IR.gather_images(t, idx, MEAN, STD, seed=9, step=3, stream_id=1, pad=pad, flip=True))
    assert not np.array_equal(a, IR.gather_images(t, idx, MEAN, STD, seed=9, step=4, stream_id=0, pad=pad, flip=True))


def test_zero_jitter_is_no_jitter_and_jitter_stays_in_range():
    t = _table(3, 4, 3, 8, 8)
    idx = np.array([0, 1, 2, 3, 0])
    kw = dict(seed=4, step=2, pad=1, flip=True)
    a = IR.gather_images(t, idx, MEAN, STD, jitter=0, **kw)
    b = IR.gather_images(t, idx, MEAN, STD, jitter=(0, 0, 0), **kw)
    assert a.tobytes() == b.tobytes()
    j = IR.gather_images(t, idx, (0, 0, 0), (1, 1, 1), jitter=0.4, **kw)
    assert not np.array_equal(j, IR.gather_images(t, idx, (0, 0, 0), (1, 1, 1), **kw))
    assert j.min() >= 0.0 and j.max() <= 1.0                                   # every step clamps to [0, 1]
    f = np.array([IR.jitter_factors(4, 2, 0, i, (0.4, 0.4, 0.4)) for i in range(500)])
    assert f.min() >= 0.6 and f.max() <= 1.4 and f.std(axis=0).min() > 0.15
    for one in ((0.4, 0, 0), (0, 0.4, 0), (0, 0, 0.4)):                        # every step acts on its own
        assert not np.array_equal(IR.gather_images(t, idx, MEAN, STD, jitter=one, **kw), a)
    j64 = IR.gather_images(t, idx, MEAN, STD, jitter=0.4, dtype=np.float64, **kw)
    j32 = IR.gather_images(t, idx, MEAN, STD, jitter=0.4, **kw)
    assert np.abs(j64 - j32).max() < 1e-5 * 5.0


# ---- load_image_split ---------------------------------------------------------------------------------------------------------------
def _write_split(root, split, images, labels, text):
    np.save(root / f"{split}_images.npy", images)
    np.save(root / f"{split}_labels.npy", labels)
    np.save(root / f"{split}_class_text.npy", text)


def test_load_image_split_reads_both_layouts(tmp_path):
    from fumi_amd.dataset.image_table import load_image_split
    rs = np.random.RandomState(0)
    planar = rs.randint(0, 256, (10, 3, 12, 14)).astype(np.uint8)
    labels = rs.randint(0, 4, 10).astype(np.int32)
    text = rs.standard_normal((4, 6)).astype(np.float32)
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    _write_split(tmp_path / "a", "train", planar, labels, text)
    _write_split(tmp_path / "b", "train", np.ascontiguousarray(planar.transpose(0, 2, 3, 1)), labels, text)
    ia, la, ta = load_image_split(str(tmp_path / "a"), "train")
    ib, lb, tb = load_image_split(str(tmp_path / "b"), "train")
    assert ia.dtype == np.uint8 and ia.shape == (10, 3, 12, 14) and ia.flags["C_CONTIGUOUS"] and ib.flags["C_CONTIGUOUS"]
    assert np.array_equal(ia, planar) and np.array_equal(ib, planar)
    assert la.dtype == np.int64 and np.array_equal(la, labels) and np.array_equal(lb, labels)
    assert ta.dtype == np.float32 and np.array_equal(ta, text) and np.array_equal(tb, text)
    with pytest.raises(FileNotFoundError):
        load_image_split(str(tmp_path / "a"), "val")


def test_load_image_split_refuses_files_that_do_not_fit(tmp_path):
    from fumi_amd.dataset.image_table import load_image_split
    rs = np.random.RandomState(1)
    planar = rs.randint(0, 256, (6, 3, 12, 12)).astype(np.uint8)
    labels = np.array([0, 1, 2, 0, 1, 2])
    text = rs.standard_normal((3, 5)).astype(np.float32)
    cases = {"float": (planar.astype(np.float32), labels, text),              # not uint8
             "layout": (rs.randint(0, 256, (6, 12, 3, 12)).astype(np.uint8), labels, text),     # channels in the middle
             "flat": (planar.reshape(6, -1), labels, text),                    # not 4-d
             "count": (planar, labels[:5], text),                              # labels != images
             "text": (planar, labels, text[:2])}                               # class id 2 has no text row
    for name, (im, lab, tx) in cases.items():
        d = tmp_path / name
        d.mkdir()
        _write_split(d, "test", im, lab, tx)
        with pytest.raises(ValueError):
            load_image_split(str(d), "test")


# ---- parser and host surface --------------------------------------------------------------------------------------------------------
def test_new_flags_parse_with_their_defaults():
    from fumi_amd.utils import utils
    d = utils.parser().parse_args([])
    assert d.augment is False and d.augment_pad == 8 and d.augment_jitter == 0.4 and d.image_mean is None and d.image_std is None
    a = utils.parser().parse_args(["--augment", "--augment_pad", "4", "--augment_jitter", "0.25", "--image_mean", "0.5", "0.4", "0.3",
                                   "--image_std", "0.2", "--dataset", "image-npy"])
    assert a.augment and a.augment_pad == 4 and a.augment_jitter == 0.25
    assert a.image_mean == [0.5, 0.4, 0.3] and a.image_std == [0.2] and a.dataset == "image-npy"


def test_train_augmentation_and_normalisation_from_the_flags():
    import torch
    from fumi_amd.utils import utils
    from fumi_amd.dataset.synthetic import SyntheticEpisodes, image_normalization, pixel_statistics, synthetic_pixel_table, train_augmentation
    d = utils.parser().parse_args([])
    assert train_augmentation(d) is None
    a = utils.parser().parse_args(["--augment"])
    assert train_augmentation(a) == dict(pad=8, flip=True, jitter=(0.4, 0.4, 0.4))
    base = SyntheticEpisodes(5, 0, 8, 3, 1, 1, 2, 1, "train", image_shape=(3, 6, 6))
    table, coi = synthetic_pixel_table(base, 7, np.random.RandomState(0))
    assert table.dtype == np.uint8 and table.shape == (35, 3, 6, 6) and np.array_equal(coi, np.repeat(np.arange(5), 7))
    assert 100 < table.mean() < 156 and table.std() > 20                      # centred in the byte range, not saturated
    t = torch.from_numpy(table)
    mean, std = pixel_statistics(t, chunk=8)
    x = table.astype(np.float64) / 255
    assert np.allclose(mean, x.mean(axis=(0, 2, 3)), atol=1e-12) and np.allclose(std, x.std(axis=(0, 2, 3)), atol=1e-9)
    assert image_normalization(d, t) == pixel_statistics(t)                   # no flags: the table's own statistics
    g = utils.parser().parse_args(["--image_mean", "0.5", "--image_std", "0.1", "0.2", "0.3"])
    assert image_normalization(g, t) == ((0.5, 0.5, 0.5), (0.1, 0.2, 0.3))


def test_host_surface_names_the_image_gather():
    from fumi_amd import hip
    assert "fumi_hip_gather_images" in hip.SYMBOLS and callable(hip.gather_images)
    import torch
    with pytest.raises(hip.FumiHipError):                                      # no CPU path, like every other entry
        hip.gather_images(None, torch.zeros(2, 3, 4, 4, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), MEAN, STD)
