"""CPU suite of the resize / random-resized-crop stage of the resident image path: the numpy restatement of
fumi_hip_gather_images_resized (tests/image_resize_ref.py) against torch's antialiased bilinear interpolation in float64, the
rectangles of the random mode, the new flags and host-side checks, and the resources of the new kernels."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import image_resize_ref as RR
from conftest import ROOT

# rectangle (h, w) -> output (Ho, Wo); the largest float32-vs-torch-float64 difference seen on the 0..255 scale was 1.5e-3 (96 -> 84)
SHAPES = [(8, 8, 12, 12), (14, 14, 12, 12), (20, 16, 12, 12), (33, 47, 12, 12), (96, 96, 84, 84), (160, 128, 84, 84)]
BOUND = 1e-2          # a wrong tap or weight moves a pixel by whole gray levels


def _torch_resize(u, Ho, Wo, antialias):
    x = torch.from_numpy(u.astype(np.float64))[None]
    return torch.nn.functional.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=False, antialias=antialias)[0].numpy()


@pytest.mark.parametrize("h,w,Ho,Wo", SHAPES)
def test_float32_restatement_is_torchs_antialiased_bilinear(h, w, Ho, Wo):
    u = np.random.RandomState(h * 131 + w).randint(0, 256, (3, h, w)).astype(np.uint8)
    u[0, 0, 0], u[0, -1, -1] = 0, 255
    r = RR.resample(u, Ho, Wo)
    assert r.dtype == np.float32 and r.shape == (3, Ho, Wo)
    err = float(np.abs(r.astype(np.float64) - _torch_resize(u, Ho, Wo, True)).max())
    print(f"{h} x {w} -> {Ho} x {Wo}: float32 restatement vs torch float64 antialias {err:.3e}")
    assert err <= BOUND
    assert float(np.abs(RR.resample(u, Ho, Wo, np.float64) - _torch_resize(u, Ho, Wo, True)).max()) <= 1e-9
    if h <= Ho and w <= Wo:                                                    # an upscale: plain bilinear with clamped edges
        assert float(np.abs(r.astype(np.float64) - _torch_resize(u, Ho, Wo, False)).max()) <= BOUND


def test_same_size_is_the_input_bit_for_bit():
    for C, h, w in ((3, 12, 12), (1, 9, 7), (3, 84, 84)):
        u = np.random.RandomState(h).randint(0, 256, (C, h, w)).astype(np.uint8)
        assert np.array_equal(RR.resample(u, h, w), u.astype(np.float32))
        assert np.array_equal(RR.resample(u, h, w, np.float64), u.astype(np.float64))


def test_random_rectangles_stay_inside_and_cover_the_scale_range():
    Hs, Ws, n = 24, 20, 10000
    lo, hi, rmax = 0.08, 1.0, 4.0 / 3.0
    rects = np.array([RR.random_rect(5, 7, 0, i, Hs, Ws, lo, hi, rmax) for i in range(n)])
    x0, y0, w, h = rects.T
    assert (w >= 1).all() and (h >= 1).all() and (x0 >= 0).all() and (y0 >= 0).all()
    assert (x0 + w <= Ws).all() and (y0 + h <= Hs).all()
    assert len({tuple(r) for r in rects.tolist()}) > 1000
    un = np.array([RR.random_rect_unclamped(5, 7, 0, i, Hs, Ws, lo, hi, rmax) for i in range(n)])
    frac = un[:, 0] * un[:, 1] / float(Hs * Ws)                                # w h / A of the unclamped draws = a
    assert abs(float(frac.mean()) - (lo + hi) / 2) < 0.02
    assert frac.min() >= lo - 1e-5 and frac.max() <= hi + 1e-5
    for i in range(200):                                                       # the whole image every time
        assert RR.random_rect(5, 7, 1, i, 16, 16, 1.0, 1.0, 1.0) == (0, 0, 16, 16)
    assert [RR.random_rect(5, 7, 0, i, Hs, Ws, lo, hi, rmax) for i in range(50)] != \
           [RR.random_rect(5, 7, 1, i, Hs, Ws, lo, hi, rmax) for i in range(50)]


def test_restatement_flip_and_whole_image_equal_the_plain_gather():
    import image_gather_ref as IR
    t = np.random.RandomState(3).randint(0, 256, (5, 3, 12, 12)).astype(np.uint8)
    idx = np.arange(11) % 5
    mean, std = (0.4, 0.5, 0.45), (0.2, 0.25, 0.3)
    for jit in ((0, 0, 0), (0.4, 0.4, 0.4)):
        a = RR.gather_images_resized(t, idx, mean, std, (12, 12), seed=3, step=4, stream_id=1, rect=(0, 0, 12, 12), flip=True, jitter=jit)
        b = IR.gather_images(t, idx, mean, std, seed=3, step=4, stream_id=1, pad=0, flip=True, jitter=jit)
        assert np.array_equal(a, b)
    c = RR.gather_images_resized(t, idx, mean, std, (12, 12), seed=3, step=4, scale=(1.0, 1.0), ratio=1.0)
    assert np.array_equal(c, IR.gather_images(t, idx, mean, std))


def test_new_flags_parse_with_their_defaults_and_train_augmentation_is_unchanged():
    from fumi_amd.utils import utils
    from fumi_amd.dataset.synthetic import center_rect, resize_settings, train_augmentation
    d = utils.parser().parse_args([])
    assert d.image_crop_frac == 0.875 and d.augment_scale is None and d.augment_ratio == 4.0 / 3.0 and d.synthetic_table_size is None
    a = utils.parser().parse_args(["--augment", "--augment_scale", "0.25", "0.9", "--augment_ratio", "1.5", "--image_crop_frac", "0.8",
                                   "--synthetic_table_size", "96"])
    assert a.augment_scale == [0.25, 0.9] and a.augment_ratio == 1.5 and a.image_crop_frac == 0.8 and a.synthetic_table_size == 96
    assert train_augmentation(d) is None
    assert train_augmentation(a) == dict(pad=8, flip=True, jitter=(0.4, 0.4, 0.4))
    assert resize_settings(d, (84, 84)) is None                                 # today's path
    assert center_rect(96, 96, 0.875) == (6, 6, 84, 84) and center_rect(20, 24, 0.875) == (3, 1, 18, 18) and center_rect(1, 1, 0.1) == (0, 0, 1, 1)
    assert center_rect(20, 24, 0.875) == RR.center_rect(20, 24, 0.875)
    r = resize_settings(d, (96, 96))
    assert r == dict(out_size=(84, 84), eval=dict(rect=(6, 6, 84, 84)), train=dict(rect=(6, 6, 84, 84)), augment=None)
    g = utils.parser().parse_args(["--augment"])
    r = resize_settings(g, (96, 96))
    assert r["eval"] == dict(rect=(6, 6, 84, 84)) and r["train"] == dict(scale=(0.08, 1.0), ratio=4.0 / 3.0)
    assert r["augment"] == dict(flip=True, jitter=(0.4, 0.4, 0.4))
    r = resize_settings(a, (84, 84))                                            # --augment_scale alone takes the resize path
    assert r["train"] == dict(scale=(0.25, 0.9), ratio=1.5) and r["eval"] == dict(rect=(8, 8, 67, 67))
    one = utils.parser().parse_args(["--augment", "--image_channels", "1"])
    assert resize_settings(one, (96, 96))["augment"] == dict(flip=True, jitter=(0.0, 0.0, 0.0))


def test_image_npy_checks_accept_another_stored_size(tmp_path):
    from fumi_amd.utils import utils
    from fumi_amd.dataset.image_table import check_image_splits, load_image_split
    rs = np.random.RandomState(0)
    for split in ("train", "val", "test"):
        np.save(tmp_path / f"{split}_images.npy", rs.randint(0, 256, (8, 20, 20, 3)).astype(np.uint8))
        np.save(tmp_path / f"{split}_labels.npy", np.arange(8) % 4)
        np.save(tmp_path / f"{split}_class_text.npy", rs.standard_normal((4, 16)).astype(np.float32))
    splits = {s: load_image_split(str(tmp_path), s) for s in ("train", "val", "test")}
    args = utils.parser().parse_args(["--image_size", "16", "--text_emb_dim", "16"])
    check_image_splits(args, splits)                                            # 20 x 20 files, 16 x 16 encoder
    check_image_splits(utils.parser().parse_args(["--image_size", "20", "--text_emb_dim", "16"]), splits)
    with pytest.raises(ValueError):                                            # channels still have to fit
        check_image_splits(utils.parser().parse_args(["--image_size", "16", "--text_emb_dim", "16", "--image_channels", "1"]), splits)
    with pytest.raises(ValueError):
        check_image_splits(utils.parser().parse_args(["--image_size", "16", "--text_emb_dim", "8"]), splits)
    mixed = dict(splits)
    mixed["val"] = (splits["val"][0][:, :, :16, :16], splits["val"][1], splits["val"][2])
    with pytest.raises(ValueError):                                            # one split of --image_size, the others not
        check_image_splits(args, mixed)


def test_host_surface_names_the_resized_gather():
    from fumi_amd import hip
    assert "fumi_hip_gather_images_resized" in hip.SYMBOLS and callable(hip.gather_images_resized)
    with pytest.raises(hip.FumiHipError):                                      # no CPU path, like every other entry
        hip.gather_images_resized(None, torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), (0,) * 3, (1,) * 3,
                                  (4, 4), rect=(0, 0, 8, 8))


def test_resized_gather_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    src = os.path.join(ROOT, "fumi_amd", "csrc", "imresize.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", str(tmp_path / "o.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen[name] = {}
        m = re.search(r"(ScratchSize \[bytes/lane\]|SGPRs Spill|VGPRs Spill): (\d+)", line)
        if m and name:
            seen[name][m.group(1)] = int(m.group(2))
    forms = {k: v for k, v in seen.items() if "gather_images_resized_kernel" in k}
    assert len(forms) == 8, sorted(seen)                                       # vector / scalar x jitter x mode
    for k, v in forms.items():
        assert len(v) == 3 and all(x == 0 for x in v.values()), (k, v)
