"""GPU suite of the blending kernel (fumi_hip_mix_images, csrc/immix.hip) against tests/image_mix_ref.py.

CutMix is a copy: bit-exact.  mixup is lam * a + u * b with u = 1.0f - lam: three float32 roundings (two products, one sum) after the
rounding of u, each at most 2^-24 relative to a value no larger than max(|a|, |b|) (lam + u <= 1 + 2^-24), so against the float64 value
of the float32 inputs, lam and u:  |got - ref| <= 4 * 2^-24 * max(|a|, |b|) per element."""
import numpy as np
import pytest
import torch

import image_mix_ref as MR

pytestmark = pytest.mark.gpu

# (M, C, H, W): one pixel; an odd image length (189 floats: single-float path); the 84 x 84 image (128-bit path, several workgroups)
SHAPES = [(2, 1, 1, 1), (5, 3, 7, 9), (16, 3, 84, 84)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _case(M, C, H, W):
    g = torch.Generator().manual_seed(10007 * M + 101 * H + W)
    x = torch.randn(M, C, H, W, generator=g)
    return x, torch.roll(torch.arange(M), max(1, M // 3))        # a permutation without a fixed point


def _boxes(H, W):
    """(bx0, by0, bx1, by1): empty, the whole image, one touching each edge, one pixel."""
    hx, hy = max(1, W // 2), max(1, H // 2)
    out = [(0, 0, 0, 0), (W // 2, H // 2, W // 2, H // 2), (0, 0, W, H),
           (0, H // 3, hx, min(H, H // 3 + hy)), (W - hx, H // 3, W, min(H, H // 3 + hy)),          # left, right
           (W // 3, 0, min(W, W // 3 + hx), hy), (W // 3, H - hy, min(W, W // 3 + hx), H),          # top, bottom
           (W - 1, H - 1, W, H), (W // 2, H // 2, W // 2 + 1, H // 2 + 1)]
    return list(dict.fromkeys(out))


@pytest.mark.parametrize("M,C,H,W", SHAPES)
def test_cutmix_is_an_exact_copy(M, C, H, W, dev, ws):
    from fumi_amd import hip
    x, partner = _case(M, C, H, W)
    xd, pd = x.to(dev), partner.to(dev)
    for box in _boxes(H, W):
        out = hip.mix_images(ws, xd, pd, mode=hip.MIX_CUTMIX, box=box)
        ref = MR.mix_images(x.numpy(), partner.numpy(), MR.CUTMIX, box=box)
        assert out.dtype == torch.float32 and out.shape == x.shape
        assert np.array_equal(out.cpu().numpy(), ref.astype(np.float32)), box
    assert torch.equal(hip.mix_images(ws, xd, pd, mode=hip.MIX_CUTMIX, box=(0, 0, W, H)), xd[pd])
    assert ws.read_status() == 0


@pytest.mark.parametrize("M,C,H,W", SHAPES)
def test_mixup_is_within_four_roundings_of_float64(M, C, H, W, dev, ws):
    from fumi_amd import hip
    x, partner = _case(M, C, H, W)
    xd, pd = x.to(dev), partner.to(dev)
    big = np.maximum(np.abs(x.numpy()), np.abs(x.numpy()[partner.numpy()])).astype(np.float64)
    for lam in (0.3, 0.5, 0.9371, 0.0):
        out = hip.mix_images(ws, xd, pd, mode=hip.MIX_MIXUP, lam=lam)
        ref = MR.mix_images(x.numpy(), partner.numpy(), MR.MIXUP, lam=lam)
        err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
        print(f"mixup ({M},{C},{H},{W}) lam {lam}: largest error / (2^-24 max(|a|,|b|)) = {float((err / (2.0 ** -24 * np.maximum(big, 1e-30))).max()):.3f}")
        assert bool((err <= 4 * 2.0 ** -24 * big).all()), lam
        assert torch.equal(hip.mix_images(ws, xd, pd, mode=hip.MIX_MIXUP, lam=lam), out)
    assert torch.equal(hip.mix_images(ws, xd, pd, mode=hip.MIX_MIXUP, lam=1.0), xd)                 # lam = 1: x, bit for bit
    assert torch.equal(hip.mix_images(ws, xd, pd, mode=hip.MIX_MIXUP, lam=0.0), xd[pd])
    assert ws.read_status() == 0


@pytest.mark.parametrize("M,C,H,W", SHAPES)
def test_identity_partner_returns_x(M, C, H, W, dev, ws):
    from fumi_amd import hip
    x, _ = _case(M, C, H, W)
    xd, ident = x.to(dev), torch.arange(M, device=dev)
    assert torch.equal(hip.mix_images(ws, xd, ident, mode=hip.MIX_MIXUP, lam=0.3), xd)
    assert torch.equal(hip.mix_images(ws, xd, ident, mode=hip.MIX_CUTMIX, box=(0, 0, W, H)), xd)
    assert ws.read_status() == 0


@pytest.mark.parametrize("M,C,H,W", SHAPES[1:])
def test_partner_out_of_range_sets_the_status_bit_and_copies_the_row(M, C, H, W, dev, ws):
    from fumi_amd import hip
    x, partner = _case(M, C, H, W)
    for bad in (M, -1, 2 ** 40):
        p = partner.clone(); p[1] = bad
        for mode, kw in ((hip.MIX_MIXUP, dict(lam=0.3)), (hip.MIX_CUTMIX, dict(box=(0, 0, W, H)))):
            out = hip.mix_images(ws, x.to(dev), p.to(dev), mode=mode, **kw)
            assert ws.read_status() & hip.ST_LABEL_RANGE
            assert ws.read_status() == 0
            assert torch.equal(out[1].cpu(), x[1])
            ref = MR.mix_images(x.numpy(), p.numpy(), mode, **kw)
            assert np.abs(out.cpu().numpy() - ref).max() <= 4 * 2.0 ** -24 * float(x.abs().max())


def test_invalid_arguments_are_refused(dev, ws):
    from fumi_amd import hip
    L = hip.lib()
    M, C, H, W = 4, 3, 8, 8
    x = torch.zeros(2 * M, C, H, W, device=dev)
    p = torch.full((M,), M, dtype=torch.int64, device=dev)                              # a launch would set the status bit
    refuse = lambda **kw: pytest.raises(hip.FumiHipError, match="fumi_hip_mix_images.*invalid argument")
    for kw in (dict(mode=2), dict(mode=-1), dict(mode=0, lam=1.5), dict(mode=0, lam=-0.1), dict(mode=0, lam=float("nan")),
               dict(mode=1, box=(0, 0, W + 1, H)), dict(mode=1, box=(0, 0, W, H + 1)), dict(mode=1, box=(-1, 0, W, H)),
               dict(mode=1, box=(0, -1, W, H)), dict(mode=1, box=(5, 0, 4, H)), dict(mode=1, box=(0, 5, W, 4))):
        with refuse():
            hip.mix_images(ws, x[:M], p, **kw)
    # out overlapping x: row i reads row partner[i]
    st = hip._stream(dev)
    call = lambda m, src, out: L.fumi_hip_mix_images(ws.handle, st, m, C, H, W, hip._f32(src, "x"), hip._i64(p, "partner"), 0, 0.5,
                                                     0, 0, 0, 0, hip._f32(out, "out"))
    assert call(M, x[:M], x[:M]) == -1                                                  # the same tensor
    assert call(M, x[:M], x[M - 1:2 * M - 1]) == -1 and call(M, x[1:M + 1], x[:M]) == -1 # one image of overlap, either side
    assert call(0, x[:M], x[M:]) == -1                                                  # M < 1
    assert ws.read_status() == 0
