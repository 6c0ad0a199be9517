"""TEST INFRASTRUCTURE: numpy restatement of fumi_hip_gather_images_resized (fumi_amd/csrc/imresize.hip; the semantics are written
out in include/fumi_hip.h).  A source rectangle of whole pixels is resampled to Ho x Wo with a separable triangle filter
(antialiased bilinear), then flipped, scaled, jittered and normalised as image_gather_ref.gather_images does.  Integer work (the
draws, the rectangles, the tap ranges of the float32 form) is exact; the float work is done in ``dtype``, one rounding per
operation in the kernel's order, so with the jitter off the float32 form IS the kernel's result bit for bit.  The rectangles of the
random mode are always drawn in float32 -- they are integers both forms must share.  The float64 form is the yardstick."""
import numpy as np

import image_gather_ref as IR
from oracle.sampler_ref import step_key, rand_below


def axis_taps(n_in, n_out, dtype=np.float32):
    """Triangle-filter taps of one axis: (k0 int [n_out], cnt int [n_out], w dtype [n_out, max cnt] zero-filled, tot dtype [n_out])."""
    f = dtype
    scale = f(n_in) / f(n_out)
    s = max(scale, f(1))
    inv = f(1) / s
    k0s, ws = [], []
    for x in range(n_out):
        c = scale * (f(x) + f(0.5))
        k0 = max(0, int(c - s + f(0.5)))
        k1 = min(n_in, int(c + s + f(0.5)))
        ws.append([max(f(0), f(1) - abs((f(k) - c + f(0.5)) * inv)) for k in range(k0, k1)])
        k0s.append(k0)
    cnt = np.array([len(w) for w in ws])
    w = np.zeros((n_out, cnt.max()), dtype=dtype)
    tot = np.zeros(n_out, dtype=dtype)
    for x, wx in enumerate(ws):
        w[x, :len(wx)] = wx
        t = f(0)
        for v in wx:
            t = t + v
        tot[x] = t
    return np.array(k0s), cnt, w, tot


def _pass(v, taps, n_in):
    """One axis (the last of ``v``): sum in ascending k of w_k * v[..., k], accumulated as acc = acc + w_k * v, then / tot.  A tap
    past an output's own count has weight +0 and adds nothing to a non-negative sum."""
    k0, cnt, w, tot = taps
    acc = np.zeros(v.shape[:-1] + (len(k0),), dtype=v.dtype)
    for j in range(w.shape[1]):
        acc = acc + w[:, j] * v[..., np.minimum(k0 + j, n_in - 1)]
    return acc / tot


def resample(u, Ho, Wo, dtype=np.float32):
    """uint8 [C, h, w] (the rectangle) -> dtype [C, Ho, Wo] on the 0..255 scale: horizontal pass, then vertical."""
    C, h, w = u.shape
    t = _pass(u.astype(dtype), axis_taps(w, Wo, dtype), w)                       # [C, h, Wo]
    r = _pass(np.ascontiguousarray(t.transpose(0, 2, 1)), axis_taps(h, Ho, dtype), h)      # [C, Wo, Ho]
    return np.ascontiguousarray(r.transpose(0, 2, 1))


def random_rect(seed, step, stream_id, i, Hs, Ws, smin, smax, rmax):
    """(x0, y0, w, h) of output image i: one random-resized-crop draw, clamped (torchvision retries instead)."""
    f = np.float32
    key, b = step_key(int(seed), int(step)), 0xFF00 + int(stream_id)
    r = lambda c, n: rand_below(key, i, b, c, n)
    U = lambda c: f(r(c, 1 << 24)) * f(2.0 ** -24)
    smin, smax, rmax = f(smin), f(smax), f(rmax)
    a = smin + (smax - smin) * U(6)
    q = f(1) + (rmax - f(1)) * U(7)
    ratio = q if r(8, 2) else f(1) / q
    A = f(Hs * Ws)
    wf, hf = np.sqrt(a * A * ratio), np.sqrt(a * A / ratio)
    w = int(min(max(np.rint(wf), f(1)), f(Ws)))
    h = int(min(max(np.rint(hf), f(1)), f(Hs)))
    return int(r(9, Ws - w + 1)), int(r(10, Hs - h + 1)), w, h


def random_rect_unclamped(seed, step, stream_id, i, Hs, Ws, smin, smax, rmax):
    """(wf, hf) before rounding and clamping, for the statistics of the draw."""
    f = np.float32
    key, b = step_key(int(seed), int(step)), 0xFF00 + int(stream_id)
    r = lambda c, n: rand_below(key, i, b, c, n)
    U = lambda c: f(r(c, 1 << 24)) * f(2.0 ** -24)
    smin, smax, rmax = f(smin), f(smax), f(rmax)
    a = smin + (smax - smin) * U(6)
    q = f(1) + (rmax - f(1)) * U(7)
    ratio = q if r(8, 2) else f(1) / q
    A = f(Hs * Ws)
    return float(np.sqrt(a * A * ratio)), float(np.sqrt(a * A / ratio))


def center_rect(Hs, Ws, frac):
    """The centred square of side max(1, min(m, round(frac m))), m = min(Hs, Ws) (fumi_amd.dataset.image_table.center_rect)."""
    m = min(Hs, Ws)
    side = max(1, min(m, int(round(frac * m))))
    return (Ws - side) // 2, (Hs - side) // 2, side, side


def gather_images_resized(table, idx, mean, std, out_size, seed=0, step=0, stream_id=0, rect=None, scale=None, ratio=1.0,
                          flip=False, jitter=(0, 0, 0), dtype=np.float32):
    """table uint8 [n, C, Hs, Ws], idx ints (read flat; an index outside the table reads image 0) -> dtype [n_idx, C, Ho, Wo].
    ``rect`` = (x0, y0, w, h): fixed mode; ``scale`` = (lo, hi) with ``ratio`` = rmax: random mode."""
    table = np.asarray(table)
    assert table.dtype == np.uint8 and table.ndim == 4 and (rect is None) != (scale is None)
    n, C, Hs, Ws = table.shape
    Ho, Wo = out_size
    jit = (jitter,) * 3 if np.isscalar(jitter) else tuple(jitter)
    idx = np.asarray(idx).reshape(-1)
    mean_d = np.asarray(mean, dtype=np.float32).astype(dtype).reshape(C, 1, 1)
    inv_d = (np.float32(1) / np.asarray(std, dtype=np.float32)).astype(dtype).reshape(C, 1, 1)
    k = dtype(np.float32(1) / np.float32(255))
    key, b = step_key(int(seed), int(step)), 0xFF00 + int(stream_id)
    out = np.empty((len(idx), C, Ho, Wo), dtype=dtype)
    cache = {}
    for i, r in enumerate(idx):
        r = int(r) if 0 <= int(r) < n else 0
        x0, y0, w, h = rect if rect is not None else random_rect(seed, step, stream_id, i, Hs, Ws, scale[0], scale[1], ratio)
        assert 1 <= w <= Ws and 1 <= h <= Hs and 0 <= x0 <= Ws - w and 0 <= y0 <= Hs - h
        if (r, x0, y0, w, h) not in cache:
            cache[(r, x0, y0, w, h)] = resample(table[r][:, y0:y0 + h, x0:x0 + w], Ho, Wo, dtype)
        v = cache[(r, x0, y0, w, h)]
        if flip and rand_below(key, i, b, 2, 2):
            v = v[:, :, ::-1]
        v = v * k
        if any(a > 0 for a in jit):
            assert C == 3
            a = [np.float32(x) for x in jit]
            f = IR.jitter_factors(seed, step, stream_id, i, a, dtype)
            if a[0] > 0:
                v = IR._clamp01(v * f[0], dtype)
            if a[1] > 0:
                m = dtype(IR._gray(v, dtype).mean(dtype=dtype))
                v = IR._clamp01(m + f[1] * (v - m), dtype)
            if a[2] > 0:
                g = IR._gray(v, dtype)
                v = IR._clamp01(g[None] + f[2] * (v - g[None]), dtype)
        out[i] = (v - mean_d) * inv_d
    return out
