"""TEST INFRASTRUCTURE: numpy restatement of fumi_hip_gather_images (fumi_amd/csrc/imgather.hip; the semantics are written out in
include/fumi_hip.h).  Integer work (draws, source pixels) is exact; the float work is done in ``dtype``, one rounding per
operation in the kernel's order, so with the jitter off the float32 form IS the kernel's result bit for bit.  With the jitter on
the float32 form differs from the kernel only in the order of the gray-mean sum (numpy's pairwise float32 sum here); the float64
form is the yardstick both are held to."""
import numpy as np

from oracle.sampler_ref import mix, step_key, rand_below  # noqa: F401  (mix: re-exported for the tests of the hash)


def draws(seed, step, stream_id, i, pad, flip):
    """(ox, oy, fl) of output image i."""
    key = step_key(int(seed), int(step))
    b = 0xFF00 + int(stream_id)
    ox = rand_below(key, i, b, 0, 2 * pad + 1) if pad > 0 else pad
    oy = rand_below(key, i, b, 1, 2 * pad + 1) if pad > 0 else pad
    fl = rand_below(key, i, b, 2, 2) if flip else 0
    return int(ox), int(oy), int(fl)


def jitter_factors(seed, step, stream_id, i, jitter, dtype=np.float32):
    """f_j = 1 + a_j (2 u_j - 1), u_j = r(3 + j, 2^24) 2^-24, in ``dtype`` (u_j and 2 u_j - 1 are exact in float32)."""
    key = step_key(int(seed), int(step))
    out = []
    for j in range(3):
        u = dtype(rand_below(key, i, 0xFF00 + int(stream_id), 3 + j, 1 << 24)) * dtype(2.0 ** -24)
        out.append(dtype(1) + dtype(jitter[j]) * (dtype(2) * u - dtype(1)))
    return out


def source_window(img, ox, oy, fl, pad):
    """The H x W window of bytes the output image is made of: zero padding, crop at (oy, ox), then the horizontal flip."""
    C, H, W = img.shape
    x, y = np.arange(W), np.arange(H)
    sx = (W - 1 - x if fl else x) + ox - pad
    sy = y + oy - pad
    ok = ((sy >= 0) & (sy < H))[:, None] & ((sx >= 0) & (sx < W))[None, :]
    win = img[:, np.clip(sy, 0, H - 1)[:, None], np.clip(sx, 0, W - 1)[None, :]]
    return np.where(ok[None], win, 0).astype(np.uint8)


def _clamp01(v, dtype):
    return np.minimum(np.maximum(v, dtype(0)), dtype(1))


def _gray(v, dtype):
    return dtype(0.299) * v[0] + dtype(0.587) * v[1] + dtype(0.114) * v[2]


def gather_images(table, idx, mean, std, seed=0, step=0, stream_id=0, pad=0, flip=False, jitter=(0, 0, 0), dtype=np.float32):
    """table uint8 [n, C, H, W], idx ints (read flat; an index outside the table reads image 0) -> dtype [n_idx, C, H, W].
    mean / std as hip.gather_images takes them: the kernel multiplies by inv_std = fl32(1) / fl32(std)."""
    table = np.asarray(table)
    assert table.dtype == np.uint8 and table.ndim == 4
    n, C, H, W = table.shape
    jit = (jitter,) * 3 if np.isscalar(jitter) else tuple(jitter)
    idx = np.asarray(idx).reshape(-1)
    mean_d = np.asarray(mean, dtype=np.float32).astype(dtype).reshape(C, 1, 1)
    inv_d = (np.float32(1) / np.asarray(std, dtype=np.float32)).astype(dtype).reshape(C, 1, 1)
    k = dtype(np.float32(1) / np.float32(255))               # the fp32 nearest to 1 / 255, in both forms
    out = np.empty((len(idx), C, H, W), dtype=dtype)
    for i, r in enumerate(idx):
        r = int(r) if 0 <= int(r) < n else 0
        ox, oy, fl = draws(seed, step, stream_id, i, pad, flip)
        v = source_window(table[r], ox, oy, fl, pad).astype(dtype) * k
        if any(a > 0 for a in jit):
            assert C == 3
            a = [np.float32(x) for x in jit]                  # the amplitudes cross the ABI as floats
            f = jitter_factors(seed, step, stream_id, i, a, dtype)
            if a[0] > 0:
                v = _clamp01(v * f[0], dtype)
            if a[1] > 0:
                m = dtype(_gray(v, dtype).mean(dtype=dtype))
                v = _clamp01(m + f[1] * (v - m), dtype)
            if a[2] > 0:
                g = _gray(v, dtype)
                v = _clamp01(g[None] + f[2] * (v - g[None]), dtype)
        out[i] = (v - mean_d) * inv_d
    return out
