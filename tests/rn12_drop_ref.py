"""Reference of the DropBlock / dropout pass of the bf16 ResNet-12 (fumi_amd/csrc/rn12_drop.hip), in numpy and
torch float64.

Two parts.  The integer part restates the mask bit for bit: the chained 32-bit counter mix, the seed test against the host's
integer threshold, the dilation of the seeds into dropped blocks, the integer kept count of one batch-statistics group and the fp32
scale total / kept; ``apply_map`` is the kernel's in-place product on a bf16 "padded channels-last" map (fp32 product, bf16
round-to-nearest-even).  The floating part is a float64 autograd ResNet-12 written from the docstring of fumi_amd/models/resnet12.py
(four-convolution residual blocks, LeakyReLU 0.1, batch statistics per group, no conv bias, 2 x 2 max-pool, global average pool)
with ``keep * scale`` multiplied in after each block's pool."""
import numpy as np
import torch
import torch.nn.functional as F

M32 = 0xFFFFFFFF
G1, G2, G3, G4 = 0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F


def mix(x):
    """The counter mix of the engine's dropout masks on uint64 arrays holding 32-bit values."""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & np.uint64(M32)
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def plan(H, W, rate, block):
    """(effective block size, integer threshold) as the host computes them: bs = min(block, H, W), thr = floor(gamma 2^32) in double."""
    bs = min(int(block), H, W)
    gamma = float(np.float32(rate)) / (bs * bs) * (H * W) / ((H - bs + 1) * (W - bs + 1))
    return bs, int(min(gamma * 4294967296.0, 4294967295.0))


def seeds(seed, blk, set_index, e, M, C, Hs, Ws, thr):
    """Seed bits [M, C, Hs, Ws] (bool) of global episode ``e``: seed (i, j) of plane (m, c) is set iff its hash is below thr."""
    u = lambda v: np.uint64(int(v) & M32)
    k = mix(np.array(u(seed) ^ u(G1 * (2 * blk + set_index + 1)), dtype=np.uint64))
    k = mix(k ^ u(int(seed) >> 32))
    k = mix((k + u(G2 * e)) & np.uint64(M32))
    m = np.arange(M, dtype=np.uint64)
    k0 = mix(k ^ ((m * np.uint64(G3)) & np.uint64(M32)))                                   # [M]
    c1 = np.arange(1, C + 1, dtype=np.uint64)
    k1 = mix(k0[:, None] ^ ((c1 * np.uint64(G4)) & np.uint64(M32))[None, :])               # [M, C]
    pos = (np.arange(Hs, dtype=np.uint64)[:, None] << np.uint64(16)) | np.arange(Ws, dtype=np.uint64)[None, :]
    h = mix(mix(k0[:, None, None, None] ^ pos[None, None]) ^ k1[:, :, None, None])
    return h < np.uint64(thr)


def dilate(s, bs, H, W):
    """Dropped cells [..., H, W] from seed planes [..., H-bs+1, W-bs+1]: seed (i, j) drops [i, i+bs) x [j, j+bs), by shift-ORs along
    the row and then down the rows (the kernel's order)."""
    Hs, Ws = H - bs + 1, W - bs + 1
    assert s.shape[-2:] == (Hs, Ws)
    row = np.zeros(s.shape[:-1] + (W,), dtype=bool)
    for k in range(bs):
        row[..., k:k + Ws] |= s
    out = np.zeros(s.shape[:-2] + (H, W), dtype=bool)
    for k in range(bs):
        out[..., k:k + Hs, :] |= row
    return out


def dilate_brute(s, bs, H, W):
    """The definition: a cell is dropped iff any seed lies within reach."""
    Hs, Ws = H - bs + 1, W - bs + 1
    out = np.zeros(s.shape[:-2] + (H, W), dtype=bool)
    for r in range(H):
        for c in range(W):
            for i in range(max(0, r - bs + 1), min(Hs, r + 1)):
                for j in range(max(0, c - bs + 1), min(Ws, c + 1)):
                    out[..., r, c] |= s[..., i, j]
    return out


def keep_mask(seed, blk, set_index, e, M, C, H, W, rate, block):
    """keep [M, C, H, W] (bool) of one group (global episode e, support 0 / query 1) at block ``blk``."""
    bs, thr = plan(H, W, rate, block)
    s = seeds(seed, blk, set_index, e, M, C, H - bs + 1, W - bs + 1, thr)
    return ~dilate(s, bs, H, W)


def kept_scale(keep):
    """(kept: int, scale: np.float32) of one group: scale = (float)total / (float)kept in fp32, 0 when nothing is kept."""
    kept = int(keep.sum())
    return kept, (np.float32(keep.size) / np.float32(kept) if kept else np.float32(0.0))


def bf16_bits_to_f32(b):
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16_bits(f):
    """fp32 -> bf16 bits, round to nearest even (finite values)."""
    u = np.asarray(f, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def apply_map(bits, M, H, W, rate, block, seed, blk, set_index, b0):
    """The kernel on a padded channels-last map of bf16 bit patterns [B, M (H+2)(W+2), C] (uint16): (out bits, kept [B] int64,
    scale [B] fp32).  Borders are passed through untouched."""
    B, _, C = bits.shape
    x = bits.reshape(B, M, H + 2, W + 2, C).copy()
    kept, scale = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.float32)
    for b in range(B):
        keep = keep_mask(seed, blk, set_index, b0 + b, M, C, H, W, rate, block).transpose(0, 2, 3, 1)       # [M, H, W, C]
        kept[b], scale[b] = kept_scale(keep)
        inner = x[b, :, 1:H + 1, 1:W + 1, :]
        prod = f32_to_bf16_bits(bf16_bits_to_f32(inner) * scale[b])
        x[b, :, 1:H + 1, 1:W + 1, :] = np.where(keep, prod, np.uint16(0))
    return x.reshape(bits.shape), kept, scale


# ---- the float64 network ---------------------------------------------------------------------------------------------------------------
def make_theta(seed, cin, channels):
    """12 fp32 tensors per block in the engine's order (W1,g1,b1, W2,g2,b2, W3,g3,b3, Ws,gs,bs)."""
    g = torch.Generator().manual_seed(seed)
    th, ci = [], cin
    for c in channels:
        for k, (ki, ks) in enumerate(((ci, 3), (c, 3), (c, 3), (ci, 1))):
            th.append(torch.randn(c, ki, ks, ks, generator=g) * (2.0 / (ki * ks * ks)) ** 0.5)
            th.append(1.0 + 0.1 * torch.randn(c, generator=g))
            th.append(0.1 * torch.randn(c, generator=g))
        ci = c
    return th


def _bn(u, g, b):
    mu = u.mean((0, 2, 3), keepdim=True)
    var = ((u - mu) ** 2).mean((0, 2, 3), keepdim=True)
    return (u - mu) / torch.sqrt(var + 1e-5) * g[None, :, None, None] + b[None, :, None, None]


def features(x, theta, masks=None):
    """Features [M, C_last] of ONE group x [M, Cin, H, W] (float64; batch statistics over its M images).  masks: per block None or a
    float64 tensor [M, C, H_l, W_l] = keep * scale multiplied into the block's pooled output."""
    h = x
    for l in range(len(theta) // 12):
        W1, g1, b1, W2, g2, b2, W3, g3, b3, Ws, gs, bs = theta[12 * l:12 * l + 12]
        a = F.leaky_relu(_bn(F.conv2d(h, W1, padding=1), g1, b1), 0.1)
        a = F.leaky_relu(_bn(F.conv2d(a, W2, padding=1), g2, b2), 0.1)
        o = F.leaky_relu(_bn(F.conv2d(a, W3, padding=1), g3, b3) + _bn(F.conv2d(h, Ws), gs, bs), 0.1)
        h = F.max_pool2d(o, 2)
        if masks is not None and masks[l] is not None:
            h = h * masks[l]
    return h.mean((2, 3))


def group_masks(seed, set_index, e, M, channels, H, W, rates, blocks):
    """The float64 ``keep * scale`` tensors of one group for every block (None where the rate is 0); H, W: the image size."""
    out = []
    for l, c in enumerate(channels):
        H, W = H // 2, W // 2
        if not rates[l] > 0:
            out.append(None)
            continue
        keep = keep_mask(seed, l, set_index, e, M, c, H, W, rates[l], blocks[l])
        _, scale = kept_scale(keep)
        out.append(torch.from_numpy(keep.astype(np.float64)) * float(scale))
    return out


def encode_pair_ref(x_s, x_q, theta, dfs, dfq, rates=None, blocks=None, seed=0):
    """(feats_s [B,S,F], feats_q [B,Qn,F], gradients of sum <dfeats, feats> w.r.t. theta) in float64 autograd."""
    th = [t.double().clone().requires_grad_(True) for t in theta]
    channels = [int(th[12 * l].shape[0]) for l in range(len(th) // 12)]
    B = x_s.shape[0]
    fs, fq = [], []
    for b in range(B):
        for set_index, (x, acc) in enumerate(((x_s[b], fs), (x_q[b], fq))):
            masks = None
            if rates is not None:
                masks = group_masks(seed, set_index, b, x.shape[0], channels, x.shape[-2], x.shape[-1], rates, blocks)
            acc.append(features(x.double(), th, masks))
    fs, fq = torch.stack(fs), torch.stack(fq)
    obj = (fs * dfs.double()).sum() + (fq * dfq.double()).sum()
    return fs.detach(), fq.detach(), [g for g in torch.autograd.grad(obj, th)]
