"""Numpy restatement of fumi_hip_mix_images (csrc/immix.hip): the blend of a batch x float32 [M, C, H, W] with
the rows ``partner`` names.  mixup is computed in float64 from the float32 inputs with lam and u = float32(1) - lam as float32 values;
CutMix is an exact copy.  A row that is its own partner, and a row whose partner lies outside [0, M) (the kernel also sets
FUMI_ST_LABEL_RANGE), is x[i] unchanged."""
import numpy as np

MIXUP, CUTMIX = 0, 1


def mix_images(x, partner, mode, lam=1.0, box=(0, 0, 0, 0)):
    """float64 [M, C, H, W] (CutMix: the float32 values, exactly)."""
    x = np.asarray(x, dtype=np.float32)
    M = x.shape[0]
    lam32 = np.float32(lam)
    lam64, u64 = float(lam32), float(np.float32(1) - lam32)
    bx0, by0, bx1, by1 = (int(v) for v in box)
    out = x.astype(np.float64)
    for i, p in enumerate(np.asarray(partner, dtype=np.int64)):
        if p < 0 or p >= M or p == i:
            continue
        if mode == MIXUP:
            out[i] = lam64 * x[i].astype(np.float64) + u64 * x[p].astype(np.float64)
        else:
            out[i, :, by0:by1, bx0:bx1] = x[p, :, by0:by1, bx0:bx1]
    return out
