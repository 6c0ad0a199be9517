"""Float64 restatement of the clipped optimizer step's first two stages (csrc/adam.hip: grad_sumsq_kernel, clip_finish_kernel) and
the tensor lists the clip tests run on.

    norm = sqrt(sum g^2)                                   in float64 over every element of every tensor
    coef = min(1, max_norm / (fp32(norm) + 1e-6))          the fp32 formula of torch.nn.utils.clip_grad_norm_, applied to the
                                                           float64 norm rounded to fp32; written `c > 1 ? 1 : c`, so NaN stays NaN
    scaled gradient = g * coef                             in float64

Bounds the tests hold the device to (derived, not measured): the double accumulation is exact to ~1e-13; what remains for the norm
is the rounding of the sum's square root to fp32 (and a possible sqrtf): relative 2^-22.  coef adds the fp32 add of 1e-6 and one
fp32 divide, 2^-24 each: relative 2^-21."""
import numpy as np

NORM_CAP = 1024                       # csrc/adam.hip: workgroups of one sum-of-squares launch; one sweep of its loop is NORM_CAP * 1024 elements
NORM_RTOL = 2.0 ** -22
COEF_RTOL = 2.0 ** -21
SHAPES = [(256, 2048), (256,), (64, 256), (65,), (7, 3), (1,)]      # tests/test_optim_fused_gpu.py: SHAPES (the production shape)

# name -> list of (shape, offset): offset 1 = a view starting one element into a larger buffer (a pointer no 16-byte load may use)
CASES = {
    "smallest": [((1,), 0)],
    "quad_tails": [((3,), 0), ((4,), 0), ((5,), 0)],
    "boundaries_in_one_workgroup": [((1023,), 0), ((1025,), 0), ((7, 3), 0)],
    "empty_between": [((9,), 0), ((0,), 0), ((6,), 0)],
    "misaligned": [((37,), 1), ((8, 5), 0), ((130,), 1)],
    "production": [(s, 0) for s in SHAPES],
    "chunk_32": [((5,), 0)] * 32,
    "chunk_33": [((5,), 0)] * 33,
    "chunk_65": [((5,), 0)] * 65,
    "grid_stride_wraps": [((NORM_CAP * 1024 + 5,), 0)],
    # two chunks of 601 workgroups each: 1202 partials, so the finish kernel goes through its 1024-entry LDS tile twice
    "two_finish_tiles": [((600 * 1024 + 3,), 0)] + [((5,), 0)] * 31 + [((600 * 1024 + 3,), 0)],
}


def case_arrays(name, seed=0):
    """The case's gradients as float32 numpy arrays (a fixed stream per case and seed; scales differ from tensor to tensor)."""
    rng = np.random.default_rng([seed, sorted(CASES).index(name)])
    out = []
    for i, (shape, _) in enumerate(CASES[name]):
        scale = np.float32(10.0 ** ((i % 5) - 2))
        out.append((rng.standard_normal(shape).astype(np.float32) * scale).astype(np.float32))
    return out


def norm64(arrays):
    return float(np.sqrt(sum(float(np.sum(np.asarray(a, dtype=np.float64) ** 2)) for a in arrays)))


def coef32(norm, max_norm):
    """The fp32 formula on the float64 norm rounded to fp32; returns a Python float holding the fp32 value."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return float(np.float32(1.0) if c > np.float32(1.0) else c)


def scaled64(arrays, coef):
    return [np.asarray(a, dtype=np.float64) * float(coef) for a in arrays]


def norm32_numpy(arrays):
    """What plain float32 numpy makes of the same inputs (pairwise sums): shows the case table asks nothing unfair of fp32 data."""
    total = np.float32(0.0)
    for a in arrays:
        total = np.float32(total + np.sum(a * a, dtype=np.float32))
    return float(np.sqrt(total))
