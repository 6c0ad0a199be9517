"""The inputs of tests/test_cos_cls_head_gpu.py, kept apart so that the CPU suite can check them too
(tests/test_cos_cls_head_cpu.py counts the rows the GPU test sets aside).  Seeded per shape as tests/test_cls_head_gpu.py seeds its
cases.  ``plain``: standard normal features and class weights; ``offset``: 8.0 added to every feature (post-ReLU features share a
large mean direction) and every row scaled by a power of ten between 1e-3 and 1e3, so that only the normalisation makes the rows
comparable."""
import torch

# (M, F, C): one row, one k-step; a ragged second tile; C one past a 128-column product pass; the ResNet-12 width, more than two row
# tiles plus a tail; the Conv4 width (13 feature blocks, the last a short one); the widest image
SHAPES = [(1, 32, 2), (17, 96, 5), (33, 64, 129), (130, 640, 64), (64, 1600, 100), (40, 64, 1024)]
INPUTS = ("plain", "offset")
TARGETS = {"hard": dict(smoothing=0.0, lam=1.0, mixed=False), "soft": dict(smoothing=0.1, lam=0.3, mixed=True)}
TAU = 10.0
GRAD_SCALE = 0.25
TOL, MARGIN = 1e-4, 1e-5           # tests/test_cls_head_gpu.py
MAX_SET_ASIDE = 0.01               # of a case's rows may lie under MARGIN


def case(M, F, C, inputs="plain"):
    """(feats [M,F], y [M], W [C,F], tau [1]) on the host."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * F + C)
    x = torch.randn(M, F, generator=g)
    W = torch.randn(C, F, generator=g) * (2.0 / F ** 0.5)
    y = torch.randint(0, C, (M,), generator=g)
    if inputs == "offset":
        x = (x + 8.0) * 10.0 ** (6.0 * torch.rand(M, 1, generator=g) - 3.0)
    return x, y, W, torch.tensor([TAU])


def second_labels(y, M, F, C):
    """A permutation of y that leaves at least one row with y_a == y_b (row 0 keeps its place)."""
    g = torch.Generator().manual_seed(7919 * M + 31 * F + C)
    perm = torch.cat((torch.zeros(1, dtype=torch.int64), 1 + torch.randperm(M - 1, generator=g)))
    return y[perm]


def target_kw(name, y, M, F, C):
    """The keyword arguments (y_b, lam, smoothing) of the target ``name``, y_b on the host."""
    t = TARGETS[name]
    return dict(y_b=second_labels(y, M, F, C) if t["mixed"] else None, lam=t["lam"], smoothing=t["smoothing"])
