"""The inputs of tests/test_cls_head_distill_gpu.py, kept apart so that the CPU suite can check them too
(tests/test_cls_head_distill_cpu.py counts the rows the GPU test sets aside): per shape a student of logit standard deviation ~2, as
in tests/test_cls_head_gpu.py, and a teacher that is a perturbed copy of it, so that some rows agree with the student and some do not."""
import torch

# (M, F, C): one row; a ragged last tile and C below one MFMA tile; the ResNet-12 width with C % 128 != 0 and more than one full tile;
# C at the limit, where the LDS image is largest
SHAPES = [(1, 32, 2), (33, 96, 5), (130, 640, 64), (257, 64, 1024)]
# (T, alpha, ce_weight, eps, lam, with y_b)
CONFIGS = [(4.0, 0.5, 0.5, 0.0, 1.0, False), (1.0, 1.0, 0.0, 0.0, 1.0, False), (2.0, 0.9, 0.1, 0.1, 0.3, True)]
GRAD_SCALE = 0.25
TOL = 1e-4                      # the existing head's bound: 1e-4 of the compared tensor's largest magnitude
GAP = 2e-4                      # rows whose float64 top-two gap in z or z_t is below GAP * max|z| are set aside for preds / correct / agree
MAX_SET_ASIDE = 2


def case(M, F, C):
    """dict(x, y, W, b, x_t, W_t, b_t, y_b) of CPU float32 / int64 tensors, seeded per shape.  The seed's offset is one at which no
    shape has more than MAX_SET_ASIDE near-ties among its rows (257 rows of 1024 logits have 1.4 on average; the CPU suite counts)."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * F + C + 53)
    x = torch.randn(M, F, generator=g)
    W = torch.randn(C, F, generator=g) * (2.0 / F ** 0.5)
    b = 0.5 * torch.randn(C, generator=g)
    y = torch.randint(0, C, (M,), generator=g)
    x_t = x + 0.5 * torch.randn(M, F, generator=g)
    W_t = W + torch.randn(C, F, generator=g) * (0.5 / F ** 0.5)
    b_t = b + 0.25 * torch.randn(C, generator=g)
    perm = torch.cat((torch.zeros(1, dtype=torch.int64), 1 + torch.randperm(M - 1, generator=g)))   # row 0 keeps its label
    return dict(x=x, y=y, W=W, b=b, x_t=x_t, W_t=W_t, b_t=b_t, y_b=y[perm])


def set_aside(ref):
    """Rows of a cls_head_distill_ref result whose student or teacher arg-max float32 arithmetic may legitimately flip."""
    scale = GAP * abs(ref["logits"]).max()
    return (ref["margin"] < scale) | (ref["margin_t"] < scale)
