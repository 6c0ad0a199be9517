"""Float64 numpy restatement of the fused logistic-regression head (fumi_hip_logreg_head_step, csrc/logreghead.hip), in the dual form
the kernel iterates.  This is the definition the kernel is held to; tests/test_logreg_head_cpu.py ties it to heavy-ball descent on the
primal objective under torch.autograd at 1e-10.

Per episode, with X the support rows [S,F], x~_i = x_i / max(|x_i|, 1e-12) when ``normalize`` (the query rows alike), n the number of
support rows with a label in [0, N) (at least 1) and wd = 1 / (C n):
    f(W, b) = (1/n) sum_i CE(W^T x~_i + b, y_i) + (wd/2) |W|^2,
T steps of V <- beta V + grad, (W, b) <- (W, b) - eta V from zero.  Every iterate is W_t = X~^T A_t, so with K~ = X~ X~^T one step is
    Z = K~ A + 1 b^T,  P = softmax_rows(Z),  R = (P - Y) / n,  VA <- beta VA + R + wd A,  Vb <- beta Vb + colsum(R),
    A <- A - eta VA,  b <- b - eta Vb,
and the query logits are z = Fq~ X~^T A_T + b_T.

A query label outside [0, N) sets ST_LABEL_RANGE: the row adds nothing to the loss or the count (the divisor stays B * Qn).  A support
label outside [0, N) sets the same bit and the row is left out exactly: its row and column of K~ and its rows of Y and R are zero and it
does not count in n.  A class without a support row sets ST_CLASS_MISSING and is fitted like any class."""
import numpy as np

from ridge_head_ref import SHAPES, case_inputs  # noqa: F401  (the ridge table and its seeded inputs)

ST_LABEL_RANGE, ST_CLASS_MISSING = 1, 2

LR, MOMENTUM, C_REG = 1.0, 0.9, 1.0           # the hyper-parameters of the parity tests (the defaults of the flags)
STEPS = (3, 100)

# (shape, steps, momentum, normalize): every shape at both step counts, momentum 0 on the two smallest, raw features on (2,7,33,3,96)
CASES = ([(s, t, MOMENTUM, True) for s in SHAPES for t in STEPS]
         + [(s, t, 0.0, True) for s in SHAPES[:2] for t in STEPS]
         + [(SHAPES[1], t, MOMENTUM, False) for t in STEPS])


def _softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def logreg_head_ref(feats_s, y_s, feats_q, y_q, n_way, steps=100, lr=LR, momentum=MOMENTUM, C=C_REG, normalize=True, dtype=np.float64):
    """dict(loss, correct, preds [B,Qn], logits [B,Qn,N], margin [B,Qn] (top-two logit gap), status, A [B,S,N], b [B,N], grad_norm (the
    largest norm over the episodes of the objective's gradient at (W_T, b_T))).  ``dtype`` float32 runs the same iteration in plain
    float32 numpy (the CPU test's measure of what fp32 can reach)."""
    dt = np.dtype(dtype).type
    ys = np.asarray(y_s, dtype=np.int64)
    yq = np.asarray(y_q, dtype=np.int64)
    N = int(n_way)
    ok_s = (ys >= 0) & (ys < N)
    ok_q = (yq >= 0) & (yq < N)
    xs = np.asarray(feats_s).astype(dtype)
    xq = np.asarray(feats_q).astype(dtype)
    B, S, F = xs.shape
    Qn = xq.shape[1]
    Y = np.zeros((B, S, N), dtype=dtype)
    bi, si = np.nonzero(ok_s)
    Y[bi, si, ys[bi, si]] = 1
    status = (0 if ok_s.all() and ok_q.all() else ST_LABEL_RANGE) | (ST_CLASS_MISSING if (Y.sum(axis=1) == 0).any() else 0)
    K = np.einsum("bsf,btf->bst", xs, xs)
    if normalize:
        inv_s = (1 / np.maximum(np.sqrt(np.einsum("bss->bs", K)), dt(1e-12))).astype(dtype)
        inv_q = (1 / np.maximum(np.sqrt((xq * xq).sum(-1)), dt(1e-12))).astype(dtype)
    else:
        inv_s, inv_q = np.ones((B, S), dtype=dtype), np.ones((B, Qn), dtype=dtype)
    inv_s = np.where(ok_s, inv_s, 0).astype(dtype)                                   # a row left out: zero row and column of K~
    Kt = K * inv_s[:, :, None] * inv_s[:, None, :]
    n = np.maximum(ok_s.sum(axis=1), 1).astype(dtype)[:, None, None]
    wd = (1 / (dt(C) * n)).astype(dtype)
    eta, beta = dt(lr), dt(momentum)
    A = np.zeros((B, S, N), dtype=dtype); VA = np.zeros_like(A)
    b = np.zeros((B, 1, N), dtype=dtype); Vb = np.zeros_like(b)
    okm = ok_s[..., None]

    def residual(A, b):
        return (np.where(okm, _softmax(Kt @ A + b) - Y, 0) / n).astype(dtype)
    for _ in range(int(steps)):
        R = residual(A, b)
        VA = beta * VA + R + wd * A
        Vb = beta * Vb + R.sum(axis=1, keepdims=True)
        A = A - eta * VA
        b = b - eta * Vb
    R = residual(A, b)
    G = R + wd * A
    gn = np.sqrt(np.maximum(np.einsum("bsn,bst,btn->b", G, Kt, G), 0) + (R.sum(axis=1) ** 2).sum(-1))
    z = np.einsum("bqf,bsf,bsn->bqn", xq, xs, A * inv_s[..., None]) * inv_q[..., None] + b
    mx = z.max(axis=-1, keepdims=True)
    lse = (mx + np.log(np.exp(z - mx).sum(axis=-1, keepdims=True)))[..., 0]
    preds = z.argmax(axis=-1)                                                      # numpy's argmax is the first one, like torch.max
    top2 = np.sort(z, axis=-1)[..., -2:]
    yc = np.where(ok_q, yq, 0)
    z_y = np.take_along_axis(z, yc[..., None], axis=-1)[..., 0]
    loss = np.where(ok_q, lse - z_y, 0).sum() / (B * Qn)
    return dict(loss=float(loss), correct=float(((preds == yq) & ok_q).sum()), preds=preds, logits=z, margin=top2[..., 1] - top2[..., 0],
                status=int(status), A=A, b=b[:, 0], grad_norm=float(gn.max()))
