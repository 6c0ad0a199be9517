"""Float64 numpy restatement of the fused ridge-regression head (fumi_hip_ridge_head_step, csrc/ridgehead.hip).  This is the
definition the kernel is held to; tests/test_ridge_head_cpu.py ties it to torch.autograd at 1e-10.

Per episode b, with X = feats_s[b] [S,F], Y = onehot(y_s[b]) [S,N], Fq = feats_q[b] [Qn,F], lam = exp(rho), params = (rho, alpha):
    M = X X^T + lam I,   A = M^-1 Y,   W = X^T A,   u = Fq W,   z = alpha u,
loss = mean over all B * Qn query rows of the softmax cross-entropy of z against y_q.  Gradients are those of grad_scale * loss:
    dz = grad_scale / (B Qn) (softmax(z) - onehot(y_q)),   dFq = alpha dz W^T,   dW = alpha Fq^T dz,   G = M^-1 (X dW),
    dX = A (dW - X^T G)^T - G W^T,   dalpha = sum dz * u,   drho = -lam sum G * A.

A query label outside [0, N) sets ST_LABEL_RANGE: the row adds nothing to the loss, the count or any gradient (the divisor stays
B * Qn).  A support label outside [0, N) sets the same bit and the row is left out exactly: its feature row is read as zero and its
row of Y is zero.  A class without a support row sets ST_CLASS_MISSING and has logits 0.  A pivot of the Cholesky factorisation that
is not > 0 sets ST_NOT_POSDEF (here: an M that is not positive definite, or not finite)."""
import numpy as np

ST_LABEL_RANGE, ST_CLASS_MISSING, ST_NOT_POSDEF = 1, 2, 8

RHO, ALPHA, GRAD_SCALE = 0.0, 4.0, 0.25       # the parameters of the parity tests

# (B, S, Qn, N, F): the smallest of everything; off every tile edge; 20-way 5-shot at the ResNet-12 width; the Conv4 width; both limits
# with S > F; the feature limit; S just past a 32-row edge with S > F
SHAPES = [(1, 2, 1, 2, 32), (2, 7, 33, 3, 96), (2, 100, 130, 20, 640), (1, 25, 17, 5, 1600), (1, 128, 18, 64, 64), (3, 10, 16, 5, 2048),
          (1, 33, 16, 3, 32)]


def case_inputs(B, S, Qn, N, F):
    """The seeded inputs of the parity tests: class means mu ~ N(0, 1) [B,N,F], rows (0.5 mu[y] + N(0, 1)) / sqrt(F), y_s =
    arange(S) % N with the last row set to class 0 when S > N (unequal class counts), y_q uniform.  float32 features, int64 labels."""
    rs = np.random.RandomState(100003 * B + 10007 * S + 1009 * Qn + 101 * N + F + 7)
    mu = rs.standard_normal((B, N, F))
    y_s = np.tile(np.arange(S) % N, (B, 1)).astype(np.int64)
    if S > N:
        y_s[:, -1] = 0
    y_q = rs.randint(0, N, (B, Qn)).astype(np.int64)
    bi = np.arange(B)[:, None]
    f_s = ((0.5 * mu[bi, y_s] + rs.standard_normal((B, S, F))) / np.sqrt(F)).astype(np.float32)
    f_q = ((0.5 * mu[bi, y_q] + rs.standard_normal((B, Qn, F))) / np.sqrt(F)).astype(np.float32)
    return f_s, y_s, f_q, y_q


def ridge_head_ref(feats_s, y_s, feats_q, y_q, params, n_way, grad_scale=1.0):
    """dict(loss, correct, preds [B,Qn], logits [B,Qn,N], margin [B,Qn] (top-two logit gap), dfeats_s, dfeats_q, dparams [2], status,
    cond (largest eigmax / eigmin of M over the episodes), A [B,S,N], W [B,F,N]), all float64."""
    ys = np.asarray(y_s, dtype=np.int64)
    yq = np.asarray(y_q, dtype=np.int64)
    rho, alpha = (float(v) for v in np.asarray(params, dtype=np.float64).reshape(-1)[:2])
    lam = np.exp(rho)
    N = int(n_way)
    ok_s = (ys >= 0) & (ys < N)
    ok_q = (yq >= 0) & (yq < N)
    xs = np.asarray(feats_s, dtype=np.float64)
    xs = np.where(ok_s[..., None], xs, 0.0)                                        # a row left out is read as zero
    xq = np.asarray(feats_q, dtype=np.float64)
    B, S, F = xs.shape
    Qn = xq.shape[1]
    Y = np.zeros((B, S, N))
    bi, si = np.nonzero(ok_s)
    Y[bi, si, ys[bi, si]] = 1.0
    status = (0 if ok_s.all() and ok_q.all() else ST_LABEL_RANGE) | (ST_CLASS_MISSING if (Y.sum(axis=1) == 0).any() else 0)
    M = np.einsum("bsf,btf->bst", xs, xs) + lam * np.eye(S)[None]
    cond = 0.0
    if np.isfinite(M).all():
        ev = np.linalg.eigvalsh(M)
        if ev.min() <= 0:
            status |= ST_NOT_POSDEF
        else:
            cond = float((ev[:, -1] / ev[:, 0]).max())
    else:
        status |= ST_NOT_POSDEF
    A = np.linalg.solve(M, Y)
    W = np.einsum("bsf,bsn->bfn", xs, A)
    u = np.einsum("bqf,bfn->bqn", xq, W)
    z = alpha * u
    mx = z.max(axis=-1, keepdims=True)
    e = np.exp(z - mx)
    s = e.sum(axis=-1, keepdims=True)
    lse = (mx + np.log(s))[..., 0]
    preds = z.argmax(axis=-1)                                                      # numpy's argmax is the first one, like torch.max
    top2 = np.sort(z, axis=-1)[..., -2:]
    yc = np.where(ok_q, yq, 0)
    z_y = np.take_along_axis(z, yc[..., None], axis=-1)[..., 0]
    Mq = B * Qn
    loss = np.where(ok_q, lse - z_y, 0.0).sum() / Mq
    onehot_q = np.zeros_like(z)
    np.put_along_axis(onehot_q, yc[..., None], 1.0, axis=-1)
    dz = (e / s - onehot_q) * ok_q[..., None] * (float(grad_scale) / Mq)
    dfeats_q = alpha * np.einsum("bqn,bfn->bqf", dz, W)
    dW = alpha * np.einsum("bqf,bqn->bfn", xq, dz)
    G = np.linalg.solve(M, np.einsum("bsf,bfn->bsn", xs, dW))
    dfeats_s = np.einsum("bsn,bfn->bsf", A, dW - np.einsum("bsf,bsn->bfn", xs, G)) - np.einsum("bsn,bfn->bsf", G, W)
    dparams = np.array([-lam * (G * A).sum(), (dz * u).sum()])
    return dict(loss=loss, correct=float(((preds == yq) & ok_q).sum()), preds=preds, logits=z, margin=top2[..., 1] - top2[..., 0],
                dfeats_s=dfeats_s, dfeats_q=dfeats_q, dparams=dparams, status=int(status), cond=cond, A=A, W=W)
