"""Float64 numpy restatement of the soft-target form of the fused classification head (fumi_hip_cls_head_step_soft,
csrc/clshead.hip).  With u = 1 - lam,

    t[m,c] = (1 - eps) * (lam * [c == y_a[m]] + u * [c == y_b[m]]) + eps / C
    loss = mean_m (lse_m - sum_c t[m,c] z[m,c]),   dlogits = grad_scale / M * (softmax - t)

dfeats, gW and gb follow from dlogits as in tests/cls_head_ref.py; ``correct`` counts the rows whose first arg-max equals y_a.
y_b None means y_b = y_a.  lam, u and eps are taken in float64 as given: the entry's float32 roundings of them (at most 2^-24 relative
each) are part of the error the GPU test bounds.  A label outside [0, C) in y_a or y_b marks its row invalid: the row adds nothing to the loss, the count or
the gradients, the divisor stays M, ``status`` carries FUMI_ST_LABEL_RANGE."""
import numpy as np

from cls_head_ref import ST_LABEL_RANGE


def cls_head_soft_ref(feats, y_a, W, b, grad_scale=1.0, y_b=None, lam=1.0, smoothing=0.0):
    """The keys of cls_head_ref: dict(loss, correct, preds [M], logits [M,C], margin [M], dlogits, dfeats, gW, gb, status)."""
    x = np.asarray(feats, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    ya = np.asarray(y_a, dtype=np.int64)
    yb = ya if y_b is None else np.asarray(y_b, dtype=np.int64)
    lam, eps = float(lam), float(smoothing)
    u = 1.0 - lam
    M, C = x.shape[0], W.shape[0]
    z = x @ W.T + b
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    lse = (mx + np.log(s))[:, 0]
    preds = z.argmax(axis=1)
    top2 = np.sort(z, axis=1)[:, -2:]
    ok = (ya >= 0) & (ya < C) & (yb >= 0) & (yb < C)
    yac, ybc = np.where(ok, ya, 0), np.where(ok, yb, 0)
    rows = np.arange(M)
    hot = np.zeros_like(z)
    np.add.at(hot, (rows, yac), lam)
    np.add.at(hot, (rows, ybc), u)
    t = (1.0 - eps) * hot + eps / C
    row_loss = np.where(ok, lse - (t * z).sum(axis=1), 0.0)
    dlogits = (p - t) * ok[:, None] * (float(grad_scale) / M)
    return dict(loss=row_loss.sum() / M, correct=float(((preds == ya) & ok).sum()), preds=preds, logits=z,
                margin=top2[:, 1] - top2[:, 0], dlogits=dlogits, dfeats=dlogits @ W, gW=dlogits.T @ x, gb=dlogits.sum(axis=0),
                status=0 if ok.all() else ST_LABEL_RANGE)
