"""Float64 numpy restatement of the fused classification head (fumi_hip_cls_head_step, csrc/clshead.hip):
F.cross_entropy(feats @ W.T + b, y) with mean reduction, its first arg-max predictions and the gradients of grad_scale * loss.

A label outside [0, C) marks its row invalid: the row adds nothing to the loss, the correct count or the gradients, and the divisor
stays M (the kernel also sets FUMI_ST_LABEL_RANGE; ``status`` below is that bit)."""
import numpy as np

ST_LABEL_RANGE = 1


def cls_head_ref(feats, y, W, b, grad_scale=1.0):
    """dict(loss, correct, preds [M], logits [M,C], margin [M] (top-two logit gap), dlogits, dfeats, gW, gb, status), all float64."""
    x = np.asarray(feats, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    M, C = x.shape[0], W.shape[0]
    z = x @ W.T + b
    mx = z.max(axis=1, keepdims=True)
    e = np.exp(z - mx)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    lse = (mx + np.log(s))[:, 0]
    preds = z.argmax(axis=1)                                   # numpy's argmax is the first one, like torch.max
    top2 = np.sort(z, axis=1)[:, -2:]
    ok = (y >= 0) & (y < C)
    yc = np.where(ok, y, 0)
    nll = np.where(ok, lse - z[np.arange(M), yc], 0.0)
    onehot = np.zeros_like(z)
    onehot[np.arange(M), yc] = 1.0
    dlogits = (p - onehot) * ok[:, None] * (float(grad_scale) / M)
    return dict(loss=nll.sum() / M, correct=float(((preds == y) & ok).sum()), preds=preds, logits=z, margin=top2[:, 1] - top2[:, 0],
                dlogits=dlogits, dfeats=dlogits @ W, gW=dlogits.T @ x, gb=dlogits.sum(axis=0),
                status=0 if ok.all() else ST_LABEL_RANGE)
