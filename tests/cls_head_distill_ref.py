"""Float64 numpy restatement of the distillation form of the fused classification head (fumi_hip_cls_head_step_distill,
csrc/clshead.hip).  With z = feats W^T + b, z_t = feats_t W_t^T + b_t, p = softmax(z_t / T), q = softmax(z / T)
and t the soft target of tests/cls_head_soft_ref.py,

    ce_m = lse(z_m) - sum_c t z                                   loss_ce = mean_m ce_m
    kl_m = sum_c p (z_t / T) - lse(z_t / T) - sum_c p (z / T) + lse(z / T)     loss_kd = T^2 mean_m kl_m
    loss = ce_weight * loss_ce + alpha * loss_kd
    dlogits = grad_scale / M * (ce_weight (softmax(z) - t) + alpha T (q - p))

No logarithm of a probability is taken, so a peaked teacher gives finite values.  dfeats, gW and gb follow from dlogits as in
tests/cls_head_ref.py; nothing of the teacher has a gradient.  ``correct`` and ``preds`` are the soft form's; ``agree`` counts the rows
whose first arg-max of z equals the first arg-max of z_t.  A label outside [0, C) in y_a or y_b marks its row invalid: it adds nothing
to either loss, to ``correct``, to ``agree`` or to any gradient, the divisor stays M, ``status`` carries FUMI_ST_LABEL_RANGE."""
import numpy as np

from cls_head_ref import ST_LABEL_RANGE
from cls_head_soft_ref import cls_head_soft_ref


def _lse(a):
    mx = a.max(axis=1, keepdims=True)
    return (mx + np.log(np.exp(a - mx).sum(axis=1, keepdims=True)))[:, 0]


def cls_head_distill_ref(feats, y_a, W, b, feats_t, W_t, b_t, T, alpha, ce_weight, grad_scale=1.0, y_b=None, lam=1.0, smoothing=0.0):
    """The keys of cls_head_soft_ref plus loss_ce, loss_kd, agree, probs_t [M,C] (and logits_t, margin_t, the teacher's top-two gap)."""
    T, alpha, ce_weight = float(T), float(alpha), float(ce_weight)
    soft = cls_head_soft_ref(feats, y_a, W, b, grad_scale=grad_scale, y_b=y_b, lam=lam, smoothing=smoothing)
    x = np.asarray(feats, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    z = soft["logits"]
    z_t = np.asarray(feats_t, dtype=np.float64) @ np.asarray(W_t, dtype=np.float64).T + np.asarray(b_t, dtype=np.float64)
    M, C = z.shape
    ya = np.asarray(y_a, dtype=np.int64)
    yb = ya if y_b is None else np.asarray(y_b, dtype=np.int64)
    ok = (ya >= 0) & (ya < C) & (yb >= 0) & (yb < C)
    lse_t, lse_s = _lse(z_t / T), _lse(z / T)
    p = np.exp(z_t / T - lse_t[:, None])
    q = np.exp(z / T - lse_s[:, None])
    kl = np.where(ok, (p * (z_t / T)).sum(axis=1) - lse_t - (p * (z / T)).sum(axis=1) + lse_s, 0.0)
    loss_ce = soft["loss"]
    loss_kd = T * T * kl.sum() / M
    dlogits = ce_weight * soft["dlogits"] + (float(grad_scale) / M) * alpha * T * (q - p) * ok[:, None]
    top2 = np.sort(z_t, axis=1)[:, -2:]
    out = dict(soft)
    out.update(loss=ce_weight * loss_ce + alpha * loss_kd, loss_ce=loss_ce, loss_kd=loss_kd,
               agree=float(((z.argmax(axis=1) == z_t.argmax(axis=1)) & ok).sum()), probs_t=p, logits_t=z_t,
               margin_t=top2[:, 1] - top2[:, 0], dlogits=dlogits, dfeats=dlogits @ W, gW=dlogits.T @ x, gb=dlogits.sum(axis=0),
               status=0 if ok.all() else ST_LABEL_RANGE)
    return out
