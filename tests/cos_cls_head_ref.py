"""Float64 numpy restatement of the fused cosine classifier head (fumi_hip_cos_cls_head_step, csrc/coshead.hip; DESIGN.md section
41).  With u_m = feats_m / max(|feats_m|, eps), v_c = W_c / max(|W_c|, eps), k = u v^T and t the soft target of
tests/cls_head_soft_ref.py,

    z = tau k,   loss = mean_m (lse(z_m) - sum_c t z),   dz = grad_scale / M * (softmax(z) - t),
    dtau     = sum_{m,c} dz k,
    dfeats_m = tau / |feats_m| * (sum_c dz[m,c] v_c - (sum_c dz[m,c] k[m,c]) u_m),
    gW_c     = tau / |W_c|     * (sum_m dz[m,c] u_m - (sum_m dz[m,c] k[m,c]) v_c).

The gradients are these closed forms, not a tape: tests/test_cos_cls_head_cpu.py holds them to central finite differences of ``loss``.
A row of feats or W whose norm is below eps is the zero direction: k = 0 along it and its gradient row is zero.  A label outside
[0, C) in y_a or y_b marks its row invalid: the row adds nothing to the loss, the count or any gradient, the divisor stays M, ``status``
carries FUMI_ST_LABEL_RANGE.  The norms are taken in float64 here and in float32 on the device; that rounding is part of the error the
GPU test bounds."""
import numpy as np

from cls_head_ref import ST_LABEL_RANGE

EPS = 1e-12


def cos_cls_head_ref(feats, y_a, W, tau, grad_scale=1.0, y_b=None, lam=1.0, smoothing=0.0):
    """dict(loss, correct, preds [M], logits [M,C], margin [M], dz, dfeats, gW, dtau, dtau_abs = sum |dz k|, status)."""
    x = np.asarray(feats, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    tau = float(np.asarray(tau, dtype=np.float64).reshape(-1)[0])
    ya = np.asarray(y_a, dtype=np.int64)
    yb = ya if y_b is None else np.asarray(y_b, dtype=np.int64)
    lam, eps = float(lam), float(smoothing)
    M, C = x.shape[0], W.shape[0]
    nf, nw = np.sqrt((x * x).sum(axis=1)), np.sqrt((W * W).sum(axis=1))
    rf = np.where(nf >= EPS, 1.0 / np.maximum(nf, EPS), 0.0)
    rw = np.where(nw >= EPS, 1.0 / np.maximum(nw, EPS), 0.0)
    u, v = x * rf[:, None], W * rw[:, None]
    k = u @ v.T
    z = tau * k
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
    np.add.at(hot, (rows, ybc), 1.0 - lam)
    t = (1.0 - eps) * hot + eps / C
    row_loss = np.where(ok, lse - (t * z).sum(axis=1), 0.0)
    dz = (p - t) * ok[:, None] * (float(grad_scale) / M)
    dzk = dz * k
    dfeats = tau * rf[:, None] * (dz @ v - dzk.sum(axis=1)[:, None] * u)
    gW = tau * rw[:, None] * (dz.T @ u - dzk.sum(axis=0)[:, None] * v)
    return dict(loss=row_loss.sum() / M, correct=float(((preds == ya) & ok).sum()), preds=preds, logits=z,
                margin=top2[:, 1] - top2[:, 0], dz=dz, dfeats=dfeats, gW=gW, dtau=dzk.sum(), dtau_abs=np.abs(dzk).sum(),
                status=0 if ok.all() else ST_LABEL_RANGE)
