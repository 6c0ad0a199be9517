"""Float64 numpy restatement of the transductive prototype refinement (fumi_hip_trans_proto_step, csrc/transproto.hip).  This is the
definition the kernel is held to; tests/test_trans_proto_cpu.py ties it to a plain torch float64 loop at 1e-12 and, at steps = 0, to
cos_proto_ref / euclid_proto_ref.

Per episode, with s_n the sum and k_n the count of the support rows with label n:  c^0_n = s_n / max(k_n, 1), and for t = 0 .. steps-1
    w = softmax_n(z(c^t)) over all query rows,   c^{t+1}_n = (s_n + sum_q w[q,n] f_q) / (k_n + sum_q w[q,n])
(soft k-means, Ren et al. 2018), with the logits of a prototype set
    metric "cosine":  z[q,n] = scale <f_q, c_n> / (max(|f_q|, EPS) max(|c_n|, EPS))        (EPS of the cosine head)
    metric "euclid":  z[q,n] = -scale |f_q - c_n|^2                                         (the plain difference, squared and summed).
The means are over the raw rows in both metrics, so steps = 0 is the cosine head or the prototypical head.  loss = mean over all
B * Qn query rows of the softmax cross-entropy of z(c^steps) against y_q.

A query label outside [0, N) sets ST_LABEL_RANGE: the row adds nothing to the loss or the count (the divisor stays B * Qn), and it
DOES take part in the refinement, which reads no query label.  A support row with such a label sets the same bit and is left out
exactly.  A class without a support row sets ST_CLASS_MISSING, starts from a zero prototype and is refined like any class.

dtype=np.float32 runs the same iteration in plain float32 numpy: the CPU test's measure of what fp32 can reach."""
import numpy as np

from cos_proto_ref import EPS, ST_CLASS_MISSING, ST_LABEL_RANGE  # noqa: F401  (re-exported to the tests)

METRICS = ("cosine", "euclid")
SCALES = {"cosine": 10.0, "euclid": 4.0}                        # the scales of the parity tests
STEPS = (0, 1, 10)
# the two limit shapes (B, S, Qn, N, F) the GPU test adds to ridge_head_ref.SHAPES: S + Qn = 512 at the 20-way 15-query episode and
# the feature limit; S + Qn = 512 and Qn * N = 8192 at the class limit
LIMIT_SHAPES = [(1, 212, 300, 20, 2048), (1, 384, 128, 64, 32)]
SHIFTED = [(2, 100, 130, 20, 640), (3, 10, 16, 5, 2048)]        # euclid, steps = 10, again with SHIFT added to every feature
SHIFT = 8.0


def _logits(xq, protos, scale, metric, dt):
    if metric == "cosine":
        eps = dt(EPS)
        pn = np.sqrt((protos * protos).sum(-1))                                    # [B, N]
        qn = np.sqrt((xq * xq).sum(-1))                                            # [B, Qn]
        dot = np.einsum("bqf,bnf->bqn", xq, protos)
        return scale * dot / (np.maximum(qn, eps)[:, :, None] * np.maximum(pn, eps)[:, None, :])
    B, Qn = xq.shape[:2]
    d2 = np.empty((B, Qn, protos.shape[1]), dtype=dt)
    for n in range(protos.shape[1]):                                               # the difference itself, one class at a time
        d2[:, :, n] = ((xq - protos[:, n][:, None, :]) ** 2).sum(-1)
    return -scale * d2


def trans_proto_ref(feats_s, y_s, feats_q, y_q, n_way, scale, metric, steps, dtype=np.float64):
    """dict(loss, correct, preds [B,Qn], logits [B,Qn,N], logits0 (z(c^0)), margin [B,Qn] (top-two logit gap), protos [B,N,F] (c^steps),
    status), in ``dtype``."""
    if metric not in METRICS:
        raise ValueError(f"metric must be cosine or euclid, got {metric}")
    dt = np.dtype(dtype).type
    xs = np.asarray(feats_s, dtype=dt)
    xq = np.asarray(feats_q, dtype=dt)
    ys = np.asarray(y_s, dtype=np.int64)
    yq = np.asarray(y_q, dtype=np.int64)
    scale = dt(np.asarray(scale, dtype=np.float64).reshape(-1)[0])
    B, S, F = xs.shape
    Qn, N = xq.shape[1], int(n_way)
    ok_s = (ys >= 0) & (ys < N)
    ok_q = (yq >= 0) & (yq < N)
    onehot_s = np.zeros((B, S, N), dtype=dt)
    bi, si = np.nonzero(ok_s)
    onehot_s[bi, si, ys[bi, si]] = 1.0
    count = onehot_s.sum(axis=1)                                                   # [B, N]
    status = (0 if ok_s.all() and ok_q.all() else ST_LABEL_RANGE) | (ST_CLASS_MISSING if (count == 0).any() else 0)
    sums = np.einsum("bsn,bsf->bnf", onehot_s, xs)                                 # [B, N, F]
    protos = sums / np.maximum(count, dt(1.0))[:, :, None]
    z = _logits(xq, protos, scale, metric, dt)
    z0 = z
    for _ in range(int(steps)):
        e = np.exp(z - z.max(axis=-1, keepdims=True))
        w = e / e.sum(axis=-1, keepdims=True)                                      # [B, Qn, N]: every query row, whatever its label
        protos = (sums + np.einsum("bqn,bqf->bnf", w, xq)) / (count + w.sum(axis=1))[:, :, None]
        z = _logits(xq, protos, scale, metric, dt)
    mx = z.max(axis=-1, keepdims=True)
    e = np.exp(z - mx)
    lse = (mx + np.log(e.sum(axis=-1, keepdims=True)))[..., 0]
    preds = z.argmax(axis=-1)                                                      # numpy's argmax is the first one, like torch.max
    top2 = np.sort(z, axis=-1)[..., -2:]
    yc = np.where(ok_q, yq, 0)
    z_y = np.take_along_axis(z, yc[..., None], axis=-1)[..., 0]
    loss = np.where(ok_q, lse - z_y, dt(0.0)).sum() / dt(B * Qn)
    return dict(loss=loss, correct=float(((preds == yq) & ok_q).sum()), preds=preds, logits=z, logits0=z0,
                margin=top2[..., 1] - top2[..., 0], protos=protos, status=int(status))
