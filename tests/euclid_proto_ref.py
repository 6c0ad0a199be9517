"""Float64 numpy restatement of the fused prototypical-network head (fumi_hip_euclid_proto_step, csrc/euclidproto.hip).  This is the
definition the kernel is held to; tests/test_euclid_proto_cpu.py ties it to torch.autograd at 1e-12.

Per episode b:  c_n = mean of the support rows with y_s == n (count clamped to >= 1),  d2[q,n] = sum_f (feats_q[q,f] - c_n[f])^2,
z = -alpha d2,  loss = mean over all B * Qn query rows of the softmax cross-entropy of z against y_q.  The distance is the plain
difference, squared and summed: no |f|^2 - 2 f.c + |c|^2 expansion, so the restatement is as good on features that share a large
offset as on centred ones.  Gradients are those of grad_scale * loss:
    dz = grad_scale / (B Qn) (softmax(z) - onehot(y_q)),   dfeats_q = 2 alpha (dz C - f_q sum_n dz[q,n]),
    dc_n = 2 alpha ((dz^T F_q)_n - c_n sum_q dz[q,n]),     dalpha = -sum dz * d2,
and every support row of class n receives dc_n / count_n.

A label outside [0, N) sets ST_LABEL_RANGE: such a query row adds nothing to the loss, the count or any gradient (the divisor stays
B * Qn), such a support row is left out of the means and gets a zero gradient.  A class without a support row sets ST_CLASS_MISSING
and has a zero prototype.

The parity inputs are those of the cosine head (cos_proto_ref.case_inputs)."""
import numpy as np

from cos_proto_ref import ST_CLASS_MISSING, ST_LABEL_RANGE, case_inputs  # noqa: F401  (re-exported to the tests)

# the shapes (B, S, Qn, N, F) of tests/test_euclid_proto_gpu.py: the smallest of everything; rows, classes and features off every tile
# edge with unequal counts; 20-way at the ResNet-12 width, more than eight row tiles plus a tail; the Conv4 width, a short last feature
# block; the class limit; the feature limit
SHAPES = [(1, 2, 1, 2, 32), (2, 7, 33, 3, 96), (2, 100, 130, 20, 640), (1, 25, 17, 5, 1600), (1, 64, 18, 64, 64), (3, 10, 16, 5, 2048)]
SHIFTED = [(2, 100, 130, 20, 640), (3, 10, 16, 5, 2048)]        # parity again with SHIFT added to every feature
SHIFT = 8.0
GRAD_SCALE = 0.25


def euclid_proto_ref(feats_s, y_s, feats_q, y_q, alpha, n_way, grad_scale=1.0):
    """dict(loss, correct, preds [B,Qn], logits [B,Qn,N], d2, margin [B,Qn] (top-two logit gap), pmax (largest softmax probability),
    protos [B,N,F], dfeats_s, dfeats_q, dalpha, dalpha_abs = sum |dz (d2 - min_n d2)| (what the round-off of dalpha scales with),
    status), all float64."""
    xs = np.asarray(feats_s, dtype=np.float64)
    xq = np.asarray(feats_q, dtype=np.float64)
    ys = np.asarray(y_s, dtype=np.int64)
    yq = np.asarray(y_q, dtype=np.int64)
    alpha = float(np.asarray(alpha, dtype=np.float64).reshape(-1)[0])
    B, S, F = xs.shape
    Qn, N = xq.shape[1], int(n_way)
    ok_s = (ys >= 0) & (ys < N)
    ok_q = (yq >= 0) & (yq < N)
    onehot_s = np.zeros((B, S, N))
    bi, si = np.nonzero(ok_s)
    onehot_s[bi, si, ys[bi, si]] = 1.0
    count = onehot_s.sum(axis=1)                                                   # [B, N]
    status = (0 if ok_s.all() and ok_q.all() else ST_LABEL_RANGE) | (ST_CLASS_MISSING if (count == 0).any() else 0)
    cnt = np.maximum(count, 1.0)
    protos = np.einsum("bsn,bsf->bnf", onehot_s, xs) / cnt[:, :, None]
    d2 = np.empty((B, Qn, N))
    for n in range(N):                                                             # the difference itself, one class at a time
        d2[:, :, n] = ((xq - protos[:, n][:, None, :]) ** 2).sum(-1)
    z = -alpha * d2
    mx = z.max(axis=-1, keepdims=True)
    e = np.exp(z - mx)
    s = e.sum(axis=-1, keepdims=True)
    lse = (mx + np.log(s))[..., 0]
    preds = z.argmax(axis=-1)                                                      # numpy's argmax is the first one, like torch.max
    top2 = np.sort(z, axis=-1)[..., -2:]
    yc = np.where(ok_q, yq, 0)
    z_y = np.take_along_axis(z, yc[..., None], axis=-1)[..., 0]
    M = B * Qn
    loss = np.where(ok_q, lse - z_y, 0.0).sum() / M
    onehot_q = np.zeros_like(z)
    np.put_along_axis(onehot_q, yc[..., None], 1.0, axis=-1)
    dz = (e / s - onehot_q) * ok_q[..., None] * (float(grad_scale) / M)
    dalpha = -(dz * d2).sum()
    dalpha_abs = np.abs(dz * (d2 - d2.min(axis=-1, keepdims=True))).sum()
    dfeats_q = 2.0 * alpha * (np.einsum("bqn,bnf->bqf", dz, protos) - xq * dz.sum(-1, keepdims=True))
    dc = 2.0 * alpha * (np.einsum("bqn,bqf->bnf", dz, xq) - protos * dz.sum(1)[:, :, None])
    dfeats_s = np.einsum("bsn,bnf->bsf", onehot_s, dc / cnt[:, :, None])
    return dict(loss=loss, correct=float(((preds == yq) & ok_q).sum()), preds=preds, logits=z, d2=d2, margin=top2[..., 1] - top2[..., 0],
                pmax=float((e / s).max()), protos=protos, dfeats_s=dfeats_s, dfeats_q=dfeats_q, dalpha=dalpha, dalpha_abs=dalpha_abs,
                status=int(status))
