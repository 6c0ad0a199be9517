"""Float64 numpy restatement of the fused cosine nearest-centroid head (fumi_hip_cos_proto_step, csrc/cosproto.hip).  This is the
definition the kernel is held to; tests/test_cos_proto_cpu.py ties it to torch.autograd at 1e-12.

Per episode b:  c_n = mean of the support rows with y_s == n (count clamped to >= 1),  norm(x) = x / max(|x|_2, 1e-12),
z[q,n] = tau <norm(feats_q[q]), norm(c_n)>,  loss = mean over all B * Qn query rows of the softmax cross-entropy of z against y_q.
Gradients are those of grad_scale * loss.  Where a norm is below the clamp the gradient through the normalisation is the plain
d / 1e-12 (what autograd gives for F.normalize); the projection onto the tangent space applies at or above the clamp.

A label outside [0, N) sets ST_LABEL_RANGE: such a query row adds nothing to the loss, the count or any gradient (the divisor stays
B * Qn), such a support row is left out of the means and gets a zero gradient.  A class without a support row sets ST_CLASS_MISSING
and has a zero prototype."""
import numpy as np

ST_LABEL_RANGE, ST_CLASS_MISSING = 1, 2
EPS = 1e-12


def case_inputs(B, S, Qn, N, F):
    """The seeded inputs of the parity tests: class means mu ~ N(0, 1) [B,N,F], rows relu(mu[y] + 2 N(0, 1)), y_s = arange(S) % N with
    the last row set to class 0 when S > N (unequal class counts), y_q uniform.  float32 features, int64 labels."""
    rs = np.random.RandomState(100003 * B + 10007 * S + 1009 * Qn + 101 * N + F)
    mu = rs.standard_normal((B, N, F))
    y_s = np.tile(np.arange(S) % N, (B, 1)).astype(np.int64)
    if S > N:
        y_s[:, -1] = 0
    y_q = rs.randint(0, N, (B, Qn)).astype(np.int64)
    bi = np.arange(B)[:, None]
    f_s = np.maximum(mu[bi, y_s] + 2.0 * rs.standard_normal((B, S, F)), 0.0).astype(np.float32)
    f_q = np.maximum(mu[bi, y_q] + 2.0 * rs.standard_normal((B, Qn, F)), 0.0).astype(np.float32)
    return f_s, y_s, f_q, y_q


def cos_proto_ref(feats_s, y_s, feats_q, y_q, tau, n_way, grad_scale=1.0):
    """dict(loss, correct, preds [B,Qn], logits [B,Qn,N], cos, margin [B,Qn] (top-two logit gap), protos [B,N,F], dfeats_s, dfeats_q,
    dtau, status), all float64."""
    xs = np.asarray(feats_s, dtype=np.float64)
    xq = np.asarray(feats_q, dtype=np.float64)
    ys = np.asarray(y_s, dtype=np.int64)
    yq = np.asarray(y_q, dtype=np.int64)
    tau = float(np.asarray(tau, dtype=np.float64).reshape(-1)[0])
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
    pn = np.sqrt((protos ** 2).sum(-1))                                            # [B, N]
    qn = np.sqrt((xq ** 2).sum(-1))                                                # [B, Qn]
    ch = protos / np.maximum(pn, EPS)[:, :, None]
    qh = xq / np.maximum(qn, EPS)[:, :, None]
    cos = np.einsum("bqf,bnf->bqn", qh, ch)
    z = tau * cos
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
    dtau = (dz * cos).sum()
    dcos = tau * dz
    # query rows through norm()
    dqh = np.einsum("bqn,bnf->bqf", dcos, ch)
    proj_q = (qn >= EPS)[..., None]
    dfeats_q = (dqh - proj_q * qh * (qh * dqh).sum(-1, keepdims=True)) / np.maximum(qn, EPS)[..., None]
    # prototypes through norm(), then the class mean
    dch = np.einsum("bqn,bqf->bnf", dcos, qh)
    proj_p = (pn >= EPS)[..., None]
    dc = (dch - proj_p * ch * (ch * dch).sum(-1, keepdims=True)) / np.maximum(pn, EPS)[..., None]
    dfeats_s = np.einsum("bsn,bnf->bsf", onehot_s, dc / cnt[:, :, None])
    return dict(loss=loss, correct=float(((preds == yq) & ok_q).sum()), preds=preds, logits=z, cos=cos, margin=top2[..., 1] - top2[..., 0],
                protos=protos, dfeats_s=dfeats_s, dfeats_q=dfeats_q, dtau=dtau, status=int(status))
