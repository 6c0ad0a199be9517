"""Float64 numpy restatement of the fused Relation Network head (fumi_hip_relation_head_step, csrc/relationhead.hip).  This is the
definition the kernels are held to; tests/test_relation_head_cpu.py ties it to torch.autograd on the plain expression (concatenate,
F.linear, relu, F.linear, MSELoss / cross_entropy) at 1e-10.

Per episode b, with c_n the mean of the valid support rows of class n (count clamped to >= 1), w1 = (W1s, W1q) [2,H,F]:
    U[n,:] = W1s c_n + b1,   V[q,:] = W1q f_q,   pre[q,n,:] = U[n,:] + V[q,:],   z[q,n] = w2 . relu(pre[q,n,:]) + b2.
loss "mse": 1 / (B Qn N) sum over the valid query rows and the N classes of (sigmoid(z) - onehot(y_q))^2; loss "ce": the softmax
cross-entropy of z over the classes, mean over all B Qn rows.  Gradients are those of grad_scale * loss.  With ``mask`` [B,Qn,N,H]
(bool) the BACKWARD uses that mask in place of pre > 0 (teacher forcing on the kernels' mask, rebuilt from their hid_s + hid_q in
fp32); the forward is unchanged.

A label outside [0, N) sets ST_LABEL_RANGE: such a query row adds nothing to the loss, the count or any gradient (the divisor stays),
such a support row takes no part and gets a zero gradient.  A class without a valid support row sets ST_CLASS_MISSING and has a zero
prototype, so U[n,:] = b1.  preds is the first arg-max of z."""
import numpy as np

from match_head_ref import case_inputs

ST_LABEL_RANGE, ST_CLASS_MISSING = 1, 2
GRAD_SCALE = 0.25
LOSSES = ("mse", "ce")

# (B, S, Qn, N, F, H): each the smallest that crosses an edge of the kernels
SHAPES = [(2, 7, 33, 3, 96, 96),         # S below a tile, unequal shots, a ragged last query tile, H no power of two
          (4, 5, 1, 5, 64, 32),          # one shot, one query, smallest H
          (1, 25, 75, 5, 640, 256),      # the workload's own class of shape
          (3, 100, 17, 20, 160, 64),     # 20-way
          (2, 129, 16, 64, 32, 1024),    # N = 64, largest H, smallest F
          (1, 130, 5, 2, 2048, 32)]      # largest F
ONE_SHOT = (4, 5, 1, 5, 64, 32)
LIMITS = (2, 1024, 32768, 2, 32, 32)
UNCERTAIN = 1e-5                         # |pre| <= UNCERTAIN * max|pre|: where an fp32 and a float64 sign may differ


def case_weights(F, H):
    """The seeded relation module of the parity tests: w1, b1 uniform in +-1/sqrt(2F) (nn.Linear's default), w2 = 4 uniform(+-1) /
    sqrt(H) (scores of a few units, so neither loss is flat), b2 = 0.1.  float32."""
    rs = np.random.RandomState(31 * H + F)
    k1 = 1.0 / np.sqrt(2.0 * F)
    w1 = rs.uniform(-k1, k1, (2, H, F)).astype(np.float32)
    b1 = rs.uniform(-k1, k1, (H,)).astype(np.float32)
    w2 = (4.0 * rs.uniform(-1.0, 1.0, (H,)) / np.sqrt(H)).astype(np.float32)
    b2 = np.array([0.1], dtype=np.float32)
    return w1, b1, w2, b2


def case(shape):
    """(features and labels of match_head_ref.case_inputs, weights of case_weights) of a (B, S, Qn, N, F, H) shape."""
    return case_inputs(*shape[:5]), case_weights(shape[4], shape[5])


def relation_head_ref(feats_s, y_s, feats_q, y_q, w1, b1, w2, b2, n_way, loss="mse", grad_scale=1.0, mask=None):
    """dict(loss, correct, preds [B,Qn], logits [B,Qn,N], margin [B,Qn] (top-two gap of z), hid_s [B,N,H], hid_q [B,Qn,H], pre
    [B,Qn,N,H], dfeats_s, dfeats_q, dw1, db1, dw2, db2, db2_abs = sum |dz|, db1_abs = max_h sum_{b,n} |dU[n,h]|, status), all float64."""
    xs_all, xq_all = np.asarray(feats_s, dtype=np.float64), np.asarray(feats_q, dtype=np.float64)
    ys_all, yq_all = np.asarray(y_s, dtype=np.int64), np.asarray(y_q, dtype=np.int64)
    w1, b1, w2 = (np.asarray(t, dtype=np.float64) for t in (w1, b1, w2))
    b2 = float(np.asarray(b2, dtype=np.float64).reshape(-1)[0])
    assert loss in LOSSES
    B, S, F = xs_all.shape
    Qn, N, H = xq_all.shape[1], int(n_way), w1.shape[1]
    W1s, W1q = w1[0], w1[1]
    out = dict(logits=np.empty((B, Qn, N)), preds=np.empty((B, Qn), dtype=np.int64), margin=np.empty((B, Qn)),
               hid_s=np.empty((B, N, H)), hid_q=np.empty((B, Qn, H)), pre=np.empty((B, Qn, N, H)),
               dfeats_s=np.zeros((B, S, F)), dfeats_q=np.empty((B, Qn, F)), dw1=np.zeros((2, H, F)), db1=np.zeros(H), dw2=np.zeros(H))
    total = correct = db2 = db2_abs = 0.0
    db1_abs = np.zeros(H)
    status = 0
    for b in range(B):
        xs, xq, ys, yq = xs_all[b], xq_all[b], ys_all[b], yq_all[b]
        ok_s, ok_q = (ys >= 0) & (ys < N), (yq >= 0) & (yq < N)
        onehot = np.zeros((S, N))
        onehot[np.nonzero(ok_s)[0], ys[ok_s]] = 1.0
        count = onehot.sum(axis=0)
        if not (ok_s.all() and ok_q.all()):
            status |= ST_LABEL_RANGE
        if (count == 0).any():
            status |= ST_CLASS_MISSING
        cnt = np.maximum(count, 1.0)
        c = (onehot.T @ xs) / cnt[:, None]                                       # [N, F]
        U = c @ W1s.T + b1                                                         # [N, H]
        V = xq @ W1q.T                                                             # [Qn, H]
        pre = V[:, None, :] + U[None, :, :]                                        # [Qn, N, H]
        act = np.maximum(pre, 0.0)
        z = act @ w2 + b2                                                          # [Qn, N]
        preds = z.argmax(axis=1)                                                   # numpy's argmax is the first one, like torch.max
        top2 = np.sort(z, axis=1)[:, -2:]
        yc = np.where(ok_q, yq, 0)
        t = np.zeros((Qn, N))
        t[np.arange(Qn), yc] = 1.0
        if loss == "mse":
            s = 1.0 / (1.0 + np.exp(-z))
            total += (((s - t) ** 2).sum(axis=1) * ok_q).sum()
            dz = float(grad_scale) * 2.0 / (B * Qn * N) * (s - t) * s * (1.0 - s)
        else:
            mx = z.max(axis=1, keepdims=True)
            e = np.exp(z - mx)
            lse = mx[:, 0] + np.log(e.sum(axis=1))
            total += ((lse - z[np.arange(Qn), yc]) * ok_q).sum()
            dz = float(grad_scale) / (B * Qn) * (e / e.sum(axis=1, keepdims=True) - t)
        dz = dz * ok_q[:, None]
        correct += float(((preds == yq) & ok_q).sum())
        m = (pre > 0.0) if mask is None else np.asarray(mask[b], dtype=bool)
        g = dz[:, :, None] * m                                                     # [Qn, N, H] dz m
        dV = w2 * g.sum(axis=1)                                                    # [Qn, H]
        dU = w2 * g.sum(axis=0)                                                    # [N, H]
        out["dw2"] += (dz[:, :, None] * act).sum(axis=(0, 1))
        db2 += dz.sum()
        db2_abs += np.abs(dz).sum()
        out["db1"] += dU.sum(axis=0)
        db1_abs += np.abs(dU).sum(axis=0)
        out["dw1"][1] += dV.T @ xq
        out["dw1"][0] += dU.T @ c
        out["dfeats_q"][b] = dV @ W1q
        dc = dU @ W1s                                                              # [N, F]
        out["dfeats_s"][b] = onehot @ (dc / cnt[:, None])
        out["logits"][b], out["preds"][b], out["margin"][b] = z, preds, top2[:, 1] - top2[:, 0]
        out["hid_s"][b], out["hid_q"][b], out["pre"][b] = U, V, pre
    out.update(loss=total / (B * Qn * (N if loss == "mse" else 1)), correct=correct, db2=np.array([db2]), db2_abs=db2_abs, db1_abs=float(db1_abs.max()),
               status=int(status))
    return out
