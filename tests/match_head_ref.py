"""Float64 numpy restatement of the fused Matching Networks head (fumi_hip_match_head_step, csrc/matchhead.hip).  This is the
definition the kernels are held to; tests/test_match_head_cpu.py ties it to torch.autograd at 1e-10 and, at one row per class, to
tests/cos_proto_ref.py at 1e-12.

Per episode b, with norm(x) = x / max(|x|_2, 1e-12) and a support row valid when its label is in [0, N):
    cos[q,i] = <norm(feats_q[q]), norm(feats_s[i])>,   a = tau cos,
    z[q,n] = logsumexp over the valid rows i with y_s == n of a[q,i]    (the class maximum is subtracted before exp),
    loss = mean over all B * Qn query rows of logsumexp_n z[q,:] - z[q,y_q],
which is -log sum_{i: y_i = y_q} softmax_i(a[q,:]).  Gradients are those of grad_scale * loss: with gs = grad_scale / (B Qn), p the
softmax of a over all valid rows and r the softmax within the class y_q (zero outside it), da = gs (p - r), dtau = sum da cos, and
dfeats_q, dfeats_s go through norm() as in the cosine head (below the clamp the projection term is dropped, what autograd gives).

A label outside [0, N) sets ST_LABEL_RANGE: such a query row adds nothing to the loss, the count or any gradient (the divisor stays
B * Qn), such a support row takes no part and gets a zero gradient.  A class without a valid support row sets ST_CLASS_MISSING and
has z = -inf; a query row labelled with it is left out like a query label out of range.  preds is the first arg-max of z over the
classes that are not NaN, class 0 when all are (or when every class is -inf)."""
import numpy as np

ST_LABEL_RANGE, ST_CLASS_MISSING = 1, 2
EPS = 1e-12
TAU, GRAD_SCALE = 10.0, 0.25

# (B, S, Qn, N, F): each the smallest that crosses an edge of the kernels
SHAPES = [(2, 7, 33, 3, 96),         # S below one tile, unequal shots, a ragged last query tile
          (4, 5, 1, 5, 64),          # one shot, one query
          (1, 25, 75, 5, 640),       # the workload's own class of shape
          (3, 100, 17, 20, 160),     # 20-way
          (2, 129, 16, 64, 32),      # N = 64, S one past a 128-column block, smallest F
          (1, 512, 5, 2, 2048)]      # both upper limits of S and F
ONE_SHOT = (4, 5, 1, 5, 64)
LIMITS = (2, 512, 32768, 2, 32)
SATURATED = (1, 12, 16, 3, 96)       # case C, at TAU_SATURATED
TAU_SATURATED = 100.0


def case_inputs(B, S, Qn, N, F):
    """The seeded inputs of the parity tests: class centres mu ~ N(0, 1) [B,N,F], rows mu[y] + 0.7 N(0, 1) (attention is neither
    uniform nor one-hot at TAU), y_s = arange(S) % N -- unequal shots wherever S is no multiple of N -- shuffled per episode so that a
    class's rows are not contiguous, y_q uniform.  float32 features, int64 labels."""
    rs = np.random.RandomState(100003 * B + 10007 * S + 1009 * Qn + 101 * N + F + 7)
    mu = rs.standard_normal((B, N, F))
    y_s = np.stack([rs.permutation(np.arange(S) % N) for _ in range(B)]).astype(np.int64)
    y_q = rs.randint(0, N, (B, Qn)).astype(np.int64)
    bi = np.arange(B)[:, None]
    f_s = (mu[bi, y_s] + 0.7 * rs.standard_normal((B, S, F))).astype(np.float32)
    f_q = (mu[bi, y_q] + 0.7 * rs.standard_normal((B, Qn, F))).astype(np.float32)
    return f_s, y_s, f_q, y_q


def saturated_inputs():
    """Case C, SATURATED at TAU_SATURATED: the first four query rows are near-copies of support row 0 (class y_s[0, 0]) and the rows of
    the next class point nearly the opposite way, so that class's log-mass lies about 2 tau = 200 below the row's largest."""
    B, S, Qn, N, F = SATURATED
    rs = np.random.RandomState(424243)
    y_s = np.tile(np.arange(S) % N, (B, 1)).astype(np.int64)
    y_q = rs.randint(0, N, (B, Qn)).astype(np.int64)
    f_s = rs.standard_normal((B, S, F))
    f_q = rs.standard_normal((B, Qn, F))
    far = (y_s[0, 0] + 1) % N
    for i in np.nonzero(y_s[0] == far)[0]:
        f_s[0, i] = -f_s[0, 0] + 1e-3 * rs.standard_normal(F)
    for q in range(4):
        f_q[0, q] = f_s[0, 0] + 1e-3 * rs.standard_normal(F)
    return f_s.astype(np.float32), y_s, f_q.astype(np.float32), y_q


def match_head_ref(feats_s, y_s, feats_q, y_q, tau, n_way, grad_scale=1.0, want_da=False):
    """dict(loss, correct, preds [B,Qn], logits [B,Qn,N], margin [B,Qn] (top-two gap of z), dfeats_s, dfeats_q, dtau, dtau_abs =
    sum |da cos|, da_rowsum_max = max |sum_i da[q,i]|, status), all float64; with want_da also cos and da [B,Qn,S]."""
    xs_all = np.asarray(feats_s, dtype=np.float64)
    xq_all = np.asarray(feats_q, dtype=np.float64)
    ys_all = np.asarray(y_s, dtype=np.int64)
    yq_all = np.asarray(y_q, dtype=np.int64)
    tau = float(np.asarray(tau, dtype=np.float64).reshape(-1)[0])
    B, S, F = xs_all.shape
    Qn, N = xq_all.shape[1], int(n_way)
    gs = float(grad_scale) / (B * Qn)
    out = dict(logits=np.empty((B, Qn, N)), preds=np.empty((B, Qn), dtype=np.int64), margin=np.empty((B, Qn)),
               dfeats_s=np.empty((B, S, F)), dfeats_q=np.empty((B, Qn, F)))
    if want_da:
        out["cos"], out["da"] = np.empty((B, Qn, S)), np.empty((B, Qn, S))
    loss = dtau = dtau_abs = correct = rowsum = 0.0
    status = 0
    for b in range(B):                                                             # (per episode: the limit shape stays within memory)
        xs, xq, ys, yq = xs_all[b], xq_all[b], ys_all[b], yq_all[b]
        ok_s = (ys >= 0) & (ys < N)
        in_q = (yq >= 0) & (yq < N)
        onehot = np.zeros((S, N), dtype=bool)
        onehot[np.nonzero(ok_s)[0], ys[ok_s]] = True
        count = onehot.sum(axis=0)
        if not (ok_s.all() and in_q.all()):
            status |= ST_LABEL_RANGE
        if (count == 0).any():
            status |= ST_CLASS_MISSING
        sn, qn = np.sqrt((xs ** 2).sum(-1)), np.sqrt((xq ** 2).sum(-1))
        rsn, rqn = 1.0 / np.maximum(sn, EPS), 1.0 / np.maximum(qn, EPS)
        sh, qh = xs * rsn[:, None], xq * rqn[:, None]
        cos = qh @ sh.T                                                            # [Qn, S]
        a = tau * cos
        z = np.full((Qn, N), -np.inf)
        cmax = np.zeros((Qn, N))
        with np.errstate(all="ignore"):                                          # (-inf logits of a class without a row)
            for n in np.nonzero(count)[0]:
                an = a[:, onehot[:, n]]
                cmax[:, n] = an.max(axis=1)
                z[:, n] = cmax[:, n] + np.log(np.exp(an - cmax[:, [n]]).sum(axis=1))
            zz = np.where(np.isnan(z), -np.inf, z)                                 # arg-max over what is not NaN
            preds = np.where(np.isneginf(zz).all(axis=1), 0, zz.argmax(axis=1))    # numpy's argmax is the first one, like torch.max
            top2 = np.sort(zz, axis=1)[:, -2:]
            margin = top2[:, 1] - top2[:, 0]
            yc = np.where(in_q, yq, 0)
            ok_q = in_q & (count[yc] > 0)                                          # a label of a class without a row is left out too
            mx = zz.max(axis=1, keepdims=True)
            mx = np.where(np.isfinite(mx), mx, 0.0)
            ez = np.exp(z - mx)
            lse = mx[:, 0] + np.log(ez.sum(axis=1))
            z_y = z[np.arange(Qn), yc]
            loss += np.where(ok_q, lse - z_y, 0.0).sum()
            correct += float(((preds == yq) & ok_q).sum())
            # p: softmax over all valid rows; r: softmax within the class y_q
            p = np.where(ok_s[None, :], np.exp(a - lse[:, None]), 0.0)
            mine = onehot[:, yc].T                                                 # [Qn, S] rows of the query's class
            r = np.where(mine, np.exp(a - z_y[:, None]), 0.0)
            da = np.where(ok_q[:, None], gs * (p - r), 0.0)
        dtau += (da * cos).sum()
        dtau_abs += np.abs(da * cos).sum()
        rowsum = max(rowsum, float(np.abs(da.sum(axis=1)).max()))
        Gq = tau * (da @ sh)
        out["dfeats_q"][b] = rqn[:, None] * (Gq - (qn >= EPS)[:, None] * qh * (qh * Gq).sum(-1, keepdims=True))
        Gs = tau * (da.T @ qh)
        out["dfeats_s"][b] = rsn[:, None] * (Gs - (sn >= EPS)[:, None] * sh * (sh * Gs).sum(-1, keepdims=True))
        out["logits"][b], out["preds"][b], out["margin"][b] = z, preds, margin
        if want_da:
            out["cos"][b], out["da"][b] = cos, da
    out.update(loss=loss / (B * Qn), correct=correct, dtau=dtau, dtau_abs=dtau_abs, da_rowsum_max=rowsum, status=int(status))
    return out
