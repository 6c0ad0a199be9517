"""Numpy restatement of the set-to-set prototype adaptation (fumi_hip_feat_adapt_fwd / _bwd, csrc/featadapt.hip; DESIGN.md section
43), forward and full analytic backward.  In float64 it is the definition the kernels are held to (tests/test_feat_adapt_cpu.py ties
the backward to central finite differences of the forward); in float32 (``dtype=np.float32``) it is the same formulas at the kernels'
precision, used only as a yardstick for the bound.

Per episode, with F the feature width:
    P   = class means of feats_s by y_s                      [N,F]   (counts clamped to >= 1)
    Q   = P Wq^T,  K = P Wk^T,  V = P Wv^T                   [N,F]   (Wqkv [3F,F] = rows of Wq, Wk, Wv)
    A   = softmax_rows(Q K^T / sqrt(F))                      [N,N]   (row maximum subtracted before exp)
    O   = A V
    U   = O Wo^T + bo
    R   = P + U
    P'  = gamma * (R - mean_f R) / sqrt(var_f R + 1e-5) + beta       (biased variance)
A support label outside [0, N) sets ST_LABEL_RANGE: the row is left out of the mean and gets a zero gradient.  A class without a
support row sets ST_CLASS_MISSING, has P_n = 0 and still takes part in the attention."""
import numpy as np

ST_LABEL_RANGE, ST_CLASS_MISSING = 1, 2
LN_EPS = 1e-5
GRAD_NAMES = ("dfeats_s", "dwq", "dwk", "dwv", "dwo", "dbo", "dgamma", "dbeta")


def feat_adapt_fwd_ref(feats_s, y_s, wqkv, wo, bo, gamma, beta, n_way, dtype=np.float64, centred=False):
    """dict(protos [B,N,F] = P', status, and every intermediate the backward reads), all in ``dtype``.  ``centred`` evaluates the same
    function the way the kernels do: K and V from the prototypes relative to the episode's mean prototype m, O = A V + m Wv^T (the rows
    of A sum to 1, and a term common to a row of the scores does not reach the softmax); the float64 definition never needs it."""
    c = lambda t: np.asarray(t, dtype=dtype)
    xs, wqkv, wo, bo, gamma, beta = c(feats_s), c(wqkv), c(wo), c(bo), c(gamma), c(beta)
    ys = np.asarray(y_s, dtype=np.int64)
    B, S, F = xs.shape
    N = int(n_way)
    ok = (ys >= 0) & (ys < N)
    onehot = np.zeros((B, S, N), dtype=dtype)
    bi, si = np.nonzero(ok)
    onehot[bi, si, ys[bi, si]] = 1
    count = onehot.sum(axis=1)                                                     # [B, N]
    status = (0 if ok.all() else ST_LABEL_RANGE) | (ST_CLASS_MISSING if (count == 0).any() else 0)
    cnt = np.maximum(count, 1).astype(dtype)
    P = np.einsum("bsn,bsf->bnf", onehot, xs) / cnt[:, :, None]
    wq, wk, wv = wqkv[:F], wqkv[F:2 * F], wqkv[2 * F:]
    m = P.mean(axis=1, keepdims=True) if centred else np.zeros_like(P[:, :1])
    Q, K, V = P @ wq.T, (P - m) @ wk.T, (P - m) @ wv.T
    scale = dtype(1.0 / np.sqrt(float(F)))
    scores = np.einsum("bnf,bmf->bnm", Q, K) * scale
    e = np.exp(scores - scores.max(axis=-1, keepdims=True))
    A = e / e.sum(axis=-1, keepdims=True)
    O = A @ V + m @ wv.T
    U = O @ wo.T + bo
    R = P + U
    mean = R.mean(axis=-1, keepdims=True)
    var = ((R - mean) ** 2).mean(axis=-1, keepdims=True)
    rstd = 1 / np.sqrt(var + dtype(LN_EPS))
    xhat = (R - mean) * rstd
    protos = gamma * xhat + beta
    return dict(protos=protos, status=int(status), onehot=onehot, cnt=cnt, P=P, Q=Q, K=K, V=V, scores=scores, A=A, O=O, R=R, rstd=rstd,
                xhat=xhat, wq=wq, wk=wk, wv=wv, wo=wo, gamma=gamma, scale=scale)


def feat_adapt_bwd_ref(fw, dprotos):
    """The gradients of <dprotos, P'> from the forward's dict ``fw``: dfeats_s [B,S,F], dwq, dwk, dwv, dwo [F,F], dbo, dgamma,
    dbeta [F], in the forward's dtype.  The order is the kernels': LayerNorm, output projection, attention, the three projections and
    the residual, then the class means."""
    dt = fw["protos"].dtype
    dy = np.asarray(dprotos, dtype=dt)
    xhat, rstd, A = fw["xhat"], fw["rstd"], fw["A"]
    dgamma = (dy * xhat).sum(axis=(0, 1))
    dbeta = dy.sum(axis=(0, 1))
    g = dy * fw["gamma"]
    dR = rstd * (g - g.mean(axis=-1, keepdims=True) - xhat * (g * xhat).mean(axis=-1, keepdims=True))
    dbo = dR.sum(axis=(0, 1))
    dwo = np.einsum("bnf,bng->fg", dR, fw["O"])
    dO = dR @ fw["wo"]
    dV = np.einsum("bkn,bkf->bnf", A, dO)                                          # A^T dO
    dA = np.einsum("bnf,bmf->bnm", dO, fw["V"])                                    # dO V^T (centred: less a term common to the row)
    dS = A * (dA - (dA * A).sum(axis=-1, keepdims=True)) * fw["scale"]
    dQ = dS @ fw["K"]
    dK = np.einsum("bkn,bkf->bnf", dS, fw["Q"])                                    # dS^T Q
    P = fw["P"]
    dwq = np.einsum("bnf,bng->fg", dQ, P)
    dwk = np.einsum("bnf,bng->fg", dK, P)
    dwv = np.einsum("bnf,bng->fg", dV, P)
    dP = dR + dQ @ fw["wq"] + dK @ fw["wk"] + dV @ fw["wv"]
    dfeats_s = np.einsum("bsn,bnf->bsf", fw["onehot"], dP / fw["cnt"][:, :, None])
    return dict(dfeats_s=dfeats_s, dwq=dwq, dwk=dwk, dwv=dwv, dwo=dwo, dbo=dbo, dgamma=dgamma, dbeta=dbeta)


def feat_adapt_ref(feats_s, y_s, w, n_way, dprotos=None, dtype=np.float64, centred=False):
    """Forward and, with dprotos, backward in one dict; w = (wqkv, wo, bo, gamma, beta)."""
    fw = feat_adapt_fwd_ref(feats_s, y_s, *w, n_way, dtype=dtype, centred=centred)
    out = dict(fw)
    if dprotos is not None:
        out.update(feat_adapt_bwd_ref(fw, dprotos))
    return out


def rel_to_max(got, want):
    """The largest error over the tensor's largest float64 magnitude."""
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / max(float(np.abs(want).max()), 1e-300))
