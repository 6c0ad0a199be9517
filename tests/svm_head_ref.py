"""Numpy restatement of the fused MetaOptNet-SVM head (fumi_hip_svm_head_step, csrc/svmhead.hip), float64 by default: exactly the
iteration the kernels run.  tests/test_svm_head_cpu.py ties it to independent witnesses (the KKT conditions of the dual, central finite
differences of the loss, a brute-force projection).

Per episode, with X the support rows [S,F], Y their one-hot labels [S,N], Fq the query rows [Qn,F], K' = X X^T + eps I:
    alpha* = argmin 1/2 tr(alpha^T K' alpha) - <alpha, Y>   s.t.  alpha_ik <= C Y_ik,  sum_k alpha_ik = 0        (Crammer-Singer dual)
    W = X^T alpha*,   z = scale Fq W.
Fit: T steps of FISTA from zero with the step 1 / L, L = max_i sum_j |K'_ij|, t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2:
    G = K' Zt - Y,  alpha+ = proj(Zt - G / L),  Zt <- alpha+ + (t_k - 1) / t_{k+1} (alpha+ - alpha).
proj, per row, with v the row, u = C Y_i: a = min(v - tau, u) with tau the root of sum_k min(v_k - tau, u_k) = 0, found exactly from the
breakpoints b_k = v_k - u_k: with the entries ordered by (b_k, k), the candidate of rank m frees the first m entries,
tau_m = (sum_free v + sum_bound u) / m, and is consistent on its lower side when tau_m > b_(m); the candidate kept is the one of the
largest such rank (in exact arithmetic the one consistent candidate; rank 1 always counts).  Bound mask: v_k - tau >= u_k.
A support row whose label is outside [0, N) has a zero row of Y and a zero row and column of X X^T: alpha_i = 0, every entry bound.

Backward (the implicit gradient at the fitted point, on a bound mask): free = not bound, P zeroes the bound entries and takes from every
row the mean over its free entries (a row with fewer than two free entries becomes zero), dZ = gs (softmax(z) - onehot(y_q)),
gs = grad_scale / (B Qn):
    M = Fq^T dZ,  g = scale X M,  p: P K' P p = P g by Tb steps of conjugate gradients from zero (stopped when r.r <= CG_FLOOR r0.r0),
    V = X^T p,  gX = alpha (scale M - V)^T - p W^T,  gFq = scale dZ W^T,  gscale = <dZ, Fq W>.
stats [B,2] = (max |alpha - proj(alpha - (K' alpha - Y))|, sqrt(r.r at the end / r.r at the start) of the CG, 0 for a zero start)."""
import numpy as np

ST_LABEL_RANGE, ST_CLASS_MISSING = 1, 2
CG_FLOOR = 1e-12                                # of r0.r0: the conjugate gradients end at a relative residual of 1e-6


def project_rows(V, U, valid=None):
    """(a, bound, margin) of the rows of V [R,N] on {a <= U, sum a = 0}.  ``valid`` [R] False: a = 0 and every entry bound."""
    R, N = V.shape
    b = V - U
    order = np.argsort(b, axis=1, kind="stable")                      # by (b_k, k)
    vs, us, bs = (np.take_along_axis(a, order, axis=1) for a in (V, U, b))
    m = np.arange(1, N + 1, dtype=V.dtype)
    tau_m = ((np.cumsum(vs, axis=1) + (us.sum(axis=1, keepdims=True) - np.cumsum(us, axis=1))) / m).astype(V.dtype)
    ok = tau_m > bs
    ok[:, 0] = True
    rank = N - 1 - np.argmax(ok[:, ::-1], axis=1)                     # the largest consistent rank (0-based)
    tau = np.take_along_axis(tau_m, rank[:, None], axis=1)
    d = (V - tau).astype(V.dtype)
    a, bound = np.minimum(d, U), d >= U
    margin = d - U                                                    # signed: >= 0 bound, < 0 free
    if valid is not None:
        a = np.where(valid[:, None], a, 0).astype(V.dtype)
        bound = np.where(valid[:, None], bound, True)
        margin = np.where(valid[:, None], margin, np.inf)             # (a row left out is bound whatever the values are)
    return a, bound, margin


def _P(v, free):
    nf = free.sum(axis=1, keepdims=True)
    mean = np.where(free, v, 0).sum(axis=1, keepdims=True) / np.maximum(nf, 1)
    return np.where(free & (nf >= 2), v - mean, 0).astype(v.dtype)


def svm_fit(X, y, N, C, eps, T, dtype=np.float64):
    """One episode: dict(alpha [S,N], bound [S,N] bool, margin [S,N] (of the last projection: >= 0 bound, < 0 free), Kp [S,S], kkt)."""
    dt = np.dtype(dtype).type
    X = np.asarray(X).astype(dtype)
    y = np.asarray(y, dtype=np.int64)
    S = X.shape[0]
    ok = (y >= 0) & (y < N)
    Y = np.zeros((S, N), dtype=dtype)
    Y[np.nonzero(ok)[0], y[ok]] = 1
    U = (dt(C) * Y).astype(dtype)
    Kp = (X @ X.T).astype(dtype)
    Kp = np.where(ok[:, None] & ok[None, :], Kp, 0).astype(dtype) + dt(eps) * np.eye(S, dtype=dtype)
    invL = dt(1) / np.abs(Kp).sum(axis=1).max()
    alpha = np.zeros((S, N), dtype=dtype)
    Zt = alpha.copy()
    t = dt(1)
    bound = np.ones((S, N), dtype=bool); margin = np.zeros((S, N), dtype=dtype)
    for _ in range(int(T)):
        G = (Kp @ Zt - Y).astype(dtype)
        new, bound, margin = project_rows((Zt - G * invL).astype(dtype), U, ok)
        tn = (dt(1) + np.sqrt(dt(1) + dt(4) * t * t)) / dt(2)
        Zt = (new + ((t - dt(1)) / tn) * (new - alpha)).astype(dtype)
        alpha, t = new, tn
    G = (Kp @ alpha - Y).astype(dtype)
    pa, _, _ = project_rows((alpha - G).astype(dtype), U, ok)
    return dict(alpha=alpha, bound=bound, margin=margin, Kp=Kp, kkt=float(np.abs(alpha - pa).max()), ok=ok)


def svm_cg(Kp, g, free, Tb, floor=CG_FLOOR):
    """(p, relative residual) of P K' P p = P g: Tb steps of conjugate gradients from zero, ended when r.r <= floor r0.r0."""
    dtype = g.dtype
    r = _P(g, free)
    p = np.zeros_like(r)
    d = r.copy()
    rr = rr0 = (r * r).sum()
    for _ in range(int(Tb)):
        if not rr > dtype.type(floor) * rr0:
            break
        q = _P((Kp @ d).astype(dtype), free)
        a = rr / (d * q).sum()
        p = (p + a * d).astype(dtype)
        r = (r - a * q).astype(dtype)
        rn = (r * r).sum()
        d = (r + (rn / rr) * d).astype(dtype)
        rr = rn
    return p, float(np.sqrt(rr / rr0)) if rr0 > 0 else 0.0


def svm_head_ref(feats_s, y_s, feats_q, y_q, n_way, scale=1.0, C=0.1, eps=1.0, steps=120, bwd_steps=40, grad_scale=1.0, mask=None,
                 need_grad=True, dtype=np.float64, cg_floor=CG_FLOOR):
    """dict(loss, correct, preds [B,Qn], logits [B,Qn,N], margin [B,Qn] (top-two logit gap), status, alpha [B,S,N], bound [B,S,N] bool,
    fit_margin [B,S,N] (|distance of the last projection's entry from its bound|), stats [B,2], gXs, gXq, gscale).  ``mask`` [B,S,N]
    (bool, True = bound) replaces the fit's own bound mask in the backward; ``cg_floor`` the kernel's floor of the conjugate gradients
    (the finite-difference test runs them to 1e-14 of the start)."""
    dt = np.dtype(dtype).type
    xs = np.asarray(feats_s).astype(dtype)
    xq = np.asarray(feats_q).astype(dtype)
    ys = np.asarray(y_s, dtype=np.int64)
    yq = np.asarray(y_q, dtype=np.int64)
    N = int(n_way)
    B, S, F = xs.shape
    Qn = xq.shape[1]
    ok_q = (yq >= 0) & (yq < N)
    ok_s = (ys >= 0) & (ys < N)
    missing = any(not np.isin(np.arange(N), ys[b][ok_s[b]]).all() for b in range(B))
    status = (0 if ok_s.all() and ok_q.all() else ST_LABEL_RANGE) | (ST_CLASS_MISSING if missing else 0)
    fits = [svm_fit(xs[b], ys[b], N, C, eps, steps, dtype) for b in range(B)]
    alpha = np.stack([f["alpha"] for f in fits])
    bound = np.stack([f["bound"] for f in fits])
    xz = np.where(ok_s[..., None], xs, 0).astype(dtype)                 # a support row left out counts as a zero row
    W = np.einsum("bsf,bsn->bfn", xz, alpha).astype(dtype)
    u = np.einsum("bqf,bfn->bqn", xq, W).astype(dtype)
    z = (dt(scale) * u).astype(dtype)
    mx = z.max(axis=-1, keepdims=True)
    e = np.exp(z - mx)
    lse = (mx + np.log(e.sum(axis=-1, keepdims=True)))[..., 0]
    preds = z.argmax(axis=-1)
    top2 = np.sort(z, axis=-1)[..., -2:]
    yc = np.where(ok_q, yq, 0)
    z_y = np.take_along_axis(z, yc[..., None], axis=-1)[..., 0]
    loss = np.where(ok_q, lse - z_y, 0).sum() / (B * Qn)
    out = dict(loss=float(loss), correct=float(((preds == yq) & ok_q).sum()), preds=preds, logits=z, margin=top2[..., 1] - top2[..., 0],
               status=int(status), alpha=alpha, bound=bound, fit_margin=np.abs(np.stack([f["margin"] for f in fits])),
               stats=np.array([[f["kkt"], 0.0] for f in fits]))
    if not need_grad:
        return out
    gs = dt(grad_scale) / dt(B * Qn)
    onehot = np.zeros_like(z)
    np.put_along_axis(onehot, yc[..., None], 1, axis=-1)
    dZ = (np.where(ok_q[..., None], e / e.sum(axis=-1, keepdims=True) - onehot, 0) * gs).astype(dtype)
    bm = bound if mask is None else np.asarray(mask).astype(bool)
    gXs = np.zeros_like(xs)
    for b in range(B):
        M = (xq[b].T @ dZ[b]).astype(dtype)
        g = (dt(scale) * (xz[b] @ M)).astype(dtype)
        p, res = svm_cg(fits[b]["Kp"], g, ~bm[b], bwd_steps, cg_floor)
        out["stats"][b, 1] = res
        V = (xz[b].T @ p).astype(dtype)
        gXs[b] = np.where(ok_s[b][:, None], alpha[b] @ (dt(scale) * M - V).T - p @ W[b].T, 0)
    out.update(gXs=gXs, gXq=(dt(scale) * np.einsum("bqn,bfn->bqf", dZ, W)).astype(dtype), gscale=float((dZ * u).sum()))
    return out
