"""Times the MetaOptNet-SVM head (--fewshot_head svm) straight through the C ABI:

  * the head alone, training and forward form, at B = 32 for 5-way 5-shot (Qn = 75) and 20-way 5-shot (Qn = 300), at F = 640 and
    F = 1600, with each form of the K' alpha product forced (VALU loop, f32 MFMA): the fused fumi_hip_svm_head_step against the same
    algorithm in plain torch fp32 ops on the GPU (bmm Gram matrix, the FISTA steps with a sort-based exact projection, the logits and
    cross-entropy, the conjugate gradients and the gradient formulas written out: no autograd through the loop) -- alternated block by
    block in one process after a warm-up of each, medians over the blocks;
  * the time of one FISTA step and of one conjugate-gradient step, from calls that differ only in the step count;
  * a whole training step (encode with tape, head, encode_bwd) with the bf16 ResNet-12 at 84 x 84 at B = 4, and the head's share of it.

python tools/bench_svm_head.py [--out results.json] [--blocks 5] [--iters 20] [--step-iters 10]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fumi_amd import hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--step-iters", type=int, default=10)
opt = ap.parse_args()

dev = torch.device("cuda:0")
ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
g = torch.Generator(device=dev).manual_seed(0)
C, EPS, SCALE, T, TB = 0.1, 1.0, 1.0, 120, 40


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6          # us per call


def alternate(routes, iters, blocks):
    """{name: (median us, min us, max us)} of routes = {name: fn}, timed block by block in turn after a warm-up of each."""
    for fn in routes.values():
        timed(fn, 3)
    ts = {k: [] for k in routes}
    for _ in range(blocks):
        for k, fn in routes.items():
            ts[k].append(timed(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def torch_project(V, U):
    """The exact projection of tests/svm_head_ref.py in torch ops."""
    N = V.shape[-1]
    b = V - U
    bs, order = torch.sort(b, dim=-1, stable=True)
    vs, us = torch.gather(V, -1, order), torch.gather(U, -1, order)
    m = torch.arange(1, N + 1, device=V.device, dtype=V.dtype)
    tau_m = (vs.cumsum(-1) + (us.sum(-1, keepdim=True) - us.cumsum(-1))) / m
    ok = tau_m > bs
    ok[..., 0] = True
    rank = (ok * m).amax(-1, keepdim=True).long() - 1
    d = V - torch.gather(tau_m, -1, rank)
    return torch.minimum(d, U), d >= U


def torch_head(xs, ys, xq, yq, N, steps, bwd_steps, train):
    """The same algorithm in torch fp32 ops (the yardstick): fit, logits, loss and, with ``train``, the implicit gradients."""
    B, S, _ = xs.shape
    Y = F.one_hot(ys, N).float()
    U = C * Y
    Kp = torch.bmm(xs, xs.transpose(1, 2)) + EPS * torch.eye(S, device=xs.device)
    invL = 1.0 / Kp.abs().sum(-1).amax(-1)[:, None, None]
    alpha = torch.zeros_like(Y); Zt = alpha
    t = 1.0
    bound = None
    for _ in range(steps):
        new, bound = torch_project(Zt - (torch.bmm(Kp, Zt) - Y) * invL, U)
        tn = (1.0 + (1.0 + 4.0 * t * t) ** 0.5) / 2.0
        Zt = new + ((t - 1.0) / tn) * (new - alpha)
        alpha, t = new, tn
    W = torch.bmm(xs.transpose(1, 2), alpha)
    u = torch.bmm(xq, W)
    z = SCALE * u
    loss = F.cross_entropy(z.reshape(-1, N), yq.reshape(-1))
    correct = (z.argmax(-1) == yq).sum()
    if not train:
        return loss, correct
    dZ = (torch.softmax(z, -1) - F.one_hot(yq, N).float()) / (B * yq.shape[1])
    M = torch.bmm(xq.transpose(1, 2), dZ)
    free = ~bound
    nf = free.sum(-1, keepdim=True)

    def P(v):
        mean = (v * free).sum(-1, keepdim=True) / nf.clamp(min=1)
        return torch.where(free & (nf >= 2), v - mean, torch.zeros_like(v))
    r = P(SCALE * torch.bmm(xs, M))
    p, d = torch.zeros_like(r), r
    rr = (r * r).sum((1, 2), keepdim=True)
    for _ in range(bwd_steps):                   # (no early exit: the yardstick does not synchronise)
        q = P(torch.bmm(Kp, d))
        a = rr / (d * q).sum((1, 2), keepdim=True).clamp(min=1e-30)
        p, r = p + a * d, r - a * q
        rn = (r * r).sum((1, 2), keepdim=True)
        d = r + (rn / rr.clamp(min=1e-30)) * d
        rr = rn
    V = torch.bmm(xs.transpose(1, 2), p)
    gXs = torch.bmm(alpha, (SCALE * M - V).transpose(1, 2)) - torch.bmm(p, W.transpose(1, 2))
    return loss, correct, gXs, SCALE * torch.bmm(dZ, W.transpose(1, 2)), (dZ * u).sum()


def head_case(B, N, K, Qn, Fd):
    y_s = (torch.arange(N * K, device=dev) % N).repeat(B, 1)
    y_q = torch.randint(0, N, (B, Qn), device=dev, generator=g)
    centres = torch.randn(B, N, Fd, device=dev, generator=g)
    rows = lambda y: F.normalize(torch.gather(centres, 1, y[..., None].expand(-1, -1, Fd))
                                 + 0.8 * torch.randn(*y.shape, Fd, device=dev, generator=g), dim=-1) * 3.0
    f_s, f_q = rows(y_s), rows(y_q)
    scale = torch.tensor([SCALE], device=dev)

    def fused(train, steps=T, bwd_steps=TB):
        return lambda: hip.svm_head_step(ws, f_s, y_s, f_q, y_q, scale, C=C, eps=EPS, steps=steps, bwd_steps=bwd_steps, need_grad=train,
                                         n_way=N)

    def plain(train):
        return lambda: torch_head(f_s, y_s, f_q, y_q, N, T, TB, train)
    return fused, plain


res = {"device": torch.cuda.get_device_name(0), "C": C, "eps": EPS, "steps": T, "bwd_steps": TB, "head": [], "per_step": [], "step": []}
for Fd in (640, 1600):
    for B, N, K, Qn in ((32, 5, 5, 75), (32, 20, 5, 300)):
        fused, plain = head_case(B, N, K, Qn, Fd)
        for train in (True, False):
            routes = {}
            for form in ("valu", "mfma"):
                def run(form=form, fn=fused(train)):
                    hip.svm_set_form(form)
                    return fn()
                routes[form] = run
            routes["torch"] = plain(train)
            t = alternate(routes, opt.iters, opt.blocks)
            res["head"].append(dict(B=B, N=N, K=K, Qn=Qn, F=Fd, train=train, **{k + "_us": v for k, v in t.items()}))
            print(f"head B={B} N={N} K={K} Qn={Qn} F={Fd} {'training' if train else 'forward'}: " +
                  ", ".join(f"{k} {v[0]:.1f} us (min {v[1]:.1f}, max {v[2]:.1f})" for k, v in t.items()), flush=True)
        if Fd == 640:                            # one FISTA step, one conjugate-gradient step: calls that differ in the step count only
            for form in ("valu", "mfma"):
                hip.svm_set_form(form)
                t = alternate({"T20": fused(False, steps=20), "T120": fused(False, steps=120), "Tb2": fused(True, 20, 2),
                               "Tb12": fused(True, 20, 12)}, opt.iters, opt.blocks)
                fit, cg = (t["T120"][0] - t["T20"][0]) / 100.0, (t["Tb12"][0] - t["Tb2"][0]) / 10.0
                res["per_step"].append(dict(B=B, N=N, K=K, form=form, fista_step_us=fit, cg_step_us=cg))
                print(f"per step B={B} N={N} K={K} {form}: FISTA {fit:.2f} us, conjugate gradients {cg:.2f} us", flush=True)
hip.svm_set_form(None)

from fumi_amd.models.resnet12 import CHANNELS, ResNet12  # noqa: E402
for B, N, K, Qn in ((4, 5, 5, 75), (4, 20, 5, 300)):
    torch.manual_seed(1)
    net = ResNet12(3, CHANNELS, 84)
    theta = [p.detach().to(dev) for p in net.theta()]
    g_theta = [torch.empty_like(t) for t in theta]
    y_s = (torch.arange(N * K, device=dev) % N).repeat(B, 1)
    y_q = torch.randint(0, N, (B, Qn), device=dev, generator=g)
    x_s = torch.randn(B, N * K, 3, 84, 84, device=dev, generator=g)
    x_q = torch.randn(B, Qn, 3, 84, 84, device=dev, generator=g)
    scale = torch.tensor([SCALE], device=dev)
    kw = dict(C=C, eps=EPS, steps=T, bwd_steps=TB, need_grad=True, n_way=N)

    def step():
        f_s, f_q = hip.resnet12_encode(ws_enc, x_s, x_q, theta, keep_tape=True)
        out = hip.svm_head_step(ws, f_s, y_s, f_q, y_q, scale, **kw)
        hip.resnet12_encode_bwd(ws_enc, x_s, x_q, out["dfeats_s"], out["dfeats_q"], theta, g_theta=g_theta)
        return out
    f_s, f_q = hip.resnet12_encode(ws_enc, x_s, x_q, theta, keep_tape=False)
    f_s, f_q = f_s.clone(), f_q.clone()
    stats = step()["stats"].amax(0).tolist()
    t = alternate({"step": step}, opt.step_iters, opt.blocks)["step"]
    h = alternate({"head": lambda: hip.svm_head_step(ws, f_s, y_s, f_q, y_q, scale, **kw)}, opt.iters, 3)["head"][0]
    res["step"].append(dict(backbone="resnet12", size=84, B=B, N=N, K=K, Qn=Qn, F=net.feature_dim, step_us=t, head_alone_us=h,
                            head_share=h / t[0], kkt=stats[0], cg_res=stats[1], feature_abs_max=float(f_s.abs().max())))
    print(f"resnet12 84x84 B={B} N={N} K={K} Qn={Qn}: {t[0] / 1e3:.2f} ms/step (min {t[1] / 1e3:.2f}, max {t[2] / 1e3:.2f}); the head "
          f"alone {h:.1f} us = {100 * h / t[0]:.2f} % of the step; KKT residual {stats[0]:.2e}, CG residual {stats[1]:.2e}", flush=True)
torch.cuda.synchronize()
if ws.read_status() or ws_enc.read_status():
    raise SystemExit("a status bit was set")
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
