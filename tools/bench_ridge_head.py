"""Times the ridge-regression head (--fewshot_head ridge) straight through the C ABI:

  * the head alone, training form, at (B, N, K, Qn, F) = (4, 5, 5, 75, 640), (4, 20, 5, 300, 640) and the same at F = 1600: the fused
    fumi_hip_ridge_head_step against the same head in plain torch ops on the GPU (bmm Gram matrix, torch.linalg.cholesky,
    cholesky_solve, bmm, F.cross_entropy, autograd backward for both feature sets and the two parameters) -- alternated block by block
    in one process, medians over the blocks;
  * a whole training step (encode with tape, head, encode_bwd) with Conv4 and with the bf16 ResNet-12 at 84 x 84 for the two workload
    shapes, and the head's share of that step (the head alone over the step);
  * the fp32 error of the head against the float64 restatement tests/ridge_head_ref.py on the features the two encoders give for
    random images at their initial weights, at --ridge_lambda 50, scale 1, with the condition number of the episodes' matrices.

python tools/bench_ridge_head.py [--out results.json] [--blocks 7] [--iters 500] [--step-iters 20] [--profile-only]
(--profile-only: a few calls of every route and nothing else, for a kernel trace)"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fumi_amd import hip  # noqa: E402
from ridge_head_ref import ridge_head_ref  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--iters", type=int, default=500)           # a block of the head alone: 0.05 - 1 s
ap.add_argument("--step-iters", type=int, default=20)      # a block of whole steps
ap.add_argument("--profile-only", action="store_true")
opt = ap.parse_args()

dev = torch.device("cuda:0")
ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
g = torch.Generator(device=dev).manual_seed(0)
LAM, SCALE = 50.0, 1.0


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
        timed(fn, 10)
    ts = {k: [] for k in routes}
    for _ in range(blocks):
        for k, fn in routes.items():
            ts[k].append(timed(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def labels(B, N, K, Qn):
    y_s = (torch.arange(N * K, device=dev) % N).repeat(B, 1)
    y_q = torch.randint(0, N, (B, Qn), device=dev, generator=g)
    return y_s, y_q


def ridge_params():
    return torch.tensor([math.log(LAM), SCALE], device=dev)


def head_case(B, N, K, Qn, Fd):
    """(fused, torch) closures of the training form on post-ReLU-like features."""
    y_s, y_q = labels(B, N, K, Qn)
    f_s = torch.relu(torch.randn(B, N * K, Fd, device=dev, generator=g))
    f_q = torch.relu(torch.randn(B, Qn, Fd, device=dev, generator=g))
    params = ridge_params()
    xs, xq, p = f_s.clone().requires_grad_(True), f_q.clone().requires_grad_(True), params.clone().requires_grad_(True)
    eye = torch.eye(N * K, device=dev)

    def fused():                               # predictions computed, every output allocated by the call
        return hip.ridge_head_step(ws, f_s, y_s, f_q, y_q, params, need_grad=True, grad_scale=1.0, n_way=N)

    def plain():
        Y = F.one_hot(y_s, N).to(torch.float32)
        M = torch.bmm(xs, xs.transpose(1, 2)) + torch.exp(p[0]) * eye
        A = torch.cholesky_solve(Y, torch.linalg.cholesky(M))
        z = p[1] * torch.bmm(xq, torch.bmm(xs.transpose(1, 2), A))
        loss = F.cross_entropy(z.reshape(-1, N), y_q.reshape(-1))
        preds = z.argmax(-1)
        return loss, (preds == y_q).sum(), torch.autograd.grad(loss, [xs, xq, p])
    return fused, plain


def encoder(backbone, size=84):
    if backbone == "conv4":
        from fumi_amd.models.conv4 import Conv4
        net = Conv4(3, 64, 4, size)
        return net, hip.conv4_encode, hip.conv4_encode_bwd
    from fumi_amd.models.resnet12 import CHANNELS, ResNet12
    net = ResNet12(3, CHANNELS, size)
    return net, hip.resnet12_encode, hip.resnet12_encode_bwd


def step_case(backbone, B, N, K, Qn, size=84):
    torch.manual_seed(1)
    net, encode, encode_bwd = encoder(backbone, size)
    theta = [p.detach().to(dev) for p in net.theta()]
    g_theta = [torch.empty_like(t) for t in theta]
    y_s, y_q = labels(B, N, K, Qn)
    x_s = torch.randn(B, N * K, 3, size, size, device=dev, generator=g)
    x_q = torch.randn(B, Qn, 3, size, size, device=dev, generator=g)
    params = ridge_params()

    def step():
        f_s, f_q = encode(ws_enc, x_s, x_q, theta, keep_tape=True)
        out = hip.ridge_head_step(ws, f_s, y_s, f_q, y_q, params, need_grad=True, grad_scale=1.0, n_way=N)
        encode_bwd(ws_enc, x_s, x_q, out["dfeats_s"], out["dfeats_q"], theta, g_theta=g_theta)

    def error():
        """fp32 head against float64 on this encoder's features."""
        f_s, f_q = encode(ws_enc, x_s, x_q, theta, keep_tape=False)
        out = hip.ridge_head_step(ws, f_s, y_s, f_q, y_q, params, need_grad=True, grad_scale=1.0, want_logits=True, n_way=N)
        ref = ridge_head_ref(f_s.cpu().numpy(), y_s.cpu().numpy(), f_q.cpu().numpy(), y_q.cpu().numpy(), params.cpu().numpy(), N)
        rel = lambda k: float(np.abs(out[k].cpu().numpy() - ref[k]).max() / max(np.abs(ref[k]).max(), 1e-30))
        e = {k: rel(k) for k in ("logits", "dfeats_s", "dfeats_q")}
        dp = out["dparams"].cpu().numpy()
        e["drho"], e["dalpha"] = (float(abs(dp[i] - ref["dparams"][i]) / max(abs(ref["dparams"][i]), 1e-30)) for i in (0, 1))
        e["loss"] = float(abs(float(out["loss"]) - ref["loss"]) / abs(ref["loss"]))
        e["cond"], e["feature_abs_max"] = ref["cond"], float(f_s.abs().max())
        return e
    return step, error, net.feature_dim


res = {"device": torch.cuda.get_device_name(0), "ridge_lambda": LAM, "ridge_scale": SCALE, "head": [], "step": [], "error": []}
WORKLOADS = [(4, 5, 5, 75), (4, 20, 5, 300)]
for Fd in (640, 1600):
    for B, N, K, Qn in WORKLOADS:
        fused, plain = head_case(B, N, K, Qn, Fd)
        if opt.profile_only:
            for _ in range(5):
                fused(); plain()
            continue
        t = alternate({"fused": fused, "torch": plain}, opt.iters, opt.blocks)
        res["head"].append(dict(B=B, N=N, K=K, Qn=Qn, F=Fd, fused_us=t["fused"], torch_us=t["torch"]))
        print(f"head B={B} N={N} K={K} Qn={Qn} F={Fd}: fused {t['fused'][0]:.1f} us (min {t['fused'][1]:.1f}, max {t['fused'][2]:.1f}), "
              f"torch ops {t['torch'][0]:.1f} us (min {t['torch'][1]:.1f}, max {t['torch'][2]:.1f})", flush=True)
for backbone in ("conv4", "resnet12"):
    for B, N, K, Qn in WORKLOADS:
        step, error, Fd = step_case(backbone, B, N, K, Qn)
        if opt.profile_only:
            for _ in range(2):
                step()
            continue
        e = error()
        res["error"].append(dict(backbone=backbone, B=B, N=N, K=K, Qn=Qn, F=Fd, **e))
        print(f"{backbone} features B={B} N={N} K={K} Qn={Qn} F={Fd}: fp32 against float64 " +
              ", ".join(f"{k} {v:.3g}" for k, v in e.items()), flush=True)
        t = alternate({"step": step}, opt.step_iters, opt.blocks)["step"]
        h = alternate({"fused": head_case(B, N, K, Qn, Fd)[0]}, opt.iters, 3)["fused"][0]
        res["step"].append(dict(backbone=backbone, size=84, B=B, N=N, K=K, Qn=Qn, F=Fd, step_us=t, episodes_per_s=B / t[0] * 1e6,
                                head_alone_us=h, head_share=h / t[0]))
        print(f"{backbone} 84x84 B={B} N={N} K={K} Qn={Qn}: {t[0] / 1e3:.2f} ms/step (min {t[1] / 1e3:.2f}, max {t[2] / 1e3:.2f}) = "
              f"{B / t[0] * 1e6:.1f} episodes/s; the head alone {h:.1f} us = {100 * h / t[0]:.3f} % of the step", flush=True)
torch.cuda.synchronize()
if ws.read_status() or ws_enc.read_status():
    raise SystemExit("a status bit was set")
if opt.out and not opt.profile_only:
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
