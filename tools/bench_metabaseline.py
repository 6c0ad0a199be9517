"""Times the Meta-Baseline stage (--model metabaseline) straight through the C ABI:

  * the head alone, training form, at (B, N, K, Qn, F) = (4, 5, 5, 75, 640), (4, 20, 5, 300, 640) and the same at F = 1600: the fused
    fumi_hip_cos_proto_step against the same head in plain torch ops on the GPU (F.normalize, one-hot bmm prototypes, bmm,
    F.cross_entropy, autograd backward for both feature sets and the temperature) -- alternated block by block in one process,
    medians over the blocks;
  * episodes/s of a whole training step (encode with tape, head, encode_bwd) with the bf16 ResNet-12 at 84 x 84 for the two workload
    shapes, and the head's share of that step (the head alone over the step).

python tools/bench_metabaseline.py [--out results.json] [--blocks 7] [--iters 2000] [--step-iters 20] [--profile-only]
(--profile-only: a few calls of every route and nothing else, for a kernel trace)"""
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
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--iters", type=int, default=2000)          # a block of the head alone: 0.1 - 1 s
ap.add_argument("--step-iters", type=int, default=20)      # a block of whole steps
ap.add_argument("--profile-only", action="store_true")
opt = ap.parse_args()

dev = torch.device("cuda:0")
ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
g = torch.Generator(device=dev).manual_seed(0)
TAU = 10.0


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


def head_case(B, N, K, Qn, Fd):
    """(fused, torch) closures of the training form on post-ReLU-like features."""
    y_s, y_q = labels(B, N, K, Qn)
    f_s = torch.relu(torch.randn(B, N * K, Fd, device=dev, generator=g))
    f_q = torch.relu(torch.randn(B, Qn, Fd, device=dev, generator=g))
    tau = torch.tensor([TAU], device=dev)
    xs, xq, t = f_s.clone().requires_grad_(True), f_q.clone().requires_grad_(True), tau.clone().requires_grad_(True)

    def fused():                               # predictions computed, every output allocated by the call
        return hip.cos_proto_step(ws, f_s, y_s, f_q, y_q, tau, need_grad=True, grad_scale=1.0, n_way=N)

    def plain():
        onehot = F.one_hot(y_s, N).to(torch.float32)
        protos = torch.bmm(onehot.transpose(1, 2), xs) / onehot.sum(1).clamp(min=1)[:, :, None]
        z = t * torch.bmm(F.normalize(xq, dim=-1), F.normalize(protos, dim=-1).transpose(1, 2))
        loss = F.cross_entropy(z.reshape(-1, N), y_q.reshape(-1))
        preds = z.argmax(-1)
        return loss, (preds == y_q).sum(), torch.autograd.grad(loss, [xs, xq, t])
    return fused, plain


def step_case(B, N, K, Qn, size=84):
    from fumi_amd.models.resnet12 import CHANNELS, ResNet12
    net = ResNet12(3, CHANNELS, size)
    theta = [p.detach().to(dev) for p in net.theta()]
    g_theta = [torch.empty_like(t) for t in theta]
    y_s, y_q = labels(B, N, K, Qn)
    x_s = torch.randn(B, N * K, 3, size, size, device=dev, generator=g)
    x_q = torch.randn(B, Qn, 3, size, size, device=dev, generator=g)
    tau = torch.tensor([TAU], device=dev)

    def step():
        f_s, f_q = hip.resnet12_encode(ws_enc, x_s, x_q, theta, keep_tape=True)
        out = hip.cos_proto_step(ws, f_s, y_s, f_q, y_q, tau, need_grad=True, grad_scale=1.0, n_way=N)
        hip.resnet12_encode_bwd(ws_enc, x_s, x_q, out["dfeats_s"], out["dfeats_q"], theta, g_theta=g_theta)
    return step, net.feature_dim


res = {"device": torch.cuda.get_device_name(0), "head": [], "step": []}
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
for B, N, K, Qn in WORKLOADS:
    step, Fd = step_case(B, N, K, Qn)
    if opt.profile_only:
        for _ in range(2):
            step()
        continue
    t = alternate({"step": step}, opt.step_iters, opt.blocks)["step"]
    h = alternate({"fused": head_case(B, N, K, Qn, Fd)[0]}, opt.iters, 3)["fused"][0]
    res["step"].append(dict(backbone="resnet12", size=84, B=B, N=N, K=K, Qn=Qn, F=Fd, step_us=t, episodes_per_s=B / t[0] * 1e6,
                            head_alone_us=h, head_share=h / t[0]))
    print(f"resnet12 84x84 B={B} N={N} K={K} Qn={Qn}: {t[0] / 1e3:.2f} ms/step (min {t[1] / 1e3:.2f}, max {t[2] / 1e3:.2f}) = "
          f"{B / t[0] * 1e6:.1f} episodes/s; the head alone {h:.1f} us = {100 * h / t[0]:.3f} % of the step", flush=True)
torch.cuda.synchronize()
if ws.read_status() or ws_enc.read_status():
    raise SystemExit("a status bit was set")
if opt.out and not opt.profile_only:
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
