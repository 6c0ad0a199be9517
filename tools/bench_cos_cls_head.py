"""Prices the cosine classifier head of --model pretrain straight through the C ABI.  Every pair of routes is
built from this commit and alternated block by block in one process; medians over the blocks:

  * the head alone, training form: fumi_hip_cos_cls_head_step against fumi_hip_cls_head_step at the same (M, F, C), at
    (128, 640, 64), (128, 1600, 64) and (512, 640, 351);
  * a whole training step at 84 x 84, M = 128, R = 64, C = 64 with the bf16 ResNet-12 and with Conv4 on an already gathered batch:
    encode with tape, the head, encode_bwd -- once with the linear head, once with the cosine head -- and the cosine head's share of
    its step (head alone over step).

python tools/bench_cos_cls_head.py [--out results.json] [--blocks 7] [--iters 2000] [--step-iters 50]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fumi_amd import hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--iters", type=int, default=2000)
ap.add_argument("--step-iters", type=int, default=50)
opt = ap.parse_args()

dev = torch.device("cuda:0")
ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
g = torch.Generator(device=dev).manual_seed(0)


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


def head_case(M, F, C):
    """Both heads write into tensors allocated once: the kernels are timed, not the allocator."""
    x = torch.randn(M, F, device=dev, generator=g)
    W = torch.randn(C, F, device=dev, generator=g) * (2.0 / F ** 0.5)
    b, tau = torch.zeros(C, device=dev), torch.full((1,), 10.0, device=dev)
    y = torch.randint(0, C, (M,), device=dev, generator=g)
    df, gW, gb, dt = torch.empty_like(x), torch.empty_like(W), torch.empty_like(b), torch.empty_like(tau)
    linear = lambda: hip.cls_head_step(ws, x, y, W, b, need_grad=True, grad_scale=1.0, dfeats=df, gW=gW, gb=gb)
    cosine = lambda: hip.cos_cls_head_step(ws, x, y, W, tau, need_grad=True, grad_scale=1.0, dfeats=df, gW=gW, dtau=dt)
    return linear, cosine


def step_case(backbone, M=128, R=64, C=64, size=84):
    B, half = M // (2 * R), M // 2
    x = torch.randn(M, 3, size, size, device=dev, generator=g)
    y = torch.randint(0, C, (M,), device=dev, generator=g)
    if backbone == "conv4":
        from fumi_amd.models.conv4 import Conv4
        net, enc, bwd = Conv4(3, 64, 4, size), hip.conv4_encode, hip.conv4_encode_bwd
    else:
        from fumi_amd.models.resnet12 import CHANNELS, ResNet12
        net, enc, bwd = ResNet12(3, CHANNELS, size), hip.resnet12_encode, hip.resnet12_encode_bwd
    theta = [p.detach().to(dev) for p in net.theta()]
    g_theta = [torch.empty_like(t) for t in theta]
    F = net.feature_dim
    W = torch.randn(C, F, device=dev, generator=g) * (2.0 / F ** 0.5)
    b, tau = torch.zeros(C, device=dev), torch.full((1,), 10.0, device=dev)
    x_s, x_q = x[:half].view(B, R, 3, size, size), x[half:].view(B, R, 3, size, size)

    def step(cosine):
        f_s, f_q = enc(ws_enc, x_s, x_q, theta, keep_tape=True)
        feats = torch.cat((f_s.view(half, F), f_q.view(half, F)))
        if cosine:
            df = hip.cos_cls_head_step(ws, feats, y, W, tau, need_grad=True)["dfeats"]
        else:
            df = hip.cls_head_step(ws, feats, y, W, b, need_grad=True)["dfeats"]
        bwd(ws_enc, x_s, x_q, df[:half].view(B, R, F), df[half:].view(B, R, F), theta, g_theta=g_theta)
    return (lambda: step(False)), (lambda: step(True)), F


res = {"device": torch.cuda.get_device_name(0), "head": [], "step": []}
for M, F, C in ((128, 640, 64), (128, 1600, 64), (512, 640, 351)):
    linear, cosine = head_case(M, F, C)
    t = alternate({"linear": linear, "cosine": cosine}, opt.iters, opt.blocks)
    res["head"].append(dict(M=M, F=F, C=C, linear_us=t["linear"], cosine_us=t["cosine"], cosine_over_linear=t["cosine"][0] / t["linear"][0]))
    print(f"head ({M},{F},{C}): linear {t['linear'][0]:.1f} us (min {t['linear'][1]:.1f}, max {t['linear'][2]:.1f}), cosine "
          f"{t['cosine'][0]:.1f} us (min {t['cosine'][1]:.1f}, max {t['cosine'][2]:.1f}): x{t['cosine'][0] / t['linear'][0]:.3f}", flush=True)

for backbone in ("resnet12", "conv4"):
    lin, cos, F = step_case(backbone)
    t = alternate({"linear": lin, "cosine": cos}, opt.step_iters, opt.blocks)
    h = alternate(dict(zip(("linear", "cosine"), head_case(128, F, 64))), opt.iters, 3)
    res["step"].append(dict(backbone=backbone, M=128, F=F, C=64, size=84, linear_us=t["linear"], cosine_us=t["cosine"],
                            added_us=t["cosine"][0] - t["linear"][0], added_share=t["cosine"][0] / t["linear"][0] - 1.0,
                            head_us=h["cosine"][0], head_share=h["cosine"][0] / t["cosine"][0]))
    print(f"{backbone} 84x84 M=128 F={F}: linear {t['linear'][0] / 1e3:.3f} ms/step, cosine {t['cosine'][0] / 1e3:.3f} ms/step: "
          f"{t['cosine'][0] - t['linear'][0]:+.1f} us = {100 * (t['cosine'][0] / t['linear'][0] - 1):+.2f} %; the cosine head alone "
          f"{h['cosine'][0]:.1f} us = {100 * h['cosine'][0] / t['cosine'][0]:.2f} % of its step", flush=True)
torch.cuda.synchronize()
if ws.read_status() or ws_enc.read_status():
    raise SystemExit("a status bit was set")
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
