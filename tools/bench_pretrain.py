"""Times supervised pre-training (--model pretrain) straight through the C ABI:

  * the head alone at (M, F, C) = (128, 640, 64) and (256, 1600, 351): the fused fumi_hip_cls_head_step against the four-unit-op
    route (linear_fwd, ce_fwd_bwd, linear_bwd_data, linear_bwd_weight) -- both built from this commit, alternated block by block in
    one process, medians over the blocks;
  * images/s of a whole training step (encode with tape, head, encode_bwd) at 84 x 84, M = 128, R = 64, C = 64 with the bf16
    ResNet-12 and with Conv4, with either head, and the head's share of that step.

python tools/bench_pretrain.py [--out results.json] [--blocks 7] [--iters 4000] [--step-iters 100] [--profile-only]
(--profile-only: a few calls of every route and nothing else, for a kernel trace)"""
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
ap.add_argument("--iters", type=int, default=4000)          # a block of the head alone: 0.2 - 2 s
ap.add_argument("--step-iters", type=int, default=100)     # a block of whole steps: 0.2 - 0.9 s
ap.add_argument("--profile-only", action="store_true")
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
    x = torch.randn(M, F, device=dev, generator=g)
    W = torch.randn(C, F, device=dev, generator=g) * (2.0 / F ** 0.5)
    b = torch.zeros(C, device=dev)
    y = torch.randint(0, C, (M,), device=dev, generator=g)

    def fused():                               # like the unit-op route: predictions computed, every output allocated by the call
        return hip.cls_head_step(ws, x, y, W, b, need_grad=True, grad_scale=1.0)

    def unit():
        loss, dz, preds = hip.ce_fwd_bwd(ws, hip.linear_fwd(ws, x, W, b), y)
        return loss, hip.linear_bwd_data(ws, dz, W), hip.linear_bwd_weight(ws, dz, x)
    return fused, unit


def step_case(backbone, M=128, R=64, C=64, size=84):
    B, half = M // (2 * R), M // 2
    x = torch.randn(M, 3, size, size, device=dev, generator=g)
    y = torch.randint(0, C, (M,), device=dev, generator=g)
    x_s, x_q = x[:half].view(B, R, 3, size, size), x[half:].view(B, R, 3, size, size)
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
    b = torch.zeros(C, device=dev)

    def step(fused):
        f_s, f_q = enc(ws_enc, x_s, x_q, theta, keep_tape=True)
        feats = torch.cat((f_s.view(half, F), f_q.view(half, F)))
        if fused:
            df = hip.cls_head_step(ws, feats, y, W, b, need_grad=True)["dfeats"]
        else:
            _, dz, _ = hip.ce_fwd_bwd(ws, hip.linear_fwd(ws, feats, W, b), y)
            df = hip.linear_bwd_data(ws, dz, W)
            hip.linear_bwd_weight(ws, dz, feats)
        bwd(ws_enc, x_s, x_q, df[:half].view(B, R, F), df[half:].view(B, R, F), theta, g_theta=g_theta)
    return (lambda: step(True)), (lambda: step(False)), (M, F, C)


res = {"device": torch.cuda.get_device_name(0), "head": [], "step": []}
for shape in [(128, 640, 64), (256, 1600, 351)]:
    fused, unit = head_case(*shape)
    if opt.profile_only:
        for _ in range(5):
            fused(); unit()
        continue
    t = alternate({"fused": fused, "unit_ops": unit}, opt.iters, opt.blocks)
    res["head"].append(dict(M=shape[0], F=shape[1], C=shape[2], fused_us=t["fused"], unit_ops_us=t["unit_ops"]))
    print(f"head {shape}: fused {t['fused'][0]:.1f} us (min {t['fused'][1]:.1f}, max {t['fused'][2]:.1f}), four unit ops "
          f"{t['unit_ops'][0]:.1f} us (min {t['unit_ops'][1]:.1f}, max {t['unit_ops'][2]:.1f})", flush=True)
for backbone in ("resnet12", "conv4"):
    s_fused, s_unit, (M, F, C) = step_case(backbone)
    if opt.profile_only:
        for _ in range(2):
            s_fused(); s_unit()
        continue
    t = alternate({"fused": s_fused, "unit_ops": s_unit}, opt.step_iters, opt.blocks)
    h_fused, _ = head_case(M, F, C)
    h = alternate({"fused": h_fused}, opt.iters, 3)["fused"][0]
    res["step"].append(dict(backbone=backbone, M=M, F=F, C=C, size=84, step_fused_us=t["fused"], step_unit_ops_us=t["unit_ops"],
                            images_per_s=M / t["fused"][0] * 1e6, head_alone_us=h, head_share=h / t["fused"][0]))
    print(f"{backbone} 84x84 M={M}: {t['fused'][0] / 1e3:.2f} ms/step = {M / t['fused'][0] * 1e6:.0f} images/s with the fused head "
          f"({t['unit_ops'][0] / 1e3:.2f} ms with the unit ops); the head alone {h:.1f} us = {100 * h / t['fused'][0]:.2f} % of the step",
          flush=True)
torch.cuda.synchronize()
if ws.read_status() or ws_enc.read_status():
    raise SystemExit("a status bit was set")
if opt.out and not opt.profile_only:
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
