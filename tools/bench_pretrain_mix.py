"""Prices label smoothing, mixup and CutMix of --model pretrain straight through the C ABI.  Every pair of routes
is built from this commit and alternated block by block in one process; medians over the blocks:

  * the soft-target head (eps 0.1, lam 0.7, two labels) against the hard head at (M, F, C) = (128, 640, 64);
  * mix_images at (128, 3, 84, 84) in both modes: microseconds and effective TB/s (mixup: two reads and a write of every float;
    CutMix: one read and one write, the least a copy with a box can move);
  * a whole training step at 84 x 84, M = 128, R = 64, C = 64 with the bf16 ResNet-12 and with Conv4 on an already gathered batch:
    off = encode with tape, hard head, encode_bwd;  on = the host draw (mix_draw), its partner list copied to the device, mix_images
    (the modes in turn), the second labels y[partner], encode, the soft head with eps = 0.1, encode_bwd.

python tools/bench_pretrain_mix.py [--out results.json] [--blocks 7] [--iters 4000] [--step-iters 100]"""
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
from fumi_amd.dataset.supervised_pixels import mix_draw  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--iters", type=int, default=4000)
ap.add_argument("--step-iters", type=int, default=100)
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
    y_b = y[torch.randperm(M, device=dev, generator=g)]
    hard = lambda: hip.cls_head_step(ws, x, y, W, b, need_grad=True, grad_scale=1.0)
    soft = lambda: hip.cls_head_step_soft(ws, x, y, W, b, y_b=y_b, lam=0.7, smoothing=0.1, need_grad=True, grad_scale=1.0)
    return hard, soft


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
    b = torch.zeros(C, device=dev)
    count = [0]

    def step(on):
        xx, kw = x, None
        if on:
            count[0] += 1
            alphas = (0.4, 0.0) if count[0] % 2 else (0.0, 1.0)              # mixup and CutMix in turn
            mode, lam, box, partner = mix_draw(1, count[0], M, size, size, *alphas, 1.0)
            partner = torch.from_numpy(partner).to(dev)
            xx = hip.mix_images(ws, x, partner, mode=mode, lam=lam, box=box)
            kw = dict(y_b=y[partner], lam=lam, smoothing=0.1)
        x_s, x_q = xx[:half].view(B, R, 3, size, size), xx[half:].view(B, R, 3, size, size)
        f_s, f_q = enc(ws_enc, x_s, x_q, theta, keep_tape=True)
        feats = torch.cat((f_s.view(half, F), f_q.view(half, F)))
        if on:
            df = hip.cls_head_step_soft(ws, feats, y, W, b, need_grad=True, **kw)["dfeats"]
        else:
            df = hip.cls_head_step(ws, feats, y, W, b, need_grad=True)["dfeats"]
        bwd(ws_enc, x_s, x_q, df[:half].view(B, R, F), df[half:].view(B, R, F), theta, g_theta=g_theta)
    return (lambda: step(False)), (lambda: step(True))


res = {"device": torch.cuda.get_device_name(0), "head": [], "mix_images": [], "step": []}
M, F, C = 128, 640, 64
hard, soft = head_case(M, F, C)
t = alternate({"hard": hard, "soft": soft}, opt.iters, opt.blocks)
res["head"].append(dict(M=M, F=F, C=C, hard_us=t["hard"], soft_us=t["soft"], soft_over_hard=t["soft"][0] / t["hard"][0]))
print(f"head ({M},{F},{C}): hard {t['hard'][0]:.1f} us (min {t['hard'][1]:.1f}, max {t['hard'][2]:.1f}), soft {t['soft'][0]:.1f} us "
      f"(min {t['soft'][1]:.1f}, max {t['soft'][2]:.1f})", flush=True)

shape = (128, 3, 84, 84)
x = torch.randn(*shape, device=dev, generator=g)
partner = torch.randperm(shape[0], device=dev, generator=g)
nbytes = x.numel() * 4
t = alternate({"mixup": lambda: hip.mix_images(ws, x, partner, mode=hip.MIX_MIXUP, lam=0.7),
               "cutmix": lambda: hip.mix_images(ws, x, partner, mode=hip.MIX_CUTMIX, box=(10, 20, 52, 62))}, opt.iters, opt.blocks)
for name, moved in (("mixup", 3 * nbytes), ("cutmix", 2 * nbytes)):
    res["mix_images"].append(dict(shape=shape, mode=name, us=t[name], bytes=moved, tb_per_s=moved / t[name][0] * 1e-6))
    print(f"mix_images {shape} {name}: {t[name][0]:.1f} us (min {t[name][1]:.1f}, max {t[name][2]:.1f}), {moved / 1e6:.1f} MB = "
          f"{moved / t[name][0] * 1e-6:.2f} TB/s (allocation of the output included)", flush=True)

for backbone in ("resnet12", "conv4"):
    off, on = step_case(backbone)
    t = alternate({"off": off, "on": on}, opt.step_iters, opt.blocks)
    res["step"].append(dict(backbone=backbone, M=128, C=64, size=84, off_us=t["off"], on_us=t["on"],
                            added_us=t["on"][0] - t["off"][0], added_share=t["on"][0] / t["off"][0] - 1.0))
    print(f"{backbone} 84x84 M=128: off {t['off'][0] / 1e3:.3f} ms/step, on {t['on'][0] / 1e3:.3f} ms/step: "
          f"{t['on'][0] - t['off'][0]:+.1f} us = {100 * (t['on'][0] / t['off'][0] - 1):+.2f} %", flush=True)
torch.cuda.synchronize()
if ws.read_status() or ws_enc.read_status():
    raise SystemExit("a status bit was set")
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
