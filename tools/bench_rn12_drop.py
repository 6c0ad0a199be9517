"""Prices DropBlock / dropout in the bf16 ResNet-12 (--drop_rate) straight through the C ABI.  Both routes are
built from this commit and alternated block by block in one process; medians over the blocks:

  * a whole --model pretrain training step at 84 x 84, M = 128, R = 64, C = 64 on an already gathered batch: encode with tape, the
    linear head, encode_bwd -- once through fumi_hip_resnet12_encode / _bwd, once through the _drop entries at rate 0.1 (dropout on
    blocks 1-2, DropBlock 5 on blocks 3-4: the MetaOptNet / RFS network);
  * the two drop launches on their own (fumi_hip_rn12_drop_apply: count, then apply) on each of the four pooled maps of one
    batch-statistics group of 64 images, and what a step issues of them (two groups, forward and backward).

python tools/bench_rn12_drop.py [--out results.json] [--blocks 7] [--iters 500] [--step-iters 20]"""
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
from fumi_amd.models.resnet12 import CHANNELS, ResNet12  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--step-iters", type=int, default=20)
opt = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("bench_rn12_drop needs the MI355X: a timing taken anywhere else says nothing")
dev = torch.device("cuda:0")
ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
g = torch.Generator(device=dev).manual_seed(0)
RATE, BLOCKS, SEED = 0.1, [1, 1, 5, 5], 0x5EED0123456789AB


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


M, R, C, SIZE = 128, 64, 64, 84
B, half = M // (2 * R), M // 2
x = torch.randn(M, 3, SIZE, SIZE, device=dev, generator=g)
y = torch.randint(0, C, (M,), device=dev, generator=g)
net = ResNet12(3, CHANNELS, SIZE)
theta = [p.detach().to(dev) for p in net.theta()]
g_theta = [torch.empty_like(t) for t in theta]
F = net.feature_dim
W = torch.randn(C, F, device=dev, generator=g) * (2.0 / F ** 0.5)
b = torch.zeros(C, device=dev)
x_s, x_q = x[:half].view(B, R, 3, SIZE, SIZE), x[half:].view(B, R, 3, SIZE, SIZE)
rates = [RATE] * 4


def step(drop):
    if drop:
        f_s, f_q = hip.resnet12_encode_drop(ws_enc, x_s, x_q, theta, rates, BLOCKS, SEED, keep_tape=True)
    else:
        f_s, f_q = hip.resnet12_encode(ws_enc, x_s, x_q, theta, keep_tape=True)
    df = hip.cls_head_step(ws, torch.cat((f_s.view(half, F), f_q.view(half, F))), y, W, b, need_grad=True)["dfeats"]
    if drop:
        hip.resnet12_encode_bwd_drop(ws_enc, x_s, x_q, df[:half].view(B, R, F), df[half:].view(B, R, F), theta, rates, BLOCKS, SEED,
                                     g_theta=g_theta)
    else:
        hip.resnet12_encode_bwd(ws_enc, x_s, x_q, df[:half].view(B, R, F), df[half:].view(B, R, F), theta, g_theta=g_theta)


res = {"device": torch.cuda.get_device_name(0), "shape": dict(M=M, R=R, C=C, size=SIZE, rate=RATE, blocks=BLOCKS)}
t = alternate({"off": lambda: step(False), "on": lambda: step(True)}, opt.step_iters, opt.blocks)
res["step"] = dict(off_us=t["off"], on_us=t["on"], added_us=t["on"][0] - t["off"][0], added_share=t["on"][0] / t["off"][0] - 1.0)
print(f"resnet12 84x84 M=128: drop off {t['off'][0] / 1e3:.3f} ms/step (min {t['off'][1] / 1e3:.3f}, max {t['off'][2] / 1e3:.3f}), "
      f"drop on {t['on'][0] / 1e3:.3f} ms/step (min {t['on'][1] / 1e3:.3f}, max {t['on'][2] / 1e3:.3f}): "
      f"{t['on'][0] - t['off'][0]:+.1f} us = {100 * (t['on'][0] / t['off'][0] - 1):+.2f} %", flush=True)

# the two launches on their own, per pooled map of one group (64 images)
res["launches"], total = [], 0.0
size = SIZE
for l, (c, bs) in enumerate(zip(CHANNELS, BLOCKS)):
    size //= 2
    m = torch.randn(1, R * (size + 2) * (size + 2), c, device=dev, generator=g).to(torch.bfloat16)
    tl = alternate({"pair": lambda: hip.rn12_drop_apply(ws, m, size, size, RATE, bs, SEED, block_index=l)}, opt.iters, 3)["pair"]
    mb = R * size * size * c * 2 / 1e6
    res["launches"].append(dict(block=l, H=size, C=c, block_size=bs, pair_us=tl, map_MB=mb))
    total += tl[0]
    print(f"block {l}: {size}x{size}x{c} x {R} images ({mb:.2f} MB), block size {bs}: count + apply {tl[0]:.1f} us "
          f"(min {tl[1]:.1f}, max {tl[2]:.1f})", flush=True)
res["launches_per_step_us"] = 4 * total                      # two groups, forward and backward
res["launches_share_of_step"] = 4 * total / t["on"][0]
print(f"a step issues each pair 4 times (two groups, forward and backward): {4 * total:.1f} us = "
      f"{100 * 4 * total / t['on'][0]:.2f} % of the drop-on step", flush=True)
torch.cuda.synchronize()
if ws.read_status() or ws_enc.read_status():
    raise SystemExit("a status bit was set")
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
