"""Prices born-again distillation of --model pretrain straight through the C ABI.  The routes of every row are
built from this commit and alternated block by block in one process (the scheme of tools/bench_pretrain_mix.py); medians over the
blocks with minimum and maximum:

  * the head alone at (M, F, C) = (128, 640, 64) and (256, 1600, 351): the distillation entry (T 4, alpha 0.5, ce_weight 0.5) against
    the soft entry on the same student, and against the same loss in torch fp32 ops with autograd (two linear layers, cross-entropy,
    kl_div, backward to feats, W and b);
  * a whole training step at 84 x 84, M = 128, R = 64, C = 64 with the bf16 ResNet-12 and with Conv4 on an already gathered batch:
    without a teacher = encode with tape, hard head, encode_bwd;  with one = the teacher's untaped encode first, then the same with the
    distillation head.

python tools/bench_distill.py [--out results.json] [--blocks 7] [--iters 4000] [--step-iters 100]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fumi_amd import hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--blocks", type=int, default=7)
ap.add_argument("--iters", type=int, default=4000)
ap.add_argument("--step-iters", type=int, default=100)
opt = ap.parse_args()

dev = torch.device("cuda:0")
ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
g = torch.Generator(device=dev).manual_seed(0)
T, ALPHA, CW = 4.0, 0.5, 0.5


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


def show(t):
    return f"{t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"


def head_case(M, F, C):
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    x, x_t = r(M, F), r(M, F)
    W, W_t = r(C, F) * (2.0 / F ** 0.5), r(C, F) * (2.0 / F ** 0.5)
    b, b_t = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    y = torch.randint(0, C, (M,), device=dev, generator=g)
    xa, Wa, ba = (t.clone().requires_grad_(True) for t in (x, W, b))

    def torch_route():
        z, z_t = TF.linear(xa, Wa, ba), TF.linear(x_t, W_t, b_t)
        loss = CW * TF.cross_entropy(z, y) + ALPHA * T * T * TF.kl_div(TF.log_softmax(z / T, 1), TF.softmax(z_t / T, 1),
                                                                       reduction="batchmean")
        return torch.autograd.grad(loss, (xa, Wa, ba)), z.argmax(1), z_t.argmax(1)
    return {"distill": lambda: hip.cls_head_step_distill(ws, x, y, W, b, x_t, W_t, b_t, temp=T, alpha=ALPHA, ce_weight=CW, need_grad=True),
            "soft": lambda: hip.cls_head_step_soft(ws, x, y, W, b, need_grad=True),
            "torch": torch_route}


def step_case(backbone, M=128, R=64, C=64, size=84):
    B, half = M // (2 * R), M // 2
    x = torch.randn(M, 3, size, size, device=dev, generator=g)
    y = torch.randint(0, C, (M,), device=dev, generator=g)
    if backbone == "conv4":
        from fumi_amd.models.conv4 import Conv4
        make, enc, bwd = (lambda: Conv4(3, 64, 4, size)), hip.conv4_encode, hip.conv4_encode_bwd
    else:
        from fumi_amd.models.resnet12 import CHANNELS, ResNet12
        make, enc, bwd = (lambda: ResNet12(3, CHANNELS, size)), hip.resnet12_encode, hip.resnet12_encode_bwd
    net = make()
    theta = [p.detach().to(dev) for p in net.theta()]
    theta_t = [p.detach().to(dev) for p in make().theta()]
    g_theta = [torch.empty_like(t) for t in theta]
    F = net.feature_dim
    W, W_t = (torch.randn(C, F, device=dev, generator=g) * (2.0 / F ** 0.5) for _ in range(2))
    b = torch.zeros(C, device=dev)
    x_s, x_q = x[:half].view(B, R, 3, size, size), x[half:].view(B, R, 3, size, size)

    def step(teacher):
        if teacher:
            t_s, t_q = enc(ws_enc, x_s, x_q, theta_t, keep_tape=False)
            feats_t = torch.cat((t_s.view(half, F), t_q.view(half, F)))
        f_s, f_q = enc(ws_enc, x_s, x_q, theta, keep_tape=True)
        feats = torch.cat((f_s.view(half, F), f_q.view(half, F)))
        if teacher:
            df = hip.cls_head_step_distill(ws, feats, y, W, b, feats_t, W_t, b, temp=T, alpha=ALPHA, ce_weight=CW, need_grad=True)["dfeats"]
        else:
            df = hip.cls_head_step(ws, feats, y, W, b, need_grad=True)["dfeats"]
        bwd(ws_enc, x_s, x_q, df[:half].view(B, R, F), df[half:].view(B, R, F), theta, g_theta=g_theta)
    return {"plain": lambda: step(False), "teacher": lambda: step(True)}


res = {"device": torch.cuda.get_device_name(0), "temp": T, "alpha": ALPHA, "ce_weight": CW, "head": [], "step": []}
for M, F, C in ((128, 640, 64), (256, 1600, 351)):
    t = alternate(head_case(M, F, C), opt.iters, opt.blocks)
    res["head"].append(dict(M=M, F=F, C=C, distill_us=t["distill"], soft_us=t["soft"], torch_us=t["torch"],
                            distill_over_soft=t["distill"][0] / t["soft"][0], distill_over_torch=t["distill"][0] / t["torch"][0]))
    print(f"head ({M},{F},{C}): distill {show(t['distill'])}, soft {show(t['soft'])}, torch fp32 autograd {show(t['torch'])}", flush=True)
for backbone in ("resnet12", "conv4"):
    t = alternate(step_case(backbone), opt.step_iters, opt.blocks)
    res["step"].append(dict(backbone=backbone, M=128, C=64, size=84, plain_us=t["plain"], teacher_us=t["teacher"],
                            added_us=t["teacher"][0] - t["plain"][0], added_share=t["teacher"][0] / t["plain"][0] - 1.0))
    print(f"{backbone} 84x84 M=128: plain {show(t['plain'])}, with a teacher {show(t['teacher'])}: "
          f"{t['teacher'][0] - t['plain'][0]:+.1f} us = {100 * (t['teacher'][0] / t['plain'][0] - 1):+.2f} %", flush=True)
torch.cuda.synchronize()
if ws.read_status() or ws_enc.read_status():
    raise SystemExit("a status bit was set")
if opt.out:
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
