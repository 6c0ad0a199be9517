"""Times the logistic-regression head (--pretrain_metric logreg / --eval_head logreg) through the binding:

  * the head alone at 5-way 5-shot and 20-way 5-shot, Qn = 15 per class, B = 32, F = 640 and 1600, T = 100: the fused
    fumi_hip_logreg_head_step, with the fit's K~ A product as the VALU loop and on the f32 MFMA (hip.logreg_set_form), against the
    same dual iteration in plain torch fp32 ops on the same tensors (bmm Gram matrix, then per
    step baddbmm, softmax and the elementwise updates) -- alternated block by block in one process after a warm-up of each, medians
    over the blocks with their minimum and maximum;
  * the per-step time of the fit launch: (the call at T = 100 minus the call at T = 1) / 99, the other three launches being the same;
  * the head's share of a --model pretrain validation meta-batch (encode without tape, then the head) with Conv4 and with the bf16
    ResNet-12 at 84 x 84, B = 4 episodes.

A timed block of the fused head lasts about --block-ms (the call count is set from a first timing of each route).

python tools/bench_logreg_head.py [--out results.json] [--blocks 7] [--block-ms 300] [--torch-iters 20] [--step-iters 10]"""
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
ap.add_argument("--block-ms", type=float, default=300.0)
ap.add_argument("--torch-iters", type=int, default=20)
ap.add_argument("--step-iters", type=int, default=10)
opt = ap.parse_args()

dev = torch.device("cuda:0")
ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
g = torch.Generator(device=dev).manual_seed(0)
T, LR, MOMENTUM, C = 100, 1.0, 0.9, 1.0


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6          # us per call


def alternate(routes, blocks):
    """{name: (median us, min us, max us)} of routes = {name: (fn, iters)}, timed block by block in turn after a warm-up of each."""
    routes = dict(routes)
    for k, (fn, iters) in routes.items():
        timed(fn, 3)
        if iters is None:                                      # calls that fill --block-ms
            routes[k] = (fn, max(10, int(opt.block_ms * 1e3 / timed(fn, 10))))
    ts = {k: [] for k in routes}
    for _ in range(blocks):
        for k, (fn, iters) in routes.items():
            ts[k].append(timed(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def labels(B, N, K, Qn):
    return (torch.arange(N * K, device=dev) % N).repeat(B, 1), torch.randint(0, N, (B, Qn), device=dev, generator=g)


def torch_logreg(xs, ys, xq, yq, N, steps):
    xs = xs / xs.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    xq = xq / xq.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    B, S, _ = xs.shape
    K = torch.bmm(xs, xs.transpose(1, 2))
    Y = torch.nn.functional.one_hot(ys, N).float()
    wd = 1.0 / (C * S)
    A = torch.zeros(B, S, N, device=dev); VA = torch.zeros_like(A)
    b = torch.zeros(B, 1, N, device=dev); Vb = torch.zeros_like(b)
    for _ in range(steps):
        R = (torch.softmax(torch.baddbmm(b, K, A), dim=-1) - Y) / S
        VA = MOMENTUM * VA + R + wd * A
        Vb = MOMENTUM * Vb + R.sum(dim=1, keepdim=True)
        A = A - LR * VA
        b = b - LR * Vb
    z = torch.bmm(xq, torch.bmm(xs.transpose(1, 2), A)) + b
    return torch.nn.functional.cross_entropy(z.reshape(-1, N), yq.reshape(-1)), (z.argmax(-1) == yq).sum()


def head_case(B, N, K, Qn, Fd):
    y_s, y_q = labels(B, N, K, Qn)
    f_s = torch.relu(torch.randn(B, N * K, Fd, device=dev, generator=g))          # post-ReLU-like features
    f_q = torch.relu(torch.randn(B, Qn, Fd, device=dev, generator=g))
    def fused(steps, form=None):
        def call():
            hip.logreg_set_form(form)
            return hip.logreg_head_step(ws, f_s, y_s, f_q, y_q, steps=steps, lr=LR, momentum=MOMENTUM, C=C, n_way=N)
        return call
    return fused, (lambda: torch_logreg(f_s, y_s, f_q, y_q, N, T))


def step_case(backbone, B, N, K, Qn, size=84):
    torch.manual_seed(1)
    if backbone == "conv4":
        from fumi_amd.models.conv4 import Conv4
        net, encode = Conv4(3, 64, 4, size), hip.conv4_encode
    else:
        from fumi_amd.models.resnet12 import CHANNELS, ResNet12
        net, encode = ResNet12(3, CHANNELS, size), hip.resnet12_encode
    theta = [p.detach().to(dev) for p in net.theta()]
    y_s, y_q = labels(B, N, K, Qn)
    x_s = torch.randn(B, N * K, 3, size, size, device=dev, generator=g)
    x_q = torch.randn(B, Qn, 3, size, size, device=dev, generator=g)

    def step():
        f_s, f_q = encode(ws_enc, x_s, x_q, theta, keep_tape=False)
        return hip.logreg_head_step(ws, f_s, y_s, f_q, y_q, steps=T, lr=LR, momentum=MOMENTUM, C=C, n_way=N)
    return step, net.feature_dim


res = {"device": torch.cuda.get_device_name(0), "steps": T, "lr": LR, "momentum": MOMENTUM, "C": C, "head": [], "step": []}
for Fd in (640, 1600):
    for B, N, K, Qn in ((32, 5, 5, 75), (32, 20, 5, 300)):
        fused, plain = head_case(B, N, K, Qn, Fd)
        t = alternate({"valu": (fused(T, "valu"), None), "mfma": (fused(T, "mfma"), None), "valu_T1": (fused(1, "valu"), None),
                       "mfma_T1": (fused(1, "mfma"), None), "default": (fused(T), None), "torch": (plain, opt.torch_iters)}, opt.blocks)
        step = {f: (t[f][0] - t[f + "_T1"][0]) / (T - 1) for f in ("valu", "mfma")}
        res["head"].append(dict(B=B, N=N, K=K, Qn=Qn, F=Fd, us=t, fit_us_per_step=step, torch_over_default=t["torch"][0] / t["default"][0]))
        f3 = lambda v: f"{v[0]:.1f} us (min {v[1]:.1f}, max {v[2]:.1f})"
        print(f"head B={B} N={N} K={K} Qn={Qn} F={Fd} T={T}: VALU form {f3(t['valu'])}, fit {step['valu']:.3f} us/step; MFMA form "
              f"{f3(t['mfma'])}, fit {step['mfma']:.3f} us/step; the default choice {f3(t['default'])}; torch ops {f3(t['torch'])} = "
              f"{t['torch'][0] / t['default'][0]:.1f} x the default", flush=True)
hip.logreg_set_form(None)
for backbone in ("conv4", "resnet12"):
    for B, N, K, Qn in ((4, 5, 5, 75), (4, 20, 5, 300)):
        step, Fd = step_case(backbone, B, N, K, Qn)
        t = alternate({"step": (step, opt.step_iters)}, opt.blocks)["step"]
        h = alternate({"fused": (head_case(B, N, K, Qn, Fd)[0](T), None)}, 3)["fused"][0]
        res["step"].append(dict(backbone=backbone, size=84, B=B, N=N, K=K, Qn=Qn, F=Fd, step_us=t, head_alone_us=h, head_share=h / t[0]))
        print(f"{backbone} 84x84 validation meta-batch B={B} N={N} K={K} Qn={Qn}: {t[0] / 1e3:.2f} ms (min {t[1] / 1e3:.2f}, max "
              f"{t[2] / 1e3:.2f}); the head alone {h:.1f} us = {100 * h / t[0]:.2f} % of it", flush=True)
torch.cuda.synchronize()
if ws.read_status() or ws_enc.read_status():
    raise SystemExit("a status bit was set")
if opt.out:
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
