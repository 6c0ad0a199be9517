"""Times the prototypical-network head (--fewshot_head proto) straight through the C ABI:

  * the head alone at (B, N, K, Qn, F) = (32, 5, 5, 75, F) and (32, 20, 5, 300, F), F = 640 and 1600 (5-way and 20-way 5-shot, 15 queries
    per class): the fused fumi_hip_euclid_proto_step, training and forward form, against the same head in plain torch fp32 ops on the
    same tensors (one-hot bmm prototypes, |f|^2 - 2 f.c + |c|^2 by bmm, F.cross_entropy, arg-max; autograd backward for both feature
    sets and the scale in the training form) -- that torch expression is the baseline.  The routes alternate block by block in one
    process; medians over the blocks with min and max;
  * a whole training step (encode with tape, head, encode_bwd) with Conv4 and with the bf16 ResNet-12 at 84 x 84, B = 4 episodes of
    the two shapes, and the head's share of that step (the head alone at the step's shape over the step).

python tools/bench_euclid_proto.py [--out results.json] [--blocks 7] [--iters 500] [--step-iters 10] [--profile-only]
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
ap.add_argument("--iters", type=int, default=500)           # a block of the head alone: 0.03 - 0.5 s
ap.add_argument("--step-iters", type=int, default=10)      # a block of whole steps
ap.add_argument("--profile-only", action="store_true")
opt = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("bench_euclid_proto.py measures on the GPU: none is visible")
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
    """{route: closure} of both forms, fused and torch, on post-ReLU-like features, and the largest logit difference between them."""
    y_s, y_q = labels(B, N, K, Qn)
    f_s = torch.relu(torch.randn(B, N * K, Fd, device=dev, generator=g))
    f_q = torch.relu(torch.randn(B, Qn, Fd, device=dev, generator=g))
    alpha = torch.tensor([1.0 / Fd], device=dev)
    xs, xq, a = f_s.clone().requires_grad_(True), f_q.clone().requires_grad_(True), alpha.clone().requires_grad_(True)

    def fused_train():                         # predictions computed, every output allocated by the call
        return hip.euclid_proto_step(ws, f_s, y_s, f_q, y_q, alpha, need_grad=True, grad_scale=1.0, n_way=N)

    def fused_fwd():
        return hip.euclid_proto_step(ws, f_s, y_s, f_q, y_q, alpha, need_grad=False, n_way=N)

    def logits_of(s, q, sc):
        onehot = F.one_hot(y_s, N).to(torch.float32)
        protos = torch.bmm(onehot.transpose(1, 2), s) / onehot.sum(1).clamp(min=1)[:, :, None]
        d2 = (q * q).sum(-1, keepdim=True) - 2.0 * torch.bmm(q, protos.transpose(1, 2)) + (protos * protos).sum(-1)[:, None, :]
        return -sc * d2

    def torch_train():
        z = logits_of(xs, xq, a)
        loss = F.cross_entropy(z.reshape(-1, N), y_q.reshape(-1))
        return loss, (z.argmax(-1) == y_q).sum(), torch.autograd.grad(loss, [xs, xq, a])

    def torch_fwd():
        with torch.no_grad():
            z = logits_of(f_s, f_q, alpha)
            return F.cross_entropy(z.reshape(-1, N), y_q.reshape(-1)), (z.argmax(-1) == y_q).sum()
    with torch.no_grad():
        z_f = hip.euclid_proto_step(ws, f_s, y_s, f_q, y_q, alpha, need_grad=False, want_logits=True, n_way=N)["logits"]
        dz = float((z_f - logits_of(f_s, f_q, alpha)).abs().max() / z_f.abs().max())
    return {"fused_train": fused_train, "torch_train": torch_train, "fused_fwd": fused_fwd, "torch_fwd": torch_fwd}, dz


def step_case(backbone, B, N, K, Qn, size=84):
    if backbone == "conv4":
        from fumi_amd.models.conv4 import Conv4
        net = Conv4(3, 64, 4, size)
        encode, encode_bwd = hip.conv4_encode, hip.conv4_encode_bwd
    else:
        from fumi_amd.models.resnet12 import CHANNELS, ResNet12
        net = ResNet12(3, CHANNELS, size)
        encode, encode_bwd = hip.resnet12_encode, hip.resnet12_encode_bwd
    theta = [p.detach().to(dev) for p in net.theta()]
    g_theta = [torch.empty_like(t) for t in theta]
    y_s, y_q = labels(B, N, K, Qn)
    x_s = torch.randn(B, N * K, 3, size, size, device=dev, generator=g)
    x_q = torch.randn(B, Qn, 3, size, size, device=dev, generator=g)
    alpha = torch.tensor([1.0 / net.feature_dim], device=dev)

    def step():
        f_s, f_q = encode(ws_enc, x_s, x_q, theta, keep_tape=True)
        out = hip.euclid_proto_step(ws, f_s, y_s, f_q, y_q, alpha, need_grad=True, grad_scale=1.0, n_way=N)
        encode_bwd(ws_enc, x_s, x_q, out["dfeats_s"], out["dfeats_q"], theta, g_theta=g_theta)
    return step, net.feature_dim


res = {"device": torch.cuda.get_device_name(0), "head": [], "step": []}
fmt = lambda t: f"{t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"
for Fd in (640, 1600):
    for B, N, K, Qn in [(32, 5, 5, 75), (32, 20, 5, 300)]:
        routes, dz = head_case(B, N, K, Qn, Fd)
        if opt.profile_only:
            for _ in range(5):
                for fn in routes.values():
                    fn()
            continue
        t = alternate(routes, opt.iters, opt.blocks)
        res["head"].append(dict(B=B, N=N, K=K, Qn=Qn, F=Fd, logits_fused_vs_torch_rel_to_max=dz, **{k + "_us": v for k, v in t.items()}))
        print(f"head B={B} N={N} K={K} Qn={Qn} F={Fd}: training form fused {fmt(t['fused_train'])}, torch ops {fmt(t['torch_train'])}; "
              f"forward form fused {fmt(t['fused_fwd'])}, torch ops {fmt(t['torch_fwd'])}; logits fused vs torch {dz:.2e} of max", flush=True)
for backbone in ("conv4", "resnet12"):
    for B, N, K, Qn in [(4, 5, 5, 75), (4, 20, 5, 300)]:
        step, Fd = step_case(backbone, B, N, K, Qn)
        if opt.profile_only:
            for _ in range(2):
                step()
            continue
        t = alternate({"step": step}, opt.step_iters, opt.blocks)["step"]
        h = alternate({"fused": head_case(B, N, K, Qn, Fd)[0]["fused_train"]}, opt.iters, 3)["fused"][0]
        res["step"].append(dict(backbone=backbone, size=84, B=B, N=N, K=K, Qn=Qn, F=Fd, step_us=t, episodes_per_s=B / t[0] * 1e6,
                                head_alone_us=h, head_share=h / t[0]))
        print(f"{backbone} 84x84 B={B} N={N} K={K} Qn={Qn} F={Fd}: {t[0] / 1e3:.2f} ms/step (min {t[1] / 1e3:.2f}, max {t[2] / 1e3:.2f}) = "
              f"{B / t[0] * 1e6:.1f} episodes/s; the head alone {h:.1f} us = {100 * h / t[0]:.3f} % of the step", flush=True)
torch.cuda.synchronize()
if ws.read_status() or ws_enc.read_status():
    raise SystemExit("a status bit was set")
if opt.out and not opt.profile_only:
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
