"""Times the transductive prototype refinement (--transductive_steps) straight through the C ABI:

  * the head alone at (B, N, K, Qn, F) = (32, 5, 5, 75, F) and (32, 20, 5, 300, F), F = 640 and 1600 (5-way and 20-way 5-shot, 15 queries
    per class), steps = 1 and 10, both metrics: the fused fumi_hip_trans_proto_step against the same iteration in plain torch fp32 ops
    on the same tensors (one-hot bmm prototypes, bmm logits, softmax, F.cross_entropy, arg-max) -- that torch expression is the
    baseline.  The routes alternate block by block in one process; medians over the blocks with min and max; the time per step is
    the slope between steps = 1 and steps = 10;
  * a validation meta-batch (encode without tape, head) with Conv4 and with the bf16 ResNet-12 at 84 x 84, B = 4 episodes of the two
    shapes at steps = 10, and the head's share of it (the head alone at that shape over the whole).

python tools/bench_trans_proto.py [--out results.json] [--blocks 7] [--iters 50] [--step-iters 10] [--profile-only]
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
ap.add_argument("--iters", type=int, default=50)            # a block of the head alone: 0.01 - 0.3 s
ap.add_argument("--step-iters", type=int, default=10)      # a block of whole validation meta-batches
ap.add_argument("--profile-only", action="store_true")
opt = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("bench_trans_proto.py measures on the GPU: none is visible")
dev = torch.device("cuda:0")
ws, ws_enc = hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")
g = torch.Generator(device=dev).manual_seed(0)
SCALE = {"cosine": 10.0, "euclid": None}                   # euclid: 1 / F, the scale at which post-ReLU-like features give logits of order 1


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
        timed(fn, 5)
    ts = {k: [] for k in routes}
    for _ in range(blocks):
        for k, fn in routes.items():
            ts[k].append(timed(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def labels(B, N, K, Qn):
    y_s = (torch.arange(N * K, device=dev) % N).repeat(B, 1)
    y_q = torch.randint(0, N, (B, Qn), device=dev, generator=g)
    return y_s, y_q


def head_case(B, N, K, Qn, Fd, metric):
    """{route: closure} for steps = 1 and 10, fused and torch, on post-ReLU-like features with a class signal, and the largest logit
    difference between the two routes at steps = 10."""
    y_s, y_q = labels(B, N, K, Qn)
    mu = torch.randn(B, N, Fd, device=dev, generator=g)
    bi = torch.arange(B, device=dev)[:, None]
    f_s = torch.relu(mu[bi, y_s] + 2.0 * torch.randn(B, N * K, Fd, device=dev, generator=g))
    f_q = torch.relu(mu[bi, y_q] + 2.0 * torch.randn(B, Qn, Fd, device=dev, generator=g))
    scale = torch.tensor([SCALE[metric] or 1.0 / Fd], device=dev)

    def fused(steps, want_logits=False):
        return lambda: hip.trans_proto_step(ws, f_s, y_s, f_q, y_q, scale, metric=metric, steps=steps, want_logits=want_logits, n_way=N)

    def logits_of(protos):
        if metric == "cosine":
            return scale * torch.bmm(F.normalize(f_q, dim=-1), F.normalize(protos, dim=-1).transpose(1, 2))
        d2 = (f_q * f_q).sum(-1, keepdim=True) - 2.0 * torch.bmm(f_q, protos.transpose(1, 2)) + (protos * protos).sum(-1)[:, None, :]
        return -scale * d2

    def torch_route(steps):
        def run():
            with torch.no_grad():
                onehot = F.one_hot(y_s, N).to(torch.float32)
                sums, count = torch.bmm(onehot.transpose(1, 2), f_s), onehot.sum(1)
                z = logits_of(sums / count.clamp(min=1)[:, :, None])
                for _ in range(steps):
                    w = torch.softmax(z, dim=-1)
                    z = logits_of((sums + torch.bmm(w.transpose(1, 2), f_q)) / (count + w.sum(1))[:, :, None])
                return F.cross_entropy(z.reshape(-1, N), y_q.reshape(-1)), (z.argmax(-1) == y_q).sum(), z
        return run
    z_f = fused(10, True)()["logits"]
    z_t = torch_route(10)()[2]
    dz = float((z_f - z_t).abs().max() / z_f.abs().max())
    return {"fused_1": fused(1), "torch_1": torch_route(1), "fused_10": fused(10), "torch_10": torch_route(10)}, dz


def val_case(backbone, B, N, K, Qn, metric, size=84):
    if backbone == "conv4":
        from fumi_amd.models.conv4 import Conv4
        net = Conv4(3, 64, 4, size)
        encode = hip.conv4_encode
    else:
        from fumi_amd.models.resnet12 import CHANNELS, ResNet12
        net = ResNet12(3, CHANNELS, size)
        encode = hip.resnet12_encode
    theta = [p.detach().to(dev) for p in net.theta()]
    y_s, y_q = labels(B, N, K, Qn)
    x_s = torch.randn(B, N * K, 3, size, size, device=dev, generator=g)
    x_q = torch.randn(B, Qn, 3, size, size, device=dev, generator=g)
    scale = torch.tensor([SCALE[metric] or 1.0 / net.feature_dim], device=dev)

    def batch():
        f_s, f_q = encode(ws_enc, x_s, x_q, theta, keep_tape=False)
        return hip.trans_proto_step(ws, f_s, y_s, f_q, y_q, scale, metric=metric, steps=10, n_way=N)
    return batch, net.feature_dim


res = {"device": torch.cuda.get_device_name(0), "head": [], "val": []}
fmt = lambda t: f"{t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"
for metric in ("cosine", "euclid"):
    for Fd in (640, 1600):
        for B, N, K, Qn in [(32, 5, 5, 75), (32, 20, 5, 300)]:
            routes, dz = head_case(B, N, K, Qn, Fd, metric)
            if opt.profile_only:
                for _ in range(3):
                    for fn in routes.values():
                        fn()
                continue
            t = alternate(routes, opt.iters, opt.blocks)
            slope = {r: (t[r + "_10"][0] - t[r + "_1"][0]) / 9.0 for r in ("fused", "torch")}
            res["head"].append(dict(metric=metric, B=B, N=N, K=K, Qn=Qn, F=Fd, logits_fused_vs_torch_rel_to_max=dz,
                                    fused_us_per_step=slope["fused"], torch_us_per_step=slope["torch"],
                                    **{k + "_us": v for k, v in t.items()}))
            print(f"head {metric} B={B} N={N} K={K} Qn={Qn} F={Fd}: steps=1 fused {fmt(t['fused_1'])}, torch ops {fmt(t['torch_1'])}; "
                  f"steps=10 fused {fmt(t['fused_10'])}, torch ops {fmt(t['torch_10'])}; per step fused {slope['fused']:.1f} us, torch ops "
                  f"{slope['torch']:.1f} us; logits fused vs torch at steps=10 {dz:.2e} of max", flush=True)
for backbone in ("conv4", "resnet12"):
    for B, N, K, Qn in [(4, 5, 5, 75), (4, 20, 5, 300)]:
        batch, Fd = val_case(backbone, B, N, K, Qn, "cosine")
        if opt.profile_only:
            for _ in range(2):
                batch()
            continue
        t = alternate({"val": batch}, opt.step_iters, opt.blocks)["val"]
        h = alternate({"fused": head_case(B, N, K, Qn, Fd, "cosine")[0]["fused_10"]}, opt.iters, 3)["fused"][0]
        res["val"].append(dict(backbone=backbone, size=84, B=B, N=N, K=K, Qn=Qn, F=Fd, steps=10, metric="cosine", val_us=t,
                               head_alone_us=h, head_share=h / t[0]))
        print(f"{backbone} 84x84 B={B} N={N} K={K} Qn={Qn} F={Fd}: validation meta-batch {t[0] / 1e3:.2f} ms (min {t[1] / 1e3:.2f}, max "
              f"{t[2] / 1e3:.2f}); the head alone (cosine, 10 steps) {h:.1f} us = {100 * h / t[0]:.2f} % of it", flush=True)
torch.cuda.synchronize()
if ws.read_status() or ws_enc.read_status():
    raise SystemExit("a status bit was set")
if opt.out and not opt.profile_only:
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
