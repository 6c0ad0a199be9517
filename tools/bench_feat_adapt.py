"""Times the set-to-set prototype adaptation (--fewshot_adapt feat):

  * the adaptation alone at B = 32, 5-way and 20-way 5-shot, F = 640 and 1600: the forward form (feat_adapt_fwd without a tape), the
    forward + backward pair (tape kept, feat_adapt_bwd for a fixed dprotos), and the same computation in plain torch fp32 ops with
    autograd on the same tensors (one-hot bmm prototypes, three F.linear, bmm, softmax, bmm, F.linear, F.layer_norm) -- that torch
    expression is the yardstick.  The routes alternate block by block in one process; medians over the blocks with min and max;
  * MetaBaseline.train_step itself on 84 x 84 images with the bf16 ResNet-12 and the prototypical head, with adapt="feat" and with
    adapt="none" in turn (B = 4 episodes, 15 queries per class, no optimizer), and the pair alone as a share of the former.

python tools/bench_feat_adapt.py [--out results.json] [--blocks 5] [--iters 200] [--step-iters 5]"""
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
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--step-iters", type=int, default=5)
opt = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("bench_feat_adapt.py measures on the GPU: none is visible")
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
        timed(fn, 5)
    ts = {k: [] for k in routes}
    for _ in range(blocks):
        for k, fn in routes.items():
            ts[k].append(timed(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def weights(Fd):
    std = (2.0 / (Fd + Fd)) ** 0.5
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    return [r(3 * Fd, Fd) * std, r(Fd, Fd) * std, 0.1 * r(Fd), 1.0 + 0.3 * r(Fd), 0.2 * r(Fd)]


def adapt_case(B, N, K, Fd):
    """{route: closure} of the forward form and the pair, fused and torch, on post-ReLU-like features; the largest difference of the
    adapted prototypes between the two."""
    y_s = (torch.arange(N * K, device=dev) % N).repeat(B, 1)
    f_s = torch.relu(torch.randn(B, N * K, Fd, device=dev, generator=g))
    w = weights(Fd)
    dpr = torch.randn(B, N, Fd, device=dev, generator=g)
    xs = f_s.clone().requires_grad_(True)
    wt = [t.clone().requires_grad_(True) for t in w]

    def fused_fwd():
        return hip.feat_adapt_fwd(ws, f_s, y_s, w, n_way=N, keep_tape=False)

    def fused_pair():
        _, tape = hip.feat_adapt_fwd(ws, f_s, y_s, w, n_way=N, keep_tape=True)
        return hip.feat_adapt_bwd(ws, f_s, y_s, w, tape, dpr, n_way=N)

    def protos_of(s, wqkv, wo, bo, gamma, beta):
        onehot = F.one_hot(y_s, N).to(torch.float32)
        P = torch.bmm(onehot.transpose(1, 2), s) / onehot.sum(1).clamp(min=1)[:, :, None]
        q, k, v = F.linear(P, wqkv).split(Fd, dim=-1)
        A = torch.softmax(torch.bmm(q, k.transpose(1, 2)) / Fd ** 0.5, dim=-1)
        return F.layer_norm(P + F.linear(torch.bmm(A, v), wo, bo), (Fd,), gamma, beta, 1e-5)

    def torch_fwd():
        with torch.no_grad():
            return protos_of(f_s, *w)

    def torch_pair():
        return torch.autograd.grad(protos_of(xs, *wt), [xs] + wt, dpr)
    with torch.no_grad():
        p_f = fused_fwd()[0]
        dp = float((p_f - torch_fwd()).abs().max() / p_f.abs().max())
    return {"fused_fwd": fused_fwd, "torch_fwd": torch_fwd, "fused_pair": fused_pair, "torch_pair": torch_pair}, dp


def step_case(B, N, K, Qn, adapt, size=84):
    """MetaBaseline.train_step itself (bf16 ResNet-12, prototypical head, no optimizer) on one fixed meta-batch."""
    from fumi_amd.models.metabaseline import MetaBaseline
    torch.manual_seed(0)
    model = MetaBaseline("resnet12", image_size=size, image_channels=3, num_ways=N, head="proto", proto_scale=1.0 / 640, adapt=adapt).to(dev)
    y_s = (torch.arange(N * K, device=dev) % N).repeat(B, 1)
    y_q = torch.randint(0, N, (B, Qn), device=dev, generator=g)
    x_s = torch.randn(B, N * K, 3, size, size, device=dev, generator=g)
    x_q = torch.randn(B, Qn, 3, size, size, device=dev, generator=g)
    batch = {"train": ((None, None, x_s), y_s), "test": ((None, None, x_q), y_q)}
    return (lambda: model.train_step(batch, dev)), model.conv.feature_dim


res = {"device": torch.cuda.get_device_name(0), "adapt": [], "step": []}
fmt = lambda t: f"{t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"
for Fd in (640, 1600):
    for B, N, K in [(32, 5, 5), (32, 20, 5)]:
        routes, dp = adapt_case(B, N, K, Fd)
        t = alternate(routes, opt.iters, opt.blocks)
        res["adapt"].append(dict(B=B, N=N, K=K, F=Fd, protos_fused_vs_torch_rel_to_max=dp, **{k + "_us": v for k, v in t.items()}))
        print(f"adapt B={B} N={N} K={K} F={Fd}: forward form fused {fmt(t['fused_fwd'])}, torch ops {fmt(t['torch_fwd'])}; forward + "
              f"backward fused {fmt(t['fused_pair'])}, torch ops {fmt(t['torch_pair'])}; protos fused vs torch {dp:.2e} of max", flush=True)
for B, N, K, Qn in [(4, 5, 5, 75), (4, 20, 5, 300)]:
    (feat, Fd), (none, _) = step_case(B, N, K, Qn, "feat"), step_case(B, N, K, Qn, "none")
    t = alternate({"feat": feat, "none": none}, opt.step_iters, opt.blocks)
    h = alternate({"pair": adapt_case(B, N, K, Fd)[0]["fused_pair"]}, opt.iters, 3)["pair"][0]
    tf, tn = t["feat"], t["none"]
    res["step"].append(dict(backbone="resnet12", size=84, B=B, N=N, K=K, Qn=Qn, F=Fd, step_feat_us=tf, step_none_us=tn,
                            adapt_pair_alone_us=h, adapt_share=h / tf[0], step_increase=(tf[0] - tn[0]) / tn[0]))
    print(f"resnet12 84x84 B={B} N={N} K={K} Qn={Qn} F={Fd}: MetaBaseline.train_step with adapt=feat {tf[0] / 1e3:.2f} ms (min "
          f"{tf[1] / 1e3:.2f}, max {tf[2] / 1e3:.2f}), with adapt=none {tn[0] / 1e3:.2f} ms (min {tn[1] / 1e3:.2f}, max {tn[2] / 1e3:.2f}): "
          f"{100 * (tf[0] - tn[0]) / tn[0]:+.2f} %; the adaptation's forward + backward alone {h:.1f} us = {100 * h / tf[0]:.3f} % of the "
          f"step", flush=True)
torch.cuda.synchronize()
if ws.read_status() or ws_enc.read_status():
    raise SystemExit("a status bit was set")
if opt.out:
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
