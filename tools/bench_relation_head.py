"""Times the Relation Network head (--fewshot_head relation) straight through the C ABI, at B = 32 episodes of
5-way 1-shot, 5-way 5-shot and 20-way 5-shot with 15 queries per class, F = 640 and H = 256, with the paper's mse loss: the fused
fumi_hip_relation_head_step, training and forward form, against

  * the same head in plain torch fp32 ops on the same tensors (class means by a one-hot bmm, two F.linear, a broadcast add, relu, a
    product with w2, sigmoid and nn.MSELoss, arg-max; autograd backward for both feature sets and the four tensors in the training
    form) -- that torch expression is the baseline.  It materialises the [B,Qn,N,H] hidden tensor, which the fused head never forms;
  * fumi_hip_cos_proto_step, the cosine nearest-centroid head, at the same shape.

The routes of a shape alternate block by block in one process; medians over the blocks with min and max.  With --small also B = 4, the
meta-batch of the 84 x 84 training steps the project reports, for the head's share of such a step.

python tools/bench_relation_head.py [--out results.json] [--blocks 7] [--iters 300] [--small] [--loss mse|ce] [--profile-only]
(--profile-only: a few calls of every route and nothing else, for a kernel trace)"""
import argparse
import json
import math
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
ap.add_argument("--iters", type=int, default=300)
ap.add_argument("--small", action="store_true")
ap.add_argument("--loss", choices=["mse", "ce"], default="mse")
ap.add_argument("--profile-only", action="store_true")
opt = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("bench_relation_head.py measures on the GPU: none is visible")
dev = torch.device("cuda:0")
ws = hip.Workspace.get(dev)
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


def head_case(B, N, K, Qn, Fd, H):
    """{route: closure} of both forms -- fused, torch and the cosine head -- on post-ReLU-like features with a class structure, and the
    largest logit difference between the fused head and the torch expression."""
    y_s = (torch.arange(N * K, device=dev) % N).repeat(B, 1)
    y_q = torch.randint(0, N, (B, Qn), device=dev, generator=g)
    mu = torch.randn(B, N, Fd, device=dev, generator=g)
    bi = torch.arange(B, device=dev)[:, None]
    f_s = torch.relu(mu[bi, y_s] + torch.randn(B, N * K, Fd, device=dev, generator=g)).contiguous()
    f_q = torch.relu(mu[bi, y_q] + torch.randn(B, Qn, Fd, device=dev, generator=g)).contiguous()
    k1, k2 = 1.0 / math.sqrt(2.0 * Fd), 1.0 / math.sqrt(float(H))
    u = lambda shape, k: (torch.rand(*shape, device=dev, generator=g) * 2.0 - 1.0) * k
    w = [u((2, H, Fd), k1), u((H,), k1), u((H,), k2), u((1,), k2)]
    tau = torch.tensor([10.0], device=dev)
    xs, xq = f_s.clone().requires_grad_(True), f_q.clone().requires_grad_(True)
    wt = [t.clone().requires_grad_(True) for t in w]
    onehot_t = F.one_hot(y_s, N).to(torch.float32).transpose(1, 2).contiguous()
    inv_cnt = 1.0 / onehot_t.sum(-1).clamp(min=1.0)[:, :, None]
    target = F.one_hot(y_q, N).to(torch.float32)

    def fused_train():                         # predictions computed, every output allocated by the call
        return hip.relation_head_step(ws, f_s, y_s, f_q, y_q, w, loss=opt.loss, need_grad=True, grad_scale=1.0, n_way=N)

    def fused_fwd():
        return hip.relation_head_step(ws, f_s, y_s, f_q, y_q, w, loss=opt.loss, need_grad=False, n_way=N)

    def cos_train():
        return hip.cos_proto_step(ws, f_s, y_s, f_q, y_q, tau, need_grad=True, grad_scale=1.0, n_way=N)

    def cos_fwd():
        return hip.cos_proto_step(ws, f_s, y_s, f_q, y_q, tau, need_grad=False, n_way=N)

    def logits_of(s, q, p):
        c = torch.bmm(onehot_t, s) * inv_cnt
        pre = F.linear(c, p[0][0], p[1])[:, None, :, :] + F.linear(q, p[0][1])[:, :, None, :]
        return torch.relu(pre) @ p[2] + p[3]

    def loss_of(z):
        if opt.loss == "mse":
            return F.mse_loss(torch.sigmoid(z), target)
        return F.cross_entropy(z.reshape(-1, N), y_q.reshape(-1))

    def torch_train():
        z = logits_of(xs, xq, wt)
        loss = loss_of(z)
        return loss, (z.argmax(-1) == y_q).sum(), torch.autograd.grad(loss, [xs, xq] + wt)

    def torch_fwd():
        with torch.no_grad():
            z = logits_of(f_s, f_q, w)
            return loss_of(z), (z.argmax(-1) == y_q).sum()
    with torch.no_grad():
        z_f = hip.relation_head_step(ws, f_s, y_s, f_q, y_q, w, loss=opt.loss, need_grad=False, want_logits=True, n_way=N)["logits"]
        dz = float((z_f - logits_of(f_s, f_q, w)).abs().max() / z_f.abs().max())
    return {"fused_train": fused_train, "torch_train": torch_train, "cos_train": cos_train,
            "fused_fwd": fused_fwd, "torch_fwd": torch_fwd, "cos_fwd": cos_fwd}, dz


res = {"device": torch.cuda.get_device_name(0), "loss": opt.loss, "head": []}
fmt = lambda t: f"{t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"
Fd, H = 640, 256
for B in (32, 4) if opt.small else (32,):
    for N, K in [(5, 1), (5, 5), (20, 5)]:
        Qn = 15 * N
        routes, dz = head_case(B, N, K, Qn, Fd, H)
        if opt.profile_only:
            for _ in range(5):
                for fn in routes.values():
                    fn()
            continue
        t = alternate(routes, opt.iters, opt.blocks)
        res["head"].append(dict(B=B, N=N, K=K, Qn=Qn, F=Fd, H=H, logits_fused_vs_torch_rel_to_max=dz, **{k + "_us": v for k, v in t.items()}))
        print(f"head B={B} N={N} K={K} Qn={Qn} F={Fd} H={H} {opt.loss}: training form fused {fmt(t['fused_train'])}, torch ops "
              f"{fmt(t['torch_train'])} ({t['torch_train'][0] / t['fused_train'][0]:.2f} x), cosine head {fmt(t['cos_train'])} "
              f"({t['fused_train'][0] / t['cos_train'][0]:.2f} x of it); forward form fused {fmt(t['fused_fwd'])}, torch ops "
              f"{fmt(t['torch_fwd'])} ({t['torch_fwd'][0] / t['fused_fwd'][0]:.2f} x), cosine head {fmt(t['cos_fwd'])} "
              f"({t['fused_fwd'][0] / t['cos_fwd'][0]:.2f} x of it); logits fused vs torch {dz:.2e} of max", flush=True)
torch.cuda.synchronize()
if ws.read_status():
    raise SystemExit("a status bit was set")
if opt.out and not opt.profile_only:
    with open(opt.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print("wrote", opt.out)
