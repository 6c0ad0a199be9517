"""Times the Matching Networks head (--fewshot_head matching) straight through the C ABI, at B = 32 episodes of
5-way 1-shot, 5-way 5-shot and 20-way 5-shot with 15 queries per class and F = 640: the fused fumi_hip_match_head_step, training and
forward form, against

  * the same head in plain torch fp32 ops on the same tensors (F.normalize, bmm scores, the class masses as exp(a - row max) times a
    one-hot matrix by bmm, log, F.cross_entropy, arg-max; autograd backward for both feature sets and the temperature in the training
    form) -- that torch expression is the baseline.  It is the formulation with one maximum per row, the one a torch user writes; the
    fused head takes one maximum per class;
  * fumi_hip_cos_proto_step, the cosine nearest-centroid head, at the same shape.

The routes of a shape alternate block by block in one process; medians over the blocks with min and max.  With --small also B = 4, the
meta-batch of the 84 x 84 training steps the project reports, for the head's share of such a step.

python tools/bench_matching_head.py [--out results.json] [--blocks 7] [--iters 500] [--small] [--profile-only]
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
ap.add_argument("--iters", type=int, default=500)           # a block of the head alone: 0.02 - 0.3 s
ap.add_argument("--small", action="store_true")
ap.add_argument("--profile-only", action="store_true")
opt = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("bench_matching_head.py measures on the GPU: none is visible")
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


def head_case(B, N, K, Qn, Fd):
    """{route: closure} of both forms -- fused, torch and the cosine head -- on post-ReLU-like features with a class structure, and the
    largest logit difference between the fused head and the torch expression."""
    y_s = (torch.arange(N * K, device=dev) % N).repeat(B, 1)
    y_q = torch.randint(0, N, (B, Qn), device=dev, generator=g)
    mu = torch.randn(B, N, Fd, device=dev, generator=g)
    bi = torch.arange(B, device=dev)[:, None]
    f_s = torch.relu(mu[bi, y_s] + torch.randn(B, N * K, Fd, device=dev, generator=g)).contiguous()
    f_q = torch.relu(mu[bi, y_q] + torch.randn(B, Qn, Fd, device=dev, generator=g)).contiguous()
    tau = torch.tensor([10.0], device=dev)
    xs, xq, t = f_s.clone().requires_grad_(True), f_q.clone().requires_grad_(True), tau.clone().requires_grad_(True)
    onehot = F.one_hot(y_s, N).to(torch.float32)

    def fused_train():                         # predictions computed, every output allocated by the call
        return hip.match_head_step(ws, f_s, y_s, f_q, y_q, tau, need_grad=True, grad_scale=1.0, n_way=N)

    def fused_fwd():
        return hip.match_head_step(ws, f_s, y_s, f_q, y_q, tau, need_grad=False, n_way=N)

    def cos_train():
        return hip.cos_proto_step(ws, f_s, y_s, f_q, y_q, tau, need_grad=True, grad_scale=1.0, n_way=N)

    def cos_fwd():
        return hip.cos_proto_step(ws, f_s, y_s, f_q, y_q, tau, need_grad=False, n_way=N)

    def logits_of(s, q, sc):
        a = sc * torch.bmm(F.normalize(q, dim=-1), F.normalize(s, dim=-1).transpose(1, 2))
        m = a.max(-1, keepdim=True).values.detach()
        return m + torch.log(torch.bmm(torch.exp(a - m), onehot))

    def torch_train():
        z = logits_of(xs, xq, t)
        loss = F.cross_entropy(z.reshape(-1, N), y_q.reshape(-1))
        return loss, (z.argmax(-1) == y_q).sum(), torch.autograd.grad(loss, [xs, xq, t])

    def torch_fwd():
        with torch.no_grad():
            z = logits_of(f_s, f_q, tau)
            return F.cross_entropy(z.reshape(-1, N), y_q.reshape(-1)), (z.argmax(-1) == y_q).sum()
    with torch.no_grad():
        z_f = hip.match_head_step(ws, f_s, y_s, f_q, y_q, tau, need_grad=False, want_logits=True, n_way=N)["logits"]
        dz = float((z_f - logits_of(f_s, f_q, tau)).abs().max() / z_f.abs().max())
    return {"fused_train": fused_train, "torch_train": torch_train, "cos_train": cos_train,
            "fused_fwd": fused_fwd, "torch_fwd": torch_fwd, "cos_fwd": cos_fwd}, dz


res = {"device": torch.cuda.get_device_name(0), "head": []}
fmt = lambda t: f"{t[0]:.1f} us (min {t[1]:.1f}, max {t[2]:.1f})"
Fd = 640
for B in (32, 4) if opt.small else (32,):
    for N, K in [(5, 1), (5, 5), (20, 5)]:
        Qn = 15 * N
        routes, dz = head_case(B, N, K, Qn, Fd)
        if opt.profile_only:
            for _ in range(5):
                for fn in routes.values():
                    fn()
            continue
        t = alternate(routes, opt.iters, opt.blocks)
        res["head"].append(dict(B=B, N=N, K=K, Qn=Qn, F=Fd, logits_fused_vs_torch_rel_to_max=dz, **{k + "_us": v for k, v in t.items()}))
        print(f"head B={B} N={N} K={K} Qn={Qn} F={Fd}: training form fused {fmt(t['fused_train'])}, torch ops {fmt(t['torch_train'])} "
              f"({t['torch_train'][0] / t['fused_train'][0]:.2f} x), cosine head {fmt(t['cos_train'])} "
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
