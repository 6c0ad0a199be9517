"""Times `--model am3 --text_encoder rand` at BASELINE configs[3]'s per-rank shape (5-way 5-shot, 32 queries per class, 32 episodes,
2048-d precomputed image embeddings, text_hid_dim 256, prototype_dim 64) through AM3.evaluate('train'), --dropout 0: the one setting
that both routes run -- the text-rows form of the step (fumi_hip_am3_step_tx, rows drawn on the device) where the engine has it, the
identity in g's place where it has not.  Prints one JSON line: ms per step of a steady loop, the host's cost per step (bursts into an
empty queue) and, with --phases, the per-phase table of the library's own HIP events (a separate loop: the events add bubbles).

    python tools/bench_am3_rand.py [--steps 200] [--warmup 20] [--phases] [--route auto|identity]

--route identity hides the capability from the model, i.e. runs the route of an engine without the form in this tree."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fumi_amd import engine, hip
from fumi_amd.utils import utils as U

ARGV = ["--model", "am3", "--text_encoder", "rand", "--batch_size", "32", "--dropout", "0", "--dataset", "synthetic"]


def batches(a, dev, n=4):
    B, N, K, Q, D, Dt = a.batch_size, a.num_ways, a.num_shots, a.num_shots_test, a.im_emb_dim, a.text_emb_dim
    S, Qn = N * K, N * Q
    out = []
    for i in range(n):
        g = torch.Generator(device=dev).manual_seed(100 + i)
        cg = torch.Generator().manual_seed(100 + i)
        y_s = torch.stack([torch.arange(N).repeat_interleave(K)[torch.randperm(S, generator=cg)] for _ in range(B)]).to(dev)
        y_q = torch.stack([torch.arange(N).repeat_interleave(Q)[torch.randperm(Qn, generator=cg)] for _ in range(B)]).to(dev)
        text_s = torch.zeros(B, S, Dt, device=dev)                          # `rand` reads only its leading shape
        x_s = torch.randn(B, S, D, device=dev, generator=g)
        x_q = torch.randn(B, Qn, D, device=dev, generator=g)
        out.append({'train': ([torch.zeros(B, S, dtype=torch.int64, device=dev), text_s, x_s], y_s),
                    'test': ([torch.zeros(B, Qn, dtype=torch.int64, device=dev), None, x_q], y_q)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--phases", action="store_true")
    ap.add_argument("--route", choices=["auto", "identity"], default="auto")
    ap.add_argument("--label", default="")
    o = ap.parse_args()
    dev = torch.device("cuda:0")
    eng = engine.get_engine()
    if o.route == "identity" and getattr(eng, "am3_rand_native", False):
        type(eng).am3_rand_native = False
    a = U.parser().parse_args(ARGV)
    a.device = dev
    torch.manual_seed(1)
    model = U.init_model(a, None, watch=False)
    opt = U.init_optim(a, model)
    opt_, sched = opt if type(opt) == tuple else (opt, None)
    bs = batches(a, dev)
    step = lambda b: model.evaluate(b, opt_, sched, a.num_ways, dev, "train")
    for i in range(o.warmup):
        step(bs[i % len(bs)])
    ws = hip.Workspace.get(dev)
    hip.raise_on_status(ws.read_status())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(o.steps):
        last = step(bs[i % len(bs)])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    burst = []
    for _ in range(15):
        torch.cuda.synchronize()
        tb = time.perf_counter()
        for i in range(4):
            step(bs[i % len(bs)])
        burst.append((time.perf_counter() - tb) / 4)
    torch.cuda.synchronize()
    burst.sort()
    plan = hip.am3_step_plan()
    rec = {"label": o.label, "route": "native (rows drawn)" if getattr(eng, "am3_rand_native", False) else "identity in g's place",
           "argv": " ".join(ARGV), "steps": o.steps, "ms_per_step": round(el / o.steps * 1e3, 4),
           "host_ms_per_step": round(burst[len(burst) // 2] * 1e3, 4), "final_loss": float(last[0]), "plan": plan,
           "workspace_MiB": round(ws.bytes() / 2 ** 20, 1)}
    if o.phases:
        ws.set_profiling(True, None, every=1)
        for i in range(o.steps):
            step(bs[i % len(bs)])
        prof = ws.profile()
        ws.set_profiling(False)
        rec["phase_us"] = {k: round(v[0] / v[1] * 1e3, 2) for k, v in prof.items()}
        rec["phase_us_sum"] = round(sum(rec["phase_us"].values()), 2)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
