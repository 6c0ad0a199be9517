"""What the outer optimizer costs per FuMI training step: ``FUMI.evaluate(task="train")`` at BASELINE.json configs[1] (bench.py's
shapes, meta-batches resident on the device) under --optim adam, SGD, adamw and adamw_lin_schedule.

The four rules are alternated in ONE process (a s w l a s w l ...), so clock and host drift hit all of them alike; each timed
region is ``--steps`` steps between two device synchronisations; the figure of a rule is the median of its regions, with min and
max.  Only ``init_optim`` and ``evaluate`` are used, so the file runs unchanged on any commit that has them.  FuMI's training
loop never steps the scheduler of adamw_lin_schedule (as the reference's does not); here it is stepped after every ``evaluate``,
so that the learning rate really changes from step to step.

    python tools/bench_optim.py [--steps 2000] [--regions 7] [--out FILE.json]
    python tools/bench_optim.py --only adamw --steps 200 --regions 1 --settle 0     # under rocprofv3 --kernel-trace --stats
    python tools/bench_optim.py --others          # one adamw figure each for AM3 (configs[3] per rank) and MAML (configs[0])
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

RULES = ["adam", "SGD", "adamw", "adamw_lin_schedule"]


def commit():
    try:
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def fumi_rules(o, dev):
    import bench
    from fumi_amd import hip
    from fumi_amd.utils import utils as U
    c = bench.CFG
    batches = bench.make_batches(c["B_per_gpu"], dev, 1000)
    runs = {}
    for rule in ([o.only] if o.only else RULES):
        model, _ = bench.make_model(dev)
        args = SimpleNamespace(device=dev, num_train_adapt_steps=c["T"], num_test_adapt_steps=c["T"], step_size=c["alpha"],
                               first_order=False, optim=rule, lr=3e-5, weight_decay=5e-4, momentum=0.9, batch_size=c["B_per_gpu"],
                               num_ways=c["N"], num_warmup_steps=100, epochs=10 ** 7)
        opt = U.init_optim(args, model)
        opt, sched = opt if type(opt) == tuple else (opt, None)
        runs[rule] = (model, args, opt, sched)

    def steps(rule, n):
        model, args, opt, sched = runs[rule]
        last = None
        for i in range(n):
            last = model.evaluate(args, batches[i % len(batches)], opt, "train")
            if sched is not None:
                sched.step()
        return last

    for rule in runs:
        steps(rule, o.warmup)
    torch.cuda.synchronize()
    hip.raise_on_status(hip.Workspace.get(dev).read_status())
    for i in range(0, o.settle, 50):                       # clock ramp of a GPU that idled while the process started
        for rule in runs:
            steps(rule, 50)
        torch.cuda.synchronize()
    times = {rule: [] for rule in runs}
    last = {}
    for r in range(o.regions):
        for rule in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[rule] = steps(rule, o.steps)
            torch.cuda.synchronize()
            times[rule].append((time.perf_counter() - t0) / o.steps * 1e3)
    out = {}
    for rule, ts in times.items():
        opt = runs[rule][2]
        out[rule] = {"ms_per_step_median": round(statistics.median(ts), 5), "min": round(min(ts), 5), "max": round(max(ts), 5),
                     "regions": [round(t, 5) for t in ts], "optimizer_class": f"{type(opt).__module__}.{type(opt).__name__}",
                     "final_loss": float(last[rule][0]), "final_lr": float(opt.param_groups[0]["lr"])}
    return out


def others(o, dev):
    """AM3 (``step_fused``) and MAML (``optimizer.step()``) under --optim adamw: no fold there, one figure each."""
    import bench_configs as bc
    from fumi_amd.models import maml as maml_mod
    from fumi_amd.utils import utils as U
    out = {}
    for name in ("am3_b32", "maml_5w1s_b4_t5"):
        a = U.parser().parse_args(bc.CONFIGS[name] + ["--dropout", "0", "--dataset", "synthetic", "--optim", "adamw"])
        a.device = dev
        torch.manual_seed(1)
        model = U.init_model(a, None, watch=False)
        opt = U.init_optim(a, model)
        bs = bc.batches(a, dev)

        def step(b):
            if a.model == "maml":
                return maml_mod.evaluate(a, model, b, opt, "train")
            return model.evaluate(b, opt, None, a.num_ways, dev, "train")
        for i in range(o.warmup + 200):
            step(bs[i % len(bs)])
        ts = []
        for r in range(o.regions):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(o.other_steps):
                step(bs[i % len(bs)])
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / o.other_steps * 1e3)
        out[name] = {"optim": "adamw", "ms_per_step_median": round(statistics.median(ts), 5), "min": round(min(ts), 5),
                     "max": round(max(ts), 5), "optimizer_class": f"{type(opt).__module__}.{type(opt).__name__}"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000, help="steps of one timed region")
    ap.add_argument("--regions", type=int, default=7, help="timed regions per rule (at least five for a figure)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--settle", type=int, default=500, help="further untimed steps per rule before the first region")
    ap.add_argument("--only", choices=RULES, default=None, help="one rule only (kernel traces)")
    ap.add_argument("--others", action="store_true", help="the AM3 and MAML adamw figures instead of the FuMI table")
    ap.add_argument("--other-steps", type=int, default=300)
    ap.add_argument("--commit", default=None, help="commit hash to record (a source tree without git history cannot tell)")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    o = ap.parse_args()
    assert torch.cuda.is_available(), "bench_optim.py measures on the GPU; there is no CPU fall-back"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rec = {"tool": "tools/bench_optim.py", "commit": o.commit or commit(), "gpu": torch.cuda.get_device_name(0), "steps_per_region": o.steps,
           "regions": o.regions, "order": "alternated in one process"}
    rec["others" if o.others else "fumi_configs1"] = others(o, dev) if o.others else fumi_rules(o, dev)
    line = json.dumps(rec)
    print(line, flush=True)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
