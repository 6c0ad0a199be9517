"""What --max_grad_norm costs: the clipped optimizer step (norm launches, finish launch, the rule on g * coef; csrc/adam.hip)
against the unclipped one.

``standalone``: per rule (adam, adamw, SGD with momentum, SGD) ``optimizer.step_fused()`` alone on fixed random gradients, at the
parameter set of BASELINE.json configs[1] (bench.py's FuMI model) and at the ResNet-12 FuMI parameter set (52 tensors: two chunks).
``fumi_configs1``: the whole training meta-step ``FUMI.evaluate(task="train")`` at configs[1] under --optim adam, flag off (the
update folded into the step's last launch) against --max_grad_norm 1e30 (separate launches; coef 1, the same parameters).

Variants alternate in ONE process (u c u c ...), so clock and host drift hit both alike; a timed region is ``--steps`` steps
between two device synchronisations; a figure is the median of its regions, with min and max (the run-to-run spread).

    python tools/bench_clip.py [--steps 2000] [--regions 5] [--out FILE.json]
    python tools/bench_clip.py --skip-standalone     # the meta-step alone: runs on any commit (a tree without the flag times "off" only)
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

from bench_optim import commit

RULES = {"adam": ("Adam", dict(lr=3e-5, weight_decay=5e-4)), "adamw": ("AdamW", dict(lr=3e-5, weight_decay=0.0)),
         "SGD_momentum": ("SGD", dict(lr=3e-5, momentum=0.9, weight_decay=5e-4)), "SGD": ("SGD", dict(lr=3e-5, momentum=0.0, weight_decay=5e-4))}


def figure(ts):
    return {"us_median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def alternate(variants, o, unit=1e6):
    """variants: name -> callable(n) running n steps.  Returns name -> list of per-step times of its regions."""
    for f in variants.values():
        f(o.warmup)
    torch.cuda.synchronize()
    for _ in range(0, o.settle, 50):
        for f in variants.values():
            f(50)
        torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(o.regions):
        for k, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f(o.steps)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / o.steps * unit)
    return times


def parameter_sets(dev):
    import bench
    from fumi_amd.utils import utils as U
    sets = {"fumi_configs1": [tuple(p.shape) for p in bench.make_model(dev)[0].parameters() if p.requires_grad]}
    a = U.parser().parse_args(["--model", "fumi", "--im_encoder", "resnet12", "--text_encoder", "BERT", "--dropout", "0"])
    a.device = torch.device("cpu")
    sets["fumi_resnet12"] = [tuple(p.shape) for p in U.init_model(a, None, watch=False).parameters() if p.requires_grad]
    return sets


def standalone(o, dev):
    from fumi_amd import optim
    out = {}
    for set_name, shapes in parameter_sets(dev).items():
        rec = {"tensors": len(shapes), "elements": int(sum(torch.Size(s).numel() for s in shapes))}
        for rule, (cls, kw) in RULES.items():
            variants = {}
            for variant, max_norm in (("unclipped", None), ("clipped", 1.0)):
                g = torch.Generator().manual_seed(0)
                ps = [torch.randn(*s, generator=g).to(dev).requires_grad_(True) for s in shapes]
                for p in ps:
                    p.grad = torch.randn(p.shape, generator=g).to(dev)
                if max_norm is None and len(ps) > optim.MAX_TENSORS:
                    continue                      # (more tensors than one unclipped launch takes: torch's own step, not a comparison)
                opt = getattr(optim, cls)(ps, **kw) if max_norm is None else getattr(optim, cls)(ps, max_grad_norm=max_norm, **kw)

                def run(n, opt=opt):
                    for _ in range(n):
                        opt.step_fused()
                variants[variant] = run
            rec[rule] = {k: figure(ts) for k, ts in alternate(variants, o).items()}
        out[set_name] = rec
    return out


def fumi_step(o, dev):
    import bench
    from fumi_amd.utils import utils as U
    c = bench.CFG
    batches = bench.make_batches(c["B_per_gpu"], dev, 1000)
    has_flag = any(f == "--max_grad_norm" for f, _ in U._ENGINE_FLAGS)
    variants = {}
    for variant, max_norm in (("off_folded", None), ("clipped_1e30", 1e30)):
        if max_norm is not None and not has_flag:
            continue
        model, _ = bench.make_model(dev)
        args = SimpleNamespace(device=dev, num_train_adapt_steps=c["T"], num_test_adapt_steps=c["T"], step_size=c["alpha"],
                               first_order=False, optim="adam", lr=3e-5, weight_decay=5e-4, momentum=0.9, batch_size=c["B_per_gpu"],
                               num_ways=c["N"], max_grad_norm=max_norm)
        opt = U.init_optim(args, model)

        def run(n, model=model, args=args, opt=opt):
            for i in range(n):
                model.evaluate(args, batches[i % len(batches)], opt, "train")
        variants[variant] = run
    return {k: figure(ts) for k, ts in alternate(variants, o).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000, help="steps of one timed region")
    ap.add_argument("--regions", type=int, default=5, help="timed regions per variant (at least five for a figure)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--settle", type=int, default=300, help="further untimed steps per variant before the first region")
    ap.add_argument("--skip-standalone", action="store_true")
    ap.add_argument("--commit", default=None, help="commit hash to record (a source tree without git history cannot tell)")
    ap.add_argument("--out", default=None, help="also write the JSON record to this file")
    o = ap.parse_args()
    assert torch.cuda.is_available(), "bench_clip.py measures on the GPU; there is no CPU fall-back"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rec = {"tool": "tools/bench_clip.py", "commit": o.commit or commit(), "gpu": torch.cuda.get_device_name(0), "steps_per_region": o.steps,
           "regions": o.regions, "order": "alternated in one process", "unit": "us per step"}
    if not o.skip_standalone:
        rec["standalone"] = standalone(o, dev)
    rec["fumi_configs1"] = fumi_step(o, dev)
    line = json.dumps(rec)
    print(line, flush=True)
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
