"""Walks the form table of the FuMI step's hypernetwork (tests/hyper_forms.py) on the GPU -- every row, then every knob setting's rows
in a child process of its own -- and writes, per row and quantity, the error of the step against the float64 oracle, the float32
oracle's error against the same (the witness), their ratio with and without the floor, the plans the step reported, and the form
margin that follows: the smallest power of two that is at least twice the largest ratio (errors below ERR_FLOOR count as ERR_FLOOR).

    python tools/hyper_forms_report.py profiles/hyper_forms/errors.json"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import hyper_forms as F  # noqa: E402
from fumi_amd import hip  # noqa: E402


def walk(names, changes=None):
    dev = torch.device("cuda:0")
    ws = hip.Workspace.get(dev)
    rows = {}
    for name in names:
        inp = F.make_inputs(name)
        r64, r32 = F.oracle(name, inp, torch.float64), F.oracle(name, inp, torch.float32)
        out = F.run_step(name, inp, dev, ws)
        status = ws.read_status()
        plan, seen = F.reported(name)
        again = F.run_step(name, inp, dev, ws)
        got, wit = F.errors(name, out, r64), F.errors(name, r32, r64)
        ratio = {q: max(got[q], F.ERR_FLOOR) / max(wit[q], F.ERR_FLOOR) for q in got}
        raw = {q: (got[q] / wit[q] if wit[q] > 0 else None) for q in got}           # without the floor: for reading, not for the bound
        q = max(ratio, key=ratio.get)
        want = F.table_plan(name, None if changes is None else changes[name])
        rows[name] = dict(status=status, plan=seen, plan_is_table=seen == want, plan_is_query=plan == F.query_plan(name),
                          guards=F.guard_report(out), rerun_differs=F.outputs_equal(out, again), form=got, witness=wit, ratio=ratio,
                          ratio_unfloored=raw, worst=[ratio[q], q])
        print(f"{name:14s} status {status} plan {'ok' if rows[name]['plan_is_table'] else seen} worst ratio {ratio[q]:.2f} ({q}) "
              f"form {got[q]:.2e} witness {wit[q]:.2e} max form {max(got.values()):.2e}", file=sys.stderr, flush=True)
    return rows


def main(path):
    res = {"default": walk(F.ALL_CASES)}
    for i, (env, rows) in enumerate(F.KNOB_SETTINGS):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--setting", str(i)], env=F.child_env(env), capture_output=True,
                           text=True, timeout=600)
        sys.stderr.write(r.stderr[-4000:])
        if r.returncode != 0:
            raise SystemExit(f"setting {F.setting_id(env)}: exit status {r.returncode}")        # (nothing more is started)
        res[F.setting_id(env)] = json.loads(r.stdout.strip().splitlines()[-1])
    worst = max(((v["worst"][0], s, n, v["worst"][1]) for s, rows in res.items() for n, v in rows.items()))
    margin = 1
    while margin < 2 * worst[0]:
        margin *= 2
    out = dict(err_floor=F.ERR_FLOOR, largest_ratio=worst[0], largest_ratio_setting=worst[1], largest_ratio_row=worst[2],
               largest_ratio_quantity=worst[3], margin=margin, margin_in_table=F.FORM_MARGIN, settings=res)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"largest ratio {worst[0]:.2f} at {worst[1]} / {worst[2]} / {worst[3]}: margin {margin} (table: {F.FORM_MARGIN})")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--setting":
        ch = F.KNOB_SETTINGS[int(sys.argv[2])][1]
        print(json.dumps(walk(list(ch), ch)))
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hyper_forms", "errors.json"))
