"""Walks the form table of the episode chain (tests/epi_forms.py) on the GPU and writes, per row and quantity, the error of the step
against the float64 oracle, the float32 oracle's error against the same (the witness), their ratio with and without the floor, and the form margin that follows:
the smallest power of two that is at least twice the largest ratio (errors below ERR_FLOOR count as ERR_FLOOR).

    python tools/epi_forms_report.py profiles/epi_forms/errors.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import epi_forms as F  # noqa: E402
from fumi_amd import hip  # noqa: E402


def main(path):
    dev = torch.device("cuda:0")
    ws = hip.Workspace.get(dev)
    rows, worst = {}, (0.0, None, None)
    for name in F.ALL_CASES:
        inp = F.make_inputs(name)
        r64, r32 = F.oracle(name, inp, torch.float64), F.oracle(name, inp, torch.float32)
        out = F.run_step(name, inp, dev, ws)
        status = ws.read_status()
        plan = hip.epi_plan()
        got, wit = F.errors(name, out, r64), F.errors(name, r32, r64)
        ratio = {q: max(got[q], F.ERR_FLOOR) / max(wit[q], F.ERR_FLOOR) for q in got}
        raw = {q: (got[q] / wit[q] if wit[q] > 0 else None) for q in got}           # without the floor: for reading, not for the bound
        q = max(ratio, key=ratio.get)
        if ratio[q] > worst[0]:
            worst = (ratio[q], name, q)
        rows[name] = dict(status=status, plan_is_table=plan == F.table_plan(name), plan_is_query=plan == F.query_plan(name),
                          form=got, witness=wit, ratio=ratio, ratio_unfloored=raw)
        print(f"{name:16s} status {status} plan {'ok' if rows[name]['plan_is_table'] else plan} worst ratio {ratio[q]:.2f} ({q}) "
              f"form {got[q]:.2e} witness {wit[q]:.2e} max form {max(got.values()):.2e}", flush=True)
    margin = 1
    while margin < 2 * worst[0]:
        margin *= 2
    res = dict(err_floor=F.ERR_FLOOR, largest_ratio=worst[0], largest_ratio_row=worst[1], largest_ratio_quantity=worst[2],
               margin=margin, margin_in_table=F.FORM_MARGIN, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(f"largest ratio {worst[0]:.2f} at {worst[1]} / {worst[2]}: margin {margin} (table: {F.FORM_MARGIN})")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "epi_forms", "errors.json"))
