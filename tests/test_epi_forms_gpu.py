"""GPU suite: every form of the episode chain (csrc/episode.hip) against oracle.fumi_ref in float64, at the form's edges.

The table (tests/epi_forms.py) holds the smallest shape that reaches each form or sits on one side of an edge between two.  For every
row: the plan the step reports (fumi_hip_epi_plan) is the table's and is what fumi_hip_epi_plan_query gives for the same arguments;
logits, losses, predictions and every gradient meet the project's bounds against the float64 oracle, and exceed the float32 oracle's
own error on that row by at most FORM_MARGIN; a second run is bit-identical.  The knob-only forms run in one child process per
setting over the rows the setting changes."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import epi_forms as F
from conftest import ROOT

pytestmark = pytest.mark.gpu

# in a child process of test_knob_setting_in_a_child_process: the setting's index; its rows are the only ones that run
_SETTING = os.environ.get("EPI_FORMS_SETTING")
_CHANGES = F.KNOB_SETTINGS[int(_SETTING)][1] if _SETTING is not None else None
_ROWS = list(_CHANGES) if _CHANGES is not None else F.ALL_CASES


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


@functools.lru_cache(maxsize=None)
def _refs(name):
    inp = F.make_inputs(name)
    return inp, F.oracle(name, inp, torch.float64), F.oracle(name, inp, torch.float32)


@pytest.mark.parametrize("name", _ROWS)
def test_row_takes_its_form_and_matches_float64(name, dev, ws):
    from fumi_amd import hip
    c = F.CASES[name]
    inp, r64, r32 = _refs(name)
    out = F.run_step(name, inp, dev, ws)
    assert ws.read_status() == 0
    plan = hip.epi_plan()
    want = F.table_plan(name, None if _CHANGES is None else _CHANGES[name])
    assert plan == want, {k: (v, plan[k]) for k, v in want.items() if plan[k] != v}
    assert plan == F.query_plan(name), "fumi_hip_epi_plan and fumi_hip_epi_plan_query disagree"
    # float64 oracle: the project's bounds, then the form bound over the float32 witness
    got, wit = F.errors(name, out, r64), F.errors(name, r32, r64)
    for q in got:
        print(f"{name} {q}: form {got[q]:.3e} witness {wit[q]:.3e}")
    for q in got:
        assert got[q] <= F.project_bound(q), f"{q}: {got[q]:.3e} of the float64 oracle's maximum"
        assert max(got[q], F.ERR_FLOOR) <= F.FORM_MARGIN * max(wit[q], F.ERR_FLOOR), \
            f"{q}: form error {got[q]:.3e}, float32 oracle {wit[q]:.3e}: more than {F.FORM_MARGIN} x"
    mask = F.margin_mask(r64["logits"])
    assert bool(mask.all())
    assert torch.equal(out["preds"].cpu()[mask], r64["preds"][mask]), "integer predictions differ"
    acc = out["preds"].cpu().eq(inp[0]["y_q"]).float().mean(-1)
    assert torch.equal(out["acc_b"].cpu(), acc)
    # a second run: bit-identical in every output
    again = F.run_step(name, inp, dev, ws)
    assert ws.read_status() == 0
    for k in ("logits", "loss_b", "preds", "acc_b"):
        assert torch.equal(out[k], again[k]), k
    if c["need_grad"]:
        for n, a, b in zip(F.names(c), out["grads"], again["grads"]):
            assert torch.equal(a, b), n


@pytest.mark.parametrize("setting", range(len(F.KNOB_SETTINGS)), ids=[F.setting_id(e) for e, _ in F.KNOB_SETTINGS])
def test_knob_setting_in_a_child_process(setting, dev):
    env = F.child_env(dict(F.KNOB_SETTINGS[setting][0], EPI_FORMS_SETTING=str(setting)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_epi_forms_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider", "-k", "test_row_takes_its_form"], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(F.KNOB_SETTINGS[setting][1])} passed" in r.stdout
