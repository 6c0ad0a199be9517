"""GPU suite: every form of the hypernetwork of the FuMI step (csrc/hyper.hip, csrc/hyper_fwd.h, csrc/hyper_bwd.h, the rider branches
of csrc/xpanel.hip) against oracle.fumi_ref in float64, at the form's edges.

The table (tests/hyper_forms.py) holds one row per form and per side of each edge.  For every row: the plan the step reports
(fumi_hip_hyper_plan) is the table's and is what fumi_hip_hyper_plan_query gives; the X-panel plan's rode entries are the table's;
logits, losses, every theta gradient, the four phi gradients by name and g_cls_text meet the project's bounds against the float64
oracle and exceed the float32 oracle's own error on that row by at most FORM_MARGIN; the gradient outputs sit between NaN guards that
stay NaN and are themselves fully written; a second run is bit-identical (an arrival counter left non-zero would show here), and so
is a run after another row has grown and re-carved the workspace.  The knob-only forms run in one child process per setting over
the rows the setting names."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import hyper_forms as F
from conftest import ROOT

pytestmark = pytest.mark.gpu

# in a child process of test_knob_setting_in_a_child_process: the setting's index; its rows are the only ones that run
_SETTING = os.environ.get("HYPER_FORMS_SETTING")
_CHANGES = F.KNOB_SETTINGS[int(_SETTING)][1] if _SETTING is not None else None
_ROWS = list(_CHANGES) if _CHANGES is not None else F.ALL_CASES
OTHER = {"rb_r143": "dt4"}           # the row run in between: a different shape on the same workspace (rb_r143 is everyone else's)


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
    c = F.CASES[name]
    inp, r64, r32 = _refs(name)
    out = F.run_step(name, inp, dev, ws)
    assert ws.read_status() == 0
    plan, got = F.reported(name)
    want = F.table_plan(name, None if _CHANGES is None else _CHANGES[name])
    assert got == want, {k: (v, got[k]) for k, v in want.items() if got[k] != v}
    assert plan == F.query_plan(name), "fumi_hip_hyper_plan and fumi_hip_hyper_plan_query disagree"
    # guards: nothing outside the gradient outputs written, nothing inside them left unwritten
    assert F.guard_report(out) == []
    # float64 oracle: the project's bounds, then the form bound over the float32 witness
    e, wit = F.errors(name, out, r64), F.errors(name, r32, r64)
    for q in e:
        print(f"{name} {q}: form {e[q]:.3e} witness {wit[q]:.3e}")
    assert set(e) >= {"logits", "loss_b"} and (not c["need_grad"] or set(e) >= {"hyper_net.0.weight", "hyper_net.0.bias",
                                                                                 "hyper_net.2.weight", "hyper_net.2.bias"})
    assert ("g_cls_text" in e) == bool(c["need_grad"] and c["want_text_grad"])
    for q in e:
        assert e[q] <= F.project_bound(q), f"{q}: {e[q]:.3e} of the float64 oracle's maximum"
        assert max(e[q], F.ERR_FLOOR) <= F.FORM_MARGIN * max(wit[q], F.ERR_FLOOR), \
            f"{q}: form error {e[q]:.3e}, float32 oracle {wit[q]:.3e}: more than {F.FORM_MARGIN} x"
    mask = F.margin_mask(r64["logits"])
    assert bool(mask.all())
    assert torch.equal(out["preds"].cpu()[mask], r64["preds"][mask]), "integer predictions differ"
    # a second run: bit-identical in every output
    again = F.run_step(name, inp, dev, ws)
    assert ws.read_status() == 0 and F.guard_report(again) == []
    assert F.outputs_equal(out, again) == []
    # another row on the same workspace (other sizes, other carving, the same counters), then this row again
    other = OTHER.get(name, "rb_r143")
    o = F.run_step(other, _refs(other)[0], dev, ws)
    assert ws.read_status() == 0 and F.guard_report(o) == []
    third = F.run_step(name, inp, dev, ws)
    assert ws.read_status() == 0 and F.guard_report(third) == []
    assert F.outputs_equal(out, third) == []


@pytest.mark.parametrize("setting", range(len(F.KNOB_SETTINGS)), ids=[F.setting_id(e) for e, _ in F.KNOB_SETTINGS])
def test_knob_setting_in_a_child_process(setting, dev):
    env = F.child_env(dict(F.KNOB_SETTINGS[setting][0], HYPER_FORMS_SETTING=str(setting)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_hyper_forms_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider", "-k", "test_row_takes_its_form"], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(F.KNOB_SETTINGS[setting][1])} passed" in r.stdout
