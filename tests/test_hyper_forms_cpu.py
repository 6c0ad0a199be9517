"""CPU suite: keeps the form table of tests/hyper_forms.py honest and pins the decisions the hypernetwork of the FuMI step takes
(csrc/hyper.hip, the rider branches of csrc/xpanel.hip, fumi_step_impl) on a machine without a GPU.
fumi_hip_hyper_plan_query asks the predicates the launch path asks, so a predicate that moves changes an entry some row states."""
import functools
import json
import subprocess
import sys

import pytest
import torch

import hyper_forms as F
from conftest import ROOT


def test_key_lists_agree_with_the_binding():
    from fumi_amd import hip
    assert F.PLAN_KEYS == hip.HYPER_PLAN_KEYS and set(F.RODE_KEYS) <= set(hip.XPANEL_PLAN_KEYS)
    assert {v: k for k, v in F.FWD.items()} == hip.HYPER_FWD_FORMS and {v: k for k, v in F.BWD.items()} == hip.HYPER_BWD_FORMS
    assert set(hip.HYPER_TEXT_GRAD) == {0, 1, 2}


@pytest.mark.parametrize("name", F.ALL_CASES)
def test_row_plan_is_what_the_library_plans(name):
    c = F.CASES[name]
    assert F.macs(c) <= F.MAX_MACS, f"{F.macs(c):.3g} multiply-adds"
    got, want = F.query_plan(name), F.table_plan(name)
    assert got == {k: want[k] for k in F.PLAN_KEYS}, {k: (want[k], got[k]) for k in F.PLAN_KEYS if got[k] != want[k]}
    R_ = c["B"] * c["N"]
    assert want["nrb"] == (R_ + 15) // 16 and want["nch"] == (0 if c["Ht"] % 64 else c["Ht"] // 64)
    assert want["fwd_rode"] == int(want["fwd_form"] in (F.FWD["rode_split"], F.FWD["rode_presplit"]))
    assert want["bwd_rode"] == int(want["bwd_form"] == F.BWD["rode"])


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import hyper_forms as F
print(json.dumps({n: F.query_plan(n) for n in F.ALL_CASES}))
"""


@pytest.mark.parametrize("setting", range(len(F.KNOB_SETTINGS)), ids=[F.setting_id(e) for e, _ in F.KNOB_SETTINGS])
def test_knob_setting_changes_its_rows_as_the_table_says(setting):
    """The named rows move to what the setting says (an empty change: the row stays); among the rows the setting does not name, only
    rows of the same kind may move -- they are listed by the failure message when a named row is wrong."""
    env, rows = F.KNOB_SETTINGS[setting]
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=F.child_env(env), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for name, changes in rows.items():
        want = F.table_plan(name, changes)
        assert got[name] == {k: want[k] for k in F.PLAN_KEYS}, (name, {k: (want[k], got[name][k]) for k in F.PLAN_KEYS if got[name][k] != want[k]})
        assert set(changes) <= set(F.PLAN_KEYS) | set(F.RODE_KEYS)
    # the setting changes nothing about a row it has no business with: the plain-GEMM rows and the row-block counts
    for name in ("gemm_dt18", "gemm_ht20"):
        assert got[name] == {k: F.table_plan(name)[k] for k in F.PLAN_KEYS}, name
    for name in F.ALL_CASES:
        assert (got[name]["nrb"], got[name]["nch"]) == (F.table_plan(name)["nrb"], F.table_plan(name)["nch"]), name


def test_knob_settings_are_the_five_the_forms_answer_to():
    assert [F.setting_id(e) for e, _ in F.KNOB_SETTINGS] == ["FUMI_HYPER_FWD=0", "FUMI_HYPER_FWD=1", "FUMI_HYPER_BWD=0", "FUMI_XP_RIDER=0",
                                                             "FUMI_OVERLAP=3"]
    for _, rows in F.KNOB_SETTINGS:
        assert any(ch for ch in rows.values()), "a setting that moves no row"


def test_every_form_instance_and_edge_is_reached():
    plans = [F.table_plan(n) for n in F.ALL_CASES]
    knob = [F.table_plan(n, ch) for _, rows in F.KNOB_SETTINGS for n, ch in rows.items()]
    assert {p["fwd_form"] for p in plans} == set(F.FWD.values())
    assert {p["bwd_form"] for p in plans} == set(F.BWD.values())
    fused = {p["fwd_inst"] for p in plans if p["fwd_form"] == F.FWD["fused"]}
    assert fused == {10 * nt + nch for nt in (1, 2) for nch in (1, 2, 3, 4)}
    assert {p["fwd_inst"] for p in plans if p["fwd_form"] == F.FWD["split"]} == {20, 48}
    assert {p["fwd_inst"] for p in plans if p["fwd_form"] in (F.FWD["rode_split"], F.FWD["rode_presplit"])} == {24}
    assert {p["bwd_dpasses"] for p in plans if p["bwd_form"] in (F.BWD["fused"], F.BWD["rode"])} == {1, 2, 3}
    assert {p["bwd_dpasses"] for p in plans if p["bwd_form"] == F.BWD["rode"]} == {1, 2, 3}
    assert {p["text_grad"] for p in plans} == {0, 1, 2}
    # the text gradient after a ridden, an own fused and a two-launch backward, and inside the fallback
    assert {(p["bwd_form"], p["text_grad"]) for p in plans + knob} >= {(4, 1), (3, 1), (2, 1), (1, 2), (4, 0), (3, 0), (2, 0)}
    assert any(p["fwd_form"] == F.FWD["per_layer"] for p in knob) and any(p["bwd_form"] == F.BWD["two_launch"] for p in knob)
    C = F.CASES
    ridden = [c for c in C.values() if c["plan"]["fwd_rode"] and (c["plan"]["bwd_rode"] or not c["need_grad"])]
    # row blocks: R = 10, 128, 129, 143 ridden both ways
    assert {10, 128, 129, 143} <= {c["B"] * c["N"] for c in ridden}
    assert {4, 16, 20, 300, 384, 388, 768} <= {c["Dt"] for c in ridden} and C["dt772"]["plan"]["fwd_rode"] == 0
    assert {64, 256, 320} <= {c["Ht"] for c in ridden}
    assert {2, 16, 17, 64, 65, 128} <= {c["hid"][-1] + 1 for c in ridden} and C["h1_129"]["plan"]["bwd_rode"] == 1
    assert {True, False} == {c["tanh"] for c in ridden} == {c["want_text_grad"] for c in ridden}
    assert any(not c["need_grad"] for c in ridden)
    # both forward hosts, both backward hosts (NB = 2 at D % 128 == 0, NB = 1 otherwise)
    assert {c["plan"]["fwd_form"] for c in ridden} == {F.FWD["rode_split"], F.FWD["rode_presplit"]}
    assert {c["D"] % 128 == 0 for c in C.values() if c["plan"]["bwd_rode"]} == {True, False}
    assert set(F.OFFS) == {c["off"] for c in C.values() if c["off"]}


@pytest.mark.parametrize("pair", F.EDGE_PAIRS, ids=[f"{a}|{b}" for a, b, _, _ in F.EDGE_PAIRS])
def test_edge_pair_differs_in_exactly_the_entries_and_arguments_it_names(pair):
    a, b, about, args = pair
    pa, pb = F.table_plan(a), F.table_plan(b)
    assert {k for k in pa if pa[k] != pb[k]} == about
    ca, cb = F.CASES[a], F.CASES[b]
    assert {k for k in ca if k not in ("plan", "seed") and ca[k] != cb[k]} == args


@functools.lru_cache(maxsize=None)
def _witness(name):
    inp = F.make_inputs(name)
    return F.oracle(name, inp, torch.float64), F.oracle(name, inp, torch.float32)


@pytest.mark.parametrize("name", F.ALL_CASES)
def test_seed_is_fit_for_purpose(name):
    """The float32 oracle is the witness of the form bound: it agrees with its own float64 run to well inside the project's bounds (no
    ReLU on a kink), and no prediction is a near-tie."""
    r64, r32 = _witness(name)
    assert bool(F.margin_mask(r64["logits"]).all()), "a near-tie: pick another seed (SEED_OVERRIDE)"
    for q, e in F.errors(name, r32, r64).items():
        assert e <= F.WITNESS_TOL, f"{q}: the float32 oracle is {e:.3e} from its float64 run: pick another seed (SEED_OVERRIDE)"
    assert torch.equal(r32["preds"], r64["preds"])
