"""CPU suite: keeps the form table of tests/epi_forms.py honest and pins the decisions of plan_episodes (csrc/episode.hip) on a
machine without a GPU.  fumi_hip_epi_plan_query is the host arithmetic run_episodes itself plans with, so a
predicate, a cap, a layout function or a staging builder that moves changes an entry some row pins here."""
import functools
import json
import subprocess
import sys

import pytest
import torch

import epi_forms as F
from conftest import ROOT


def test_key_lists_agree_with_the_binding():
    from fumi_amd import hip
    assert F.PLAN_KEYS == hip.EPI_PLAN_KEYS and set(F.FORM_KEYS) | set(F.DERIVED_KEYS) == set(F.PLAN_KEYS)
    assert {v: k for k, v in F.ADAPT.items()} == hip.EPI_ADAPT_FORMS and {v: k for k, v in F.QUERY.items()} == hip.EPI_QUERY_FORMS
    assert {v: k for k, v in F.REVERSE.items()} == hip.EPI_REVERSE_FORMS


@pytest.mark.parametrize("name", F.ALL_CASES)
def test_row_plan_is_what_the_library_plans(name):
    c = F.CASES[name]
    assert F.macs(c) <= F.MAX_MACS, f"{F.macs(c):.3g} multiply-adds"
    assert c["B"] <= 9 and c["D"] <= 128
    got = F.query_plan(name)
    assert got == F.table_plan(name), {k: (v, got[k]) for k, v in F.table_plan(name).items() if got[k] != v}


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import epi_forms as F
print(json.dumps({n: F.query_plan(n) for n in sys.argv[2:]}))
"""


@pytest.mark.parametrize("setting", range(len(F.KNOB_SETTINGS)), ids=[F.setting_id(e) for e, _ in F.KNOB_SETTINGS])
def test_knob_setting_changes_its_rows_as_the_table_says(setting):
    env, rows = F.KNOB_SETTINGS[setting]
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT] + list(rows), env=F.child_env(env), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for name, changes in rows.items():
        want = F.table_plan(name, changes)
        assert got[name] == want, (name, {k: (v, got[name][k]) for k, v in want.items() if got[name][k] != v})


def test_every_form_and_every_part_count_is_reached():
    plans = [F.table_plan(n) for n in F.ALL_CASES]
    assert {p["adapt"] for p in plans} == set(F.ADAPT.values())
    assert {p["query"] for p in plans} == set(F.QUERY.values())
    assert {p["reverse"] for p in plans} == set(F.REVERSE.values())
    assert {1, 2, 4, 8} <= {p["P"] for p in plans if p["reverse"] != F.REVERSE["global"]}
    assert {p["P"] for p in plans if p["reverse"] == F.REVERSE["lds"]} >= {1, 2, 4, 8}          # 4 in the run-time-shaped sweep too
    assert {p["two_part"] for p in plans} == {0, 1} and {p["drop"] for p in plans} == {0, 1}
    assert {(p["query"], p["drop"]) for p in plans} >= {(0, 0), (0, 1)}                         # both fused_fixed instances
    knob_ap = {ch.get("AP") for _, rows in F.KNOB_SETTINGS for ch in rows.values()}
    assert {2, 4, 8} <= knob_ap
    C = F.CASES.values()
    assert {0, 1, 2} <= {c["T"] for c in C} and {1, 2, 3, 4, 5} <= {len(c["hid"]) for c in C}
    assert {1, 2, 17} <= {c["N"] for c in C} and {1, 9} <= {c["B"] for c in C}
    assert any(c["entry"] == "maml" and c["first_order"] for c in C) and any(not c["need_grad"] for c in C)
    assert any(F.dims(c)[1] == 1 for c in C) and any(F.dims(c)[1] % 32 == 1 and F.dims(c)[1] > 32 for c in C)
    assert {"W1", "b1", "b0"} <= {c["off"] for c in C}
    # the reverse grid 8 ceil(B/8) P with B % 8 != 0 and P > 1, fixed-shape and run-time-shaped
    assert any(c["B"] % 8 and c["plan"]["P"] > 1 and c["plan"]["reverse"] == 0 for c in C)
    assert any(c["B"] % 8 and c["plan"]["P"] > 1 and c["plan"]["reverse"] == 1 for c in C)


@pytest.mark.parametrize("pair", F.EDGE_PAIRS, ids=[f"{a}|{b}" for a, b, _, _ in F.EDGE_PAIRS])
def test_edge_pair_differs_in_exactly_the_entries_and_arguments_it_names(pair):
    a, b, about, args = pair
    pa, pb = F.table_plan(a), F.table_plan(b)
    assert {k for k in F.FORM_KEYS if pa[k] != pb[k]} == about
    ca, cb = F.CASES[a], F.CASES[b]
    assert {k for k in ca if k != "plan" and ca[k] != cb[k]} == args


def test_every_p_step_has_a_pair_about_p_alone():
    steps = {(F.table_plan(a)["P"], F.table_plan(b)["P"]) for a, b, about, args in F.EDGE_PAIRS if about <= {"reverse", "P"} and len(args) == 1}
    assert {(1, 2), (2, 4), (4, 8), (8, 0)} <= steps


def test_layout_restatements_give_every_pinned_total():
    for n, c in F.CASES.items():
        p, (S, _) = c["plan"], F.dims(c)
        if p["al_total"]:
            assert p["al_total"] == F.adapt_total(c["hid"], S, c["N"]), n
        if p["rl_total"] and p["reverse"] == F.REVERSE["lds"]:
            assert p["rl_total"] == F.reverse_total(c["hid"], S, c["N"], p["P"]), n
        if p["ql_total"] and p["query"] != F.QUERY["fused_fixed"] and c["off"] is None:
            assert p["ql_total"] == F.query_total(c["hid"], S, c["N"], fused=p["query"] == F.QUERY["fused"]), n


def test_every_cap_has_a_row_whose_rejected_layout_a_cap_of_40960_would_take():
    """The rejected layout lies in (40000, 40960]: with the cap at 40960 plan_episodes takes it and the row's pinned plan changes."""
    for name, cap, total in F.CAP_OUTSIDE:
        c = F.CASES[name]
        t = total(c, F.dims(c)[0])
        assert F.LDS_CAP < t <= F.LDS_MAX, (name, cap, t)
    assert {cap for _, cap, _ in F.CAP_OUTSIDE} == {"QLDS_CAP", "ALDS_CAP", "RLDS_CAP"}
    plans = {n: F.table_plan(n) for n in F.ALL_CASES}
    assert plans["q_lds_s30"]["query"] == F.QUERY["lds"] and plans["a_glob_s42"]["adapt"] == F.ADAPT["global"]
    assert plans["r_p2_s18"]["P"] == 2 and plans["r_glob_s46"]["reverse"] == F.REVERSE["global"]
    # the 512-unit cap: the outside row's layout fits, so only its table can have refused the form; the inside row is at the cap
    for name, what, total in F.UNITS_OUTSIDE:
        c = F.CASES[name]
        assert total(c, F.dims(c)[0]) <= F.LDS_CAP, (name, what)
    assert plans["s_q511_s28"]["nu_query"] == 511 and plans["s_qglob_s30"]["query"] == F.QUERY["global"]
    assert plans["s_a512_h126"]["nu_adapt"] == 512 and plans["s_aglob_h127"]["adapt"] == F.ADAPT["global"]


def test_lds_rows_fit_their_caps_and_every_cap_has_a_neighbour():
    for n in F.ALL_CASES:
        p = F.table_plan(n)
        assert max(p["ql_total"], p["al_total"], p["rl_total"]) <= F.LDS_CAP, n
        assert max(p[k] for k in F.PLAN_KEYS if k.startswith("nu_")) <= F.UNIT_CAP, n
    for name, arg, granule, what in F.CAP_NEIGHBOURS:
        c = F.CASES[name]
        cur = c["hid"][0] if arg == "h0" else c["hid"][1] if arg == "h1" else c[arg]
        here, there = F.query_plan(name), F.query_plan(name, **{arg: cur + granule})
        assert any(here[k] != there[k] for k in ("adapt", "query", "reverse", "P")), (name, what)


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
