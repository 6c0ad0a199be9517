"""CPU suite: keeps the case table of tests/xpanel_forms.py honest (no GPU, no library).

tests/test_xpanel_forms_gpu.py holds every kernel form of csrc/xpanel.hip to a float64 product at 2e-6 (A0, gW0) / 4e-6 (G) of the
reference's maximum.  That only means something when a plain float32 product of the same inputs stays within HALF of each bound
(the bound then has a factor 2 over the reference's own rounding), when no case is larger than it has to be, when the plans the
table spells out are the ones the restated dispatch rules give, and when every kernel instance the two launchers can launch is
named by the expected plan of some row under some setting."""
import pytest
import torch

import xpanel_forms as F


@pytest.mark.parametrize("name", F.ALL_CASES)
def test_case_is_small_and_float32_meets_half_the_bound(name):
    c = F.CASES[name]
    assert F.macs(c) <= F.MAX_MACS, f"{F.macs(c):.3g} multiply-adds"
    assert c["align"] in F.ALIGNS and (c["S"] > 0 or c["Qn"] > 0)
    d = F.make_inputs(name)
    r64 = F.reference(name, d, torch.float64)
    r32 = F.reference(name, d, torch.float32)
    tols = (F.A0_TOL, F.G_TOL) if c["pass_"] == "fwd" else (F.A0_TOL,)
    for a, b, tol in zip(r32, r64, tols):
        assert float(b.abs().max()) > 0
        e = F.rel_err(a, b)
        assert e <= 0.5 * tol, f"float32 matmul off by {e:.3e} of the maximum (half bound {0.5 * tol:.1e})"


@pytest.mark.parametrize("name", F.ALL_CASES)
def test_table_plan_is_the_default_dispatch(name):
    want = F.expected_plan(name, {})
    for k, v in F.table_plan(name).items():
        assert want[k] == v, f"{k}: the table says {v}, the dispatch rules give {want[k]}"
    p = F.CASES[name]["parent"]
    if p:                                   # a one-sided panel stays in its parent's kernel family
        assert F.expected_plan(p, {})["bwd_kernel"] == want["bwd_kernel"]


def test_every_kernel_instance_is_named_by_some_expected_plan():
    seen = {}
    for env in [{}] + F.KNOB_SETTINGS:
        for name in F.ALL_CASES:
            seen.setdefault(F.instance(F.expected_plan(name, env)), (F.setting_id(env) or "default", name))
    assert set(seen) == F.INSTANCES, (F.INSTANCES - set(seen), set(seen) - F.INSTANCES)
    default = {F.instance(F.expected_plan(n, {})) for n in F.ALL_CASES}
    assert default == {i for i in F.INSTANCES if i not in ("xpanel_fwd_generic_kernel<true>", "xpanel_fwd_kernel<1>", "xpanel_fwd_kernel<2>",
                                                           "xpanel_fwd_kernel<3>", "xpanel_fwd_sb_kernel<4,false>", "xpanel_bwd256_kernel<false>",
                                                           "xpanel_bwd256_sb_kernel<false,2,1,32>")}


def test_knob_plans():
    """What each setting moves, on the rows it is there for."""
    P = F.expected_plan
    assert P("f_ps_d288", {"FUMI_XP_SB": "0"})["fwd_kernel"] == 2 and P("f_sb_d96", {"FUMI_XP_SB": "0"})["fwd_kernel"] == 2
    assert P("f_sb_d256_h128", {"FUMI_XP_SB": "0"})["fwd_kernel"] == 3
    assert P("f_sb_seam", {"FUMI_XP_SB": "0", "FUMI_XP_NST": "1"})["fwd_ring"] == 1
    assert P("f_sb_seam", {"FUMI_XP_SB": "0", "FUMI_XP_NST": "3"})["fwd_ring"] == 3
    assert P("f_ps_d288", {"FUMI_XP_PS": "0"})["fwd_kernel"] == 4
    assert P("f_sb_seam", {"FUMI_XP_SBN": "4"})["fwd_ring"] == 4 and P("f_ps_d288", {"FUMI_XP_SBN": "4"})["fwd_kernel"] == 5
    assert P("b_wide_nb2_h256", {"FUMI_XPB_SB": "0"})["bwd_kernel"] == 3 and P("b_nar_k340", {"FUMI_XPB_SB": "0"})["bwd_kernel"] == 2
    assert P("b_wide_nb2_h256", {"FUMI_XPB_NB": "1"})["bwd_nb"] == 1
    assert P("b_wide_nb2_h256", {"FUMI_XPB_NB": "1", "FUMI_XPB_SK": "32"})["bwd_sk"] == 32
    assert P("b_wide_nb2_h256", {"FUMI_XPB_64": "1"})["bwd_kernel"] == 2 and P("b_nar_k340", {"FUMI_XPB_64": "1"})["bwd_kernel"] == 5
    one = {"FUMI_XPB_WG": "1"}
    narrow_shape = lambda c: c["h0"] == 64 and c["D"] % 256 == 0            # (its split is sized by D alone, whatever runs it)
    assert all(P(n, one)["bwd_nsplit"] == 1 for n, c in F.CASES.items() if c["pass_"] == "bwd" and not narrow_shape(c))
    assert P("b_wide_straddle", {"FUMI_XPB_WG": "100000"})["bwd_nsplit"] == 26         # the split is clamped at 32 slabs
    assert P("b_g64_d72_h40", {"FUMI_XPB_WG": "100000"})["bwd_kchunk"] == 32


def test_table_holds_the_edges_it_is_there_for():
    C = F.CASES
    fwd = [c for c in C.values() if c["pass_"] == "fwd"]
    bwd = [c for c in C.values() if c["pass_"] == "bwd"]
    ps = [c for c in fwd if c["kernel"] == "presplit"]
    assert {63, 64, 65, 129} <= {c["S"] + c["Qn"] for c in ps} and {1, 32, 33, 65} <= {c["S"] for c in ps}
    assert {1, 8, 9} <= {c["B"] for c in ps} and 288 in {c["D"] for c in ps} and 384 in {c["h0"] for c in ps}
    assert {72, 130, 31, 1} <= {c["D"] for c in fwd if c["kernel"] == "generic" and c["align"] == "none"}
    assert {"x_s", "x_q", "W0"} <= {c["align"] for c in fwd if c["D"] == 256}
    nar = [c for c in bwd if c["kernel"] == "narrow_split" and c["S"] and c["Qn"]]
    assert {5, 32, 33, 340} <= {c["B"] * (c["S"] + c["Qn"]) for c in nar} and {256, 512} <= {c["D"] for c in nar}
    wide = [n for n, c in C.items() if c["kernel"] == "wide_split"]
    assert {(1, 256), (1, 512), (2, 256), (2, 512)} <= {(F.expected_plan(n, {})["bwd_nb"], C[n]["h0"]) for n in wide}
    assert any(F.expected_plan(n, {})["bwd_nsplit"] % 8 for n in wide)
    assert {1.0, 0.125, -3.0} <= {c["scale"] for c in bwd}
    for k in F.BWD_KERNELS.values():
        if k != "wide_fp32":
            assert any(c["kernel"] == k and c["S"] == 0 for c in bwd) and any(c["kernel"] == k and c["Qn"] == 0 for c in bwd), k
