"""CPU suite: keeps the case table of tests/am3_forms.py honest (no GPU, no library).

tests/test_am3_forms_gpu.py holds the HIP AM3 step to the float64 oracle at GRAD_TOL = 1e-4 of every tensor's own maximum and to
bit-exact predictions on the "safe" rows.  That only means something when the table's inputs leave room for it: nearly every row
safe, a float32 run of the same oracle agreeing with the float64 one a decade below the GPU tolerance (the inputs are not
ill-conditioned), and no gradient tensor so small that the 1e-5 floor of helpers.rel_to_max decides its comparison.

Weakest values of the table (seeds 4000 + row index): safe share 0.984 (n64_p48); float32-vs-float64 gradient error 6.6e-6 of the
tensor's own maximum (n2_p512); lamda 1.2e-7; loss 7.1e-7; smallest own maximum of a parameter gradient 8.1e-3 (h.0.weight of n65_p8),
of an image-row adjoint 7.1e-4 (dx_q of n20_p64_q8)."""
import pytest
import torch

import am3_forms as F
from helpers import FLOOR, rel_to_max

F32_TOL = 1e-5            # a tenth of the GPU tolerance


@pytest.mark.parametrize("name", list(F.ALL_CASES))
def test_case_is_well_conditioned(name):
    c, ep, w, masks = F.make_inputs(name)
    r64 = F.run_oracle(c, ep, w, masks, torch.float64)
    r32 = F.run_oracle(c, ep, w, masks, torch.float32)
    safe, pred, empty, first_empty = F.safe_rows(r64["dist"], ep["y_s"], c["N"])
    share = float(safe.float().mean())
    assert share >= F.SAFE_SHARE, f"safe share {share:.3f}"
    if c["ragged"]:
        assert bool(empty[:, c["N"] - 1].all()), "the ragged labels leave class N-1 without a support row"
    # the float32 oracle decides every safe row like the float64 one (its own first arg-min may sit on a LATER empty class only
    # where torch breaks the exact tie differently: collapse it the same way)
    _, pred32, _, _ = F.safe_rows(r32["dist"], ep["y_s"], c["N"])
    assert torch.equal(pred32[safe], pred[safe])
    assert abs(float(r32["loss"]) - float(r64["loss"])) <= F32_TOL * max(1.0, abs(float(r64["loss"])))
    assert rel_to_max(r32["lamda_s"], r64["lamda_s"]) <= F32_TOL
    zero = F.zero_grads(c)
    for k, g64 in r64["all_grads"].items():
        own = float(g64.abs().max())
        if k in zero:
            assert own == 0.0, f"{k} is listed as analytically zero but the oracle gives {own:.3e}"
            assert float(r32["all_grads"][k].abs().max()) == 0.0
            continue
        # the ten parameter gradients stand 100x above the floor.  dx_s / dx_q are per-row adjoints, 1 / (B Qn) of a parameter
        # gradient's size (7.1e-4 at the 5 x 160 query rows of n20_p64_q8): for them the floor must simply not decide, i.e. stay
        # a decade below the tensor's own maximum, which rel_to_max then divides by
        room = 10 if k in ("dx_s", "dx_q") else 100
        assert own > room * FLOOR, f"{k}: own maximum {own:.3e} is within {room}x of the comparison floor"
        e = rel_to_max(r32["all_grads"][k], g64)
        assert e <= F32_TOL, f"{k}: float32 oracle off by {e:.3e} of the tensor's own maximum"


def test_table_covers_every_form():
    """Every branch of the form tree is named by at least one row's plan."""
    plans = [c["plan"] for c in F.CASES.values()]
    assert {p["fast_head"] for p in plans} == {0, 1}
    assert {p["nwaves"] for p in plans if p["fast_head"]} == {16, 8, 4}
    assert {p["hgq"] for p in plans} == {1, 2, 4, 8}
    assert {p["imparts"] for p in plans} >= {1, 2, 4}
    assert any(p["xks"] > 1 and not p["fast_head"] for p in plans), "a split contraction reduced by the launch (generic head)"
    for k in ("g_fwd_split", "g_fwd_rode", "h_fwd_split", "h_bwd_fused", "g_bwd_fused"):
        assert {p[k] for p in plans} == {0, 1}, k
    assert any(p["h_fwd_split"] and not p["g_fwd_split"] for p in plans)
    assert {p["tx_nparts"] for p in plans} >= {0, 1, 2, 5}
    # the shapes behind the forms: a second and a third class pass, a cut chunk of P in a multi-chunk row, all 8 chunks
    Ns = {c["N"] for c in F.CASES.values()}
    assert {1, 9, 17, 20, 64, 65} <= Ns
    assert any(c["P"] > 64 and c["P"] % 64 for c in F.CASES.values() if c["plan"]["fast_head"])
    assert any(c["P"] == 512 and c["plan"]["fast_head"] for c in F.CASES.values())
    assert any(c["P"] > 512 for c in F.CASES.values())


def test_knob_plans():
    """expected_plan: what each knob overrides, and that the overridden rows still name a plan."""
    p, keys = F.expected_plan("n5_p128_ht128", {})
    assert p == F.CASES["n5_p128_ht128"]["plan"] and keys == set(p)
    p, _ = F.expected_plan("n5_p128_ht128", {"FUMI_AM3_GENERIC": 1})
    assert (p["fast_head"], p["nwaves"], p["hgq"], p["imparts"], p["xks"]) == (0, 4, 1, 1, 2)
    p, _ = F.expected_plan("n9_p16", {"FUMI_AM3_GQ": 3})
    assert p["hgq"] == 3
    p, _ = F.expected_plan("n9_p16", {"FUMI_AM3_GQ": 99})
    assert p["hgq"] == 16
    p, _ = F.expected_plan("n65_p8", {"FUMI_AM3_GQ": 3})
    assert p["hgq"] == 1                                      # the generic head has no shares
    p, _ = F.expected_plan("n20_p64_q8", {"FUMI_AM3_MLP": 0})
    assert not any(p[k] for k in ("g_fwd_split", "g_fwd_rode", "h_fwd_split", "h_bwd_fused", "g_bwd_fused", "tx_nparts"))
    p, _ = F.expected_plan("n5_p100_d1024", {"FUMI_XP_KSPLIT": 1})
    assert (p["xks"], p["imparts"]) == (1, 1)
