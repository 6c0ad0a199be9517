"""CPU suite: keeps the table of tests/rn12_conv_forms.py honest against the library's own host query (no GPU: the query of
fumi_hip_rn12_conv_query / fumi_hip_rn12_wgrad_query is host arithmetic shared with the launchers).

Every row is small; the integer rows cannot round in any summation order; a plain float32 restatement stays within half of each
fp32 cap (and the recorded bf16 allowances are the measured ones); the plans the table spells out are what the dispatcher chooses;
every instance the dispatcher can choose by default is named by a default row, and the table holds the edges it is there for."""
import pytest
import torch

import rn12_conv_forms as F


@pytest.fixture(scope="module")
def hip():
    import os
    from fumi_amd import hip
    assert not any(os.environ.get(k) for k in F.KNOBS), "the table's plans are those of a process with no knob set"
    return hip


@pytest.mark.parametrize("name", F.ALL_CASES)
def test_row_is_small_and_its_plan_is_the_default_dispatch(name, hip):
    c = F.CASES[name]
    assert F.macs(c) <= F.MAX_MACS, f"{F.macs(c):.3g} multiply-adds"
    assert c["H"] * c["W"] <= 32 * 33, "no row is sized like the workload"
    assert F.PLANS[name] == F.query(name, hip)


@pytest.mark.parametrize("name", F.ALL_CASES)
def test_integer_row_cannot_round(name):
    """Sum of the absolute values of every output's terms: <= 256 for a bf16 output (every partial sum is an integer of at most 9
    bits: exact in bf16 and in fp32), < 2^24 for dW and for the statistics (sum |y|, sum |y| |dot| or sum |y|^2)."""
    c = F.CASES[name]
    d = F.make_inputs(name, "int")
    for t in d.get("x", []) + d.get("dy", []) + d.get("w", []):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 2
    a = F.reference(name, d, torch.float64, absolute=True)
    if c["pass_"] == "wgrad":
        assert float(a.max()) < 2 ** 24
        return
    assert float(a.max()) <= 256
    ws = d["w"]
    touched = [w.abs().sum((0, 2 if c["pass_"] == "dgrad" else 1)) for w in ws]        # per (input channel, tap) over episodes and Cout
    assert all(bool((t > 0).all()) for t in touched), "a (tap, input channel) position no output channel reads"
    if c["stats"]:
        dot = None if d["dot"] is None else d["dot"].abs().double()
        assert float(F.stats_of(a, dot).max()) < 2 ** 24


@pytest.mark.parametrize("name", F.ALL_CASES)
def test_float32_restatement_meets_half_of_each_cap(name):
    c = F.CASES[name]
    r64, e32 = F.gauss_reference(name)
    assert float(r64.abs().max()) > 0
    # (E32 records this measurement on the machine the table was written on; the summation order of a CPU float32 product depends on
    #  the host and its thread count, so the GPU suite measures it again where it runs and the record is not compared)
    assert name in F.E32 and e32 < 1e-3
    if c["pass_"] == "wgrad":
        assert e32 / float(r64.abs().max()) <= 0.5 * F.FP32_CAP
        return
    # the allowance stays a small part of a bf16 step at the outputs' scale: the bracket is a rounding test, not a tolerance
    assert F.E_FACTOR * e32 <= 2.0 ** -9 * float(r64.abs().max()) / 16
    if c["stats"]:
        y = F.bf(r64.float())
        dot = F.make_inputs(name, "gauss")["dot"]
        s32, s64 = F.stats_of(y, dot), F.stats_of(y.double(), None if dot is None else dot.double())
        assert F.rel_err(s32, s64) <= 0.5 * F.FP32_CAP


def test_every_reachable_instance_is_named(hip):
    default = {F.instance(F.PLANS[n]) for n in F.CONV_CASES}
    assert default == F.DEFAULT_INSTANCES, (F.DEFAULT_INSTANCES - default, default - F.DEFAULT_INSTANCES)
    assert F.DEFAULT_INSTANCES < F.INSTANCES and len(F.INSTANCES) == 40
    # the rest under FUMI_RN_BKS (the knobs are static: the GPU suite checks the plans in one child per setting): a default row of
    # every (NF, 128-pixel tile, S16) for FUMI_RN_BKS=2, and the two NF = 5 rows on 256-pixel tiles for FUMI_RN_BKS=4
    for i in F.INSTANCES - F.DEFAULT_INSTANCES:
        nf, mw, bks, s = i[len("rn_conv_kernel<"):-1].split(",")
        assert (mw, bks) == ("1", "2") or (nf, mw, bks) == ("5", "2", "4")
        twin = "rn_conv_kernel<%s,%s,%s,%s>" % (nf, mw, "4" if mw == "1" else "2", s)
        assert twin in default
    assert {(F.PLANS[n]["ntap"], F.PLANS[n]["reduce"]) for n in F.WGRAD_CASES} == F.WGRAD_INSTANCES
    assert len(F.KNOB_SETTINGS) == 9 and all(set(s) <= set(F.KNOBS) for s in F.KNOB_SETTINGS)


def test_mw2_is_reached_by_default_and_both_lds_branches(hip):
    two = 80 * 1024 - 256
    m2 = [n for n in F.CONV_CASES if F.PLANS[n]["mw"] == 2]
    assert {(F.PLANS[n]["nf"], F.PLANS[n]["bks"]) for n in m2} == {(1, 4), (2, 4), (3, 4), (4, 4), (1, 2), (2, 2), (3, 2), (4, 2), (5, 2)}
    assert all(F.PLANS[n]["lds"] <= two for n in m2)
    # the fall to BKS = 2: the 4-k-step tile of the same row would not fit two workgroups
    assert all(F.PLANS[n]["lds"] + 2 * 2 * F.PLANS[n]["nf"] * 1024 > two for n in m2 if F.PLANS[n]["bks"] == 2 and F.PLANS[n]["nf"] < 5)
    assert F.PLANS["i_fall_m1"]["mw"] == 1 and (F.npix(F.CASES["i_fall_m1"]) + 255) // 256 * 4 >= 256


def test_table_holds_the_edges_it_is_there_for(hip):
    C, P = F.CASES, F.PLANS
    conv = [C[n] for n in F.CONV_CASES]
    inner = lambda c: c["M"] * c["H"] * c["W"]
    assert {127, 128, 129, 255, 256, 257} <= {inner(c) for c in conv if c["B"] == 1}
    # a last tile of one pixel on 128-pixel tiles; on 256-pixel tiles (no knob set) one pixel short of, on, and one pixel past a tile
    assert any(inner(C[n]) % 128 == 1 and inner(C[n]) > 128 and P[n]["mw"] == 1 and not P[n]["tpi"] for n in F.CONV_CASES)
    for r in (255, 0, 1):
        assert any(inner(C[n]) % 256 == r and P[n]["mw"] == 2 and not P[n]["tpi"] and P[n]["tiles"] == (inner(C[n]) + 255) // 256
                   for n in F.CONV_CASES), f"no 256-pixel-tile row with {r} pixels (mod 256)"
    assert any(C[n]["H"] * C[n]["W"] % 256 == 1 and P[n]["mw"] == 2 and P[n]["tpi"] for n in F.CONV_CASES)   # ... and per image
    # 255 and 256 pixels in all take 256-pixel tiles under FUMI_RN_MW=2 (their slabs fit two workgroups): asserted in that child
    assert all(P[n]["mw"] == 1 for n in ("t_255", "t_256", "t_257_1x1"))
    assert any((c["H"], c["W"]) == (1, 1) for c in conv) and any(c["H"] != c["W"] for c in conv)
    assert any((c["H"], c["W"]) == (5, 5) and c["M"] >= 20 for c in conv) and any((c["H"], c["W"]) == (2, 2) and c["M"] >= 50 for c in conv)
    for mt, mw in ((128, 1), (256, 2)):                                                           # both sides of rn_per_image
        rows = [n for n in F.CONV_CASES if P[n]["mw"] == mw]
        assert any(P[n]["tpi"] == 0 and 4 * mt - 4 <= C[n]["H"] * C[n]["W"] < 4 * mt for n in rows)
        assert any(P[n]["tpi"] > 0 and C[n]["H"] * C[n]["W"] >= 4 * mt for n in rows)
    p = P["p_529_img"]
    assert p["tpi"] == 5 and 529 - 4 * 128 == 17 and p["tiles"] == 10 > (F.npix(C["p_529_img"]) + 127) // 128 - 1
    cins = {s[0] for c in conv for s in c["srcs"]}
    assert {16, 32, 48, 64, 80, 96, 160, 320} <= cins
    assert {16, 48, 80} <= {s[0] for n in F.CONV_CASES if not P[n]["s16"] for s in C[n]["srcs"]}
    assert all(s[0] % 32 == 0 for c in conv if c["pass_"] == "dgrad" for s in c["srcs"])      # (32x32x16 there: FUMI_RN_S16=0)
    assert {32, 64, 96, 128, 160, 224, 320} <= {c["Cout"] for c in conv}
    assert {1, 2, 3, 4, 5} == {P[n]["nf"] for n in F.CONV_CASES} and {1, 2, 7} <= {P[n]["ncg"] for n in F.CONV_CASES}
    combos = {tuple(s[1] for s in c["srcs"]) for c in conv}
    assert {(9,), (1,), (9, 9), (9, 1), (9, 9, 1, 1)} <= combos
    assert any(len({s[2] for s in c["srcs"]}) == 2 for c in conv)                                 # shared beside per-episode weights
    mixed = [n for n in F.CONV_CASES if len({s[0] % 32 == 0 for s in C[n]["srcs"]}) == 2]
    assert mixed and all(not P[n]["s16"] for n in mixed)
    assert any(c["dot"] for c in conv) and any(c["stats"] and not c["dot"] for c in conv)
    assert {1, 3, 8, 12} <= {c["B"] for c in conv}
    assert any(P[n]["xcd"] for n in F.CONV_CASES) and any(not P[n]["xcd"] and C[n]["B"] == 12 and P[n]["ncg"] == 1 for n in F.CONV_CASES)
    assert {3, 8, 12} <= {c["B"] for c in C.values() if c["chunk"]}
    w = [C[n] for n in F.WGRAD_CASES]
    assert {9, 1} <= {c["ntaps"] for c in w} and {1, 2} <= {c["npair"] for c in w}
    assert any(c["Cin"] == 16 and c["Cin_real"] == 3 for c in w) and any(c["Cin"] == 48 for c in w) and {32, 96} <= {c["Cout"] for c in w}
    assert any(P[n]["nsplit"] == 1 for n in F.WGRAD_CASES)
    assert any(P[n]["nsplit"] > 1 and C[n]["nsplit"] == 0 and F.npix(C[n]) % (128 * P[n]["nsplit"]) for n in F.WGRAD_CASES)
    assert any(P[n]["nsplit"] > 1 and P[n]["ntap"] == 1 and P[n]["reduce"] == 1 for n in F.WGRAD_CASES)
    assert any(P[n]["nsplit"] >= 16 and P[n]["ntap"] == 1 and P[n]["reduce"] == 2 for n in F.WGRAD_CASES)
    assert any(c["chunk"] for c in w)


def test_query_refuses_what_the_launchers_refuse(hip):
    for args in ((1, 1, 4, 4, 48, [32]), (1, 1, 4, 4, 32, [24]), (1, 1, 4, 4, 32, []), (1, 1, 4, 4, 32, [32] * 5), (0, 1, 4, 4, 32, [32])):
        with pytest.raises(hip.FumiHipError, match=r"invalid argument \(-1\)"):
            hip.rn12_conv_query(*args)
    for args in ((1, 1, 4, 4, 32, 48, 9), (1, 1, 4, 4, 24, 32, 9), (1, 1, 4, 4, 32, 32, 3), (1, 1, 4, 4, 32, 32, 9, 3)):
        with pytest.raises(hip.FumiHipError, match=r"invalid argument \(-1\)"):
            hip.rn12_wgrad_query(*args)
