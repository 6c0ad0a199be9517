"""What tests/test_front_forms_gpu.py relies on, checked without a GPU, so that the GPU tests cannot hide anything:
  * every case of tests/front_forms.py reaches the branch it is named for, by the restated host geometry (change a case's E, L, S,
    row_f or index count so that it no longer does and this file fails);
  * the float64 bag reference equals oracle.fumi_ref.word_embedding_pool in float64; a plain float32 accumulation in index order stays
    within HALF of the mean's bound on every case; the mean that skips PAD tokens is more than 100 bounds away from the right one;
  * the float64 reference of the bare linear MAML head (oracle.fumi_ref.maml_meta_step, autograd) equals the autograd-free restatement
    of csrc/linhead.hip's algebra to 1e-10 on every case, and NO query row of any case lies under the 1e-5 prediction margin, so the
    GPU test sets no row aside."""
import numpy as np
import pytest
import torch

import front_forms as FF
from oracle import fumi_ref as R


# ---- embedding bag -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FF.BAG_CASES))
def test_bag_cases_reach_the_edges_they_are_named_for(name):
    FF.bag_case_reaches_its_edge(name)


def test_restated_bag_geometry():
    """Values worked out by hand from csrc/glove.hip (bag_geometry) and csrc/glove_bag.h."""
    g = FF.bag_geometry(300, 128)                       # the bench shape: 75 float4 -> 2 chunks, one pair pass
    assert (g["vec"], g["nchunk"], g["Ep"], g["lds"], g["lw"], g["pair_passes"], g["single_pass"]) == (True, 2, 512, 16416, 16, 1, 0)
    g = FF.bag_geometry(300, 600)
    assert g["ntok"] == [75] * 8 and g["reloads"] == [2] * 8 and g["last_nl"] == [11] * 8
    g = FF.bag_geometry(130, 20)                        # scalar: 130 floats -> 3 chunks of 64
    assert (g["vec"], g["nchunk"], g["Ep"], g["lds"]) == (False, 3, 192, (8 * 192 + 8) * 4)
    assert FF.bag_geometry(300, 20, aligned=False)["nchunk"] == 5
    assert FF.bag_geometry(12, 3)["ntok"] == [1, 1, 1, 0, 0, 0, 0, 0]
    # 8 Ep + 8 floats > 16384 floats  <=>  Ep >= 2048: scalar E > 1984, vector E / 4 > 448
    assert FF.smallest_refused_E(False) == 1985 and FF.smallest_refused_E(True) == 1796
    assert FF.largest_accepted_E(False) == 1983 and FF.largest_accepted_E(True) == 1792
    assert FF.bag_geometry(1985, 4)["lds"] == (8 * 2048 + 8) * 4 and FF.bag_geometry(1792, 4)["lds"] == (8 * 1792 + 8) * 4


@pytest.mark.parametrize("name", list(FF.BAG_CASES))
def test_bag_reference_and_its_bound(name):
    tok, table = FF.bag_inputs(name)
    lw = FF.bag_case_geometry(name)["lw"]
    t64 = torch.from_numpy(table).double()
    with np.errstate(all="ignore"):
        for mode in ("mean", "max"):
            ref, bound = FF.bag_reference(tok, table, mode, lw)
            want = R.word_embedding_pool(torch.from_numpy(tok), t64, FF.PAD, mode).numpy()
            assert np.allclose(ref, want, rtol=1e-15, atol=0, equal_nan=True), (name, mode)
    live = (tok != FF.PAD).sum(1) > 0
    assert live.sum() >= FF.BAG_R - 1
    err = np.abs(FF.bag_fp32_in_index_order(tok, table)[live].astype(np.float64) - ref_mean(tok, table, lw)[0][live])
    ratio = float((err / ref_mean(tok, table, lw)[1][live]).max())
    print(f"bag {name}: float32 in index order, largest error / bound = {ratio:.3f}")
    assert ratio <= 0.5, (name, ratio)
    # a kernel that skipped PAD tokens: wrong by more than 100 bounds in every element of every row that has a PAD token and a
    # non-PAD one, except the column where the PAD row is 0
    skip, _ = FF.bag_reference(tok, table, "mean", lw, skip_pad=True)
    right, bound = ref_mean(tok, table, lw)
    rows = live & ((tok == FF.PAD).sum(1) > 0)
    cols = table[FF.PAD] != 0
    assert rows.sum() >= 3 and cols.sum() == table.shape[1] - 1
    far = np.abs(skip - right)[rows][:, cols] / bound[rows][:, cols]
    print(f"bag {name}: the PAD-skipping mean is at least {far.min():.0f} bounds away")
    assert far.min() > 100.0, (name, far.min())


def ref_mean(tok, table, lw):
    with np.errstate(all="ignore"):
        return FF.bag_reference(tok, table, "mean", lw)


def test_all_pad_row_divides_by_zero_as_the_reference_does():
    tok, table = FF.bag_inputs("all_pad_row")
    r = int(np.nonzero((tok != FF.PAD).sum(1) == 0)[0][0])
    out = ref_mean(tok, table, 16)[0][r]
    assert np.isnan(out[1]) and np.isinf(np.delete(out, 1)).all() and (np.sign(np.delete(out, 1)) == np.sign(np.delete(table[FF.PAD], 1))).all()
    want = R.word_embedding_pool(torch.from_numpy(tok), torch.from_numpy(table), FF.PAD, "mean").numpy()[r]       # the fp32 reference
    assert np.array_equal(np.isnan(want), np.isnan(out)) and np.array_equal(want[~np.isnan(want)], out[~np.isnan(out)].astype(np.float32))


def test_select_labels_reach_both_ballot_passes():
    FF.select_reaches_its_edge()
    y, (b, c) = FF.select_missing_labels()
    assert (y[b] == c).sum() == 0 and all((y[e] == k).any() for e in range(FF.SEL_B) for k in range(FF.SEL_N) if (e, k) != (b, c))
    for E in (50, 300):
        tok, _ = FF.select_bag_inputs(E)
        _, first = FF.select_labels()
        rows = tok[np.arange(FF.SEL_B)[:, None], first]                  # the selected token rows differ from every other support row
        for e in range(FF.SEL_B):
            for k in range(FF.SEL_N):
                same = (tok[e] == rows[e, k]).all(-1)
                assert same.sum() == 1 and same[first[e, k]]


# ---- row gather ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FF.GATHER_CASES))
def test_gather_cases_reach_the_edges_they_are_named_for(name):
    g = FF.gather_case_reaches_its_edge(name)
    table, idx = FF.gather_inputs(name)
    assert set(idx.tolist()) == set(range(table.shape[0])) or len(idx) < table.shape[0]
    assert np.unique(table).size == table.size
    if name == "grid_wraps":
        assert g["blocks"] * 4 < len(idx) <= g["blocks"] * 8              # the loop's second trip, and only for some waves


def test_restated_gather_geometry():
    """Values worked out by hand from csrc/sampler.hip."""
    g = FF.gather_geometry(2048, 513)                    # the shape every earlier test used: one pass, 129 workgroups, no wrap
    assert (g["vec"], g["n4"], g["passes"], g["last_live"], g["blocks"], g["wraps"]) == (True, 512, 1, 512, 129, False)
    g = FF.gather_geometry(2052, 9)
    assert (g["n4"], g["passes"], g["last_live"], g["blocks"]) == (513, 2, 1, 3)
    assert FF.gather_geometry(4100, 6)["passes"] == 3
    assert FF.gather_geometry(8, 16384)["wraps"] is False and FF.gather_geometry(8, 16385)["wraps"] is True
    assert FF.gather_geometry(8, 21, aligned=False)["vec"] is False and FF.gather_geometry(1, 21)["vec"] is False


# ---- bare linear MAML head -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FF.LIN_CASES))
def test_linhead_cases_reach_the_edges_they_are_named_for(name):
    FF.linhead_case_reaches_its_edge(name)


def test_restated_linhead_lds_floats():
    """Worked out by hand from csrc/linhead.hip.  N = 20, S = 100, Qn = 20: 6000 + 60 + 16 + 2000 = 8076 floats plus 2000 a taped step:
    T = 14 is 36076 (fits under 38000), T = 15 is 38076 (refused); first order never tapes."""
    assert FF.linhead_lds_floats(20, 100, 20, 14, True) == 36076
    assert FF.linhead_lds_floats(20, 100, 20, 15, True) == 38076 > FF.LINHEAD_LIMIT
    assert FF.linhead_lds_floats(20, 100, 20, 15, False) == 8076
    assert FF.linhead_lds_floats(4, 20, 4, 3, True) == 3 * 80 + 12 + 16 + 80 + 240
    assert FF.linhead_lds_floats(2, 2, 300, 1, True) == 12 + 6 + 16 + 600 + 4


@pytest.mark.parametrize("name", list(FF.LIN_CASES))
def test_linhead_reference_equals_the_autograd_free_restatement(name):
    c, ref = FF.LIN_CASES[name], FF.lin_reference(name)
    zq, loss_b, gW, gb = FF.lin_manual(c)
    assert float((zq - ref["logits"]).abs().max()) <= 1e-10
    assert float((loss_b - ref["loss_b"]).abs().max()) <= 1e-10
    for a, r in ((gW, ref["g_params"][0]), (gb, ref["g_params"][1])):
        assert float((a - r).abs().max()) <= 1e-10 * max(1.0, float(r.abs().max())), name
    top2 = ref["logits"].topk(2, dim=-1)[0]
    margin = float((top2[..., 0] - top2[..., 1]).min())
    print(f"linhead {name}: smallest top-two margin {margin:.2e}")
    assert margin > FF.MARGIN, (name, margin)             # a seed that breaks this is changed, never the margin
    if c["T"] == 0:                                      # no inner step: the logits are X W^T + b
        ep, p = FF.lin_inputs(c)
        assert float((ref["logits"] - (ep["x_q"].double() @ p[0].double().t() + p[1].double())).abs().max()) <= 1e-12
    if c["fo"] and c["T"] > 0:                           # first order: gW comes from the query rows alone
        ep, _ = FF.lin_inputs(c)
        lbar = (torch.softmax(ref["logits"], -1) - torch.eye(c["N"], dtype=torch.float64)[ep["y_q"]]) / (c["N"] * c["Q"])
        gq = torch.einsum("bqn,bqd->nd", lbar, ep["x_q"].double()) / c["B"]
        assert float((gq - ref["g_params"][0]).abs().max()) <= 1e-10


def test_orders_agree_without_an_inner_step_and_differ_with_one():
    a, b = FF.lin_reference("no_inner_step_second_order"), FF.lin_reference("no_inner_step_first_order")
    assert all(torch.equal(x, y) for x, y in zip(a["g_params"], b["g_params"]))
    a, b = FF.lin_reference("S_above_Qn_second_order"), FF.lin_reference("S_above_Qn_first_order")
    assert torch.equal(a["logits"], b["logits"])
    rel = float((a["g_params"][0] - b["g_params"][0]).abs().max() / a["g_params"][0].abs().max())
    assert rel > 100 * FF.GRAD_TOL, rel                   # the second-order terms are far above the gradient tolerance
