"""The trimmed fixed-shape reverse sweep (csrc/episode.hip, reverse_lds_kernel<true, DROP>: both stagings written out as
fixed-address loads, no G_ss staging, no last Dbar update, no second zeroing) against the run-time-shaped
kernels (FUMI_EPI_FIXED=0), at the edges of the written-out staging.

The staging gives every lane one float4 of each 64-column image (row = lane / 16, masked at S rows / N head rows), sums up to
8 tile slabs in tile order from clamped addresses, and exits for episodes past B in the last group of 8.  So the cases cover
S = 1, 5, 21, 25, 28 and 32 (32: the sweep alone is fixed-shape, the fused query layout does not fit), N = 1 (the only way to
S = 1), 2, 5, 7, 8, query sets of 1, 5 and 8 tiles with a ragged last tile, and B = 1, 7, 32.

What is compared, torch.equal, form against form: loss, accuracy and predictions of every step, and after each of two Adam
steps every `.grad` and every parameter.  The gradients of one step ARE the sweep's outputs summed over the episodes: gW_1 from
Wbar_1, gb_1 from bbar_1, gb_0 from b0bar, the head's (hypernetwork's) gradients from head_bar, gW_0 from the support and query
rows of A0bar -- so the removed Dbar update, had anything read it, would show in one of them."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CASES = {
    # name: (B, N, K, Q, dropout, fixed kernels expected: 1 = query, 2 = reverse)
    # (up to 20 support rows the sweep's layout fits LDS in 2 column parts: the run-time-shaped sweep runs, as before, because the
    # sum over the parts depends on their number; the fixed-shape query kernel runs)
    "s1_one_tile": (1, 1, 1, 3, 0.0, 1),                 # S = 1, Qn = 3
    "s5_b7_one_tile": (7, 5, 1, 6, 0.0, 1),              # S = 5, Qn = 30 (one short tile), B not a multiple of 8
    "s21_n7_b7_one_tile": (7, 7, 3, 4, 0.0, 3),          # S = 21: the fewest rows at which the sweep takes 4 parts; Qn = 28
    "s25_b32_five_tiles": (32, 5, 5, 31, 0.0, 3),        # S = 25, Qn = 155: five tiles, the last of 27 rows
    "s28_n2_eight_tiles": (7, 2, 14, 125, 0.0, 3),       # S = 28 (the fused query layout's limit), Qn = 250: eight tiles, last of 26
    "s32_n8_eight_tiles": (1, 8, 4, 31, 0.0, 2),         # S = 32: sweep only; Qn = 248: eight tiles, last of 24
    "s32_n8_b7_five_tiles": (7, 8, 4, 20, 0.0, 2),       # S = 32, Qn = 160: five whole tiles
    "s25_b7_dropout": (7, 5, 5, 6, 0.25, 3),             # the DROP instance, Qn = 30
}
STEPS = 2


def _worker(case, out):
    sys.path.insert(0, ROOT)
    from oracle import casegen as cg
    from fumi_amd import hip, optim
    from fumi_amd.models.fumi import FUMI
    B, N, K, Q, drop, _ = CASES[case]
    dev = torch.device("cuda:0")
    D, Dt = 512, 48
    torch.manual_seed(7)
    m = FUMI(n_way=N, im_emb_dim=D, im_hid_dim=[256, 64], text_encoder="BERT", text_emb_dim=Dt, text_hid_dim=64,
             dropout_rate=drop, norm_hypernet=True).to(dev)
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-4)
    args = SimpleNamespace(device=dev, num_train_adapt_steps=1, num_test_adapt_steps=1, step_size=0.05, first_order=False,
                           num_ways=N, batch_size=B)
    rec = {"losses": [], "preds": [], "forms": [], "grads": [], "params": []}
    for i in range(STEPS):
        ep = cg.make_episodes(700 + i, B, N, K, Q, D, Dt)
        loss, acc, pr, _ = m.evaluate(args, cg.to_batch(ep), opt, "train")
        rec["forms"].append(int(hip.lib().fumi_hip_epi_fixed_last()))
        rec["losses"].append(torch.tensor([float(loss), float(acc)], dtype=torch.float64))
        rec["preds"].append(pr.detach().cpu().clone())
        rec["grads"].append([p.grad.detach().cpu().clone() for p in m.parameters()])
        rec["params"].append([p.detach().cpu().clone() for p in m.parameters()])
    torch.cuda.synchronize()
    torch.save(rec, out)


def _run(case, fixed, tmp_path):
    out = str(tmp_path / f"{case}_{fixed}.pt")
    env = dict(os.environ, FUMI_EPI_FIXED=str(fixed))
    env.pop("FUMI_EPI_GLOBAL", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out)


@pytest.mark.parametrize("case", list(CASES))
def test_trimmed_sweep_is_bit_identical(case, tmp_path):
    a = _run(case, 1, tmp_path)
    b = _run(case, 0, tmp_path)
    assert a["forms"] == [CASES[case][5]] * STEPS, a["forms"]
    assert b["forms"] == [0] * STEPS, b["forms"]
    for x, y in zip(a["losses"] + a["preds"], b["losses"] + b["preds"]):
        assert torch.equal(x, y)
    assert all(torch.isfinite(x).all() for x in a["losses"])
    for step in range(STEPS):
        ga, gb = a["grads"][step], b["grads"][step]
        assert len(ga) == len(gb) > 0
        for i, (x, y) in enumerate(zip(ga, gb)):
            assert torch.equal(x, y), f"step {step}: .grad of parameter {i} differs"
        if CASES[case][1] > 1:                # (one class: the loss is 0 for every parameter value, every gradient is exactly 0)
            assert any(bool((x != 0).any()) for x in ga)
        for i, (x, y) in enumerate(zip(a["params"][step], b["params"][step])):
            assert torch.equal(x, y), f"step {step}: parameter {i} differs"


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
