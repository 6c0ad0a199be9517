"""The trimmed fixed-shape query kernel (csrc/episode.hip, query_lds_kernel<true, true, DROP>: staging loads in front of the arena
clear, a_0 = relu(A0_s + b_0) from the staging registers, the head's backward products in one phase with zbar_1 in the image of
D_1, the Abar0 rows stored by the epilogue of zbar_0, second clears only of rows nr .. S - 1) against the
run-time-shaped kernels (FUMI_EPI_FIXED=0), at the edges of what changed.

One training meta-step per case, D = 64.  The cases: S = 1, 5, 27 and 28 (28 is the fixed query layout's cap; 32 must fall back
to the run-time-shaped query kernel and say so), N = 1, 3, 4, 5 and 8, one tile of 15 rows, five tiles with a ragged last one
(Qn = 150: 22 rows, fewer than S = 25 and no multiple of 4, so the left-over clears and the K padding rows of the zbar_1 image
are exercised), eight tiles (Qn = 256), Qn = 32 (tile 0 is the only tile and writes all of the tape) and Qn = 33 (tile 1 has one
row), B = 1, 7 and 32, dropout 0 and 0.25.

What is compared, torch.equal, form against form: loss, accuracy, predictions, every `.grad` and every parameter after the
optimizer step.  fumi_hip_epi_fixed_last() says which form of the query kernel ran (bit 1)."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CASES = {
    # name: (B, N, K, Q, dropout, fixed-shape query kernel expected)
    "s1_n1_one_tile_b1": (1, 1, 1, 15, 0.0, True),                # S = 1: a single-row inner step; Qn = 15
    "s5_n5_one_tile_b7": (7, 5, 1, 3, 0.0, True),                 # S = 5, Qn = 15
    "s25_n5_five_tiles_ragged_b32": (32, 5, 5, 30, 0.0, True),    # Qn = 150: five tiles, the last of 22 rows (< S)
    "s27_n3_qn33_b7": (7, 3, 9, 11, 0.0, True),                   # Qn = 33: tile 1 has one row
    "s28_n4_eight_tiles_b1": (1, 4, 7, 64, 0.0, True),            # S = 28 (the cap), Qn = 256: eight whole tiles
    "s24_n8_qn32_dropout_b32": (32, 8, 3, 4, 0.25, True),         # Qn = 32: tile 0 is the only tile; the DROP instance
    "s25_n5_five_tiles_dropout_b7": (7, 5, 5, 30, 0.25, True),    # the DROP instance over five tiles
    "s32_n8_falls_back": (7, 8, 4, 4, 0.0, False),                # S = 32: over the fused layout's cap, the run-time-shaped form
}


def _worker(case, out):
    sys.path.insert(0, ROOT)
    from oracle import casegen as cg
    from fumi_amd import hip, optim
    from fumi_amd.models.fumi import FUMI
    B, N, K, Q, drop, _ = CASES[case]
    dev = torch.device("cuda:0")
    D, Dt = 64, 48
    torch.manual_seed(11)
    m = FUMI(n_way=N, im_emb_dim=D, im_hid_dim=[256, 64], text_encoder="BERT", text_emb_dim=Dt, text_hid_dim=64,
             dropout_rate=drop, norm_hypernet=True).to(dev)
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-4)
    args = SimpleNamespace(device=dev, num_train_adapt_steps=1, num_test_adapt_steps=1, step_size=0.05, first_order=False,
                           num_ways=N, batch_size=B)
    ep = cg.make_episodes(900, B, N, K, Q, D, Dt)
    loss, acc, pr, _ = m.evaluate(args, cg.to_batch(ep), opt, "train")
    rec = {"form": int(hip.lib().fumi_hip_epi_fixed_last()),
           "loss": torch.tensor([float(loss), float(acc)], dtype=torch.float64),
           "preds": pr.detach().cpu().clone(),
           "grads": [p.grad.detach().cpu().clone() for p in m.parameters()],
           "params": [p.detach().cpu().clone() for p in m.parameters()]}
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
def test_trimmed_query_kernel_is_bit_identical(case, tmp_path):
    a = _run(case, 1, tmp_path)
    b = _run(case, 0, tmp_path)
    assert bool(a["form"] & 1) == CASES[case][5], a["form"]       # the fixed-shape query kernel ran (or fell back, S = 32)
    assert b["form"] == 0, b["form"]
    assert torch.isfinite(a["loss"]).all()
    assert torch.equal(a["loss"], b["loss"])
    assert torch.equal(a["preds"], b["preds"])
    assert len(a["grads"]) == len(b["grads"]) > 0
    for i, (x, y) in enumerate(zip(a["grads"], b["grads"])):
        assert torch.equal(x, y), f".grad of parameter {i} differs"
    if CASES[case][1] > 1:                    # (one class: the loss is 0 for every parameter value, every gradient is exactly 0)
        assert any(bool((x != 0).any()) for x in a["grads"])
    for i, (x, y) in enumerate(zip(a["params"], b["params"])):
        assert torch.equal(x, y), f"parameter {i} differs"


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
