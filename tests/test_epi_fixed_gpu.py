"""The per-episode chain compiled for the reference shape (csrc/episode.hip: query_lds_kernel<true, true, DROP>,
reverse_lds_kernel<true, DROP>) against the run-time-shaped kernels it replaces (FUMI_EPI_FIXED=0).

The fixed-shape instances run the same code with the dimensions, flags and LDS layout folded to constants, so every product keeps
its accumulation order: several FuMI meta-steps with Adam must agree BIT FOR BIT in the losses, the predictions, every `.grad` and
every parameter after the step (then one evaluation step in the same process).  The knob is read once per process, so each form runs in a subprocess of its own."""
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CASES = {
    # name: (B, N, K, Q, dropout, inner steps T, fixed kernels expected: 1 = query, 2 = reverse)
    "bench_shape": (32, 5, 5, 32, 0.0, 1, 3),
    "s32_n8": (8, 8, 4, 4, 0.0, 1, 2),                  # S = 32: the fused query layout does not fit -> adapt + run-time query
    "ragged_tile": (6, 5, 5, 3, 0.0, 1, 3),              # Qn = 15: one short query tile
    "dropout": (8, 5, 5, 8, 0.25, 1, 3),
    "two_steps": (8, 5, 5, 8, 0.0, 2, 0),                # T = 2: the dispatch falls back (FuMI's meta-step is always second order)
}


def _worker(case, out):
    sys.path.insert(0, ROOT)
    from oracle import casegen as cg
    from fumi_amd import hip, optim
    from fumi_amd.models.fumi import FUMI
    B, N, K, Q, drop, T, _ = CASES[case]
    dev = torch.device("cuda:0")
    D, Dt = 512, 48
    torch.manual_seed(5)
    m = FUMI(n_way=N, im_emb_dim=D, im_hid_dim=[256, 64], text_encoder="BERT", text_emb_dim=Dt, text_hid_dim=64,
             dropout_rate=drop, norm_hypernet=True).to(dev)
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-4)
    args = SimpleNamespace(device=dev, num_train_adapt_steps=T, num_test_adapt_steps=T, step_size=0.05, first_order=False,
                           num_ways=N, batch_size=B)
    losses, preds, forms = [], [], []
    for i in range(3):
        ep = cg.make_episodes(300 + i, B, N, K, Q, D, Dt)
        loss, acc, pr, _ = m.evaluate(args, cg.to_batch(ep), opt, "train")
        forms.append(int(hip.lib().fumi_hip_epi_fixed_last()))
        losses.append(torch.tensor([float(loss), float(acc)], dtype=torch.float64))
        preds.append(pr.detach().cpu().clone())
    # an evaluation step in the same process (no gradient: the run-time-shaped kernels) after the fixed-shape training steps
    ep = cg.make_episodes(400, B, N, K, Q, D, Dt)
    loss, acc, pr, _ = m.evaluate(args, cg.to_batch(ep), opt, "test")
    forms.append(int(hip.lib().fumi_hip_epi_fixed_last()))
    losses.append(torch.tensor([float(loss), float(acc)], dtype=torch.float64))
    preds.append(pr.detach().cpu().clone())
    torch.cuda.synchronize()
    torch.save({"losses": losses, "preds": preds, "forms": forms,
                "params": [p.detach().cpu().clone() for p in m.parameters()],
                "grads": [p.grad.detach().cpu().clone() for p in m.parameters()]}, out)


def _run(case, fixed, tmp_path):
    out = str(tmp_path / f"{case}_{fixed}.pt")
    env = dict(os.environ, FUMI_EPI_FIXED=str(fixed))
    env.pop("FUMI_EPI_GLOBAL", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case, out], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out)


@pytest.mark.parametrize("case", list(CASES))
def test_fixed_shape_chain_is_bit_identical(case, tmp_path):
    a = _run(case, 1, tmp_path)
    b = _run(case, 0, tmp_path)
    assert a["forms"] == [CASES[case][6]] * 3 + [0], a["forms"]
    assert b["forms"] == [0] * 4, b["forms"]
    for x, y in zip(a["losses"] + a["preds"], b["losses"] + b["preds"]):
        assert torch.equal(x, y)
    assert len(a["grads"]) == len(b["grads"]) > 0
    for x, y in zip(a["grads"] + a["params"], b["grads"] + b["params"]):
        assert torch.equal(x, y)
    assert all(torch.isfinite(x).all() for x in a["losses"])


if __name__ == "__main__":
    _worker(sys.argv[1], sys.argv[2])
