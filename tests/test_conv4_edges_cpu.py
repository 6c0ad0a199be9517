"""What tests/test_conv4_edges_gpu.py relies on, checked without a GPU, so that the GPU tests cannot hide anything:
  * at every shape of the case table (tests/conv4_forms.py) and 64 channels the float64 sweep oracle/conv4_manual.py equals float64
    autograd through oracle/conv4_ref.py at the bounds of tests/test_conv4_manual.py (logits 1e-11, gradients 1e-9);
  * no episode of any case -- with the head of the per-intermediate walker / the MAML steps, and with the hypernetwork's heads of the
    FuMI step -- has more than 6 decisions within TIE_TOL of a tie: _match_episodes enumerates at most 6, so this is a condition on
    the inputs (a seed that breaks it is changed, never the cap);
  * the restated host formulas give, for every case, the chunk counts the table claims."""
import pytest
import torch
import torch.nn.functional as F

import conv4_forms as CF
from oracle import conv4_manual as M
from oracle import conv4_ref as C


def _f64(ep):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in ep.items()}


@pytest.mark.parametrize("name", list(CF.CASES))
def test_manual_sweep_equals_autograd_at_the_edge_shapes(name):
    c = CF.CASES[name]
    ep, theta, head = CF.maml_inputs(c["shape"], 1, c["N"], c["K"], c["Q"], c["seed"])
    ep, theta, head = _f64(ep), [t.double() for t in theta], head.double()
    th = [t.clone().requires_grad_(True) for t in theta]
    h0 = head.clone().requires_grad_(True)
    lq = C.episode(th, h0, ep["x_s"][0], ep["y_s"][0], ep["x_q"][0], c["T"], CF.ALPHA, False)
    loss = F.cross_entropy(lq, ep["y_q"][0])
    g = torch.autograd.grad(loss, th + [h0])
    zq, l2, bar_th, bar_h = M.episode_grads(theta, head, ep["x_s"][0], ep["y_s"][0], ep["x_q"][0], ep["y_q"][0], c["T"], CF.ALPHA, False)
    assert torch.allclose(zq, lq.detach(), rtol=0, atol=1e-11)
    assert abs(float(l2 - loss.detach())) < 1e-12
    for a, r in zip(bar_th + [bar_h], g):
        assert float((a - r).abs().max()) <= 1e-9 * max(1.0, float(r.abs().max())), (a - r).abs().max()


def _ties(theta, heads, ep, T):
    th = [t.double() for t in theta]
    out = []
    for b in range(ep["x_s"].shape[0]):
        tr = {}
        M.episode_grads(th, heads[b].double(), ep["x_s"][b].double(), ep["y_s"][b], ep["x_q"][b].double(), ep["y_q"][b], T, CF.ALPHA,
                        True, trace=tr)                  # (the decisions are those of the forward passes: the order does not matter)
        out.append(len(M.ambiguous_decisions(tr, CF.TIE_TOL, limit=100)))
    return out


@pytest.mark.parametrize("name", list(CF.CASES))
def test_near_tie_decisions_stay_within_what_the_matcher_enumerates(name):
    c = CF.CASES[name]
    ep, theta, head = CF.maml_inputs(c["shape"], c["B"], c["N"], c["K"], c["Q"], c["seed"])
    n = _ties(theta, head[None].expand(c["B"], -1, -1), ep, c["T"])
    assert max(n) <= CF.MAX_TIES, n
    if name == "A":                                      # the FuMI whole step of case A (tanh on the hypernetwork's output)
        ep, theta, phi = CF.fumi_inputs(name)
        heads, _ = CF.fumi_heads(ep, phi, c["N"], True)
        n = _ties(theta, heads.detach(), ep, c["T"])
        assert max(n) <= CF.MAX_TIES, n


@pytest.mark.parametrize("name", list(CF.CASES))
def test_cases_reach_the_edges_they_are_named_for(name):
    CF.case_reaches_its_edge(name)


def test_restated_host_formulas():
    """Values worked out by hand from csrc/conv_first.hip and csrc/conv_ew.hip."""
    assert CF.c1_chunks(16, 6, 21) == (2, 33, 11)           # 66 bands over ceil(1024 / 16) = 64 workgroups -> 2 bands each, 33 used
    assert CF.c1_chunks(16, 9, 21) == (2, 50, 11)           # 99 bands -> 2 each, 50 workgroups (the last one walks a single band)
    assert CF.c1_chunks(2, 9, 9) == (1, 45, 5)              # small shapes: one band per workgroup
    assert CF.c1_chunks(32, 160, 84) == (210, 32, 42)       # bench shape, one lane: 6720 bands over 32 workgroups
    assert CF.coef_chunks(9, 29, 31) == 2                   # 9 x 31 x 33 = 9207 padded pixels = 72 tiles = 64 + 8
    assert CF.coef_chunks(9, 21, 23) == 1                   # 5175 pixels = 41 tiles
    assert CF.coef_chunks(64, 9, 14) == 2                   # 64 x 11 x 16 = 11264 = 88 tiles exactly
