"""The text-rows form of the AM3 step (csrc/am3.hip: fumi_hip_am3_step_tx; DESIGN.md "AM3 text-rows form") -- TEST INFRASTRUCTURE ONLY,
shared by tests/test_am3_rand_host.py and tests/test_am3_rand_gpu.py.

The case table, the device draw restated on the host, and the float64 oracle: ``oracle.fumi_ref.am3_step`` (unchanged) with an exact
identity in g's place at the oracle's own hidden width 2P (x = relu(x) - relu(-x): every sum has one non-zero term, so tx is the
rows bit for bit in any precision) and masks = (ones, h's mask)."""
import functools
from collections import OrderedDict

import numpy as np
import torch

import am3_forms as F
from helpers import _mix, dropout_mask_flat
from oracle import casegen as cg
from oracle import fumi_ref as R

SEED = 0x0BADC0DE12345678          # the step's seed: h's dropout mask (tag 2) and the drawn rows (tag 3)
SEED_B = 0x1122334455667788


def _c(B, N, K, Q, D, Ht, P, lamda_fixed=None, dropout=0.0, ragged=False, ep_seed=0):
    return dict(B=B, N=N, K=K, Q=Q, D=D, Ht=Ht, P=P, lamda_fixed=lamda_fixed, dropout=dropout, ragged=ragged, ep_seed=ep_seed)


# the smallest shape at which each path can go wrong
CASES = OrderedDict([
    ("fused", _c(3, 5, 2, 3, 64, 128, 64, dropout=0.25, ep_seed=7101)),           # fused h forward / backward, fast head
    # Ht < 2P, Ht no multiple of 64 (GEMM fallback), P at the fast head's limit
    ("published", _c(2, 5, 1, 2, 48, 300, 512, dropout=0.5, ep_seed=7102)),
    ("small_p", _c(2, 9, 1, 2, 40, 20, 16, ragged=True, ep_seed=7103)),           # tiny P, odd N, ragged class counts, no mask
    ("lamda0", _c(2, 5, 2, 3, 64, 128, 64, lamda_fixed=0, dropout=0.25, ep_seed=7104)),   # h out of the graph
    ("lamda1", _c(2, 5, 2, 3, 64, 128, 64, lamda_fixed=1, dropout=0.25, ep_seed=7104)),
])
FORMS = ("given", "drawn")


def draw_key(seed, tag):
    """dkey(tag) of csrc/am3.hip for a 64-bit seed."""
    lo, hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    one = lambda v: _mix(np.array([v & 0xFFFFFFFF], dtype=np.uint64))[0]
    return int(one(int(one(lo ^ ((0x9E3779B9 * tag) & 0xFFFFFFFF))) ^ hi))


def draw_rows(seed, rows, P):
    """The device draw (am3_draw_rows_kernel): element e = row * P + col is (float)(mix(dkey(3) ^ (uint32)e) >> 8) * 2^-23 - 1."""
    e = np.arange(rows * P, dtype=np.uint64) & 0xFFFFFFFF
    u = _mix((np.uint64(draw_key(seed, 3)) ^ e) & 0xFFFFFFFF)
    v = (u >> 8).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    return torch.from_numpy(v.reshape(rows, P))


def identity_g(P, dtype=torch.float32):
    """g's four tensors at hidden width 2P: G0 = [I; -I], G1 = [I, -I], zero biases."""
    eye = torch.eye(P, dtype=dtype)
    return torch.cat([eye, -eye], 0), torch.zeros(2 * P, dtype=dtype), torch.cat([eye, -eye], 1), torch.zeros(P, dtype=dtype)


def make_inputs(name, form, seed=SEED):
    """(case, episodes with ``rows`` [B,S,P], weights dict with the identity in g's place, masks or None)"""
    c = CASES[name]
    B, S, P, Ht = c["B"], c["N"] * c["K"], c["P"], c["Ht"]
    ep = cg.make_episodes(c["ep_seed"], B, c["N"], c["K"], c["Q"], c["D"], P)
    if c["ragged"]:
        ep = F.make_ragged(c["ep_seed"], ep, c["N"], P)
    if form == "given":
        rs = np.random.RandomState(c["ep_seed"] + 1)
        rows = torch.from_numpy(rs.uniform(-1.0, 1.0, size=(B, S, P)).astype(np.float32))
    else:
        rows = draw_rows(seed, B * S, P).reshape(B, S, P)
    ep = dict(ep, rows=rows)
    w = dict(cg.make_am3_params(c["ep_seed"], c["D"], P, Ht, P))
    w["G0"], w["g0"], w["G1"], w["g1"] = identity_g(P)
    masks = None
    if c["dropout"] > 0:
        masks = (torch.ones(B * S, 2 * P), dropout_mask_flat(seed, c["dropout"], 2, B * S, Ht))
    return c, ep, w, masks


@functools.lru_cache(maxsize=None)
def reference(name, form):
    """Inputs, float64 oracle and safe rows of a case: computed once, shared by every test, never modified."""
    c, ep, w, masks = make_inputs(name, form)
    ref = F.run_oracle(c, dict(ep, text_s=ep["rows"]), w, masks, torch.float64)
    assert torch.equal(ep["rows"].to(torch.float64), _oracle_tx(ep, w))               # the identity is exact
    return c, ep, w, ref, F.safe_rows(ref["dist"], ep["y_s"], c["N"])


def _oracle_tx(ep, w):
    x = ep["rows"].to(torch.float64)
    return torch.relu(x @ w["G0"].to(torch.float64).t()) @ w["G1"].to(torch.float64).t()


G_KEYS = ("G0", "g0", "G1", "g1")


def zero_grads(c):
    """Gradients that are exactly zero in the engine (am3_forms.zero_grads without g, which this form never writes)."""
    return F.zero_grads(c) - set(G_KEYS)


def cancelling_sums(name, form):
    """{key: scale} for gradients that are zero analytically but NOT exactly zero in fp32, with the scale that stands in for the
    tensor's own maximum (which is 0).

    lamda fixed at 1 with a support row in every class: every prototype is a mean of image embeddings, so adding a constant to bi
    moves prototypes and queries alike, no distance changes and d loss / d bi = colsum(imbar) = 0.  The engine forms that column sum
    from non-zero adjoints imbar; the test grants every adjoint GRAD_TOL of its scale, so their sum can be off by GRAD_TOL times the
    sum of their magnitudes -- the largest column of sum_rows |imbar| (float64, from the oracle's own functions) is the scale."""
    c, ep, w, ref, (_, _, empty, _) = reference(name, form)
    if c["lamda_fixed"] != 1 or bool(empty.any()):
        return {}
    d = torch.float64
    im_s = torch.nn.functional.linear(ep["x_s"].to(d), w["Wi"].to(d), w["bi"].to(d)).requires_grad_(True)
    im_q = torch.nn.functional.linear(ep["x_q"].to(d), w["Wi"].to(d), w["bi"].to(d)).requires_grad_(True)
    lam = torch.ones(c["B"], c["N"] * c["K"], 1, dtype=d)
    loss = R.prototypical_loss(R.get_prototypes(im_s, ep["rows"].to(d), lam, ep["y_s"], c["N"]), im_q, ep["y_q"])
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-12 * max(1.0, abs(float(ref["loss"])))
    bar_s, bar_q = torch.autograd.grad(loss, [im_s, im_q])
    scale = float((bar_s.abs().sum((0, 1)) + bar_q.abs().sum((0, 1))).max())
    assert float(ref["all_grads"]["bi"].abs().max()) <= 1e-12 * scale          # the oracle's own sum: zero to float64 round-off
    return {"bi": scale}
