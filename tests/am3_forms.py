"""The AM3 form table shared by tests/test_am3_forms_cpu.py and tests/test_am3_forms_gpu.py -- TEST INFRASTRUCTURE ONLY.

One row per form of ``am3_step_impl`` (csrc/am3.hip; DESIGN.md "AM3 form tree"): the smallest shape that reaches it, the inputs
(oracle/casegen.py, plus ragged labels), the float64 oracle (oracle/fumi_ref.py: am3_step) and the rule that decides on which query
rows the integer prediction has to be bit-exact.  The expected plan of a row is what the dispatch rules of am3_step_impl give for
its shape with no knob set; ``expected_plan`` restates the four knobs on top of it."""
import os
from collections import OrderedDict

import numpy as np
import torch

from oracle import casegen as cg
from oracle import fumi_ref as R

LOGIT_TOL = 1e-4          # loss: x max(1, |loss|)              (tests/test_hip_parity.py)
LAMDA_TOL = 1e-5
GRAD_TOL = 1e-4           # every gradient tensor at its OWN maximum (helpers.rel_to_max, floored at helpers.FLOOR only)
MARGIN = 1e-4             # x max(1, d2): the AM3 margin between the two nearest prototypes (tests/test_hip_parity.py)
SAFE_SHARE = 0.95

H_KEYS = ("H0", "h0", "H1", "h1")
R_KEYS = ["Wi", "bi", "G0", "g0", "G1", "g1", "H0", "h0", "H1", "h1"]            # = fumi_amd.hip.AM3_KEYS (no GPU library needed here)


def _c(B, N, K, Q, D, Dt, Ht, P, ragged=False, lamda_fixed=None, dropout=0.0, **plan):
    return dict(B=B, N=N, K=K, Q=Q, D=D, Dt=Dt, Ht=Ht, P=P, ragged=ragged, lamda_fixed=lamda_fixed, dropout=dropout, plan=plan)


def _p(fast_head, nwaves, hgq=1, imparts=1, xks=1, g_fwd_split=0, g_fwd_rode=0, h_fwd_split=0, h_bwd_fused=0, g_bwd_fused=0,
       tx_nparts=0):
    return dict(fast_head=fast_head, nwaves=nwaves, hgq=hgq, imparts=imparts, xks=xks, g_fwd_split=g_fwd_split,
                g_fwd_rode=g_fwd_rode, h_fwd_split=h_fwd_split, h_bwd_fused=h_bwd_fused, g_bwd_fused=g_bwd_fused, tx_nparts=tx_nparts)


# name -> shape, labels, and the plan of the default process (no knob set).  Seeds are 4000 + the row's index.
CASES = OrderedDict([
    # one class, P = 1: the soft-max over one class is 1, every gradient is exactly zero
    ("n1", _c(1, 1, 1, 3, 32, 8, 8, 1, **_p(1, 16))),
    # a second pass of 8 classes that holds one class (seven clamped duplicates); D % 32 != 0
    ("n9_p16", _c(3, 9, 2, 3, 72, 20, 24, 16, **_p(1, 16))),
    # three class passes, two chunks of P with the second cut at 6 lanes, B no multiple of 8, many classes without a support row;
    # 2 query shares of 17 rows: one row beyond a pass of the 16 waves
    ("n17_p70", _c(9, 17, 1, 2, 130, 12, 40, 70, ragged=True, **_p(1, 16, hgq=2))),
    # N = 64: 16 waves at the LDS edge (148416 of 153600 bytes), 4 query shares of one row per wave
    ("n64_p24", _c(2, 64, 1, 1, 64, 16, 64, 24, **_p(1, 16, hgq=4, g_fwd_split=1, g_fwd_rode=1, h_fwd_split=1, h_bwd_fused=1, g_bwd_fused=1,
                                                    tx_nparts=1))),
    # 8 waves (16 would take 191936 bytes of LDS), 8 query shares; lamda fixed at 1 (the h network's gradients are memset)
    ("n64_p32", _c(2, 64, 1, 2, 64, 16, 64, 32, ragged=True, lamda_fixed=1,
                   **_p(1, 8, hgq=8, g_fwd_split=1, g_fwd_rode=1, g_bwd_fused=1))),
    # 4 waves (8 would not fit), 8 query shares of 2 rows per wave
    ("n64_p48", _c(1, 64, 1, 1, 96, 16, 32, 48, **_p(1, 4, hgq=8))),
    # the fast head does not fit LDS even with 4 waves: generic head
    ("n64_p64", _c(2, 64, 1, 1, 64, 16, 32, 64, **_p(0, 4))),
    # generic head by N > 64
    ("n65_p8", _c(2, 65, 1, 1, 64, 16, 32, 8, ragged=True, **_p(0, 4))),
    # P = 512: all 8 register chunks; g on the GEMMs in both directions (forward: P > 128, Dt > 768; backward: its [P, 64] weight chunk
    # does not fit LDS) while h's forward is split and its backward fused
    ("n2_p512", _c(9, 2, 1, 5, 128, 800, 64, 512, **_p(1, 16, h_fwd_split=1, h_bwd_fused=1))),
    # generic head by P > 512, the 2-part encoder contraction reduced by the X-panel launch; lamda fixed at 0; g on the GEMMs
    ("n3_p513", _c(2, 3, 2, 4, 512, 24, 64, 513, ragged=True, lamda_fixed=0, **_p(0, 4, xks=2))),
    # fast head adding 4 encoder parts where it reads, at a ragged P; the txbar hand-over in 2 parts
    ("n5_p100_d1024", _c(2, 5, 3, 7, 1024, 300, 128, 100, ragged=True,
                         **_p(1, 16, hgq=2, imparts=4, xks=4, g_fwd_split=1, g_fwd_rode=1, h_fwd_split=1, h_bwd_fused=1, g_bwd_fused=1,
                              tx_nparts=2))),
    # natural 4 query shares of 17,17,17,14 rows; P = 128 and Dt = 768: the edges of the fused MLP forms
    ("n5_p128_ht128", _c(10, 5, 5, 13, 512, 768, 128, 128,
                         **_p(1, 16, hgq=4, imparts=2, xks=2, g_fwd_split=1, g_fwd_rode=1, h_fwd_split=1, h_bwd_fused=1,
                              g_bwd_fused=1, tx_nparts=2))),
    # 20-way, natural 8 query shares, Ht = 320; 8 waves (16 would take 155408 bytes of LDS)
    ("n20_p64_q8", _c(5, 20, 5, 8, 256, 52, 320, 64, ragged=True,
                      **_p(1, 8, hgq=8, imparts=1, xks=1, g_fwd_split=1, g_fwd_rode=1, h_fwd_split=1, h_bwd_fused=1, g_bwd_fused=1,
                           tx_nparts=5))),
])
# the fused MLP forms have to index the dropout mask like the GEMM epilogue does
DROPOUT_CASES = OrderedDict([
    ("n5_p128_ht128_drop25", dict(CASES["n5_p128_ht128"], dropout=0.25, base="n5_p128_ht128")),
    ("n9_p16_drop50", dict(CASES["n9_p16"], dropout=0.5, base="n9_p16")),
])
ALL_CASES = OrderedDict(list(CASES.items()) + list(DROPOUT_CASES.items()))
DROPOUT_SEED = 0x1234567089ABCDEF

KNOBS = ("FUMI_AM3_GENERIC", "FUMI_AM3_GQ", "FUMI_AM3_MLP", "FUMI_XP_KSPLIT")
# the settings the GPU file re-runs its table under, one child process each (the knobs are read once per process)
KNOB_SETTINGS = [("FUMI_AM3_GENERIC", "1"), ("FUMI_AM3_GQ", "3"), ("FUMI_AM3_GQ", "16"), ("FUMI_AM3_MLP", "0"), ("FUMI_XP_KSPLIT", "1")]


def case_seed(name):
    base = ALL_CASES[name].get("base", name)
    return 4000 + list(CASES).index(base)


def zero_grads(c):
    """Names (AM3 keys, 'dx_s', 'dx_q') of the gradients that are zero analytically, and exactly zero in the engine: everything at
    N = 1 (the soft-max over one class is 1); the h network under a fixed lamda (the engine memsets its four); with lamda = 1 also the
    g network (the prototype is the image mean alone: txbar = (1 - 1) x ...), with lamda = 0 the support images' adjoints (the
    prototype is the text mean alone: imbar_s = 0 x ...)."""
    if c["N"] == 1:
        return set(list(R_KEYS) + ["dx_s", "dx_q"])
    if c["lamda_fixed"] is None:
        return set()
    return set(H_KEYS) | ({"G0", "g0", "G1", "g1"} if c["lamda_fixed"] == 1 else {"dx_s"})


def make_ragged(seed, ep, N, Dt):
    """Labels drawn uniformly in [0, N), every support label N-1 moved to class 0 (so class N-1, and by chance others, has no support
    row), and a text row of its own for every support row."""
    rs = np.random.RandomState(seed + 15485863)
    B, S = ep["y_s"].shape
    Qn = ep["y_q"].shape[1]
    y_s = rs.randint(0, N, size=(B, S))
    y_q = rs.randint(0, N, size=(B, Qn))
    y_s[y_s == N - 1] = 0
    ep = dict(ep)
    ep["y_s"] = torch.from_numpy(y_s.astype(np.int64))
    ep["y_q"] = torch.from_numpy(y_q.astype(np.int64))
    ep["text_s"] = torch.from_numpy(rs.standard_normal((B, S, Dt))).to(torch.float32)
    return ep


def make_inputs(name):
    """(case, episodes dict of float32 CPU tensors, weights dict, dropout masks or None)"""
    c = ALL_CASES[name]
    seed = case_seed(name)
    ep = cg.make_episodes(seed, c["B"], c["N"], c["K"], c["Q"], c["D"], c["Dt"])
    if c["ragged"]:
        ep = make_ragged(seed, ep, c["N"], c["Dt"])
    w = cg.make_am3_params(seed, c["D"], c["Dt"], c["Ht"], c["P"])
    masks = None
    if c["dropout"] > 0:
        from helpers import dropout_mask_flat
        Rs = c["B"] * c["N"] * c["K"]
        masks = (dropout_mask_flat(DROPOUT_SEED, c["dropout"], 1, Rs, c["Ht"]), dropout_mask_flat(DROPOUT_SEED, c["dropout"], 2, Rs, c["Ht"]))
    return c, ep, w, masks


def run_oracle(c, ep, w, masks, dtype):
    """oracle.fumi_ref.am3_step in ``dtype`` on the same inputs cast up, with dL/dx_s and dL/dx_q."""
    wr = {k: v.to(dtype).clone().requires_grad_(True) for k, v in w.items()}
    x_s, x_q = ep["x_s"].to(dtype).clone().requires_grad_(True), ep["x_q"].to(dtype).clone().requires_grad_(True)
    m = None if masks is None else tuple(t.to(dtype) for t in masks)
    ref = R.am3_step(wr, ep["text_s"].to(dtype), x_s, ep["y_s"], x_q, ep["y_q"], c["N"], c["lamda_fixed"], masks=m, extra=[x_s, x_q])
    g = OrderedDict(ref["grads"])
    g["dx_s"], g["dx_q"] = ref["g_extra"]
    ref["all_grads"] = g
    return ref


def safe_rows(dist, y_s, N):
    """(safe [B,Qn] bool, pred [B,Qn], empty [B,N] bool, first_empty [B]) from the oracle's distances [B,N,Qn].

    All classes without a support row have the same prototype (zero), so their distances tie exactly in any arithmetic: they are
    collapsed to the first of them before the margin between the two nearest prototypes is taken.  ``pred`` is the first arg-min
    (of the collapsed distances: the exact ties are gone, the first of the empty classes stands for all)."""
    B = dist.shape[0]
    cnt = torch.zeros(B, N, dtype=torch.int64).scatter_add_(1, y_s, torch.ones_like(y_s))
    empty = cnt == 0
    first_empty = torch.where(empty.any(1), empty.to(torch.int64).argmax(1), torch.full((B,), -1, dtype=torch.int64))
    drop = empty.clone()
    for b in range(B):
        if first_empty[b] >= 0:
            drop[b, first_empty[b]] = False
    d = dist.detach().to(torch.float64).transpose(1, 2).clone()                       # [B,Qn,N]
    d[drop.unsqueeze(1).expand_as(d)] = float("inf")
    pred = d.argmin(-1)
    if N == 1:
        return torch.ones_like(pred, dtype=torch.bool), pred, empty, first_empty
    d2 = d.topk(2, dim=-1, largest=False)[0]
    second = d2[..., 1]
    safe = torch.isinf(second) | ((second - d2[..., 0]) > MARGIN * second.abs().clamp_min(1.0))
    return safe, pred, empty, first_empty


# ---- the dispatch rules of am3_step_impl that the knobs override, restated for the child processes ----------------------------
def knob_env():
    return {k: int(os.environ[k]) for k in KNOBS if os.environ.get(k) is not None}


def expected_plan(name, env=None):
    """(plan the case must report, keys to compare) under the knobs of ``env`` (default: this process's).  Without a knob: the whole
    plan of the table.  A knob replaces the entries it decides; entries that then depend on code paths the row was not sized for
    (how many parts an overridden contraction split leaves, which MLP form a generic head's launch carries) are not compared --
    such a row checks values only."""
    c = ALL_CASES[name]
    env = knob_env() if env is None else env
    plan, keys = dict(c["plan"]), set(c["plan"])
    if env.get("FUMI_AM3_GENERIC"):
        plan.update(fast_head=0, nwaves=4, hgq=1, imparts=1)
        keys -= {"g_fwd_rode"}
    if env.get("FUMI_AM3_GQ", 0) > 0 and plan["fast_head"]:
        plan["hgq"] = min(env["FUMI_AM3_GQ"], 16)
    if "FUMI_AM3_MLP" in env and not env["FUMI_AM3_MLP"]:
        plan.update(g_fwd_split=0, g_fwd_rode=0, h_fwd_split=0, h_bwd_fused=0, g_bwd_fused=0, tx_nparts=0)
    if env.get("FUMI_XP_KSPLIT", -1) > 0:
        if env["FUMI_XP_KSPLIT"] == 1:
            plan.update(xks=1, imparts=1)
        else:
            keys -= {"xks", "imparts"}
    # knobs of the kernels underneath (tools/run_env_forms.sh runs this table under them too): the entries they decide are not compared
    if os.environ.get("FUMI_XP_RIDER") is not None or os.environ.get("FUMI_XP_SB") is not None:
        keys -= {"g_fwd_rode", "imparts"}
    if os.environ.get("FUMI_HYPER_BWD") is not None:
        keys -= {"h_bwd_fused", "g_bwd_fused", "tx_nparts"}
    return plan, keys
