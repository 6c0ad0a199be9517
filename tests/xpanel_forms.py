"""The X-panel form table shared by tests/test_xpanel_forms_cpu.py and tests/test_xpanel_forms_gpu.py -- TEST INFRASTRUCTURE ONLY.

One row per case of the two passes of csrc/xpanel.hip that read X:
    forward   [A0 | G] = [Xs ; Xq] . [W0 ; Xs]^T          (hip.xpanel_fwd)
    backward  gW0 = scale * sum_b Abar_b^T [Xs_b ; Xq_b]   (hip.xpanel_bwd; S = 0 or Qn = 0: a one-sided panel)
A row is (id, pass, B, S, Qn, D, h0, align, expected plan): the smallest shape that reaches a kernel form or one of its tile edges,
and the kernel (plus, for the backward pass, the split of the contraction) that the launchers of xpanel.hip take for it with no
environment knob set.  ``expected_plan`` restates the dispatch rules of launch_xpanel_fwd / launch_xpanel_bwd over the knobs, so
that a predicate that moves in xpanel.hip makes the plan assertion fail instead of quietly changing the kernel under a test."""
import os
from collections import OrderedDict

import torch

A0_TOL = 2e-6             # A0 and gW0: of the float64 reference's maximum (tests/test_hip_parity.py)
G_TOL = 4e-6              # G: all-positive support rows add up their truncated tails
MAX_MACS = 2e8            # B (S + Qn) D (h0 + S) of any case
GUARD = 256               # floats of NaN before and after every output

ALIGNS = ("none", "x_s", "x_q", "W0", "Abar")          # which tensor starts one float past a 16-byte boundary

FWD_KERNELS = {1: "generic", 2: "generic_fast", 3: "fp32", 4: "split", 5: "presplit"}              # = hip.XPANEL_FWD_KERNELS
BWD_KERNELS = {1: "guarded64", 2: "fast64", 3: "wide_fp32", 4: "wide_split", 5: "narrow_split"}    # = hip.XPANEL_BWD_KERNELS
FWD_KEYS = ("fwd_kernel", "fwd_ring", "fwd_ksplit", "fwd_gram_blocks", "fwd_rode")
BWD_KEYS = ("bwd_kernel", "bwd_nb", "bwd_sk", "bwd_nsplit", "bwd_kchunk", "bwd_rode")

KNOBS = ("FUMI_XP_SB", "FUMI_XP_PS", "FUMI_XP_SBN", "FUMI_XP_NST", "FUMI_XPB_SB", "FUMI_XPB_NB", "FUMI_XPB_SK", "FUMI_XPB_64",
         "FUMI_XPB_WG", "FUMI_XP_RIDER", "FUMI_XP_KSPLIT")
# one child process per setting (the knobs are `static` in the library)
KNOB_SETTINGS = [
    {"FUMI_XP_SB": "0"},
    {"FUMI_XP_SB": "0", "FUMI_XP_NST": "1"},
    {"FUMI_XP_SB": "0", "FUMI_XP_NST": "3"},
    {"FUMI_XP_PS": "0"},
    {"FUMI_XP_SBN": "4"},
    {"FUMI_XPB_SB": "0"},
    {"FUMI_XPB_NB": "1"},
    {"FUMI_XPB_NB": "1", "FUMI_XPB_SK": "32"},
    {"FUMI_XPB_64": "1"},
    {"FUMI_XPB_WG": "1"},
    {"FUMI_XPB_WG": "100000"},
]


def setting_id(s):
    return " ".join(f"{k}={v}" for k, v in s.items())


def _f(B, S, Qn, D, h0, kernel, align="none", **extra):
    return dict(pass_="fwd", B=B, S=S, Qn=Qn, D=D, h0=h0, align=align, scale=1.0, kernel=kernel, sides=False, extra=extra)


def _b(B, S, Qn, D, h0, kernel, align="none", scale=1.0, sides=False, **extra):
    return dict(pass_="bwd", B=B, S=S, Qn=Qn, D=D, h0=h0, align=align, scale=scale, kernel=kernel, sides=sides, extra=extra)


# id -> case.  `kernel` (and the extra plan entries) is what the default process reports.  Seeds are 7000 + the row's index.
_BASE = OrderedDict([
    # ---- forward: the pre-split kernel (h0 % 128 == 0, D % 32 == 0, at least PS_MIN_SLABS = 9 slabs, aligned)
    ("f_ps_d288", _f(2, 5, 15, 288, 128, "presplit", fwd_gram_blocks=1)),             # exactly 9 slabs
    ("f_sb_d256_h128", _f(2, 5, 15, 256, 128, "split")),                              # 8 slabs: falls to the per-tile split kernel
    ("f_ps_h384", _f(2, 5, 20, 288, 384, "presplit", fwd_gram_blocks=1)),             # three 128-column tiles
    ("f_ps_r63", _f(2, 5, 58, 288, 128, "presplit")),                                 # below one 64-row tile
    ("f_ps_r64", _f(2, 5, 59, 288, 128, "presplit")),                                 # exactly one
    ("f_ps_r65", _f(2, 5, 60, 288, 128, "presplit")),                                 # one and a ragged one
    ("f_ps_r129", _f(2, 5, 124, 288, 128, "presplit")),                               # two 128-row Gram tiles plus one row
    # Gram column blocks of 32 at their edges.  (S = 1: the largest entries of G are the B diagonal ones, |xs|^2, seven times any
    # other; the maxima the split-against-fp32 rule compares are taken over those alone, so the row has nine episodes, not two)
    ("f_ps_s1", _f(9, 1, 10, 288, 128, "presplit", fwd_gram_blocks=1)),
    ("f_ps_s32", _f(2, 32, 10, 288, 128, "presplit", fwd_gram_blocks=1)),
    ("f_ps_s33", _f(2, 33, 10, 288, 128, "presplit", fwd_gram_blocks=2)),
    ("f_ps_s65", _f(2, 65, 10, 320, 128, "presplit", fwd_gram_blocks=3)),
    ("f_ps_b1", _f(1, 5, 15, 288, 128, "presplit")),                                  # one episode, a full XCD group, one more
    ("f_ps_b8", _f(8, 5, 15, 288, 128, "presplit")),
    ("f_ps_b9", _f(9, 5, 15, 288, 128, "presplit")),
    ("f_ps_d512_h256", _f(3, 40, 100, 512, 256, "presplit", fwd_gram_blocks=2)),       # 16 slabs: the steady-state loop runs
    # ---- forward: the per-tile split kernel (D % 32 == 0, aligned)
    ("f_sb_seam", _f(3, 25, 43, 256, 96, "split", fwd_gram_blocks=1)),                # a 64-column tile straddles the W0 / Gram seam
    ("f_sb_h5", _f(3, 25, 40, 256, 5, "split", fwd_gram_blocks=1)),                   # the MAML head: h0 = N
    ("f_sb_h64_s64", _f(2, 64, 10, 256, 64, "split", fwd_gram_blocks=1)),             # the seam on a tile edge
    ("f_sb_d32", _f(2, 5, 15, 32, 40, "split")),                                      # 1 slab
    ("f_sb_d96", _f(2, 5, 15, 96, 40, "split")),                                      # 3 slabs (generic-fast under FUMI_XP_SB=0)
    ("f_sb_d128", _f(2, 5, 15, 128, 40, "split")),                                    # 4 slabs: the last count without the main loop
    ("f_sb_d160", _f(2, 5, 15, 160, 40, "split")),                                    # 5 slabs: the first with it
    ("f_sb_d288_h96", _f(9, 33, 32, 288, 96, "split", fwd_gram_blocks=2)),            # 9 slabs (the main loop at ring depth 4), B = 9
    ("f_sb_r65", _f(2, 5, 60, 64, 128, "split")),                                     # 2 slabs, a ragged second row tile
    # ---- forward: the generic guarded kernel, by shape and by alignment
    ("f_gen_d72", _f(2, 5, 15, 72, 40, "generic")),
    ("f_gen_d130", _f(2, 5, 60, 130, 70, "generic", fwd_gram_blocks=1)),
    ("f_gen_d31", _f(2, 5, 15, 31, 40, "generic")),
    ("f_gen_d1", _f(3, 5, 15, 1, 5, "generic")),
    ("f_gen_xs_off", _f(2, 5, 15, 256, 128, "generic", align="x_s")),
    ("f_gen_xq_off", _f(2, 5, 15, 256, 128, "generic", align="x_q")),
    ("f_gen_w0_off", _f(2, 5, 15, 256, 128, "generic", align="W0")),
    # ---- backward: the narrow swapped split kernel (h0 == 64, D % 256 == 0): K_tot = B (S + Qn) of 5, 32, 33, 340
    ("b_nar_k5", _b(1, 2, 3, 256, 64, "narrow_split", bwd_nsplit=1, bwd_kchunk=32, sides=True)),
    ("b_nar_k32", _b(2, 6, 10, 512, 64, "narrow_split", bwd_nsplit=1, bwd_kchunk=32)),
    ("b_nar_k33", _b(3, 4, 7, 256, 64, "narrow_split", bwd_nsplit=2, bwd_kchunk=32, scale=0.125)),
    ("b_nar_k340", _b(5, 25, 43, 512, 64, "narrow_split", bwd_nsplit=11, bwd_kchunk=32, scale=-3.0, sides=True)),
    ("b_nar_k2405", _b(13, 25, 160, 256, 64, "narrow_split", bwd_nsplit=26, bwd_kchunk=96)),     # 6 slabs of 16 each: the main loop
    # ---- backward: the wide split kernel (h0 % 256 == 0, D % 64 == 0): NB = 2 (D % 128 == 0), NB = 1
    ("b_wide_nb2_h256", _b(5, 25, 43, 128, 256, "wide_split", bwd_nb=2, bwd_sk=16, bwd_nsplit=11, bwd_kchunk=32, sides=True)),
    ("b_wide_nb1_h256", _b(5, 25, 43, 192, 256, "wide_split", bwd_nb=1, bwd_sk=16, bwd_nsplit=11, bwd_kchunk=32, scale=0.125,
                           sides=True)),
    ("b_wide_nb2_h512", _b(3, 10, 21, 128, 512, "wide_split", bwd_nb=2, bwd_sk=16, bwd_nsplit=3, bwd_kchunk=32, scale=-3.0)),
    ("b_wide_nb1_h512", _b(3, 10, 23, 192, 512, "wide_split", bwd_nb=1, bwd_sk=16, bwd_nsplit=4, bwd_kchunk=32)),
    # 26 slabs of 96 rows over episodes of 185: every slab border falls inside an episode (lcm(96, 185) > K_tot); six 16-row steps
    # per workgroup run the steady-state loop; 26 = 3 * 8 + 2: six of the last eight workgroups of a tile fall idle
    ("b_wide_straddle", _b(13, 25, 160, 128, 256, "wide_split", bwd_nb=2, bwd_sk=16, bwd_nsplit=26, bwd_kchunk=96)),
    ("b_wide_nb1_long", _b(13, 5, 180, 64, 256, "wide_split", bwd_nb=1, bwd_sk=16, bwd_nsplit=26, bwd_kchunk=96)),
    ("b_wide_k20", _b(1, 5, 15, 128, 256, "wide_split", bwd_nb=2, bwd_sk=16, bwd_nsplit=1, bwd_kchunk=32)),   # one partly filled slab
    # ---- backward: the 64 x 64 fast kernel (h0 % 64 == 0, D % 64 == 0, aligned; neither wide nor narrow)
    ("b_f64_h128", _b(5, 25, 43, 128, 128, "fast64", bwd_nsplit=11, sides=True)),
    ("b_f64_h192", _b(3, 10, 23, 64, 192, "fast64", bwd_nsplit=4, scale=0.125)),
    ("b_f64_h64_d192", _b(3, 4, 7, 192, 64, "fast64", bwd_nsplit=2, scale=-3.0)),
    # ---- backward: the 64 x 64 guarded kernel, by shape and by alignment
    ("b_g64_d72_h40", _b(5, 25, 43, 72, 40, "guarded64", bwd_nsplit=11, sides=True)),
    ("b_g64_d130_h5", _b(3, 25, 40, 130, 5, "guarded64", bwd_nsplit=7, scale=0.125)),               # the MAML head
    ("b_g64_abar_off", _b(3, 10, 23, 64, 64, "guarded64", align="Abar", bwd_nsplit=4)),
    ("b_g64_xs_off_wide", _b(3, 10, 23, 128, 256, "guarded64", align="x_s", bwd_nsplit=4, scale=-3.0)),
    ("b_g64_xq_off_narrow", _b(3, 4, 7, 256, 64, "guarded64", align="x_q", bwd_nsplit=2)),
])


def _one_sided(name, c, side):
    """The panel of a two-sided case cut to its query rows (S = 0) or its support rows (Qn = 0): same kernel family; the split of
    the contraction follows from the rows that are left (expected_plan)."""
    d = dict(c, sides=False, extra={k: v for k, v in c["extra"].items() if k not in ("bwd_nsplit", "bwd_kchunk")}, parent=name)
    if side == "s0":
        d["S"] = 0
    else:
        d["Qn"] = 0
    return d


CASES = OrderedDict()
for _n, _c in _BASE.items():
    CASES[_n] = dict(_c, parent=None)
    if _c["sides"]:
        CASES[_n + "_s0"] = _one_sided(_n, _c, "s0")
        CASES[_n + "_q0"] = _one_sided(_n, _c, "q0")
ALL_CASES = list(CASES)
SEEDS = {n: 7000 + i for i, n in enumerate(_BASE)}


def table_plan(name):
    """What the table itself says the default process reports for a row: the kernel, and the plan entries the row spells out."""
    c = CASES[name]
    ids = {v: k for k, v in (FWD_KERNELS if c["pass_"] == "fwd" else BWD_KERNELS).items()}
    return dict(c["extra"], **{c["pass_"] + "_kernel": ids[c["kernel"]]})


def macs(c):
    return c["B"] * (c["S"] + c["Qn"]) * c["D"] * (c["h0"] + c["S"])


# ---- the dispatch rules of xpanel.hip, restated ---------------------------------------------------------------------------------
def _knob(env, name, default):
    v = env.get(name)
    return default if v is None or v == "" else int(v)


def _bwd_split(c, env):
    """xpanel_bwd_nsplit: (nsplit, kchunk)."""
    B, S, Qn, D, h0 = (c[k] for k in ("B", "S", "Qn", "D", "h0"))
    ktot = B * (S + Qn)
    wide = not _knob(env, "FUMI_XPB_64", 0) and h0 % 256 == 0 and D % 64 == 0
    narrow = _knob(env, "FUMI_XPB_SB", 1) and h0 == 64 and D % 256 == 0
    r32 = lambda v: (v + 31) // 32 * 32
    if narrow:
        ns = max(1, min(32, (256 + D // 256 - 1) // (D // 256)))
        kc = r32((ktot + ns - 1) // ns)
        return (ktot + kc - 1) // kc, kc
    tiles = (h0 // 256) * (D // 64) if wide else ((h0 + 63) // 64) * ((D + 63) // 64)
    target = _knob(env, "FUMI_XPB_WG", 0)
    want = target if target > 0 else (512 if wide else 1024)
    ns = max(1, min(32, (want + tiles - 1) // tiles))
    kc = max(32, r32((ktot + ns - 1) // ns))
    return (ktot + kc - 1) // kc, kc


def expected_plan(name, env=None):
    """The plan entries of the pass of case ``name`` (FWD_KEYS or BWD_KEYS) under the knobs of ``env`` (default: os.environ)."""
    env = os.environ if env is None else env
    c = CASES[name]
    B, S, Qn, D, h0, al = (c[k] for k in ("B", "S", "Qn", "D", "h0", "align"))
    if c["pass_"] == "fwd":
        sb, ps = _knob(env, "FUMI_XP_SB", 1), _knob(env, "FUMI_XP_PS", 1)
        sbn, nst = _knob(env, "FUMI_XP_SBN", 2), _knob(env, "FUMI_XP_NST", 2)
        aligned = al not in ("x_s", "x_q", "W0")
        gram_tiles = (h0 + S + 63) // 64 - h0 // 64
        if aligned and ps and sb and h0 % 128 == 0 and D % 32 == 0 and D // 32 >= 9:
            v = (5, 2, 1, (S + 31) // 32, 0)
        elif aligned and D % 32 == 0 and sb:
            v = (4, 2 if sbn <= 2 else 4, 1, gram_tiles, 0)
        elif aligned and D % 64 == 0:
            v = (3, 1 if nst == 1 else 2 if nst == 2 else 3, 1, gram_tiles, 0)
        elif aligned and D % 32 == 0:
            v = (2, 2, 1, gram_tiles, 0)
        else:
            v = (1, 2, 1, gram_tiles, 0)
        return dict(zip(FWD_KEYS, v))
    bsb = _knob(env, "FUMI_XPB_SB", 1)
    ns, kc = _bwd_split(c, env)
    present = ("x_s", "x_q") if S and Qn else ("x_s",) if S else ("x_q",)     # (an absent side's pointer is the present side's)
    fast = D % 64 == 0 and h0 % 64 == 0 and al not in present and al != "Abar"
    wide = not _knob(env, "FUMI_XPB_64", 0) and h0 % 256 == 0 and D % 64 == 0
    narrow = bsb and h0 == 64 and D % 256 == 0
    if fast and narrow and kc % 16 == 0:
        v = (5, 1, 16, ns, kc, 0)
    elif fast and wide and bsb and kc % 16 == 0:
        nb = 2 if _knob(env, "FUMI_XPB_NB", 2) == 2 and D % 128 == 0 else 1
        sk = 32 if nb == 1 and _knob(env, "FUMI_XPB_SK", 16) == 32 and kc % 32 == 0 else 16
        v = (4, nb, sk, ns, kc, 0)
    elif fast and wide:
        v = (3, 1, 32, ns, kc, 0)
    else:
        v = (2 if fast else 1, 1, 32, ns, kc, 0)
    return dict(zip(BWD_KEYS, v))


def instance(plan):
    """The kernel template instance a plan names (riders and ksplit > 1 aside)."""
    if "fwd_kernel" in plan:
        k = FWD_KERNELS[plan["fwd_kernel"]]
        return {"generic": "xpanel_fwd_generic_kernel<false>", "generic_fast": "xpanel_fwd_generic_kernel<true>",
                "fp32": f"xpanel_fwd_kernel<{plan['fwd_ring']}>", "split": f"xpanel_fwd_sb_kernel<{plan['fwd_ring']},false>",
                "presplit": "xpanel_presplit_kernel+xpanel_fwd_ps_kernel<2,false>"}[k]
    k = BWD_KERNELS[plan["bwd_kernel"]]
    return {"guarded64": "xpanel_bwd_kernel<false>", "fast64": "xpanel_bwd_kernel<true>", "wide_fp32": "xpanel_bwd256_kernel<false>",
            "wide_split": f"xpanel_bwd256_sb_kernel<false,2,{plan['bwd_nb']},{plan['bwd_sk']}>",
            "narrow_split": "xpanel_bwd256_sb_kernel<false,2,1,16,true>"}[k]


# every instance launch_xpanel_fwd / launch_xpanel_bwd can launch without a rider, a `parts` buffer or a pending embedding bag
INSTANCES = {"xpanel_fwd_generic_kernel<false>", "xpanel_fwd_generic_kernel<true>", "xpanel_fwd_kernel<1>", "xpanel_fwd_kernel<2>",
             "xpanel_fwd_kernel<3>", "xpanel_fwd_sb_kernel<2,false>", "xpanel_fwd_sb_kernel<4,false>",
             "xpanel_presplit_kernel+xpanel_fwd_ps_kernel<2,false>", "xpanel_bwd_kernel<false>", "xpanel_bwd_kernel<true>",
             "xpanel_bwd256_kernel<false>", "xpanel_bwd256_sb_kernel<false,2,2,16>", "xpanel_bwd256_sb_kernel<false,2,1,16>",
             "xpanel_bwd256_sb_kernel<false,2,1,32>", "xpanel_bwd256_sb_kernel<false,2,1,16,true>"}


# ---- inputs and the float64 reference -------------------------------------------------------------------------------------------
def make_inputs(name):
    """x_s = |randn| (post-ReLU-like), x_q = 3 randn, W0 = 0.05 randn, Abar = randn x rand per row (rows of very different scale):
    the data of tests/test_hip_parity.py.  A one-sided case is its parent's data cut to the rows that are left."""
    c = CASES[name]
    p = CASES[c["parent"]] if c["parent"] else c
    g = torch.Generator().manual_seed(SEEDS[c["parent"] or name])
    B, S, Qn, D, h0 = (p[k] for k in ("B", "S", "Qn", "D", "h0"))
    d = dict(x_s=torch.randn(B, S, D, generator=g).abs(), x_q=torch.randn(B, Qn, D, generator=g) * 3.0)
    if c["pass_"] == "fwd":
        d["W0"] = torch.randn(h0, D, generator=g) * 0.05
    else:
        d["Abar"] = torch.randn(B, S + Qn, h0, generator=g) * torch.rand(B, S + Qn, 1, generator=g)
        if c["S"] == 0:
            d["x_s"], d["Abar"] = None, d["Abar"][:, S:].contiguous()
        elif c["Qn"] == 0:
            d["x_q"], d["Abar"] = None, d["Abar"][:, :S].contiguous()
    return d


def panel(d):
    return torch.cat([t for t in (d["x_s"], d["x_q"]) if t is not None], 1)


def reference(name, d, dtype=torch.float64):
    """fwd: (A0, G); bwd: (gW0,) -- plain products in ``dtype``."""
    c = CASES[name]
    X = panel(d).to(dtype)
    if c["pass_"] == "fwd":
        return X @ d["W0"].to(dtype).T, X @ d["x_s"].to(dtype).transpose(1, 2)
    return (c["scale"] * (d["Abar"].to(dtype).reshape(-1, c["h0"]).T @ X.reshape(-1, c["D"])),)


def rel_err(got, ref):
    """Largest error of the reference's maximum."""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
