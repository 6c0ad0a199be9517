"""The form table of the hypernetwork of the FuMI step (csrc/hyper.hip, csrc/hyper_fwd.h, csrc/hyper_bwd.h and the rider branches of
csrc/xpanel.hip), shared by tests/test_hyper_forms_cpu.py, tests/test_hyper_forms_gpu.py and
tools/hyper_forms_report.py -- TEST INFRASTRUCTURE ONLY.

One row per form and per side of each edge of hyper_net = Linear(Dt, Ht) -> ReLU -> Linear(Ht, H1) [-> Tanh] and its backward, over
R = B N rows in nrb = ceil(R / 16) row blocks and nch = Ht / 64 hidden chunks.  A row is the step's shape, its options and, written
by hand, the plan `fumi_hip_hyper_plan` must report for it plus the `fwd_rode` / `bwd_rode` entries of `fumi_hip_xpanel_plan`.  The
inputs, the float64 / float32 oracle, the error measure and the margin mask are those of tests/epi_forms.py; every row has K = Q = 1
and T = 1 so that the episode side stays small.

What carries a rider.  The forward rider sits in either split-bf16 forward X-panel kernel: the per-tile split one takes any aligned
D % 32 == 0 (so D = 32 DOES ride), the pre-split one h0 % 128 == 0 with D / 32 >= 9.  The backward rider sits in the wide backward
kernels: h0 % 256 == 0 and D % 64 == 0, 256 x 128 tiles (NB = 2) at D % 128 == 0, else 256 x 64 (NB = 1).  Rows that must not ride
use D = 24 and h0 = 8.

What the step cannot reach, so that no row holds it:
  * H1 = 1: H1 = hid[-1] + 1 and the API refuses a hidden width of 0; the smallest output width is H1 = 2 (h1_2).
  * nrb = 1024 | 1025 (FUMI_HCNT) in the split forward: hyper_lds_fits holds R to 279 rows (the two-launch backward stages all R
    rows of ubar and c in one workgroup), and the step only offers the split forward where hyper_lds_fits holds, so nrb <= 18 there;
    the counter limit can only bind through AM3's text towers.  A step with R = 16384 runs the hypernetwork forward as plain GEMMs.
  * the LDS-resident forward with H1 >= 128 at Ht >= 256: the two-launch backward's layout (hyper_lds_fits) is over its cap, the
    forward is plain GEMMs (h1_128_ht256, gemm_ht320) while the fused backward, which has its own rule, stays.  Per-layer at
    Ht = 320 is therefore reached by the FUMI_HYPER_FWD knobs and by a misaligned pointer, not by H1 = 129.
  * hyper_net.2.bias (phi[3]) one float off: no form reads it as float4, the row (off_phi3) keeps every form.

No row costs more than MAX_MACS = 2e8 multiply-adds: epi_forms.macs plus 3 R (Dt Ht + Ht H1)."""
import os
from collections import OrderedDict

import torch

import epi_forms as E
from oracle import casegen as cg, fumi_ref as R

MAX_MACS = E.MAX_MACS
LOGIT_TOL, GRAD_TOL, WITNESS_TOL, ERR_FLOOR = E.LOGIT_TOL, E.GRAD_TOL, E.WITNESS_TOL, E.ERR_FLOOR
# Form bound: a form's error against float64 may exceed the float32 oracle's on the same row by this factor -- the smallest power of
# two that is at least twice the largest ratio measured over every row and knob setting (profiles/hyper_forms/errors.json, written by
# tools/hyper_forms_report.py); both sides floored at ERR_FLOOR.
FORM_MARGIN = 16
GUARD = 64             # floats of NaN before and after every gradient output (256 bytes: the outputs keep their 16-byte alignment)

PLAN_KEYS = ("fwd_form", "fwd_inst", "nrb", "nch", "bwd_form", "bwd_dpasses", "text_grad")          # = hip.HYPER_PLAN_KEYS
RODE_KEYS = ("fwd_rode", "bwd_rode")                                                                # of hip.XPANEL_PLAN_KEYS
FWD = {"gemm": 0, "per_layer": 1, "fused": 2, "split": 3, "rode_split": 4, "rode_presplit": 5}
BWD = {"none": 0, "gemm": 1, "two_launch": 2, "fused": 3, "rode": 4}
OFFS = ("cls_text", "phi0", "phi1", "phi2", "phi3")


def _row(B, N, D, hid, Dt, Ht, plan, **o):
    """plan: 'fwd/inst nrb x nch bwd/dpasses text_grad' by name, e.g. 'rode_split/24 9x4 rode/1 0'."""
    f, blocks, b, tg = plan.split()
    fn, fi = f.split("/")
    bn, bd = b.split("/")
    nrb, nch = blocks.split("x")
    p = dict(fwd_form=FWD[fn], fwd_inst=int(fi), nrb=int(nrb), nch=int(nch), bwd_form=BWD[bn], bwd_dpasses=int(bd), text_grad=int(tg))
    p["fwd_rode"], p["bwd_rode"] = int(fn.startswith("rode")), int(bn == "rode")
    c = dict(entry="fumi", B=B, N=N, K=1, Q=1, D=D, hid=list(hid), T=1, Dt=Dt, Ht=Ht, tanh=False, need_grad=True, want_text_grad=False,
             off=None, dropout=0.0, first_order=False, plan=p)
    c.update(o)
    return c


W64, W128 = (64, [256, 64]), (128, [256, 64])          # carry both riders: per-tile split forward; wide backward with NB = 1 / NB = 2
OWN = 24                                                # D of the rows that carry no rider (with h0 = 8)

CASES = OrderedDict([
    # ---- row blocks, both riders: one ragged block | eight full | nine with 1 row and 7 idle slots | nine with 15 rows
    ("rb_r10", _row(2, 5, *W64, 300, 256, "rode_split/24 1x4 rode/1 0")),
    ("rb_r128", _row(16, 8, *W64, 300, 256, "rode_split/24 8x4 rode/1 0")),
    ("rb_r129", _row(43, 3, *W64, 300, 256, "rode_split/24 9x4 rode/1 1", want_text_grad=True)),
    ("rb_r143", _row(13, 11, *W64, 300, 256, "rode_split/24 9x4 rode/1 0", tanh=True)),
    # ---- text width, both riders (Ht = 128): the clamp to Dt - 4 (4 | 16 | 20), a last 16-step partly past Dt (300), the rider's
    # second register chunk and the backward's second pass (384 | 388), the rider's end (768 | 772: one launch per layer, third pass)
    ("dt4", _row(2, 5, *W64, 4, 128, "rode_split/24 1x2 rode/1 1", want_text_grad=True)),
    ("dt16", _row(2, 5, *W64, 16, 128, "rode_split/24 1x2 rode/1 0")),
    ("dt20", _row(2, 5, *W64, 20, 128, "rode_split/24 1x2 rode/1 0", tanh=True)),
    ("dt300", _row(2, 5, *W64, 300, 128, "rode_split/24 1x2 rode/1 1", want_text_grad=True, tanh=True)),
    ("dt384", _row(2, 5, *W64, 384, 128, "rode_split/24 1x2 rode/1 0")),
    ("dt388", _row(2, 5, *W64, 388, 128, "rode_split/24 1x2 rode/2 0")),
    ("dt768", _row(2, 5, *W64, 768, 128, "rode_split/24 1x2 rode/2 1", want_text_grad=True)),
    ("dt772", _row(2, 5, *W64, 772, 128, "per_layer/16 1x2 rode/3 1", want_text_grad=True)),
    # ---- hidden width, both riders: every workgroup its block's last arriver (64) | four chunks | five
    ("ht64", _row(3, 7, *W64, 20, 64, "rode_split/24 2x1 rode/1 1", want_text_grad=True)),
    ("ht256", _row(3, 7, *W64, 20, 256, "rode_split/24 2x4 rode/1 1", want_text_grad=True)),
    ("ht320", _row(3, 7, *W64, 20, 320, "rode_split/24 2x5 rode/1 1", want_text_grad=True, tanh=True)),
    # ---- output width, both riders, the NB = 2 backward host (Ht = 192): tiles wave and wave + 4 of layer 1, rows of h / hbar off
    # 16-byte alignment (17, 65, 129), the split form's cap (128 | 129: the fused forward takes over, the backward keeps its own rule)
    ("h1_2", _row(3, 7, 128, [256, 1], 20, 192, "rode_split/24 2x3 rode/1 0")),
    ("h1_16", _row(3, 7, 128, [256, 15], 20, 192, "rode_split/24 2x3 rode/1 0")),
    ("h1_17", _row(3, 7, 128, [256, 16], 20, 192, "rode_split/24 2x3 rode/1 0", tanh=True)),
    ("h1_64", _row(3, 7, 128, [256, 63], 20, 192, "rode_split/24 2x3 rode/1 0")),
    ("h1_65", _row(3, 7, *W128, 20, 192, "rode_split/24 2x3 rode/1 0")),
    ("h1_128", _row(3, 7, 128, [256, 127], 20, 192, "rode_split/24 2x3 rode/1 0", tanh=True)),
    ("h1_129", _row(3, 7, 128, [256, 128], 20, 192, "fused/21 2x3 rode/1 0", tanh=True)),
    # ---- need_grad = 0; the pre-split forward host, alone (h0 = 128: no wide backward) and with the NB = 1 backward host
    ("nograd", _row(2, 5, *W64, 300, 128, "rode_split/24 1x2 none/0 0", need_grad=False)),
    ("ps_fwd", _row(2, 5, 288, [128, 64], 388, 128, "rode_presplit/24 1x2 fused/2 1", want_text_grad=True)),
    ("ps_both", _row(2, 5, 320, [256, 64], 768, 256, "rode_presplit/24 1x4 rode/2 0", tanh=True)),
    # ---- own launches (no rider: D = 24, h0 = 8).  split<20> | split<48>
    ("own_base", _row(3, 7, OWN, [8, 16], 20, 64, "split/20 2x1 fused/1 1", want_text_grad=True)),
    ("own_dt320", _row(3, 7, OWN, [8, 16], 320, 64, "split/20 2x1 fused/1 0")),
    ("own_dt324", _row(3, 7, OWN, [8, 16], 324, 64, "split/48 2x1 fused/1 0", tanh=True)),
    # the eight instances of the one-workgroup-per-row-block forward: H1 = 129 loses the split form; NT = 1 | 2 at Ht = 128 | 192,
    # NCH = ceil(Dt / 192)
    ("f11", _row(3, 7, OWN, [8, 128], 192, 128, "fused/11 2x2 fused/1 0")),
    ("f12", _row(3, 7, OWN, [8, 128], 384, 128, "fused/12 2x2 fused/1 0", tanh=True)),
    ("f13", _row(3, 7, OWN, [8, 128], 388, 128, "fused/13 2x2 fused/2 0")),
    ("f14", _row(3, 7, OWN, [8, 128], 768, 128, "fused/14 2x2 fused/2 0")),
    ("f21", _row(3, 7, OWN, [8, 128], 20, 192, "fused/21 2x3 fused/1 0")),
    ("f22", _row(3, 7, OWN, [8, 128], 300, 192, "fused/22 2x3 fused/1 0")),
    ("f23", _row(3, 7, OWN, [8, 128], 576, 192, "fused/23 2x3 fused/2 0", tanh=True)),
    ("f24", _row(3, 7, OWN, [8, 128], 768, 192, "fused/24 2x3 fused/2 1", want_text_grad=True)),
    # one launch per layer and the two-launch backward: each pointer one float past a 16-byte boundary.  The forward reads cls_text,
    # phi[0], phi[1], phi[2] as float4, the fused backward cls_text and phi[2]; nothing reads phi[3] so
    ("off_cls_text", _row(3, 7, OWN, [8, 16], 20, 64, "per_layer/64 2x1 two_launch/0 1", want_text_grad=True, off="cls_text")),
    ("off_phi0", _row(3, 7, OWN, [8, 16], 20, 64, "per_layer/64 2x1 fused/1 1", want_text_grad=True, off="phi0")),
    ("off_phi1", _row(3, 7, OWN, [8, 16], 20, 64, "per_layer/64 2x1 fused/1 1", want_text_grad=True, off="phi1")),
    ("off_phi2", _row(3, 7, OWN, [8, 16], 20, 64, "per_layer/64 2x1 two_launch/0 1", want_text_grad=True, off="phi2")),
    ("off_phi3", _row(3, 7, OWN, [8, 16], 20, 64, "split/20 2x1 fused/1 1", want_text_grad=True, off="phi3")),
    ("off_rider", _row(2, 5, *W64, 300, 256, "per_layer/64 1x4 two_launch/0 0", off="phi2")),           # a riding shape: no rider is offered
    # plain GEMMs: Dt % 4, Ht % 64, and the two-launch layout over its cap (forward only)
    ("gemm_dt18", _row(3, 7, OWN, [8, 16], 18, 64, "gemm/0 2x1 gemm/0 2", want_text_grad=True)),
    ("gemm_ht20", _row(3, 7, OWN, [8, 16], 20, 20, "gemm/0 2x0 gemm/0 2", want_text_grad=True)),
    ("gemm_ht320", _row(3, 7, OWN, [8, 128], 20, 320, "gemm/0 2x5 fused/1 0", tanh=True)),
    ("h1_128_ht256", _row(3, 7, 128, [256, 127], 20, 256, "gemm/0 2x4 rode/1 0", tanh=True)),
])
ALL_CASES = list(CASES)
SEED_OVERRIDE = {}
SEEDS = {n: 9400 + i for i, n in enumerate(CASES)}
SEEDS.update(SEED_OVERRIDE)
for _n, _c in CASES.items():
    _c["seed"] = SEEDS[_n]

# (inside, outside, the plan and rode entries that differ, the row arguments that differ)
EDGE_PAIRS = [
    ("rb_r10", "rb_r128", {"nrb"}, {"B", "N"}),
    ("rb_r128", "rb_r129", {"nrb", "text_grad"}, {"B", "N", "want_text_grad"}),            # 8 | 9 row blocks: the XCD-grouped ids leave 7 slots idle
    ("rb_r129", "rb_r143", {"text_grad"}, {"B", "N", "want_text_grad", "tanh"}),           # 1 | 15 rows in the last block
    ("dt16", "dt20", set(), {"Dt", "tanh"}),
    ("dt384", "dt388", {"bwd_dpasses"}, {"Dt"}),                                           # HBW_DC and the rider's register chunk
    ("dt768", "dt772", {"fwd_form", "fwd_inst", "fwd_rode", "bwd_dpasses"}, {"Dt"}),        # the split form's and the fused forward's end
    ("own_dt320", "own_dt324", {"fwd_inst"}, {"Dt", "tanh"}),                              # KS = 20 | 48
    ("ht256", "ht320", {"nch"}, {"Ht", "tanh"}),
    ("f12", "f13", {"fwd_inst", "bwd_dpasses"}, {"Dt", "tanh"}),                           # 384 | 388: a third chunk of 192
    ("f14", "f24", {"fwd_inst", "nch", "text_grad"}, {"Ht", "want_text_grad"}),            # NT = 1 | 2
    ("h1_16", "h1_17", set(), {"hid", "tanh"}),
    ("h1_64", "h1_65", set(), {"hid"}),
    ("h1_128", "h1_129", {"fwd_form", "fwd_inst", "fwd_rode"}, {"hid"}),                   # the split form's cap; the backward rides on
    ("h1_128", "h1_128_ht256", {"fwd_form", "fwd_inst", "fwd_rode", "nch"}, {"Ht"}),       # hyper_lds_fits: the two-launch layout's cap
    ("own_base", "off_cls_text", {"fwd_form", "fwd_inst", "bwd_form", "bwd_dpasses"}, {"off"}),
    ("own_base", "off_phi0", {"fwd_form", "fwd_inst"}, {"off"}),
    ("own_base", "off_phi1", {"fwd_form", "fwd_inst"}, {"off"}),
    ("own_base", "off_phi2", {"fwd_form", "fwd_inst", "bwd_form", "bwd_dpasses"}, {"off"}),
    ("own_base", "off_phi3", set(), {"off"}),
    ("rb_r10", "off_rider", {"fwd_form", "fwd_inst", "fwd_rode", "bwd_form", "bwd_dpasses", "bwd_rode"}, {"off"}),
    ("own_base", "gemm_dt18", {"fwd_form", "fwd_inst", "bwd_form", "bwd_dpasses", "text_grad"}, {"Dt"}),          # Dt % 4
    ("own_base", "gemm_ht20", {"fwd_form", "fwd_inst", "nch", "bwd_form", "bwd_dpasses", "text_grad"}, {"Ht"}),   # Ht % 64
    ("dt300", "nograd", {"bwd_form", "bwd_dpasses", "bwd_rode", "text_grad"}, {"need_grad", "want_text_grad", "tanh"}),
]

# ---- knob settings: one child process each; the rows a setting changes and the entries it changes them to (an empty dict: the row
# is run under the setting and keeps its plan)
_LIN = lambda nc: dict(fwd_form=FWD["per_layer"], fwd_inst=nc, fwd_rode=0)
_TWO = dict(bwd_form=BWD["two_launch"], bwd_dpasses=0, bwd_rode=0)
KNOB_SETTINGS = [
    # one launch per layer wherever the forward is its own launch; a rider is still a rider
    ({"FUMI_HYPER_FWD": "0"}, {"own_dt320": _LIN(64), "own_dt324": _LIN(64), "f14": _LIN(32), "f21": _LIN(64), "dt300": dict()}),
    # a workgroup per row block wherever the forward is its own launch and Ht <= 256
    ({"FUMI_HYPER_FWD": "1"}, {"own_base": dict(fwd_form=FWD["fused"], fwd_inst=11), "own_dt320": dict(fwd_form=FWD["fused"], fwd_inst=12),
                               "own_dt324": dict(fwd_form=FWD["fused"], fwd_inst=12), "rb_r10": dict()}),
    # the two-launch backward, or plain GEMMs where hyper_lds_fits says no; the text gradient stays a GEMM of its own / moves inside
    ({"FUMI_HYPER_BWD": "0"}, {"rb_r129": _TWO, "dt768": _TWO, "own_base": _TWO, "f23": _TWO,
                               "gemm_ht320": dict(bwd_form=BWD["gemm"], bwd_dpasses=0)}),
    # nothing rides: the split forward and the fused backward as their own launches
    ({"FUMI_XP_RIDER": "0"}, {"rb_r129": dict(fwd_form=FWD["split"], fwd_inst=20, fwd_rode=0, bwd_form=BWD["fused"], bwd_rode=0),
                              "dt388": dict(fwd_form=FWD["split"], fwd_inst=48, fwd_rode=0, bwd_form=BWD["fused"], bwd_rode=0),
                              "ps_both": dict(fwd_form=FWD["split"], fwd_inst=48, fwd_rode=0, bwd_form=BWD["fused"], bwd_rode=0),
                              "h1_129": dict(bwd_form=BWD["fused"], bwd_rode=0)}),
    # both directions on the side stream: own launches both ways
    ({"FUMI_OVERLAP": "3"}, {"rb_r143": dict(fwd_form=FWD["split"], fwd_inst=20, fwd_rode=0, **_TWO),
                             "dt768": dict(fwd_form=FWD["split"], fwd_inst=48, fwd_rode=0, **_TWO),
                             "own_base": _TWO, "nograd": dict(fwd_form=FWD["split"], fwd_inst=20, fwd_rode=0)}),
]
KNOBS = ("FUMI_HYPER_FWD", "FUMI_HYPER_BWD", "FUMI_XP_RIDER", "FUMI_OVERLAP")

setting_id = E.setting_id


def child_env(env):
    e = dict(os.environ)
    for k in KNOBS:
        e.pop(k, None)
    e.update(env)
    return e


def dims(c):
    return c["N"] * c["K"], c["N"] * c["Q"]


def macs(c):
    R_, H1 = c["B"] * c["N"], c["hid"][-1] + 1
    return E.macs(c) + 3 * R_ * (c["Dt"] * c["Ht"] + c["Ht"] * H1)


def table_plan(name, changes=None):
    """PLAN_KEYS + RODE_KEYS the table says row ``name`` reports (``changes``: what a knob setting moves)."""
    p = dict(CASES[name]["plan"])
    p.update(changes or {})
    return p


def query_plan(name):
    """fumi_hip_hyper_plan_query for the row, under this process's knobs (PLAN_KEYS only)."""
    from fumi_amd import hip
    c = CASES[name]
    S, Qn = dims(c)
    off = c["off"]
    return hip.hyper_plan_query(c["B"], c["N"], S, Qn, c["D"], c["hid"], c["Dt"], c["Ht"], c["T"], need_grad=c["need_grad"],
                                want_text_grad=c["want_text_grad"], side=True, cls_text_off=off == "cls_text",
                                phi_off=(int(off[3]),) if off and off.startswith("phi") else ())


# ---- inputs, the oracle, the step ------------------------------------------------------------------------------------------------
def make_inputs(name):
    return E.make_inputs(CASES[name])


def cls_rows(text_s, y_s, n_way):
    """[B,S,*] -> [B,N,*]: the row of the first support sample of each class (oracle.fumi_ref.class_text_select per episode)."""
    return torch.stack([R.class_text_select(text_s[b], y_s[b], n_way) for b in range(text_s.shape[0])])


def grad_names(c):
    return E.names(c) + (["g_cls_text"] if c["need_grad"] and c["want_text_grad"] else [])


def oracle(name, inputs, dtype):
    """E.oracle plus, where the row asks for it, g_cls_text [B,N,Dt] appended to ``grads``: the text gradient at each class's row."""
    c = CASES[name]
    want = c["need_grad"] and c["want_text_grad"]
    r = E.oracle(c, inputs, dtype, text_grad=want)
    if want:
        r["grads"] = list(r["grads"]) + [cls_rows(r.pop("g_text_s"), inputs[0]["y_s"], c["N"])]
    return r


def _guarded(shape, dev):
    """(buffer, view): the view is ``shape`` floats behind GUARD floats of NaN and before GUARD more; itself NaN too."""
    n = 1
    for s in shape:
        n *= int(s)
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev, dtype=torch.float32)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _one_off(t, dev):
    buf = torch.zeros(t.numel() + 4, device=dev, dtype=torch.float32)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def run_step(name, inputs, dev, ws):
    """The row through hip.fumi_step with the class text rows passed in: dict(logits, loss_b, preds, acc_b, grads or None, guards).
    Every gradient output (theta, phi and g_cls_text where asked for) is a NaN-filled view between NaN guards; ``guards`` holds the
    buffers.  The tensor named by the row's ``off`` is a view one float into a larger buffer."""
    from fumi_amd import hip
    c = CASES[name]
    ep, theta, phi = inputs
    g = lambda t: t.to(dev).contiguous()
    th, ph = [g(t) for t in theta], [g(t) for t in phi]
    ct = g(cls_rows(ep["text_s"], ep["y_s"], c["N"]))
    if c["off"] == "cls_text":
        ct = _one_off(ct, dev)
    elif c["off"]:
        i = int(c["off"][3])
        ph[i] = _one_off(ph[i], dev)
    guards, g_theta, g_phi, g_ct = [], None, None, None
    if c["need_grad"]:
        pairs = [_guarded(t.shape, dev) for t in th + ph]
        guards = [b for b, _ in pairs]
        g_theta, g_phi = [v for _, v in pairs[:len(th)]], [v for _, v in pairs[len(th):]]
        if c["want_text_grad"]:
            b, g_ct = _guarded(ct.shape, dev)
            guards.append(b)
    out = hip.fumi_step(ws, g(ep["x_s"]), g(ep["y_s"]), g(ep["x_q"]), g(ep["y_q"]), th, ph, c["T"], cg.ALPHA, c["tanh"], cls_text=ct,
                        need_grad=c["need_grad"], g_theta=g_theta, g_phi=g_phi, g_cls_text=g_ct)
    grads = None
    if c["need_grad"]:
        grads = list(out["g_theta"]) + list(out["g_phi"]) + ([g_ct] if g_ct is not None else [])
    return dict(logits=out["logits"], loss_b=out["loss_b"], preds=out["preds"], acc_b=out["acc_b"], grads=grads, guards=guards)


def guard_report(out):
    """[] when nothing outside the gradient outputs was written and nothing inside them was left unwritten, else what was."""
    bad = []
    for i, b in enumerate(out["guards"]):
        if not bool(torch.isnan(b[:GUARD]).all()) or not bool(torch.isnan(b[-GUARD:]).all()):
            bad.append(f"gradient output {i}: a guard was written")
        if bool(torch.isnan(b[GUARD:-GUARD]).any()):
            bad.append(f"gradient output {i}: {int(torch.isnan(b[GUARD:-GUARD]).sum())} elements left unwritten")
    for k in ("logits", "loss_b", "acc_b"):
        if bool(torch.isnan(out[k]).any()):
            bad.append(f"{k}: not a number")
    return bad


def errors(name, got, ref):
    """{quantity: error against ``ref`` as a fraction of the reference's maximum}: epi_forms.errors, the four phi gradients under their
    own names, and g_cls_text with the same floor rule where the row asks for it."""
    c = CASES[name]
    e = {"logits": E.rel_to_max(got["logits"].cpu(), ref["logits"]), "loss_b": E.rel_to_max(got["loss_b"].cpu(), ref["loss_b"])}
    if ref["grads"] is not None:
        fl = E.grad_floor(ref["grads"][:len(E.names(c))])
        for n, a, r in zip(grad_names(c), got["grads"], ref["grads"]):
            e[n] = E.rel_to_max(a.cpu(), r, fl)
    return e


def reported(name):
    """PLAN_KEYS + RODE_KEYS as the last step of this process reported them (fumi_hip_hyper_plan, fumi_hip_xpanel_plan).  A step
    without gradients launches no backward X-panel pass, whose record then still is an earlier step's: bwd_rode counts as 0."""
    from fumi_amd import hip
    plan, xplan = hip.hyper_plan(), hip.xpanel_plan()
    seen = dict(plan, **{k: xplan[k] for k in RODE_KEYS})
    if not CASES[name]["need_grad"]:
        seen["bwd_rode"] = 0
    return plan, seen


project_bound = E.project_bound
margin_mask = E.margin_mask


def outputs_equal(a, b):
    """Names of the outputs of two runs that are not bit-identical."""
    bad = [k for k in ("logits", "loss_b", "preds", "acc_b") if not torch.equal(a[k], b[k])]
    if a["grads"] is not None:
        bad += [f"grad {i}" for i, (x, y) in enumerate(zip(a["grads"], b["grads"])) if not torch.equal(x, y)]
    return bad
