"""The form table of csrc/rn12_conv.hip shared by tests/test_rn12_conv_forms_cpu.py and tests/test_rn12_conv_forms_gpu.py -- TEST
INFRASTRUCTURE ONLY.

One row per case of the three products of the bf16 ResNet-12 (fwd: conv_bn's launch, dgrad: conv_plain's, wgrad: wgrad()'s), each the
smallest shape that reaches a kernel instance, a tile edge, a source combination or a reduce kernel, with the plan the launcher
reports for it when no knob is set (PLANS; the CPU suite holds it to the library's own host query).  Inputs, the float64 reference,
its float32 restatement and the exact-integer data are built here, on the CPU, once per row."""
import functools
import os
from collections import OrderedDict

import torch
import torch.nn.functional as TF

MAX_MACS = 1.2e8          # multiply-adds of any row (B x interior pixels x sum of Cin taps x Cout)
FP32_CAP = 1e-5           # dW and the statistics: of the reference's maximum (tests/test_resnet12_gpu.py)
E_FACTOR = 4.0            # allowance e = 4 x the largest deviation of a CPU float32 restatement from float64
GUARD = 1024              # elements of NaN before and after every buffer
SENTINEL = 0x7FC1         # bf16 bits every output map is pre-filled with (a NaN no product of finite data gives)

KNOBS = ("FUMI_RN_S16", "FUMI_RN_MW", "FUMI_RN_BKS", "FUMI_RN_XCD", "FUMI_RN_GLDS", "FUMI_RN_WSPLIT", "FUMI_RN_WSLOTS")
KNOB_SETTINGS = [{"FUMI_RN_S16": "0"}, {"FUMI_RN_MW": "1"}, {"FUMI_RN_MW": "2"}, {"FUMI_RN_BKS": "2"}, {"FUMI_RN_BKS": "4"},
                 {"FUMI_RN_XCD": "0"}, {"FUMI_RN_GLDS": "0"}, {"FUMI_RN_WSPLIT": "1"}, {"FUMI_RN_WSLOTS": "512"}]
SPEED_ONLY = ({"FUMI_RN_XCD": "0"}, {"FUMI_RN_GLDS": "0"})       # documented as placement / staging only: the default run's bits
CONV_KEYS = ("nf", "mw", "bks", "s16", "tiles", "tpi", "ncg", "xcd", "glds", "slab_rows", "lds")      # = hip.RN12_CONV_KEYS
WGRAD_KEYS = ("ntap", "nsplit", "ci_tiles", "co_tiles", "xcd", "reduce")                             # = hip.RN12_WGRAD_KEYS


def setting_id(s):
    return " ".join(f"{k}={v}" for k, v in s.items()) or "default"


def _c(pass_, B, M, H, W, Cout, srcs, dot=False, stats=None, chunk=False, xmax=2):
    """srcs: (Cin, ntaps, shared weights) per source.  dgrad: a source is a dy map of Cin channels and its weights are the forward
    layer's [Cin][Cout][k][k]."""
    stats = (pass_ == "fwd") if stats is None else stats
    return dict(pass_=pass_, B=B, M=M, H=H, W=W, Cout=Cout, srcs=[tuple(s) + (0,) * (3 - len(s)) for s in srcs], dot=dot, stats=stats,
                chunk=chunk, xmax=xmax)


def _w(B, M, H, W, Cin, Cin_real, Cout, ntaps, npair=1, nsplit=0, chunk=False):
    return dict(pass_="wgrad", B=B, M=M, H=H, W=W, Cin=Cin, Cin_real=Cin_real, Cout=Cout, ntaps=ntaps, npair=npair, nsplit=nsplit,
                chunk=chunk)


CASES = OrderedDict([
    # ---- every instance a launch takes with no knob set.  MW = 2 needs ceil(npix / 256) ncg RN_BREF >= 256: 16 129 padded pixels
    #      at one column group.  BKS = 4 while slab_rows 128 + 8 NF KiB fits half a CU's LDS less 256 bytes, else BKS = 2, else MW = 1.
    ("i_n1_m2_k4_s", _c("fwd", 1, 113, 10, 10, 32, [(32, 9)])),
    ("i_n1_m2_k4_n", _c("fwd", 1, 113, 10, 10, 32, [(16, 9)])),                  # the nine taps walked as k-steps on 256-pixel tiles
    ("i_n2_m2_k4_s", _c("fwd", 1, 113, 10, 10, 64, [(32, 1)])),
    ("i_n2_m2_k4_n", _c("fwd", 1, 113, 10, 10, 64, [(48, 1)])),
    ("i_n3_m2_k4_s", _c("dgrad", 1, 113, 10, 10, 96, [(32, 1)])),
    ("i_n3_m2_k4_n", _c("fwd", 1, 113, 10, 10, 96, [(16, 1)])),
    ("i_n4_m2_k4_s", _c("fwd", 1, 34, 20, 20, 128, [(64, 1)])),
    ("i_n4_m2_k4_n", _c("fwd", 1, 34, 20, 20, 128, [(48, 1)])),
    ("i_n1_m2_k2_s", _c("fwd", 1, 449, 4, 4, 32, [(32, 9)])),                    # slab of 576 rows: BKS = 4 no longer fits
    ("i_n1_m2_k2_n", _c("fwd", 1, 449, 4, 4, 32, [(16, 9)])),
    ("i_n2_m2_k2_s", _c("fwd", 1, 330, 5, 5, 64, [(32, 1)])),                    # 330 images of 5 x 5: every tile straddles ten
    ("i_n2_m2_k2_n", _c("fwd", 1, 330, 5, 5, 64, [(48, 1)])),
    ("i_n3_m2_k2_s", _c("fwd", 1, 253, 6, 6, 96, [(32, 1)])),
    ("i_n3_m2_k2_n", _c("fwd", 1, 253, 6, 6, 96, [(16, 1)])),
    ("i_n4_m2_k2_s", _c("dgrad", 1, 113, 10, 10, 128, [(32, 1)])),
    ("i_n4_m2_k2_n", _c("fwd", 1, 113, 10, 10, 128, [(80, 1)])),
    ("i_n5_m2_k2_s", _c("fwd", 1, 113, 10, 10, 160, [(32, 1)])),
    ("i_n5_m2_k2_n", _c("fwd", 1, 113, 10, 10, 160, [(48, 1)])),
    ("i_fall_m1", _c("fwd", 1, 1009, 2, 2, 32, [(32, 9)])),                      # enough tiles for MW = 2, but no slab of 2 x 2 maps fits
    # ---- pixel tile edges.  MT = 128: 127, 128, 129 interior pixels (t_255 / t_256 / t_257_1x1 likewise end one pixel short of,
    #      on, and one pixel past a 128-pixel tile; 129 and 257 end in a tile of ONE pixel; 257 maps of 1 x 1, which no slab of a
    #      256-pixel tile fits).  MT = 256 with no knob set (Cout = 224: ncg = 7): 9 tiles less one pixel, 5 whole tiles, 29 tiles and
    #      ONE pixel (t_m2_*), and per image 4 tiles and one pixel (p_1025_img_m2).  t_255 and t_256 are 256-pixel tiles under
    #      FUMI_RN_MW=2; 257 pixels (a prime: 1 x 257 or 257 x 1, a slab of 776 rows or more) fit no two-workgroup 256-pixel tile under any one knob.
    ("t_127", _c("fwd", 1, 1, 1, 127, 32, [(32, 9)])),
    ("t_128", _c("fwd", 1, 2, 8, 8, 32, [(32, 9)])),
    ("t_129", _c("fwd", 1, 1, 3, 43, 32, [(32, 9)])),
    ("t_255", _c("fwd", 1, 1, 15, 17, 32, [(32, 9)])),
    ("t_256", _c("dgrad", 1, 1, 16, 16, 32, [(32, 9)])),
    ("t_257_1x1", _c("fwd", 1, 257, 1, 1, 224, [(32, 9)])),
    ("t_m2_255", _c("fwd", 1, 7, 7, 47, 224, [(32, 1)])),                        # 2 303 = 9 x 256 - 1
    ("t_m2_256", _c("fwd", 1, 20, 2, 32, 224, [(32, 1)])),                       # 1 280 = 5 x 256
    ("t_m2_257", _c("fwd", 1, 33, 5, 45, 224, [(32, 1)])),                       # 7 425 = 29 x 256 + 1
    ("t_2x2_many", _c("fwd", 3, 50, 2, 2, 64, [(32, 9)], chunk=True)),
    ("t_5x5_many", _c("dgrad", 1, 21, 5, 5, 32, [(64, 9)])),
    # ---- both sides of rn_per_image (H W >= 4 MT): 511 flat / 529 per image with a last tile of 17 (5 tiles per image where the
    #      flat count says 4.88) at MT = 128; 1023 flat / 1024 per image at MT = 256
    ("p_511_flat", _c("fwd", 1, 2, 7, 73, 32, [(32, 9)])),
    ("p_529_img", _c("fwd", 3, 2, 23, 23, 32, [(32, 9)], chunk=True)),
    ("p_1023_flat_m2", _c("fwd", 1, 2, 31, 33, 224, [(32, 1)])),
    ("p_1024_img_m2", _c("fwd", 1, 2, 32, 32, 224, [(32, 1)])),
    ("p_1025_img_m2", _c("fwd", 1, 2, 25, 41, 224, [(32, 1)])),                  # five tiles per image, the last of ONE pixel
    # ---- channel chunks: Cin tails of 16, 32, 48 channels behind 0, 1, 2 and 5 whole chunks; Cout for NF 1..5, ncg 7 and 2
    ("c_16_32", _c("fwd", 3, 2, 6, 6, 32, [(16, 9)])),
    ("c_32_64", _c("fwd", 1, 2, 6, 6, 64, [(32, 9)])),
    ("c_48_96", _c("fwd", 1, 2, 6, 6, 96, [(48, 9)])),
    ("c_64_128", _c("fwd", 1, 2, 6, 6, 128, [(64, 9)])),
    ("c_80_160", _c("fwd", 1, 2, 6, 6, 160, [(80, 9)])),
    ("c_96_224", _c("fwd", 1, 2, 6, 6, 224, [(96, 9)])),
    ("c_160_320", _c("fwd", 1, 2, 6, 6, 320, [(160, 9)])),
    ("c_320_32", _c("fwd", 1, 2, 6, 6, 32, [(320, 9)])),
    ("c_320_32_1x1", _c("fwd", 1, 2, 6, 6, 32, [(320, 1)])),
    ("d_64_32", _c("dgrad", 1, 2, 6, 6, 32, [(64, 9)])),
    # (a backward copy exists only where both channel counts are multiples of 32: its 32x32x16 form runs under FUMI_RN_S16=0)
    ("d_96_64", _c("dgrad", 3, 2, 6, 6, 64, [(96, 9)])),
    ("c_80_128", _c("fwd", 1, 2, 6, 6, 128, [(80, 1)])),
    ("c_64_96", _c("fwd", 1, 2, 6, 6, 96, [(64, 9)])),
    ("d_320_160", _c("dgrad", 1, 1, 5, 5, 160, [(320, 9)])),
    # ---- sources, as the engine issues them: tangent forward (3x3 + 3x3 with `dot`), input gradient into a block (3x3 + 1x1),
    #      its tangent (3x3, 3x3, 1x1, 1x1); shared and per-episode weights; a launch whose sources select different MFMA forms
    ("s2_33_dot", _c("fwd", 8, 1, 5, 5, 32, [(64, 9), (64, 9, 1)], dot=True, chunk=True)),
    ("s2_11_dot", _c("fwd", 3, 2, 6, 6, 64, [(32, 1, 1), (32, 1)], dot=True)),
    ("s2_31", _c("dgrad", 3, 2, 6, 6, 32, [(64, 9), (64, 1)], chunk=True)),
    ("s4_3311", _c("dgrad", 3, 2, 6, 6, 32, [(64, 9), (64, 9, 1), (64, 1), (64, 1, 1)])),
    ("s4_3311_stats", _c("dgrad", 1, 2, 6, 6, 64, [(32, 9), (32, 9), (32, 1), (32, 1)], stats=True)),
    ("s2_mixed_cin", _c("fwd", 3, 2, 6, 6, 32, [(64, 9), (48, 1)], dot=True)),   # 48 % 32 != 0: the whole launch on 32x32x16
    ("s3_mixed_cin", _c("fwd", 1, 2, 6, 6, 64, [(16, 9), (96, 9, 1), (32, 1)])),
    # ---- episodes: groups = ncg B of 1, 3, 8 (XCD-grouped ids), 12 (not a multiple of 8), 16 (ncg = 2)
    ("e_b8", _c("fwd", 8, 2, 6, 6, 32, [(32, 9)], chunk=True)),
    ("e_b12", _c("fwd", 12, 1, 5, 5, 32, [(32, 9)], chunk=True)),
    ("e_b8_ncg2", _c("fwd", 8, 1, 5, 5, 320, [(32, 1)], chunk=True)),
    ("e_b8_dgrad", _c("dgrad", 8, 1, 5, 5, 32, [(32, 9)], chunk=True)),
    # ---- weight gradient: NTAP 9 / 1, the padded image layer, Ci32 != Cin, partial 64-wide tiles, one and two pairs, the three reduces
    ("w_img_3of16", _w(2, 3, 10, 10, 16, 3, 64, 9)),
    ("w_48_96_pair", _w(1, 4, 7, 7, 48, 48, 96, 9, npair=2)),
    ("w_64_32_1x1", _w(3, 2, 6, 6, 64, 64, 32, 1, chunk=True)),
    ("w_48_96_1x1_pair", _w(1, 4, 7, 7, 48, 48, 96, 1, npair=2)),
    ("w_split9", _w(1, 9, 10, 10, 96, 96, 96, 9)),                               # 1 296 pixels: not a multiple of 128 nsplit
    ("w_split1x1_b8", _w(8, 9, 10, 10, 96, 96, 96, 1, chunk=True)),
    ("w_b8_9", _w(8, 2, 6, 6, 32, 32, 32, 9, npair=2, chunk=True)),
    ("w_1x1_split3", _w(1, 9, 10, 10, 32, 32, 32, 1, nsplit=3)),
    ("w_1x1_split16", _w(3, 20, 10, 10, 32, 32, 32, 1, nsplit=16, chunk=True)),  # 23 stages on 16 slabs: four slabs stay empty
    ("w_1x1_split17_pair", _w(1, 20, 10, 10, 160, 160, 96, 1, npair=2, nsplit=17)),
    ("w_knobs", _w(1, 25, 10, 10, 32, 32, 32, 1)),                               # 29 stages: 6 slabs, 8 under FUMI_RN_WSPLIT=1, 4 under FUMI_RN_WSLOTS=512
    ("w_160_160", _w(1, 2, 6, 6, 160, 160, 160, 9)),
    ("w_1pix", _w(1, 1, 1, 1, 32, 32, 32, 9)),
])
ALL_CASES = list(CASES)
CONV_CASES = [n for n, c in CASES.items() if c["pass_"] != "wgrad"]
WGRAD_CASES = [n for n, c in CASES.items() if c["pass_"] == "wgrad"]
SEEDS = {n: 9100 + i for i, n in enumerate(CASES)}


def npix(c):
    return c["M"] * (c["H"] + 2) * (c["W"] + 2)


def macs(c):
    n = c["B"] * c["M"] * c["H"] * c["W"]
    if c["pass_"] == "wgrad":
        return n * c["Cin"] * c["Cout"] * c["ntaps"] * c["npair"]
    return n * c["Cout"] * sum(ci * t for ci, t, _ in c["srcs"])


# ---- the instances of rn_conv_kernel<NF, MW, BKS, S16> conv_tile_shape / rn_conv_plan can choose ------------------------------------
def instance(plan):
    return "rn_conv_kernel<%d,%d,%d,%s>" % (plan["nf"], plan["mw"], plan["bks"], "true" if plan["s16"] else "false")


# no knob: 256-pixel tiles with 4-k-step weight tiles (never at NF = 5) or 2-k-step ones, 128-pixel tiles with 4-k-step ones
DEFAULT_INSTANCES = {"rn_conv_kernel<%d,%d,%d,%s>" % (nf, mw, bks, s) for nf in range(1, 6) for s in ("true", "false")
                     for mw, bks in ((2, 4), (2, 2), (1, 4)) if not (nf == 5 and (mw, bks) == (2, 4))}
# FUMI_RN_BKS=2 adds the 128-pixel tiles with 2-k-step weight tiles, FUMI_RN_BKS=4 the NF = 5 tile with 4-k-step ones
INSTANCES = {"rn_conv_kernel<%d,%d,%d,%s>" % (nf, mw, bks, s) for nf in range(1, 6) for s in ("true", "false") for mw in (1, 2)
             for bks in (2, 4)}
WGRAD_INSTANCES = {(9, 3), (1, 1), (1, 2)}           # (NTAP, reduce kernel)


def query(name, hip, B=None):
    """The library's host query for a row under this process's knobs (no GPU)."""
    c = CASES[name]
    B = c["B"] if B is None else B
    if c["pass_"] == "wgrad":
        return hip.rn12_wgrad_query(B, c["M"], c["H"], c["W"], c["Cin"], c["Cout"], c["ntaps"], c["npair"], c["nsplit"])
    return hip.rn12_conv_query(B, c["M"], c["H"], c["W"], c["Cout"], [s[0] for s in c["srcs"]])


# ---- layout -----------------------------------------------------------------------------------------------------------------------
def to_cl(x):
    """[B, M, C, H, W] -> padded channels-last [B, M (H+2) (W+2), C] with a zero border."""
    B, M, C, H, W = x.shape
    return TF.pad(x, (1, 1, 1, 1)).permute(0, 1, 3, 4, 2).reshape(B, M * (H + 2) * (W + 2), C).contiguous()


def from_cl(y, M, H, W):
    """[B, npix, C] -> [B, M, C, H+2, W+2]."""
    B, _, C = y.shape
    return y.reshape(B, M, H + 2, W + 2, C).permute(0, 1, 4, 2, 3)


def interior_mask(M, H, W):
    m = torch.zeros(M, H + 2, W + 2, dtype=torch.bool)
    m[:, 1:-1, 1:-1] = True
    return m.reshape(-1)


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _wshape(c, s):
    cin, taps, _ = c["srcs"][s]
    k = 3 if taps == 9 else 1
    return (cin, c["Cout"], k, k) if c["pass_"] == "dgrad" else (c["Cout"], cin, k, k)


def _sparse_weights(c, g):
    """+-1 weights, one output channel per (source, tap, input channel) position: the union over the output channels touches every
    position, and an output element is a sum of at most ceil(positions / Cout) terms of size <= xmax."""
    B, Cout = c["B"], c["Cout"]
    out, j = [], int(torch.randint(0, Cout, (1,), generator=g))
    for s, (cin, taps, shared) in enumerate(c["srcs"]):
        k = 3 if taps == 9 else 1
        nb = 1 if shared else B
        w = torch.zeros(nb, Cout, cin, k * k)
        for b in range(nb):
            pos = torch.arange(cin * k * k)
            co = (pos * 11 + j + 3 * b) % Cout
            sign = torch.randint(0, 2, (cin * k * k,), generator=g) * 2.0 - 1.0
            w[b, co, pos // (k * k), pos % (k * k)] = sign
        j += cin * k * k * 11
        w = w.reshape(nb, Cout, cin, k, k)
        if c["pass_"] == "dgrad":                    # stored as the forward layer's [Cin][Cout][k][k]: out = conv(dy, flip(W)^T)
            w = w.flip(3, 4).transpose(1, 2).contiguous()
        out.append(w)
    return out


@functools.lru_cache(maxsize=None)
def make_inputs(name, kind):
    """kind "gauss": bf16-rounded Gaussian maps and weights of unit output variance; "int": small integers, exact in bf16 (module
    docstring).  Maps as [B, M, C, H, W] float32; weights per source [B or 1, ...] float32.  Never modified."""
    c = CASES[name]
    g = torch.Generator().manual_seed(SEEDS[name] + (0 if kind == "gauss" else 50000))
    B, M, H, W = c["B"], c["M"], c["H"], c["W"]
    if c["pass_"] == "wgrad":
        n = c["npair"]
        if kind == "gauss":
            x = [bf(torch.randn(B, M, c["Cin"], H, W, generator=g)) for _ in range(n)]
            dy = [bf(torch.randn(B, M, c["Cout"], H, W, generator=g)) for _ in range(n)]
        else:
            x = [torch.randint(-2, 3, (B, M, c["Cin"], H, W), generator=g).float() for _ in range(n)]
            dy = [torch.randint(-2, 3, (B, M, c["Cout"], H, W), generator=g).float() for _ in range(n)]
        return dict(x=x, dy=dy)
    xs, ws = [], []
    fan = sum(ci * t for ci, t, _ in c["srcs"])
    if kind == "int":
        ws = _sparse_weights(c, g)
    for s, (cin, taps, shared) in enumerate(c["srcs"]):
        if kind == "gauss":
            xs.append(bf(torch.randn(B, M, cin, H, W, generator=g)))
            ws.append(bf(torch.randn((1 if shared else B,) + _wshape(c, s), generator=g) / fan ** 0.5))
        else:
            xs.append(torch.randint(-c["xmax"], c["xmax"] + 1, (B, M, cin, H, W), generator=g).float())
    d = dict(x=xs, w=ws, dot=None)
    if c["dot"]:
        d["dot"] = bf(torch.randn(B, M, c["Cout"], H, W, generator=g)) if kind == "gauss" else \
            torch.randint(-2, 3, (B, M, c["Cout"], H, W), generator=g).float()
    return d


# ---- references ---------------------------------------------------------------------------------------------------------------------
def conv_bwd_weight(x, dy, k):
    """oracle/resnet12_manual.py's conv_bwd_weight: dW[o][i][ky][kx] = sum dy[m][o][h][w] x[m][i][h + ky - 1][w + kx - 1]."""
    from oracle import resnet12_manual as RM
    return RM.conv_bwd_weight(x, dy, k)


def reference(name, d, dtype=torch.float64, absolute=False):
    """conv rows: y [B, M, Cout, H, W] = sum over the sources of F.conv2d; wgrad rows: dW [B, Cout, Cin_real, k, k] = sum over the
    pairs.  absolute: the same sum over the absolute values of the terms (the exactness condition of the integer data)."""
    c = CASES[name]
    a = (lambda t: t.abs()) if absolute else (lambda t: t)
    if c["pass_"] == "wgrad":
        k = 3 if c["ntaps"] == 9 else 1
        out = 0
        for x, dy in zip(d["x"], d["dy"]):
            out = out + torch.stack([conv_bwd_weight(a(x[b]).to(dtype), a(dy[b]).to(dtype), k) for b in range(c["B"])])
        return out[:, :, :c["Cin_real"]].contiguous()
    y = 0
    for s, (cin, taps, shared) in enumerate(c["srcs"]):
        x, w = a(d["x"][s]).to(dtype), a(d["w"][s]).to(dtype)
        if c["pass_"] == "dgrad":
            w = w.flip(3, 4).transpose(1, 2)
        y = y + torch.stack([TF.conv2d(x[b], w[0 if shared else b], None, padding=taps // 9) for b in range(c["B"])])
    return y


def stats_of(y, dot):
    """[B, 2, C]: per-channel sum of y and of y * dot (dot None: y * y) over images and pixels, in y's dtype."""
    return torch.stack([y.sum((1, 3, 4)), (y * (y if dot is None else dot.to(y.dtype))).sum((1, 3, 4))], 1)


@functools.lru_cache(maxsize=None)
def gauss_reference(name):
    """(float64 reference, e32) of the Gaussian data: e32 is the largest deviation of the float32 restatement (CPU torch float32 on
    the same inputs) from float64; the allowance of the GPU suite is E_FACTOR x e32."""
    d = make_inputs(name, "gauss")
    r64 = reference(name, d, torch.float64)
    r32 = reference(name, d, torch.float32)
    return r64, float((r32.double() - r64).abs().max())


@functools.lru_cache(maxsize=None)
def int_reference(name):
    return reference(name, make_inputs(name, "int"), torch.float64)


def bracket(r64, e):
    """RNE-bf16(r - e), RNE-bf16(r + e) as float64 (through float32, as the engine rounds: module docstring of the GPU suite)."""
    lo = (r64 - e).float().to(torch.bfloat16).double()
    hi = (r64 + e).float().to(torch.bfloat16).double()
    return lo, hi


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


# ---- what the default process reports per row (generated from the host query; test_rn12_conv_forms_cpu.py holds it to the query) ----
# E32: the measured float32-restatement deviation per row (gauss_reference) at the time the table was written.
PLANS = {
    'i_n1_m2_k4_s': {'nf': 1, 'mw': 2, 'bks': 4, 's16': 1, 'tiles': 45, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 408, 'lds': 60432},
    'i_n1_m2_k4_n': {'nf': 1, 'mw': 2, 'bks': 4, 's16': 0, 'tiles': 45, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 408, 'lds': 60432},
    'i_n2_m2_k4_s': {'nf': 2, 'mw': 2, 'bks': 4, 's16': 1, 'tiles': 45, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 408, 'lds': 68624},
    'i_n2_m2_k4_n': {'nf': 2, 'mw': 2, 'bks': 4, 's16': 0, 'tiles': 45, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 408, 'lds': 68624},
    'i_n3_m2_k4_s': {'nf': 3, 'mw': 2, 'bks': 4, 's16': 1, 'tiles': 45, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 408, 'lds': 76816},
    'i_n3_m2_k4_n': {'nf': 3, 'mw': 2, 'bks': 4, 's16': 0, 'tiles': 45, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 408, 'lds': 76816},
    'i_n4_m2_k4_s': {'nf': 4, 'mw': 2, 'bks': 4, 's16': 1, 'tiles': 54, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 376, 'lds': 80912},
    'i_n4_m2_k4_n': {'nf': 4, 'mw': 2, 'bks': 4, 's16': 0, 'tiles': 54, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 376, 'lds': 80912},
    'i_n1_m2_k2_s': {'nf': 1, 'mw': 2, 'bks': 2, 's16': 1, 'tiles': 29, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 576, 'lds': 77840},
    'i_n1_m2_k2_n': {'nf': 1, 'mw': 2, 'bks': 2, 's16': 0, 'tiles': 29, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 576, 'lds': 77840},
    'i_n2_m2_k2_s': {'nf': 2, 'mw': 2, 'bks': 2, 's16': 1, 'tiles': 33, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 528, 'lds': 75792},
    'i_n2_m2_k2_n': {'nf': 2, 'mw': 2, 'bks': 2, 's16': 0, 'tiles': 33, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 528, 'lds': 75792},
    'i_n3_m2_k2_s': {'nf': 3, 'mw': 2, 'bks': 2, 's16': 1, 'tiles': 36, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 472, 'lds': 72720},
    'i_n3_m2_k2_n': {'nf': 3, 'mw': 2, 'bks': 2, 's16': 0, 'tiles': 36, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 472, 'lds': 72720},
    'i_n4_m2_k2_s': {'nf': 4, 'mw': 2, 'bks': 2, 's16': 1, 'tiles': 45, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 408, 'lds': 68624},
    'i_n4_m2_k2_n': {'nf': 4, 'mw': 2, 'bks': 2, 's16': 0, 'tiles': 45, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 408, 'lds': 68624},
    'i_n5_m2_k2_s': {'nf': 5, 'mw': 2, 'bks': 2, 's16': 1, 'tiles': 45, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 408, 'lds': 72720},
    'i_n5_m2_k2_n': {'nf': 5, 'mw': 2, 'bks': 2, 's16': 0, 'tiles': 45, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 408, 'lds': 72720},
    'i_fall_m1': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 32, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 512, 'lds': 73744},
    't_127': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 648, 'lds': 91152},
    't_128': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 200, 'lds': 33808},
    't_129': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 2, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 320, 'lds': 49168},
    't_255': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 2, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 224, 'lds': 36880},
    't_256': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 2, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 184, 'lds': 31760},
    't_257_1x1': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 3, 'tpi': 0, 'ncg': 7, 'xcd': 0, 'glds': 1, 'slab_rows': 1152, 'lds': 155664},
    't_m2_255': {'nf': 1, 'mw': 2, 'bks': 4, 's16': 1, 'tiles': 9, 'tpi': 0, 'ncg': 7, 'xcd': 0, 'glds': 1, 'slab_rows': 472, 'lds': 68624},
    't_m2_256': {'nf': 1, 'mw': 2, 'bks': 4, 's16': 1, 'tiles': 5, 'tpi': 0, 'ncg': 7, 'xcd': 0, 'glds': 1, 'slab_rows': 544, 'lds': 77840},
    't_m2_257': {'nf': 1, 'mw': 2, 'bks': 4, 's16': 1, 'tiles': 30, 'tpi': 0, 'ncg': 7, 'xcd': 0, 'glds': 1, 'slab_rows': 552, 'lds': 78864},
    't_2x2_many': {'nf': 2, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 2, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 512, 'lds': 81936},
    't_5x5_many': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 5, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 280, 'lds': 44048},
    'p_511_flat': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 8, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 440, 'lds': 64528},
    'p_529_img': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 10, 'tpi': 5, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 192, 'lds': 32784},
    'p_1023_flat_m2': {'nf': 1, 'mw': 2, 'bks': 4, 's16': 1, 'tiles': 8, 'tpi': 0, 'ncg': 7, 'xcd': 0, 'glds': 1, 'slab_rows': 416, 'lds': 61456},
    'p_1024_img_m2': {'nf': 1, 'mw': 2, 'bks': 4, 's16': 1, 'tiles': 8, 'tpi': 4, 'ncg': 7, 'xcd': 0, 'glds': 1, 'slab_rows': 344, 'lds': 52240},
    'p_1025_img_m2': {'nf': 1, 'mw': 2, 'bks': 4, 's16': 1, 'tiles': 10, 'tpi': 5, 'ncg': 7, 'xcd': 0, 'glds': 1, 'slab_rows': 360, 'lds': 54288},
    'c_16_32': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 0, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 40976},
    'c_32_64': {'nf': 2, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 49168},
    'c_48_96': {'nf': 3, 'mw': 1, 'bks': 4, 's16': 0, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 57360},
    'c_64_128': {'nf': 4, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 65552},
    'c_80_160': {'nf': 5, 'mw': 1, 'bks': 4, 's16': 0, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 73744},
    'c_96_224': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 7, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 40976},
    'c_160_320': {'nf': 5, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 2, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 73744},
    'c_320_32': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 40976},
    'c_320_32_1x1': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 40976},
    'd_64_32': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 40976},
    'd_96_64': {'nf': 2, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 49168},
    'c_80_128': {'nf': 4, 'mw': 1, 'bks': 4, 's16': 0, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 65552},
    'c_64_96': {'nf': 3, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 57360},
    'd_320_160': {'nf': 5, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 280, 'lds': 76816},
    's2_33_dot': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 1, 'glds': 1, 'slab_rows': 280, 'lds': 44048},
    's2_11_dot': {'nf': 2, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 49168},
    's2_31': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 40976},
    's4_3311': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 40976},
    's4_3311_stats': {'nf': 2, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 49168},
    's2_mixed_cin': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 0, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 40976},
    's3_mixed_cin': {'nf': 2, 'mw': 1, 'bks': 4, 's16': 0, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 256, 'lds': 49168},
    'e_b8': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 1, 'glds': 1, 'slab_rows': 256, 'lds': 40976},
    'e_b12': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 0, 'glds': 1, 'slab_rows': 280, 'lds': 44048},
    'e_b8_ncg2': {'nf': 5, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 2, 'xcd': 1, 'glds': 1, 'slab_rows': 280, 'lds': 76816},
    'e_b8_dgrad': {'nf': 1, 'mw': 1, 'bks': 4, 's16': 1, 'tiles': 1, 'tpi': 0, 'ncg': 1, 'xcd': 1, 'glds': 1, 'slab_rows': 280, 'lds': 44048},
    'w_img_3of16': {'ntap': 9, 'nsplit': 1, 'ci_tiles': 1, 'co_tiles': 1, 'xcd': 0, 'reduce': 3},
    'w_48_96_pair': {'ntap': 9, 'nsplit': 1, 'ci_tiles': 1, 'co_tiles': 2, 'xcd': 0, 'reduce': 3},
    'w_64_32_1x1': {'ntap': 1, 'nsplit': 1, 'ci_tiles': 1, 'co_tiles': 1, 'xcd': 0, 'reduce': 1},
    'w_48_96_1x1_pair': {'ntap': 1, 'nsplit': 1, 'ci_tiles': 1, 'co_tiles': 2, 'xcd': 0, 'reduce': 1},
    'w_split9': {'ntap': 9, 'nsplit': 2, 'ci_tiles': 2, 'co_tiles': 2, 'xcd': 0, 'reduce': 3},
    'w_split1x1_b8': {'ntap': 1, 'nsplit': 2, 'ci_tiles': 2, 'co_tiles': 2, 'xcd': 1, 'reduce': 1},
    'w_b8_9': {'ntap': 9, 'nsplit': 1, 'ci_tiles': 1, 'co_tiles': 1, 'xcd': 1, 'reduce': 3},
    'w_1x1_split3': {'ntap': 1, 'nsplit': 3, 'ci_tiles': 1, 'co_tiles': 1, 'xcd': 0, 'reduce': 1},
    'w_1x1_split16': {'ntap': 1, 'nsplit': 16, 'ci_tiles': 1, 'co_tiles': 1, 'xcd': 1, 'reduce': 2},
    'w_1x1_split17_pair': {'ntap': 1, 'nsplit': 17, 'ci_tiles': 3, 'co_tiles': 2, 'xcd': 0, 'reduce': 2},
    'w_knobs': {'ntap': 1, 'nsplit': 6, 'ci_tiles': 1, 'co_tiles': 1, 'xcd': 0, 'reduce': 1},
    'w_160_160': {'ntap': 9, 'nsplit': 1, 'ci_tiles': 3, 'co_tiles': 3, 'xcd': 0, 'reduce': 3},
    'w_1pix': {'ntap': 9, 'nsplit': 1, 'ci_tiles': 1, 'co_tiles': 1, 'xcd': 0, 'reduce': 3},
}
E32 = {
    'i_n1_m2_k4_s': 8.643e-07,
    'i_n1_m2_k4_n': 9.388e-07,
    'i_n2_m2_k4_s': 4.768e-07,
    'i_n2_m2_k4_n': 6.482e-07,
    'i_n3_m2_k4_s': 7.898e-07,
    'i_n3_m2_k4_n': 5.960e-07,
    'i_n4_m2_k4_s': 7.749e-07,
    'i_n4_m2_k4_n': 9.239e-07,
    'i_n1_m2_k2_s': 8.522e-07,
    'i_n1_m2_k2_n': 8.047e-07,
    'i_n2_m2_k2_s': 5.960e-07,
    'i_n2_m2_k2_n': 6.929e-07,
    'i_n3_m2_k2_s': 7.451e-07,
    'i_n3_m2_k2_n': 4.768e-07,
    'i_n4_m2_k2_s': 6.575e-07,
    'i_n4_m2_k2_n': 9.425e-07,
    'i_n5_m2_k2_s': 6.240e-07,
    'i_n5_m2_k2_n': 9.984e-07,
    'i_fall_m1': 3.576e-07,
    't_127': 2.719e-07,
    't_128': 6.449e-07,
    't_129': 8.484e-07,
    't_255': 8.717e-07,
    't_256': 8.717e-07,
    't_257_1x1': 1.080e-07,
    't_m2_255': 7.153e-07,
    't_m2_256': 5.811e-07,
    't_m2_257': 6.855e-07,
    't_2x2_many': 3.576e-07,
    't_5x5_many': 4.191e-07,
    'p_511_flat': 6.370e-07,
    'p_529_img': 9.090e-07,
    'p_1023_flat_m2': 4.768e-07,
    'p_1024_img_m2': 4.768e-07,
    'p_1025_img_m2': 5.215e-07,
    'c_16_32': 6.557e-07,
    'c_32_64': 4.321e-07,
    'c_48_96': 5.111e-07,
    'c_64_128': 6.016e-07,
    'c_80_160': 6.612e-07,
    'c_96_224': 6.189e-07,
    'c_160_320': 4.927e-07,
    'c_320_32': 5.981e-07,
    'c_320_32_1x1': 8.591e-07,
    'd_64_32': 3.707e-07,
    'd_96_64': 5.921e-07,
    'c_80_128': 5.588e-07,
    'c_64_96': 4.610e-07,
    'd_320_160': 5.310e-07,
    's2_33_dot': 5.856e-07,
    's2_11_dot': 3.465e-07,
    's2_31': 4.773e-07,
    's4_3311': 6.391e-07,
    's4_3311_stats': 4.276e-07,
    's2_mixed_cin': 5.443e-07,
    's3_mixed_cin': 5.671e-07,
    'e_b8': 6.631e-07,
    'e_b12': 1.069e-06,
    'e_b8_ncg2': 4.172e-07,
    'e_b8_dgrad': 8.643e-07,
    'w_img_3of16': 1.287e-05,
    'w_48_96_pair': 1.186e-05,
    'w_64_32_1x1': 3.844e-06,
    'w_48_96_1x1_pair': 1.115e-05,
    'w_split9': 3.278e-05,
    'w_split1x1_b8': 2.668e-05,
    'w_b8_9': 4.709e-06,
    'w_1x1_split3': 1.189e-05,
    'w_1x1_split16': 2.660e-05,
    'w_1x1_split17_pair': 4.204e-05,
    'w_knobs': 2.451e-05,
    'w_160_160': 5.722e-06,
    'w_1pix': 0.000e+00,
}
