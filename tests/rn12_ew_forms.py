"""The form table of csrc/rn12_ew.hip shared by tests/test_rn12_ew_forms_cpu.py and tests/test_rn12_ew_forms_gpu.py -- TEST
INFRASTRUCTURE ONLY.

Three tables.  MAPS: one row per map shape; every row runs every pass that takes a map (act, BN backward reduce / apply, join forward
/ reduce / apply, plain and tangent) unless `only` names a subset.  COEFS: the coefficient pass on synthetic partial sums with
caller-given slab counts, slices and strides.  POOLS / PREPS: the average pool with its adjoint and the image prep.  Each row names
the plan it is there to reach (`why`; plan_of restates the arithmetic and the CPU suite holds it to the library's host query).  Inputs and references are built here, on the
CPU, once per row: `int` data whose every sum is an exact integer (the engine must equal it bit for bit) and `gauss` data (bf16-rounded
Gaussians and a random fp32 coefficient table, repaired so that no LeakyReLU argument and no pooling decision is near a tie)."""
import functools
from collections import OrderedDict

import torch

import rn12_ew_ref as R

E_FACTOR = 4.0            # allowance = 4 x the deviation of the CPU float32 restatement from float64 (DESIGN.md section 28's margin)
TIE_FACTOR = 64.0         # every LeakyReLU argument and every top-two gap of a window exceeds 64 x the row's allowance ...
TIE_FLOOR = 2.0 ** -8     # ... because the inputs are repaired until they exceed this, and the suites assert 64 e below it
GUARD = 1024              # elements of NaN before and after every buffer
SENTINEL = 0x7FC1         # bf16 bits every output map is pre-filled with (a NaN no finite data gives)
EW_KEYS = ("nch", "nrg", "active", "unit", "rb", "nt", "map_rb", "wb", "ncy", "ncx", "cb", "cell", "first", "nt2", "lds", "gx", "gy")

PLAIN = ("act", "red", "du", "jf", "jred", "ja3", "jas")
ALL_OUT = PLAIN + tuple(k + "_t" for k in PLAIN)
BF16_OUT = {"act", "du", "jf", "ja3", "jas"}
KIND_OF = {"act": "act", "red": "bwd_reduce", "du": "bwd_apply", "jf": "join_fwd", "jred": "join_reduce", "ja3": "join_apply",
           "jas": "join_apply"}


def _m(B, M, H, W, C, why, gauss=True, chunk=False, only=None):
    return dict(B=B, M=M, H=H, W=W, C=C, why=why, gauss=gauss, chunk=chunk, only=only)


MAPS = OrderedDict([
    # ---- channels: nch = C / 8 chunks, nrg = 256 / nch pixel groups; the join sizes of the issue ride on them
    ("c16_5x8", _m(1, 3, 5, 8, 16, "nrg 128; 210 pixels < one workgroup's 1024 of a map pass; 5 x 8: an uncovered last row")),
    ("c32_5x5_b3", _m(3, 2, 5, 5, 32, "nrg 64; B = 3; odd map: uncovered last row and column", chunk=True)),
    ("c64_14x9", _m(1, 9, 14, 9, 64, "nrg 32, all threads; 1584 pixels: not a multiple of 256, of 128 (UNR 4), of 64 (UNR 2) or of rb 64")),
    ("c96_3x3", _m(1, 2, 3, 3, 96, "nch 12, nrg 21: 4 idle threads")),
    ("c160_2x2_b8", _m(8, 2, 2, 2, 160, "nrg 12, 240 active; B = 8; 2 x 2: one window per image", chunk=True)),
    ("c320_5x5", _m(1, 5, 5, 5, 320, "nrg 6")),
    ("c640_21x21", _m(1, 1, 21, 21, 640, "nrg 3; one image: no window straddles anything; 21 x 21")),
    ("c2048_3x3", _m(1, 2, 3, 3, 2048, "nrg 1: the widest map; LDS of the tangent join reduce 40 960")),
    # ---- slabs of the reductions (rb = clamp(npix / 512, 64, 1024), nt = ceil(npix / rb)) and what the coefficient pass does behind
    ("nt1_5x5", _m(1, 1, 5, 5, 16, "49 pixels: nt = 1, a partial only slab")),
    ("nt3_5x7", _m(1, 3, 5, 7, 16, "189 pixels: nt = 3 < the four thread groups of the coefficient kernel; slabs straddle images")),
    ("nt128", _m(1, 8, 30, 30, 16, "8192 pixels: nt = 128, the longest single-stage list")),
    ("nt129", _m(1, 1, 80, 98, 16, "8200 pixels: nt = 129, a last slab of 8 pixels; first stage with a last group of ONE slab")),
    ("nt144", _m(1, 9, 30, 30, 16, "9216 pixels: nt = 144, groups of 64, 64, 16")),
    ("idle_3x3", _m(1, 40, 3, 3, 32, "40 windows on nt = 16 workgroups: wb = 3, 14 workgroups used, the last with ONE window, 2 idle")),
    ("rb_mid", _m(1, 40, 29, 31, 16, "40 920 pixels: rb = 79 (npix / 512 = 79.9), nt = 518, last slab 77; groups 8 x 64 + 6", gauss=False)),
    ("rb_cap", _m(1, 512, 30, 30, 16, "524 288 pixels: the first point of the 1024 cap, nt = 512 (exact rows of the reductions only)",
                  gauss=False, only=("red", "jred"))),
])


def _k(B, C, nt, K, ks, mode, why, scratch=True, pad=24, like=None):
    """like: the row whose data this row shares."""
    return dict(B=B, C=C, nt=nt, K=K, ks=ks, mode=mode, why=why, scratch=scratch, pad=pad, like=like)


COEFS = OrderedDict([
    # (slices as the engine passes them: conv statistics K = 2 (0, 1); join K = 3: BN3 (0, 1), BNs (0, 2); tangent join K = 5: BN3
    #  (0, 1, 2), BNs (0, 3, 4); tangent BN backward K = 3 (0, 1, 2))
    ("k_nt1_fwd", _k(1, 16, 1, 2, (0, 1, 0), "fwd", "one slab: three of the four thread groups add nothing")),
    ("k_nt3_bwd_s", _k(3, 96, 3, 3, (0, 2, 0), "bwd", "three slabs; BNs' slices of the join; C = 96: a second, half-empty 64-channel block")),
    ("k_nt128_fwd", _k(1, 16, 128, 2, (0, 1, 0), "fwd", "the longest single-stage list")),
    ("k_nt129_tbwd_s", _k(2, 24, 129, 5, (0, 3, 4), "tbwd", "first stage, last group of one slab; K C = 120: not a multiple of 64")),
    ("k_nt129_noscratch", _k(2, 24, 129, 5, (0, 3, 4), "tbwd", "the same list and data without scratch: the single stage", scratch=False,
                              like="k_nt129_tbwd_s")),
    ("k_nt144_bwd_3", _k(1, 160, 144, 3, (0, 1, 0), "bwd", "groups 64, 64, 16; C = 160; BN3's slices of the join")),
    ("k_nt512_tfwd", _k(2, 16, 512, 2, (0, 1, 0), "tfwd", "the cap row's 512 slabs: eight whole groups")),
    ("k_nt144_tbwd_3", _k(1, 32, 144, 5, (0, 1, 2), "tbwd", "BN3's slices of the tangent join")),
    ("k_nt2167_fwd", _k(3, 64, 2167, 2, (0, 1, 0), "fwd", "the slab count of block 0's query maps: 33 groups and one of 55")),
    ("k_nt130_tbwd_bn", _k(1, 96, 130, 3, (0, 1, 2), "tbwd", "tangent BN backward's K = 3; C = 96 in the first stage: K C = 288")),
])

POOLS = OrderedDict([("p64_1x1", (3, 1, 1, 64)), ("p320_5x5", (2, 5, 5, 320)), ("p640_5x3", (3, 5, 3, 640))])     # (BM, H, W, C)
PREPS = OrderedDict([("i1", (3, 1, 5, 4)), ("i3", (5, 3, 7, 6)), ("i8", (2, 8, 3, 3))])                            # (BM, Cin, H, W)

SEEDS = {n: 4800 + i for i, n in enumerate(list(MAPS) + list(COEFS) + list(POOLS) + list(PREPS))}


def outputs_of(name):
    c = MAPS[name]
    if c["only"]:
        return tuple(c["only"])
    return ALL_OUT


def query(name, hip, key, B=None):
    """the library's plan of the launch behind output `key` of a MAPS row."""
    c = MAPS[name]
    base = key[:-2] if key.endswith("_t") else key
    return hip.rn12_ew_query(B or c["B"], c["M"], c["H"], c["W"], c["C"], KIND_OF[base], key.endswith("_t"))


def plan_of(name):
    """The plan arithmetic of rn_ew_plan restated from the kernels' comments (the CPU suite holds it to the query): what the row's
    launches must decide."""
    c = MAPS[name]
    Pp = (c["H"] + 2) * (c["W"] + 2)
    npix = c["M"] * Pp
    nch = c["C"] // 8
    nrg = 256 // nch
    rb = min(max(npix // 512, 64), 1024)
    nt = -(-npix // rb)
    nwin = c["M"] * (c["H"] // 2) * (c["W"] // 2)
    ncy, ncx = (c["H"] + 2) // 2 + 1, (c["W"] + 2) // 2 + 1
    return dict(nch=nch, nrg=nrg, active=nch * nrg, rb=rb, nt=nt, first=int(nt > 128), nt2=-(-nt // 64) if nt > 128 else nt,
                map_rb=8 * nrg, wb=-(-nwin // nt), ncy=ncy, ncx=ncx, cb=4 * nrg, npix=npix, nwin=nwin, ncell=c["M"] * ncy * ncx)


# the five plans of the configs[4] shape (4 episodes per chunk; 100 support and 300 query images; maps of 84, 42, 21, 10 pixels at 64,
# 160, 320, 640 channels and the pooled 5 x 5 map): recorded values, asserted on the CPU only
PRODUCTION = [
    # (M, H, C, kind, tangent): (rb, nt, first, nt2, map_rb | wb | cb, lds, gx)
    ((100, 84, 64, "bwd_reduce", 1), dict(rb=1024, nt=723, first=1, nt2=12, lds=24576, gx=723)),
    ((300, 84, 64, "bwd_reduce", 1), dict(rb=1024, nt=2167, first=1, nt2=34, lds=24576, gx=2167)),
    ((300, 84, 64, "join_reduce", 1), dict(nt=2167, wb=245, lds=40960, gx=2167)),
    ((300, 84, 64, "join_apply", 0), dict(ncy=44, ncx=44, cb=128, cell=0, gx=4538)),
    ((300, 84, 64, "join_apply", 1), dict(cell=1, unit=1, gx=18150)),
    ((300, 84, 64, "act", 0), dict(unit=1, gx=69338)),
    ((300, 84, 64, "act", 1), dict(map_rb=256, gx=8668)),
    ((100, 42, 160, "bwd_reduce", 0), dict(nrg=12, active=240, rb=378, nt=513, first=1, nt2=9, lds=15360)),
    ((300, 42, 160, "bwd_reduce", 0), dict(rb=1024, nt=568, first=1, nt2=9)),
    ((300, 42, 160, "bwd_apply", 1), dict(map_rb=96, gx=6050)),
    ((100, 21, 320, "join_reduce", 0), dict(nrg=6, rb=103, nt=514, wb=20, lds=23040)),
    ((300, 21, 320, "join_reduce", 0), dict(rb=309, nt=514, wb=59)),
    ((100, 10, 640, "bwd_reduce", 1), dict(nrg=3, active=240, rb=64, nt=225, first=1, nt2=4, lds=23040)),
    ((300, 10, 640, "join_apply", 0), dict(ncy=7, ncx=7, cb=12, gx=1225)),
    ((100, 5, 640, "avgpool", 0), dict(gx=3, gy=400)),
    ((300, 5, 640, "avgpool_bwd", 0), dict(gx=123, gy=1200)),
]


# ---- layout helpers -----------------------------------------------------------------------------------------------------------------
def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def bracket(r, e):
    """[RNE-bf16(r - e), RNE-bf16(r + e)] in float64: an fp32 value within e of r rounds to bf16 inside it (rounding is monotone)."""
    return (r - e).to(torch.bfloat16).double(), (r + e).to(torch.bfloat16).double()


def _border_zero(t):
    return torch.where(R._in(t), t, torch.zeros((), dtype=t.dtype))


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _int_table(B, C, g):
    t = torch.randint(-1, 2, (B, 13, C), generator=g).float()
    t[:, R.FI["mu"]] = 0
    t[:, R.FI["c0"]] = 0
    t[:, R.FI["r"]] = 1
    t[:, R.FI["a"]] = 1
    return t


def _gauss_table(B, C, g):
    t = torch.randn(B, 13, C, generator=g) * 0.5
    t[:, R.FI["r"]] = 0.5 + 1.5 * torch.rand(B, C, generator=g)
    t[:, R.FI["a"]] = (0.5 + torch.rand(B, C, generator=g)) * t[:, R.FI["r"]] * (torch.randint(0, 2, (B, C), generator=g) * 2 - 1).float()
    return t.float()


@functools.lru_cache(maxsize=None)
def make_inputs(name, kind):
    """-> dict of float32 CPU tensors holding bf16 values: maps u (= u3), us, ud (= u3d), usd, da, dad [B, M, Hp, Wp, C] with zero
    borders, dout, doutd on the pooled grid, and the tables coef (= coef3), coefs [B, 13, C]."""
    c = MAPS[name]
    B, M, H, W, C = c["B"], c["M"], c["H"], c["W"], c["C"]
    g = _gen(SEEDS[name] + (0 if kind == "int" else 100000))
    shape, pshape = (B, M, H + 2, W + 2, C), (B, M, H // 2 + 2, W // 2 + 2, C)
    d = {}
    if kind == "int":
        # positive u: every LeakyReLU mask is 1 and, with MU = 0 and R = A = 1, xh = u and s = u3 + us; values 1..3 tie often: the
        # first maximum in window order must win in the forward, the reduce and both apply kernels
        for k in ("u", "us"):
            d[k] = torch.randint(1, 4, shape, generator=g).float()
        for k, sh in (("ud", shape), ("usd", shape), ("da", shape), ("dad", shape), ("dout", pshape), ("doutd", pshape)):
            d[k] = torch.randint(-2, 3, sh, generator=g).float()
        d["coef"], d["coefs"] = _int_table(B, C, g), _int_table(B, C, g)
    else:
        for k, sh in (("u", shape), ("us", shape), ("ud", shape), ("usd", shape), ("da", shape), ("dad", shape), ("dout", pshape),
                      ("doutd", pshape)):
            d[k] = bf(torch.randn(sh, generator=g))
        d["coef"], d["coefs"] = _gauss_table(B, C, g), _gauss_table(B, C, g)
        _repair(d, g)
    for k in ("u", "us", "ud", "usd", "da", "dad", "dout", "doutd"):
        d[k] = _border_zero(d[k])
    return d


def decisions(d):
    """(smallest |LeakyReLU argument| of BN(u), smallest top-two gap of a window, smallest |s| at an arg-max) in float64."""
    v = R.act_arg(d["u"], d["coef"]).abs().min()
    gap, top = R.join_gaps(d["u"], d["us"], d["coef"], d["coefs"])
    return float(v), float(gap.min()) if gap.numel() else float("inf"), float(top.min()) if top.numel() else float("inf")


def _repair(d, g):
    """Re-draw, on the CPU and before anything runs, every element whose LeakyReLU argument or whose window's decision lies within
    TIE_FLOOR of a tie in float64 -- nothing is masked out of a comparison afterwards."""
    for _ in range(64):
        bad = R.act_arg(d["u"], d["coef"]).abs() <= TIE_FLOOR
        gap, top = R.join_gaps(d["u"], d["us"], d["coef"], d["coefs"])
        badw = (gap <= TIE_FLOOR) | (top <= TIE_FLOOR)                # [B, M, Ho, Wo, C]
        Hp, Wp = d["u"].shape[2], d["u"].shape[3]
        if badw.numel():
            bad = bad | (R.unwindows(badw.unsqueeze(-2).expand(*badw.shape[:-1], 4, badw.shape[-1]).float(), Hp, Wp) > 0)
        n = int(bad.sum())
        if not n:
            return
        d["u"][bad] = bf(torch.randn(n, generator=g))
    raise AssertionError("the inputs could not be repaired")


# ---- references -----------------------------------------------------------------------------------------------------------------------
def _pad_slabs(t, nt):
    out = t.new_zeros(t.shape[0], nt, t.shape[2], t.shape[3])
    out[:, :t.shape[1]] = t
    return out


def compute(name, kind, dt, seq=False, B=None):
    """every output of the row in dtype dt (episodes [:B])."""
    c = MAPS[name]
    d = {k: v[:B] for k, v in make_inputs(name, kind).items()}
    p = plan_of(name)
    u, us, ud, usd, da, dad, dout, doutd, cf, cs = (d[k] for k in ("u", "us", "ud", "usd", "da", "dad", "dout", "doutd", "coef", "coefs"))
    want = outputs_of(name)
    o = {}
    for t in (False, True):
        s = "_t" if t else ""
        tan = dict(ud=ud, dad=dad) if t else {}
        if "act" + s in want:
            o["act" + s] = R.act(u, cf, ud if t else None, dt)
        if "red" + s in want:
            o["red" + s] = R.bwd_reduce(u, da, cf, p["rb"], dt=dt, seq=seq, **tan)
        if "du" + s in want:
            o["du" + s] = R.bwd_apply(u, da, cf, dt=dt, **tan)
        jt = dict(u3d=ud, usd=usd) if t else {}
        if "jf" + s in want:
            o["jf" + s] = R.join_fwd(u, us, cf, cs, dt=dt, **jt)
        if "jred" + s in want:
            o["jred" + s] = _pad_slabs(R.join_reduce(u, us, cf, cs, dout, p["wb"], dt=dt, seq=seq, doutd=doutd if t else None, **jt), p["nt"])
        if "ja3" + s in want:
            o["ja3" + s], o["jas" + s] = R.join_apply(u, us, cf, cs, dout, dt=dt, doutd=doutd if t else None, **jt)
    return o


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """-> (r64 {key: float64 tensor}, e32 {key: largest |float32 restatement - float64|}); int rows: e32 is all zero by construction."""
    r64 = compute(name, kind, torch.float64)
    if kind == "int":
        return r64, {k: 0.0 for k in r64}
    r32 = compute(name, kind, torch.float32, seq=True)
    return r64, {k: float((r32[k].double() - r64[k]).abs().max()) for k in r64}


# ---- the coefficient rows -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coef_inputs(name, kind):
    c = COEFS[name]
    B, C, nt, K = c["B"], c["C"], c["nt"], c["K"]
    g = _gen(SEEDS[c["like"] or name] + (0 if kind == "int" else 100000))
    n = float(nt * 7)
    if kind == "int":
        part = torch.randint(-3, 4, (B, nt, K, C), generator=g).float()
        if c["mode"] == "fwd":                                       # sum, sum of squares: channel 0 a constant map of 2s -> var = 0
            part[:, :, c["ks"][1]] = part[:, :, c["ks"][1]].abs() + 9 * 7
            part[:, :, c["ks"][0], 0] = 2 * 7
            part[:, :, c["ks"][1], 0] = 4 * 7
        table = _int_table(B, C, g)
        table[:, R.FI["r"]] = 2                                      # (exact in every product the pass forms)
        vec = lambda: torch.randint(-2, 3, (B, C), generator=g).float()
    else:
        part = torch.randn(B, nt, K, C, generator=g) + 0.5           # (a mean: every channel's sums are of one order)
        if c["mode"] == "fwd":
            part[:, :, c["ks"][1]] = part[:, :, c["ks"][1]].abs() * 3 + 3
            part[:, :, c["ks"][0], 0] = 0.3 * 7                      # channel 0: sum of squares a little BELOW n mu^2: the clamp
            part[:, :, c["ks"][1], 0] = 0.3 * 0.3 * 7 * (1 - 1e-4)
        table = _gauss_table(B, C, g)
        vec = lambda: torch.randn(B, C, generator=g)
    return dict(part=part, table=table, n=n, g=vec(), beta=vec(), gd=vec(), betad=vec())


@functools.lru_cache(maxsize=None)
def coef_reference(name, kind):
    """-> (table64, dg, dbeta) of float64 and, for gauss rows, the per-output share of a float32 restatement (sequential float32 sums
    and float32 formulas) -- {field or 'dg' / 'dbeta': share of the field's maximum}."""
    c = COEFS[name]
    d = coef_inputs(name, kind)
    t64, dg, db = R.coef_pass(c["mode"], d["part"], c["ks"], d["n"], d["table"], d["g"], d["beta"], d["gd"], d["betad"])
    if kind == "int":
        return (t64, dg, db), {}
    t32, dg32, db32 = coef_pass32(c["mode"], d["part"], c["ks"], d["n"], d["table"], d["g"], d["beta"], d["gd"], d["betad"])
    sh = {f: share(t32[:, R.FI[f]], t64[:, R.FI[f]]) for f in R.MODE_FIELDS[c["mode"]]}
    if dg is not None:
        sh["dg"], sh["dbeta"] = share(dg32, dg), share(db32, db)
    return (t64, dg, db), sh


def share(x, r):
    return float((x.double() - r.double()).abs().max() / r.double().abs().max())


def coef_pass32(mode, part, ks, n, table, g, beta, gd, betad):
    """the float32 restatement of the coefficient pass: slabs added one after the other in float32, the formulas in float32."""
    f = torch.float32
    s = R.seqsum(part.to(f), 1)
    s0, s1, s2 = s[:, ks[0]], s[:, ks[1]], s[:, ks[2]]
    n = torch.tensor(n, dtype=f)
    t = table.to(f).clone()
    I = R.FI
    dg = db = None
    if mode == "fwd":
        mu = s0 / n
        var = (s1 / n - mu * mu).clamp_min(0.0)
        r = 1.0 / torch.sqrt(var + torch.tensor(R.EPS, dtype=f))
        A = g * r
        t[:, I["mu"]], t[:, I["r"]], t[:, I["a"]], t[:, I["c0"]] = mu, r, A, beta - mu * A
    elif mode == "bwd":
        t[:, I["d1"]], t[:, I["d2"]] = s0 / n, s1 / n
        db, dg = s0, s1
    elif mode == "tfwd":
        mu, r, A = t[:, I["mu"]], t[:, I["r"]], t[:, I["a"]]
        m1, m2 = s0 / n, r * (s1 - mu * s0) / n
        t[:, I["m1"]], t[:, I["m2"]], t[:, I["tb"]], t[:, I["tc"]] = m1, m2, gd - A * m2, betad - A * m1
    else:
        r, A, m2 = t[:, I["r"]], t[:, I["a"]], t[:, I["m2"]]
        t[:, I["dd1"]], t[:, I["e12"]], t[:, I["k0"]] = s0 / n, (s1 + s2) / n, gd * r - A * r * m2
        db, dg = s0, s1 + s2
    return t, dg, db


# ---- pooling and image prep -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_inputs(name, kind):
    BM, H, W, C = POOLS[name]
    g = _gen(SEEDS[name] + (0 if kind == "int" else 100000))
    if kind == "int":                                                # H W a power of two or not: the quotient is one IEEE division
        o = torch.randint(-3, 4, (BM, H + 2, W + 2, C), generator=g).float()
        df = torch.randint(-3, 4, (BM, C), generator=g).float() * (H * W)
    else:
        o, df = bf(torch.randn(BM, H + 2, W + 2, C, generator=g)), torch.randn(BM, C, generator=g)
    o[:, 0], o[:, -1], o[:, :, 0], o[:, :, -1] = 0, 0, 0, 0
    return dict(o=o, df=df)


@functools.lru_cache(maxsize=None)
def prep_inputs(name):
    BM, Cin, H, W = PREPS[name]
    return torch.randn(BM, Cin, H, W, generator=_gen(SEEDS[name]))
