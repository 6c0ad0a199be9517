"""Plain statements of the element-wise passes of csrc/rn12_ew.hip, one function per kernel -- TEST INFRASTRUCTURE ONLY (DESIGN.md
section 48).  Every function takes the STORED operands (bf16 values held in any float dtype, the fp32 coefficient table) and computes
in the dtype `dt` it is given: float64 is the reference, float32 the restatement whose own deviation sizes the allowance.

Layout: a map is [B, M, H + 2, W + 2, C] (padded channels-last, the engine's), a coefficient table [B, 13, C] with the fields of
FIELDS, partial sums [B, nt, K, C].  Border pixels of every output are zero; border pixels of inputs are never used (torch.where,
so a NaN there cannot leak).  tests/test_rn12_ew_forms_cpu.py ties these formulas to oracle/resnet12_manual.py on one block."""
import torch

SLOPE = 0.1
EPS = 1e-5
FIELDS = ("mu", "r", "a", "c0", "d1", "d2", "tb", "tc", "m1", "m2", "k0", "dd1", "e12")
FI = {n: i for i, n in enumerate(FIELDS)}
f64 = torch.float64


def interior(M, H, W):
    m = torch.zeros(M, H + 2, W + 2, dtype=torch.bool)
    m[:, 1:-1, 1:-1] = True
    return m


def _f(coef, dt, *names):
    return [coef[:, FI[n]].to(dt)[:, None, None, None, :] for n in names]


def _in(t):
    B, M, Hp, Wp, C = t.shape
    return interior(M, Hp - 2, Wp - 2)[None, :, :, :, None]


def _zero_border(t):
    return torch.where(_in(t), t, torch.zeros((), dtype=t.dtype))


def lmask(v):
    return torch.where(v > 0, torch.ones((), dtype=v.dtype), torch.full((), SLOPE, dtype=v.dtype))


def act_arg(u, coef, dt=f64):
    """v = A u + C0, the LeakyReLU argument (interior only; border 1: never near zero)."""
    A, C0 = _f(coef, dt, "a", "c0")
    return torch.where(_in(u), A * u.to(dt) + C0, torch.ones((), dtype=dt))


def act(u, coef, ud=None, dt=f64):
    MU, R, A, C0, TB, TC = _f(coef, dt, "mu", "r", "a", "c0", "tb", "tc")
    u = u.to(dt)
    v = A * u + C0
    if ud is None:
        o = torch.where(v > 0, v, SLOPE * v)
    else:
        o = lmask(v) * (A * ud.to(dt) + TB * ((u - MU) * R) + TC)
    return _zero_border(o)


def _slabs(terms, per):
    """terms [B, n, K, C] -> sums of `per` consecutive rows: [B, ceil(n / per), K, C] (plain sum: exact for the integer rows)."""
    B, n, K, C = terms.shape
    nt = (n + per - 1) // per
    pad = terms.new_zeros(B, nt * per, K, C)
    pad[:, :n] = terms
    return pad.view(B, nt, per, K, C).sum(2)


def seqsum(t, dim):
    """sum along dim, one element after the other, every addition rounded to t's own dtype (torch.cumsum and torch.sum accumulate a
    float32 tensor in higher precision or pairwise on the CPU: neither is a float32 restatement of a running sum)."""
    acc = torch.zeros_like(t.select(dim, 0))
    for i in range(t.shape[dim]):
        acc = acc + t.select(dim, i)
    return acc


def _slabs_seq(terms, per):
    """the same sums, accumulated one row after the other in the terms' own dtype (the float32 restatement's order)."""
    B, n, K, C = terms.shape
    nt = (n + per - 1) // per
    pad = terms.new_zeros(B, nt * per, K, C)
    pad[:, :n] = terms
    return seqsum(pad.view(B, nt, per, K, C), 2)


def bwd_terms(u, da, coef, ud=None, dad=None, dt=f64):
    """per pixel (dv, dv xh) | tangent (dv', dv' xh, dv xh'): [B, npix, K, C], zero on the border."""
    MU, R, A, C0, M1, M2 = _f(coef, dt, "mu", "r", "a", "c0", "m1", "m2")
    u, da = u.to(dt), da.to(dt)
    mk = lmask(A * u + C0)
    xh = (u - MU) * R
    dv = da * mk
    if ud is None:
        t = [dv, dv * xh]
    else:
        dvd = dad.to(dt) * mk
        xhd = R * (ud.to(dt) - M1 - xh * M2)
        t = [dvd, dvd * xh, dv * xhd]
    t = torch.stack([_zero_border(x) for x in t], -2)                # [B, M, Hp, Wp, K, C]
    return t.reshape(t.shape[0], -1, t.shape[-2], t.shape[-1])


def bwd_reduce(u, da, coef, rb, ud=None, dad=None, dt=f64, seq=False):
    return (_slabs_seq if seq else _slabs)(bwd_terms(u, da, coef, ud, dad, dt), rb)


def bwd_apply(u, da, coef, ud=None, dad=None, dt=f64):
    MU, R, A, C0, D1, D2, M1, M2, K0, DD1, E12 = _f(coef, dt, "mu", "r", "a", "c0", "d1", "d2", "m1", "m2", "k0", "dd1", "e12")
    u, da = u.to(dt), da.to(dt)
    mk = lmask(A * u + C0)
    xh = (u - MU) * R
    dv = da * mk
    if ud is None:
        o = A * (dv - D1 - xh * D2)
    else:
        dvd = dad.to(dt) * mk
        xhd = R * (ud.to(dt) - M1 - xh * M2)
        o = K0 * (dv - D1 - xh * D2) + A * (dvd - DD1 - xhd * D2 - xh * E12)
    return _zero_border(o)


# ---- the residual join ------------------------------------------------------------------------------------------------------------
def windows(t):
    """[B, M, Hp, Wp, C] -> the 2 x 2 pooling windows of the interior [B, M, Ho, Wo, 4, C], window order (dy, dx) row-major."""
    B, M, Hp, Wp, C = t.shape
    Ho, Wo = (Hp - 2) // 2, (Wp - 2) // 2
    v = t[:, :, 1:1 + 2 * Ho, 1:1 + 2 * Wo]
    return v.reshape(B, M, Ho, 2, Wo, 2, C).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, M, Ho, Wo, 4, C)


def unwindows(w, Hp, Wp):
    """the inverse: zero on the border and on interior pixels no window covers."""
    B, M, Ho, Wo, _, C = w.shape
    out = w.new_zeros(B, M, Hp, Wp, C)
    out[:, :, 1:1 + 2 * Ho, 1:1 + 2 * Wo] = w.reshape(B, M, Ho, Wo, 2, 2, C).permute(0, 1, 2, 4, 3, 5, 6).reshape(B, M, 2 * Ho, 2 * Wo, C)
    return out


def join_s(u3, us, c3, cs, dt=f64):
    A3, C3 = _f(c3, dt, "a", "c0")
    As, Cs = _f(cs, dt, "a", "c0")
    return (A3 * u3.to(dt) + C3) + (As * us.to(dt) + Cs)


def first_argmax(sw):
    """sw [..., 4, C] -> index of the FIRST maximum in window order [..., C]."""
    mx = sw.max(-2, keepdim=True)[0]
    return (sw == mx).to(torch.int8).argmax(-2)                      # (argmax of a 0 / 1 tensor: the first 1)


def _pick(w, arg):
    return torch.gather(w, -2, arg.unsqueeze(-2)).squeeze(-2)


def _pad_pooled(o):
    """[B, M, Ho, Wo, C] -> padded [B, M, Ho + 2, Wo + 2, C]."""
    B, M, Ho, Wo, C = o.shape
    out = o.new_zeros(B, M, Ho + 2, Wo + 2, C)
    out[:, :, 1:-1, 1:-1] = o
    return out


def join_sd(u3, us, u3d, usd, c3, cs, dt=f64):
    MU3, R3, A3, TB3, TC3 = _f(c3, dt, "mu", "r", "a", "tb", "tc")
    MUs, Rs, As, TBs, TCs = _f(cs, dt, "mu", "r", "a", "tb", "tc")
    xh3, xhs = (u3.to(dt) - MU3) * R3, (us.to(dt) - MUs) * Rs
    return (A3 * u3d.to(dt) + TB3 * xh3 + TC3) + (As * usd.to(dt) + TBs * xhs + TCs)


def join_fwd(u3, us, c3, cs, u3d=None, usd=None, dt=f64):
    sw = windows(join_s(u3, us, c3, cs, dt))
    arg = first_argmax(sw)
    mx = _pick(sw, arg)
    if u3d is None:
        return _pad_pooled(torch.where(mx > 0, mx, SLOPE * mx))
    return _pad_pooled(lmask(mx) * _pick(windows(join_sd(u3, us, u3d, usd, c3, cs, dt)), arg))


def _pooled_interior(d):
    return d[:, :, 1:-1, 1:-1]


def join_terms(u3, us, c3, cs, dout, u3d=None, usd=None, doutd=None, dt=f64):
    """per window (ds, ds xh3, ds xhs) | tangent (ds', ds' xh3, ds xh3', ds' xhs, ds xhs') at the arg-max: [B, nwin, K, C]."""
    MU3, R3, M13, M23 = _f(c3, dt, "mu", "r", "m1", "m2")
    MUs, Rs, M1s, M2s = _f(cs, dt, "mu", "r", "m1", "m2")
    sw = windows(join_s(u3, us, c3, cs, dt))
    arg = first_argmax(sw)
    lm = lmask(_pick(sw, arg))
    a3, as_ = _pick(windows(u3.to(dt)), arg), _pick(windows(us.to(dt)), arg)
    ds = _pooled_interior(dout.to(dt)) * lm
    xh3, xhs = (a3 - MU3) * R3, (as_ - MUs) * Rs
    if u3d is None:
        t = [ds, ds * xh3, ds * xhs]
    else:
        dsd = _pooled_interior(doutd.to(dt)) * lm
        xh3d = R3 * (_pick(windows(u3d.to(dt)), arg) - M13 - xh3 * M23)
        xhsd = Rs * (_pick(windows(usd.to(dt)), arg) - M1s - xhs * M2s)
        t = [dsd, dsd * xh3, ds * xh3d, dsd * xhs, ds * xhsd]
    t = torch.stack(t, -2)
    return t.reshape(t.shape[0], -1, t.shape[-2], t.shape[-1])


def join_reduce(u3, us, c3, cs, dout, wb, u3d=None, usd=None, doutd=None, dt=f64, seq=False):
    return (_slabs_seq if seq else _slabs)(join_terms(u3, us, c3, cs, dout, u3d, usd, doutd, dt), wb)


def join_ds(u3, us, c3, cs, dout, dt=f64):
    """ds of every pixel: dout lrelu'(s) at the window's first arg-max, zero elsewhere (border, losers, uncovered pixels)."""
    sw = windows(join_s(u3, us, c3, cs, dt))
    arg = first_argmax(sw)
    hit = torch.zeros_like(sw).scatter_(-2, arg.unsqueeze(-2), 1.0)
    w = hit * (_pooled_interior(dout.to(dt)) * lmask(_pick(sw, arg))).unsqueeze(-2)
    return unwindows(w, u3.shape[2], u3.shape[3])


def join_apply(u3, us, c3, cs, dout, u3d=None, usd=None, doutd=None, dt=f64):
    """(du3, dus) | tangent (du3', dus'): the BN backward of both branches from the shared ds."""
    ds = join_ds(u3, us, c3, cs, dout, dt)
    dsd = None if u3d is None else join_ds(u3, us, c3, cs, doutd, dt)
    outs = []
    for c, u, ud in ((c3, u3, u3d), (cs, us, usd)):
        MU, R, A, D1, D2, M1, M2, K0, DD1, E12 = _f(c, dt, "mu", "r", "a", "d1", "d2", "m1", "m2", "k0", "dd1", "e12")
        xh = (u.to(dt) - MU) * R
        if ud is None:
            o = A * (ds - D1 - xh * D2)
        else:
            xhd = R * (ud.to(dt) - M1 - xh * M2)
            o = K0 * (ds - D1 - xh * D2) + A * (dsd - DD1 - xhd * D2 - xh * E12)
        outs.append(_zero_border(o))
    return outs


def join_gaps(u3, us, c3, cs, dt=f64):
    """(smallest top-two gap of any window, smallest |s| at an arg-max): what float32 and float64 could decide differently."""
    sw = windows(join_s(u3, us, c3, cs, dt))
    top = sw.topk(2, dim=-2)[0]
    return top[..., 0, :] - top[..., 1, :], top[..., 0, :].abs()


# ---- the coefficient pass -----------------------------------------------------------------------------------------------------------
def coef_pass(mode, part, ks, n, table, g=None, beta=None, gd=None, betad=None):
    """part [B, nt, K, C] (any dtype), slices ks -> (table [B, 13, C] float64 with the mode's fields replaced, dg, dbeta or None).
    The other fields are read from `table` as stored (the kernel reads its own fp32 table back)."""
    s = part.double().sum(1)                                         # [B, K, C]
    s0, s1, s2 = s[:, ks[0]], s[:, ks[1]], s[:, ks[2]]
    t = table.double().clone()
    dg = db = None
    if mode == "fwd":
        mu = s0 / n
        var = (s1 / n - mu * mu).clamp_min(0.0)
        r = 1.0 / torch.sqrt(var + float(torch.tensor(EPS, dtype=torch.float32)))
        A = g.double() * r
        t[:, FI["mu"]], t[:, FI["r"]], t[:, FI["a"]], t[:, FI["c0"]] = mu, r, A, beta.double() - mu * A
    elif mode == "bwd":
        t[:, FI["d1"]], t[:, FI["d2"]] = s0 / n, s1 / n
        db, dg = s0, s1
    elif mode == "tfwd":
        mu, r, A = t[:, FI["mu"]], t[:, FI["r"]], t[:, FI["a"]]
        m1, m2 = s0 / n, r * (s1 - mu * s0) / n
        t[:, FI["m1"]], t[:, FI["m2"]] = m1, m2
        t[:, FI["tb"]], t[:, FI["tc"]] = gd.double() - A * m2, betad.double() - A * m1
    else:
        r, A, m2 = t[:, FI["r"]], t[:, FI["a"]], t[:, FI["m2"]]
        t[:, FI["dd1"]], t[:, FI["e12"]] = s0 / n, (s1 + s2) / n
        t[:, FI["k0"]] = gd.double() * r - A * r * m2
        db, dg = s0, s1 + s2
    return t, dg, db


MODE_FIELDS = {"fwd": ("mu", "r", "a", "c0"), "bwd": ("d1", "d2"), "tfwd": ("m1", "m2", "tb", "tc"), "tbwd": ("k0", "dd1", "e12")}


# ---- pooling and image prep -----------------------------------------------------------------------------------------------------------
def avgpool(o, dt=f64, seq=False):
    """o [BM, Hp, Wp, C] -> [BM, C]: mean over the interior (row-major order when seq)."""
    v = o[:, 1:-1, 1:-1].to(dt).reshape(o.shape[0], -1, o.shape[-1])
    s = seqsum(v, 1) if seq else v.sum(1)
    return s / torch.tensor(float(v.shape[1]), dtype=dt)


def avgpool_bwd(df, H, W, dt=f64):
    out = torch.zeros(df.shape[0], H + 2, W + 2, df.shape[1], dtype=dt)
    out[:, 1:-1, 1:-1] = (df.to(dt) / torch.tensor(float(H * W), dtype=dt))[:, None, None, :]
    return out


def img_prep(img):
    """img [BM, Cin, H, W] -> [BM, Hp, Wp, 16]: the values themselves (the kernel only rounds them to bf16)."""
    BM, Cin, H, W = img.shape
    out = torch.zeros(BM, H + 2, W + 2, 16, dtype=img.dtype)
    out[:, 1:-1, 1:-1, :Cin] = img.permute(0, 2, 3, 1)
    return out
