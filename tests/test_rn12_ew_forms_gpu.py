"""GPU suite: every form of the thirteen element-wise kernels of csrc/rn12_ew.hip against float64, through the raw-buffer hooks
(DESIGN.md section 48).  The tables are tests/rn12_ew_forms.py.  Per row:

* the plan the launcher reports (fumi_hip_rn12_ew_plan) is what the host query gives for the shape;
* `int` data: every output EQUALS the integer reference -- every slab of every reduction, every pixel of every map, the arg-max of
  every tied window -- so a dropped or doubled pixel, slab, group, window or cell of any size shows;
* `gauss` data: a bf16 output lies between RNE-bf16(r - e) and RNE-bf16(r + e), r the float64 formula on the same stored inputs and
  e = 4 x the largest deviation of the CPU float32 restatement from float64; an fp32 output (partial sums, coefficient fields, dg,
  dbeta, pooled features) is within 4 x the restatement's own share of the output's maximum.  Nothing is excluded: the inputs were
  repaired on the CPU until no decision is near a tie (the CPU suite asserts it);
* memory: every buffer sits between NaN bands; input maps carry NaN in every border pixel (no kernel may use one); outputs are
  pre-filled with a sentinel: border pixels come back exactly zero, interior pixels written, bands and stride gaps untouched;
* rows flagged `chunk`: episode 0 alone has the bits of episode 0 of the B-episode call.
The tables run forward and then in reverse in one process and give the same bits; the plain join apply gives the same bits on the
walking kernel and on the one-cell-per-thread kernel."""
import hashlib

import pytest
import torch

import rn12_ew_forms as F
import rn12_ew_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _put(t, dev, dtype, nan_border=False):
    """CPU tensor -> (whole buffer, view of the payload) on the device between NaN bands; map borders NaN on request."""
    if nan_border:
        t = torch.where(R._in(t) if t.dim() == 5 else R._in(t[None])[0], t, torch.full((), NAN))
    flat = torch.full((t.numel() + 2 * F.GUARD,), NAN, device=dev, dtype=dtype)
    flat[F.GUARD:F.GUARD + t.numel()] = t.reshape(-1).to(dtype).to(dev)
    return flat, flat[F.GUARD:F.GUARD + t.numel()]


def _out_map(shape, dev):
    n = 1
    for s in shape:
        n *= s
    bits = torch.full((n + 2 * F.GUARD,), F.SENTINEL, device=dev, dtype=torch.int16)
    return bits, bits.view(torch.bfloat16)[F.GUARD:F.GUARD + n]


def _get_map(bits, shape, what):
    """the written map as float32 [shape]; bands kept, border pixels exactly (+)zero, interior pixels written."""
    b = bits.cpu()
    n = b.numel() - 2 * F.GUARD
    assert bool((b[:F.GUARD] == F.SENTINEL).all()) and bool((b[-F.GUARD:] == F.SENTINEL).all()), f"{what}: a guard band was written"
    body = b[F.GUARD:F.GUARD + n].view(*shape)
    inn = R._in(body).expand(*shape)
    assert bool((body[~inn] == 0).all()), f"{what}: {int((body[~inn] != 0).sum())} border elements are not +0"
    assert not bool((body[inn] == F.SENTINEL).any()), f"{what}: {int((body[inn] == F.SENTINEL).sum())} interior elements not written"
    return body.view(torch.bfloat16).float()


def _out_f32(n, dev):
    flat = torch.full((n + 2 * F.GUARD,), NAN, device=dev, dtype=torch.float32)
    return flat, flat[F.GUARD:F.GUARD + n]


def _get_f32(flat, shape, what):
    f = flat.cpu()
    assert bool(torch.isnan(f[:F.GUARD]).all()) and bool(torch.isnan(f[-F.GUARD:]).all()), f"{what}: a guard band was written"
    body = f[F.GUARD:-F.GUARD].view(*shape).clone()
    assert not bool(torch.isnan(body).any()), f"{what}: {int(torch.isnan(body).sum())} elements not written (or NaN)"
    return body


def run_maps(name, kind, dev, ws, one=False, cell=False):
    """every output of a MAPS row (one: episode 0 alone) -> ({key: CPU float32}, {key: reported plan})."""
    from fumi_amd import hip
    c = F.MAPS[name]
    B, M, H, W, C = (1 if one else c["B"]), c["M"], c["H"], c["W"], c["C"]
    d = {k: v[:B] for k, v in F.make_inputs(name, kind).items()}
    bfl = torch.bfloat16
    keep, g = [], {}
    for k in ("u", "us", "ud", "usd", "da", "dad", "dout", "doutd"):
        buf, g[k] = _put(d[k], dev, bfl, nan_border=True)
        keep.append(buf)
    for k in ("coef", "coefs"):
        buf, g[k] = _put(d[k], dev, torch.float32)
        keep.append(buf)
    shape, pshape = tuple(d["u"].shape), tuple(d["dout"].shape)
    nt = F.plan_of(name)["nt"]
    want = F.outputs_of(name)
    outs, plans = {}, {}
    for t in (False, True):
        s = "_t" if t else ""
        ud, dad, usd, doutd = (g["ud"], g["dad"], g["usd"], g["doutd"]) if t else (None,) * 4
        if "act" + s in want:
            bits, o = _out_map(shape, dev)
            hip.rn12_ew_act(ws, B, M, H, W, C, g["u"], ud, g["coef"], o)
            plans["act" + s] = hip.rn12_ew_plan()
            outs["act" + s] = _get_map(bits, shape, f"{name} act{s}")
        if "red" + s in want:
            flat, o = _out_f32(B * nt * (3 if t else 2) * C, dev)
            hip.rn12_ew_bwd(ws, B, M, H, W, C, False, g["u"], ud, g["da"], dad, g["coef"], o)
            plans["red" + s] = hip.rn12_ew_plan()
            outs["red" + s] = _get_f32(flat, (B, nt, 3 if t else 2, C), f"{name} red{s}")
        if "du" + s in want:
            bits, o = _out_map(shape, dev)
            hip.rn12_ew_bwd(ws, B, M, H, W, C, True, g["u"], ud, g["da"], dad, g["coef"], o)
            plans["du" + s] = hip.rn12_ew_plan()
            outs["du" + s] = _get_map(bits, shape, f"{name} du{s}")
        if "jf" + s in want:
            bits, o = _out_map(pshape, dev)
            hip.rn12_ew_join(ws, B, M, H, W, C, 0, g["u"], g["us"], ud, usd, g["coef"], g["coefs"], None, None, o)
            plans["jf" + s] = hip.rn12_ew_plan()
            outs["jf" + s] = _get_map(bits, pshape, f"{name} jf{s}")
        if "jred" + s in want:
            flat, o = _out_f32(B * nt * (5 if t else 3) * C, dev)
            hip.rn12_ew_join(ws, B, M, H, W, C, 1, g["u"], g["us"], ud, usd, g["coef"], g["coefs"], g["dout"], doutd, o)
            plans["jred" + s] = hip.rn12_ew_plan()
            outs["jred" + s] = _get_f32(flat, (B, nt, 5 if t else 3, C), f"{name} jred{s}")
        if "ja3" + s in want:
            b3, o3 = _out_map(shape, dev)
            bs_, os_ = _out_map(shape, dev)
            hip.rn12_ew_join(ws, B, M, H, W, C, 2, g["u"], g["us"], ud, usd, g["coef"], g["coefs"], g["dout"], doutd, o3, os_,
                             form=1 if (cell and not t) else 0)
            plans["ja3" + s] = plans["jas" + s] = hip.rn12_ew_plan()
            outs["ja3" + s], outs["jas" + s] = _get_map(b3, shape, f"{name} ja3{s}"), _get_map(bs_, shape, f"{name} jas{s}")
    assert ws.read_status() == 0
    return outs, plans


_RUNS = {}


def _measure(name, kind, dev, ws):
    if (name, kind) not in _RUNS:
        _RUNS[(name, kind)] = run_maps(name, kind, dev, ws)
    return _RUNS[(name, kind)]


def _digest(outs):
    h = hashlib.sha256()
    for k in sorted(outs):
        h.update(outs[k].contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


@pytest.mark.parametrize("name", list(F.MAPS))
def test_maps_exact(name, dev, ws):
    from fumi_amd import hip
    outs, plans = _measure(name, "int", dev, ws)
    r64, _ = F.reference(name, "int")
    assert set(outs) == set(r64)
    for k in outs:
        q = F.query(name, hip, k)
        assert plans[k] == q, k
        bad = outs[k].double() != r64[k]
        assert not bool(bad.any()), f"{name} {k}: {int(bad.sum())} of {bad.numel()} elements differ from the integer reference; first at " \
                                    f"{tuple(bad.nonzero()[0].tolist())}: {float(outs[k][bad][0])} for {float(r64[k][bad][0])}"
    c = F.MAPS[name]
    if "ja3" in outs:                                                # the two plain apply kernels: equal bits
        cell, cplans = run_maps(name, "int", dev, ws, cell=True)
        assert cplans["ja3"]["cell"] == 1 and plans["ja3"]["cell"] == 0
        assert torch.equal(cell["ja3"], outs["ja3"]) and torch.equal(cell["jas"], outs["jas"])
    if c["chunk"]:
        one, _ = run_maps(name, "int", dev, ws, one=True)
        for k in outs:
            assert torch.equal(one[k][0], outs[k][0]), f"{name} {k}: episode 0 alone differs from episode 0 of {c['B']}"


@pytest.mark.parametrize("name", [n for n in F.MAPS if F.MAPS[n]["gauss"]])
def test_maps_gauss(name, dev, ws):
    outs, plans = _measure(name, "gauss", dev, ws)
    r64, e32 = F.reference(name, "gauss")
    fails = []
    for k in outs:
        y, r = outs[k].double(), r64[k]
        if k.split("_t")[0] in F.BF16_OUT:
            e = F.E_FACTOR * e32[k]
            lo, hi = F.bracket(r, e)
            outside = int(((y < lo) | (y > hi)).sum())
            print(f"\n[{name}] {k}: e32 {e32[k]:.2e} allowance {e:.2e} engine max|y - r| {float((y - r).abs().max()):.2e} "
                  f"(max|r| {float(r.abs().max()):.2f}) outside the bracket: {outside}", end="")
            if outside:
                fails.append((k, outside))
        else:
            m = float(r.abs().max())
            bound, got = F.E_FACTOR * e32[k] / m, float((y - r).abs().max()) / m
            print(f"\n[{name}] {k}: restatement share {e32[k] / m:.2e} bound {bound:.2e} engine {got:.2e}", end="")
            if not got <= bound:
                fails.append((k, got, bound))
    assert not fails, fails
    c = F.MAPS[name]
    if "ja3" in outs:
        cell, _ = run_maps(name, "gauss", dev, ws, cell=True)
        assert torch.equal(cell["ja3"], outs["ja3"]) and torch.equal(cell["jas"], outs["jas"])
    if c["chunk"]:
        one, _ = run_maps(name, "gauss", dev, ws, one=True)
        for k in outs:
            assert torch.equal(one[k][0], outs[k][0]), f"{name} {k}: episode 0 alone differs from episode 0 of {c['B']}"


# ---- the coefficient pass -------------------------------------------------------------------------------------------------------------
def run_coef(name, kind, dev, ws):
    """-> (table [B, 13, C], dg, dbeta or None, reported plan): strides longer than C with NaN gaps, scratch before a NaN band."""
    from fumi_amd import hip
    c = F.COEFS[name]
    B, C, nt, K, mode = c["B"], c["C"], c["nt"], c["K"], c["mode"]
    d = F.coef_inputs(name, kind)
    st = C + c["pad"]

    def strided(v):
        t = torch.full((B, st), NAN)
        t[:, :C] = v
        return _put(t, dev, torch.float32)
    keep = [_put(d["part"], dev, torch.float32), _put(d["table"], dev, torch.float32)]
    vec = {k: strided(d[k]) for k in ("g", "beta", "gd", "betad")}
    dgf, dgv = _out_f32(B * st, dev)
    dbf, dbv = _out_f32(B * st, dev)
    q = hip.rn12_coef_query(B, nt, K, C, c["scratch"])
    sf, sv = _out_f32(max(q["scratch"], 1), dev)
    kw = {}
    if mode == "fwd":
        kw = dict(g=vec["g"][1], beta=vec["beta"][1], pstride=st)
    elif mode == "tfwd":
        kw = dict(gd=vec["gd"][1], betad=vec["betad"][1], dstride=st)
    elif mode == "bwd":
        kw = dict(dg=dgv, dbeta=dbv, gstride=st)
    else:
        kw = dict(gd=vec["gd"][1], dstride=st, dg=dgv, dbeta=dbv, gstride=st)
    hip.rn12_ew_coef(ws, B, C, mode, nt, K, c["ks"], d["n"], keep[0][1], keep[1][1], scratch=sv if c["scratch"] else None, **kw)
    plan = hip.rn12_ew_plan()
    assert ws.read_status() == 0
    assert (plan["first"], plan["nt2"]) == (q["first"], q["nt2"])
    table = _get_f32(keep[1][0], (B, 13, C), f"{name} table")
    s = sf.cpu()
    assert bool(torch.isnan(s[:F.GUARD]).all()) and bool(torch.isnan(s[F.GUARD + q["scratch"]:]).all()), f"{name}: written beyond the scratch"
    assert bool(torch.isnan(s[F.GUARD:F.GUARD + q["scratch"]]).any()) != bool(q["first"]), f"{name}: the scratch is written by the first stage alone"
    untouched = [f for f in R.FIELDS if f not in R.MODE_FIELDS[mode]]
    for f in untouched:
        assert torch.equal(table[:, R.FI[f]], d["table"][:, R.FI[f]]), f"{name}: field {f} is not the mode's to write"
    dg = db = None
    if mode in ("bwd", "tbwd"):
        a, b = dgf.cpu()[F.GUARD:-F.GUARD].view(B, st), dbf.cpu()[F.GUARD:-F.GUARD].view(B, st)
        assert bool(torch.isnan(a[:, C:]).all()) and bool(torch.isnan(b[:, C:]).all()), f"{name}: a gap between the gradient rows was written"
        dg, db = a[:, :C].clone(), b[:, :C].clone()
        assert not bool(torch.isnan(dg).any() | torch.isnan(db).any())
    else:
        assert bool(torch.isnan(dgf.cpu()).all()) and bool(torch.isnan(dbf.cpu()).all())
    return table, dg, db, plan


SUMS_ONLY = {"mu", "d1", "d2", "m1", "dd1", "e12"}       # one IEEE division of an exact sum: the bits of the float64 reference


@pytest.mark.parametrize("name", list(F.COEFS))
def test_coef_exact(name, dev, ws):
    c = F.COEFS[name]
    table, dg, db, _ = run_coef(name, "int", dev, ws)
    (t64, dg64, db64), _ = F.coef_reference(name, "int")
    for f in R.MODE_FIELDS[c["mode"]]:
        got, ref = table[:, R.FI[f]], t64[:, R.FI[f]].float()
        if f in SUMS_ONLY:
            assert torch.equal(got, ref), f"{name}: field {f}"
        else:       # a few double operations behind an exact sum: a last-bit difference in double moves the fp32 result one ulp at most
            assert bool(((got - ref).abs() <= ref.abs() * 2.0 ** -23).all()), f"{name}: field {f}"
    if dg is not None:
        assert torch.equal(dg.double(), dg64) and torch.equal(db.double(), db64), name


@pytest.mark.parametrize("name", list(F.COEFS))
def test_coef_gauss(name, dev, ws):
    c = F.COEFS[name]
    table, dg, db, _ = run_coef(name, "gauss", dev, ws)
    (t64, dg64, db64), sh = F.coef_reference(name, "gauss")
    got = {f: (table[:, R.FI[f]], t64[:, R.FI[f]]) for f in R.MODE_FIELDS[c["mode"]]}
    if dg is not None:
        got["dg"], got["dbeta"] = (dg, dg64), (db, db64)
    fails = []
    for f, (x, r) in got.items():
        s = F.share(x, r)
        print(f"\n[{name}] {f}: restatement share {sh[f]:.2e} bound {F.E_FACTOR * sh[f]:.2e} engine {s:.2e}", end="")
        if not s <= F.E_FACTOR * sh[f]:
            fails.append((f, s, F.E_FACTOR * sh[f]))
    assert not fails, fails
    if c["mode"] == "fwd":                                           # the clamped channel
        assert torch.equal(table[:, R.FI["r"], 0], t64[:, R.FI["r"], 0].float())


def test_coef_single_stage_and_first_stage_agree(dev, ws):
    """k_nt129_noscratch is k_nt129_tbwd_s without scratch, on the SAME integer sums: equal bits (both orders are exact)."""
    assert torch.equal(F.coef_inputs("k_nt129_tbwd_s", "int")["part"], F.coef_inputs("k_nt129_noscratch", "int")["part"])
    a, b = run_coef("k_nt129_tbwd_s", "int", dev, ws), run_coef("k_nt129_noscratch", "int", dev, ws)
    assert (a[3]["first"], b[3]["first"]) == (1, 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ---- pooling, image prep ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(F.POOLS))
@pytest.mark.parametrize("kind", ["int", "gauss"])
def test_avgpool_and_adjoint(name, kind, dev, ws):
    from fumi_amd import hip
    BM, H, W, C = F.POOLS[name]
    d = F.pool_inputs(name, kind)
    buf, o = _put(d["o"], dev, torch.bfloat16, nan_border=True)
    flat, f = _out_f32(BM * C, dev)
    hip.rn12_ew_avgpool(ws, BM, H, W, C, False, o, f)
    assert hip.rn12_ew_plan() == hip.rn12_ew_query(1, BM, H, W, C, "avgpool")
    feats = _get_f32(flat, (BM, C), name)
    dbuf, df = _put(d["df"], dev, torch.float32)
    bits, dout = _out_map((BM, H + 2, W + 2, C), dev)
    hip.rn12_ew_avgpool(ws, BM, H, W, C, True, df, dout)
    assert hip.rn12_ew_plan() == hip.rn12_ew_query(1, BM, H, W, C, "avgpool_bwd")
    dmap = _get_map(bits, (1, BM, H + 2, W + 2, C), name)[0]
    assert ws.read_status() == 0
    r64, radj = R.avgpool(d["o"]), R.avgpool_bwd(d["df"], H, W)
    if kind == "int":
        assert torch.equal(feats, (d["o"][:, 1:-1, 1:-1].sum((1, 2)) / float(H * W)).float())     # an exact sum, one fp32 division
        assert torch.equal(dmap.double(), radj)
        return
    sh = F.share(R.avgpool(d["o"], torch.float32, seq=True), r64)
    got = F.share(feats, r64)
    print(f"\n[{name}] pooled features: restatement share {sh:.2e} bound {F.E_FACTOR * sh:.2e} engine {got:.2e}")
    e = F.E_FACTOR * float((R.avgpool_bwd(d["df"], H, W, torch.float32).double() - radj).abs().max())
    lo, hi = F.bracket(radj, e)
    assert not bool(((dmap.double() < lo) | (dmap.double() > hi)).any())
    assert got <= F.E_FACTOR * sh if H * W > 1 else got == 0.0


@pytest.mark.parametrize("name", list(F.PREPS))
def test_img_prep(name, dev, ws):
    from fumi_amd import hip
    BM, Cin, H, W = F.PREPS[name]
    img = F.prep_inputs(name)
    buf, x = _put(img, dev, torch.float32)
    bits, out = _out_map((BM, H + 2, W + 2, 16), dev)
    hip.rn12_ew_img_prep(ws, BM, Cin, H, W, x, out)
    assert hip.rn12_ew_plan() == hip.rn12_ew_query(1, BM, H, W, Cin, "img_prep")
    b = bits.cpu()
    assert bool((b[:F.GUARD] == F.SENTINEL).all()) and bool((b[-F.GUARD:] == F.SENTINEL).all())
    got = b[F.GUARD:-F.GUARD].view(torch.bfloat16).view(BM, H + 2, W + 2, 16)
    want = R.img_prep(img).to(torch.bfloat16)                        # RNE of the fp32 pixel; channels Cin..15 and the border +0
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert not bool(got[..., Cin:].view(torch.int16).any())


def test_hooks_refuse_before_anything_is_launched(dev, ws):
    from fumi_amd import hip
    z = torch.zeros(1 << 16, device=dev, dtype=torch.bfloat16)
    f = torch.zeros(1 << 16, device=dev, dtype=torch.float32)
    before = hip.rn12_ew_plan()
    bad = r"invalid argument \(-1\)"
    with pytest.raises(hip.FumiHipError) as e:
        hip.rn12_ew_act(ws, 1, 1, 2, 2, 2056, z, None, f, z)
    assert "invalid argument" not in str(e.value)
    for call in (lambda: hip.rn12_ew_act(ws, 1, 1, 2, 2, 12, z, None, f, z),
                 lambda: hip.rn12_ew_bwd(ws, 1, 1, 2, 2, 16, False, z, None, None, None, f, f),
                 lambda: hip.rn12_ew_join(ws, 1, 1, 1, 2, 16, 0, z, z, None, None, f, f, None, None, z),
                 lambda: hip.rn12_ew_join(ws, 1, 1, 2, 2, 16, 2, z, z, None, None, f, f, None, None, z, z),
                 lambda: hip.rn12_ew_coef(ws, 1, 16, "fwd", 1, 2, (0, 2, 0), 4.0, f, f, g=f, beta=f, pstride=16),
                 lambda: hip.rn12_ew_coef(ws, 1, 16, "fwd", 1, 2, (0, 1, 0), 4.0, f, f, g=f, beta=f, pstride=8),
                 lambda: hip.rn12_ew_coef(ws, 1, 16, "bwd", 0, 2, (0, 1, 0), 4.0, f, f, dg=f, dbeta=f, gstride=16),
                 lambda: hip.rn12_ew_img_prep(ws, 1, 0, 2, 2, f, z), lambda: hip.rn12_ew_img_prep(ws, 1, 9, 2, 2, f, z)):
        with pytest.raises(hip.FumiHipError, match=bad):
            call()
    torch.cuda.synchronize()
    assert hip.rn12_ew_plan() == before and not bool(z.any()) and not bool(f.any()) and ws.read_status() == 0


def test_forward_then_reverse_order_gives_the_same_bits(dev, ws):
    rows = [(n, k) for n in F.MAPS for k in ("int", "gauss") if F.MAPS[n]["gauss"]]
    first = {r: _digest(_measure(*r, dev, ws)[0]) for r in rows}
    for r in reversed(rows):
        assert _digest(run_maps(*r, dev, ws)[0]) == first[r], r
    crow = [(n, k) for n in F.COEFS for k in ("int", "gauss")]
    cfirst = {r: run_coef(*r, dev, ws)[0] for r in crow}
    for r in reversed(crow):
        assert torch.equal(run_coef(*r, dev, ws)[0], cfirst[r]), r
