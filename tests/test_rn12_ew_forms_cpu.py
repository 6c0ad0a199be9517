"""CPU suite: keeps the tables of tests/rn12_ew_forms.py honest against the library's own host query (fumi_hip_rn12_ew_query and
fumi_hip_rn12_coef_query are host arithmetic shared with the launchers: no GPU), holds the integer rows to
sums no order can round, and ties the per-kernel float64 formulas of tests/rn12_ew_ref.py to oracle/resnet12_manual.py."""
import pytest
import torch

import rn12_ew_forms as F
import rn12_ew_ref as R


@pytest.fixture(scope="module")
def hip():
    from fumi_amd import hip
    return hip


@pytest.mark.parametrize("name", list(F.MAPS))
def test_table_equals_query(name, hip):
    c, p = F.MAPS[name], F.plan_of(name)
    assert tuple(hip.RN12_EW_KEYS) == F.EW_KEYS
    for key in F.outputs_of(name):
        q = F.query(name, hip, key)
        base, tan = (key[:-2], True) if key.endswith("_t") else (key, False)
        for k in ("nch", "nrg", "rb", "nt", "first", "nt2"):
            assert q[k] == p[k], (key, k)
        assert q["gy"] == c["B"]
        if base == "act" and not tan:
            assert (q["unit"], q["active"], q["gx"], q["map_rb"]) == (1, 256, -(-p["npix"] * p["nch"] // 256), 0)
        elif base in ("act", "du"):
            assert (q["unit"], q["active"], q["map_rb"], q["gx"]) == (0, p["active"], p["map_rb"], -(-p["npix"] // p["map_rb"]))
        elif base == "red":
            assert (q["lds"], q["gx"], q["active"]) == (p["nrg"] * (3 if tan else 2) * c["C"] * 4, p["nt"], p["active"])
        elif base == "jf":
            assert (q["unit"], q["gx"]) == (1, -(-c["M"] * (c["H"] // 2 + 2) * (c["W"] // 2 + 2) * p["nch"] // 256))
        elif base == "jred":
            assert (q["lds"], q["gx"], q["wb"]) == (p["nrg"] * (5 if tan else 3) * c["C"] * 4, p["nt"], p["wb"])
        else:
            assert (q["ncy"], q["ncx"]) == (p["ncy"], p["ncx"])
            if tan:
                assert (q["cell"], q["unit"], q["cb"], q["gx"]) == (1, 1, 0, -(-p["ncell"] * p["nch"] // 256))
            else:
                assert (q["cell"], q["unit"], q["cb"], q["gx"]) == (0, 0, p["cb"], -(-p["ncell"] // p["cb"]))
                f = hip.rn12_ew_query(c["B"], c["M"], c["H"], c["W"], c["C"], "join_apply", False, form=1)
                assert (f["cell"], f["gx"]) == (1, -(-p["ncell"] * p["nch"] // 256))


def test_every_plan_form_is_reached_and_the_rows_hold_their_edges(hip):
    P = {n: F.plan_of(n) for n in F.MAPS}
    C = F.MAPS
    assert {P[n]["nrg"] for n in P} == {128, 64, 32, 21, 12, 6, 3, 1}
    assert {(P[n]["nch"], P[n]["active"]) for n in P} >= {(12, 252), (20, 240), (40, 240), (80, 240), (256, 256), (2, 256), (8, 256)}
    # the three ranges of rb, each with a partial last slab; the cap at its first point
    floor = [n for n in P if P[n]["rb"] == 64]
    assert any(P[n]["npix"] % 64 for n in floor) and any(P[n]["npix"] % 64 == 0 for n in floor)
    mid = P["rb_mid"]
    assert 64 < mid["rb"] < 1024 and mid["npix"] % 512 and mid["npix"] % mid["rb"] and mid["nt"] == 518
    assert P["rb_cap"]["npix"] == 524288 == 512 * 1024 and P["rb_cap"]["rb"] == 1024 and (524288 - 1) // 512 < 1024
    # single stage up to 128 slabs, first stage from 129; last groups of 1, 16, 6 slabs and whole groups
    assert {P[n]["nt"] for n in P} >= {1, 3, 128, 129, 144, 512, 518}
    assert [(P[n]["first"], P[n]["nt2"]) for n in ("nt128", "nt129", "nt144", "rb_cap", "rb_mid")] == [(0, 128), (1, 3), (1, 3), (1, 8), (1, 9)]
    assert {P[n]["nt"] % 64 for n in P if P[n]["first"]} >= {1, 16, 0, 6}
    # map passes: a partial last workgroup, a partial last trip of UNR 4 and of UNR 2, fewer pixels than one workgroup's share
    assert any(P[n]["npix"] % P[n]["map_rb"] and P[n]["npix"] > P[n]["map_rb"] for n in P)
    assert any(P[n]["npix"] < P[n]["map_rb"] for n in P)
    for unr in (4, 2):
        assert any(P[n]["npix"] % (unr * P[n]["nrg"]) and P[n]["npix"] > unr * P[n]["nrg"] for n in P)
    assert {C[n]["B"] for n in C} >= {1, 3, 8} and {C[n]["B"] for n in C if C[n]["chunk"]} >= {3, 8}
    assert any(C[n]["M"] > 1 and P[n]["rb"] % ((C[n]["H"] + 2) * (C[n]["W"] + 2)) for n in C)            # slabs straddle images
    # join: the sizes, windows per workgroup that do not divide, workgroups without a window, cells not a multiple of cb
    assert {(C[n]["H"], C[n]["W"]) for n in C} >= {(2, 2), (3, 3), (5, 5), (5, 8), (14, 9), (21, 21)}
    assert any(C[n]["M"] == 1 for n in C) and any(C[n]["M"] >= 40 for n in C)
    i = P["idle_3x3"]
    assert (i["nwin"], i["nt"], i["wb"]) == (40, 16, 3) and -(-i["nwin"] // i["wb"]) == 14 < i["nt"] and i["nwin"] % i["wb"] == 1
    # (nwin < nt cannot happen: a window needs at most 25 padded pixels and a slab has at least 64, so nwin / nt >= 2.56; workgroups
    #  without a window come from the rounding of wb instead)
    assert all(P[n]["nwin"] > P[n]["nt"] for n in P)
    assert any(P[n]["ncell"] % P[n]["cb"] for n in P) and any(P[n]["nwin"] % P[n]["wb"] for n in P)
    # dynamic LDS of the tangent join reduce at both ends of the channel range: nrg 5 C 4 bytes
    for n in ("c16_5x8", "c2048_3x3"):
        assert F.query(n, hip, "jred_t")["lds"] == P[n]["nrg"] * 5 * C[n]["C"] * 4 == 40960
    # coefficient rows
    K = F.COEFS
    assert {k["nt"] for k in K.values()} >= {1, 3, 128, 129, 144, 512, 2167}
    assert {k["mode"] for k in K.values()} == {"fwd", "bwd", "tfwd", "tbwd"}
    assert {(k["K"], k["ks"]) for k in K.values()} >= {(2, (0, 1, 0)), (3, (0, 1, 0)), (3, (0, 2, 0)), (5, (0, 1, 2)), (5, (0, 3, 4)), (3, (0, 1, 2))}
    assert any(k["K"] * k["C"] % 64 and k["nt"] > 128 for k in K.values()) and {96, 160} <= {k["C"] for k in K.values()}
    for name, k in K.items():
        q = hip.rn12_coef_query(k["B"], k["nt"], k["K"], k["C"], k["scratch"])
        first = int(k["nt"] > 128 and k["scratch"])
        assert q == dict(first=first, nt2=-(-k["nt"] // 64) if first else k["nt"], gx1=-(-k["nt"] // 64) if first else 0,
                         gy1=-(-k["K"] * k["C"] // 64) if first else 0, gx=-(-k["C"] // 64), gy=k["B"],
                         scratch=k["B"] * -(-k["nt"] // 64) * k["K"] * k["C"]), name
    assert hip.rn12_coef_query(2, 129, 5, 24, False)["first"] == 0 and hip.rn12_coef_query(2, 129, 5, 24, True)["first"] == 1
    # pooling: the guard (C = 64 in a workgroup of 256) and more than one workgroup column
    assert [hip.rn12_ew_query(1, bm, h, w, c, "avgpool")["gx"] for bm, h, w, c in F.POOLS.values()] == [1, 2, 3]
    assert {(h, w) for _, h, w, _ in F.POOLS.values()} == {(1, 1), (5, 5), (5, 3)} and {v[1] for v in F.PREPS.values()} == {1, 3, 8}
    for bm, h, w, c in F.POOLS.values():
        assert hip.rn12_ew_query(1, bm, h, w, c, "avgpool_bwd") ["gx"] == -(-(h + 2) * (w + 2) * c // 256)


def test_production_plans(hip):
    for (M, H, C, kind, tan), want in F.PRODUCTION:
        q = hip.rn12_ew_query(4, M, H, H, C, kind, tan)
        assert {k: q[k] for k in want} == want, (M, H, C, kind, tan, q)
    assert hip.rn12_coef_query(4, 2167, 2, 64)["nt2"] == 34


def test_query_refuses_what_the_launchers_refuse(hip):
    bad = r"invalid argument \(-1\)"
    for kind in ("act", "bwd_reduce", "bwd_apply", "join_reduce", "join_apply"):
        with pytest.raises(hip.FumiHipError) as e:
            hip.rn12_ew_query(1, 1, 4, 4, 2056, kind)
        assert "invalid argument" not in str(e.value)                 # FUMI_ENOTSUP, not FUMI_EINVAL
        assert hip.rn12_ew_query(1, 1, 4, 4, 2048, kind)["nrg"] == 1
    for args in ((0, 1, 4, 4, 32, "act"), (1, 0, 4, 4, 32, "act"), (1, 1, 0, 4, 32, "act"), (1, 1, 4, 4, 12, "act"), (1, 1, 4, 4, 0, "act"),
                 (1, 1, 1, 4, 32, "join_fwd"), (1, 1, 4, 1, 32, "join_apply"), (1, 1, 4, 4, 0, "img_prep"), (1, 1, 4, 4, 9, "img_prep")):
        with pytest.raises(hip.FumiHipError, match=bad):
            hip.rn12_ew_query(*args)
    with pytest.raises(hip.FumiHipError, match=bad):
        hip.rn12_ew_query(1, 1, 4, 4, 32, "act", False, form=1)      # the forced form is the join apply's alone
    for args in ((0, 1, 2, 16), (1, 0, 2, 16), (1, 1, 2, 4), (1, 1, 0, 16)):
        with pytest.raises(hip.FumiHipError, match=bad):
            hip.rn12_coef_query(*args)
    with pytest.raises(hip.FumiHipError):
        hip.rn12_ew_query(1, 1 << 20, 64, 64, 16, "act")             # 2^32 padded pixels: 32-bit pixel indices


@pytest.mark.parametrize("name", list(F.MAPS))
def test_integer_rows_cannot_round(name):
    """Every input is a small integer (exact in bf16), u is positive (mask 1), the tables are integers with MU = C0 = 0 and R = A = 1;
    the sum of the ABSOLUTE values of every reduction's terms stays below 2^24, so no order of fp32 additions rounds; every bf16
    output is an integer of at most 8 bits.  The join rows tie on purpose."""
    d = F.make_inputs(name, "int")
    for k, t in d.items():
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3, k
    assert float(R.act_arg(d["u"], d["coef"]).min()) >= 1
    r = F.compute(name, "int", torch.float64)
    for k, t in r.items():
        assert torch.equal(t, t.round()), k
        if k.split("_t")[0] in F.BF16_OUT:
            assert float(t.abs().max()) <= 256, k
    p = F.plan_of(name)
    for t in (False, True):
        tan = dict(ud=d["ud"], dad=d["dad"]) if t else {}
        assert float(R.bwd_terms(d["u"], d["da"], d["coef"], **tan).abs().sum(1).max()) < 2 ** 24
        jt = dict(u3d=d["ud"], usd=d["usd"], doutd=d["doutd"]) if t else {}
        assert float(R.join_terms(d["u"], d["us"], d["coef"], d["coefs"], d["dout"], **jt).abs().sum(1).max()) < 2 ** 24
    gap, _ = R.join_gaps(d["u"], d["us"], d["coef"], d["coefs"])
    assert int((gap == 0).sum()) > 0.2 * gap.numel(), "the integer join rows are there for the exact-tie rule"
    # odd maps: pixels no window covers have ds exactly zero (du3 / dus there are the BN backward of a zero ds: -A (D1 + xh D2))
    c = F.MAPS[name]
    ds = R.join_ds(d["u"], d["us"], d["coef"], d["coefs"], d["dout"])
    if c["H"] % 2:
        assert not bool(ds[:, :, c["H"]].any())
    if c["W"] % 2:
        assert not bool(ds[:, :, :, c["W"]].any())
    assert p["nwin"] > 0


@pytest.mark.parametrize("name", [n for n in F.MAPS if F.MAPS[n]["gauss"]])
def test_gauss_rows_are_repaired_and_their_allowance_is_a_rounding_test(name):
    d = F.make_inputs(name, "gauss")
    r64, e32 = F.reference(name, "gauss")
    v, gap, top = F.decisions(d)
    emax = max(e32[k] for k in e32 if k.split("_t")[0] in ("act", "jf"))          # the outputs whose arguments decide
    print(f"\n[{name}] min |v| {v:.3e} min gap {gap:.3e} min |s max| {top:.3e}; e32 " + " ".join(f"{k} {e:.1e}" for k, e in e32.items()))
    assert min(v, gap, top) > F.TIE_FLOOR
    # every decision clears 64 allowances of the VALUE it is taken on (v and s are single fused expressions of the act / join forward)
    assert F.TIE_FACTOR * F.E_FACTOR * emax < F.TIE_FLOOR
    for k, e in e32.items():
        m = float(r64[k].abs().max())
        assert m > 0 and F.E_FACTOR * e < 2.0 ** -9 * m, (k, e, m)   # a small part of one bf16 step at the output's scale


@pytest.mark.parametrize("name", list(F.COEFS))
def test_coef_rows(name):
    c = F.COEFS[name]
    d = F.coef_inputs(name, "int")
    assert float(d["part"].abs().sum(1).max()) < 2 ** 24 and torch.equal(d["part"], d["part"].round())
    (t64, dg, db), _ = F.coef_reference(name, "int")
    if c["mode"] == "fwd":                                           # the constant channel: variance 0, r = 1 / sqrt(eps)
        assert torch.equal(t64[:, R.FI["r"], 0], torch.full((c["B"],), 1.0 / float(torch.tensor(R.EPS, dtype=torch.float32)) ** 0.5, dtype=torch.float64))
    (g64, _, _), sh = F.coef_reference(name, "gauss")
    print(f"\n[{name}] float32 restatement, share of each field's maximum: " + " ".join(f"{k} {v:.1e}" for k, v in sh.items()))
    if c["mode"] == "fwd":
        dd = F.coef_inputs(name, "gauss")
        s = dd["part"].double().sum(1)
        mu = s[:, 0, 0] / dd["n"]
        assert bool((s[:, 1, 0] / dd["n"] - mu * mu < 0).all()), "channel 0 is there for the variance clamp"
        assert torch.allclose(g64[:, R.FI["r"], 0], torch.full((c["B"],), 1e-5 ** -0.5, dtype=torch.float64), rtol=1e-6)
    assert all(v < 1e-3 for v in sh.values())


# ---- the per-kernel formulas against the block algebra of oracle/resnet12_manual.py --------------------------------------------------
def _cl(x):
    """[M, C, H, W] -> [1, M, H + 2, W + 2, C] padded channels-last."""
    M, C, H, W = x.shape
    o = torch.zeros(1, M, H + 2, W + 2, C, dtype=x.dtype)
    o[0, :, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    return o


def _nchw(t):
    return t[0, :, 1:-1, 1:-1].permute(0, 3, 1, 2)


def _stats(u, dot=None):
    """what a convolution's epilogue leaves: [1, 1, 2, C] (sum, sum of u * dot or of squares) over the interior."""
    v = u[0, :, 1:-1, 1:-1]
    w = v if dot is None else dot[0, :, 1:-1, 1:-1]
    return torch.stack([v.sum((0, 1, 2)), (v * w).sum((0, 1, 2))])[None, None]


def test_reference_composes_to_resnet12_manual():
    """One 5 x 7 block, 3 images, 8 -> 16 channels, float64, no rounding: the coefficient pass, act, the BN backward, the join and
    their tangents, chained as the engine chains them, give what block_fwd / block_bwd / block_tan_fwd / block_tan_bwd give."""
    from oracle import resnet12_manual as RM
    torch.manual_seed(5)
    dt = torch.float64
    M, Ci, C, H, W = 3, 8, 16, 5, 7
    x = torch.randn(M, Ci, H, W, dtype=dt)
    mk = lambda *s: torch.randn(*s, dtype=dt) * 0.3
    def params():
        return [mk(C, Ci, 3, 3), 1 + mk(C), mk(C), mk(C, C, 3, 3), 1 + mk(C), mk(C), mk(C, C, 3, 3), 1 + mk(C), mk(C), mk(C, Ci, 1, 1), 1 + mk(C), mk(C)]
    p, pd = params(), params()
    out, tp = RM.block_fwd(x, p, RM._id)
    do = torch.randn_like(out)
    dx, grads = RM.block_bwd(do, tp, RM._id)
    xd = torch.randn_like(x)
    outd = RM.block_tan_fwd(xd, pd, tp, RM._id)
    dod = torch.randn_like(out)
    dxd, gradsd = RM.block_tan_bwd(dod, tp, RM._id)

    n = float(M * H * W)
    tabs, us = [], [_cl(u) for u in tp["u"]]
    for k in range(4):
        t, _, _ = R.coef_pass("fwd", _stats(us[k]), (0, 1, 0), n, torch.zeros(1, 13, C, dtype=dt), g=p[3 * k + 1][None], beta=p[3 * k + 2][None])
        tabs.append(t)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-9 * max(1.0, float(b.abs().max()))
    assert close(_nchw(R.act(us[0], tabs[0])), tp["a"][0]) and close(_nchw(R.act(us[1], tabs[1])), tp["a"][1])
    assert close(_nchw(R.join_fwd(us[2], us[3], tabs[2], tabs[3])), out)
    # backward: join, then BN2, BN1
    dout = _cl(do)
    part = R.join_reduce(us[2], us[3], tabs[2], tabs[3], dout, 4)
    tabs[2], dg3, db3 = R.coef_pass("bwd", part, (0, 1, 0), n, tabs[2])
    tabs[3], dgs, dbs = R.coef_pass("bwd", part, (0, 2, 0), n, tabs[3])
    du3, dus = R.join_apply(us[2], us[3], tabs[2], tabs[3], dout)
    assert close(_nchw(du3), tp["du"][2]) and close(_nchw(dus), tp["du"][3])
    assert close(dg3[0], grads[7]) and close(db3[0], grads[8]) and close(dgs[0], grads[10]) and close(dbs[0], grads[11])
    das = [_cl(tp["da"][0]), _cl(tp["da"][1])]
    for k in (1, 0):
        part = R.bwd_reduce(us[k], das[k], tabs[k], 7)
        tabs[k], dg, db = R.coef_pass("bwd", part, (0, 1, 0), n, tabs[k])
        assert close(_nchw(R.bwd_apply(us[k], das[k], tabs[k])), tp["du"][k])
        assert close(dg[0], grads[3 * k + 1]) and close(db[0], grads[3 * k + 2])
    # tangent forward: the conv epilogue leaves (sum u', sum u' u)
    uds = [_cl(u) for u in tp["ud"]]
    for k in range(4):
        tabs[k], _, _ = R.coef_pass("tfwd", _stats(uds[k], us[k]), (0, 1, 0), n, tabs[k], gd=pd[3 * k + 1][None], betad=pd[3 * k + 2][None])
    assert close(_nchw(R.act(us[0], tabs[0], uds[0])), tp["ad"][0]) and close(_nchw(R.act(us[1], tabs[1], uds[1])), tp["ad"][1])
    assert close(_nchw(R.join_fwd(us[2], us[3], tabs[2], tabs[3], uds[2], uds[3])), outd)
    # tangent backward
    doutd = _cl(dod)
    part = R.join_reduce(us[2], us[3], tabs[2], tabs[3], dout, 5, uds[2], uds[3], doutd)
    tabs[2], dg3d, db3d = R.coef_pass("tbwd", part, (0, 1, 2), n, tabs[2], gd=pd[7][None])
    tabs[3], dgsd, dbsd = R.coef_pass("tbwd", part, (0, 3, 4), n, tabs[3], gd=pd[10][None])
    du3d, dusd = R.join_apply(us[2], us[3], tabs[2], tabs[3], dout, uds[2], uds[3], doutd)
    assert close(_nchw(du3d), tp["dud"][2]) and close(_nchw(dusd), tp["dud"][3])
    assert close(dg3d[0], gradsd[7]) and close(db3d[0], gradsd[8]) and close(dgsd[0], gradsd[10]) and close(dbsd[0], gradsd[11])
    dads = [_cl(tp["dad"][0]), _cl(tp["dad"][1])]
    for k in (1, 0):
        part = R.bwd_reduce(us[k], das[k], tabs[k], 9, uds[k], dads[k])
        tabs[k], dgd, dbd = R.coef_pass("tbwd", part, (0, 1, 2), n, tabs[k], gd=pd[3 * k + 1][None])
        assert close(_nchw(R.bwd_apply(us[k], das[k], tabs[k], uds[k], dads[k])), tp["dud"][k])
        assert close(dgd[0], gradsd[3 * k + 1]) and close(dbd[0], gradsd[3 * k + 2])
    # pooling and its adjoint
    o = _cl(out)[0]
    assert close(R.avgpool(o), out.mean((2, 3)))
    df = torch.randn(M, C, dtype=dt)
    assert close(R.avgpool_bwd(df, H // 2, W // 2)[:, 1:-1, 1:-1].permute(0, 3, 1, 2), (df / ((H // 2) * (W // 2)))[:, :, None, None].expand(M, C, H // 2, W // 2))
