"""GPU suite: every kernel form of the two X-panel passes (csrc/xpanel.hip) against a float64 product.

The table (tests/xpanel_forms.py) holds the smallest shape that reaches each form and each of its tile edges.  Per case:
the plan the launcher reports (fumi_hip_xpanel_plan) is the one the table expects; A0 and gW0 within 2e-6 and G within 4e-6 of the
float64 reference's maximum; the outputs sit between two bands of 256 NaN floats that stay NaN while every output element is
written; zero rows give exact zeros; a power-of-two rescaling of the operands gives the same bits; the device status stays 0.
The whole table runs twice in one process, forward and then in reverse order, and must give the same bits (the plane buffer and the
workspace are reused larger-to-smaller and smaller-to-larger).  The knobs are `static` in the library: the table runs again in one
child process per setting, each child leaves its per-case errors as JSON lines, and a split-bf16 form must be no worse than the fp32
MFMA form of the same case (err_split <= 1.5 err_fp32 + 5e-8)."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import xpanel_forms as F

pytestmark = pytest.mark.gpu

ERR_FILE = "FUMI_TEST_XPANEL_ERRORS"        # a child appends one JSON line per case here
REPORT = "FUMI_TEST_XPANEL_REPORT"          # optional: every process appends its per-case errors to this file (evidence runs)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Inputs and float64 reference of a case: computed once, shared by every test, never modified."""
    d = F.make_inputs(name)
    return d, tuple(F.reference(name, d))


def _place(t, dev, off):
    """A contiguous device copy that starts ``off`` floats past an allocation's (16-byte aligned) start."""
    flat = torch.empty(t.numel() + 4, device=dev, dtype=torch.float32)
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (off % 4 == 0)
    return v


def _guarded(shape, dev):
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * F.GUARD,), float("nan"), device=dev, dtype=torch.float32)
    return flat, flat[F.GUARD:F.GUARD + n].view(shape)


def _run(name, d, dev, ws, scale=None):
    """One call of the case's pass on inputs ``d`` (CPU tensors): outputs on the CPU and the reported plan.  Checks the guard bands,
    that every output element was written, and the device status."""
    from fumi_amd import hip
    c = F.CASES[name]
    t = {k: (None if v is None else _place(v, dev, 1 if c["align"] == k else 0)) for k, v in d.items()}
    B, D, h0 = c["B"], c["D"], c["h0"]
    if c["pass_"] == "fwd":
        bufs = [_guarded((B, c["S"] + c["Qn"], h0), dev), _guarded((B, c["S"] + c["Qn"], c["S"]), dev)]
        hip.xpanel_fwd(ws, t["x_s"], t["x_q"], t["W0"], out=(bufs[0][1], bufs[1][1]))
    else:
        bufs = [_guarded((h0, D), dev)]
        hip.xpanel_bwd(ws, t["x_s"], t["x_q"], t["Abar"], scale=c["scale"] if scale is None else scale, out=bufs[0][1])
    plan = hip.xpanel_plan()
    assert ws.read_status() == 0
    outs = []
    for flat, view in bufs:
        f = flat.cpu()
        assert bool(torch.isnan(f[:F.GUARD]).all()) and bool(torch.isnan(f[-F.GUARD:]).all()), f"{name}: a guard band was written"
        o = f[F.GUARD:-F.GUARD].view(view.shape).clone()
        assert not bool(torch.isnan(o).any()), f"{name}: {int(torch.isnan(o).sum())} output elements not written (or NaN)"
        outs.append(o)
    keys = F.FWD_KEYS if c["pass_"] == "fwd" else F.BWD_KEYS
    return outs, {k: plan[k] for k in keys}


_MEASURED = {}


def _measure(name, dev, ws):
    """(outputs, plan, errors against float64) of the unmodified case in this process: one call, shared."""
    if name not in _MEASURED:
        d, ref = _reference(name)
        outs, plan = _run(name, d, dev, ws)
        labels = ("A0", "G") if F.CASES[name]["pass_"] == "fwd" else ("gW0",)
        _MEASURED[name] = (outs, plan, {k: F.rel_err(o, r) for k, o, r in zip(labels, outs, ref)})
    return _MEASURED[name]


def _no_knob_set():
    return not any(os.environ.get(k) for k in F.KNOBS)


def _record(name, plan, errs):
    line = json.dumps({"case": name, "env": F.setting_id({k: os.environ[k] for k in F.KNOBS if os.environ.get(k)}) or "default",
                       "plan": plan, "errs": errs})
    for var in (ERR_FILE, REPORT):
        if os.environ.get(var):
            with open(os.environ[var], "a") as f:
                f.write(line + "\n")


@pytest.mark.parametrize("name", F.ALL_CASES)
def test_case(name, dev, ws):
    c = F.CASES[name]
    d, ref = _reference(name)
    outs, plan, errs = _measure(name, dev, ws)
    fam = (F.FWD_KERNELS if c["pass_"] == "fwd" else F.BWD_KERNELS)[plan[c["pass_"] + "_kernel"]]
    print(f"\n[{name}] {fam} plan {plan} errors " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    _record(name, plan, errs)

    # ---- 1. the form
    assert plan == F.expected_plan(name)
    if _no_knob_set():
        assert {k: plan[k] for k in F.table_plan(name)} == F.table_plan(name)

    # ---- 2. accuracy against float64
    for k, e in errs.items():
        assert e <= (F.G_TOL if k == "G" else F.A0_TOL), f"{k}: {e:.3e} of the reference's maximum"

    if c["pass_"] == "fwd":
        B, S = c["B"], c["S"]
        # ---- 5. exact zeros: a zero support row (episode B-1) and a zero query row (episode 0)
        z = dict(d, x_s=d["x_s"].clone(), x_q=d["x_q"].clone())
        z["x_s"][B - 1, S // 2] = 0.0
        z["x_q"][0, 0] = 0.0
        (A0, G), _ = _run(name, z, dev, ws)
        assert bool((A0[B - 1, S // 2] == 0).all()) and bool((G[B - 1, S // 2] == 0).all()), "zero support row: nonzero output row"
        assert bool((A0[0, S] == 0).all()) and bool((G[0, S] == 0).all()), "zero query row: nonzero output row"
        assert bool((G[B - 1, :, S // 2] == 0).all()), "zero support row: nonzero Gram column"
        # ---- 6. powers of two: X 2^20, W0 2^-12 -> A0 2^8, G 2^40, the same bits
        s = dict(d, x_s=d["x_s"] * 2.0 ** 20, x_q=d["x_q"] * 2.0 ** 20, W0=d["W0"] * 2.0 ** -12)
        (A1, G1), _ = _run(name, s, dev, ws)
        assert torch.equal(A1 * 2.0 ** -8, outs[0]), f"A0 rescaled: {F.rel_err(A1 * 2.0 ** -8, ref[0]):.3e}"
        assert torch.equal(G1 * 2.0 ** -40, outs[1]), f"G rescaled: {F.rel_err(G1 * 2.0 ** -40, ref[1]):.3e}"
    else:
        # ---- 5. a zero row of Abar: the X row it meets decides nothing
        side = "x_s" if d["x_s"] is not None else "x_q"
        b, r = c["B"] - 1, d["Abar"].shape[1] // 2
        z = dict(d, Abar=d["Abar"].clone())
        z["Abar"][b, r] = 0.0
        (g0,), _ = _run(name, z, dev, ws)
        if d["x_s"] is not None and d["x_q"] is not None:
            side, r = ("x_s", r) if r < c["S"] else ("x_q", r - c["S"])
        z[side] = d[side].clone()
        z[side][b, r] = 12345.678 * torch.randn(c["D"], generator=torch.Generator().manual_seed(1))
        (g1,), _ = _run(name, z, dev, ws)
        assert torch.equal(g0, g1), "a zero row of Abar: gW0 depends on the X row it multiplies"
        # ---- 6. powers of two: Abar 2^-20 -> gW0 2^-20, the same bits
        (g2,), _ = _run(name, dict(d, Abar=d["Abar"] * 2.0 ** -20), dev, ws)
        assert torch.equal(g2 * 2.0 ** 20, outs[0]), f"gW0 rescaled: {F.rel_err(g2 * 2.0 ** 20, ref[0]):.3e}"


@pytest.mark.parametrize("name", [n for n, c in F.CASES.items() if c["sides"]])
def test_one_sided_panels_add_up_to_the_two_sided_call(name, dev, ws):
    """S = 0 and Qn = 0 (what the two-launch backward of run_episodes passes): each against the float64 product over its rows in
    test_case; here their sum against the two-sided call and its reference."""
    (both,), _, _ = _measure(name, dev, ws)
    (gq,), _, _ = _measure(name + "_s0", dev, ws)
    (gs,), _, _ = _measure(name + "_q0", dev, ws)
    ref = _reference(name)[1][0]
    total = gq.double() + gs.double()
    e_ref = F.rel_err(total, ref)
    e_both = float((total - both.double()).abs().max() / ref.abs().max())
    print(f"\n[{name}] one-sided sum: {e_ref:.2e} of float64, {e_both:.2e} of the two-sided call")
    assert e_ref <= F.A0_TOL and e_both <= F.A0_TOL


def test_table_twice_forward_then_reverse_gives_the_same_bits(dev, ws):
    """No stale state: the plane buffer (ws->w0p) and the workspace are reused larger-to-smaller and smaller-to-larger."""
    first = {}
    for name in F.ALL_CASES:
        first[name], _ = _run(name, _reference(name)[0], dev, ws)
    for name in reversed(F.ALL_CASES):
        again, _ = _run(name, _reference(name)[0], dev, ws)
        for a, b in zip(first[name], again):
            assert torch.equal(a, b), f"{name} differs between two runs of the table"
    # the planes are rebuilt every call: a changed weight must show, also after a larger case has used them
    _run("f_ps_d512_h256", _reference("f_ps_d512_h256")[0], dev, ws)
    d, ref = _reference("f_ps_d288")
    (A1, _), plan = _run("f_ps_d288", dict(d, W0=2.0 * d["W0"]), dev, ws)
    assert F.rel_err(A1, 2.0 * ref[0]) <= F.A0_TOL
    if plan["fwd_kernel"] == 5:
        assert torch.equal(A1, 2.0 * first["f_ps_d288"][0])


def _child_env(setting):
    env = {k: v for k, v in os.environ.items() if k not in F.KNOBS and k != ERR_FILE}
    env.update(setting)
    return env


@pytest.mark.parametrize("setting", F.KNOB_SETTINGS, ids=[F.setting_id(s) for s in F.KNOB_SETTINGS])
def test_table_under_knob_in_subprocess(setting, dev, ws, tmp_path):
    """One child pytest process per setting runs test_case over the whole table (its plan assertion reads the knobs:
    xpanel_forms.expected_plan) and leaves its per-case errors as JSON lines.  The child is not run again if it fails."""
    env = _child_env(setting)
    path = str(tmp_path / "errors.jsonl")
    env[ERR_FILE] = path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_xpanel_forms_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider", "-k", "test_case"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
    rows = {}
    with open(path) as f:
        for line in f:
            j = json.loads(line)
            rows[j["case"]] = j
    assert sorted(rows) == sorted(F.ALL_CASES)
    for name, j in rows.items():
        assert j["plan"] == F.expected_plan(name, setting), name
    # a split-bf16 form is no worse than the exact-fp32 MFMA form the same case takes with the split switched off
    off = {"fwd": "FUMI_XP_SB", "bwd": "FUMI_XPB_SB"}
    for name, j in rows.items():
        p = F.CASES[name]["pass_"]
        if setting.get(off[p]) != "0" or j["plan"][p + "_kernel"] > 3:
            continue
        _, plan, errs = _measure(name, dev, ws)
        if plan[p + "_kernel"] < 4:              # (this process runs under a knob of its own: nothing to compare)
            continue
        for k, e in errs.items():
            print(f"[{name}] {k}: split {e:.2e} fp32 MFMA {j['errs'][k]:.2e}")
            assert e <= 1.5 * j["errs"][k] + 5e-8, f"{name} {k}: split {e:.3e}, fp32 MFMA {j['errs'][k]:.3e}"
