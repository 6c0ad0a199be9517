"""GPU suite: every form of the convolution, weight-gradient, reduce and weight-prep kernels of csrc/rn12_conv.hip against float64
(DESIGN.md section 28).  The table is tests/rn12_conv_forms.py.  Per row:

* the plan the launcher reports (fumi_hip_rn12_conv_plan) is what the library's host query gives for the shape, and, with no knob
  set, what the table spells out;
* exact-integer data (inputs and sparse +-1 weights, exact in bf16; every output's terms add up to at most 256 in absolute value,
  2^24 for the fp32 outputs -- the CPU suite asserts that): no summation order can round, the engine must EQUAL the integer
  reference, so a dropped, doubled or misplaced term of any size shows;
* Gaussian data on bf16-rounded operands: a bf16 output y must lie between RNE-bf16(r - e) and RNE-bf16(r + e), r the float64
  reference (F.conv2d per source, summed; oracle/resnet12_manual.conv_bwd_weight for dW) and e = 4 x the largest deviation of a
  CPU float32 restatement of the same operation from float64 (measured per row; the engine rounds an fp32 sum v with |v - r| <= e
  once, and rounding is monotone, so the bracket is exact for it).  dW and the statistics (against the STORED y) within 1e-5 of the
  reference's maximum;
* memory: every input map, `dot`, y, the statistics and dW sit between NaN bands, episode strides are longer than the maps and the
  gaps hold NaN (an unclamped read outside an episode poisons the result); y is pre-filled with a sentinel pattern which every
  border pixel, gap and band keeps while every interior element is written; the device status stays 0;
* rows flagged `chunk`: episode 0 of a one-episode call has the bits of episode 0 of the B-episode call (y, statistics, dW).
The table runs forward and then in reverse order in one process and must give the same bits.  The knobs are `static` in the library:
the table runs again in one fresh child process per setting (subprocess.run), one after another from a single test."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

import rn12_conv_forms as F

pytestmark = pytest.mark.gpu

ERR_FILE = "FUMI_TEST_RN12_CONV_RESULTS"    # a child appends one JSON line per case here
# One child runs test_case over the whole table: 4.5 s measured per child on an MI355X host with 16 CPUs (3 s for the default run of
# the table, the rest start-up); 120 s leaves head room for a loaded host.
CHILD_TIMEOUT = 120
FATAL = (134, 139, 124, 137)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _nan_buffer(n, dtype, dev):
    return torch.full((n + 2 * F.GUARD,), float("nan"), device=dev, dtype=dtype)


def _place_maps(x, H, W, dev, nan_border=False):
    """x [B, M, C, H, W] -> (flat bf16 buffer, view that starts at episode 0, episode stride): NaN bands, NaN gaps."""
    cl = F.to_cl(x)
    B, npix, C = cl.shape
    if nan_border:
        cl = cl.clone()
        cl[:, ~F.interior_mask(x.shape[1], H, W)] = float("nan")
    stride = npix * C + C * (W + 5)                       # a gap longer than the halo (W + 3 pixels)
    flat = _nan_buffer(B * stride, torch.bfloat16, dev)
    flat[F.GUARD:F.GUARD + B * stride].view(B, stride)[:, :npix * C] = cl.reshape(B, -1).to(torch.bfloat16).to(dev)
    return flat, flat[F.GUARD:], stride


def _digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        if t is not None:
            h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def _run(name, kind, dev, ws, one=False):
    """One call of the row on its `kind` data (one: episode 0 alone).  Returns (outputs on the CPU, plan): conv rows (y
    [B, M, Cout, H, W] float32 interior, stats or None), wgrad rows (dW,).  Checks the memory discipline and the device status."""
    from fumi_amd import hip
    c = F.CASES[name]
    d = F.make_inputs(name, kind)
    B, M, H, W = (1 if one else c["B"]), c["M"], c["H"], c["W"]
    npix = F.npix(c)
    keep = []
    if c["pass_"] == "wgrad":
        k2 = c["ntaps"]
        pairs, xs_, ds_ = [], 0, 0
        for x, dy in zip(d["x"], d["dy"]):
            fx, vx, xs_ = _place_maps(x[:B], H, W, dev)
            fd, vd, ds_ = _place_maps(dy[:B], H, W, dev)
            keep += [fx, fd]
            pairs.append((vx, vd))
        # (both pairs share the strides: equal shapes)
        n1 = c["Cout"] * c["Cin_real"] * k2
        dws = n1 + 64
        flat = _nan_buffer(B * dws, torch.float32, dev)
        hip.rn12_wgrad_multi(ws, B, M, H, W, c["Cin"], c["Cin_real"], c["Cout"], k2, pairs, xs_, ds_, flat[F.GUARD:], dws, c["nsplit"])
        plan = hip.rn12_conv_plan()[1]
        assert ws.read_status() == 0
        f = flat.cpu()
        body = f[F.GUARD:F.GUARD + B * dws].view(B, dws)
        assert bool(torch.isnan(f[:F.GUARD]).all()) and bool(torch.isnan(f[-F.GUARD:]).all()) and bool(torch.isnan(body[:, n1:]).all()), \
            f"{name}: a guard band or a gap of dW was written"
        dW = body[:, :n1].reshape(B, c["Cout"], c["Cin_real"], *((3, 3) if k2 == 9 else (1, 1))).clone()
        assert not bool(torch.isnan(dW).any()), f"{name}: {int(torch.isnan(dW).sum())} elements of dW not written (or NaN)"
        return (dW,), plan
    Cout = c["Cout"]
    srcs = []
    for s, (cin, taps, shared) in enumerate(c["srcs"]):
        fx, vx, xst = _place_maps(d["x"][s][:B], H, W, dev)
        w = d["w"][s][:1 if shared else B].contiguous().to(dev)
        keep += [fx, w]
        srcs.append((vx, xst, cin, w, 0 if shared else w[0].numel(), taps))
    dot, dst = None, 0
    if c["dot"]:
        fdot, dot, dst = _place_maps(d["dot"][:B], H, W, dev, nan_border=True)
        keep.append(fdot)
    yst = npix * Cout + Cout * (W + 5)
    ybits = torch.full((B * yst + 2 * F.GUARD,), F.SENTINEL, device=dev, dtype=torch.int16)
    yflat = ybits.view(torch.bfloat16)
    st = _nan_buffer(B * 2 * Cout, torch.float32, dev) if c["stats"] else None
    hip.rn12_conv_multi(ws, B, M, H, W, Cout, srcs, yflat[F.GUARD:], yst, transpose=c["pass_"] == "dgrad", dot=dot, dot_stride=dst,
                        stats=None if st is None else st[F.GUARD:F.GUARD + B * 2 * Cout].view(B, 2, Cout))
    plan = hip.rn12_conv_plan()[0]
    assert ws.read_status() == 0
    bits = ybits.cpu()
    written = torch.zeros(bits.numel(), dtype=torch.bool)
    inner = F.interior_mask(M, H, W)[:, None].expand(npix, Cout).reshape(-1)
    written[F.GUARD:F.GUARD + B * yst].view(B, yst)[:, :npix * Cout] = inner
    assert bool((bits[~written] == F.SENTINEL).all()), \
        f"{name}: {int((bits[~written] != F.SENTINEL).sum())} elements of a border pixel, a gap or a guard band were written"
    y = bits.view(torch.bfloat16)[F.GUARD:F.GUARD + B * yst].view(B, yst)[:, :npix * Cout].reshape(B, npix, Cout).float()
    yi = F.from_cl(y, M, H, W)[..., 1:-1, 1:-1].contiguous()
    assert not bool(torch.isnan(yi).any()), f"{name}: {int(torch.isnan(yi).sum())} interior elements not written (or NaN)"
    stats = None
    if st is not None:
        f = st.cpu()
        assert bool(torch.isnan(f[:F.GUARD]).all()) and bool(torch.isnan(f[-F.GUARD:]).all()), f"{name}: a guard band of the statistics was written"
        stats = f[F.GUARD:-F.GUARD].view(B, 2, Cout).clone()
        assert not bool(torch.isnan(stats).any()), f"{name}: statistics not written (or NaN)"
    return (yi, stats), plan


_MEASURED = {}


def _measure(name, dev, ws):
    if name not in _MEASURED:
        _MEASURED[name] = _run(name, "gauss", dev, ws)
    return _MEASURED[name]


def _no_knob_set():
    return not any(os.environ.get(k) for k in F.KNOBS)


def _record(row):
    row["env"] = F.setting_id({k: os.environ[k] for k in F.KNOBS if os.environ.get(k)})
    if os.environ.get(ERR_FILE):
        with open(os.environ[ERR_FILE], "a") as f:
            f.write(json.dumps(row) + "\n")


def _dot_of(name, kind, B=None):
    d = F.make_inputs(name, kind)["dot"]
    return None if d is None else d[:B]


@pytest.mark.parametrize("name", F.ALL_CASES)
def test_case(name, dev, ws):
    from fumi_amd import hip
    c = F.CASES[name]
    conv = c["pass_"] != "wgrad"
    outs, plan = _measure(name, dev, ws)
    r64, e32 = F.gauss_reference(name)
    row = {"case": name, "plan": plan, "query": F.query(name, hip), "e32": e32, "digest": _digest(*outs)}

    # ---- 1. the form
    assert plan == row["query"]
    if _no_knob_set():
        assert plan == F.PLANS[name]

    # ---- 2. Gaussian data against float64
    if conv:
        y, stats = outs
        e = F.E_FACTOR * e32
        lo, hi = F.bracket(r64, e)
        yd = y.double()
        row["err"] = float((yd - r64).abs().max())
        row["outside"] = int(((yd < lo) | (yd > hi)).sum())
        print(f"\n[{name}] {F.instance(plan)} e32 {e32:.2e} allowance {e:.2e} max|y - r| {row['err']:.2e} (max|r| {float(r64.abs().max()):.2f})"
              f" outside the bracket: {row['outside']}")
        if stats is not None:
            s_ref = F.stats_of(yd, _dot_of(name, "gauss"))              # of the STORED values
            row["stats_err"] = F.rel_err(stats, s_ref)
            print(f"[{name}] statistics {row['stats_err']:.2e} of the maximum")
        _record(row)
        assert row["outside"] == 0, f"{row['outside']} elements outside [bf16(r - e), bf16(r + e)], e = {e:.2e}; largest |y - r| {row['err']:.3e}"
        if stats is not None:
            assert row["stats_err"] <= F.FP32_CAP
    else:
        row["err"] = F.rel_err(outs[0], r64)
        print(f"\n[{name}] {plan} dW {row['err']:.2e} of the maximum (float32 restatement {e32 / float(r64.abs().max()):.2e})")
        _record(row)
        assert row["err"] <= F.FP32_CAP

    # ---- 3. exact-integer data, bit for bit
    outs_i, plan_i = _run(name, "int", dev, ws)
    assert plan_i == plan
    ri = F.int_reference(name)
    assert torch.equal(outs_i[0].double(), ri), f"{int((outs_i[0].double() != ri).sum())} elements differ from the integer reference " \
                                                f"(largest difference {float((outs_i[0].double() - ri).abs().max())})"
    if conv and outs_i[1] is not None:
        s_ref = F.stats_of(ri, _dot_of(name, "int"))
        assert torch.equal(outs_i[1].double(), s_ref), "statistics of the integer data differ from the exact sums"

    # ---- 4. an episode's results do not depend on how many episodes share its chunk
    if c["chunk"]:
        one, plan1 = _run(name, "gauss", dev, ws, one=True)
        assert plan1 == F.query(name, hip, B=1)
        for a, b, what in zip(one, outs, ("y", "statistics") if conv else ("dW",)):
            if a is not None:
                assert torch.equal(a[0], b[0]), f"{what} of episode 0 alone differs from episode 0 of {c['B']}: " \
                                                f"{float((a[0].double() - b[0].double()).abs().max()):.3e}"


def test_table_twice_forward_then_reverse_gives_the_same_bits(dev, ws):
    """No stale state: the workspace (fragment copies, partial sums) is reused larger-to-smaller and smaller-to-larger."""
    first = {name: _run(name, "gauss", dev, ws)[0] for name in F.ALL_CASES}
    for name in reversed(F.ALL_CASES):
        again = _run(name, "gauss", dev, ws)[0]
        for a, b in zip(first[name], again):
            assert (a is None and b is None) or torch.equal(a, b), f"{name} differs between two runs of the table"


def test_refusals_launch_nothing(dev, ws):
    """Every refusal of launch_rn_conv / launch_rn_wgrad / launch_rn_wprep through the general hooks: FUMI_EINVAL, outputs untouched."""
    from fumi_amd import hip
    H = W = 4
    npix, M = 36, 1

    def maps(C):
        return torch.zeros(npix * C, device=dev, dtype=torch.bfloat16)

    def conv(Cout, srcs, transpose=False):
        y = torch.full((npix * max(Cout, 32),), F.SENTINEL, device=dev, dtype=torch.int16)
        with pytest.raises(hip.FumiHipError, match=r"invalid argument \(-1\)"):
            hip.rn12_conv_multi(ws, 1, M, H, W, Cout, [(maps(ci), npix * ci, ci, torch.zeros(max(Cout, 32) * ci * t, device=dev), 0, t)
                                                      for ci, t in srcs], y.view(torch.bfloat16), npix * Cout, transpose=transpose)
        assert bool((y == F.SENTINEL).all()) and ws.read_status() == 0

    conv(48, [(32, 9)])                                  # Cout % 32 != 0
    conv(48, [(32, 9)], transpose=True)                  # ... which is the backward copy of a layer with Cin % 32 != 0
    conv(32, [(24, 9)])                                  # Cin % 16 != 0
    conv(32, [(48, 9)], transpose=True)                  # a backward copy of a layer with Cout % 32 != 0
    conv(32, [])                                         # nsrc 0
    conv(32, [(32, 9)] * 5)                              # nsrc 5
    conv(32, [(32, 3)])                                  # ntaps neither 1 nor 9
    conv(32, [(32, 9), (32, 4)])
    # the older single-source hook clears y itself: not when it refuses
    y = torch.full((npix * 64,), F.SENTINEL, device=dev, dtype=torch.int16)
    for cin, cout, tr in ((32, 48, 0), (24, 32, 0), (48, 32, 1)):
        rc = hip.lib().fumi_hip_rn12_conv(ws.handle, None, 1, M, H, W, cin, cout, 9, tr, maps(64).data_ptr(),
                                          torch.zeros(64 * 64 * 9, device=dev).data_ptr(), y.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == -1 and bool((y == F.SENTINEL).all())
    dW = torch.full((32 * 32 * 9,), float("nan"), device=dev)
    for kw in (dict(npair=3), dict(Cout=48), dict(Cin=24), dict(ntaps=3)):
        a = dict(dict(npair=1, Cout=32, Cin=32, ntaps=9), **kw)
        pairs = [(maps(a["Cin"]), maps(a["Cout"]))] * a["npair"]
        with pytest.raises(hip.FumiHipError, match=r"invalid argument \(-1\)"):
            hip.rn12_wgrad_multi(ws, 1, M, H, W, a["Cin"], a["Cin"], a["Cout"], a["ntaps"], pairs, npix * a["Cin"], npix * a["Cout"], dW,
                                 dW.numel())
        assert bool(torch.isnan(dW).all()) and ws.read_status() == 0


def _child_env(setting):
    env = {k: v for k, v in os.environ.items() if k not in F.KNOBS and k != ERR_FILE}
    env.update(setting)
    return env


def test_table_under_every_knob_in_subprocesses(dev, ws, tmp_path):
    """One fresh child pytest process per setting, one after another, each under its own timeout, runs test_case over the whole table
    (its plan assertion reads the library's host query IN THE CHILD, which reads the knobs) and leaves per-case JSON lines.  A child
    that ends on a signal or at its limit ends the sequence: nothing further is started."""
    assert _no_knob_set(), "the sweep starts from a process with no knob set (a child never selects this test: -k test_case)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    seen = {F.instance(_measure(n, dev, ws)[1]) for n in F.CONV_CASES}
    seen_w = {(p["ntap"], p["reduce"]) for p in (_measure(n, dev, ws)[1] for n in F.WGRAD_CASES)}
    assert seen == F.DEFAULT_INSTANCES
    for setting in F.KNOB_SETTINGS:
        sid = F.setting_id(setting)
        path = str(tmp_path / (sid.replace("=", "_") + ".jsonl"))
        env = _child_env(setting)
        env[ERR_FILE] = path
        try:
            r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_rn12_conv_forms_gpu.py"), "-q", "-m", "gpu",
                                "-p", "no:cacheprovider", "-x", "-k", "test_case"], env=env, cwd=root, capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            pytest.fail(f"{sid}: the child ran into its limit of {CHILD_TIMEOUT} s; no further child is started")
        assert r.returncode >= 0 and r.returncode not in FATAL, f"{sid}: the child ended with status {r.returncode}; no further child " \
                                                                f"is started\n" + r.stdout[-2000:] + r.stderr[-2000:]
        assert r.returncode == 0, sid + "\n" + r.stdout[-3000:] + r.stderr[-2000:]
        assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
        rows = {}
        with open(path) as f:
            for line in f:
                j = json.loads(line)
                rows[j["case"]] = j
        assert sorted(rows) == sorted(F.ALL_CASES)
        for name, j in rows.items():
            assert j["env"] == sid and j["plan"] == j["query"], name
            if F.CASES[name]["pass_"] == "wgrad":
                seen_w.add((j["plan"]["ntap"], j["plan"]["reduce"]))
            else:
                seen.add(F.instance(j["plan"]))
            if setting in F.SPEED_ONLY:              # placement / staging only: the default run's bits
                want = _digest(*_measure(name, dev, ws)[0])
                assert j["digest"] == want, f"{sid}: {name} differs from the default run"
        if setting == {"FUMI_RN_S16": "0"}:
            assert not any(j["plan"].get("s16") for j in rows.values())          # (the backward copies too: the dgrad rows)
        if setting == {"FUMI_RN_MW": "2"}:           # 255 and 256 pixels in all on ONE 256-pixel tile (t_m2_*: 256-pixel tiles by default)
            assert all(rows[n]["plan"]["mw"] == 2 for n in ("t_255", "t_256", "t_128", "t_129", "t_m2_255", "t_m2_256", "t_m2_257"))
            assert rows["t_255"]["plan"]["tiles"] == 1 and rows["t_256"]["plan"]["tiles"] == 1
        if setting in ({"FUMI_RN_WSPLIT": "1"}, {"FUMI_RN_WSLOTS": "512"}):        # the split the knob is there to move
            assert rows["w_knobs"]["plan"]["nsplit"] != F.PLANS["w_knobs"]["nsplit"], sid
    assert seen == F.INSTANCES, (F.INSTANCES - seen)
    assert seen_w == F.WGRAD_INSTANCES
