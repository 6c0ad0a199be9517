"""GPU suite: the Gram tiles of the pre-split forward X-panel pass split their own column operand (csrc/xpanel.hip).

By default a Gram tile (128 rows x 32 support columns) fetches its 32 support rows as fp32, splits them once per tile into the three
bf16 pieces and stages them in LDS beside its rows of X; `FUMI_XP_GSPLIT=0` restores the planes the pre-split launch used to write
for them.  The pieces are the same bits in the same MFMA order, so every output is the same bits.

Shapes: the pre-split form needs D / 32 >= 9 slabs, so D = 128 and D = 192 never reach it: D = 288 (9 slabs: the smallest accepted,
odd, not a power of two) and D = 320 (10 slabs: the smallest accepted even count) stand in.  h0 = 128; S in {1, 25, 31, 32, 33, 40}
(masking inside a column block, a full block, two blocks); Qn in {7, 135} (one and two 128-row tiles, ragged); B in {1, 3, 9}
(one and two episodes per XCD slot, not a multiple of 8); one case through the index table with a permuted idx_s; one without G.

Per case: (a) A0 and G under FUMI_XP_GSPLIT=0 (one fresh child process for the whole table: the knob is read once) are bit-equal
to the default; (b) A0 within 2e-6 and G within 4e-6 of a float64 product's maximum, the bounds of
test_hip_parity.py::test_xpanel_fwd_presplit_column_operand_has_fp32_accuracy; (c) NaN behind x_s (and in every table row no index
names) leaves G finite, and the NaN bands around A0 and G stay NaN; (d) the plan names the in-tile form by default and the planes
under the knob, and the planes in use are 3 * h0 * D * 2 bytes by default."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KNOB = "FUMI_XP_GSPLIT"
A0_TOL, G_TOL = 2e-6, 4e-6            # test_hip_parity.py::test_xpanel_fwd_presplit_column_operand_has_fp32_accuracy
GUARD = 256
H0 = 128
#        name              B  S   Qn   D    rows     gram
CASES = {"s1":            (1, 1,  7,   288, "dense", True),
         "s25_two_tiles": (3, 25, 135, 320, "dense", True),
         "s31":           (9, 31, 7,   288, "dense", True),
         "s32_full":      (3, 32, 135, 288, "dense", True),
         "s33_two_blocks": (9, 33, 135, 320, "dense", True),
         "s40":           (1, 40, 7,   320, "dense", True),
         "table_permuted": (3, 25, 7,  288, "table", True),
         "no_gram":       (3, 25, 7,   288, "table", False)}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """CPU inputs and the float64 reference of a case: computed once, shared, never modified."""
    B, S, Qn, D, rows, gram = CASES[name]
    g = torch.Generator().manual_seed(1000 * B + 10 * S + D + Qn)
    x_s = torch.randn(B, S, D, generator=g).abs()
    x_q = torch.randn(B, Qn, D, generator=g) * 3.0
    W0 = torch.randn(H0, D, generator=g) * 0.05
    X = torch.cat([x_s, x_q], 1).double()
    ref = (X @ W0.double().T, X @ x_s.double().transpose(1, 2))
    d = dict(x_s=x_s, x_q=x_q, W0=W0)
    if rows == "table":
        # every row lives once in a table at a shuffled place; the rows no index names are NaN
        n = B * (S + Qn)
        n_rows = n + 17
        place = torch.randperm(n_rows, generator=g)[:n]
        table = torch.full((n_rows, D), float("nan"))
        table[place] = torch.cat([x_s.reshape(-1, D), x_q.reshape(-1, D)], 0)
        d.update(table=table, idx_s=place[:B * S].view(B, S).contiguous(), idx_q=place[B * S:].view(B, Qn).contiguous())
    return d, ref


def _guarded(shape, dev):
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * GUARD,), float("nan"), device=dev, dtype=torch.float32)
    return flat, flat[GUARD:GUARD + n].view(shape)


def _run(name, dev, ws):
    """One forward of the case: A0, G (None without a Gram block) as CPU tensors, the plan, the planes in use."""
    from fumi_amd import hip
    B, S, Qn, D, rows, gram = CASES[name]
    d, _ = _inputs(name)
    fa, A0 = _guarded((B, S + Qn, H0), dev)
    fg, G = _guarded((B, S + Qn, S), dev)
    if rows == "table":
        hip.xpanel_fwd_rows(ws, d["table"].to(dev), d["idx_s"].to(dev), d["idx_q"].to(dev), d["W0"].to(dev), gram=gram,
                            out=(A0, G) if gram else (A0, None))
    else:
        # x_s is followed by 64 rows of NaN in its own allocation: a support row fetched past column S - 1 would show
        flat = torch.full(((B * S + 64) * D,), float("nan"), device=dev, dtype=torch.float32)
        x_s = flat[:B * S * D].view(B, S, D)
        x_s.copy_(d["x_s"])
        hip.xpanel_fwd(ws, x_s, d["x_q"].to(dev), d["W0"].to(dev), out=(A0, G))
    plan, planes = hip.xpanel_plan(), hip.xpanel_planes_bytes()
    assert ws.read_status() == 0
    fa, fg = fa.cpu(), fg.cpu()
    for f in (fa, fg):
        assert bool(torch.isnan(f[:GUARD]).all()) and bool(torch.isnan(f[-GUARD:]).all()), f"{name}: a guard band was written"
    A0 = fa[GUARD:-GUARD].view(A0.shape).clone()
    G = fg[GUARD:-GUARD].view(G.shape).clone()
    if not gram:
        assert bool(torch.isnan(G).all()), f"{name}: G written though none was asked for"
        G = None
    return A0, G, plan, planes


def _run_table(dev, ws):
    out = {}
    for name in CASES:
        A0, G, plan, planes = _run(name, dev, ws)
        out[name] = dict(A0=A0.numpy(), G=None if G is None else G.numpy(), plan=plan, planes=planes)
    return out


def _child_table(setting, tmp):
    """The whole table in one fresh child process with the knob set to ``setting`` (None: unset)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != KNOB}
    if setting is not None:
        env[KNOB] = setting
    path = os.path.join(str(tmp), "table.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(path)
    meta = json.loads(str(z["meta"]))
    return {name: dict(A0=z[name + ".A0"], G=z[name + ".G"] if name + ".G" in z.files else None, plan=meta[name]["plan"],
                       planes=meta[name]["planes"]) for name in CASES}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tables(dev, tmp_path_factory):
    """{"tile": ..., "planes": ...}: the table under the default and under FUMI_XP_GSPLIT=0.  The form this process itself runs
    (normally the default) is computed here, the other one in a single child."""
    from fumi_amd import hip
    here = os.environ.get(KNOB)
    mine = "planes" if here is not None and int(here) == 0 else "tile"
    t = {mine: _run_table(dev, hip.Workspace.get(dev))}
    other = "planes" if mine == "tile" else "tile"
    t[other] = _child_table("0" if other == "planes" else None, tmp_path_factory.mktemp("gsplit"))
    return t


@pytest.mark.parametrize("name", list(CASES))
def test_knob_gives_the_same_bits(name, tables):
    a, b = tables["tile"][name], tables["planes"][name]
    assert a["A0"].tobytes() == b["A0"].tobytes(), "A0 differs between the in-tile split and the planes"
    if CASES[name][5]:
        assert a["G"].tobytes() == b["G"].tobytes(), "G differs between the in-tile split and the planes"
    else:
        assert a["G"] is None and b["G"] is None


@pytest.mark.parametrize("form", ["tile", "planes"])
@pytest.mark.parametrize("name", list(CASES))
def test_float64_accuracy_and_finite_columns(name, form, tables):
    r = tables[form][name]
    _, (A0r, Gr) = _inputs(name)
    ea = float((torch.from_numpy(r["A0"]).double() - A0r).abs().max() / A0r.abs().max())
    print(f"\n[{name} {form}] A0 {ea:.2e}", end="")
    assert np.isfinite(r["A0"]).all()
    assert ea < A0_TOL
    if CASES[name][5]:
        assert np.isfinite(r["G"]).all(), "a Gram column is not finite: a row past S - 1 was read and kept"
        eg = float((torch.from_numpy(r["G"]).double() - Gr).abs().max() / Gr.abs().max())
        print(f" G {eg:.2e}")
        assert eg < G_TOL


@pytest.mark.parametrize("name", list(CASES))
def test_plan_names_the_form_and_the_planes_in_use(name, tables):
    from fumi_amd import hip
    B, S, Qn, D, rows, gram = CASES[name]
    cbg = (S + 31) // 32 if gram else 0
    w0_bytes = 3 * H0 * D * 2
    for form, planes in (("tile", w0_bytes), ("planes", w0_bytes + B * 3 * cbg * 32 * D * 2)):
        r = tables[form][name]
        assert hip.XPANEL_FWD_KERNELS[r["plan"]["fwd_kernel"]] == "presplit", r["plan"]
        assert hip.XPANEL_GRAM_SPLIT[r["plan"]["fwd_gram_split"]] == form, r["plan"]
        assert r["plan"]["fwd_gram_blocks"] == cbg
        assert r["planes"] == planes, f"{form}: {r['planes']} bytes of planes in use, expected {planes}"


if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    from fumi_amd import hip as _hip
    _dev = torch.device("cuda:0")
    res = _run_table(_dev, _hip.Workspace.get(_dev))
    arrays = {"meta": np.array(json.dumps({n: dict(plan=r["plan"], planes=r["planes"]) for n, r in res.items()}))}
    for n, r in res.items():
        arrays[n + ".A0"] = r["A0"]
        if r["G"] is not None:
            arrays[n + ".G"] = r["G"]
    np.savez(sys.argv[1], **arrays)
