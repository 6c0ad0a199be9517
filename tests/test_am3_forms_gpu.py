"""GPU suite: every form of the AM3 step (csrc/am3.hip: am3_step_impl; DESIGN.md "AM3 form tree") against the float64 oracle.

The table (tests/am3_forms.py) holds the smallest shape that reaches each form; the plan the step reports (fumi_hip_am3_step_plan)
must be the form the row is named for.  Values: loss within LOGIT_TOL x max(1, |loss|), lamda_s within 1e-5, integer predictions
bit-exact on every safe row (and the LOWEST-numbered empty class where an empty class is nearest), `correct` and the confusion
counts recomputed on the host from the engine's own predictions, and all ten gradients plus dx_s / dx_q within GRAD_TOL = 1e-4 of the
tensor's OWN maximum (helpers.rel_to_max: no model-wide floor) -- exactly zero where they are zero analytically.  A forward-only
call returns the same loss bits and predictions; a second gradient call the same bits everywhere (the query shares arrive in any
order and are summed in share order).  The four knobs are read once per process: the table runs again in one child process per
setting."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import am3_forms as F
from helpers import rel_to_max

pytestmark = pytest.mark.gpu

DEFAULT_RUN = "FUMI_TEST_AM3_DEFAULT_RUN"          # file with the default process's predictions (the FUMI_AM3_GQ children compare)


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
    """Inputs, float64 oracle and safe rows of a case: computed once, shared by every test, never modified."""
    c, ep, w, masks = F.make_inputs(name)
    ref = F.run_oracle(c, ep, w, masks, torch.float64)
    return c, ep, w, ref, F.safe_rows(ref["dist"], ep["y_s"], c["N"])


def _step(name, dev, ws, **kw):
    from fumi_amd import hip
    c, ep, w, _, _ = _reference(name)
    g = lambda t: t.to(dev).contiguous()
    out = hip.am3_step(ws, g(ep["x_s"]), g(ep["y_s"]), g(ep["x_q"]), g(ep["y_q"]), g(ep["text_s"]), [g(w[k]) for k in hip.AM3_KEYS],
                       c["N"], c["lamda_fixed"], dropout_p=c["dropout"], seed=F.DROPOUT_SEED, **kw)
    plan = hip.am3_step_plan()
    torch.cuda.synchronize()
    return out, plan


def _grads(out):
    from fumi_amd import hip
    g = {k: t.cpu() for k, t in zip(hip.AM3_KEYS, out["grads"])}
    g["dx_s"], g["dx_q"] = out["dx_s"].cpu(), out["dx_q"].cpu()
    return g


@pytest.mark.parametrize("name", list(F.ALL_CASES))
def test_form_matches_oracle(name, dev, ws):
    from fumi_amd import hip
    from fumi_amd.utils.utils import macro_metrics
    c, ep, w, ref, (safe, ref_pred, empty, first_empty) = _reference(name)
    B, N, S, Qn = c["B"], c["N"], c["N"] * c["K"], c["N"] * c["Q"]
    stats = torch.zeros(3 + N * N, device=dev)
    g_w = [torch.full_like(w[k], float("nan")).to(dev) for k in hip.AM3_KEYS]       # every element has to be written
    out, plan = _step(name, dev, ws, want_dx=True, stats=stats, g_w=g_w)
    assert ws.read_status() == 0

    # ---- form
    want, keys = F.expected_plan(name)
    print(f"\n[{name}] plan {plan}")
    assert {k: plan[k] for k in sorted(keys)} == {k: want[k] for k in sorted(keys)}

    # ---- loss, lamda
    loss, rl = float(out["loss"]), float(ref["loss"])
    lam = out["lamda_s"].cpu()
    e_lam = rel_to_max(lam, ref["lamda_s"])
    print(f"[{name}] loss {loss:.7f} oracle {rl:.7f} rel {abs(loss - rl) / max(1.0, abs(rl)):.2e}  lamda {e_lam:.2e}")
    assert abs(loss - rl) <= F.LOGIT_TOL * max(1.0, abs(rl))
    assert e_lam <= F.LAMDA_TOL
    if c["lamda_fixed"] is not None:
        assert bool((lam == float(c["lamda_fixed"])).all())

    # ---- predictions
    preds = out["preds"].cpu()
    assert float(safe.float().mean()) >= F.SAFE_SHARE
    assert torch.equal(preds[safe], ref_pred[safe]), "integer predictions differ on safe rows"
    to_empty = safe & torch.gather(empty, 1, ref_pred)                              # an empty class is nearest:
    fe = first_empty.unsqueeze(1).expand_as(preds)
    assert torch.equal(preds[to_empty], fe[to_empty]), "exact tie of the empty classes: the lowest-numbered one wins"
    if c["ragged"] and c["plan"]["fast_head"] and N > 8:
        assert int(to_empty.sum()) > 0
    assert float(out["correct"]) == float((preds == ep["y_q"]).sum())

    # ---- confusion counts, lamda sum, device metrics
    st = stats.cpu()
    conf = np.zeros((N, N), dtype=np.float32)
    np.add.at(conf, (ep["y_q"].numpy().ravel(), preds.numpy().ravel()), 1.0)
    assert np.array_equal(st[3:].numpy().reshape(N, N), conf)
    assert float(st[1]) == float(out["correct"])
    assert abs(float(st[0]) - loss) <= 1e-6 * max(1.0, abs(loss))
    lam_sum = float(lam.to(torch.float64).mean(1).sum()) / B                          # grad_scale = 1 / B
    assert abs(float(st[2]) - lam_sum) <= F.LAMDA_TOL * max(1.0, abs(lam_sum))
    if N <= 64:
        got = hip.am3_metrics(ws, N, stats).cpu().numpy()
        np.testing.assert_allclose(got[1:5], np.array(macro_metrics(ep["y_q"].numpy(), preds.numpy())), rtol=3e-6, atol=1e-7)
        assert got[0] == float(st[0]) and got[5] == float(st[2])

    # ---- gradients: own scale
    got = _grads(out)
    zero = F.zero_grads(c)
    errs = {}
    for k, r in ref["all_grads"].items():
        assert bool(torch.isfinite(got[k]).all()), f"{k}: not written or not finite"
        errs[k] = float(got[k].abs().max()) if k in zero else rel_to_max(got[k], r)
    worst = max(errs, key=errs.get)
    print(f"[{name}] grad errors (own scale) " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    print(f"[{name}] worst {worst} {errs[worst]:.2e}")
    for k, e in errs.items():
        if k in zero:
            assert bool((got[k] == 0).all()), f"{k}: analytically zero, engine max {e:.3e}"
        else:
            assert e <= F.GRAD_TOL, f"grad {k}: error {e:.3e} of its own maximum"

    # ---- determinism (no stats this time: the form without confusion counts)
    out2, _ = _step(name, dev, ws, want_dx=True)
    got2 = _grads(out2)
    for k in got:
        assert torch.equal(got[k], got2[k]), f"{k} differs between two calls"
    assert torch.equal(out["loss"], out2["loss"]) and torch.equal(out["preds"], out2["preds"])

    # ---- forward only
    out3, _ = _step(name, dev, ws, need_grad=False)
    assert torch.equal(out["loss"], out3["loss"]) and torch.equal(out["preds"], out3["preds"])
    assert torch.equal(out["correct"], out3["correct"]) and torch.equal(out["lamda_s"], out3["lamda_s"])
    assert ws.read_status() == 0

    # ---- a fixed number of query shares decides nothing: same integers as the default process
    if os.environ.get(DEFAULT_RUN):
        d = np.load(os.environ[DEFAULT_RUN])
        assert np.array_equal(d[name + ".preds"], preds.numpy()) and float(d[name + ".correct"]) == float(out["correct"])


def _child_env(knob, value):
    env = {k: v for k, v in os.environ.items() if k not in F.KNOBS and k != DEFAULT_RUN}
    env[knob] = value
    return env


@pytest.mark.parametrize("knob,value", F.KNOB_SETTINGS, ids=[f"{k}={v}" for k, v in F.KNOB_SETTINGS])
def test_table_under_knob_in_subprocess(knob, value, dev, ws, tmp_path):
    """The knobs are `static` in the library: one child pytest process per setting runs the table again.  A row whose form the knob
    overrides checks values against the oracle; its plan assertion reads the knob (am3_forms.expected_plan)."""
    env = _child_env(knob, value)
    if knob == "FUMI_AM3_GQ":
        rec = {}
        for name in F.ALL_CASES:
            out, _ = _step(name, dev, ws, need_grad=False)
            rec[name + ".preds"], rec[name + ".correct"] = out["preds"].cpu().numpy(), out["correct"].cpu().numpy()
        path = str(tmp_path / "default_run.npz")
        np.savez(path, **rec)
        env[DEFAULT_RUN] = path
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_am3_forms_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider", "-k", "test_form_matches_oracle"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
