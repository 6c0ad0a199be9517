"""GPU suite: the text-rows form of the AM3 step (csrc/am3.hip: fumi_hip_am3_step_tx; text_encoder='rand', am3.py:118-126) against
the float64 oracle, through the C ABI binding ``hip.am3_step_tx``.

Every case of tests/am3_rand.py runs two ways: prototype-space rows given (form 1) and rows drawn on the device (form 2: ``tx`` must
be the host restatement of the draw bit for bit).  The oracle is ``oracle.fumi_ref.am3_step`` with an exact identity in g's place at
its own hidden width 2P and masks = (ones, h's mask of tag 2); tolerances and the safe-row treatment of the integer predictions are
those of tests/am3_forms.py.  The knob FUMI_AM3_MLP is read once per process: the fused case runs again in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import am3_forms as F
import am3_rand as A
from helpers import rel_to_max

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
MLP_FUSED = int(os.environ.get("FUMI_AM3_MLP", "1")) != 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _weights(c, w, dev, with_g):
    """(w, g_w) lists for the binding: g's slots None, or poisoned tensors of arbitrary shape that must come back untouched."""
    from fumi_amd import hip
    wl = [w[k].to(dev).contiguous() for k in hip.AM3_KEYS]
    gl = [torch.full_like(t, float("nan")) for t in wl]                       # every element has to be written
    for i in range(2, 6):
        wl[i] = torch.full((3, 5), SENTINEL, device=dev) if with_g else None
        gl[i] = torch.full((3, 5), SENTINEL, device=dev) if with_g else None
    return wl, gl


def _step(name, form, dev, ws, seed=A.SEED, with_g=False, dropout=None, **kw):
    from fumi_amd import hip
    c, ep, w, _, _ = A.reference(name, form)
    g = lambda t: t.to(dev).contiguous()
    wl, gl = _weights(c, w, dev, with_g)
    out = hip.am3_step_tx(ws, g(ep["x_s"]), g(ep["y_s"]), g(ep["x_q"]), g(ep["y_q"]), g(ep["rows"]) if form == "given" else None, wl,
                          c["N"], c["lamda_fixed"], dropout_p=c["dropout"] if dropout is None else dropout, seed=seed,
                          g_w=gl if kw.get("need_grad", True) else None, **kw)
    plan = hip.am3_step_plan()
    torch.cuda.synchronize()
    out["w_in"] = wl
    return out, plan


def _grads(out):
    from fumi_amd import hip
    g = {k: t.cpu() for k, t in zip(hip.AM3_KEYS, out["grads"]) if k not in A.G_KEYS}
    g["dx_s"], g["dx_q"] = out["dx_s"].cpu(), out["dx_q"].cpu()
    return g


@pytest.mark.parametrize("form", A.FORMS)
@pytest.mark.parametrize("name", list(A.CASES))
def test_text_rows_form_matches_oracle(name, form, dev, ws):
    c, ep, w, ref, (safe, ref_pred, empty, first_empty) = A.reference(name, form)
    B, N, S, Qn, P = c["B"], c["N"], c["N"] * c["K"], c["N"] * c["Q"], c["P"]
    stats = torch.zeros(3 + N * N, device=dev)
    out, plan = _step(name, form, dev, ws, with_g=True, want_dx=True, stats=stats)
    assert ws.read_status() == 0

    # ---- form: g is not in the plan; h takes the fused kernels where the case is named for them
    print(f"\n[{name}/{form}] plan {plan}")
    assert plan["text_form"] == (1 if form == "given" else 2)
    assert [plan[k] for k in ("g_fwd_split", "g_fwd_rode", "g_bwd_fused", "tx_nparts")] == [0, 0, 0, 0]
    assert plan["fast_head"] == 1
    h_fused = int(MLP_FUSED and c["Ht"] % 64 == 0 and c["lamda_fixed"] is None)      # the fused kernels take whole 64-column chunks
    assert (plan["h_fwd_split"], plan["h_bwd_fused"]) == (h_fused, h_fused)
    assert h_fused == (1 if (name == "fused" and MLP_FUSED) else 0)

    # ---- the rows the step used
    tx = out["tx"].cpu()
    assert tx.shape == (B, S, P)
    if form == "drawn":
        assert torch.equal(tx, A.draw_rows(A.SEED, B * S, P).reshape(B, S, P)), "the device draw is not the host restatement"
        assert float(tx.min()) >= -1.0 and float(tx.max()) < 1.0
    assert torch.equal(tx, ep["rows"])

    # ---- g untouched: weights and gradients of slots 2..5 keep the sentinel
    for i in range(2, 6):
        assert bool((out["w_in"][i] == SENTINEL).all()) and bool((out["grads"][i] == SENTINEL).all())

    # ---- loss, lamda
    loss, rl = float(out["loss"]), float(ref["loss"])
    lam = out["lamda_s"].cpu()
    e_lam = rel_to_max(lam, ref["lamda_s"])
    print(f"[{name}/{form}] loss {loss:.7f} oracle {rl:.7f} rel {abs(loss - rl) / max(1.0, abs(rl)):.2e}  lamda {e_lam:.2e}")
    assert abs(loss - rl) <= F.LOGIT_TOL * max(1.0, abs(rl))
    assert e_lam <= F.LAMDA_TOL
    if c["lamda_fixed"] is not None:
        assert bool((lam == float(c["lamda_fixed"])).all())

    # ---- predictions on margin-safe rows, correct
    preds = out["preds"].cpu()
    assert float(safe.float().mean()) >= F.SAFE_SHARE
    assert torch.equal(preds[safe], ref_pred[safe]), "integer predictions differ on safe rows"
    to_empty = safe & torch.gather(empty, 1, ref_pred)
    fe = first_empty.unsqueeze(1).expand_as(preds)
    assert torch.equal(preds[to_empty], fe[to_empty]), "exact tie of the empty classes: the lowest-numbered one wins"
    assert float(out["correct"]) == float((preds == ep["y_q"]).sum())

    # ---- the stats tail
    st = stats.cpu()
    conf = np.zeros((N, N), dtype=np.float32)
    np.add.at(conf, (ep["y_q"].numpy().ravel(), preds.numpy().ravel()), 1.0)
    assert np.array_equal(st[3:].numpy().reshape(N, N), conf)
    assert float(st[1]) == float(out["correct"])
    assert abs(float(st[0]) - loss) <= 1e-6 * max(1.0, abs(loss))
    lam_sum = float(lam.to(torch.float64).mean(1).sum()) / B                          # grad_scale = 1 / B
    assert abs(float(st[2]) - lam_sum) <= F.LAMDA_TOL * max(1.0, abs(lam_sum))

    # ---- gradients of the image encoder and of h, dx: own scale; exactly zero where they are zero analytically
    got = _grads(out)
    zero = A.zero_grads(c)
    cancel = A.cancelling_sums(name, form)              # zero analytically, a sum of non-zero adjoints in fp32: scale of the summands
    errs = {}
    for k in got:
        r = ref["all_grads"][k]
        assert bool(torch.isfinite(got[k]).all()), f"{k}: not written or not finite"
        if k in zero:
            errs[k] = float(got[k].abs().max())
        elif k in cancel:
            errs[k] = float((got[k].to(torch.float64) - r).abs().max()) / cancel[k]
        else:
            errs[k] = rel_to_max(got[k], r)
    print(f"[{name}/{form}] grad errors (own scale) " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    for k, e in errs.items():
        if k in zero:
            assert bool((got[k] == 0).all()), f"{k}: analytically zero, engine max {e:.3e}"
        else:
            assert e <= F.GRAD_TOL, f"grad {k}: error {e:.3e} of its own maximum"

    # ---- the same seed: the same bits everywhere, with None in g's slots; forward only: the same loss bits and predictions
    out2, _ = _step(name, form, dev, ws, want_dx=True)
    assert out2["grads"][2:6] == [None] * 4
    got2 = _grads(out2)
    for k in got:
        assert torch.equal(got[k], got2[k]), f"{k} differs between two calls"
    for k in ("loss", "preds", "lamda_s", "correct", "tx"):
        assert torch.equal(out[k], out2[k]), f"{k} differs between two calls"
    out3, _ = _step(name, form, dev, ws, need_grad=False)
    for k in ("loss", "preds", "lamda_s", "correct", "tx"):
        assert torch.equal(out[k], out3[k]), f"{k} differs in the forward-only call"
    assert ws.read_status() == 0


def test_another_seed_draws_other_rows(dev, ws):
    a, _ = _step("small_p", "drawn", dev, ws, need_grad=False)
    b, _ = _step("small_p", "drawn", dev, ws, seed=A.SEED_B, need_grad=False)
    c = A.CASES["small_p"]
    rows, P = c["B"] * c["N"] * c["K"], c["P"]
    assert not torch.equal(a["tx"], b["tx"])
    assert torch.equal(b["tx"].cpu().reshape(rows, P), A.draw_rows(A.SEED_B, rows, P))


def test_draw_tail_and_unaligned_sizes(dev, ws):
    """Rs * P no multiple of 4: the float4 body and the scalar tail meet without a gap (B * S * P = 1 * 3 * 3 and 2 * 3 * 7)."""
    from fumi_amd import hip
    for (B, N, P) in ((1, 3, 3), (2, 3, 7)):
        x_s, x_q = torch.randn(B, N, 32, device=dev), torch.randn(B, N, 32, device=dev)
        y = torch.arange(N, device=dev).repeat(B, 1)
        w = [torch.randn(P, 32, device=dev), torch.zeros(P, device=dev), None, None, None, None,
             torch.randn(4, P, device=dev), torch.zeros(4, device=dev), torch.randn(1, 4, device=dev), torch.zeros(1, device=dev)]
        out = hip.am3_step_tx(ws, x_s, y, x_q, y, None, w, N, need_grad=False, seed=A.SEED)
        assert torch.equal(out["tx"].cpu().reshape(B * N, P), A.draw_rows(A.SEED, B * N, P))
    assert ws.read_status() == 0


def test_dropout_hits_h_only(dev, ws):
    """lamda fixed at 0: the prototypes are the text rows themselves and h is out of the graph, so no mask may touch the loss."""
    for form in A.FORMS:
        a, _ = _step("lamda0", form, dev, ws, dropout=0.5, want_dx=True)
        b, _ = _step("lamda0", form, dev, ws, dropout=0.0, want_dx=True)
        assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["preds"], b["preds"])
        assert torch.equal(a["dx_q"], b["dx_q"]) and torch.equal(a["grads"][0], b["grads"][0])
    # ... and with lamda learned the mask does act
    a, _ = _step("fused", "given", dev, ws, dropout=0.5, need_grad=False)
    b, _ = _step("fused", "given", dev, ws, dropout=0.0, need_grad=False)
    assert not torch.equal(a["lamda_s"], b["lamda_s"])


def test_text_grad_buffer_is_refused_and_not_kept(dev, ws):
    from fumi_amd import hip
    c, ep, w, _, _ = A.reference("small_p", "given")
    g = lambda t: t.to(dev).contiguous()
    canary = torch.full((c["B"], c["N"] * c["K"], c["P"]), SENTINEL, device=dev)
    with pytest.raises(hip.FumiHipError, match="invalid argument"):
        _step("small_p", "given", dev, ws, g_text=canary)
    torch.cuda.synchronize()
    assert bool((canary == SENTINEL).all())
    # nothing was kept: the next plain step runs as if no buffer had been given and writes no text adjoint
    from oracle import casegen as cg
    wf = cg.make_am3_params(c["ep_seed"], c["D"], c["P"], c["Ht"], c["P"])         # a g of h's own hidden width for the plain step
    full = [wf[k].to(dev).contiguous() for k in hip.AM3_KEYS]
    args = (ws, g(ep["x_s"]), g(ep["y_s"]), g(ep["x_q"]), g(ep["y_q"]), g(ep["rows"]), full, c["N"], None)
    a = hip.am3_step(*args)
    torch.cuda.synchronize()
    assert bool((canary == SENTINEL).all())
    b = hip.am3_step(*args)
    assert torch.equal(a["loss"], b["loss"]) and all(torch.equal(x, y) for x, y in zip(a["grads"], b["grads"]))
    assert hip.am3_step_plan()["text_form"] == 0
    assert ws.read_status() == 0


def test_binding_validates_shapes(dev, ws):
    from fumi_amd import hip
    c, ep, w, _, _ = A.reference("small_p", "given")
    g = lambda t: t.to(dev).contiguous()
    wl, _ = _weights(c, w, dev, False)
    base = (g(ep["x_s"]), g(ep["y_s"]), g(ep["x_q"]), g(ep["y_q"]))
    with pytest.raises(hip.FumiHipError, match="text_rows"):
        hip.am3_step_tx(ws, *base, g(ep["rows"])[:, :, :-1].contiguous(), wl, c["N"], need_grad=False)
    with pytest.raises(hip.FumiHipError, match="contiguous"):
        hip.am3_step_tx(ws, *base, g(ep["rows"]).transpose(0, 1).contiguous().transpose(0, 1), wl, c["N"], need_grad=False)
    with pytest.raises(hip.FumiHipError, match="H0"):
        hip.am3_step_tx(ws, *base, None, wl[:6] + [None] + wl[7:], c["N"], need_grad=False)


def _episodes_batch(B, N, K, Q, D, dev):
    from oracle import casegen as cg
    ep = cg.make_episodes(11, B, N, K, Q, D, 8)
    return {k: ([t.to(dev) for t in v[0]], v[1].to(dev)) for k, v in cg.to_batch(ep).items()}


def test_model_trains_rand_at_published_sizes(dev):
    """AM3's own sizes (text_hid_dim 300 < 2 * prototype_dim 512) with dropout on: one training step on the product engine."""
    from fumi_amd import engine
    from fumi_amd.models.am3 import AM3
    assert engine.get_engine().am3_rand_native
    B, N, K, Q, D = 2, 5, 1, 2, 48
    batch = _episodes_batch(B, N, K, Q, D, dev)
    losses = []
    for _ in range(2):
        torch.manual_seed(3)
        model = AM3("precomputed", D, "rand", text_hid_dim=300, prototype_dim=512, dropout=0.25).to(dev)
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        torch.manual_seed(17)
        losses.append(float(model.evaluate(batch, opt, None, N, dev, "train")[0]))
        torch.cuda.synchronize()
        after = model.state_dict()
        assert all(p.grad is None for p in model.g.parameters())
        moved = {k: not torch.equal(before[k], after[k]) for k in before}
        assert not any(v for k, v in moved.items() if k.startswith("g."))
        assert moved["h.0.weight"] and moved["h.3.weight"] and moved["image_encoder.weight"] and moved["image_encoder.bias"]
        assert all(bool(torch.isfinite(v).all()) for v in after.values())
    assert np.isfinite(losses[0]) and losses[0] == losses[1]
    engine.check_status(dev)


def test_cli_accepts_rand_with_default_dropout():
    from fumi_amd import main as cli
    args = cli.parse_args(["--model", "am3", "--text_encoder", "rand"])
    assert args.device.type == "cuda" and args.dropout > 0
    cli.check_supported(args)


def test_fused_case_without_the_fused_mlp_in_subprocess():
    """FUMI_AM3_MLP is `static` in the library: one child pytest process runs the fused case on the per-product GEMMs."""
    env = {k: v for k, v in os.environ.items() if k not in F.KNOBS}
    env["FUMI_AM3_MLP"] = "0"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_am3_rand_gpu.py"), "-q", "-m", "gpu",
                        "-p", "no:cacheprovider", "-k", "test_text_rows_form_matches_oracle and fused"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
