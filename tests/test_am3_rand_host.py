"""CPU suite: AM3's text_encoder='rand' as a native form of the step -- the draw restated on the host, the cases the GPU file runs
(the oracle alone keeps the safe-row share), the model's dispatch onto ``am3_step_tx`` and the capability gating of the CLI check,
with a stub engine standing in for the GPU."""
import ctypes
import re

import numpy as np
import pytest
import torch

import am3_forms as F
import am3_rand as A
from oracle import casegen as cg
from oracle_engine import OracleEngine


def test_draw_restatement_is_a_uniform_grid():
    n = 1 << 20
    a = A.draw_rows(A.SEED, 1 << 10, 1 << 10).numpy().ravel()
    assert a.dtype == np.float32 and a.size == n
    assert np.array_equal(a, A.draw_rows(A.SEED, 1 << 10, 1 << 10).numpy().ravel())               # deterministic
    assert np.array_equal(a[:4096], A.draw_rows(A.SEED, 64, 64).numpy().ravel())                # a function of the flat index alone
    assert not np.array_equal(a[:4096], A.draw_rows(A.SEED_B, 64, 64).numpy().ravel())
    assert float(a.min()) >= -1.0 and float(a.max()) < 1.0
    k = a.astype(np.float64) * 2.0 ** 23
    assert np.array_equal(k, np.round(k))                                                         # multiples of 2^-23
    assert abs(float(a.astype(np.float64).mean())) < 0.01                                         # sanity bound at a fixed seed


@pytest.mark.parametrize("form", A.FORMS)
@pytest.mark.parametrize("name", list(A.CASES))
def test_oracle_alone_keeps_the_safe_share(name, form):
    """The episode seeds of the table are chosen so that the float64 oracle itself leaves >= SAFE_SHARE of the query rows with a
    margin between the two nearest prototypes; the identity that stands in for g is exact (checked inside ``reference``)."""
    c, ep, w, ref, (safe, pred, empty, first_empty) = A.reference(name, form)
    assert float(safe.float().mean()) >= F.SAFE_SHARE
    assert bool(torch.isfinite(ref["loss"]))
    if c["lamda_fixed"] is not None:
        assert bool((ref["lamda_s"] == float(c["lamda_fixed"])).all())
    # the one gradient that is zero by cancellation (not by a zero factor): bi under lamda = 1 (checked inside ``cancelling_sums``)
    assert set(A.cancelling_sums(name, form)) == ({"bi"} if name == "lamda1" else set())


class _StubEngine(OracleEngine):
    """The oracle engine plus the capability: am3_step_tx records what the model hands over and computes the step through
    ``am3_step`` with the identity in g's place (dropout 0 only: the oracle engine draws g's and h's masks at one width)."""
    am3_rand_native = True

    def __init__(self):
        self.calls = []

    def am3_step_tx(self, x_s, y_s, x_q, y_q, text_rows, w, n_way, lamda_fixed, need_grad, grad_scale, g_w=None, dropout_p=0.0,
                    seed=0, stats=None, want_dx=False):
        self.calls.append(dict(text_rows=text_rows, w=list(w), g_w=None if g_w is None else list(g_w), dropout_p=dropout_p, seed=seed))
        assert dropout_p == 0.0
        B, S = y_s.shape
        P = w[0].shape[0]
        rows = A.draw_rows(seed, B * S, P).reshape(B, S, P) if text_rows is None else text_rows
        w_full = list(w[:2]) + list(A.identity_g(P)) + list(w[6:])
        g_full = None
        if need_grad:
            g_full = list(g_w[:2]) + [torch.empty_like(t) for t in w_full[2:6]] + list(g_w[6:])
        out = self.am3_step(x_s, y_s, x_q, y_q, rows, w_full, n_way, lamda_fixed, need_grad, grad_scale, g_w=g_full, want_dx=want_dx)
        return dict(out, tx=rows)


@pytest.fixture()
def stub_engine():
    from fumi_amd import engine
    stub = _StubEngine()
    old = engine.set_engine(stub)
    yield stub
    engine.set_engine(old)


def test_model_dispatches_rand_onto_the_native_form(stub_engine, monkeypatch):
    from fumi_amd.models.am3 import AM3
    c = cg.AM3_CASES["am3_lam"]
    P, Ht = 8, 12                                         # Ht < 2P: the identity route would refuse this
    ep = cg.make_episodes(4, c["B"], c["N"], c["K"], c["Q"], c["D"], c["Dt"])
    model = AM3("precomputed", c["D"], "rand", text_emb_dim=c["Dt"], text_hid_dim=Ht, prototype_dim=P, dropout=0.0)

    def no_identity(*a, **k):
        raise AssertionError("_rand_g / _encode_text must not be called on the native form")
    monkeypatch.setattr(model, "_rand_g", no_identity)
    monkeypatch.setattr(model, "_encode_text", no_identity)
    g_before = [p.detach().clone() for p in model.g.parameters()]
    h_before = [p.detach().clone() for p in model.h.parameters()]
    i_before = [p.detach().clone() for p in model.image_encoder.parameters()]
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    losses = []
    for _ in range(2):
        torch.manual_seed(5)
        losses.append(float(model.evaluate(cg.to_batch(ep), opt, None, c["N"], torch.device("cpu"), "train")[0]))
    first, second = stub_engine.calls
    assert first["text_rows"] is None
    assert first["w"][2:6] == [None] * 4 and first["g_w"][2:6] == [None] * 4
    assert all(t is not None for t in first["w"][:2] + first["w"][6:] + first["g_w"][:2] + first["g_w"][6:])
    assert first["dropout_p"] == 0.0
    torch.manual_seed(5)
    assert first["seed"] == int(torch.randint(0, 2 ** 62, (1,)).item())        # a seed even at dropout 0: the draw consumes it
    assert second["seed"] == first["seed"]                                      # torch.manual_seed fixes the run
    assert np.isfinite(losses[0])
    assert all(p.grad is None for p in model.g.parameters())
    assert all(torch.equal(a, b.detach()) for a, b in zip(g_before, model.g.parameters()))
    assert any(not torch.equal(a, b.detach()) for a, b in zip(h_before, model.h.parameters()))
    assert any(not torch.equal(a, b.detach()) for a, b in zip(i_before, model.image_encoder.parameters()))
    # evaluation draws too: a seed is passed with dropout off
    model.evaluate(cg.to_batch(ep), None, None, c["N"], torch.device("cpu"), "val")
    assert stub_engine.calls[2]["text_rows"] is None and stub_engine.calls[2]["dropout_p"] == 0.0


def test_check_supported_is_gated_by_the_capability(stub_engine, monkeypatch):
    from fumi_amd import main as cli
    rand = ["--model", "am3", "--disable_cuda", "--text_encoder", "rand"]
    cli.check_supported(cli.parse_args(rand))                                   # CLI default dropout 0.25
    cli.check_supported(cli.parse_args(rand + ["--dropout", "0.5"]))
    monkeypatch.setattr(_StubEngine, "am3_rand_native", False)
    with pytest.raises(NotImplementedError, match="--dropout 0"):
        cli.check_supported(cli.parse_args(rand))
    cli.check_supported(cli.parse_args(rand + ["--dropout", "0"]))


def test_header_library_and_binding_name_the_two_exports():
    import os
    from conftest import ROOT
    from fumi_amd import hip
    names = ["fumi_hip_am3_step_tx", "fumi_hip_am3_step_tx_dx"]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fumi_hip.h")).read(), flags=re.S)
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = ctypes.CDLL(hip.LIB_PATH)
    for n in names:
        assert re.search(r"\b" + n + r"\s*\(", src) and n in hip.SYMBOLS and hasattr(L, n)
    assert hip.AM3_PLAN_KEYS[11] == "text_form" and len(hip.AM3_PLAN_KEYS) == 12
    plan = (ctypes.c_int * 12)(*([-7] * 12))
    assert L.fumi_hip_am3_step_plan(plan, 11) == 0 and plan[11] == -7            # a caller that asks for 11 sees no difference
