"""The oldest kernels on the data path against float64 restatements at the edges of their launch forms (cases, references and the
restated host geometry: tests/front_forms.py; what these tests rely on is checked without a GPU in tests/test_front_forms_cpu.py).

  embedding bag (csrc/glove_bag.h, glove.hip): the scalar instance (E % 4 != 0, a table or an output one float off a 16-byte boundary),
     three and five chunks (a pair pass plus a single pass), waves with no token, a short last wave, a second 64-token reload of 11
     tokens, a non-zero PAD row, an all-PAD row, token ids outside [0, V), the select form past 64 support rows, the deferred form
     flushed on its own and inside a FuMI step, the 64 KB refusal and the argument checks.  max: bit-equal to float64; mean: every
     element within (lw + 8 + 1) 2^-24 sum|x| / count.
  row gather (csrc/sampler.hip): a second and a third c0 pass with one live column, a grid that wraps, the scalar instance by either
     pointer, one-float rows, no index, a negative index and one equal to n_rows.  Always torch.equal.
  class text select (csrc/episode.hip): first rows at 0, 63, 64 and 129 of 130; a missing class.
  bare linear MAML head (csrc/linhead.hip): S > Qn, T = 0, rows per thread > 1, the smallest D, the largest tape that fits and the
     refusal one step later, at the tolerances of tests/test_hip_parity.py against oracle.fumi_ref.maml_meta_step in float64.

Every comparison prints its error in the unit of its own bound."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import front_forms as FF
from oracle import fumi_ref as R
from reduce_forms_common import two_chains

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _off(a, dev, off=0):
    """numpy array -> contiguous device tensor that starts `off` floats past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
    return v


def _sentinel(shape, dev, off=0):
    n = int(np.prod(shape))
    buf = torch.full((n + 4 + 64,), FF.SENTINEL, device=dev)
    return buf, buf[off:off + n].view(shape)


def _bag(hip, ws, dev, tok, table, mode, out, y_s=None, n_way=0, form="direct", Ls=None):
    """The three entry points with a caller-owned output; returns the status code.  Ls: the token count to CLAIM (argument checks)."""
    L, p = hip.lib(), ctypes.c_void_p
    V, E = table.shape
    m = {"mean": 0, "max": 1}.get(mode, mode)
    Ls = tok.shape[-1] if Ls is None else Ls
    if y_s is None:
        return L.fumi_hip_glove_bag(ws.handle, hip._stream(dev), p(tok.data_ptr()), tok.shape[0], Ls, FF.PAD, p(table.data_ptr()), V, E, m,
                                    p(out.data_ptr()))
    B, S, _ = tok.shape
    if form == "deferred":
        return L.fumi_hip_glove_bag_select_deferred(ws.handle, p(tok.data_ptr()), p(y_s.data_ptr()), B, n_way, S, Ls, FF.PAD,
                                                    p(table.data_ptr()), V, E, m, p(out.data_ptr()))
    return L.fumi_hip_glove_bag_select(ws.handle, hip._stream(dev), p(tok.data_ptr()), p(y_s.data_ptr()), B, n_way, S, Ls, FF.PAD,
                                       p(table.data_ptr()), V, E, m, p(out.data_ptr()))


# ==== embedding bag ===========================================================================================================
@pytest.mark.parametrize("name", list(FF.BAG_CASES))
def test_bag_at_the_edges(name, dev, ws):
    from fumi_amd import hip
    FF.bag_case_reaches_its_edge(name)
    c, g = FF.BAG_CASES[name], FF.bag_case_geometry(name)
    tok, table = FF.bag_inputs(name)
    d_tok, d_table = _off(tok, dev), _off(table, dev, c.get("table_off", 0))
    for mode in ("mean", "max"):
        buf, out = _sentinel((FF.BAG_R, c["E"]), dev, c.get("out_off", 0))
        assert _bag(hip, ws, dev, d_tok, d_table, mode, out) == 0
        assert ws.read_status() == 0
        FF.bag_check(name, mode, out.cpu().numpy(), tok, table, g["lw"])
        rest = torch.cat([buf[:c.get("out_off", 0)], buf[c.get("out_off", 0) + out.numel():]])
        assert bool((rest == FF.SENTINEL).all()), (name, mode, "wrote outside its output")
        if not (c.get("table_off") or c.get("out_off")):          # the wrapper (its own, aligned output) gives the same bits
            again = hip.glove_bag(ws, d_tok, d_table, FF.PAD, mode)
            assert torch.equal(again.view(torch.int32), out.view(torch.int32))            # (bits: an all-PAD row holds a NaN)


@pytest.mark.parametrize("vec", [False, True], ids=["scalar", "vector"])
def test_bag_at_the_largest_row_that_fits_and_refusal_one_past_it(vec, dev, ws):
    """The largest E whose partial sums fit 64 KB runs and is right (31 scalar / 7 vector chunks); the smallest E past it returns
    FUMI_ENOTSUP from all three entry points and leaves a sentinel output and the status word untouched."""
    from fumi_amd import hip
    rng = np.random.default_rng(5 + vec)
    E = FF.largest_accepted_E(vec)
    g = FF.bag_geometry(E, 20)
    assert g["vec"] == vec and g["lds"] <= 64 * 1024 and g["nchunk"] == (7 if vec else 31)
    table, tok = FF.bag_table(rng, 23, E), FF.bag_tokens(rng, 3, 20, 23)
    for mode in ("mean", "max"):
        buf, out = _sentinel((3, E), dev)
        assert _bag(hip, ws, dev, _off(tok, dev), _off(table, dev), mode, out) == 0
        assert ws.read_status() == 0
        FF.bag_check(f"largest E = {E}", mode, out.cpu().numpy(), tok, table, g["lw"])
    E = FF.smallest_refused_E(vec)
    assert FF.bag_geometry(E, 20)["vec"] == vec and FF.bag_geometry(E, 20)["lds"] > 64 * 1024
    table = FF.bag_table(rng, 23, E)
    y, _ = FF.select_labels()
    tok_s = FF.bag_tokens(rng, FF.SEL_B * FF.SEL_S, 4, 23).reshape(FF.SEL_B, FF.SEL_S, 4)
    d_table, d_tok, d_toks, d_y = _off(table, dev), _off(tok, dev), _off(tok_s, dev), _off(y, dev)
    buf, out = _sentinel((FF.SEL_B * FF.SEL_N, E), dev)
    assert _bag(hip, ws, dev, d_tok, d_table, "mean", out) == FF.ENOTSUP
    assert _bag(hip, ws, dev, d_toks, d_table, "mean", out, d_y, FF.SEL_N) == FF.ENOTSUP
    assert _bag(hip, ws, dev, d_toks, d_table, "max", out, d_y, FF.SEL_N, form="deferred") == FF.ENOTSUP
    hip.glove_flush(ws, dev)                                       # nothing is pending after a refused request
    assert ws.read_status() == 0 and bool((buf == FF.SENTINEL).all())


def test_bag_argument_checks(dev, ws):
    from fumi_amd import hip
    tok, table = FF.bag_inputs("scalar_one_chunk")
    d_tok, d_table = _off(tok, dev), _off(table, dev)
    y, _ = FF.select_labels()
    d_toks, d_y = _off(FF.select_bag_inputs(50)[0], dev), _off(y, dev)
    buf, out = _sentinel((FF.SEL_B * FF.SEL_N, 50), dev)
    for mode in (-1, 2):
        assert _bag(hip, ws, dev, d_tok, d_table, mode, out) == FF.EINVAL
        assert _bag(hip, ws, dev, d_toks, d_table, mode, out, d_y, FF.SEL_N) == FF.EINVAL
        assert _bag(hip, ws, dev, d_toks, d_table, mode, out, d_y, FF.SEL_N, form="deferred") == FF.EINVAL
    assert _bag(hip, ws, dev, d_tok, d_table, "mean", out, Ls=0) == FF.EINVAL              # L = 0
    assert _bag(hip, ws, dev, d_toks, d_table, "mean", out, d_y, FF.SEL_N, Ls=0) == FF.EINVAL
    assert _bag(hip, ws, dev, d_toks, d_table, "mean", out, d_y, FF.SEL_N, form="deferred", Ls=0) == FF.EINVAL
    hip.glove_flush(ws, dev)
    assert ws.read_status() == 0 and bool((buf == FF.SENTINEL).all())


def test_bag_token_ids_outside_the_table(dev, ws):
    """One negative id and one equal to V: FUMI_ST_LABEL_RANGE, the id is read as row 0 (and counted as a non-PAD token), every other
    row keeps the bits of the clean call."""
    from fumi_amd import hip
    name = "scalar_three_chunks"
    tok, table = FF.bag_inputs(name)
    lw = FF.bag_case_geometry(name)["lw"]
    bad = tok.copy()
    bad[1, 4], bad[3, 2] = -5, FF.BAG_V
    d_table = _off(table, dev)
    for mode in ("mean", "max"):
        clean = hip.glove_bag(ws, _off(tok, dev), d_table, FF.PAD, mode)
        assert ws.read_status() == 0
        got = hip.glove_bag(ws, _off(bad, dev), d_table, FF.PAD, mode)
        assert ws.read_status() == FF.ST_LABEL_RANGE
        FF.bag_check(name + " with bad ids", mode, got.cpu().numpy(), bad, table, lw)
        assert torch.equal(got[[0, 2, 4]], clean[[0, 2, 4]]) and not torch.equal(got[[1, 3]], clean[[1, 3]])


@pytest.mark.parametrize("E", [50, 300])
def test_bag_select_past_64_support_rows(E, dev, ws):
    """B = 2, N = 5, S = 130 with first rows at 0, 63, 64, 70 / 100 and 129, classes unsorted: glove_bag_select equals glove_bag on the
    hand-selected rows bit for bit (and so inherits its float64 check, repeated here); a missing class gives a NaN row, the status bit
    and leaves the other rows' bits."""
    from fumi_amd import hip
    FF.select_reaches_its_edge()
    tok, table = FF.select_bag_inputs(E)
    y, first = FF.select_labels()
    rows = tok[np.arange(FF.SEL_B)[:, None], first].reshape(FF.SEL_B * FF.SEL_N, -1)
    d_tok, d_table, d_y = _off(tok, dev), _off(table, dev), _off(y, dev)
    y_miss, (mb, mc) = FF.select_missing_labels()
    lw = FF.bag_geometry(E, tok.shape[-1])["lw"]
    for mode in ("mean", "max"):
        got = hip.glove_bag_select(ws, d_tok, d_y, FF.SEL_N, d_table, FF.PAD, mode)
        by_hand = hip.glove_bag(ws, _off(rows, dev), d_table, FF.PAD, mode)
        assert ws.read_status() == 0
        assert torch.equal(got.reshape(-1, E), by_hand), (E, mode)
        FF.bag_check(f"select E = {E}", mode, got.reshape(-1, E).cpu().numpy(), rows, table, lw)
        miss = hip.glove_bag_select(ws, d_tok, _off(y_miss, dev), FF.SEL_N, d_table, FF.PAD, mode)
        assert ws.read_status() == FF.ST_CLASS_MISSING
        assert bool(torch.isnan(miss[mb, mc]).all())
        keep = torch.ones(FF.SEL_B, FF.SEL_N, dtype=torch.bool)
        keep[mb, mc] = False                                     # (the class that took over row 129 still starts at row 0)
        assert torch.equal(miss.cpu()[keep], got.cpu()[keep])


@pytest.mark.parametrize("E", [50, 516])
def test_bag_deferred_then_flushed_equals_the_direct_call(E, dev, ws):
    from fumi_amd import hip
    tok, table = FF.select_bag_inputs(E)
    y, _ = FF.select_labels()
    d_tok, d_table, d_y = _off(tok, dev), _off(table, dev), _off(y, dev)
    for mode in ("mean", "max"):
        direct = hip.glove_bag_select(ws, d_tok, d_y, FF.SEL_N, d_table, FF.PAD, mode)
        buf, out = _sentinel((FF.SEL_B, FF.SEL_N, E), dev)
        assert _bag(hip, ws, dev, d_tok, d_table, mode, out, d_y, FF.SEL_N, form="deferred") == 0
        torch.cuda.synchronize()
        assert bool((buf == FF.SENTINEL).all())                   # nothing was launched
        hip.glove_flush(ws, dev)
        assert ws.read_status() == 0
        assert torch.equal(out, direct), (E, mode)
        hip.glove_flush(ws, dev)                                   # a second flush has nothing to launch
        assert torch.equal(out, direct)


def _run_glove(dev, ride, E, table_off, steps=2):
    """tests/test_folded_step_gpu.py: _run_glove at another vector size, optionally with the embedding table one float off a 16-byte
    boundary (the scalar instance): the bag is either handed to the step (deferred: it rides in the step's first launch, or the step
    launches it) or is a launch of its own."""
    from fumi_amd import engine, hip, optim
    from fumi_amd.models import common
    from fumi_amd.models.fumi import FUMI
    c = dict(B=8, N=5, K=5, Q=8, D=512, hid=[128, 64], E=E, L=24, V=400, Ht=64)
    rs = np.random.RandomState(5)
    words = [f"w{i}" for i in range(c["V"])]
    common.register_word_vectors("glove", common.ArrayKeyedVectors(words, rs.standard_normal((c["V"], c["E"])).astype(np.float32)))
    dictionary = {"PAD": 0, **{w: i for i, w in enumerate(words) if i > 0}}
    torch.manual_seed(4)
    m = FUMI(n_way=c["N"], im_emb_dim=c["D"], im_hid_dim=c["hid"], text_encoder="glove", text_emb_dim=c["E"], text_hid_dim=c["Ht"],
             dropout_rate=0.0, dictionary=dictionary, pooling_strat="mean", norm_hypernet=False).to(dev)
    if table_off:
        w = m.text_encoder.embed.weight
        buf = torch.empty(w.numel() + 4, device=dev)
        w.data = buf[table_off:table_off + w.numel()].view_as(w).copy_(w.data)
        assert w.data_ptr() % 16 == 4 * table_off and w.is_contiguous()
    opt = optim.Adam(m.parameters(), lr=1e-3, weight_decay=5e-4)
    args = SimpleNamespace(device=dev, num_train_adapt_steps=1, num_test_adapt_steps=1, step_size=0.05, first_order=False, num_ways=c["N"],
                           batch_size=c["B"])
    eng = engine.get_engine()
    calls, plans = [], []
    orig = eng.glove_bag_select

    def bag(*a, defer=False, **k):
        calls.append(defer)
        return orig(*a, defer=defer and ride, **k)
    eng.glove_bag_select = bag
    try:
        out = []
        for i in range(steps):
            g = torch.Generator().manual_seed(50 + i)
            S, Qn = c["N"] * c["K"], c["N"] * c["Q"]
            y_s = torch.stack([torch.arange(c["N"]).repeat_interleave(c["K"])[torch.randperm(S, generator=g)] for _ in range(c["B"])])
            y_q = torch.stack([torch.arange(c["N"]).repeat_interleave(c["Q"])[torch.randperm(Qn, generator=g)] for _ in range(c["B"])])
            tok = torch.randint(1, c["V"], (c["B"], c["N"], c["L"]), generator=g)
            tok = tok * (torch.arange(c["L"])[None, None] < torch.randint(3, c["L"] + 1, (c["B"], c["N"], 1), generator=g))
            batch = {"train": ([torch.zeros(c["B"], S, dtype=torch.long), torch.gather(tok, 1, y_s[..., None].expand(-1, -1, c["L"])).to(dev),
                                torch.randn(c["B"], S, c["D"], generator=g).to(dev)], y_s.to(dev)),
                     "test": ([torch.zeros(c["B"], Qn, dtype=torch.long), torch.gather(tok, 1, y_q[..., None].expand(-1, -1, c["L"])).to(dev),
                               torch.randn(c["B"], Qn, c["D"], generator=g).to(dev)], y_q.to(dev))}
            loss, acc, _, _ = m.evaluate(args, batch, opt, "train")
            out.append((float(loss), float(acc)))
            plans.append((hip.xpanel_plan()["fwd_kernel"], hip.hyper_plan()["fwd_form"]))
            te = m.evaluate(args, batch, None, "test")
            out.append((float(te[0]), float(te[1])))
        torch.cuda.synchronize()
    finally:
        eng.glove_bag_select = orig
    return out, [p.detach().clone() for p in m.parameters()], calls, plans


@pytest.mark.parametrize("E,table_off,rides", [(50, 0, False), (52, 1, True)], ids=["E50", "E52_table_off"])
def test_scalar_bag_deferred_into_a_fumi_step_changes_nothing(E, table_off, rides, dev):
    """The pattern of test_embedding_bag_riding_in_the_steps_first_launch_changes_nothing on the scalar instance: losses and parameters
    of the run whose bag is handed to the step equal, bit for bit, those of the run where it is a launch of its own.
    E = 50: the hypernetwork's riding forward needs Dt % 4 == 0 (csrc/hyper.hip: hyper_fwd_split_ok) and the bag rides only beside
    it (csrc/api.hip), so this bag never rides: the step launches the deferred request itself, before anything reads its output.
    E = 52 with the table one float off a 16-byte boundary: the one way the scalar instance CAN ride (xpanel_presplit_glove_kernel<false>);
    that it rode is told by what evaluate asked for, as in the pattern, and by the plan records of the launch that carries it (the
    pre-split forward X-panel kernel, 5, with the hypernetwork forward as its rider, form 5: the two conditions csrc/api.hip rides on)."""
    la, pa, calls, plans = _run_glove(dev, True, E, table_off)
    lb, pb, _, _ = _run_glove(dev, False, E, table_off)
    print(f"E = {E}: evaluate asked for the ride {calls}; (forward X-panel kernel, hypernetwork forward form) per training step {plans}")
    assert calls and all(calls)                                            # evaluate asked for the ride in train AND test mode
    assert all((p == (5, 5)) == rides for p in plans), plans
    assert la == lb
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    assert all(np.isfinite(v) for t in la for v in t) and la[0][0] != la[-2][0]


# ==== row gather ================================================================================================================
def _gather(hip, ws, dev, table, idx, out, n_idx=None):
    p = ctypes.c_void_p
    return hip.lib().fumi_hip_gather_rows(ws.handle, hip._stream(dev), p(table.data_ptr()), table.shape[0], table.shape[1] * 4,
                                          p(idx.data_ptr()), idx.numel() if n_idx is None else n_idx, p(out.data_ptr()))


@pytest.mark.parametrize("name", list(FF.GATHER_CASES))
def test_gather_at_the_edges(name, dev, ws):
    from fumi_amd import hip
    FF.gather_case_reaches_its_edge(name)
    c = FF.GATHER_CASES[name]
    table, idx = FF.gather_inputs(name)
    d_table, d_idx = _off(table, dev, c.get("table_off", 0)), _off(idx, dev)
    off = c.get("out_off", 0)
    buf, out = _sentinel((c["n_idx"], c["row_f"]), dev, off)
    assert _gather(hip, ws, dev, d_table, d_idx, out) == 0
    assert ws.read_status() == 0
    want = torch.from_numpy(table)[torch.from_numpy(idx)]
    wrong = int((out.cpu() != want).any(1).sum())
    print(f"gather {name}: {wrong} of {c['n_idx']} rows differ")
    assert torch.equal(out.cpu(), want)
    assert bool((torch.cat([buf[:off], buf[off + out.numel():]]) == FF.SENTINEL).all()), "wrote outside its output"
    if not (c.get("table_off") or off):
        assert torch.equal(hip.gather_rows(ws, d_table, d_idx).cpu(), want)


def test_gather_no_index_and_bad_indices(dev, ws):
    from fumi_amd import hip
    table, idx = FF.gather_inputs("one_float_rows")
    table = np.ascontiguousarray(np.repeat(table, 8, 1) + np.arange(8, dtype=np.float32) / 16)         # 40 rows of 8 floats
    d_table = _off(table, dev)
    buf, out = _sentinel((len(idx), 8), dev)
    assert _gather(hip, ws, dev, d_table, _off(idx, dev), out, n_idx=0) == 0                        # n_idx = 0: returns, writes nothing
    assert ws.read_status() == 0 and bool((buf == FF.SENTINEL).all())
    bad = idx.copy()
    bad[7], bad[12] = -1, table.shape[0]
    assert _gather(hip, ws, dev, d_table, _off(bad, dev), out) == 0
    assert ws.read_status() == FF.ST_LABEL_RANGE
    want = torch.from_numpy(table)[torch.from_numpy(np.where((bad < 0) | (bad >= table.shape[0]), 0, bad))]
    assert torch.equal(out.cpu(), want) and torch.equal(out[7].cpu(), torch.from_numpy(table[0])) and torch.equal(out[12], out[7])
    assert bool((buf[out.numel():] == FF.SENTINEL).all())


# ==== class text select =========================================================================================================
def test_class_text_select_past_64_support_rows(dev, ws):
    from fumi_amd import hip
    FF.select_reaches_its_edge()
    Dt = 130
    y, first = FF.select_labels()
    text = torch.from_numpy(np.random.default_rng(3).standard_normal((FF.SEL_B, FF.SEL_S, Dt)).astype(np.float32))
    ty = torch.from_numpy(y)
    got = hip.class_text_select(ws, text.to(dev), ty.to(dev), FF.SEL_N)
    assert ws.read_status() == 0
    want = torch.stack([R.class_text_select(text[b], ty[b], FF.SEL_N) for b in range(FF.SEL_B)])
    assert torch.equal(got.cpu(), want)
    assert torch.equal(want, text[torch.arange(FF.SEL_B)[:, None], torch.from_numpy(first)])
    y_miss, (mb, mc) = FF.select_missing_labels()
    with pytest.raises(IndexError):
        R.class_text_select(text[mb], torch.from_numpy(y_miss)[mb], FF.SEL_N)
    miss = hip.class_text_select(ws, text.to(dev), torch.from_numpy(y_miss).to(dev), FF.SEL_N).cpu()
    assert ws.read_status() == FF.ST_CLASS_MISSING
    assert bool(torch.isnan(miss[mb, mc]).all())
    keep = torch.ones(FF.SEL_B, FF.SEL_N, dtype=torch.bool)
    keep[mb, mc] = False
    assert torch.equal(miss[keep], want[keep])


# ==== bare linear MAML head =====================================================================================================
def _lin_dev(c, dev):
    ep, p = FF.lin_inputs(c)
    return ([ep[k].to(dev).contiguous() for k in ("x_s", "y_s", "x_q", "y_q")], [t.to(dev).contiguous() for t in p])


def _cpu(out):
    return {k: ([t.cpu() for t in v] if isinstance(v, list) else v.cpu()) for k, v in out.items() if v is not None}


@pytest.mark.parametrize("name", list(FF.LIN_CASES))
def test_linhead_at_the_edges(name, dev, ws):
    from fumi_amd import hip
    FF.linhead_case_reaches_its_edge(name)
    c = FF.LIN_CASES[name]
    ep, p = _lin_dev(c, dev)
    out = _cpu(hip.maml_step(ws, *ep, p, c["T"], FF.ALPHA, c["fo"]))
    assert ws.read_status() == 0
    FF.lin_check(name, out)


def test_linhead_orders_give_the_same_bits_without_an_inner_step(dev, ws):
    from fumi_amd import hip
    c = FF.LIN_CASES["no_inner_step_second_order"]
    ep, p = _lin_dev(c, dev)
    a = _cpu(hip.maml_step(ws, *ep, p, 0, FF.ALPHA, False))
    b = _cpu(hip.maml_step(ws, *ep, p, 0, FF.ALPHA, True))
    assert ws.read_status() == 0
    for k in ("logits", "preds", "loss_b", "acc_b"):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(x, y) for x, y in zip(a["g_params"], b["g_params"]))
    ref = FF.lin_reference("no_inner_step_second_order")
    assert FF.rel_to_max(a["logits"], ep[2].cpu().double() @ p[0].cpu().double().t() + p[1].cpu().double()) <= FF.LOGIT_TOL
    assert FF.rel_to_max(a["logits"], ref["logits"]) <= FF.LOGIT_TOL


def test_linhead_forward_only_repeat_and_stats(dev, ws):
    """On the S > Qn case: need_grad = False gives the training call's bits and touches no gradient buffer; a second training call
    gives equal bits; stats are the fixed-order sums of loss_b and acc_b (tests/reduce_forms_common.py: two_chains, bit for bit)."""
    from fumi_amd import hip
    name = "S_above_Qn_second_order"
    c = FF.LIN_CASES[name]
    ep, p = _lin_dev(c, dev)
    stats = torch.full((2,), FF.SENTINEL, device=dev)
    a = _cpu(hip.maml_step(ws, *ep, p, c["T"], FF.ALPHA, False, stats=stats))
    FF.lin_check(name, a)
    for k, col in (("loss_b", 0), ("acc_b", 1)):
        want = two_chains(a[k].numpy()[:, None], 1.0 / c["B"])
        diff = abs(float(stats[col]) - float(want[0]))
        print(f"linhead stats[{col}]: |difference| to the two-chain sum {diff:.3e}")
        assert np.array_equal(stats[col:col + 1].cpu().numpy().view(np.int32), want.view(np.int32)), (k, float(stats[col]), float(want[0]))
    b = _cpu(hip.maml_step(ws, *ep, p, c["T"], FF.ALPHA, False))
    for k in ("logits", "preds", "preds_f", "loss_b", "acc_b"):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(x, y) for x, y in zip(a["g_params"], b["g_params"]))
    g = [torch.full_like(t, FF.SENTINEL) for t in p]
    f = _cpu(hip.maml_step(ws, *ep, p, c["T"], FF.ALPHA, False, need_grad=False, g_params=g))
    assert ws.read_status() == 0
    for k in ("logits", "preds", "preds_f", "loss_b", "acc_b"):
        assert torch.equal(a[k], f[k]), k
    assert all(bool((t == FF.SENTINEL).all()) for t in g)
    FF.lin_check(name, f, need_grad=False)


def test_linhead_labels_outside_the_classes(dev, ws):
    from fumi_amd import hip
    c = FF.LIN_CASES["S_above_Qn_second_order"]
    for which, value in ((1, c["N"]), (3, -1)):                    # a support label equal to N; a negative query label
        ep, p = _lin_dev(c, dev)
        ep[which][1, 2] = value
        out = _cpu(hip.maml_step(ws, *ep, p, c["T"], FF.ALPHA, False))
        assert ws.read_status() == FF.ST_LABEL_RANGE
        assert all(bool(torch.isfinite(t).all()) for t in [out["logits"], out["loss_b"]] + out["g_params"])
        with pytest.raises(IndexError):
            hip.raise_on_status(FF.ST_LABEL_RANGE)


def test_linhead_refuses_a_tape_that_does_not_fit(dev, ws):
    """B = 1, N = 20, K = 5, Q = 1: T = 14 tapes 36076 floats and runs (case largest_tape_that_fits); T = 15 tapes 38076 > 38000 and is
    refused with FUMI_ENOTSUP before anything writes an output; the first-order form of T = 15 keeps no tape and runs."""
    from fumi_amd import hip
    c = FF.LIN_REFUSED
    S, Qn = c["N"] * c["K"], c["N"] * c["Q"]
    assert FF.linhead_lds_floats(c["N"], S, Qn, c["T"], True) > FF.LINHEAD_LIMIT >= FF.linhead_lds_floats(c["N"], S, Qn, c["T"], False)
    ep, p = _lin_dev(c, dev)
    f32, i64 = hip._f32, hip._i64
    sent = lambda *shape: torch.full(shape, FF.SENTINEL, device=dev)
    logits, preds_f, loss_b, acc_b, stats = sent(c["B"], Qn, c["N"]), sent(c["B"], Qn), sent(c["B"]), sent(c["B"]), sent(2)
    preds = torch.full((c["B"], Qn), -77, dtype=torch.int64, device=dev)
    g = [torch.full_like(t, FF.SENTINEL) for t in p]
    hid = (ctypes.c_int * 1)()

    def call(first_order):
        return hip.lib().fumi_hip_maml_step(
            ws.handle, hip._stream(dev), c["B"], c["N"], S, Qn, c["D"], 0, hid, c["T"], FF.ALPHA, int(first_order), 1, 1.0 / c["B"],
            f32(ep[0], "x_s"), i64(ep[1], "y_s"), f32(ep[2], "x_q"), i64(ep[3], "y_q"), hip._parr(p, "params"),
            f32(logits, "logits"), i64(preds, "preds"), f32(preds_f, "preds_f"), f32(loss_b, "loss_b"), f32(acc_b, "acc_b"),
            f32(stats, "stats"), hip._parr(g, "g_params"))
    assert call(False) == FF.ENOTSUP
    assert ws.read_status() == 0
    assert all(bool((t == FF.SENTINEL).all()) for t in [logits, preds_f, loss_b, acc_b, stats] + g) and bool((preds == -77).all())
    with pytest.raises(hip.FumiHipError):
        hip.maml_step(ws, *ep, p, c["T"], FF.ALPHA, False)
    assert call(True) == 0
    assert ws.read_status() == 0
    ep64, p64 = FF.lin_inputs(c)
    pl = [t.double().requires_grad_(True) for t in p64]
    ref = R.maml_meta_step(pl, ep64["x_s"].double(), ep64["y_s"], ep64["x_q"].double(), ep64["y_q"], c["T"], FF.ALPHA, True)
    e_log = FF.rel_to_max(logits.cpu(), ref["logits"])
    floor = max(0.05 * max(float(r.abs().max()) for r in ref["g_params"]), 1e-5)
    e_g = max(FF.rel_to_max(a.cpu(), r, floor) for a, r in zip(g, ref["g_params"]))
    print(f"linhead first order at the refused shape: logits {e_log / FF.LOGIT_TOL:.4f}, gradients {e_g / FF.GRAD_TOL:.4f} (units of the bound)")
    assert e_log <= FF.LOGIT_TOL and e_g <= FF.GRAD_TOL and torch.equal(preds.cpu(), ref["preds"])
