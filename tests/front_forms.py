"""Case tables, seeded inputs and float64 restatements for the oldest kernels on the data path -- the embedding bag
(csrc/glove_bag.h, glove.hip), the row gather (csrc/sampler.hip: gather_rows_kernel), the class text select (csrc/episode.hip) and the
bare linear MAML head (csrc/linhead.hip) -- used by tests/test_front_forms_cpu.py and tests/test_front_forms_gpu.py.
TEST INFRASTRUCTURE ONLY.

The host geometry of each launch is restated here in plain Python (bag_geometry: bag_geometry / glove_bag_row of csrc/glove.hip and
csrc/glove_bag.h; gather_geometry: fumi_hip_gather_rows; linhead_lds_floats: csrc/linhead.hip) ONLY so that a case can assert that it
still reaches the branch it is named for: when someone changes 8 waves, 64 lanes, 512 columns a pass, 4096 workgroups or 38000 floats
in the engine, or a shape in a table below, the case fails instead of going quiet.
"""
import functools
import zlib
from collections import OrderedDict

import numpy as np
import torch

from oracle import casegen as cg
from oracle import fumi_ref as R

ST_LABEL_RANGE, ST_CLASS_MISSING = 1, 2                  # include/fumi_hip.h: FUMI_ST_*
EINVAL, ENOTSUP = -1, -4                                 # include/fumi_hip.h: FUMI_E*
SENTINEL = -7.5e7
U = 2.0 ** -24                                           # unit round-off of float32


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ==== embedding bag ===========================================================================================================
GW, GU = 8, 16                                           # csrc/glove_bag.h: waves per output row, row gathers in flight per wave
PAD = 2                                                  # (not 0: a token outside [0, V) is read as row 0, which must not be the PAD row)


def bag_geometry(E, L, aligned=True):
    """What csrc/glove.hip bag_geometry and glove_bag_row derive from (E, L, the alignment of the table and output pointers)."""
    vec = E % 4 == 0 and aligned
    W = 4 if vec else 1
    nchunk = (E // W + 63) // 64
    Ep = nchunk * 64 * W
    lw = (L + GW - 1) // GW
    ntok = [max(0, min(L, w * lw + lw) - w * lw) for w in range(GW)]           # tokens of each wave
    return dict(vec=vec, W=W, nchunk=nchunk, Ep=Ep, lds=(GW * Ep + GW) * 4, lw=lw, ntok=ntok,
                reloads=[(n + 63) // 64 for n in ntok],                        # 64-token reloads of each wave
                last_nl=[n - 64 * ((n - 1) // 64) if n else 0 for n in ntok],  # tokens of each wave's last reload
                pair_passes=nchunk // 2, single_pass=nchunk % 2)


def smallest_refused_E(vec):
    """Smallest E of the scalar (E % 4 != 0) / vector (E % 4 == 0) instance whose partial sums pass 64 KB of LDS."""
    E = 4 if vec else 1
    while bag_geometry(E, 1)["lds"] <= 64 * 1024:
        E += 4 if vec else (2 if E % 4 == 3 else 1)
    return E


def largest_accepted_E(vec):
    E = smallest_refused_E(vec)
    E -= 4 if vec else 1
    while not vec and E % 4 == 0:
        E -= 1
    assert bag_geometry(E, 1)["lds"] <= 64 * 1024 and bag_geometry(E, 1)["vec"] == vec
    return E


# table_off / out_off: the table / the output starts one float into its buffer.  `want`: what bag_geometry must give.
BAG_CASES = OrderedDict([
    ("scalar_one_chunk", dict(E=50, L=20, want=dict(vec=False, nchunk=1, lw=3))),
    ("scalar_three_chunks", dict(E=130, L=20, want=dict(vec=False, nchunk=3, pair_passes=1, single_pass=1))),
    ("scalar_by_table_pointer", dict(E=300, L=20, table_off=1, want=dict(vec=False, nchunk=5, pair_passes=2, single_pass=1))),
    ("scalar_by_output_pointer", dict(E=300, L=20, out_off=1, want=dict(vec=False, nchunk=5))),
    ("vector_three_chunks", dict(E=516, L=20, want=dict(vec=True, nchunk=3, pair_passes=1, single_pass=1))),
    ("empty_waves", dict(E=12, L=3, want=dict(vec=True, nchunk=1, lw=1, ntok=[1, 1, 1, 0, 0, 0, 0, 0]))),
    ("short_last_wave", dict(E=12, L=13, want=dict(vec=True, lw=2, ntok=[2, 2, 2, 2, 2, 2, 1, 0]))),
    ("second_reload", dict(E=300, L=600, want=dict(vec=True, nchunk=2, lw=75, reloads=[2] * 8, last_nl=[11] * 8))),
    ("all_pad_row", dict(E=64, L=128, all_pad=1, want=dict(vec=True, nchunk=1, lw=16))),
])
BAG_R, BAG_V = 5, 97
VALID_FRACTION = (0.4, 0.55, 0.7, 0.85, 1.0)             # non-PAD share of each row: the pad counts differ
# ... but at most this many PAD tokens a row.  Adding ONE row hundreds of times rounds the same way every time, so the error of a plain
# index-order float32 sum then grows with L itself, while the kernel's bound counts the lw = L / 8 additions of a wave: the cap keeps
# the index-order sum of tests/test_front_forms_cpu.py within half of that bound at L = 600 (a condition on the inputs; the bound on
# the kernel is a worst case and needs no such condition).
PAD_CAP = (48, 40, 24, 8, 0)


def bag_case_geometry(name):
    c = BAG_CASES[name]
    return bag_geometry(c["E"], c["L"], aligned=not (c.get("table_off") or c.get("out_off")))


def bag_case_reaches_its_edge(name):
    c, g = BAG_CASES[name], bag_case_geometry(name)
    for k, v in c["want"].items():
        assert g[k] == v, (name, k, g[k], v)
    assert g["lds"] <= 64 * 1024 and BAG_R <= 6 and BAG_V <= 600
    if name == "scalar_by_table_pointer" or name == "scalar_by_output_pointer":
        assert c["E"] % 4 == 0 and bag_geometry(c["E"], c["L"])["vec"]           # scalar ONLY because of the pointer
    if name == "empty_waves":
        assert sum(1 for n in g["ntok"] if n == 0) == 5
    if name == "short_last_wave":
        assert any(0 < n < g["lw"] for n in g["ntok"])
    if name == "second_reload":
        assert g["last_nl"][0] % GU != 0 and g["last_nl"][0] < 64
    tok, table = bag_inputs(name)
    npad = (tok == PAD).sum(1)
    assert len(set(npad.tolist())) >= 3 and (table[PAD] != 0).sum() == c["E"] - 1
    assert ((npad == c["L"]).sum() == 1) == bool(c.get("all_pad"))


def bag_table(rng, V, E):
    """fp32 [V, E] standard normal; the PAD row has entries of magnitude 0.5 .. 1.5 (so that a kernel that skipped PAD tokens shows)
    except entry 1, which is 0 (so that an all-PAD row holds a NaN beside its infinities)."""
    table = rng.standard_normal((V, E)).astype(np.float32)
    table[PAD] = (rng.uniform(0.5, 1.5, E) * rng.choice([-1.0, 1.0], E)).astype(np.float32)
    table[PAD, 1] = 0.0
    return table


def bag_tokens(rng, R, L, V, all_pad_row=None):
    """int64 [R, L]: row r has max(1, round(VALID_FRACTION[r] L), L - PAD_CAP[r]) non-PAD tokens at random positions (PAD tokens lie
    between them, so the waves meet some), the rest PAD; all_pad_row: that row is PAD only."""
    tok = np.full((R, L), PAD, dtype=np.int64)
    for r in range(R):
        k = r % len(VALID_FRACTION)
        n = 0 if r == all_pad_row else max(1, int(round(VALID_FRACTION[k] * L)), L - PAD_CAP[k])
        ids = rng.integers(0, V - 1, n)
        ids[ids >= PAD] += 1                                                     # any row but PAD
        tok[r, np.sort(rng.permutation(L)[:n])] = ids
    return tok


@functools.lru_cache(maxsize=None)
def bag_inputs(name):
    c, rng = BAG_CASES[name], _rng("bag " + name)
    table = bag_table(rng, BAG_V, c["E"])
    return bag_tokens(rng, BAG_R, c["L"], BAG_V, c.get("all_pad")), table


def bag_reference(tok, table, mode, lw, skip_pad=False):
    """float64 WordEmbedding.forward (fumi/models/common.py:23-41) on the fp32 table, with the kernel's documented reading of a token
    outside [0, V) (row 0, counted as a non-PAD token).  Returns (out [R, E] float64, bound [R, E] or None): the mean's bound is
    (lw + 8 + 1) 2^-24 sum_l |table[tok_l, j]| / count -- at most lw sequential additions per wave, 8 wave partials, one division.
    An all-PAD row divides by zero as the reference does.  skip_pad: the WRONG mean that leaves PAD tokens out of the sum."""
    V = table.shape[0]
    emb = table.astype(np.float64)[np.where((tok < 0) | (tok >= V), 0, tok)]      # [R, L, E]
    if mode == "max":
        return emb.max(1), None
    cnt = (tok != PAD).sum(1).astype(np.float64)[:, None]
    if skip_pad:
        emb = emb * (tok != PAD)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return emb.sum(1) / cnt, (lw + GW + 1) * U * np.abs(emb).sum(1) / cnt


def bag_fp32_in_index_order(tok, table):
    """The mean as a plain float32 accumulation over l = 0 .. L-1, then one division."""
    acc = np.zeros((tok.shape[0], table.shape[1]), np.float32)
    for l in range(tok.shape[1]):
        acc = acc + table[tok[:, l]]
    with np.errstate(divide="ignore", invalid="ignore"):
        return acc / (tok != PAD).sum(1).astype(np.float32)[:, None]


def bag_check(name, mode, got, tok, table, lw):
    """got [R, E] float32 numpy against the float64 reference: max mode bit for bit; mean mode every element of every row with a
    non-PAD token within its bound, an all-PAD row equal as NaN / +-inf.  Prints and returns the largest error / bound."""
    ref, bound = bag_reference(tok, table, mode, lw)
    if mode == "max":
        assert np.array_equal(got, ref.astype(np.float32)), (name, "max differs", int((got != ref.astype(np.float32)).sum()))
        print(f"bag {name} max: bit-equal")
        return 0.0
    live = (tok != PAD).sum(1) > 0
    for r in np.nonzero(~live)[0]:
        want = ref[r].astype(np.float32)
        assert np.isnan(want).any() and np.isinf(want).any()
        assert np.array_equal(np.isnan(got[r]), np.isnan(want)) and np.array_equal(got[r][~np.isnan(want)], want[~np.isnan(want)]), (name, r)
    err, b = np.abs(got[live].astype(np.float64) - ref[live]), bound[live]
    assert (b > 0).all()
    ratio = float((err / b).max())
    print(f"bag {name} mean: largest error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)
    return ratio


# ---- select form ---------------------------------------------------------------------------------------------------------------
SEL_B, SEL_N, SEL_S = 2, 5, 130
# per episode: (class, index of its FIRST support row), unsorted classes; the rows between first occurrences repeat earlier classes
SEL_FIRST = (((3, 0), (0, 63), (4, 64), (2, 70), (1, 129)),
             ((1, 0), (4, 63), (0, 64), (3, 100), (2, 129)))


@functools.lru_cache(maxsize=None)
def select_labels():
    """int64 [B, S] and the first row of every class [B, N]."""
    rng = _rng("select labels")
    y = np.zeros((SEL_B, SEL_S), dtype=np.int64)
    first = np.zeros((SEL_B, SEL_N), dtype=np.int64)
    for b, plan in enumerate(SEL_FIRST):
        seen = []
        for s in range(SEL_S):
            new = [c for c, f in plan if f == s]
            if new:
                seen.append(new[0]); y[b, s] = new[0]; first[b, new[0]] = s
            else:
                y[b, s] = seen[rng.integers(0, len(seen))]
    return y, first


def select_reaches_its_edge():
    y, first = select_labels()
    for b in range(SEL_B):
        assert sorted(first[b].tolist()) == sorted(f for _, f in SEL_FIRST[b]) and {0, 63, 64, 129} <= set(first[b].tolist())
        for c in range(SEL_N):
            assert int(np.nonzero(y[b] == c)[0][0]) == first[b, c]
        order = [c for c, _ in SEL_FIRST[b]]
        assert order != sorted(order)
    assert SEL_S > 128 and (first >= 64).any() and (first < 64).any()             # both ballot passes, and a third that must not run


def select_missing_labels():
    """Class SEL_FIRST[0][-1] of episode 0 loses its only row (index 129)."""
    y, _ = select_labels()
    y = y.copy()
    c, f = SEL_FIRST[0][-1]
    assert (y[0] == c).sum() == 1
    y[0, f] = SEL_FIRST[0][0][0]
    return y, (0, c)


@functools.lru_cache(maxsize=None)
def select_bag_inputs(E, L=20):
    rng = _rng(f"select bag {E}")
    table = bag_table(rng, BAG_V, E)
    tok = bag_tokens(rng, SEL_B * SEL_S, L, BAG_V).reshape(SEL_B, SEL_S, L)
    return tok, table


# ==== row gather ================================================================================================================
def gather_geometry(row_f, n_idx, aligned=True):
    """fumi_hip_gather_rows / gather_rows_kernel: instance, float4 columns, passes of the 512-column c0 loop, live columns of the last
    pass, workgroups (4 rows each) and whether the grid-stride loop wraps."""
    vec = row_f % 4 == 0 and aligned
    n4 = row_f >> 2
    passes = (n4 + 511) // 512 if vec else 0
    blocks = min(4096, (n_idx + 3) // 4)
    return dict(vec=vec, n4=n4, passes=passes, last_live=n4 - 512 * (passes - 1) if vec else 0, blocks=blocks, wraps=n_idx > 4 * blocks)


GATHER_CASES = OrderedDict([
    ("second_pass_one_column", dict(row_f=2052, n_rows=7, n_idx=9, want=dict(vec=True, n4=513, passes=2, last_live=1, wraps=False))),
    ("third_pass_one_column", dict(row_f=4100, n_rows=5, n_idx=6, want=dict(vec=True, n4=1025, passes=3, last_live=1))),
    ("grid_wraps", dict(row_f=8, n_rows=40, n_idx=16389, want=dict(vec=True, blocks=4096, wraps=True, passes=1))),
    ("scalar_by_table_pointer", dict(row_f=8, n_rows=40, n_idx=21, table_off=1, want=dict(vec=False, blocks=6))),
    ("scalar_by_output_pointer", dict(row_f=8, n_rows=40, n_idx=21, out_off=1, want=dict(vec=False))),
    ("one_float_rows", dict(row_f=1, n_rows=40, n_idx=21, want=dict(vec=False, n4=0))),
])


def gather_case_reaches_its_edge(name):
    c = GATHER_CASES[name]
    g = gather_geometry(c["row_f"], c["n_idx"], aligned=not (c.get("table_off") or c.get("out_off")))
    for k, v in c["want"].items():
        assert g[k] == v, (name, k, g[k], v)
    if c.get("table_off") or c.get("out_off"):
        assert gather_geometry(c["row_f"], c["n_idx"])["vec"]
    assert c["n_rows"] * c["row_f"] * 4 < 1 << 20
    return g


@functools.lru_cache(maxsize=None)
def gather_inputs(name):
    """(table [n_rows, row_f] float32 with no two equal elements, idx [n_idx] int64 that names every row)."""
    c, rng = GATHER_CASES[name], _rng("gather " + name)
    table = (np.arange(c["n_rows"] * c["row_f"], dtype=np.float32) + 1.0).reshape(c["n_rows"], c["row_f"])
    idx = rng.integers(0, c["n_rows"], c["n_idx"]).astype(np.int64)
    idx[rng.permutation(c["n_idx"])[:min(c["n_rows"], c["n_idx"])]] = rng.permutation(c["n_rows"])[:min(c["n_rows"], c["n_idx"])]
    return table, idx


# ==== bare linear MAML head =====================================================================================================
LOGIT_TOL, GRAD_TOL, MARGIN = 1e-4, 1e-4, 1e-5           # tests/test_hip_parity.py:18-20
ALPHA = 0.05


def linhead_lds_floats(N, S, Qn, T, taped):
    """csrc/linhead.hip linhead_lds_floats: E, Ebar, Z [S, N]; three [N] vectors; 16 partials; lbar [max(Qn, S), N]; the tape."""
    return 3 * S * N + 3 * N + 16 + max(Qn, S) * N + (T * S * N if taped else 0)


LINHEAD_LIMIT = 38000
# fo: first order.  `want`: relations the case is named for (checked in linhead_case_reaches_its_edge).
LIN_CASES = OrderedDict([
    ("S_above_Qn_second_order", dict(B=3, N=4, K=5, Q=1, T=3, D=33, fo=False, seed=11)),
    ("S_above_Qn_first_order", dict(B=3, N=4, K=5, Q=1, T=3, D=33, fo=True, seed=11)),
    ("no_inner_step_second_order", dict(B=2, N=3, K=2, Q=4, T=0, D=64, fo=False, seed=12)),
    ("no_inner_step_first_order", dict(B=2, N=3, K=2, Q=4, T=0, D=64, fo=True, seed=12)),
    ("two_query_rows_a_thread", dict(B=1, N=2, K=1, Q=150, T=1, D=33, fo=False, seed=13)),
    ("two_support_rows_a_thread", dict(B=2, N=5, K=60, Q=2, T=2, D=64, fo=False, seed=14)),
    ("smallest_D", dict(B=2, N=3, K=2, Q=3, T=2, D=8, fo=False, seed=15)),
    ("largest_tape_that_fits", dict(B=1, N=20, K=5, Q=1, T=14, D=33, fo=False, seed=16)),
])
# the taped form of this shape is refused; its first-order form fits (one inner step more than "largest_tape_that_fits")
LIN_REFUSED = dict(B=1, N=20, K=5, Q=1, T=15, D=33, seed=16)


def linhead_case_reaches_its_edge(name):
    c = LIN_CASES[name]
    S, Qn = c["N"] * c["K"], c["N"] * c["Q"]
    fl = linhead_lds_floats(c["N"], S, Qn, c["T"], not c["fo"])
    assert fl <= LINHEAD_LIMIT, (name, fl)
    if name.startswith("S_above_Qn"):
        assert S > Qn and c["T"] >= 1
        by_qn_alone = 3 * S * c["N"] + 3 * c["N"] + 16 + Qn * c["N"] + c["T"] * S * c["N"]       # zbar_t [S, N] would run into the tape
        assert linhead_lds_floats(c["N"], S, Qn, c["T"], True) - by_qn_alone == (S - Qn) * c["N"] > 0
    if name.startswith("no_inner_step"):
        assert c["T"] == 0
    if name == "two_query_rows_a_thread":
        assert Qn > 256 >= S
    if name == "two_support_rows_a_thread":
        assert S > 256 and S > Qn
    if name == "largest_tape_that_fits":
        r = LIN_REFUSED
        assert (r["N"], r["K"], r["Q"], r["T"]) == (c["N"], c["K"], c["Q"], c["T"] + 1)
        assert linhead_lds_floats(r["N"], r["N"] * r["K"], r["N"] * r["Q"], r["T"], True) > LINHEAD_LIMIT
        assert linhead_lds_floats(r["N"], r["N"] * r["K"], r["N"] * r["Q"], r["T"], False) <= LINHEAD_LIMIT
    return fl


def lin_inputs(c):
    """(episodes, [W [N, D], b [N]]) of a case (or of LIN_REFUSED), fp32 on the CPU."""
    ep = cg.make_episodes(7000 + c["seed"], c["B"], c["N"], c["K"], c["Q"], c["D"], 8)
    return ep, cg.make_maml_params(7000 + c["seed"], c["D"], None, c["N"])


@functools.lru_cache(maxsize=None)
def lin_reference(name):
    """oracle.fumi_ref.maml_meta_step in float64 on the fp32 inputs of case `name` (computed once, shared, never modified)."""
    c = LIN_CASES[name]
    ep, p = lin_inputs(c)
    pl = [t.double().requires_grad_(True) for t in p]
    out = R.maml_meta_step(pl, ep["x_s"].double(), ep["y_s"], ep["x_q"].double(), ep["y_q"], c["T"], ALPHA, c["fo"])
    return {k: ([g.detach() for g in v] if isinstance(v, list) else v.detach()) for k, v in out.items()}


def lin_manual(c):
    """The same meta-step without autograd, in float64: the low-rank algebra csrc/linhead.hip documents (E_t, the reverse sweep over
    the taped soft-max rows, gW = Abar^T X).  Returns (logits [B, Qn, N], loss_b [B], gW, gb of the mean loss)."""
    ep, p = lin_inputs(c)
    W, b = p[0].double(), p[1].double()
    B, N, T = c["B"], c["N"], c["T"]
    logits, loss_b, gW, gb = [], [], torch.zeros_like(W), torch.zeros_like(b)
    for e in range(B):
        xs, xq, ys, yq = ep["x_s"][e].double(), ep["x_q"][e].double(), ep["y_s"][e], ep["y_q"][e]
        S, Qn = xs.shape[0], xq.shape[0]
        Gss, Gqs = xs @ xs.t(), xq @ xs.t()
        oh_s, oh_q = torch.eye(N, dtype=torch.float64)[ys], torch.eye(N, dtype=torch.float64)[yq]
        E, tape = torch.zeros(S, N, dtype=torch.float64), []
        for _ in range(T):
            pt = torch.softmax(xs @ W.t() - ALPHA * (Gss @ E) + b - ALPHA * E.sum(0), -1)
            tape.append(pt)
            E = E + (pt - oh_s) / S
        zq = xq @ W.t() - ALPHA * (Gqs @ E) + b - ALPHA * E.sum(0)
        logits.append(zq)
        loss_b.append(-(torch.log_softmax(zq, -1) * oh_q).sum(-1).mean())
        lbar = (torch.softmax(zq, -1) - oh_q) / Qn
        Abar_s, bbar = torch.zeros(S, N, dtype=torch.float64), lbar.sum(0)
        if not c["fo"]:
            Eb = -ALPHA * (Gqs.t() @ lbar + lbar.sum(0)[None])
            for pt in reversed(tape):
                zb = pt * (Eb - (pt * Eb).sum(-1, keepdim=True)) / S
                Abar_s, bbar = Abar_s + zb, bbar + zb.sum(0)
                Eb = Eb - ALPHA * (Gss.t() @ zb + zb.sum(0)[None])
        gW += (Abar_s.t() @ xs + lbar.t() @ xq) / B
        gb += bbar / B
    return torch.stack(logits), torch.stack(loss_b), gW, gb


def rel_to_max(a, b, floor=1e-5):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def lin_check(name, out, need_grad=True):
    """A maml_step result (CPU tensors) against lin_reference(name) at the tolerances of tests/test_hip_parity.py: logits and loss_b
    1e-4 of the largest logit, predictions equal (tests/test_front_forms_cpu.py shows that no row is under the 1e-5 margin), acc_b,
    every gradient 1e-4 of its maximum with the floor of 5 % of the largest gradient.  Prints every error in units of its bound."""
    ref = lin_reference(name)
    zmax = float(ref["logits"].abs().max())
    e_log = rel_to_max(out["logits"], ref["logits"])
    e_loss = float((out["loss_b"].double() - ref["loss_b"]).abs().max()) / zmax
    msg = f"linhead {name}: logits {e_log / LOGIT_TOL:.4f}, loss {e_loss / LOGIT_TOL:.4f}"
    assert e_log <= LOGIT_TOL and e_loss <= LOGIT_TOL, msg
    assert torch.equal(out["preds"], ref["preds"]) and torch.equal(out["preds_f"], ref["preds"].float()), name
    assert torch.allclose(out["acc_b"].double(), ref["acc_b"].double(), rtol=0, atol=1e-6), name
    if need_grad:
        floor = max(0.05 * max(float(r.abs().max()) for r in ref["g_params"]), 1e-5)
        e_g = [rel_to_max(a, r, floor) for a, r in zip(out["g_params"], ref["g_params"])]
        msg += f", gW {e_g[0] / GRAD_TOL:.4f}, gb {e_g[1] / GRAD_TOL:.4f}"
        assert max(e_g) <= GRAD_TOL, msg
    print(msg + "  (units of the bound)")
