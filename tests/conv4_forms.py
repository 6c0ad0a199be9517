"""Shared checkers and the edge-case table of the fp32 Conv4 encoder (csrc/conv_gemm.hip, conv_first.hip, conv_ew.hip, conv4.hip),
used by tests/test_conv4_gpu.py, tests/test_conv4_edges_gpu.py and tests/test_conv4_edges_cpu.py -- TEST INFRASTRUCTURE ONLY.

The checkers compare the engine with the float64 autograd-free sweep oracle/conv4_manual.py (tied to autograd in
tests/test_conv4_manual.py and, at the shapes of the table below, in tests/test_conv4_edges_cpu.py).

The case table names, per case, the launch edge it is there for.  Two host formulas of the engine are restated here in plain Python
(c1_chunks: csrc/conv_first.hip; coef_chunks: cv_tiles of csrc/conv4.h over COEF_CHUNK of csrc/conv_ew.hip) ONLY to assert that a
case still reaches its edge: when someone changes 1024, 128 or 64 in the engine the case fails instead of going quiet.
"""
import itertools
from collections import OrderedDict

import torch

from oracle import conv4_manual as M
from oracle import conv4_ref as C
from helpers import rel_to_max

LOGIT_TOL, GRAD_TOL, MARGIN = 1e-4, 1e-3, 1e-5
TIE_TOL = 3e-6
MAX_TIES = 6            # near-tie decisions _match_episodes enumerates per episode (2^6 assignments at the most)


def _g(t, dev):
    return t.to(dev).contiguous()


def _unpad(flat, B, Mi, H, W):
    """padded channels-last [B*M][(H+2)(W+2)][64] -> NCHW [B, M, 64, H, W]; also returns the largest |border| value."""
    t = flat.reshape(B, Mi, H + 2, W + 2, 64)
    inner = t[:, :, 1:-1, 1:-1, :]
    frame = t.clone()
    frame[:, :, 1:-1, 1:-1, :] = 0
    return inner.permute(0, 1, 4, 2, 3), float(frame.abs().max())


def _case(seed, B, N, K, Q, Cin, H, W, nblk):
    ep = C.make_image_episodes(seed, B, N, K, Q, Cin, H, W, 12)
    theta = C.make_conv4_params(seed, Cin, 64, nblk)
    Fd = C.feature_dim(H, W, 64, nblk)
    return ep, theta, Fd


def _slab_to_torch(slab, Cin, nblk):
    """One episode's parameter slab in the engine's canonical layouts (csrc/conv4.hip: W1 [64][32], W_l [tap][co][ci], BN weight,
    BN bias per block) -> tensors in torch layouts."""
    out, off = [], 0
    for l in range(nblk):
        if l == 0:
            out.append(slab[off:off + 2048].reshape(64, 32)[:, :Cin * 9].reshape(64, Cin, 3, 3)); off += 2048
        else:
            out.append(slab[off:off + 36864].reshape(9, 64, 64).permute(1, 2, 0).reshape(64, 64, 3, 3)); off += 36864
        out += [slab[off:off + 64], slab[off + 64:off + 128]]; off += 128
    return out


def _match_episodes(hip, ws, dev, logits, theta, heads, ep, T, alpha, first_order, need_grad=True):
    """Per episode: the float64 autograd-free sweep (oracle/conv4_manual.py, tied to autograd at 1e-9) against the engine's query
    logits and its per-episode meta-gradients (fumi_hip_conv4_probe).  A ReLU / arg-max decision within fp32 noise of a tie may
    fall either way in two correct fp32 implementations: the forward value does not move, but the gradient routed through that
    unit switches on or off and moves a weight gradient by O(1/sqrt(#terms)) (tests/dev/probe_conv4_flip.py).  With ~5e5
    decisions per case such a tie (margin < 3e-6) is present in most cases, so the checker enumerates the decisions of the
    float64 sweep that lie within TIE_TOL of a tie (at most 6) and requires the engine to agree with ONE assignment of them, at
    the usual tolerances.  Returns the matched per-episode (logits, loss, d theta, d head, trace)."""
    B, Cin, nblk = logits.shape[0], ep["x_s"].shape[2], len(theta) // 3
    th64 = [t.double() for t in theta]
    if need_grad:
        bar = hip.conv4_probe(ws, dev, -1, 4).cpu().reshape(B, -1)
        barh = hip.conv4_probe(ws, dev, -1, 5).cpu().reshape(B, heads.shape[1], -1)
    out = []
    for b in range(B):
        args = (th64, heads[b].double(), ep["x_s"][b].double(), ep["y_s"][b], ep["x_q"][b].double(), ep["y_q"][b], T, alpha, first_order)
        tr0 = {}
        M.episode_grads(*args, trace=tr0)
        amb = M.ambiguous_decisions(tr0, TIE_TOL, limit=MAX_TIES)
        subsets = [()] + [c for k in range(1, len(amb) + 1) for c in itertools.combinations(amb, k)]
        got = _slab_to_torch(bar[b], Cin, nblk) + [barh[b]] if need_grad else None
        errs = None
        for sub in subsets:
            tr = {}
            zq, loss, bth, bh = M.episode_grads(*args, trace=tr, flips=M.flips_of(sub))
            e_log = rel_to_max(logits[b], zq)
            e_g = 0.0
            if need_grad:
                ref = bth + [bh]
                floor = max(0.02 * max(float(r.abs().max()) for r in ref), 1e-9)
                e_g = max(rel_to_max(a, r, floor) for a, r in zip(got, ref))
            errs = errs or (e_log, e_g)
            if e_log <= LOGIT_TOL and e_g <= GRAD_TOL:
                out.append((zq, loss, bth, bh, tr))
                break
        else:
            raise AssertionError(f"episode {b}: logits / gradient error {errs[0]:.2e} / {errs[1]:.2e} against the float64 sweep, and no "
                                 f"assignment of its {len(amb)} near-tie decisions (margins {[f'{m[0]:.1e}' for m in amb]}) explains it")
    return out


def _cmp(name, got, ref, tol=2e-4):
    e = rel_to_max(got, ref, floor=1e-6)
    assert e <= tol, f"{name}: rel-to-max error {e:.3e}"


def _check_grads(names, got, ref):
    floor = max(0.02 * max(float(r.abs().max()) for r in ref), 1e-7)
    for n, a, r in zip(names, got, ref):
        e = rel_to_max(a.cpu(), r, floor)
        assert e <= GRAD_TOL, f"grad {n}: rel-to-max error {e:.3e}"


def maml_inputs(shape, B, N, K, Q, seed):
    """(episodes, theta, head [N, F+1]) of the per-intermediate walker and of the whole-step checks at the edges: the head is drawn
    from a generator of its own so that the parameters of a shape do not depend on N."""
    Cin, H, W, nblk = shape
    ep, theta, Fd = _case(seed, B, N, K, Q, Cin, H, W, nblk)
    g = torch.Generator().manual_seed(5)
    head = torch.cat([torch.randn(N, Fd, generator=g) * 0.2, torch.rand(N, 1, generator=g) * 0.2 - 0.1], 1)
    return ep, theta, head


def check_every_intermediate(hip, ws, dev, shape, B, N, K, Q, T, alpha, seed, fused):
    """One second-order MAML meta-step; then EVERY tensor the engine stored on the way (fumi_hip_conv4_probe) against the float64
    sweep: conv outputs, pooled maps, soft-max, dz, dxo, du of every pass and block, and the tangent counterparts of the last
    Hessian-vector product, each to 2e-4 of its scale with borders exactly 0.  fused: block 1 ran band by band and stored no map."""
    Cin, H, W, nblk = shape
    ep, theta, head = maml_inputs(shape, B, N, K, Q, seed)
    S, Qn = N * K, N * Q
    p = theta + [head[:, :-1].contiguous(), head[:, -1].contiguous()]
    out = hip.maml_conv4_step(ws, _g(ep["x_s"], dev), _g(ep["y_s"], dev), _g(ep["x_q"], dev), _g(ep["y_q"], dev),
                              [_g(t, dev) for t in p], T, alpha)
    assert ws.read_status() == 0
    probe = lambda pa, kind, blk=0: hip.conv4_probe(ws, dev, pa, kind, blk).cpu()
    # the float64 sweep of each episode, with its near-tie decisions taken the way the engine took them
    traces = [m[4] for m in _match_episodes(hip, ws, dev, out["logits"].cpu(), theta, head[None].expand(B, -1, -1), ep, T, alpha, False)]
    geo = [(H >> l, W >> l) for l in range(nblk + 1)]
    for t in range(T + 1):                                              # support steps, then the query pass
        Mi = S if t < T else Qn
        tapes = [tr["tapes"][t] if t < T else tr["query"] for tr in traces]
        for l in range(nblk):
            Hl, Wl = geo[l]
            if not (fused and l == 0):                              # (the fused path never stores block 1's maps)
                u, bu = _unpad(probe(t, 0, l), B, Mi, Hl, Wl)
                _cmp(f"pass {t} block {l} u", u, torch.stack([tp["blocks"][l]["u"] for tp in tapes]))
                assert bu == 0.0, f"pass {t} block {l}: conv output border not zero"
            xo = probe(t, 1, l)
            ref_xo = torch.stack([tp["blocks"][l]["xo"] for tp in tapes])
            if l + 1 < nblk:
                xo, bx = _unpad(xo, B, Mi, *geo[l + 1])
                assert bx == 0.0
            else:
                xo = xo.reshape(B, Mi, -1); ref_xo = ref_xo.reshape(B, Mi, -1)
            _cmp(f"pass {t} block {l} pooled", xo, ref_xo)
        _cmp(f"pass {t} p", probe(t, 5).reshape(B, Mi, N), torch.stack([tp["p"] for tp in tapes]))
        _cmp(f"pass {t} dz", probe(t, 6).reshape(B, Mi, N), torch.stack([tp["dz"] for tp in tapes]))
        for l in reversed(range(nblk)):
            Hl, Wl = geo[l]
            dxo = probe(t, 3, l)
            ref = torch.stack([tp["blocks"][l]["dxo"] for tp in tapes])
            if l + 1 < nblk:
                dxo, _ = _unpad(dxo, B, Mi, *geo[l + 1])
            else:
                dxo = dxo.reshape(ref.shape)
            _cmp(f"pass {t} block {l} dxo", dxo, ref)
            if fused and l == 0:
                continue
            du, bd = _unpad(probe(t, 2, l), B, Mi, Hl, Wl)
            _cmp(f"pass {t} block {l} du", du, torch.stack([tp["blocks"][l]["du"] for tp in tapes]))
            assert bd == 0.0, f"pass {t} block {l}: du border not zero"
    # tangent scratch of the last Hessian-vector product (inner step 0)
    tp0 = [tr["tapes"][0] for tr in traces]
    for l in range(nblk):
        Hl, Wl = geo[l]
        if not (fused and l == 0):
            ud, _ = _unpad(probe(T + 1, 0, l), B, S, Hl, Wl)
            _cmp(f"tangent block {l} u'", ud, torch.stack([tp["blocks"][l]["ud"] for tp in tp0]))
        xod = probe(T + 1, 1, l)
        ref = torch.stack([tp["blocks"][l]["xod"] for tp in tp0])
        xod = _unpad(xod, B, S, *geo[l + 1])[0] if l + 1 < nblk else xod.reshape(ref.shape)
        _cmp(f"tangent block {l} x'", xod, ref)
    for l in reversed(range(nblk)):
        Hl, Wl = geo[l]
        dxod = probe(T + 1, 3, l)
        ref = torch.stack([tp["blocks"][l]["dxod"] for tp in tp0])
        dxod = _unpad(dxod, B, S, *geo[l + 1])[0] if l + 1 < nblk else dxod.reshape(ref.shape)
        _cmp(f"tangent block {l} dxo'", dxod, ref)
        if fused and l == 0:
            continue
        dud, bd = _unpad(probe(T + 1, 2, l), B, S, Hl, Wl)
        _cmp(f"tangent block {l} du'", dud, torch.stack([tp["blocks"][l]["dud"] for tp in tp0]))
        assert bd == 0.0


# ---- the edges of the launch forms ------------------------------------------------------------------------------------------
def c1_chunks(B, M, H):
    """csrc/conv_first.hip c1_chunks for B episodes (of one lane) of M images of height H: (bands a persistent workgroup walks,
    workgroups per episode, bands per image)."""
    bpi = (H + 1) // 2
    nbands = M * bpi
    nt = max(1, min((1024 + B - 1) // B, nbands))
    chunk = (nbands + nt - 1) // nt
    return chunk, (nbands + chunk - 1) // chunk, bpi


def coef_chunks(M, H, W):
    """Level-1 workgroups of the two-level coefficient sum over the per-tile statistics of a convolution of M images at H x W:
    ceil(M (H+2) (W+2) / 128) tiles (cv_tiles, CV_TILE) in chunks of 64 (COEF_CHUNK)."""
    tiles = (M * (H + 2) * (W + 2) + 127) // 128
    return (tiles + 63) // 64


ALPHA = 0.05
# shape = (Cin, H, W, nblk).  `lanes`: value of conv4_set_option(1, .) for the case (None: the default).  `chunk`: what c1_chunks must
# give for (support, query); `coef`: what coef_chunks must give at block 1.  The seeds are conditions on the INPUTS: every episode of
# a case has at most MAX_TIES decisions of the float64 sweep within TIE_TOL of a tie (tests/test_conv4_edges_cpu.py) -- if a seed
# breaks that, change the seed, never the cap.
CASES = OrderedDict([
    ("A", dict(shape=(3, 9, 13, 2), B=2, N=3, K=2, Q=3, T=2, seed=41, lanes=None, chunk=(1, 1), coef=1)),
    ("B", dict(shape=(2, 15, 10, 3), B=2, N=3, K=2, Q=3, T=2, seed=42, lanes=None, chunk=(1, 1), coef=1)),
    ("C", dict(shape=(1, 7, 22, 2), B=2, N=3, K=2, Q=3, T=2, seed=43, lanes=None, chunk=(1, 1), coef=1)),
    ("D", dict(shape=(3, 21, 23, 2), B=16, N=3, K=2, Q=3, T=1, seed=44, lanes=1, chunk=(2, 2), coef=1)),
    ("E", dict(shape=(3, 29, 31, 2), B=2, N=3, K=3, Q=3, T=1, seed=45, lanes=None, chunk=(1, 1), coef=2)),
])
WHOLE_STEP_CASES = ("A", "B", "C")


def case_reaches_its_edge(name):
    """Asserts, from the restated host formulas, that case `name` still reaches the branch it is named for."""
    c = CASES[name]
    Cin, H, W, nblk = c["shape"]
    S, Qn = c["N"] * c["K"], c["N"] * c["Q"]
    chunks = tuple(c1_chunks(c["B"], m, H)[0] for m in (S, Qn))
    assert chunks == c["chunk"], (name, chunks)
    assert max(coef_chunks(m, H, W) for m in (S, Qn)) == c["coef"], name
    assert C.feature_dim(H, W, 64, nblk) >= 64
    if name == "A":
        assert H % 2 and W % 2 and H != W and (H >> nblk) != (W >> nblk)
    if name == "B":
        assert Cin == 2 and H % 2 and not W % 2 and (H >> 1) % 2 and (W >> 1) % 2 and (H >> nblk, W >> nblk) == (1, 1)
    if name == "C":
        assert Cin == 1 and H % 2 and 8 < (W + 1) // 2 < 16 and (H >> 1) % 2 and (W >> 1) % 2
    if name == "D":
        assert c["lanes"] == 1 and min(chunks) >= 2 and c1_chunks(c["B"], S, H)[2] % 2 == 1
        assert all(c1_chunks(c["B"], m, H)[1] <= 64 for m in (S, Qn))
    if name == "E":
        tiles = (Qn * (H + 2) * (W + 2) + 127) // 128
        assert coef_chunks(Qn, H, W) >= 2 and 0 < tiles % 64 < 16 and H % 2 and W % 2 and H != W


def fumi_inputs(name):
    """(episodes, theta, phi, Dt) of the FuMI whole-step check of a case (the hypernetwork emits the [N, F+1] head)."""
    from oracle import casegen as cg
    c = CASES[name]
    Cin, H, W, nblk = c["shape"]
    ep, theta, Fd = _case(c["seed"] + 100, c["B"], c["N"], c["K"], c["Q"], Cin, H, W, nblk)
    _, phi = cg.make_fumi_params(c["seed"], 8, [Fd], 12, 16, head_scale=0.3)
    return ep, theta, phi


def fumi_heads(ep, phi, N, tanh):
    """The hypernetwork in float64 (graph kept on the returned phi copies): heads [B, N, F+1]."""
    from oracle import fumi_ref as R
    ph = [t.double().requires_grad_(True) for t in phi]
    B = ep["x_s"].shape[0]
    heads = torch.stack([R.hyper_net(R.class_text_select(ep["text_s"][b].double(), ep["y_s"][b], N), ph, tanh) for b in range(B)])
    return heads, ph


def deepest_tie_block(groups, theta):
    """Largest block index at which the float64 forward of any group of images (one batch-statistics group each) takes a ReLU /
    arg-max decision within TIE_TOL of a tie; -1 when none does.  A decision at block l that falls the other way in fp32 re-routes
    the gradient of block l and of every block before it."""
    th = [t.double() for t in theta]
    h = torch.zeros(1, C.feature_dim(groups[0].shape[2], groups[0].shape[3], 64, len(theta) // 3) + 1, dtype=torch.float64)
    deepest = -1
    for x in groups:
        _, tape = M.net_fwd(x.double(), th, h)
        for l, tp in enumerate(tape["blocks"]):
            if tp["margin"] < TIE_TOL:
                deepest = max(deepest, l)
    return deepest
