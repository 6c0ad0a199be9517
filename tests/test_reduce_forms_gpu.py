"""GPU suite: the three slab-reduction kernels and the embedding bag keep their bits.  The plain reduction (fumi_hip_reduce_segments)
against the float32 numpy restatement of its documented order, bit for bit, over slab counts around the load batch, element counts
around the workgroup, misaligned and strided segments; the folded reduction + optimizer launch against FUMI_ADAM_FUSE=0 in a fresh
process (the knob is read once); the bag's two-chunk pass against the stand-alone launch and the float32 CPU oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import reduce_forms_common as C
from helpers import rel_to_max
from oracle import casegen as cg
from oracle import fumi_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _launch_and_check(ws, dev, cases, scale):
    """All `cases` as the segments of ONE launch; every destination sits in a buffer of sentinels with GUARD words behind it."""
    from fumi_amd import hip
    segs, want, bufs = [], [], []
    for c in cases:
        x = c.slabs()
        src = torch.empty(x.size + 4, device=dev, dtype=torch.float32)                 # (torch allocations are 16-byte aligned)
        src[c.src_off:c.src_off + x.size] = torch.from_numpy(x.reshape(-1)).to(dev)
        dst = torch.full((c.dst_off + c.count + C.GUARD,), float(C.SENTINEL), device=dev, dtype=torch.float32)
        assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
        segs.append((src[c.src_off:c.src_off + x.size], c.ns, c.stride, c.count, dst[c.dst_off:]))
        want.append(C.two_chains(x[:, :c.count], scale))
        bufs.append(dst)
    hip.reduce_segments(ws, segs, scale)
    torch.cuda.synchronize()
    for c, w, dst in zip(cases, want, bufs):
        got = dst.cpu().numpy()
        out = got[c.dst_off:c.dst_off + c.count]
        assert np.array_equal(out.view(np.int32), w.view(np.int32)), (c.name, scale, int((out.view(np.int32) != w.view(np.int32)).sum()))
        rest = np.concatenate([got[:c.dst_off], got[c.dst_off + c.count:]])
        assert rest.size == c.dst_off + C.GUARD and (rest == C.SENTINEL).all(), (c.name, "wrote outside its segment")


@pytest.mark.parametrize("scale", [1.0, 1.0 / 32])
@pytest.mark.parametrize("ns", C.SLABS)
def test_every_slab_count_at_every_element_count(ns, scale, ws, dev):
    _launch_and_check(ws, dev, C.grid_cases(ns), scale)


@pytest.mark.parametrize("scale", [1.0, 1.0 / 32])
def test_offset_by_one_float_and_strides_beyond_the_count(scale, ws, dev):
    cases = C.odd_cases()
    for i in range(0, len(cases), 24):
        _launch_and_check(ws, dev, cases[i:i + 24], scale)


@pytest.mark.parametrize("scale", [1.0, 1.0 / 32])
def test_one_launch_of_24_mixed_segments(scale, ws, dev):
    _launch_and_check(ws, dev, C.mixed24(), scale)


def test_single_segments_and_argument_checks(ws, dev):
    from fumi_amd import hip
    _launch_and_check(ws, dev, [C.Case(16, 1028)], 1.0)
    _launch_and_check(ws, dev, [C.Case(33, 1)], 1.0)
    hip.reduce_segments(ws, [], 1.0)
    x = torch.zeros(64, device=dev)
    with pytest.raises(hip.FumiHipError):
        hip.reduce_segments(ws, [(x, 2, 64, 1, x)], 1.0)                  # the second slab lies past the source
    with pytest.raises(hip.FumiHipError):
        hip.reduce_segments(ws, [(x, 1, 1, 1, x)] * 25, 1.0)


def test_folded_optimizer_launch_equals_the_separate_launches_bit_for_bit(tmp_path):
    """Deferred Adam, AdamW, SGD with momentum (the step that creates the buffers and the next ones) and plain SGD, three steps at
    B = 2, N = 5, S = 5, Qn = 10, D = 256, h = [256, 64]: every gradient, parameter and state tensor and both published statistics
    of the default (folded) run equal those of a FUMI_ADAM_FUSE=0 child."""
    assert os.environ.get("FUMI_ADAM_FUSE", "1") == "1"
    out = tmp_path / "unfused.pt"
    r = subprocess.run([sys.executable, os.path.abspath(C.__file__), str(out)], env=dict(os.environ, FUMI_ADAM_FUSE="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    b = torch.load(out, weights_only=False)
    a = C.run_rules()
    for rule in C.RULES:
        assert len(a[rule]["folded"]) == 2 and all(a[rule]["folded"]), (rule, a[rule]["folded"])       # steps 2 and 3 were folded
        # (the child's flags say the same: with FUMI_ADAM_FUSE=0 the step launches the pending update itself, right behind its plain
        # reduction, so nothing is left for finish_deferred there either -- the knob, not the flag, is what separates the two runs)
        assert len(b[rule]["folded"]) == 2
        assert a[rule]["stats"] == b[rule]["stats"], rule
        assert len({s[0] for s in a[rule]["stats"]}) == 3 and all(np.isfinite(v) for s in a[rule]["stats"] for v in s)
        assert len(a[rule]["tensors"]) == len(b[rule]["tensors"]) >= 16
        for i, (x, y) in enumerate(zip(a[rule]["tensors"], b[rule]["tensors"])):
            assert torch.equal(x, y), (rule, i)


# ---- the embedding bag ------------------------------------------------------------------------------------------------------------
def _tokens(V, L, rows, seed):
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(1, V, (rows, L), generator=g)
    for r in range(rows):
        if r % 3 == 1:
            tok[r, 1 + (r * 5) % L:] = 0                       # a PAD tail of varying length
    keep = int(torch.randint(0, L, (1,), generator=g))
    tok[rows - 1] = 0
    tok[rows - 1, keep] = 7                                    # all but one token PAD
    tok[rows - 2, 1:] = 0                                      # ... and the one kept is the first
    return tok


@pytest.mark.parametrize("L", [1, 8, 17, 128])
@pytest.mark.parametrize("E", [300, 4, 257])
def test_bag_rows_against_the_cpu_oracle(E, L, ws, dev):
    """E = 300: two chunks of 64 float4 lanes gathered in one pass; E = 4: one chunk; E = 257: the scalar path, five chunks."""
    from fumi_amd import hip
    V = 500
    table = torch.rand(V, E, generator=torch.Generator().manual_seed(E)) * 2 - 1
    table[0] = 0
    tok = _tokens(V, L, 12, 1000 * E + L)
    for mode in ("mean", "max"):
        out = hip.glove_bag(ws, tok.to(dev), table.to(dev), 0, mode).cpu()
        assert rel_to_max(out, R.word_embedding_pool(tok, table, 0, mode)) <= 1e-6, mode
    assert ws.read_status() == 0


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("L", [1, 8, 17, 128])
@pytest.mark.parametrize("E", [300, 4])
def test_bag_riding_in_the_step_equals_the_stand_alone_launch(E, L, mode, ws, dev):
    """The deferred bag (carried by the first launch of the FuMI step, xpanel.hip) against the stand-alone kernel (glove.hip) on the
    same rows: both run the one device body, so the pooled rows are equal bit for bit.  E = 300: two chunks in one pass; E = 4: one
    chunk.  (E = 257 cannot ride: the hypernetwork forward that carries the bag takes text widths that are multiples of 4 only, and
    the step then launches the stand-alone kernel, which the test above covers.)  That the bag DID ride is read from the record of
    the forward X-panel launch: the pre-split form with its rider is exactly the condition under which the step carries the bag."""
    from fumi_amd import hip
    B, N, K, Q, D, hid, Ht, V = 2, 5, 1, 2, 512, [256, 64], 256, 500          # (D >= 288: the forward pass pre-splits from 9 slabs of 32)
    ep = cg.make_episodes(40 + L, B, N, K, Q, D, 1, tokens=(V, L, 0))
    tok = ep["text_s"].clone()
    tok[0, 0, 1:] = 0                                          # one row with all but one token PAD
    theta, phi = cg.make_fumi_params(41, D, hid, E, Ht)
    table = torch.rand(V, E, generator=torch.Generator().manual_seed(42)) * 2 - 1
    table[0] = 0
    g = lambda t: t.to(dev).contiguous()
    tk, ys, tb = g(tok), g(ep["y_s"]), g(table)
    alone = hip.glove_bag_select(ws, tk, ys, N, tb, 0, mode)
    rode = hip.glove_bag_select(ws, tk, ys, N, tb, 0, mode, defer=True)
    hip.fumi_step(ws, g(ep["x_s"]), ys, g(ep["x_q"]), g(ep["y_q"]), [g(t) for t in theta], [g(t) for t in phi], 1, cg.ALPHA, False,
                  cls_text=rode)
    torch.cuda.synchronize()
    assert ws.read_status() == 0
    plan = hip.xpanel_plan()
    assert hip.XPANEL_FWD_KERNELS[plan["fwd_kernel"]] == "presplit" and plan["fwd_rode"] == 1, plan
    assert torch.equal(rode, alone)
    rows = torch.stack([R.class_text_select(tok[b], ep["y_s"][b], N) for b in range(B)])
    assert rel_to_max(alone.cpu(), R.word_embedding_pool(rows, table, 0, mode)) <= 1e-6
