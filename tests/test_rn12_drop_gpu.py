"""GPU tests of DropBlock / dropout in the bf16 ResNet-12 (fumi_amd/csrc/rn12_drop.hip, fumi_hip_resnet12_encode_drop /
fumi_hip_resnet12_encode_bwd_drop) against tests/rn12_drop_ref.py.

  * the two launches on a raw map: kept, scale and every output element bit-exact, borders untouched;
  * all rates 0: the bits of the pair without drop;
  * rates on: the taped and the recompute form, every chunking and a rerun bit-identical (the mask is indexed globally);
  * against the float64 network with the reference's masks.  The encoder is bf16 and "parity unpinned": the bound is relative to the
    engine's own error with drop OFF on the same shape -- the drop-on relative L2 error of the features and of every gradient tensor
    must stay within 2 x the drop-off one (scale <= ~2 at rate 0.5 amplifies the bf16 rounding of the masked maps; a mask missing
    from the backward, or another mask, misses by orders of magnitude);
  * the tape refuses a backward under another seed;
  * one Pretrain and one MetaBaseline training step, and their evaluation paths, which never drop."""
import numpy as np
import pytest
import torch

import rn12_drop_ref as R

pytestmark = pytest.mark.gpu
SEED = 0x5EED0123456789AB


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wss(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev), hip.Workspace.get(dev, "encoder")


def _to_dev_bf16(bits, dev):
    return torch.from_numpy(bits.view(np.int16).copy()).to(dev).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


# ---- the two launches on a raw map ------------------------------------------------------------------------------------------------------
RAW_CASES = [  # C, H, W, M, block, rate, b0   (B = 3)
    (32, 5, 5, 1, 1, 0.1, 0), (32, 5, 5, 5, 3, 0.5, 2), (160, 5, 5, 7, 5, 0.1, 0), (32, 5, 5, 5, 8, 0.5, 1),
    (160, 10, 10, 5, 3, 0.1, 3), (32, 10, 10, 7, 5, 0.5, 0), (32, 10, 10, 1, 1, 0.5, 0),
    (32, 11, 11, 7, 3, 0.5, 5), (160, 11, 11, 1, 5, 0.1, 0), (32, 11, 11, 5, 1, 0.1, 2),
    (32, 21, 21, 5, 5, 0.1, 1), (160, 21, 21, 1, 3, 0.5, 0), (32, 21, 21, 7, 1, 0.5, 0),
    (32, 42, 42, 5, 1, 0.1, 0), (32, 42, 42, 7, 5, 0.5, 4), (160, 42, 42, 1, 5, 0.1, 0), (160, 42, 42, 5, 1, 0.5, 1),
    (32, 5, 11, 5, 8, 0.5, 0), (64, 11, 5, 7, 3, 0.1, 1),            # not square: the block size clamps to the shorter side
]


@pytest.mark.parametrize("C,H,W,M,block,rate,b0", RAW_CASES)
def test_drop_apply_is_bit_exact(C, H, W, M, block, rate, b0, dev, wss):
    from fumi_amd import hip
    B, npix = 3, M * (H + 2) * (W + 2)
    rs = np.random.RandomState(C + H + 7 * M + block)
    inner = np.zeros((B, M, H + 2, W + 2, C), dtype=np.float32)
    ones, rand = inner.copy(), inner.copy()
    ones[:, :, 1:-1, 1:-1] = 1.0
    rand[:, :, 1:-1, 1:-1] = rs.standard_normal((B, M, H, W, C)).astype(np.float32)
    for name, src in (("ones", ones), ("random", rand)):
        bits = R.f32_to_bf16_bits(src).reshape(B, npix, C)
        want, kept_w, scale_w = R.apply_map(bits, M, H, W, rate, block, SEED, 2, 1, b0)
        x = _to_dev_bf16(bits, dev)
        kept, scale = hip.rn12_drop_apply(wss[0], x, H, W, rate, block, SEED, block_index=2, set_index=1, b0=b0)
        torch.cuda.synchronize()
        assert np.array_equal(kept.cpu().numpy(), kept_w), (name, kept.cpu().numpy(), kept_w)
        assert np.array_equal(scale.cpu().numpy().view(np.uint32), scale_w.view(np.uint32)), name
        got = _bits(x)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        g5 = got.reshape(B, M, H + 2, W + 2, C)
        assert not g5[:, :, 0].any() and not g5[:, :, -1].any() and not g5[:, :, :, 0].any() and not g5[:, :, :, -1].any()
    assert 0 < kept_w.min() and kept_w.max() < M * H * W * C              # something dropped, something kept, in every group


def test_drop_apply_refuses_oversize_arguments(dev, wss):
    from fumi_amd import hip
    x = torch.ones(1, 67 * 67, 32, device=dev, dtype=torch.bfloat16)
    for H, W, rate, block in ((5, 5, 0.1, 9), (5, 5, 0.1, 0), (65, 65, 0.1, 5), (65, 5, 0.1, 2), (5, 5, 1.0, 3), (5, 5, -0.1, 1)):
        with pytest.raises(hip.FumiHipError):
            hip.rn12_drop_apply(wss[0], x, H, W, rate, block, SEED)
    assert bool((x == 1).all())                                            # a refused call launches nothing
    hip.rn12_drop_apply(wss[0], x, 65, 65, 0.1, 1, SEED)                   # element-wise dropout has no 64-limit
    torch.cuda.synchronize()
    inner = x.view(67, 67, 32)[1:-1, 1:-1]
    assert 0.05 < float((inner == 0).float().mean()) < 0.15


# ---- the encoder pair ---------------------------------------------------------------------------------------------------------------------
CHANNELS = (32, 64)
RATES, BLOCKS = [0.1, 0.5], [1, 3]       # dropout at the literature's rate on the first block, DropBlock 3 at the harshest tested rate on the 5 x 5 map


def _case(seed, H, B=3, S=5, Qn=7):
    g = torch.Generator().manual_seed(seed)
    x_s, x_q = torch.randn(B, S, 3, H, H, generator=g), torch.randn(B, Qn, 3, H, H, generator=g)
    dfs, dfq = torch.randn(B, S, CHANNELS[-1], generator=g), torch.randn(B, Qn, CHANNELS[-1], generator=g)
    return x_s, x_q, R.make_theta(seed, 3, CHANNELS), dfs, dfq


def _pair(wss, dev, case, drop=None, seed_bwd=None):
    """(feats_s, feats_q, g_theta, plan) of encode (tape kept) -> encode_bwd; drop = (rates, blocks, seed) runs the _drop entries."""
    from fumi_amd import hip
    x_s, x_q, theta, dfs, dfq = case
    xs, xq, th = x_s.to(dev), x_q.to(dev), [t.to(dev).contiguous() for t in theta]
    if drop is None:
        fs, fq = hip.resnet12_encode(wss[1], xs, xq, th, keep_tape=True)
        plan = hip.resnet12_encode_plan()
        g = hip.resnet12_encode_bwd(wss[1], xs, xq, dfs.to(dev), dfq.to(dev), th)
    else:
        fs, fq = hip.resnet12_encode_drop(wss[1], xs, xq, th, *drop, keep_tape=True)
        plan = hip.resnet12_encode_plan()
        g = hip.resnet12_encode_bwd_drop(wss[1], xs, xq, dfs.to(dev), dfq.to(dev), th, drop[0], drop[1],
                                         drop[2] if seed_bwd is None else seed_bwd)
    torch.cuda.synchronize()
    assert wss[1].read_status() == 0
    return fs.clone(), fq.clone(), [t.clone() for t in g], plan


def _same(a, b, what):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what
    assert len(a[2]) == len(b[2]) == 12 * len(CHANNELS)
    for i, (x, y) in enumerate(zip(a[2], b[2])):
        assert torch.equal(x, y), (what, i)


@pytest.mark.parametrize("H", [20, 22])
def test_all_rates_zero_is_the_pair_without_drop(H, dev, wss):
    case = _case(51, H)
    plain = _pair(wss, dev, case)
    zero = _pair(wss, dev, case, ([0.0, 0.0], [1, 5], SEED))
    assert plain[3] == zero[3]
    _same(plain, zero, "rates 0")


def _forms(wss, dev, case, drop):
    """The pair under every plan a budget can force at this shape: {(taped, chunk): run}."""
    from fumi_amd import hip
    runs = {}
    try:
        for gb in [0.0, 1e-6] + list(np.geomspace(2e-4, 5e-2, 14)):
            hip.resnet12_set_budget(gb)
            r = _pair(wss, dev, case, drop)
            runs.setdefault((r[3][0], r[3][1]), r)
    finally:
        hip.resnet12_set_budget(0)
    wss[1].set_profiling(True)                             # (phase timing runs one lane: the whole meta-batch is one chunk)
    try:
        r = _pair(wss, dev, case, drop)
        runs.setdefault((r[3][0], r[3][1]), r)
    finally:
        wss[1].set_profiling(False)
    return runs


@pytest.mark.parametrize("H", [20, 22])
def test_forms_chunkings_and_a_rerun_are_bit_identical_with_drop_on(H, dev, wss):
    case, drop = _case(53, H), (RATES, BLOCKS, SEED)
    runs = _forms(wss, dev, case, drop)
    print("plans seen (taped, chunk):", sorted(runs))
    assert {(False, 1), (True, 2), (True, 3)} <= set(runs), sorted(runs)   # recompute one by one, taped in two chunks, one chunk
    base = runs[(True, 2)]
    for k, r in runs.items():
        _same(base, r, k)
    _same(base, _pair(wss, dev, case, drop), "rerun")
    plain = _pair(wss, dev, case)
    assert not torch.equal(plain[0], base[0]) and not torch.equal(plain[1], base[1])
    other = _pair(wss, dev, case, (RATES, BLOCKS, SEED + 1))
    assert not torch.equal(other[0], base[0])


def _rel_l2(got, ref):
    return float((got.cpu().double() - ref).norm() / ref.norm())


@pytest.mark.parametrize("H", [20, 22])
def test_drop_on_stays_within_twice_the_drop_off_error_of_the_float64_network(H, dev, wss):
    """Measured (rel-L2 against float64, drop off / drop on) are printed per tensor; DESIGN.md section 46 records them."""
    case = _case(55, H)
    x_s, x_q, theta, dfs, dfq = case
    off = _pair(wss, dev, case)
    on = _pair(wss, dev, case, (RATES, BLOCKS, SEED))
    ref_off = R.encode_pair_ref(x_s, x_q, theta, dfs, dfq)
    ref_on = R.encode_pair_ref(x_s, x_q, theta, dfs, dfq, RATES, BLOCKS, SEED)
    names = ["feats_s", "feats_q"] + [f"g_theta[{i}]" for i in range(12 * len(CHANNELS))]
    rows = []
    for i, n in enumerate(names):
        pick = (lambda r: r[i]) if i < 2 else (lambda r: r[2][i - 2])
        rows.append((n, _rel_l2(pick(off), pick(ref_off)), _rel_l2(pick(on), pick(ref_on))))
    for n, e0, e1 in rows:
        print(f"H={H} {n}: drop off {e0:.3e}, drop on {e1:.3e}, ratio {e1 / e0:.2f}")
    for n, e0, e1 in rows:
        assert e1 <= 2.0 * e0, (n, e0, e1)


def test_backward_under_another_seed_is_refused_and_the_tape_stays(dev, wss):
    from fumi_amd import hip
    case, drop = _case(57, 20), (RATES, BLOCKS, SEED)
    good = _pair(wss, dev, case, drop)
    x_s, x_q, theta, dfs, dfq = case
    xs, xq, th = x_s.to(dev), x_q.to(dev), [t.to(dev).contiguous() for t in theta]
    hip.resnet12_encode_drop(wss[1], xs, xq, th, *drop, keep_tape=True)
    for bad in ((RATES, BLOCKS, SEED + 1), ([0.1, 0.25], BLOCKS, SEED), (RATES, [1, 5], SEED)):
        with pytest.raises(hip.FumiHipError):
            hip.resnet12_encode_bwd_drop(wss[1], xs, xq, dfs.to(dev), dfq.to(dev), th, *bad)
    with pytest.raises(hip.FumiHipError):                  # the entry without drop is not this tape's backward either
        hip.resnet12_encode_bwd(wss[1], xs, xq, dfs.to(dev), dfq.to(dev), th)
    g = hip.resnet12_encode_bwd_drop(wss[1], xs, xq, dfs.to(dev), dfq.to(dev), th, *drop)
    torch.cuda.synchronize()
    for a, b in zip(good[2], g):
        assert torch.equal(a, b)
    with pytest.raises(hip.FumiHipError):                  # rates the kernels refuse, before anything runs
        hip.resnet12_encode_drop(wss[1], xs, xq, th, [0.1, 1.0], BLOCKS, SEED, keep_tape=True)
    with pytest.raises(hip.FumiHipError):
        hip.resnet12_encode_drop(wss[1], xs, xq, th, RATES, [1, 9], SEED, keep_tape=True)


# ---- the models -----------------------------------------------------------------------------------------------------------------------
SIZE, N, K, Q = 16, 3, 2, 4


def _episodes(seed, dev, B=2):
    g = torch.Generator().manual_seed(seed)
    y_s = torch.stack([(torch.arange(N * K) % N)[torch.randperm(N * K, generator=g)] for _ in range(B)])
    y_q = torch.stack([(torch.arange(N * Q) % N)[torch.randperm(N * Q, generator=g)] for _ in range(B)])
    x_s, x_q = torch.randn(B, N * K, 3, SIZE, SIZE, generator=g), torch.randn(B, N * Q, 3, SIZE, SIZE, generator=g)
    return {"train": ((None, None, x_s.to(dev)), y_s.to(dev)), "test": ((None, None, x_q.to(dev)), y_q.to(dev))}


def _build(kind, dev, drop):
    """The model with a two-block backbone (the step reads the depth from the module) and, with ``drop``, rate 0.5 from step 0."""
    from fumi_amd.models.metabaseline import MetaBaseline
    from fumi_amd.models.pretrain import Pretrain
    from fumi_amd.models.resnet12 import DropSchedule, ResNet12
    torch.manual_seed(23)
    if kind == "pretrain":
        model = Pretrain("resnet12", image_size=SIZE, image_channels=3, n_classes=6, bn_group=4, num_ways=N)
    else:
        model = MetaBaseline("resnet12", image_size=SIZE, image_channels=3, num_ways=N)
    torch.manual_seed(29)
    model.conv = ResNet12(3, (32, 32), SIZE)
    if kind == "pretrain":
        model.classifier = torch.nn.Linear(model.conv.feature_dim, 6)
    if drop:
        model.drop = DropSchedule(0.5, block_size=3, blocks=1, anneal_steps=0, seed=11, n_blocks=2)
    return model.to(dev)


@pytest.mark.parametrize("kind", ["pretrain", "metabaseline"])
def test_training_step_drops_and_evaluation_never_does(kind, dev, monkeypatch):
    from fumi_amd import engine as eng_mod
    from fumi_amd import hip
    eng = eng_mod.get_engine()
    seen = {}

    def record(name):
        fn = getattr(eng, name)

        def wrapped(*a, **kw):
            out = fn(*a, **kw)
            seen.setdefault(name, []).append(tuple(t.clone() for t in out))
            return out
        monkeypatch.setattr(eng, name, wrapped)
    record("resnet12_encode"); record("resnet12_encode_drop")
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(16, 3, SIZE, SIZE, generator=g).to(dev), torch.randint(0, 6, (16,), generator=g).to(dev)
    ep = _episodes(5, dev)
    feats, evals = {}, {}
    for drop in (False, True):
        model = _build(kind, dev, drop)
        seen.clear()
        model.drop_step = 4
        loss, acc = model.evaluate((x, y) if kind == "pretrain" else ep, None, None, dev, task="train")
        assert np.isfinite(float(loss)) and 0.0 <= float(acc) <= 1.0
        assert all(bool(torch.isfinite(p.grad).all()) for p in model.conv.theta())
        used = "resnet12_encode_drop" if drop else "resnet12_encode"
        assert list(seen) == [used] and len(seen[used]) == 1, list(seen)
        feats[drop] = seen[used][0]
        seen.clear()
        evals[drop] = (model.few_shot(ep, dev).clone(), np.asarray(model.evaluate(ep, None, None, dev, task="test")))
        assert list(seen) == ["resnet12_encode"], list(seen)               # validation / test / few_shot: never the drop entries
        assert hip.Workspace.get(dev).read_status() == 0 and hip.Workspace.get(dev, "encoder").read_status() == 0
    assert not torch.equal(feats[False][0], feats[True][0]) and not torch.equal(feats[False][1], feats[True][1])
    assert torch.equal(evals[False][0], evals[True][0]) and np.array_equal(evals[False][1], evals[True][1])
