"""GPU suite of the resize / random-resized-crop stage: fumi_hip_gather_images_resized (csrc/imresize.hip) against its numpy
restatement (tests/image_resize_ref.py), the ``out_size`` form of GpuEpisodeSampler, and the two datasets from the command line.

Jitter off: the float32 restatement is the kernel's result bit for bit (no FMA contraction, one rounding per operation; dropping a
tap of weight 0 adds +0 to a non-negative sum).  Jitter on: the rule of tests/test_image_sampler_gpu.py -- the kernel's only
freedom is the order of the gray-mean sum; it must be within 4 x the float32 restatement's own largest distance from the float64
one, and never beyond 1e-5 * max(inv_std).  The tests print the figures; profiles/image_resize/jitter_tolerance.txt records them.

Measured on one MI355X (largest distance from the float64 restatement, kernel / float32 restatement, jitter 0.4 all three):
  3 x 24 x 20 -> 12 x 12, random mode, 37 images             2.689e-06 / 2.689e-06
  3 x 96 x 96 -> 84 x 84, 0.875 centre rectangle, 7 images   8.571e-07 / 8.571e-07
"""
import numpy as np
import pytest
import torch

import image_gather_ref as IR
import image_resize_ref as RR
from oracle import sampler_ref as SR

pytestmark = pytest.mark.gpu

N_IMAGES = 11
# C, Hs, Ws, Ho, Wo, rect (x0, y0, w, h), n_idx
FIXED_CASES = [(3, 12, 12, 12, 12, (0, 0, 12, 12), 37),        # whole image, same size: a copy; equals hip.gather_images(pad=0)
               (3, 20, 16, 12, 12, (1, 3, 14, 14), 37),        # centre 14 x 14 of a 20-row, 16-column image
               (3, 8, 8, 12, 12, (0, 0, 8, 8), 37),            # an upscale
               (1, 9, 7, 5, 6, (0, 0, 7, 9), 37),              # scalar form: 63-byte images, non-square output, odd width
               (3, 33, 47, 12, 12, (0, 0, 47, 33), 37),        # eight taps (scalar staging: 4,653-byte images)
               (2, 16, 16, 8, 8, (0, 0, 16, 16), 37),          # an exact factor of two
               (3, 96, 96, 84, 84, (6, 6, 84, 84), 7)]         # the production shape, 0.875 centre rectangle


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ws(dev):
    from fumi_amd import hip
    return hip.Workspace.get(dev)


def _norm(C):
    return tuple(0.3 + 0.05 * c for c in range(C)), tuple(0.2 + 0.03 * c for c in range(C))


def _table(C, H, W, seed=0, n=N_IMAGES):
    t = np.random.RandomState(seed + 131 * C + H).randint(0, 256, (n, C, H, W)).astype(np.uint8)
    t[0, :, 0, 0], t[n - 1, :, H - 1, W - 1] = 0, 255
    return t


def _idx(n_idx, n=N_IMAGES, seed=5):
    idx = np.random.RandomState(seed).randint(0, n, n_idx)
    idx[0], idx[-1], idx[1] = 0, n - 1, idx[2]                   # first and last image of the table; a repeated index
    assert len(set(idx.tolist())) < n_idx
    return idx


@pytest.mark.parametrize("C,Hs,Ws,Ho,Wo,rect,n_idx", FIXED_CASES)
def test_fixed_mode_is_the_float32_restatement_bit_for_bit(C, Hs, Ws, Ho, Wo, rect, n_idx, dev, ws):
    from fumi_amd import hip
    table, idx, (mean, std) = _table(C, Hs, Ws), _idx(n_idx), _norm(C)
    t_d, i_d = torch.from_numpy(table).to(dev), torch.from_numpy(idx).to(dev)
    for flip in (False, True):
        kw = dict(seed=77, step=3, stream_id=0, rect=rect, flip=flip)
        out = hip.gather_images_resized(ws, t_d, i_d, mean, std, (Ho, Wo), **kw)
        assert out.shape == (n_idx, C, Ho, Wo) and out.dtype == torch.float32
        ref = torch.from_numpy(RR.gather_images_resized(table, idx, mean, std, (Ho, Wo), **kw))
        assert torch.equal(out.cpu(), ref)
        assert torch.equal(hip.gather_images_resized(ws, t_d, i_d, mean, std, (Ho, Wo), **kw), out)      # two calls: equal bits
        assert torch.equal(hip.gather_images_resized(ws, t_d, i_d, mean, std, (Ho, Wo), jitter=0, **kw), out)
        if rect == (0, 0, Ws, Hs) and (Ho, Wo) == (Hs, Ws):                    # nothing to resample: the plain gather, same flip draw
            assert torch.equal(out, hip.gather_images(ws, t_d, i_d, mean, std, seed=77, step=3, stream_id=0, pad=0, flip=flip))
    if n_idx == 37:
        assert {IR.draws(77, 3, 0, i, 0, True)[2] for i in range(n_idx)} == {0, 1}
    assert ws.read_status() == 0


def test_random_mode(dev, ws):
    from fumi_amd import hip
    C, Hs, Ws, n_idx = 3, 24, 20, 37
    table, idx, (mean, std) = _table(C, Hs, Ws), _idx(n_idx), _norm(C)
    t_d, i_d = torch.from_numpy(table).to(dev), torch.from_numpy(idx).to(dev)
    kw = dict(scale=(0.08, 1.0), ratio=4.0 / 3.0, flip=True)
    run = lambda **o: hip.gather_images_resized(ws, t_d, i_d, mean, std, (12, 12), **{**dict(seed=9, step=2, stream_id=0), **kw, **o})
    ref = lambda **o: torch.from_numpy(RR.gather_images_resized(table, idx, mean, std, (12, 12), **{**dict(seed=9, step=2, stream_id=0), **kw, **o}))
    out = run()
    assert torch.equal(out.cpu(), ref())                                        # pins the rectangles too
    assert len({RR.random_rect(9, 2, 0, i, Hs, Ws, 0.08, 1.0, 4.0 / 3.0) for i in range(n_idx)}) > 30
    assert torch.equal(run(), out)                                              # same (seed, step): equal
    for over in (dict(step=3), dict(stream_id=1)):                              # another step, the other stream: other draws
        other = run(**over)
        assert torch.equal(other.cpu(), ref(**over)) and not torch.equal(other, out)
    sq = _table(3, 16, 16)
    s_d = torch.from_numpy(sq).to(dev)
    whole = hip.gather_images_resized(ws, s_d, i_d, mean, std, (12, 12), seed=9, step=2, rect=(0, 0, 16, 16))
    assert torch.equal(hip.gather_images_resized(ws, s_d, i_d, mean, std, (12, 12), seed=9, step=2, scale=(1.0, 1.0), ratio=1.0), whole)
    assert ws.read_status() == 0


JITTER_CASES = [(24, 20, 12, dict(scale=(0.08, 1.0), ratio=4.0 / 3.0), 37), (96, 96, 84, dict(rect=(6, 6, 84, 84)), 7)]


@pytest.mark.parametrize("Hs,Ws,Ho,mode,n_idx", JITTER_CASES)
def test_jitter_within_the_float32_restatements_own_error(Hs, Ws, Ho, mode, n_idx, dev, ws):
    from fumi_amd import hip
    table, idx, (mean, std) = _table(3, Hs, Ws), _idx(n_idx), _norm(3)
    t_d, i_d = torch.from_numpy(table).to(dev), torch.from_numpy(idx).to(dev)
    inv_max = float((np.float32(1) / np.asarray(std, np.float32)).max())
    kw = dict(seed=21, step=6, stream_id=1, flip=True, **mode)
    plain = hip.gather_images_resized(ws, t_d, i_d, mean, std, (Ho, Ho), **kw)
    outs = {}
    for jit in ((0.4, 0.4, 0.4), (0.4, 0, 0), (0, 0.4, 0), (0, 0, 0.4)):              # all three, then each step alone
        out = hip.gather_images_resized(ws, t_d, i_d, mean, std, (Ho, Ho), jitter=jit, **kw)
        assert torch.equal(hip.gather_images_resized(ws, t_d, i_d, mean, std, (Ho, Ho), jitter=jit, **kw), out)      # fixed-order gray mean
        assert not torch.equal(out, plain)
        r64 = RR.gather_images_resized(table, idx, mean, std, (Ho, Ho), jitter=jit, dtype=np.float64, **kw)
        r32 = RR.gather_images_resized(table, idx, mean, std, (Ho, Ho), jitter=jit, dtype=np.float32, **kw)
        yard = float(np.abs(r32.astype(np.float64) - r64).max())
        err = float(np.abs(out.cpu().numpy().astype(np.float64) - r64).max())
        print(f"jitter {jit} 3x{Hs}x{Ws} -> {Ho}x{Ho} {sorted(mode)[0]} n {n_idx}: kernel vs float64 {err:.3e}, "
              f"float32 restatement vs float64 {yard:.3e}")
        assert yard > 0
        assert err <= 4 * yard, (jit, err, yard)
        assert err <= 1e-5 * inv_max, (jit, err)
        outs[jit] = out
    assert len({o.cpu().numpy().tobytes() for o in outs.values()}) == 4
    assert ws.read_status() == 0


def test_status_bit_and_refusals(dev, ws):
    from fumi_amd import hip
    table, (mean, std) = _table(3, 20, 16), _norm(3)
    t_d = torch.from_numpy(table).to(dev)
    dv = lambda v: torch.tensor(v, device=dev, dtype=torch.int64)
    g = lambda t, i, m=mean, s=std, size=(12, 12), **kw: hip.gather_images_resized(ws, t, i, m, s, size, **kw)
    assert ws.read_status() == 0
    want = g(t_d, dv([0, 0]), seed=1, step=2, rect=(1, 3, 14, 14), flip=True)
    for bad in (N_IMAGES, -1):                                        # flagged, read as image 0, no fault
        out = g(t_d, dv([0, bad]), seed=1, step=2, rect=(1, 3, 14, 14), flip=True)
        st = ws.read_status()
        assert st & hip.ST_LABEL_RANGE
        assert torch.equal(out, want)
    assert ws.read_status() == 0
    for rect in ((3, 0, 14, 14), (0, 7, 14, 14), (0, 0, 17, 20), (0, 0, 16, 21), (-1, 0, 4, 4), (0, 0, 0, 4)):      # leaves the image
        with pytest.raises(hip.FumiHipError, match=r"\(-1\)"):
            g(t_d, dv([0]), rect=rect)
    for bad in (dict(scale=(0.6, 0.5)), dict(scale=(0.0, 0.5)), dict(scale=(0.5, 1.5)), dict(scale=(0.5, 1.0), ratio=0.9)):
        with pytest.raises(hip.FumiHipError, match=r"\(-1\)"):                 # FUMI_EINVAL
            g(t_d, dv([0]), **bad)
    for jit in (-0.1, 1.5):
        with pytest.raises(hip.FumiHipError, match=r"\(-1\)"):
            g(t_d, dv([0]), rect=(0, 0, 16, 20), jitter=jit)
    one = torch.from_numpy(_table(1, 9, 7)).to(dev)
    with pytest.raises(hip.FumiHipError, match=r"\(-4\)"):                     # FUMI_ENOTSUP: the jitter is a colour transform
        g(one, dv([0]), (0.5,), (0.2,), (5, 6), rect=(0, 0, 7, 9), jitter=0.4)
    big = torch.zeros(1, 3, 256, 256, dtype=torch.uint8, device=dev)          # 3 x 256 x 256 rows: 196,608 bytes > 160 KiB of LDS
    with pytest.raises(hip.FumiHipError, match=r"\(-4\)"):
        g(big, dv([0]), rect=(0, 0, 256, 256))
    with pytest.raises(hip.FumiHipError, match=r"\(-4\)"):
        g(big, dv([0]), scale=(0.5, 1.0), ratio=1.0)                            # random mode stages whole images
    assert g(big, dv([0]), rect=(0, 64, 256, 128)).shape == (1, 3, 12, 12)     # half the rows fit
    with pytest.raises(hip.FumiHipError):
        g(t_d, dv([0]))                                                         # neither rect nor scale
    with pytest.raises(hip.FumiHipError):
        g(t_d.float(), dv([0]), rect=(0, 0, 16, 20))
    assert g(t_d, dv([]), rect=(0, 0, 16, 20)).shape == (0, 3, 12, 12)
    assert ws.read_status() == 0


def test_large_rectangle_at_the_documented_size(dev, ws):
    """3 x 160 x 160 into 3 x 84 x 84 (more than 64 KB of LDS: one workgroup per CU), fixed and random mode."""
    from fumi_amd import hip
    table, (mean, std) = _table(3, 160, 160, n=3), _norm(3)
    idx = np.array([2, 0, 2])
    t_d, i_d = torch.from_numpy(table).to(dev), torch.from_numpy(idx).to(dev)
    for mode in (dict(rect=(0, 0, 160, 160)), dict(scale=(0.5, 1.0), ratio=4.0 / 3.0)):
        out = hip.gather_images_resized(ws, t_d, i_d, mean, std, (84, 84), seed=4, step=1, flip=True, **mode)
        ref = RR.gather_images_resized(table, idx, mean, std, (84, 84), seed=4, step=1, flip=True, **mode)
        assert torch.equal(out.cpu(), torch.from_numpy(ref))
    assert ws.read_status() == 0


# ---- the sampler over a table of another size -----------------------------------------------------------------------------------------
def test_sampler_with_out_size(dev, ws):
    from fumi_amd.dataset.gpu_sampler import GpuEpisodeSampler
    rs = np.random.RandomState(8)
    n_cls, per, C, H, W, Dt = 6, 9, 3, 20, 20, 5
    N, K, Q, B = 3, 2, 3, 4
    table = rs.randint(0, 256, (n_cls * per, C, H, W)).astype(np.uint8)
    coi = np.repeat(np.arange(n_cls), per); rs.shuffle(coi)
    text = torch.from_numpy(rs.standard_normal((n_cls, Dt)).astype(np.float32))
    norm = _norm(C)
    mk = lambda **kw: GpuEpisodeSampler(torch.from_numpy(table), coi, text, N, K, Q, B, seed=31, normalize=norm, out_size=(16, 16), **kw)
    rect = RR.center_rect(H, W, 0.875)
    cases = [(mk(resize=dict(rect=rect)), dict(rect=rect)),
             (mk(), dict(rect=(0, 0, W, H))),
             (mk(resize=dict(scale=(0.08, 1.0), ratio=4.0 / 3.0), augment=dict(flip=True)), dict(scale=(0.08, 1.0), ratio=4.0 / 3.0, flip=True))]
    for step in (0, 5):
        cls, it_s, it_q = SR.sample_episodes(31, step, B, N, K, Q, cases[0][0].class_ptr_host, cases[0][0].class_items_host)
        for smp, kw in cases:
            b = smp.batch(step)
            (id_s, _, x_s), _ = b['train']
            (id_q, _, x_q), _ = b['test']
            assert x_s.shape == (B, N * K, C, 16, 16) and x_q.shape == (B, N * Q, C, 16, 16) and x_s.is_contiguous()
            assert np.array_equal(id_s.cpu().numpy(), it_s.reshape(B, N * K)) and np.array_equal(id_q.cpu().numpy(), it_q.reshape(B, N * Q))
            r_s = RR.gather_images_resized(table, it_s, *norm, (16, 16), seed=31, step=step, stream_id=0, **kw).reshape(x_s.shape)
            r_q = RR.gather_images_resized(table, it_q, *norm, (16, 16), seed=31, step=step, stream_id=1, **kw).reshape(x_q.shape)
            assert torch.equal(x_s.cpu(), torch.from_numpy(r_s)) and torch.equal(x_q.cpu(), torch.from_numpy(r_q))
    assert ws.read_status() == 0
    with pytest.raises(ValueError):
        mk(augment=dict(pad=2))
    with pytest.raises(ValueError):
        mk(resize=dict(rectangle=(0, 0, 4, 4)))
    with pytest.raises(ValueError):
        GpuEpisodeSampler(torch.from_numpy(table), coi, text, N, K, Q, B, resize=dict(rect=rect))


def _cli_args(extra):
    from fumi_amd import main as cli
    return cli.parse_args(["--im_encoder", "conv4", "--image_size", "16", "--num_ways", "3", "--num_shots", "1", "--num_shots_test", "2",
                           "--batch_size", "2", "--epochs", "2", "--eval_freq", "1", "--num_ep_test", "4", "--num_train_adapt_steps", "1",
                           "--num_test_adapt_steps", "1", "--dropout", "0", "--synthetic_classes", "10", "--wandb_offline"] + extra)


def test_augment_changes_the_train_batches_only(dev):
    from fumi_amd.dataset.synthetic import get_synthetic_resident
    base = ["--model", "maml", "--dataset", "synthetic-resident", "--synthetic_table_size", "20"]
    tr0, va0, te0, _ = get_synthetic_resident(_cli_args(base))
    tr1, va1, te1, _ = get_synthetic_resident(_cli_args(base + ["--augment"]))
    assert tr0.images.dtype == torch.uint8 and tuple(tr0.images.shape[1:]) == (3, 20, 20)
    rect = dict(rect=RR.center_rect(20, 20, 0.875))
    assert tr0.out_size == (16, 16) and tr0.resize == rect and va1.resize == rect and te1.resize == rect
    assert tr1.resize == dict(scale=(0.08, 1.0), ratio=4.0 / 3.0) and tr1.augment == dict(pad=0, flip=True, jitter=(0.4, 0.4, 0.4))
    for step in (0, 3):
        for l0, l1, same in ((tr0, tr1, False), (va0, va1, True), (te0, te1, True)):
            b0, b1 = l0.batch(step), l1.batch(step)
            for part in ("train", "test"):
                assert b0[part][0][2].shape[2:] == (3, 16, 16)
                assert torch.equal(b0[part][0][0], b1[part][0][0]) and torch.equal(b0[part][1], b1[part][1])       # same episodes
                assert torch.equal(b0[part][0][2], b1[part][0][2]) == same
    x = tr0.batch(0)['train'][0][2]                               # normalised with the train table's statistics as stored
    assert abs(float(x.mean())) < 0.5 and 0.3 < float(x.std()) < 2.0


# ---- command line, end to end -------------------------------------------------------------------------------------------------------
def test_cli_synthetic_resident_with_a_larger_table(dev, tmp_path, monkeypatch, capsys):
    from fumi_amd import main as cli
    monkeypatch.chdir(tmp_path)
    args = _cli_args(["--model", "maml", "--dataset", "synthetic-resident", "--synthetic_table_size", "20", "--augment",
                      "--log_dir", str(tmp_path / "res")])
    res = cli.main(args)
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    out = capsys.readouterr().out
    assert "--augment is ignored" not in out and out.count("--augment_pad is not used") == 1


@pytest.mark.parametrize("augment", [False, True])
def test_cli_image_npy_stored_at_another_size(augment, dev, tmp_path, monkeypatch):
    from fumi_amd import main as cli
    monkeypatch.chdir(tmp_path)
    rs = np.random.RandomState(3)
    data = tmp_path / "data"
    data.mkdir()
    n_cls, per, Dt = 6, 36, 16                                    # evaluation episodes take 1 + 100 // 3 images per class
    for split in ("train", "val", "test"):
        proto = rs.randint(40, 216, (n_cls, 20, 20, 3))
        labels = np.repeat(np.arange(n_cls), per)
        images = np.clip(proto[labels] + rs.randint(-40, 41, (n_cls * per, 20, 20, 3)), 0, 255).astype(np.uint8)     # [n, H, W, C]
        np.save(data / f"{split}_images.npy", images)
        np.save(data / f"{split}_labels.npy", labels)
        np.save(data / f"{split}_class_text.npy", rs.standard_normal((n_cls, Dt)).astype(np.float32))
    args = _cli_args(["--model", "fumi", "--dataset", "image-npy", "--data_dir", str(data), "--text_encoder", "BERT", "--text_emb_dim",
                      str(Dt), "--log_dir", str(tmp_path / "res")] + (["--augment"] if augment else []))
    res = cli.main(args)
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
