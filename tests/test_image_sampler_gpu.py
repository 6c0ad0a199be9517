"""GPU suite of the resident uint8 image path: fumi_hip_gather_images (csrc/imgather.hip) against its numpy restatement
(tests/image_gather_ref.py), the pixel-table form of GpuEpisodeSampler, and the two datasets from the command line.

Jitter off: the float32 restatement is the kernel's result bit for bit (no FMA contraction, one rounding per operation).
Jitter on: the kernel's only freedom is the order of the gray-mean sum.  The yardstick is the float32 restatement's own largest
distance from the float64 one on the same inputs; the kernel must be within 4 x that distance of the float64 restatement, and
never worse than 1e-5 * max(inv_std).  The tests print both figures; DESIGN.md section 19 records them.
"""
import numpy as np
import pytest
import torch

import image_gather_ref as IR
from oracle import sampler_ref as SR

pytestmark = pytest.mark.gpu

# C, H, W, pad, flip, n_idx
EXACT_CASES = [(3, 12, 12, 0, False, 5),       # plain gather + normalise; image size is a multiple of 16 bytes
               (3, 12, 12, 2, True, 37),       # crop + flip; repeated indices
               (1, 11, 7, 3, True, 9),         # scalar form (77-byte images, odd row width); one channel
               (8, 4, 4, 4, True, 6),          # pad >= image size: windows that are mostly padding; eight channels
               (3, 84, 84, 8, True, 7)]        # the production shape
N_IMAGES = 11


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
    t[0, :, 0, 0], t[n - 1, :, H - 1, W - 1] = 0, 255            # both ends of the byte range in every channel
    return t


def _idx(n_idx, n=N_IMAGES, seed=5):
    idx = np.random.RandomState(seed).randint(0, n, n_idx)
    idx[0], idx[-1] = 0, n - 1                                    # first and last image of the table
    if n_idx > n:
        assert len(set(idx.tolist())) < n_idx                     # repeated indices
    return idx


@pytest.mark.parametrize("C,H,W,pad,flip,n_idx", EXACT_CASES)
def test_gather_is_the_float32_restatement_bit_for_bit(C, H, W, pad, flip, n_idx, dev, ws):
    from fumi_amd import hip
    table, idx, (mean, std) = _table(C, H, W), _idx(n_idx), _norm(C)
    t_d, i_d = torch.from_numpy(table).to(dev), torch.from_numpy(idx).to(dev)
    kw = dict(seed=77, step=3, pad=pad, flip=flip)
    run = lambda **over: hip.gather_images(ws, t_d, i_d, mean, std, **{**kw, "stream_id": 0, **over})
    ref = lambda **over: torch.from_numpy(IR.gather_images(table, idx, mean, std, **{**kw, "stream_id": 0, **over}))
    out = run()
    assert out.shape == (n_idx, C, H, W) and out.dtype == torch.float32
    assert torch.equal(out.cpu(), ref())
    assert torch.equal(run(), out)                                                   # two calls: equal bits
    for over in (dict(stream_id=1), dict(step=4)):
        other = run(**over)
        assert torch.equal(other.cpu(), ref(**over))
        if pad > 0 or flip:
            assert not torch.equal(other, out)                                       # another stream / step: other draws
        else:
            assert torch.equal(other, out)                                           # nothing is drawn without augmentation
    assert torch.equal(run(jitter=0), out) and torch.equal(run(jitter=(0, 0, 0)), out)
    assert ws.read_status() == 0
    if n_idx == 37:                                                                  # the draws behind the 37 images
        d = [IR.draws(77, 3, 0, i, pad, flip) for i in range(n_idx)]
        assert {f for _, _, f in d} == {0, 1} and len({(ox, oy) for ox, oy, _ in d}) >= 3


@pytest.mark.parametrize("H,pad,n_idx", [(12, 2, 37), (84, 8, 7)])
def test_jitter_within_the_float32_restatements_own_error(H, pad, n_idx, dev, ws):
    from fumi_amd import hip
    table, idx, (mean, std) = _table(3, H, H), _idx(n_idx), _norm(3)
    t_d, i_d = torch.from_numpy(table).to(dev), torch.from_numpy(idx).to(dev)
    inv_max = float((np.float32(1) / np.asarray(std, np.float32)).max())
    kw = dict(seed=21, step=6, stream_id=1, pad=pad, flip=True)
    plain = hip.gather_images(ws, t_d, i_d, mean, std, **kw)
    outs = {}
    for jit in ((0.4, 0.4, 0.4), (0.4, 0, 0), (0, 0.4, 0), (0, 0, 0.4)):              # all three, then each step alone
        out = hip.gather_images(ws, t_d, i_d, mean, std, jitter=jit, **kw)
        assert torch.equal(hip.gather_images(ws, t_d, i_d, mean, std, jitter=jit, **kw), out)          # fixed-order gray mean
        assert not torch.equal(out, plain)
        r64 = IR.gather_images(table, idx, mean, std, jitter=jit, dtype=np.float64, **kw)
        r32 = IR.gather_images(table, idx, mean, std, jitter=jit, dtype=np.float32, **kw)
        yard = float(np.abs(r32.astype(np.float64) - r64).max())
        err = float(np.abs(out.cpu().numpy().astype(np.float64) - r64).max())
        print(f"jitter {jit} 3x{H}x{H} pad {pad} n {n_idx}: kernel vs float64 {err:.3e}, float32 restatement vs float64 {yard:.3e}")
        assert yard > 0
        assert err <= 4 * yard, (jit, err, yard)
        assert err <= 1e-5 * inv_max, (jit, err)
        outs[jit] = out
    assert len({o.cpu().numpy().tobytes() for o in outs.values()}) == 4
    assert torch.equal(hip.gather_images(ws, t_d, i_d, mean, std, jitter=0.4, **kw), outs[(0.4, 0.4, 0.4)])     # one amplitude for all
    assert ws.read_status() == 0


def test_status_bit_and_refusals(dev, ws):
    from fumi_amd import hip
    table, (mean, std) = _table(3, 12, 12), _norm(3)
    t_d = torch.from_numpy(table).to(dev)
    dv = lambda v: torch.tensor(v, device=dev, dtype=torch.int64)
    assert ws.read_status() == 0
    want = hip.gather_images(ws, t_d, dv([0, 0]), mean, std, seed=1, step=2, pad=2, flip=True)
    assert ws.read_status() == 0
    for bad in (N_IMAGES, -1):                                        # flagged, read as image 0, no fault
        out = hip.gather_images(ws, t_d, dv([0, bad]), mean, std, seed=1, step=2, pad=2, flip=True)
        st = ws.read_status()
        assert st & hip.ST_LABEL_RANGE
        with pytest.raises(IndexError):
            hip.raise_on_status(st)
        assert torch.equal(out, want)
    assert ws.read_status() == 0
    one = torch.from_numpy(_table(1, 11, 7)).to(dev)
    with pytest.raises(hip.FumiHipError, match=r"\(-4\)"):                 # FUMI_ENOTSUP: the jitter is a colour transform
        hip.gather_images(ws, one, dv([0]), (0.5,), (0.2,), jitter=0.4)
    for jit in (-0.1, 1.5):
        with pytest.raises(hip.FumiHipError, match=r"\(-1\)"):             # FUMI_EINVAL
            hip.gather_images(ws, t_d, dv([0]), mean, std, jitter=jit)
    with pytest.raises(hip.FumiHipError, match=r"\(-1\)"):
        hip.gather_images(ws, t_d, dv([0]), mean, std, pad=65)
    with pytest.raises(hip.FumiHipError):                             # a float table
        hip.gather_images(ws, t_d.float(), dv([0]), mean, std)
    with pytest.raises(hip.FumiHipError):                             # not [n, C, H, W]
        hip.gather_images(ws, t_d.view(N_IMAGES, -1), dv([0]), mean, std)
    assert hip.gather_images(ws, t_d, dv([]), mean, std).shape == (0, 3, 12, 12)
    assert ws.read_status() == 0


# ---- the sampler over a pixel table -------------------------------------------------------------------------------------------------
def test_sampler_over_a_pixel_table(dev, ws):
    from fumi_amd import hip
    from fumi_amd.dataset.gpu_sampler import GpuEpisodeSampler
    rs = np.random.RandomState(8)
    n_cls, per, C, H, W, Dt = 6, 9, 3, 12, 12, 5
    N, K, Q, B = 3, 2, 3, 4
    table = rs.randint(0, 256, (n_cls * per, C, H, W)).astype(np.uint8)
    coi = np.repeat(np.arange(n_cls), per); rs.shuffle(coi)
    text = torch.from_numpy(rs.standard_normal((n_cls, Dt)).astype(np.float32))
    norm = _norm(C)
    mk = lambda aug: GpuEpisodeSampler(torch.from_numpy(table), coi, text, N, K, Q, B, seed=31, normalize=norm, augment=aug)
    plain, crop, full = mk(None), mk(dict(pad=2, flip=True)), mk(dict(pad=2, flip=True, jitter=(0.4, 0.4, 0.4)))
    assert plain.images.dtype == torch.uint8 and plain.images.is_cuda
    for step in (0, 5):
        cls, it_s, it_q = SR.sample_episodes(31, step, B, N, K, Q, plain.class_ptr_host, plain.class_items_host)
        for smp, aug in ((plain, {}), (crop, dict(pad=2, flip=True))):
            b = smp.batch(step)
            (id_s, text_s, x_s), y_s = b['train']
            (id_q, text_q, x_q), y_q = b['test']
            assert x_s.shape == (B, N * K, C, H, W) and x_q.shape == (B, N * Q, C, H, W)
            assert x_s.dtype == torch.float32 and x_q.dtype == torch.float32 and x_s.is_contiguous() and x_q.is_contiguous()
            assert id_s.shape == (B, N * K) and id_s.dtype == torch.int64 and y_s.shape == (B, N * K) and y_q.shape == (B, N * Q)
            assert text_s.shape == (B, N * K, Dt) and text_q.shape == (B, N * Q, Dt)
            assert np.array_equal(id_s.cpu().numpy(), it_s.reshape(B, N * K)) and np.array_equal(id_q.cpu().numpy(), it_q.reshape(B, N * Q))
            assert torch.equal(text_s.cpu(), text[torch.from_numpy(coi)[id_s.cpu()]])
            r_s = IR.gather_images(table, it_s, *norm, seed=31, step=step, stream_id=0, **aug).reshape(x_s.shape)
            r_q = IR.gather_images(table, it_q, *norm, seed=31, step=step, stream_id=1, **aug).reshape(x_q.shape)
            assert torch.equal(x_s.cpu(), torch.from_numpy(r_s)) and torch.equal(x_q.cpu(), torch.from_numpy(r_q))
        aug = dict(pad=2, flip=True, jitter=(0.4, 0.4, 0.4))
        x_s = full.batch(step)['train'][0][2]
        r64 = IR.gather_images(table, it_s, *norm, seed=31, step=step, stream_id=0, dtype=np.float64, **aug).reshape(x_s.shape)
        r32 = IR.gather_images(table, it_s, *norm, seed=31, step=step, stream_id=0, **aug).reshape(x_s.shape)
        assert np.abs(x_s.cpu().numpy() - r64).max() <= 4 * np.abs(r32 - r64).max()
    assert ws.read_status() == 0
    with pytest.raises(ValueError):
        GpuEpisodeSampler(torch.from_numpy(table), coi, text, N, K, Q, B, zero_copy=True)
    with pytest.raises(ValueError):
        GpuEpisodeSampler(torch.from_numpy(table).float(), coi, text, N, K, Q, B)
    # a 2-d fp32 table is what it was: rows of hip.gather_rows
    emb = torch.from_numpy(rs.standard_normal((n_cls * per, 40)).astype(np.float32))
    smp = GpuEpisodeSampler(emb, coi, text, N, K, Q, B, seed=31)
    b = smp.batch(2)
    (id_s, _, x_s), _ = b['train']
    (id_q, _, x_q), _ = b['test']
    assert torch.equal(x_s, hip.gather_rows(ws, smp.images, id_s.view(-1)).view(B, N * K, 40))
    assert torch.equal(x_q, hip.gather_rows(ws, smp.images, id_q.view(-1)).view(B, N * Q, 40))
    assert torch.equal(x_s.cpu(), emb[id_s.cpu()])
    with pytest.raises(ValueError):
        GpuEpisodeSampler(emb, coi, text, N, K, Q, B, augment=dict(pad=2))


def _cli_args(extra):
    from fumi_amd import main as cli
    return cli.parse_args(["--im_encoder", "conv4", "--image_size", "16", "--num_ways", "3", "--num_shots", "1", "--num_shots_test", "2",
                           "--batch_size", "2", "--epochs", "3", "--eval_freq", "1", "--num_ep_test", "4", "--num_train_adapt_steps", "1",
                           "--num_test_adapt_steps", "1", "--dropout", "0", "--synthetic_classes", "10", "--wandb_offline"] + extra)


def test_augment_changes_the_train_batches_only(dev):
    from fumi_amd.dataset.synthetic import get_synthetic_resident
    a0 = _cli_args(["--model", "maml", "--dataset", "synthetic-resident"])
    a1 = _cli_args(["--model", "maml", "--dataset", "synthetic-resident", "--augment"])
    tr0, va0, te0, _ = get_synthetic_resident(a0)
    tr1, va1, te1, _ = get_synthetic_resident(a1)
    assert tr0.images.dtype == torch.uint8 and tuple(tr0.images.shape[1:]) == (3, 16, 16)
    assert tr0.augment == dict(pad=0, flip=False, jitter=(0, 0, 0)) and tr1.augment == dict(pad=8, flip=True, jitter=(0.4, 0.4, 0.4))
    assert va1.augment == va0.augment and te1.augment == te0.augment == tr0.augment
    for step in (0, 3):
        for l0, l1, same in ((tr0, tr1, False), (va0, va1, True), (te0, te1, True)):
            b0, b1 = l0.batch(step), l1.batch(step)
            for part in ("train", "test"):
                assert torch.equal(b0[part][0][0], b1[part][0][0]) and torch.equal(b0[part][1], b1[part][1])       # same episodes
                assert torch.equal(b0[part][0][2], b1[part][0][2]) == same
    x = tr0.batch(0)['train'][0][2]                               # normalised with the train table's own statistics
    assert abs(float(x.mean())) < 0.5 and 0.5 < float(x.std()) < 2.0


# ---- command line, end to end -------------------------------------------------------------------------------------------------------
def test_cli_synthetic_resident_images_with_augment(dev, tmp_path, monkeypatch, capsys):
    from fumi_amd import main as cli
    monkeypatch.chdir(tmp_path)
    args = _cli_args(["--model", "maml", "--dataset", "synthetic-resident", "--augment", "--log_dir", str(tmp_path / "res")])
    res = cli.main(args)
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    assert "--augment is ignored" not in capsys.readouterr().out
    runs = list((tmp_path / "res" / "runs").iterdir())
    assert runs and (runs[0] / "ckpt.pth.tar").exists()


def test_cli_image_npy_dataset(dev, tmp_path, monkeypatch):
    from fumi_amd import main as cli
    monkeypatch.chdir(tmp_path)
    rs = np.random.RandomState(3)
    data = tmp_path / "data"
    data.mkdir()
    n_cls, per, Dt = 6, 36, 16                                    # evaluation episodes take 1 + 100 // 3 images per class
    for split in ("train", "val", "test"):
        proto = rs.randint(40, 216, (n_cls, 16, 16, 3))
        labels = np.repeat(np.arange(n_cls), per)
        images = np.clip(proto[labels] + rs.randint(-40, 41, (n_cls * per, 16, 16, 3)), 0, 255).astype(np.uint8)     # [n, H, W, C]
        np.save(data / f"{split}_images.npy", images)
        np.save(data / f"{split}_labels.npy", labels)
        np.save(data / f"{split}_class_text.npy", rs.standard_normal((n_cls, Dt)).astype(np.float32))
    args = _cli_args(["--model", "fumi", "--dataset", "image-npy", "--data_dir", str(data), "--text_encoder", "BERT", "--text_emb_dim",
                      str(Dt), "--augment", "--log_dir", str(tmp_path / "res")])
    res = cli.main(args)
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    runs = list((tmp_path / "res" / "runs").iterdir())
    assert runs and (runs[0] / "ckpt.pth.tar").exists()
