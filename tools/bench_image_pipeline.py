"""Dev tool (GPU box): where a Conv4 / ResNet-12 meta-step's images come from, and what that costs.

Times the FuMI Conv4 meta-step at the as-worded shape (5-way 5-shot, Q = 32, B = 32, 3 x 84 x 84) fed four ways:
  (a) pre-generated fp32 batches resident in HBM (what bench.py times);
  (b) the host loader of ``--dataset synthetic`` (numpy draws the fp32 batch, then a host-to-device copy);
  (c) the GPU-resident uint8 pixel table, sampled and gathered on the device (csrc/imgather.hip), no augmentation;
  (d) the same with the ``--augment`` defaults (pad 8, flip, jitter 0.4);
  (e) a 3 x 96 x 96 uint8 table resampled on the device (csrc/imresize.hip): the 0.875 centre rectangle resized to 84 x 84;
  (f) the same with ``--augment``: random-resized crop (area 0.08 - 1, ratio up to 4/3), flip, jitter 0.4;
and the sampler alone per meta-batch.  The variants alternate inside one process; a figure is the median of the regions with
its min / max.  ``--resnet12`` adds the sampler alone at the ResNet-12 20-way shape (B = 64, 400 images per episode).

    python tools/bench_image_pipeline.py [--regions 5] [--steps 6] [--host-steps 2] [--resnet12]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o img -- python tools/bench_image_pipeline.py --profile

``--profile`` launches only what the trace is read for: the two gather_images calls of a meta-batch (with and without
augmentation), the two gather_images_resized calls of rows (e) and (f) and, as the yardstick, fumi_hip_gather_rows over the same
number of 8 KB fp32 rows.  Effective bandwidth of the image gather = n_idx * C*H*W * 5 bytes (1 read as uint8, 4 written as fp32)
over the kernel's average duration; of the resized gather = n_idx * (C*h*w + 4*C*Ho*Wo) with h x w the rectangle (row (f): the mean
rectangle area of the draws, printed); of the row gather = n_idx * row_bytes * 2."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fumi_amd import hip  # noqa: E402
from fumi_amd.dataset.gpu_sampler import GpuEpisodeSampler  # noqa: E402
from fumi_amd.dataset.synthetic import SyntheticEpisodes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--regions", type=int, default=5)
ap.add_argument("--steps", type=int, default=6, help="meta-steps per timed region (resident variants)")
ap.add_argument("--host-steps", type=int, default=2, help="meta-steps per timed region of the host loader")
ap.add_argument("--resnet12", action="store_true")
ap.add_argument("--profile", action="store_true")
opt = ap.parse_args()

N, K, Q, B, Cin, H, W, nblk, Dt, Ht, T = 5, 5, 32, 32, 3, 84, 84, 4, 300, 256, 1
S, Qn = N * K, N * Q
AUG = dict(pad=8, flip=True, jitter=(0.4, 0.4, 0.4))
NORM = ((0.5,) * Cin, (0.25,) * Cin)
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
ws = hip.Workspace.get(dev)
g = torch.Generator(device=dev).manual_seed(0)
n_cls, per = 256, 64                                   # 16,384 images = 347 MB of uint8: larger than the 256 MB Infinity Cache
table = torch.randint(0, 256, (n_cls * per, Cin, H, W), device=dev, generator=g, dtype=torch.uint8)
coi = np.repeat(np.arange(n_cls), per)
text = torch.randn(n_cls, Dt, device=dev, generator=g)
HS = 96                                                 # rows (e), (f): the table as stored, 16,384 x 3 x 96 x 96 = 453 MB
table96 = torch.randint(0, 256, (n_cls * per, Cin, HS, HS), device=dev, generator=g, dtype=torch.uint8)
side = max(1, min(HS, int(round(0.875 * HS))))
RECT = ((HS - side) // 2, (HS - side) // 2, side, side)
RRC = dict(scale=(0.08, 1.0), ratio=4.0 / 3.0)
sync = torch.cuda.synchronize


def sampler(aug, b=B, n=N, k=K, q=Q):
    return GpuEpisodeSampler(table, coi, text, n, k, q, b, seed=1, normalize=NORM, augment=aug)


def sampler96(resize, aug, b=B, n=N, k=K, q=Q):
    return GpuEpisodeSampler(table96, coi, text, n, k, q, b, seed=1, normalize=NORM, out_size=(H, W), resize=resize, augment=aug)


if opt.profile:
    n_idx = B * (S + Qn)
    it = torch.randint(0, n_cls * per, (n_idx,), device=dev, generator=g)
    rows = torch.randn(65536, 2048, device=dev, generator=g)                  # 512 MB of 8 KB rows
    it_r = torch.randint(0, 65536, (n_idx,), device=dev, generator=g)
    for i in range(30):
        hip.gather_images(ws, table, it, *NORM, seed=1, step=i, stream_id=0)
        hip.gather_images(ws, table, it, *NORM, seed=1, step=i, stream_id=0, **AUG)
        hip.gather_rows(ws, rows, it_r)
        hip.gather_images_resized(ws, table96, it, *NORM, (H, W), seed=1, step=i, stream_id=0, rect=RECT)
        hip.gather_images_resized(ws, table96, it, *NORM, (H, W), seed=1, step=i, stream_id=0, flip=True, jitter=AUG["jitter"], **RRC)
    sync()
    area = 0.5 * (RRC["scale"][0] + RRC["scale"][1]) * HS * HS              # mean rectangle area of the draws (before clamping)
    print(json.dumps(dict(profile=True, n_idx=n_idx, image_bytes=Cin * H * W, image_gather_bytes=n_idx * Cin * H * W * 5,
                          row_gather_bytes=n_idx * 2048 * 4 * 2,
                          resized_fixed_bytes=n_idx * (Cin * RECT[2] * RECT[3] + 4 * Cin * H * W),
                          resized_random_bytes=int(n_idx * (Cin * area + 4 * Cin * H * W)))))
    sys.exit(0)

F = hip.conv4_feature_dim(nblk, H, W)
theta = []
for l in range(nblk):
    ci = Cin if l == 0 else 64
    theta += [(torch.rand(64, ci, 3, 3, device=dev, generator=g) * 2 - 1) / (ci * 9) ** 0.5, torch.ones(64, device=dev),
              torch.zeros(64, device=dev)]
phi = [(torch.rand(Ht, Dt, device=dev, generator=g) * 2 - 1) / Dt ** 0.5, torch.zeros(Ht, device=dev),
       (torch.rand(F + 1, Ht, device=dev, generator=g) * 2 - 1) / Ht ** 0.5, torch.zeros(F + 1, device=dev)]
g_theta, g_phi = [torch.empty_like(t) for t in theta], [torch.empty_like(t) for t in phi]


def step(batch):
    (_, text_s, x_s), y_s = batch['train']
    (_, _, x_q), y_q = batch['test']
    d = lambda t: t.to(dev, non_blocking=False)
    return hip.fumi_conv4_step(ws, N, d(x_s).contiguous(), d(y_s), d(x_q).contiguous(), d(y_q), theta, phi, T, 0.01, False,
                               text_s=d(text_s).contiguous(), g_theta=g_theta, g_phi=g_phi)


smp_c, smp_d = sampler(None), sampler(AUG)
smp_e, smp_f = sampler96(dict(rect=RECT), None), sampler96(RRC, dict(flip=True, jitter=AUG["jitter"]))
fixed = [smp_c.batch(i) for i in range(2)]                                  # (a): two resident fp32 batches, 1 GB
host = SyntheticEpisodes(64, 0, Dt, N, K, Q, B, 1, "train", image_shape=(Cin, H, W))
variants = [("a: resident pre-generated fp32 batches", lambda i: fixed[i % 2], opt.steps),
            ("b: host loader (--dataset synthetic)", host.batch, opt.host_steps),
            ("c: uint8 resident sampler", smp_c.batch, opt.steps),
            ("d: uint8 resident sampler, --augment", smp_d.batch, opt.steps),
            ("e: 3 x 96 x 96 uint8 table, centre crop + resize", smp_e.batch, opt.steps),
            ("f: 3 x 96 x 96 uint8 table, --augment (random-resized crop)", smp_f.batch, opt.steps)]
alone = [("sampler alone, no augmentation", smp_c.batch), ("sampler alone, --augment", smp_d.batch),
         ("sampler alone, 96 x 96 table, centre crop + resize", smp_e.batch), ("sampler alone, 96 x 96 table, --augment", smp_f.batch)]
if opt.resnet12:
    alone += [("sampler alone, ResNet-12 20-way shape (B 64, 400 images / episode)", sampler(None, 64, 20, 5, 15).batch),
              ("sampler alone, ResNet-12 20-way shape, --augment", sampler(AUG, 64, 20, 5, 15).batch)]

for _, get, _ in variants:                                                  # warm every shape the timed regions use
    step(get(0))
for _, get in alone:
    get(0)
sync()
times = {name: [] for name, _, _ in variants}
times.update({name: [] for name, _ in alone})
for r in range(opt.regions):                                                # the variants alternate inside every region
    for name, get, n in variants:
        sync(); t0 = time.perf_counter()
        for i in range(n):
            step(get(10 + r * n + i))
        sync(); times[name].append((time.perf_counter() - t0) / n * 1e3)
    for name, get in alone:
        sync(); t0 = time.perf_counter()
        for i in range(20):
            get(10 + r * 20 + i)
        sync(); times[name].append((time.perf_counter() - t0) / 20 * 1e3)
hip.raise_on_status(ws.read_status())
res = {}
for name, ts in times.items():
    res[name] = dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))
    print(f"{name:75s} {res[name]['median_ms']:9.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f}, {len(ts)} regions)", flush=True)
print(json.dumps(dict(shape=dict(N=N, K=K, Q=Q, B=B, C=Cin, H=H, W=W, T=T), regions=opt.regions, results=res)))
