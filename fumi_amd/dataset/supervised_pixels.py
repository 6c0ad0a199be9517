"""Supervised mini-batches over a GPU-resident uint8 pixel table (``--model pretrain``).

The few-shot recipes train the backbone first as a plain classifier over all training classes.  ``SupervisedPixelBatches`` serves
that step from the table the episodic samplers use (fumi_amd/dataset/gpu_sampler.py): the image indices of a batch are a slice of a
permutation of the table drawn per epoch from (seed, epoch) -- every image once per epoch, the short tail of an epoch dropped -- and
the pixels go through ``hip.gather_images`` / ``hip.gather_images_resized`` with the arguments ``GpuEpisodeSampler`` gives them
(``seed``, ``step``, ``stream_id`` 0), so normalisation, resizing and ``--augment`` are the same kernels with the same draws.

    batch(step) -> (x fp32 [M, C, H, W], y int64 [M])      y = the class id of the train table, dense 0..n_classes-1

With ``mix=dict(mixup_alpha=, cutmix_alpha=, prob=)`` (``--mixup_alpha`` / ``--cutmix_alpha`` / ``--mix_prob``) the
gathered batch is blended with a permutation of itself by ``hip.mix_images`` under the draw ``mix_draw`` makes for the step:

    batch(step) -> (x_mixed, y_a, y_b = y_a[partner], lam)      a step that draws "no mixing": the unmixed x, y_b = y_a, lam = 1

The permutation schedule (``epoch_permutation`` / ``batch_indices``) and ``mix_draw`` are host code and run without a GPU."""
import math

import numpy as np
import torch

MIXUP, CUTMIX = 0, 1


def epoch_permutation(n, seed, epoch):
    """The order of the n table rows in epoch ``epoch``: torch.randperm from a generator seeded with (seed, epoch)."""
    g = torch.Generator()
    g.manual_seed((int(seed) * 1000003 + int(epoch)) % (2 ** 63 - 1))
    return torch.randperm(int(n), generator=g)


def batch_indices(n, batch, seed, step):
    """int64 [batch]: the table rows of batch ``step``.  An epoch is n // batch whole batches (the short tail is dropped); batch k of
    epoch e is slice k of ``epoch_permutation(n, seed, e)``: reproducible from (seed, step)."""
    n, batch, step = int(n), int(batch), int(step)
    per_epoch = n // batch
    if per_epoch < 1:
        raise ValueError(f"a batch of {batch} images needs a table of at least that many, got {n}")
    epoch, k = divmod(step, per_epoch)
    return epoch_permutation(n, seed, epoch)[k * batch:(k + 1) * batch]


def _mix_key(seed, step):
    """Seed words of the mixing stream of (seed, step); the leading word keeps it apart from ``epoch_permutation``'s torch stream and
    from any other numpy stream keyed by the same pair."""
    return [0x6D697875, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF]


def mix_draw(seed, step, M, H, W, mixup_alpha, cutmix_alpha, prob):
    """(mode, lam, box, partner): what batch ``step`` is mixed with, from numpy.random.Generator(PCG64(_mix_key(seed, step))).
      mode     None with probability 1 - prob (and when both alphas are 0), else MIXUP or CUTMIX: the one whose alpha is > 0, one half
               each when both are
      lam      ~ Beta(alpha, alpha) of the chosen mode; for CutMix recomputed from the box as 1 - area / (H W); 1.0 without mixing
      box      (bx0, by0, bx1, by1), CutMix as in its paper: r = sqrt(1 - lam), int(W r) columns by int(H r) rows around a uniform
               centre, clipped to the image; (0, 0, 0, 0) otherwise
      partner  int64 [M], a permutation of range(M) (the identity without mixing)
    The draws are made in this order: mix or not, mode, lam, centre x, centre y, partner."""
    M, H, W = int(M), int(H), int(W)
    rng = np.random.Generator(np.random.PCG64(_mix_key(seed, step)))
    a_mix, a_cut = float(mixup_alpha), float(cutmix_alpha)
    mixes = rng.random() < float(prob)
    if not mixes or (a_mix <= 0 and a_cut <= 0):
        return None, 1.0, (0, 0, 0, 0), np.arange(M, dtype=np.int64)
    if a_mix > 0 and a_cut > 0:
        mode = MIXUP if rng.random() < 0.5 else CUTMIX
    else:
        mode = MIXUP if a_mix > 0 else CUTMIX
    alpha = a_mix if mode == MIXUP else a_cut
    lam = min(1.0, max(0.0, float(rng.beta(alpha, alpha))))
    box = (0, 0, 0, 0)
    if mode == CUTMIX:
        r = math.sqrt(1.0 - lam)
        cut_w, cut_h = int(W * r), int(H * r)
        cx, cy = int(rng.integers(W)), int(rng.integers(H))
        clip = lambda v, hi: min(max(v, 0), hi)
        box = (clip(cx - cut_w // 2, W), clip(cy - cut_h // 2, H), clip(cx + cut_w // 2, W), clip(cy + cut_h // 2, H))
        lam = 1.0 - (box[2] - box[0]) * (box[3] - box[1]) / float(H * W)
    return mode, lam, box, rng.permutation(M).astype(np.int64)


class SupervisedPixelBatches:
    pixels = True                    # (what main.py asks a train loader before it reports --augment as ignored)

    def __init__(self, images_u8, labels, batch, seed=123, normalize=None, augment=None, out_size=None, resize=None, length=None,
                 mix=None):
        """images_u8 uint8 [n, C, H, W] (moved to the device once), labels [n] ints in [0, n_classes); normalize / augment / out_size /
        resize as ``GpuEpisodeSampler`` takes them for a pixel table.  length: batches an iteration yields (None: endless).
        mix: None | dict(mixup_alpha=, cutmix_alpha=, prob=) as ``mix_draw`` takes them."""
        from .. import hip
        if images_u8.dim() != 4 or images_u8.dtype != torch.uint8:
            raise ValueError(f"a pixel table [n_images, C, H, W] must be uint8, got {images_u8.dtype} {tuple(images_u8.shape)}")
        lab = np.asarray(labels, dtype=np.int64)
        if lab.ndim != 1 or len(lab) != images_u8.shape[0] or (len(lab) and lab.min() < 0):
            raise ValueError("labels must hold one class id >= 0 per image row")
        C_img = int(images_u8.shape[1])
        mean, std = normalize if normalize is not None else ((0.0,) * C_img, (1.0,) * C_img)
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        if len(self.mean) != C_img or len(self.std) != C_img or min(self.std) <= 0:
            raise ValueError(f"normalize needs {C_img} means and {C_img} positive standard deviations")
        aug = dict(augment or {})
        self.augment = dict(pad=int(aug.pop("pad", 0)), flip=bool(aug.pop("flip", False)), jitter=aug.pop("jitter", (0, 0, 0)))
        if aug:
            raise ValueError(f"unknown augment keys {sorted(aug)}")
        self.out_size, self.resize = None, None
        if out_size is not None:
            self.out_size = (int(out_size[0]), int(out_size[1]))
            rs = dict(resize or {})
            if "scale" in rs:
                lo, hi = rs.pop("scale")
                self.resize = dict(scale=(float(lo), float(hi)), ratio=float(rs.pop("ratio", 1.0)))
            else:
                self.resize = dict(rect=tuple(int(v) for v in rs.pop("rect", (0, 0, int(images_u8.shape[3]), int(images_u8.shape[2])))))
            if rs:
                raise ValueError(f"unknown resize keys {sorted(rs)}")
            if self.augment["pad"]:
                raise ValueError("augment pad= does not apply with out_size: the random-resized crop takes its place")
        elif resize is not None:
            raise ValueError("resize needs out_size=(Ho, Wo)")
        self.mix = None
        if mix is not None:
            m = dict(mix)
            self.mix = dict(mixup_alpha=float(m.pop("mixup_alpha", 0.0)), cutmix_alpha=float(m.pop("cutmix_alpha", 0.0)),
                            prob=float(m.pop("prob", 1.0)))
            if m:
                raise ValueError(f"unknown mix keys {sorted(m)}")
            if self.mix["mixup_alpha"] < 0 or self.mix["cutmix_alpha"] < 0 or not 0.0 <= self.mix["prob"] <= 1.0:
                raise ValueError("mix needs mixup_alpha >= 0, cutmix_alpha >= 0 and prob in [0, 1]")
        self.M, self.seed, self.length = int(batch), int(seed), length
        self.n = int(images_u8.shape[0])
        if self.n < self.M:
            raise ValueError(f"a batch of {self.M} images needs a table of at least that many, got {self.n}")
        self.n_classes = int(lab.max()) + 1
        self.dev = images_u8.device if images_u8.is_cuda else torch.device("cuda", torch.cuda.current_device())
        self.images = images_u8.to(self.dev).contiguous()
        self.labels = torch.from_numpy(lab).to(self.dev)
        self.ws = hip.Workspace.get(self.dev)
        self._epoch = (-1, None)               # (epoch, its permutation on the device)

    def indices(self, step):
        """Device int64 [M]: ``batch_indices(n, M, seed, step)`` (the epoch's permutation is drawn once and kept on the device)."""
        per_epoch = self.n // self.M
        epoch, k = divmod(int(step), per_epoch)
        if self._epoch[0] != epoch:
            self._epoch = (epoch, epoch_permutation(self.n, self.seed, epoch).to(self.dev))
        return self._epoch[1][k * self.M:(k + 1) * self.M].contiguous()

    def gather(self, step):
        """(x, y) of batch ``step``, unmixed."""
        from .. import hip
        idx = self.indices(step)
        if self.out_size is None:
            x = hip.gather_images(self.ws, self.images, idx, self.mean, self.std, seed=self.seed, step=step, stream_id=0, **self.augment)
        else:
            x = hip.gather_images_resized(self.ws, self.images, idx, self.mean, self.std, self.out_size, seed=self.seed, step=step,
                                          stream_id=0, flip=self.augment["flip"], jitter=self.augment["jitter"], **self.resize)
        return x, self.labels[idx]

    def batch(self, step):
        x, y = self.gather(step)
        if self.mix is None:
            return x, y
        from .. import hip
        mode, lam, box, partner = mix_draw(self.seed, step, self.M, x.shape[2], x.shape[3], **self.mix)
        if mode is None:
            return x, y, y, 1.0
        partner = torch.from_numpy(partner).to(self.dev)
        return hip.mix_images(self.ws, x, partner, mode=mode, lam=lam, box=box), y, y[partner], lam

    def __iter__(self):
        i = 0
        while self.length is None or i < self.length:
            yield self.batch(i)
            i += 1
