"""Supervised mini-batches over a GPU-resident uint8 pixel table (``--model pretrain``).

The few-shot recipes train the backbone first as a plain classifier over all training classes.  ``SupervisedPixelBatches`` serves
that step from the table the episodic samplers use (fumi_amd/dataset/gpu_sampler.py): the image indices of a batch are a slice of a
permutation of the table drawn per epoch from (seed, epoch) -- every image once per epoch, the short tail of an epoch dropped -- and
the pixels go through ``hip.gather_images`` / ``hip.gather_images_resized`` with the arguments ``GpuEpisodeSampler`` gives them
(``seed``, ``step``, ``stream_id`` 0), so normalisation, resizing and ``--augment`` are the same kernels with the same draws.

    batch(step) -> (x fp32 [M, C, H, W], y int64 [M])      y = the class id of the train table, dense 0..n_classes-1

The permutation schedule (``epoch_permutation`` / ``batch_indices``) is host code and runs without a GPU."""
import numpy as np
import torch


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


class SupervisedPixelBatches:
    pixels = True                    # (what main.py asks a train loader before it reports --augment as ignored)

    def __init__(self, images_u8, labels, batch, seed=123, normalize=None, augment=None, out_size=None, resize=None, length=None):
        """images_u8 uint8 [n, C, H, W] (moved to the device once), labels [n] ints in [0, n_classes); normalize / augment / out_size /
        resize as ``GpuEpisodeSampler`` takes them for a pixel table.  length: batches an iteration yields (None: endless)."""
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

    def batch(self, step):
        from .. import hip
        idx = self.indices(step)
        if self.out_size is None:
            x = hip.gather_images(self.ws, self.images, idx, self.mean, self.std, seed=self.seed, step=step, stream_id=0, **self.augment)
        else:
            x = hip.gather_images_resized(self.ws, self.images, idx, self.mean, self.std, self.out_size, seed=self.seed, step=step,
                                          stream_id=0, flip=self.augment["flip"], jitter=self.augment["jitter"], **self.resize)
        return x, self.labels[idx]

    def __iter__(self):
        i = 0
        while self.length is None or i < self.length:
            yield self.batch(i)
            i += 1
