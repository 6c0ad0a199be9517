"""Synthetic episodic loader with the reference loader's batch contract (fumi/dataset/data.py:571-581 + torchmeta
collate):

    batch = {'train': ([idx i64 [B,S], text f32 [B,S,Dt] | i64 [B,S,L], im f32 [B,S,D]], targets i64 [B,S]),
             'test' : same with Qn = N * num_shots_test rows}

The iNat-Anim files (Zenodo JSON + HDF5 embeddings, BERT/GloVe downloads) cannot be fetched here, so
``--dataset synthetic`` draws a learnable task instead: class prototypes mu_c ~ N(0, I_D), images x = mu_c + 2 eps,
class text = P mu_c + 0.5 eps with a fixed random P [Dt, D] (the text is identical for all samples of a class, like
data.py:543-549).  Deterministic in (seed, split, batch index); every rank regenerates the SAME meta-batch."""
import numpy as np
import torch


class SyntheticEpisodes:
    def __init__(self, n_classes, D, Dt, N, K, Q, batch_size, seed, split, tokens=None, length=None, image_shape=None):
        """image_shape=(C, H, W): the samples are raw images (--im_encoder conv4) -- the class prototype is a D = C*H*W pattern
        and a sample is prototype + noise, reshaped to [C, H, W]."""
        rs = np.random.RandomState(seed * 7 + {"train": 0, "val": 1, "test": 2}[split])
        self.image_shape = image_shape
        if image_shape is not None:
            D = int(np.prod(image_shape))
        self.mu = rs.standard_normal((n_classes, D)).astype(np.float32)
        proj = np.random.RandomState(seed + 99).standard_normal((Dt if tokens is None else 16, D)).astype(np.float32) / np.sqrt(D)
        self.N, self.K, self.Q, self.B, self.D = N, K, Q, batch_size, D
        self.tokens = tokens
        if tokens is None:
            self.text = (self.mu @ proj.T + 0.5 * rs.standard_normal((n_classes, Dt))).astype(np.float32)
        else:
            V, L, pad = tokens
            self.text = np.full((n_classes, L), pad, dtype=np.int64)
            for c in range(n_classes):
                ln = rs.randint(4, L + 1)
                self.text[c, :ln] = rs.randint(1, V, size=ln)
        self.seed, self.split, self.length = seed, split, length

    def batch(self, index):
        rs = np.random.RandomState((self.seed * 1000003 + index * 31 + len(self.split)) % (2 ** 31))
        B, N, K, Q = self.B, self.N, self.K, self.Q
        S, Qn = N * K, N * Q
        cls = np.stack([rs.choice(len(self.mu), N, replace=False) for _ in range(B)])          # [B,N]
        y_s = np.stack([rs.permutation(np.repeat(np.arange(N), K)) for _ in range(B)])
        y_q = np.stack([rs.permutation(np.repeat(np.arange(N), Q)) for _ in range(B)])
        cs, cq = np.take_along_axis(cls, y_s, 1), np.take_along_axis(cls, y_q, 1)
        x_s = self.mu[cs] + 2.0 * rs.standard_normal((B, S, self.D)).astype(np.float32)
        x_q = self.mu[cq] + 2.0 * rs.standard_normal((B, Qn, self.D)).astype(np.float32)
        if self.image_shape is not None:
            x_s, x_q = x_s.reshape(B, S, *self.image_shape), x_q.reshape(B, Qn, *self.image_shape)
        t = torch.from_numpy
        return {'train': ([t(cs.astype(np.int64)), t(self.text[cs]), t(x_s.astype(np.float32))], t(y_s.astype(np.int64))),
                'test': ([t(cq.astype(np.int64)), t(self.text[cq]), t(x_q.astype(np.float32))], t(y_q.astype(np.int64)))}

    def __iter__(self):
        i = 0
        while self.length is None or i < self.length:
            yield self.batch(i)
            i += 1


def get_synthetic(args):
    """(train_loader, val_loader, test_loader, dictionary) like fumi/dataset/data.py:25-86."""
    tokens, dictionary = None, None
    if args.text_encoder in ("glove", "w2v"):
        V, L = args.synthetic_vocab, args.synthetic_seq_len
        tokens = (V, L, 0)
        dictionary = {"PAD": 0}
        dictionary.update({f"tok{i}": i for i in range(1, V)})
    shape = (args.image_channels, args.image_size, args.image_size) if getattr(args, "im_encoder", "") in ("conv4", "resnet12") else None
    mk = lambda split, q: SyntheticEpisodes(args.synthetic_classes, args.im_emb_dim, args.text_emb_dim, args.num_ways,
                                            args.num_shots, q, args.batch_size, args.seed, split, tokens, image_shape=shape)
    q_eval = int(100 / args.num_ways)                      # data.py:163-166,180-183
    return mk("train", args.num_shots_test), mk("val", q_eval), mk("test", q_eval), dictionary


def get_synthetic_resident(args, images_per_class=48):
    """``--dataset synthetic-resident``: the same learnable task family as ``synthetic``, but as a FIXED table of image
    embeddings per split (n_classes x images_per_class rows) that lives in HBM and is sampled by the GPU-resident episode
    sampler (fumi_amd/dataset/gpu_sampler.py) -- the shape of the real pipeline (precomputed embeddings + class descriptions)
    without the files.  With ``--im_encoder conv4 | resnet12`` the table holds uint8 pixels ([n, C, H, W], the host loader's image
    form mapped into 0..255) and the sampler gathers, augments (``--augment``) and normalises them on the device.  Needs a GPU."""
    from .gpu_sampler import GpuEpisodeSampler
    tokens, dictionary = None, None
    if args.text_encoder in ("glove", "w2v"):
        V, L = args.synthetic_vocab, args.synthetic_seq_len
        tokens = (V, L, 0)
        dictionary = {"PAD": 0}
        dictionary.update({f"tok{i}": i for i in range(1, V)})
    q_eval = int(100 / args.num_ways)
    per = max(images_per_class, args.num_shots + max(args.num_shots_test, q_eval))
    if getattr(args, "im_encoder", "") in ("conv4", "resnet12"):
        return _synthetic_resident_images(args, per, tokens, q_eval) + (dictionary,)

    def mk(split, q):
        base = SyntheticEpisodes(args.synthetic_classes, args.im_emb_dim, args.text_emb_dim, args.num_ways, args.num_shots, q,
                                 args.batch_size, args.seed, split, tokens)
        rs = np.random.RandomState(args.seed * 13 + len(split))
        coi = np.repeat(np.arange(args.synthetic_classes), per)
        images = base.mu[coi] + 2.0 * rs.standard_normal((len(coi), args.im_emb_dim)).astype(np.float32)
        return GpuEpisodeSampler(torch.from_numpy(images.astype(np.float32)).to(args.device), coi, torch.from_numpy(base.text),
                                 args.num_ways, args.num_shots, q, args.batch_size, seed=args.seed + len(split))
    return mk("train", args.num_shots_test), mk("val", q_eval), mk("test", q_eval), dictionary


PIXEL_RANGE = 8.0      # the image form's values (prototype N(0, 1) + 2 N(0, 1): sigma 2.24) map affinely from [-8, 8] onto 0..255


def synthetic_pixel_table(base, per, rs):
    """uint8 [n_classes * per, C, H, W] + the class of every image: ``SyntheticEpisodes``' image form (class prototype pattern plus
    noise) mapped affinely into 0..255 and rounded, one class at a time (the fp32 form of a whole split is never held)."""
    n_classes = len(base.mu)
    table = np.empty((n_classes * per,) + tuple(base.image_shape), dtype=np.uint8)
    for c in range(n_classes):
        x = base.mu[c] + 2.0 * rs.standard_normal((per, base.D)).astype(np.float32)
        u = np.clip(np.rint((x + PIXEL_RANGE) * (255.0 / (2 * PIXEL_RANGE))), 0, 255).astype(np.uint8)
        table[c * per:(c + 1) * per] = u.reshape((per,) + tuple(base.image_shape))
    return table, np.repeat(np.arange(n_classes), per)


def pixel_statistics(table, chunk=4096):
    """Per-channel mean and standard deviation of a device uint8 table [n, C, H, W] on the [0, 1] pixel scale (computed once, on
    the device, in float64 sums)."""
    C = table.shape[1]
    s1 = torch.zeros(C, dtype=torch.float64, device=table.device)
    s2 = torch.zeros(C, dtype=torch.float64, device=table.device)
    for i in range(0, table.shape[0], chunk):
        x = table[i:i + chunk].to(torch.float64) / 255.0
        s1 += x.sum(dim=(0, 2, 3))
        s2 += (x * x).sum(dim=(0, 2, 3))
    n = table.shape[0] * table.shape[2] * table.shape[3]
    mean = s1 / n
    std = (s2 / n - mean * mean).clamp_min(0).sqrt().clamp_min(1e-6)
    return tuple(mean.tolist()), tuple(std.tolist())


def image_normalization(args, train_table):
    """--image_mean / --image_std, or the train table's own per-channel statistics (used for all three splits)."""
    C = train_table.shape[1]
    mean, std = getattr(args, "image_mean", None), getattr(args, "image_std", None)
    if mean is None or std is None:
        m, s = pixel_statistics(train_table)
        mean, std = (m if mean is None else mean), (s if std is None else std)
    spread = lambda v: tuple(float(x) for x in (list(v) * C if len(v) == 1 else v))      # one value serves every channel
    mean, std = spread(mean), spread(std)
    if len(mean) != C or len(std) != C:
        raise ValueError(f"--image_mean / --image_std need one value or {C} (one per channel)")
    return mean, std


def train_augmentation(args):
    """--augment for a pixel table: random crop out of the zero-padded image, horizontal flip, colour jitter (three channels only);
    None without the flag."""
    if not getattr(args, "augment", False):
        return None
    j = float(args.augment_jitter) if args.image_channels == 3 else 0.0
    return dict(pad=int(args.augment_pad), flip=True, jitter=(j, j, j))


def center_rect(Hs, Ws, frac):
    """(x0, y0, w, h): the centred square of side max(1, min(m, round(frac m))), m = min(Hs, Ws)."""
    m = min(Hs, Ws)
    side = max(1, min(m, int(round(float(frac) * m))))
    return (Ws - side) // 2, (Hs - side) // 2, side, side


def resize_settings(args, table_hw):
    """How the samplers of a pixel table stored at ``table_hw`` = (Hs, Ws) resample to --image_size: None when nothing is resampled
    (the table is of that size and --augment_scale is not given), else dict(out_size=, eval=, train=, augment=) -- the keyword
    arguments of GpuEpisodeSampler: ``eval`` (validation, test) is the --image_crop_frac centre square; ``train`` is the same
    without --augment and the random-resized crop (--augment_scale, default 0.08 1.0; --augment_ratio) with it, when ``augment``
    holds flip and jitter (--augment_pad is not used on this path)."""
    Hs, Ws = int(table_hw[0]), int(table_hw[1])
    size = int(args.image_size)
    scale = getattr(args, "augment_scale", None)
    if (Hs, Ws) == (size, size) and scale is None:
        return None
    rect = dict(rect=center_rect(Hs, Ws, getattr(args, "image_crop_frac", 0.875)))
    out = dict(out_size=(size, size), eval=rect, train=rect, augment=None)
    if getattr(args, "augment", False):
        lo, hi = scale if scale is not None else (0.08, 1.0)
        j = float(args.augment_jitter) if args.image_channels == 3 else 0.0
        out["train"] = dict(scale=(float(lo), float(hi)), ratio=float(getattr(args, "augment_ratio", 4.0 / 3.0)))
        out["augment"] = dict(flip=True, jitter=(j, j, j))
    return out


def pixel_samplers(args, tables, norm, q_eval):
    """(train, val, test) GpuEpisodeSamplers over tables[split] = (uint8 table on the device, class of every image, class text)."""
    from .gpu_sampler import GpuEpisodeSampler
    rs = resize_settings(args, tables["train"][0].shape[2:])
    for split in ("val", "test"):
        if (rs is None) != (resize_settings(args, tables[split][0].shape[2:]) is None):
            raise ValueError(f"the {split} table is stored at {tuple(tables[split][0].shape[2:])}, the train table at "
                             f"{tuple(tables['train'][0].shape[2:])}: either all are of --image_size or none")

    def mk(split, q, train):
        kw = {}
        if rs is None:
            kw["augment"] = train_augmentation(args) if train else None
        else:
            r = resize_settings(args, tables[split][0].shape[2:])
            kw.update(out_size=r["out_size"], resize=r["train"] if train else r["eval"], augment=r["augment"] if train else None)
        return GpuEpisodeSampler(*tables[split], args.num_ways, args.num_shots, q, args.batch_size, seed=args.seed + len(split),
                                 normalize=norm, **kw)
    if getattr(args, "model", "") == "pretrain":       # supervised batches over the train table, the episodic val / test samplers
        return supervised_pixel_source(args, tables["train"], norm, rs), mk("val", q_eval, False), mk("test", q_eval, False)
    return mk("train", args.num_shots_test, True), mk("val", q_eval, False), mk("test", q_eval, False)


def supervised_pixel_source(args, table, norm, rs):
    """``--model pretrain``: SupervisedPixelBatches over table = (uint8 table on the device, class of every image, class text) with the
    gather arguments the episodic train sampler would get (``rs`` = resize_settings of the table); the class ids are the rows of
    the class text."""
    from .supervised_pixels import SupervisedPixelBatches
    images, labels, text = table
    if rs is None:
        kw = dict(augment=train_augmentation(args))
    else:
        kw = dict(out_size=rs["out_size"], resize=rs["train"], augment=rs["augment"])
    if getattr(args, "mixup_alpha", 0.0) > 0 or getattr(args, "cutmix_alpha", 0.0) > 0:
        kw["mix"] = dict(mixup_alpha=args.mixup_alpha, cutmix_alpha=args.cutmix_alpha, prob=getattr(args, "mix_prob", 1.0))
    src = SupervisedPixelBatches(images, labels, args.pretrain_batch, seed=args.seed + len("train"), normalize=norm, **kw)
    src.n_classes = int(text.shape[0])
    return src


def _synthetic_resident_images(args, per, tokens, q_eval):
    """``--dataset synthetic-resident`` with an image encoder: a uint8 pixel table per split, resident in HBM."""
    stored = int(getattr(args, "synthetic_table_size", None) or args.image_size)
    shape = (args.image_channels, stored, stored)
    tables = {}
    for split in ("train", "val", "test"):
        base = SyntheticEpisodes(args.synthetic_classes, args.im_emb_dim, args.text_emb_dim, args.num_ways, args.num_shots, 1,
                                 args.batch_size, args.seed, split, tokens, image_shape=shape)
        table, coi = synthetic_pixel_table(base, per, np.random.RandomState(args.seed * 13 + len(split)))
        tables[split] = (torch.from_numpy(table).to(args.device), coi, torch.from_numpy(base.text))
    norm = image_normalization(args, tables["train"][0])
    return pixel_samplers(args, tables, norm, q_eval)


class SyntheticSupervised:
    """Supervised (image embedding, class text embedding, class id) mini-batches with the item contract of the reference's
    SupervisedInatAnim + DataLoader (fumi/dataset/data.py:54-70,231-291): batch = [images [bs, D], text [bs, Dt], ids [bs]],
    shuffled every epoch.  Same learnable task family as SyntheticEpisodes."""

    def __init__(self, n_classes, per_class, D, Dt, batch_size, seed, split):
        base = SyntheticEpisodes(n_classes, D, Dt, 1, 1, 1, 1, seed, split)
        rs = np.random.RandomState(seed * 17 + len(split))
        self.ids = np.repeat(np.arange(n_classes), per_class)
        self.images = torch.from_numpy((base.mu[self.ids] + 2.0 * rs.standard_normal((len(self.ids), D))).astype(np.float32))
        self.text = torch.from_numpy(base.text)
        self.bs, self.rs = batch_size, rs

    def __iter__(self):
        perm = self.rs.permutation(len(self.ids))
        for i in range(0, len(perm), self.bs):
            idx = perm[i:i + self.bs]
            yield [self.images[idx], self.text[self.ids[idx]], torch.from_numpy(self.ids[idx])]


def get_synthetic_supervised(args, per_class=6):
    mk = lambda split: SyntheticSupervised(args.synthetic_classes, per_class, args.im_emb_dim, args.text_emb_dim, args.batch_size,
                                           args.seed, split)
    return mk("train"), mk("val"), mk("test"), {}
