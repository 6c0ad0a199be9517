"""``--dataset image-npy``: raw uint8 images from .npy files into an HBM-resident pixel table (--im_encoder conv4 | resnet12).

Per split (train / val / test) under ``--data_dir``:

    {split}_images.npy       uint8 [n, H, W, C] or [n, C, H, W]  (memory-mapped, converted once to planar, moved to HBM)
    {split}_labels.npy       ints  [n]: the class id of every image
    {split}_class_text.npy   fp32  [n_classes, Dt]: one precomputed text row per class id (--text_encoder BERT)

The table stays uint8 on the device (21 KB per 3 x 84 x 84 image); the GPU-resident episode sampler draws the episodes and
csrc/imgather.hip gathers, augments (``--augment``: train split only) and normalises a meta-batch without touching the host.
Decoding is out of scope.  Files stored at another size than the encoder is built for (--image_size) are resampled on the device
(csrc/imresize.hip): the --image_crop_frac centre square for validation, test and un-augmented training, a random-resized crop
(--augment_scale, --augment_ratio) with --augment."""
import os

import numpy as np
import torch

MAX_CHANNELS = 8          # what the encoders and fumi_hip_gather_images take


def to_planar(images):
    """uint8 [n, H, W, C] or [n, C, H, W] -> [n, C, H, W].  The channel axis is the one of at most 8 entries; the two image axes
    must then both be larger than that, or the layout cannot be told."""
    if images.dtype != np.uint8:
        raise ValueError(f"images must be uint8 pixels, got {images.dtype}")
    if images.ndim != 4:
        raise ValueError(f"images must be [n, H, W, C] or [n, C, H, W], got shape {tuple(images.shape)}")
    _, a, b, c = images.shape
    if c <= MAX_CHANNELS < min(a, b):
        return np.ascontiguousarray(np.moveaxis(images, 3, 1))
    if a <= MAX_CHANNELS < min(b, c):
        return np.ascontiguousarray(images)
    raise ValueError(f"cannot tell the layout of images of shape {tuple(images.shape)}: neither [n, H, W, C] nor [n, C, H, W] "
                     f"with C <= {MAX_CHANNELS} < H, W")


def load_image_split(root, split):
    """Host-side parsing and validation of one split (no GPU): -> (images uint8 [n, C, H, W], labels int64 [n],
    class_text fp32 [n_classes, Dt]).  FileNotFoundError for a missing file, ValueError for files that do not fit together."""
    paths = {k: os.path.join(root, f"{split}_{k}.npy") for k in ("images", "labels", "class_text")}
    for p in paths.values():
        if not os.path.exists(p):
            raise FileNotFoundError(f"{p} not found: --dataset image-npy needs {{train,val,test}}_images.npy, _labels.npy and "
                                    f"_class_text.npy under {root}")
    images = to_planar(np.load(paths["images"], mmap_mode="r"))
    labels = np.load(paths["labels"])
    if labels.ndim != 1 or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"{paths['labels']}: expected one integer class id per image, got {labels.dtype} {tuple(labels.shape)}")
    if len(labels) != len(images):
        raise ValueError(f"{split}: {len(labels)} labels for {len(images)} images")
    text = np.load(paths["class_text"])
    if text.ndim != 2 or not np.issubdtype(text.dtype, np.floating):
        raise ValueError(f"{paths['class_text']}: expected fp32 [n_classes, Dt], got {text.dtype} {tuple(text.shape)}")
    labels = labels.astype(np.int64)
    if len(labels) and (labels.min() < 0 or labels.max() >= len(text)):
        raise ValueError(f"{split}: class ids span {int(labels.min())}..{int(labels.max())} but {paths['class_text']} has "
                         f"{len(text)} rows: every class id needs a text row")
    return images, labels, np.ascontiguousarray(text, dtype=np.float32)


def check_image_splits(args, splits):
    """Host-side checks of the loaded splits against the flags (no GPU): the channels and the text width must fit; the stored image
    size may differ from --image_size (the samplers then resample), but not between the splits' need to resample."""
    from .synthetic import resize_settings
    for s, (images, _, text) in splits.items():
        if images.shape[1] != args.image_channels:
            raise ValueError(f"{s}_images.npy holds {tuple(images.shape[1:])} images; --image_channels says {args.image_channels}")
        if text.shape[1] != args.text_emb_dim:
            raise ValueError(f"{s}_class_text.npy rows are {text.shape[1]} wide; --text_emb_dim is {args.text_emb_dim}")
    need = {s: resize_settings(args, images.shape[2:]) is not None for s, (images, _, _) in splits.items()}
    if len(set(need.values())) > 1:
        raise ValueError(f"the splits are stored at {[tuple(v[0].shape[2:]) for v in splits.values()]}: either all are of "
                         f"--image_size {args.image_size} or none")


def get_image_npy(args):
    """(train, val, test, dictionary) for ``--dataset image-npy``: three GPU-resident samplers over uint8 pixel tables."""
    from .synthetic import image_normalization, pixel_samplers
    if getattr(args, "im_encoder", "") not in ("conv4", "resnet12"):
        raise ValueError("--dataset image-npy holds raw pixels: it needs --im_encoder conv4 or resnet12")
    if args.text_encoder != "BERT":
        raise NotImplementedError("--dataset image-npy reads precomputed text rows ({split}_class_text.npy): --text_encoder BERT")
    if args.device.type != "cuda":
        raise RuntimeError("--dataset image-npy keeps the pixel table in HBM and samples on the GPU: no GPU visible")
    splits = {s: load_image_split(args.data_dir, s) for s in ("train", "val", "test")}
    check_image_splits(args, splits)
    tables = {s: (torch.from_numpy(images).to(args.device), labels, torch.from_numpy(text)) for s, (images, labels, text) in splits.items()}
    norm = image_normalization(args, tables["train"][0])
    q_eval = int(100 / args.num_ways)                                                   # data.py:163-166,180-183
    return pixel_samplers(args, tables, norm, q_eval) + ({},)
