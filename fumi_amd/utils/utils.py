"""Flag system, model / optimizer factories and checkpoint IO -- the host-side mirror of fumi/utils/utils.py.

Same flag names, defaults and types as the reference parser (fumi/utils/utils.py:19-229); same factory
behaviour (:232-299) and checkpoint dictionary (:406-441).  Additive flags of this engine are listed last.
The AM3 head math of the reference file (get_prototypes / prototypical_loss / get_preds, :302-402) runs inside the
fused HIP AM3 step; the functions of the same names below are thin device wrappers around it.
"""
import argparse
import os
import shutil

import numpy as np
import torch

from .wandb_compat import wandb

# (flag, kwargs) in the reference's order; defaults/types/help are the contract
_REFERENCE_FLAGS = [
    ("--wandb_entity", dict(type=str, default="multimodal-image-cls", help="W&B entity")),
    ("--wandb_project", dict(type=str, default="fumi", help="W&B project")),
    ("--dataset", dict(type=str, default="inat-anim", help="Dataset to use (inat-anim, supervised-inat-anim, synthetic, synthetic-resident, image-npy)")),
    ("--data_dir", dict(type=str, default="./data", help="Directory to use for data")),
    ("--checkpoint", dict(type=str, default=None, help="Path to pretrained model (a best.pth.tar file, or a W&B run id when wandb is installed)")),
    ("--log_dir", dict(type=str, default="./results", help="Directory to use for results")),
    ("--remove_stop_words", dict(action="store_true", help="Whether to remove stop words")),
    ("--colab", dict(action="store_true", help="Whether the script is running on Google Colab")),
    # optimizer
    ("--epochs", dict(type=int, default=50000, help="Number of meta-learning batches to train for")),
    ("--optim", dict(type=str, default="adam", help="Optimiser")),
    ("--lr", dict(type=float, default=3e-5, help="Learning rate")),
    ("--momentum", dict(type=float, default=0.9, help="Momentum for SGD")),
    ("--batch_size", dict(type=int, default=4, help="Number of tasks in mini-batch")),
    ("--weight_decay", dict(type=float, default=5e-4, help="L2 regulariser")),
    ("--num_warmup_steps", dict(type=float, default=10, help="Warm up lr scheduler")),
    # dataloader
    ("--num_shots", dict(type=int, default=5, help="Number of examples per class (k-shot)")),
    ("--num_ways", dict(type=int, default=5, help="Number of classes per task (N-way)")),
    ("--num_shots_test", dict(type=int, default=32, help="Number of examples per class in query set")),
    ("--augment", dict(action="store_true", help="Augment data with image transformations")),
    ("--num_workers", dict(type=int, default=0, help="Number of workers for dataloader")),
    ("--image_embedding_model", dict(type=str, default="resnet-152", help="resnet-152 embedding (2048 dimensions) or resnet-34 (512 dimensions)")),
    # model
    ("--model", dict(type=str, default="fumi", help="Model to be trained")),
    ("--prototype_dim", dict(type=int, default=64, help="Dimension of latent space")),
    ("--im_encoder", dict(type=str, default="precomputed", help="Type of vision feature extractor (resnet, precomputed; conv4 / resnet12 = Conv4 / bf16 ResNet-12 on raw images for fumi, maml and am3, this engine's extensions at the im_net / image_encoder seam)")),
    ("--im_emb_dim", dict(type=int, default=2048, help="Dimension of image embedding (if precomputed)")),
    ("--im_hid_dim", dict(type=int, nargs="+", default=[256, 64], help="Hidden dimension of image model")),
    ("--text_encoder", dict(type=str, choices=["glove", "w2v", "RNN", "RNNhid", "BERT", "rand"], default="BERT",
                            help="Type of text embedding (glove, w2v, RNN, RNNhid, BERT, rand)")),
    ("--pooling_strat", dict(type=str, default="mean", help="Pooling strategy if using word embeddings (mean, max)")),
    ("--fine_tune", dict(action="store_true", help="Whether to fine tune text encoder")),
    ("--text_type", dict(type=str, nargs="+", default=["description"], help="What to use for text embedding (label, description or common_name)")),
    ("--text_emb_dim", dict(type=int, default=768, help="Dimension of text embedding (if precomputed)")),
    ("--text_hid_dim", dict(type=int, default=256, help="Hidden dimension for NN mapping to prototypes and lamda")),
    ("--dropout", dict(type=float, default=0.25, help="Dropout rate")),
    ("--step_size", dict(type=float, default=0.01, help="MAML step size")),
    ("--first_order", dict(action="store_true", help="Whether to use first-order MAML")),
    ("--num_train_adapt_steps", dict(type=int, default=5, help="Number of MAML inner train loop adaptation steps")),
    ("--num_test_adapt_steps", dict(type=int, default=100, help="Number of MAML inner test loop adaptation steps")),
    ("--init_all_layers", dict(action="store_true", help="Whether to initialise all (vs. last) layer weights in FUMI")),
    ("--norm_hypernet", dict(action="store_true", help="Whether to normalize output of the FUMI hypernetwork (tanh)")),
    ("--hypernet_bias_init", dict(action="store_true", help="Whether to initialise hypernet bias for policy")),
    ("--lamda_fixed", dict(default=None, type=int, help="Lambda fixed for am3. Lambda = 0 is text only, Lambda = 1 is image only")),
    ("--clip_latent_dim", dict(type=int, default=512, help="Dimension of CLIP latent space")),
    # run
    ("--seed", dict(type=int, default=123, help="patience for early stopping")),
    ("--patience", dict(type=int, default=10000, help="Early stopping patience")),
    ("--eval_freq", dict(type=int, default=2500, help="Number of batches between validation/checkpointing")),
    ("--wandb_experiment", dict(type=str, default="debug", help="Name for experiment (for wandb group)")),
    ("--evaluate", dict(action="store_true", help="skip training")),
    ("--num_ep_test", dict(type=int, default=1000, help="Number of few-shot episodes to compute test accuracy")),
    ("--disable_cuda", dict(action="store_true", help="don't use GPU")),
    ("--wandb_offline", dict(action="store_true", help="don't save to wandb")),
]
_DISTILL_FLAGS = [          # born-again distillation of --model pretrain: the tail of _FLAGS, the one open slot
    ("--distill_checkpoint", dict(type=str, default=None, help="[--model pretrain] a --model pretrain checkpoint of the same backbone: the frozen teacher the classifier is distilled from (a born-again chain is repeated runs, each naming the previous run's best.pth.tar)")),
    ("--distill_temp", dict(type=float, default=4.0, help="[--distill_checkpoint] temperature T of the distillation term T^2 KL(softmax(z_teacher / T) || softmax(z / T)) (positive)")),
    ("--distill_alpha", dict(type=float, default=0.5, help="[--distill_checkpoint] weight of the distillation term (not negative)")),
    ("--distill_ce_weight", dict(type=float, default=0.5, help="[--distill_checkpoint] weight of the cross-entropy term (not negative)")),
]
_FLAGS = _REFERENCE_FLAGS + _DISTILL_FLAGS
_SVM_FLAGS = [              # the MetaOptNet-SVM head; a list of its own that cli_parser() appends to parser()'s
    ("--svm_C", dict(type=float, default=0.1, help="[--fewshot_head svm / --pretrain_metric svm] the regularisation parameter C of the multi-class SVM: alpha_ik <= C onehot(y)_ik (positive)")),
    ("--svm_eps", dict(type=float, default=1.0, help="[--fewshot_head svm / --pretrain_metric svm] the weight eps of the identity added to the support Gram matrix (positive)")),
    ("--svm_scale", dict(type=float, default=1.0, help="[--fewshot_head svm] initial logit scale (learned); [--pretrain_metric svm] its fixed value (positive)")),
    ("--svm_steps", dict(type=int, default=120, help="[--fewshot_head svm / --pretrain_metric svm] FISTA steps of the per-episode fit (1 to 10000)")),
    ("--svm_bwd_steps", dict(type=int, default=40, help="[--fewshot_head svm] conjugate-gradient steps of the implicit backward (1 to 1000)")),
]
_ENGINE_FLAGS = [     # additive, not in the reference
    ("--synthetic_classes", dict(type=int, default=64, help="[synthetic dataset] number of classes per split")),
    ("--synthetic_vocab", dict(type=int, default=2000, help="[synthetic dataset] vocabulary size for token text")),
    ("--synthetic_seq_len", dict(type=int, default=32, help="[synthetic dataset] token sequence length")),
    ("--image_size", dict(type=int, default=84, help="[--im_encoder conv4 / resnet12] height = width of the input images")),
    ("--image_channels", dict(type=int, default=3, help="[--im_encoder conv4 / resnet12] input channels (conv4: 1-3, resnet12: 1-8)")),
    ("--augment_pad", dict(type=int, default=8, help="[--augment on a resident pixel table] zero padding of the random crop (0-64)")),
    ("--augment_jitter", dict(type=float, default=0.4, help="[--augment on a resident pixel table] amplitude of the brightness / contrast / saturation jitter (0-1; three-channel images)")),
    ("--image_crop_frac", dict(type=float, default=0.875, help="[resident pixel table stored at another size than --image_size] validation, test and un-augmented train batches take the centred square of this fraction of the shorter side, resized to --image_size")),
    ("--augment_scale", dict(type=float, nargs=2, default=None, metavar=("LO", "HI"), help="[--augment on a resident pixel table] random-resized crop: area fraction range (given, or with a table of another size than --image_size: default 0.08 1.0)")),
    ("--augment_ratio", dict(type=float, default=4.0 / 3.0, help="[--augment, random-resized crop] largest aspect ratio rmax: ratios are drawn from [1 / rmax, rmax]")),
    ("--synthetic_table_size", dict(type=int, default=None, help="[--dataset synthetic-resident with an image encoder] stored height = width of the pixel table (default: --image_size)")),
    ("--image_mean", dict(type=float, nargs="+", default=None, help="[resident pixel table] per-channel mean on the 0..1 pixel scale (default: the train table's own)")),
    ("--image_std", dict(type=float, nargs="+", default=None, help="[resident pixel table] per-channel standard deviation on the 0..1 pixel scale (default: the train table's own)")),
    ("--max_grad_norm", dict(type=float, default=None, help="clip the global L2 norm of the outer gradient to this value before every optimizer step (torch.nn.utils.clip_grad_norm_ semantics, computed on the device; default: no clipping)")),
    ("--pretrain_batch", dict(type=int, default=128, help="[--model pretrain] images per supervised training step (a multiple of 2 * --pretrain_bn_group)")),
    ("--pretrain_bn_group", dict(type=int, default=64, help="[--model pretrain] images per batch-statistics group of a training step")),
    ("--encoder_checkpoint", dict(type=str, default=None, help="[--model fumi / maml / am3 with --im_encoder conv4 / resnet12] a --model pretrain checkpoint whose backbone (conv.*) is loaded into the model's image encoder before training")),
]
_METRIC_FLAGS = [           # the cosine nearest-centroid metric; a list of its own, between the two others
    ("--metric_temp", dict(type=float, default=10.0, help="[--model metabaseline] initial temperature of the cosine classifier; [--model pretrain --pretrain_metric cosine] its fixed temperature (positive)")),
    ("--pretrain_metric", dict(type=str, choices=["euclidean", "cosine", "ridge", "logreg", "svm"], default="euclidean", help="[--model pretrain] few-shot validation / test metric: squared Euclidean distance to the class means, their cosine at --metric_temp, the ridge-regression head at --ridge_lambda / --ridge_scale, the logistic-regression head at --logreg_steps / --logreg_lr / --logreg_momentum / --logreg_C, or the SVM head at --svm_C / --svm_eps / --svm_scale / --svm_steps")),
]
_RIDGE_FLAGS = [            # the ridge-regression head; a list of its own, between _FLAGS and _ENGINE_FLAGS
    ("--fewshot_head", dict(type=str, choices=["cosine", "ridge", "proto"], default="cosine", help="[--model metabaseline] the episodic classifier: cosine nearest-centroid with a learned temperature, closed-form ridge regression on the support features with a learned ridge weight and logit scale, or Prototypical Networks (squared Euclidean distance to the class means at --proto_scale); the command line (cli_parser) also takes svm: MetaOptNet's multi-class SVM on the support features with a learned logit scale and an implicit gradient (--svm_*)")),
    ("--ridge_lambda", dict(type=float, default=50.0, help="[--fewshot_head ridge] initial ridge weight lambda (learned as its logarithm); [--pretrain_metric ridge] its fixed value (positive)")),
    ("--ridge_scale", dict(type=float, default=1.0, help="[--fewshot_head ridge] initial logit scale (learned); [--pretrain_metric ridge] its fixed value (positive)")),
    # (transductive inference, DESIGN.md section 36: appended here, the one list whose content no caller depends on)
    ("--transductive_steps", dict(type=int, default=0, help="[--model metabaseline / pretrain] soft k-means refinement of the class prototypes on each validation / test episode's queries: the number of steps (0 to 100; 0: inductive, every query row is classified alone)")),
]
_LOGREG_FLAGS = [           # the logistic-regression head; a list of its own, after _RIDGE_FLAGS
    ("--logreg_steps", dict(type=int, default=100, help="[--pretrain_metric logreg / --eval_head logreg] heavy-ball steps of the per-episode fit (1 to 10000)")),
    ("--logreg_lr", dict(type=float, default=1.0, help="[--pretrain_metric logreg / --eval_head logreg] step size of the fit (positive)")),
    ("--logreg_momentum", dict(type=float, default=0.9, help="[--pretrain_metric logreg / --eval_head logreg] heavy-ball momentum of the fit, in [0, 1)")),
    ("--logreg_C", dict(type=float, default=1.0, help="[--pretrain_metric logreg / --eval_head logreg] inverse regularisation strength, scikit-learn's LogisticRegression(C) (positive)")),
    ("--logreg_raw", dict(action="store_true", help="[--pretrain_metric logreg / --eval_head logreg] fit on the raw features: skip the L2 normalisation of the support and query rows")),
    ("--eval_head", dict(type=str, choices=["train", "logreg"], default="train", help="[--model metabaseline] the classifier of validation and test episodes: the head the model trains with, or a logistic regression fitted on each episode's backbone features")),
]
_PROTO_FLAGS = [            # the prototypical-network head; a list of its own, directly after _LOGREG_FLAGS
    ("--proto_scale", dict(type=float, default=1.0, help="[--fewshot_head proto] the scale alpha of the logits -alpha * |query - class mean|^2: its initial value (learned), or with --proto_scale_fixed its value (positive)")),
    ("--proto_scale_fixed", dict(action="store_true", help="[--fewshot_head proto] keep --proto_scale fixed: plain Prototypical Networks at the default 1.0")),
]
_PRETRAIN_MIX_FLAGS = [     # regularisers of --model pretrain; a list of their own, after _ENGINE_FLAGS
    ("--label_smoothing", dict(type=float, default=0.0, help="[--model pretrain] label smoothing eps of the training loss, in [0, 1)")),
    ("--mixup_alpha", dict(type=float, default=0.0, help="[--model pretrain] mixup: lam ~ Beta(alpha, alpha) per training batch (0: off)")),
    ("--cutmix_alpha", dict(type=float, default=0.0, help="[--model pretrain] CutMix: box area fraction 1 - lam, lam ~ Beta(alpha, alpha) per training batch (0: off; with --mixup_alpha too, one of the two per batch)")),
    ("--mix_prob", dict(type=float, default=1.0, help="[--model pretrain] probability that a training batch is mixed at all")),
]
_PRETRAIN_HEAD_FLAGS = [    # the cosine classifier of --model pretrain; a list of its own that run_parser() appends to cli_parser()'s
    ("--pretrain_head", dict(type=str, choices=["linear", "cosine"], default="linear", help="[--model pretrain] the classifier the backbone is trained with: nn.Linear on the raw features, or a cosine classifier, --pretrain_head_scale * cos(feature, class weight), without a bias")),
    ("--pretrain_head_scale", dict(type=float, default=10.0, help="[--pretrain_head cosine] the scale of the cosine logits: its initial value (learned), or with --pretrain_head_scale_fixed its value (positive)")),
    ("--pretrain_head_scale_fixed", dict(action="store_true", help="[--pretrain_head cosine] keep --pretrain_head_scale fixed")),
]
_ADAPT_FLAGS = [            # the set-to-set prototype adaptation; a list of its own that main_parser() appends to run_parser()'s
    ("--fewshot_adapt", dict(type=str, choices=["none", "feat"], default="none", help="[--model metabaseline, --fewshot_head cosine | proto] adapt the class prototypes of an episode to the task before the head classifies against them: feat is FEAT's one-head self-attention block over the set of prototypes, with a residual and a LayerNorm")),
]
_DROP_FLAGS = [             # DropBlock / dropout inside the ResNet-12; a list of its own that drop_parser() appends to main_parser()'s
    ("--drop_rate", dict(type=float, default=0.0, help="[--model pretrain | metabaseline, --im_encoder resnet12] final drop probability of the regulariser on the block outputs of the ResNet-12 in training steps (the MetaOptNet / RFS network: 0.1); 0: off")),
    ("--drop_block_size", dict(type=int, default=5, help="[--drop_rate > 0] block size of the DropBlock blocks (1 to 8)")),
    ("--drop_blocks", dict(type=int, default=2, help="[--drop_rate > 0] the last this-many blocks use DropBlock, the earlier ones element-wise dropout")),
    ("--drop_anneal_steps", dict(type=int, default=40000, help="[--drop_rate > 0] the rate at training step t is --drop_rate * min(1, t / this); 0: the full rate from step 0")),
]


def parser():
    p = argparse.ArgumentParser(description="Multimodal image classification")
    for flag, kw in _FLAGS + _RIDGE_FLAGS + _LOGREG_FLAGS + _PROTO_FLAGS + _ENGINE_FLAGS + _METRIC_FLAGS + _PRETRAIN_MIX_FLAGS:
        p.add_argument(flag, **kw)
    return p


def cli_parser():
    """What the command line takes (``main.parse_args``): ``parser()``, the choice ``svm`` of --fewshot_head, and after every flag of
    ``parser()`` the --svm_* flags.  ``parser()`` itself keeps the flag sequence and the choices the earlier heads were written
    against."""
    p = parser()
    for act in p._actions:
        if act.dest == "fewshot_head":
            act.choices = list(act.choices) + ["svm"]
    for flag, kw in _SVM_FLAGS:
        p.add_argument(flag, **kw)
    return p


def run_parser():
    """``cli_parser()`` and after every flag of it the --pretrain_head* flags.  ``cli_parser()`` and ``parser()`` keep the flag
    sequences the earlier heads were written against."""
    p = cli_parser()
    for flag, kw in _PRETRAIN_HEAD_FLAGS:
        p.add_argument(flag, **kw)
    return p


def main_parser():
    """``run_parser()`` and after every flag of it --fewshot_adapt: what ``main.parse_args`` reads.  ``run_parser()`` keeps the flag
    sequence the cosine classifier was written against."""
    p = run_parser()
    for flag, kw in _ADAPT_FLAGS:
        p.add_argument(flag, **kw)
    return p


def drop_parser():
    """``main_parser()`` and after every flag of it the --drop_* flags: what ``main.parse_args`` reads.  ``main_parser()`` keeps the
    flag sequence the prototype adaptation was written against."""
    p = main_parser()
    for flag, kw in _DROP_FLAGS:
        p.add_argument(flag, **kw)
    return p


def match_parser():
    """``drop_parser()`` with the choice ``matching`` of --fewshot_head and of --pretrain_metric (the Matching Networks head, DESIGN.md
    section 47): what ``main.parse_args`` reads.  ``drop_parser()`` keeps the flag sequence and the choices the regulariser was written
    against."""
    p = drop_parser()
    for act in p._actions:
        if act.dest in ("fewshot_head", "pretrain_metric"):
            act.choices = list(act.choices) + ["matching"]
    return p


_RELATION_FLAGS = [         # the Relation Network head; a list of its own that relation_parser() appends to match_parser()'s
    ("--relation_hidden", dict(type=int, default=256, help="[--fewshot_head relation] hidden width H of the relation module Linear(2F, H) -> ReLU -> Linear(H, 1) (a multiple of 32 from 32 to 1024)")),
    ("--relation_loss", dict(type=str, choices=["mse", "ce"], default="mse", help="[--fewshot_head relation] the training loss: mse regresses sigmoid(score) onto the one-hot label (the paper's), ce is the softmax cross-entropy of the scores over the classes")),
]


def relation_parser():
    """``match_parser()`` with the choice ``relation`` of --fewshot_head (not of --pretrain_metric: a classifier pre-training has no
    relation module to evaluate with) and after every flag of it the --relation_* flags (the Relation Network head, DESIGN.md section
    51): what ``main.parse_args`` reads.  ``match_parser()`` keeps the flag sequence and the choices the matching head was written
    against."""
    p = match_parser()
    for act in p._actions:
        if act.dest == "fewshot_head":
            act.choices = list(act.choices) + ["relation"]
    for flag, kw in _RELATION_FLAGS:
        p.add_argument(flag, **kw)
    return p


def relation_config(args):
    """None (another head), or ``MetaBaseline``'s ``relation=`` dict (hidden, loss) from an argparse namespace."""
    if getattr(args, "fewshot_head", "cosine") != "relation":
        return None
    return dict(hidden=int(getattr(args, "relation_hidden", 256)), loss=str(getattr(args, "relation_loss", "mse")))


def drop_config(args):
    """None (--drop_rate 0), or the keyword arguments of ``resnet12.DropSchedule`` from an argparse namespace."""
    if not getattr(args, "drop_rate", 0.0) > 0.0:
        return None
    return dict(rate=float(args.drop_rate), block_size=int(getattr(args, "drop_block_size", 5)), blocks=int(getattr(args, "drop_blocks", 2)),
                anneal_steps=int(getattr(args, "drop_anneal_steps", 40000)), seed=int(getattr(args, "seed", 0) or 0))


def logreg_config(cfg=None):
    """The keyword arguments of ``logreg_head_step`` from a dict, an argparse namespace (--logreg_*) or None (the defaults), checked
    against the kernel's limits."""
    get = cfg.get if isinstance(cfg, dict) else (lambda k, dflt: getattr(cfg, "logreg_" + k, dflt))
    c = dict(steps=int(get("steps", 100)), lr=float(get("lr", 1.0)), momentum=float(get("momentum", 0.9)), C=float(get("C", 1.0)))
    c["normalize"] = bool(get("normalize", True)) if isinstance(cfg, dict) else not bool(get("raw", False))
    if not 1 <= c["steps"] <= 10000:
        raise ValueError(f"--logreg_steps {c['steps']} must lie in [1, 10000]")
    if not c["lr"] > 0.0:
        raise ValueError(f"--logreg_lr {c['lr']} must be positive")
    if not 0.0 <= c["momentum"] < 1.0:
        raise ValueError(f"--logreg_momentum {c['momentum']} must lie in [0, 1)")
    if not c["C"] > 0.0:
        raise ValueError(f"--logreg_C {c['C']} must be positive")
    return c


_SVM_DEFAULTS = dict(C=0.1, eps=1.0, scale=1.0, steps=120, bwd_steps=40)


def svm_config(cfg=None):
    """C, eps, scale and the two step counts of the SVM head from a dict, an argparse namespace (--svm_*) or None (the defaults),
    checked against the kernel's limits."""
    get = cfg.get if isinstance(cfg, dict) else (lambda k, dflt: getattr(cfg, "svm_" + k, dflt))
    c = {k: type(v)(get(k, v)) for k, v in _SVM_DEFAULTS.items()}
    for k in ("C", "eps", "scale"):
        if not c[k] > 0.0:
            raise ValueError(f"--svm_{k} {c[k]} must be positive")
    if not 1 <= c["steps"] <= 10000:
        raise ValueError(f"--svm_steps {c['steps']} must lie in [1, 10000]")
    if not 1 <= c["bwd_steps"] <= 1000:
        raise ValueError(f"--svm_bwd_steps {c['bwd_steps']} must lie in [1, 1000]")
    return c


def svm_flags_moved(args):
    """The --svm_* flags that differ from their defaults (they belong to --fewshot_head svm / --pretrain_metric svm)."""
    return ["--svm_" + k for k, v in _SVM_DEFAULTS.items() if getattr(args, "svm_" + k, v) != v]


def init_model(args, dictionary, watch=True):
    """Model factory (utils.py:232-274).  Unknown names fall through to AM3 exactly like the reference."""
    from ..models import am3, clip, fumi, maml
    if args.model == "maml":
        conv = (dict(im_encoder=args.im_encoder, image_size=args.image_size, image_channels=args.image_channels)
                if args.im_encoder in ("conv4", "resnet12") else {})
        model = maml.PureImageNetwork(im_embed_dim=args.im_emb_dim, n_way=args.num_ways, hidden_dims=args.im_hid_dim, **conv)
    elif args.model == "fumi":
        model = fumi.FUMI(n_way=args.num_ways, im_emb_dim=args.im_emb_dim, im_hid_dim=args.im_hid_dim,
                          text_encoder=args.text_encoder, text_emb_dim=args.text_emb_dim,
                          text_hid_dim=args.text_hid_dim, dropout_rate=args.dropout, dictionary=dictionary,
                          pooling_strat=args.pooling_strat, init_all_layers=args.init_all_layers,
                          norm_hypernet=args.norm_hypernet, fine_tune=args.fine_tune, init_bias=args.hypernet_bias_init,
                          **(dict(im_encoder=args.im_encoder, image_size=args.image_size, image_channels=args.image_channels)
                             if args.im_encoder in ("conv4", "resnet12") else {}))
    elif args.model == "pretrain":
        from ..models import pretrain
        model = pretrain.Pretrain(im_encoder=args.im_encoder, image_size=args.image_size, image_channels=args.image_channels,
                                  n_classes=args.n_classes, bn_group=args.pretrain_bn_group, num_ways=args.num_ways,
                                  label_smoothing=getattr(args, "label_smoothing", 0.0),
                                  metric=getattr(args, "pretrain_metric", "euclidean"), metric_temp=getattr(args, "metric_temp", 10.0),
                                  ridge_lambda=getattr(args, "ridge_lambda", 50.0), ridge_scale=getattr(args, "ridge_scale", 1.0),
                                  logreg=logreg_config(args) if getattr(args, "pretrain_metric", "euclidean") == "logreg" else None,
                                  svm=svm_config(args) if getattr(args, "pretrain_metric", "euclidean") == "svm" else None,
                                  transductive_steps=getattr(args, "transductive_steps", 0),
                                  distill=(dict(temp=getattr(args, "distill_temp", 4.0), alpha=getattr(args, "distill_alpha", 0.5),
                                                ce_weight=getattr(args, "distill_ce_weight", 0.5))
                                           if getattr(args, "distill_checkpoint", None) else None),
                                  **(dict(head="cosine", head_scale=getattr(args, "pretrain_head_scale", 10.0),
                                          head_scale_fixed=getattr(args, "pretrain_head_scale_fixed", False))
                                     if getattr(args, "pretrain_head", "linear") == "cosine" else {}),
                                  **(dict(drop=drop_config(args)) if drop_config(args) else {}))
    elif args.model == "metabaseline":
        from ..models import metabaseline
        model = metabaseline.MetaBaseline(im_encoder=args.im_encoder, image_size=args.image_size, image_channels=args.image_channels,
                                          num_ways=args.num_ways, init_temp=getattr(args, "metric_temp", 10.0),
                                          head=getattr(args, "fewshot_head", "cosine"), ridge_lambda=getattr(args, "ridge_lambda", 50.0),
                                          ridge_scale=getattr(args, "ridge_scale", 1.0), eval_head=getattr(args, "eval_head", "train"),
                                          logreg=logreg_config(args) if getattr(args, "eval_head", "train") == "logreg" else None,
                                          proto_scale=getattr(args, "proto_scale", 1.0),
                                          proto_scale_fixed=getattr(args, "proto_scale_fixed", False),
                                          transductive_steps=getattr(args, "transductive_steps", 0),
                                          svm=svm_config(args) if getattr(args, "fewshot_head", "cosine") == "svm" else None,
                                          **(dict(adapt="feat") if getattr(args, "fewshot_adapt", "none") == "feat" else {}),
                                          **(dict(drop=drop_config(args)) if drop_config(args) else {}),
                                          **(dict(relation=relation_config(args)) if relation_config(args) else {}))
    elif args.model == "clip":
        model = clip.CLIP(text_input_dim=args.text_emb_dim, image_input_dim=args.im_emb_dim, latent_dim=args.clip_latent_dim)
    else:
        model = am3.AM3(im_encoder=args.im_encoder, im_emb_dim=args.im_emb_dim, text_encoder=args.text_encoder,
                        text_emb_dim=args.text_emb_dim, text_hid_dim=args.text_hid_dim,
                        prototype_dim=args.prototype_dim, dropout=args.dropout, fine_tune=args.fine_tune,
                        dictionary=dictionary, pooling_strat=args.pooling_strat, lamda_fixed=args.lamda_fixed,
                        **(dict(image_size=args.image_size, image_channels=args.image_channels)
                           if args.im_encoder in ("conv4", "resnet12") else {}))
    if watch:
        wandb.watch(model, log="all")
    model.to(args.device)
    return model


def _linear_warmup_schedule(opt, num_warmup_steps, num_training_steps):
    """transformers.get_linear_schedule_with_warmup (utils.py:11,293-294): linear ramp then linear decay to 0."""
    def lr_lambda(step):
        if step < num_warmup_steps:
            return float(step) / float(max(1, num_warmup_steps))
        return max(0.0, float(num_training_steps - step) / float(max(1, num_training_steps - num_warmup_steps)))
    return torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda)


def init_optim(args, model):
    """Optimizer factory (utils.py:277-299); may return an (optimizer, scheduler) tuple."""
    # torch.optim's classes whose step() is one fused HIP launch on the GPU (and folds into the FuMI meta-step's last launch)
    from ..optim import SGD, Adam, AdamW
    clip = dict(max_grad_norm=getattr(args, "max_grad_norm", None))        # --max_grad_norm (additive; None: no clipping)
    if args.optim == "adam":
        return Adam(params=model.parameters(), lr=args.lr, weight_decay=args.weight_decay, **clip)
    if args.optim == "SGD":
        return SGD(params=model.parameters(), lr=args.lr, weight_decay=args.weight_decay, momentum=args.momentum, **clip)
    if args.optim == "adamw":
        # transformers.AdamW(lr) of the pinned 4.5.1: decoupled weight decay, default weight_decay 0.0
        return AdamW(params=model.parameters(), lr=args.lr, weight_decay=0.0, **clip)
    if args.optim == "adamw_lin_schedule":
        opt = AdamW(params=model.parameters(), lr=args.lr, weight_decay=0.0, **clip)
        return opt, _linear_warmup_schedule(opt, args.num_warmup_steps, args.epochs)
    raise NotImplementedError()


# ---- checkpoints (utils.py:406-441): same dictionary keys, same ckpt/best file names ---------------------------------
def save_checkpoint(checkpoint_dict, is_best):
    """fumi/utils/utils.py:406-419.  Episode-sharded runs keep replicated parameters, so rank 0 alone writes; the others wait
    (the best checkpoint is reloaded by every rank at the end of training)."""
    import torch.distributed as dist
    sharded = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    if not sharded or dist.get_rank() == 0:
        ckpt = os.path.join(wandb.run.dir, "ckpt.pth.tar")
        best = os.path.join(wandb.run.dir, "best.pth.tar")
        torch.save(checkpoint_dict, ckpt)
        wandb.save(ckpt)
        if is_best:
            shutil.copyfile(ckpt, best)
            wandb.save(best)
    if sharded:
        dist.barrier()


def load_checkpoint(model, optimizer, device, checkpoint_file):
    checkpoint = torch.load(checkpoint_file, map_location=device, weights_only=False)
    model.load_state_dict(checkpoint["state_dict"])
    optimizer.load_state_dict(checkpoint["optimizer"])
    print(f"Loaded {checkpoint_file}, trained to epoch {checkpoint['batch_idx']} "
          f"with best loss (acc for CLIP) {checkpoint['best_loss']}")
    return model, optimizer


def load_backbone_state(model, state_dict):
    """Copy the ``conv.*`` tensors of a ``--model pretrain`` state_dict into the model's backbone module (``backbone_module()``: the
    Conv4 / ResNet12 of FuMI, MAML, AM3 or Pretrain).  Every backbone tensor must be present with the same shape (ValueError naming
    the tensor otherwise); the classifier and anything else in the state_dict is ignored, nothing else in the model changes.  The
    model's cached parameter views (``_pcache``) are dropped so that the first step sees the loaded weights."""
    get = getattr(model, "backbone_module", None)
    bb = get() if get is not None else None
    if bb is None:
        raise ValueError("--encoder_checkpoint needs a model with an image backbone (--im_encoder conv4 or resnet12)")
    own = bb.state_dict()
    for name, dst in own.items():
        src = state_dict.get("conv." + name)
        if src is None:
            raise ValueError(f"--encoder_checkpoint: the checkpoint has no backbone tensor conv.{name}")
        if tuple(src.shape) != tuple(dst.shape):
            raise ValueError(f"--encoder_checkpoint: backbone tensor conv.{name} is {tuple(src.shape)} in the checkpoint, "
                             f"{tuple(dst.shape)} in the model")
    with torch.no_grad():
        for name, dst in own.items():
            dst.copy_(state_dict["conv." + name])
    if hasattr(model, "_pcache"):
        model._pcache = None
    return sorted("conv." + n for n in own)


def load_encoder_checkpoint(model, device, checkpoint_file):
    """--encoder_checkpoint: the backbone of a ``--model pretrain`` checkpoint file into ``model`` (``load_backbone_state``)."""
    checkpoint = torch.load(checkpoint_file, map_location=device, weights_only=False)
    names = load_backbone_state(model, checkpoint["state_dict"])
    print(f"Loaded the backbone ({len(names)} tensors) of {checkpoint_file}, pre-trained to batch {checkpoint.get('batch_idx')}")
    return model


def load_distill_checkpoint(model, args, checkpoint_file):
    """--distill_checkpoint: the ``--model pretrain`` checkpoint file becomes the frozen teacher of ``model`` (``Pretrain.load_teacher``).
    A teacher saved with another --im_encoder, --image_size or --image_channels is refused by name."""
    checkpoint = torch.load(checkpoint_file, map_location=args.device, weights_only=False)
    saved = checkpoint.get("args") or {}
    for key in ("im_encoder", "image_size", "image_channels"):
        if key in saved and saved[key] != getattr(args, key):
            raise ValueError(f"--distill_checkpoint: the teacher was trained with --{key} {saved[key]}, this run has --{key} "
                             f"{getattr(args, key)}")
    model.load_teacher(checkpoint["state_dict"])
    print(f"Loaded the teacher of {checkpoint_file}, pre-trained to batch {checkpoint.get('batch_idx')}")
    return model


# ---- classification metrics of AM3 (utils.py:319-326) on host integers ------------------------------------------------
def macro_metrics(flat_targets, flat_preds):
    """accuracy + macro precision/recall/F1 (what sklearn's accuracy_score / precision_recall_fscore_support
    (average='macro', zero_division -> 0) return); labels = union of targets and predictions."""
    t = np.asarray(flat_targets).reshape(-1)
    p = np.asarray(flat_preds).reshape(-1)
    acc = float((t == p).mean()) if t.size else 0.0
    labels = np.union1d(t, p)
    prec, rec, f1 = [], [], []
    for c in labels:
        tp = float(((p == c) & (t == c)).sum())
        pp, tt = float((p == c).sum()), float((t == c).sum())
        pr = tp / pp if pp > 0 else 0.0
        rc = tp / tt if tt > 0 else 0.0
        prec.append(pr)
        rec.append(rc)
        f1.append(2 * pr * rc / (pr + rc) if (pr + rc) > 0 else 0.0)
    return acc, float(np.mean(f1)), float(np.mean(prec)), float(np.mean(rec))
