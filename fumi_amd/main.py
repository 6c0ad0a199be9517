"""CLI driver -- drop-in for ``python fumi/main.py <flags>`` (fumi/main.py:19-156).

    python -m fumi_amd.main --model fumi --dataset synthetic --dropout 0 --batch_size 32 ...
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m fumi_amd.main ...   (episode-sharded)

Same flags (fumi_amd/utils/utils.py), same flag validation and error types, same train -> test flow and logged
metrics.  ``--dataset inat-anim`` reads the reference's files (inat_anim.json + image_embeddings_<model>.hdf5 / .npy) into
HBM-resident tables (fumi_amd/dataset/inat_anim.py) and raises FileNotFoundError when they are absent; ``--dataset
synthetic`` / ``synthetic-resident`` have the same batch contract and need no files; ``--dataset image-npy`` reads uint8
pixels (fumi_amd/dataset/image_table.py) into an HBM-resident table for ``--im_encoder conv4 | resnet12``."""
import os
import random
import sys

import numpy as np
import torch

from . import dist as fdist
from . import engine as _engine
from . import hip
from .models import am3, clip, fumi, maml, metabaseline, pretrain
from .utils import utils
from .utils.wandb_compat import wandb


def get_dataset(args):
    if args.model == "pretrain" and args.dataset not in ("synthetic-resident", "image-npy"):
        raise ValueError(f"--model pretrain trains on a GPU-resident uint8 pixel table: --dataset synthetic-resident or image-npy, "
                         f"not {args.dataset} (embeddings and host loaders have no pixels for the backbone)")
    if args.model == "metabaseline" and args.dataset not in ("synthetic-resident", "image-npy"):
        raise ValueError(f"--model metabaseline trains on a GPU-resident uint8 pixel table: --dataset synthetic-resident or image-npy, "
                         f"not {args.dataset} (embeddings and host loaders have no pixels for the backbone)")
    if args.model == "clip" and args.dataset == "synthetic":        # the CLIP baseline consumes supervised mini-batches
        from .dataset.synthetic import get_synthetic_supervised
        return get_synthetic_supervised(args)
    if args.dataset == "supervised-inat-anim":                       # data.py:54-70
        from .dataset.inat_anim import get_supervised_inat_anim
        return get_supervised_inat_anim(args)
    if args.dataset == "synthetic":
        from .dataset.synthetic import get_synthetic
        return get_synthetic(args)
    if args.dataset == "synthetic-resident":       # same task family, drawn from an HBM-resident table by the GPU sampler
        from .dataset.synthetic import get_synthetic_resident
        return get_synthetic_resident(args)
    if args.dataset == "inat-anim":                # the reference's files (fumi/dataset/data.py) -> HBM-resident tables
        from .dataset.inat_anim import get_inat_anim
        return get_inat_anim(args)
    if args.dataset == "image-npy":                # uint8 pixels from {split}_images.npy -> HBM-resident tables, sampled on the GPU
        from .dataset.image_table import get_image_npy
        return get_image_npy(args)
    raise NotImplementedError()                    # data.py:73-74 ('cub' needs a torchmeta download, 'supervised-inat-anim' is CLIP's)


# embedding width each image model produces (fumi/main.py:34-44: the three ValueErrors, same messages)
_EMBEDDING_DIMS = {"resnet-152": ("Resnet-152", 2048), "resnet-34": ("Resnet-34", 512)}
# names the test metrics are logged and printed under, in the order the test loops return them
_TEST_METRICS = {"maml": ("loss", "acc"), "fumi": ("loss", "acc"), "am3": ("loss", "acc", "f1", "prec", "rec", "avg_lamda"),
                 "pretrain": ("loss", "acc"), "metabaseline": ("loss", "acc")}
_FAMILIES = ("maml", "fumi", "clip", "pretrain", "metabaseline")                                  # unknown names are AM3, like utils.init_model


def _check_embedding_flags(args):
    if args.image_embedding_model not in _EMBEDDING_DIMS:
        raise ValueError("Image embedding model must be one of " + " ".join(_EMBEDDING_DIMS))
    pretty, dim = _EMBEDDING_DIMS[args.image_embedding_model]
    if args.im_emb_dim != dim:
        raise ValueError(f"{pretty} outputs {dim}-dimensional embeddings, hence --im_emb_dim should be set to {dim}")


def _restore(args, model, optimizer):
    """--checkpoint: a file, or (like the reference, main.py:61-76) a W&B run id whose best.pth.tar is fetched first."""
    ckpt = args.checkpoint
    if not os.path.exists(ckpt):
        model_path = f"./checkpoints/{args.model}/{args.checkpoint}"
        os.makedirs(model_path, exist_ok=True)
        ckpt = wandb.restore("best.pth.tar", run_path=f"multimodal-image-cls/{args.model}/{args.checkpoint}",
                             root=model_path).name
    opt = optimizer[0] if type(optimizer) == tuple else optimizer
    return utils.load_checkpoint(model, opt, args.device, ckpt)[0]


def main(args):
    check_supported(args)
    family = args.model if args.model in _FAMILIES else "am3"
    mod = {"maml": maml, "fumi": fumi, "am3": am3, "clip": clip, "pretrain": pretrain, "metabaseline": metabaseline}[family]
    results_path = f"{args.log_dir}/results"
    os.makedirs(results_path, exist_ok=True)
    os.environ["FUMI_LOG_DIR"] = args.log_dir        # where the local W&B stand-in keeps run directories
    os.environ["WANDB_MODE"] = "offline" if args.wandb_offline else "online"
    wandb.init(entity=args.wandb_entity, project=args.wandb_project, group=args.wandb_experiment,
               job_type="eval" if args.evaluate else "train", save_code=True)
    wandb.config.update(args)
    _check_embedding_flags(args)

    train_loader, val_loader, test_loader, dictionary = get_dataset(args)
    if args.augment and not getattr(train_loader, "pixels", False):
        # the reference parses --augment and never reads it; here it acts on a resident pixel table only
        print("--augment is ignored: it applies to a GPU-resident pixel table (--dataset synthetic-resident / image-npy with "
              "--im_encoder conv4 | resnet12), not to embeddings or the host loader")
    if args.augment and getattr(train_loader, "out_size", None) is not None:
        print(f"--augment on a table stored at {tuple(train_loader.images.shape[2:])}: random-resized crop "
              f"(area {train_loader.resize['scale']}, ratio up to {train_loader.resize['ratio']:.4g}), flip and jitter; "
              "--augment_pad is not used")
    max_test_batches = int(args.num_ep_test / args.batch_size)
    for seed_fn in (torch.manual_seed, np.random.seed, random.seed):
        seed_fn(args.seed)

    if family == "pretrain":
        args.n_classes = int(train_loader.n_classes)                     # the head's width: the classes of the train table
    model = utils.init_model(args, dictionary)
    print(model)
    if getattr(args, "encoder_checkpoint", None):                        # the backbone of a --model pretrain checkpoint
        model = utils.load_encoder_checkpoint(model, args.device, args.encoder_checkpoint)
    if getattr(args, "distill_checkpoint", None):                        # the frozen teacher of a --model pretrain run
        model = utils.load_distill_checkpoint(model, args, args.distill_checkpoint)
    optimizer = utils.init_optim(args, model)
    if args.checkpoint:
        model = _restore(args, model, optimizer)
    if family == "clip":                                               # supervised baseline (main.py:86-91,109-111)
        opt = optimizer[0] if type(optimizer) == tuple else optimizer
        if not args.evaluate:
            model = clip.training_run(args, model, opt, train_loader, val_loader, n_epochs=args.epochs)
        test_acc = clip.evaluate(args, model, test_loader)
        print(f"\n TEST: \ntest acc: {test_acc}")
        wandb.log({"test/acc": test_acc})
        wandb.finish()
        return dict(test_acc=float(test_acc))
    if not args.evaluate:
        model = mod.training_run(args, model, optimizer, train_loader, val_loader, max_test_batches // 2)

    out = mod.test_loop(args, model, test_loader, max_test_batches)     # (ends with the device status check)
    names = _TEST_METRICS[family]
    values = dict(zip(names, out))
    print("\n TEST: \n" + ", ".join(f"test {k.replace('_', ' ')}: {v}" for k, v in values.items()))
    wandb.log({f"test/{k}": v for k, v in values.items()})
    result = dict(test_loss=float(values["loss"]), test_acc=float(values["acc"]))
    if family == "am3":
        result["test_f1"] = float(values["f1"])
        test_preds, test_true, query_idx, support_idx, support_lamda = out[len(names):len(names) + 5]
        if fdist.world()[0] == 0:                                        # per-query records (main.py:126-138)
            import pandas as pd
            pd.DataFrame({"support_idx": support_idx, "support_lamda": support_lamda, "query_idx": query_idx,
                          "query_preds": test_preds, "query_targets": test_true}
                         ).to_csv(path_or_buf=f"{results_path}/run_{wandb.run.name}.csv")
    wandb.finish()
    return result


def parse_args(argv=None):
    """Flags -> args (+ args.device, fumi/main.py:141-149).  Pure: nothing here touches the engine, so host-only users of the parser
    (tools, tests, a dry run on a login node) get the same namespace the reference builds."""
    args = utils.relation_parser().parse_args(sys.argv[1:] if argv is None else argv)
    use_gpu = (not args.disable_cuda) and torch.cuda.is_available()
    local = int(os.environ.get("LOCAL_RANK", "0"))
    args.device = torch.device("cuda", local) if use_gpu else torch.device("cpu")
    print(f"running on device {args.device}")
    return args


def check_supported(args):
    """What the reference runs and this engine does not, refused where the engine is first needed (the top of ``main``) instead
    of from inside the first meta-step -- with the reference's exception types where it has one."""
    eng = _engine.get_engine()                  # (raises FumiHipError when the shared object has not been built)
    if args.device.type != "cuda" and not getattr(eng, "runs_on_host", False):
        # the reference falls back to the CPU here (fumi/main.py:145-146); this engine is MI355X-only
        raise hip.FumiHipError(
            ("--disable_cuda was given" if args.disable_cuda else "no GPU is visible (torch.cuda.is_available() is False)")
            + ": fumi_amd has no CPU execution path -- every step runs on the MI355X library "
              "(fumi_amd/lib/libfumi_hip.so).  Run the reference itself for a CPU run.")
    family = args.model if args.model in _FAMILIES else "am3"
    raw = args.im_encoder in ("conv4", "resnet12")
    if family == "pretrain":
        if not raw:
            raise ValueError("--model pretrain trains an image backbone: it needs --im_encoder conv4 or resnet12")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise NotImplementedError("--model pretrain runs on one rank: per-rank batch-statistics groups and the gradient "
                                      "all-reduce of the supervised step are not implemented (WORLD_SIZE > 1)")
        if args.pretrain_bn_group < 1 or args.pretrain_batch < 1 or args.pretrain_batch % (2 * args.pretrain_bn_group) != 0:
            raise ValueError(f"--pretrain_batch {args.pretrain_batch} must be a multiple of 2 * --pretrain_bn_group "
                             f"{args.pretrain_bn_group}: the encoder normalises groups of that many images, half of them on "
                             f"each side of its call")
    if family == "metabaseline":
        if not raw:
            raise ValueError("--model metabaseline trains an image backbone: it needs --im_encoder conv4 or resnet12")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise NotImplementedError("--model metabaseline runs on one rank: episode sharding and the gradient all-reduce of the "
                                      "episodic step are not implemented (WORLD_SIZE > 1)")
    metric, temp = getattr(args, "pretrain_metric", "euclidean"), getattr(args, "metric_temp", 10.0)
    if family != "pretrain" and metric != "euclidean":
        raise ValueError("--pretrain_metric chooses the few-shot validation metric of the supervised classifier: it needs --model pretrain")
    if not temp > 0.0:
        raise ValueError(f"--metric_temp {temp} must be positive")
    head, r_lam, r_scale = (getattr(args, k, d) for k, d in (("fewshot_head", "cosine"), ("ridge_lambda", 50.0), ("ridge_scale", 1.0)))
    if head in ("ridge", "proto", "svm", "matching", "relation") and family != "metabaseline":
        raise ValueError(f"--fewshot_head chooses the episodic classifier of the Meta-Baseline stage: {head} needs --model metabaseline")
    if not r_lam > 0.0:
        raise ValueError(f"--ridge_lambda {r_lam} must be positive")
    if not r_scale > 0.0:
        raise ValueError(f"--ridge_scale {r_scale} must be positive")
    if (head == "ridge" or metric == "ridge") and args.num_ways * args.num_shots > 128:
        raise NotImplementedError(f"the ridge head factors the [S, S] Gram matrix of an episode's support set in LDS: S = --num_ways * "
                                  f"--num_shots = {args.num_ways * args.num_shots} must not exceed 128")
    p_scale, p_fixed = getattr(args, "proto_scale", 1.0), getattr(args, "proto_scale_fixed", False)
    if not p_scale > 0.0:
        raise ValueError(f"--proto_scale {p_scale} must be positive")
    if p_fixed and head != "proto":
        raise ValueError("--proto_scale_fixed fixes the scale of the prototypical head: it needs --fewshot_head proto")
    if head == "proto" and not 2 <= args.num_ways <= 64:
        raise NotImplementedError(f"the prototypical head takes 2 to 64 classes, got --num_ways {args.num_ways}")
    e_head = getattr(args, "eval_head", "train")
    if e_head == "logreg" and family != "metabaseline":
        raise ValueError("--eval_head chooses the validation / test classifier of the Meta-Baseline stage: logreg needs --model "
                         "metabaseline (--model pretrain takes --pretrain_metric logreg)")
    if e_head == "logreg" or metric == "logreg":   # (the --logreg_* values are asked of nothing that does not run the head)
        lg = utils.logreg_config(args)          # (raises ValueError outside the kernel's limits)
        S = args.num_ways * args.num_shots
        if S > 128:
            raise NotImplementedError(f"the logistic-regression head fits on the [S, S] Gram matrix of an episode's support set in LDS: "
                                      f"S = --num_ways * --num_shots = {S} must not exceed 128")
        if not 2 <= args.num_ways <= 64:
            raise NotImplementedError(f"the logistic-regression head takes 2 to 64 classes, got --num_ways {args.num_ways}")
        wd = 1.0 / (lg["C"] * max(S, 1))
        if lg["normalize"] and lg["lr"] * (1.0 + wd) >= 2.0 * (1.0 + lg["momentum"]):
            raise ValueError(f"--logreg_lr {lg['lr']} can diverge: on L2-normalised rows with a bias the curvature of the mean "
                             f"cross-entropy is at most 1, so the objective's is at most 1 + wd with wd = 1 / (--logreg_C * S) = {wd:.4g}, "
                             f"and the heavy-ball iteration is stable only for lr * (1 + wd) < 2 * (1 + --logreg_momentum) = "
                             f"{2.0 * (1.0 + lg['momentum']):.4g}")
    sv = utils.svm_config(args)                 # (raises ValueError for a non-positive --svm_C / --svm_eps / --svm_scale, a step count outside the kernel's limits)
    if head != "svm" and metric != "svm":
        moved = utils.svm_flags_moved(args)
        if moved:
            raise ValueError(f"{', '.join(moved)} set the MetaOptNet-SVM head: they need --fewshot_head svm or --pretrain_metric svm")
    else:
        if head != "svm" and sv["bwd_steps"] != 40:
            raise ValueError("--svm_bwd_steps counts the conjugate-gradient steps of the SVM head's backward: it needs --fewshot_head svm "
                             "(--pretrain_metric svm runs the forward form only)")
        S = args.num_ways * args.num_shots
        if S > 128:
            raise NotImplementedError(f"the SVM head fits on the [S, S] Gram matrix of an episode's support set in LDS: S = --num_ways * "
                                      f"--num_shots = {S} must not exceed 128")
        if not 2 <= args.num_ways <= 64:
            raise NotImplementedError(f"the SVM head takes 2 to 64 classes, got --num_ways {args.num_ways}")
    t_steps = getattr(args, "transductive_steps", 0)
    if not 0 <= t_steps <= 100:
        raise ValueError(f"--transductive_steps {t_steps} must lie in [0, 100]")
    if head == "matching" or metric == "matching":
        # the limits of fumi_hip_match_head_step (csrc/matchhead.hip): a tile's scores against every support row are held in LDS
        S = args.num_ways * args.num_shots
        if not 1 <= S <= 512:
            raise NotImplementedError(f"the matching head holds a query tile's scores against every support row in LDS: S = --num_ways * "
                                      f"--num_shots = {S} must lie in [1, 512]")
        if not 2 <= args.num_ways <= 64:
            raise NotImplementedError(f"the matching head takes 2 to 64 classes, got --num_ways {args.num_ways}")
        if t_steps > 0:
            raise ValueError("--fewshot_head matching / --pretrain_metric matching attends over the support rows and has no class "
                             f"prototypes for the transductive refinement to move: --transductive_steps must be 0, got {t_steps}")
        if getattr(args, "fewshot_adapt", "none") == "feat":
            raise ValueError("--fewshot_head matching attends over the support rows and has no class prototypes for --fewshot_adapt "
                             "feat to adapt: it goes with --fewshot_adapt none")
    r_hid, r_loss = getattr(args, "relation_hidden", 256), getattr(args, "relation_loss", "mse")
    if head != "relation" and (r_hid != 256 or r_loss != "mse"):
        raise ValueError("--relation_hidden / --relation_loss set the Relation Network head: they need --fewshot_head relation")
    if head == "relation":
        # the limits of fumi_hip_relation_head_step (csrc/relationhead.hip)
        if r_loss not in ("mse", "ce"):
            raise ValueError(f"--relation_loss {r_loss} must be mse or ce")
        if t_steps > 0:
            raise ValueError("--fewshot_head relation scores (class mean, query) pairs with a learned module and has no metric for the "
                             f"transductive refinement to move prototypes in: --transductive_steps must be 0, got {t_steps}")
        if getattr(args, "fewshot_adapt", "none") == "feat":
            raise ValueError("--fewshot_head relation does not take adapted prototypes: it goes with --fewshot_adapt none, not "
                             "--fewshot_adapt feat")
        if r_hid % 32 != 0 or not 32 <= r_hid <= 1024:
            raise NotImplementedError(f"the relation head takes a hidden width in multiples of 32 from 32 to 1024, got --relation_hidden "
                                      f"{r_hid}")
        if not 2 <= args.num_ways <= 64:
            raise NotImplementedError(f"the relation head takes 2 to 64 classes, got --num_ways {args.num_ways}")
        S = args.num_ways * args.num_shots
        if not 1 <= S <= 1024:
            raise NotImplementedError(f"the relation head stages an episode's support labels in LDS: S = --num_ways * --num_shots = {S} "
                                      "must lie in [1, 1024]")
    if t_steps > 0:
        if family not in ("metabaseline", "pretrain"):
            raise ValueError("--transductive_steps refines the class prototypes of a nearest-centroid few-shot evaluation: it needs "
                             "--model metabaseline or pretrain")
        if head in ("ridge", "svm") or e_head == "logreg" or metric in ("ridge", "logreg", "svm"):
            raise ValueError("--transductive_steps refines class prototypes: it goes with the cosine and the Euclidean metric, not with "
                             "--fewshot_head ridge | svm, --eval_head logreg or --pretrain_metric ridge | logreg | svm")
        # the limits of fumi_hip_trans_proto_step (csrc/transproto.hip): w and the query rows of G of an episode are held in LDS
        S, Qn = args.num_ways * args.num_shots, args.num_ways * args.num_shots_test
        if not 2 <= args.num_ways <= 64:
            raise NotImplementedError(f"the transductive head takes 2 to 64 classes, got --num_ways {args.num_ways}")
        if S < 1 or Qn < 1 or S + Qn > 512 or Qn * args.num_ways > 8192:
            raise NotImplementedError(f"the transductive head holds an episode's soft assignments in LDS: S + Qn = --num_ways * "
                                      f"(--num_shots + --num_shots_test) = {S + Qn} must not exceed 512 and Qn * --num_ways = "
                                      f"{Qn * args.num_ways} must not exceed 8192")
    adapt = getattr(args, "fewshot_adapt", "none")
    if adapt not in ("none", "feat"):
        raise ValueError(f"--fewshot_adapt {adapt} must be none or feat")
    if adapt == "feat":
        if family != "metabaseline":
            raise ValueError("--fewshot_adapt adapts the class prototypes of the Meta-Baseline stage: feat needs --model metabaseline")
        if head not in ("cosine", "proto"):
            raise ValueError(f"--fewshot_adapt feat adapts class prototypes: it goes with --fewshot_head cosine or proto, not {head} "
                             "(the ridge and the SVM head fit on the support rows, not on prototypes)")
        if e_head == "logreg":
            raise ValueError("--fewshot_adapt feat classifies against the adapted prototypes: --eval_head logreg fits on the support "
                             "rows and would not see them")
        if t_steps > 0:
            raise ValueError("--fewshot_adapt feat is inductive: the transductive refinement starts from the plain class means, so "
                             "--transductive_steps must be 0")
        if not 2 <= args.num_ways <= 64:
            raise NotImplementedError(f"the prototype adaptation takes 2 to 64 classes, got --num_ways {args.num_ways}")
    d_rate, d_bs, d_nb, d_an = (getattr(args, k, d) for k, d in (("drop_rate", 0.0), ("drop_block_size", 5), ("drop_blocks", 2),
                                                                   ("drop_anneal_steps", 40000)))
    if not 0.0 <= d_rate < 1.0:
        raise ValueError(f"--drop_rate {d_rate} must lie in [0, 1)")
    if d_rate == 0.0 and (d_bs != 5 or d_nb != 2 or d_an != 40000):
        raise ValueError("--drop_block_size, --drop_blocks and --drop_anneal_steps shape the DropBlock / dropout regulariser: they "
                         "need --drop_rate > 0")
    if d_rate > 0.0:
        if family in ("fumi", "maml"):
            raise NotImplementedError(f"--drop_rate with --model {family}: DropBlock / dropout is built into the first-order encoder "
                                      "pair; the second-order FuMI / MAML ResNet-12 steps are out of scope and run without it")
        if family not in ("pretrain", "metabaseline"):
            raise NotImplementedError(f"--drop_rate with --model {args.model}: the regulariser is wired into the training steps of "
                                      "--model pretrain and metabaseline only")
        if args.im_encoder != "resnet12":
            raise NotImplementedError(f"--drop_rate is DropBlock / dropout inside the ResNet-12 encoder: it needs --im_encoder resnet12, "
                                      f"got {args.im_encoder}")
        if not 1 <= d_bs <= 8:
            raise ValueError(f"--drop_block_size {d_bs} must lie in [1, 8]")
        if not 0 <= d_nb <= 4:
            raise ValueError(f"--drop_blocks {d_nb} must lie in [0, 4]")
        if d_an < 0:
            raise ValueError(f"--drop_anneal_steps {d_an} must not be negative")
        if d_bs > 1 and d_nb > 0 and (args.image_size >> (4 - d_nb + 1)) > 64:
            raise NotImplementedError(f"DropBlock holds a row of the map in one 64-bit word: the first DropBlock block's pooled map "
                                      f"({args.image_size >> (4 - d_nb + 1)} wide at --image_size {args.image_size}) must be at most 64 wide")
    eps, a_mix, a_cut, p_mix = (getattr(args, k, d) for k, d in (("label_smoothing", 0.0), ("mixup_alpha", 0.0),
                                                                    ("cutmix_alpha", 0.0), ("mix_prob", 1.0)))
    if family != "pretrain" and (eps != 0.0 or a_mix != 0.0 or a_cut != 0.0 or p_mix != 1.0):
        raise ValueError("--label_smoothing, --mixup_alpha, --cutmix_alpha and --mix_prob regularise the supervised classifier: "
                         "they need --model pretrain")
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"--label_smoothing {eps} must lie in [0, 1)")
    if a_mix < 0 or a_cut < 0:
        raise ValueError(f"--mixup_alpha {a_mix} and --cutmix_alpha {a_cut} must not be negative (0 turns the mix off)")
    if not 0.0 <= p_mix <= 1.0:
        raise ValueError(f"--mix_prob {p_mix} must lie in [0, 1]")
    d_ckpt, d_temp, d_alpha, d_ce = (getattr(args, k, d) for k, d in (("distill_checkpoint", None), ("distill_temp", 4.0),
                                                                       ("distill_alpha", 0.5), ("distill_ce_weight", 0.5)))
    d_moved = d_temp != 4.0 or d_alpha != 0.5 or d_ce != 0.5
    if family != "pretrain" and (d_ckpt or d_moved):
        raise ValueError("--distill_checkpoint, --distill_temp, --distill_alpha and --distill_ce_weight distil the supervised "
                         "classifier from a teacher: they need --model pretrain")
    if d_moved and not d_ckpt:
        raise ValueError("--distill_temp, --distill_alpha and --distill_ce_weight weigh the distillation from a teacher: they need "
                         "--distill_checkpoint")
    if not d_temp > 0.0 or not d_temp < float("inf"):
        raise ValueError(f"--distill_temp {d_temp} must be positive and finite")
    if not 0.0 <= d_alpha < float("inf") or not 0.0 <= d_ce < float("inf"):
        raise ValueError(f"--distill_alpha {d_alpha} and --distill_ce_weight {d_ce} must not be negative")
    c_head, c_scale, c_fixed = (getattr(args, k, d) for k, d in (("pretrain_head", "linear"), ("pretrain_head_scale", 10.0),
                                                                  ("pretrain_head_scale_fixed", False)))
    if family != "pretrain" and (c_head != "linear" or c_scale != 10.0 or c_fixed):
        raise ValueError("--pretrain_head, --pretrain_head_scale and --pretrain_head_scale_fixed choose the classifier of the "
                         "supervised stage: they need --model pretrain")
    if not (c_scale > 0.0 and c_scale < float("inf")):
        raise ValueError(f"--pretrain_head_scale {c_scale} must be positive and finite")
    if c_head != "cosine" and (c_scale != 10.0 or c_fixed):
        raise ValueError("--pretrain_head_scale and --pretrain_head_scale_fixed set the scale of the cosine classifier: they need "
                         "--pretrain_head cosine")
    if c_head == "cosine" and d_ckpt:
        raise NotImplementedError("--distill_checkpoint with --pretrain_head cosine: the distillation head is a form of the linear "
                                  "head, a cosine student or teacher is not implemented")
    if d_ckpt and not os.path.isfile(d_ckpt):
        raise ValueError(f"--distill_checkpoint {d_ckpt} does not exist")
    if getattr(args, "encoder_checkpoint", None) and (family == "clip" or not raw):
        raise ValueError("--encoder_checkpoint loads a Conv4 / ResNet-12 backbone: it needs --model fumi, maml, am3 or metabaseline "
                         "with --im_encoder conv4 or resnet12")
    # (--fine_tune with --text_encoder RNN / RNNhid trains the bi-LSTM like the reference, fumi/models/fumi.py:65-67 / am3.py:74-76:
    # every meta-step hands back the adjoint of its text input, csrc/textenc.hip runs the LSTM's backward)
    if (family == "am3" and args.text_encoder == "rand" and args.dropout > 0 and not args.evaluate
            and not getattr(eng, "am3_rand_native", False)):
        # fumi/models/am3.py:118-126 applies dropout inside h only.  The engine's text-rows form of the step (am3_step_tx) does that;
        # an engine without it runs `rand` through an identity in g's place, whose hidden layer the step's dropout would hit too: there
        # training this combination needs --dropout 0 (the CLI default is 0.25)
        raise NotImplementedError("--model am3 --text_encoder rand trains only with --dropout 0 on this engine "
                                  "(the step's dropout would also hit the identity that stands in for g)")


def _maybe_init_distributed(args):
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and not torch.distributed.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.device.type == "cuda":
            torch.cuda.set_device(args.device)
            torch.distributed.init_process_group("nccl", device_id=args.device)
        else:
            torch.distributed.init_process_group("gloo")


if __name__ == "__main__":
    _args = parse_args()
    _maybe_init_distributed(_args)
    main(_args)
