"""Supervised pre-training of the image backbone (``--model pretrain``).

The few-shot recipes this code base follows (AM3's own paper, every ResNet-12 baseline since) train the backbone first as a plain
classifier over all training classes and carry those weights into the episodic model.  ``Pretrain`` is that classifier: the same
``Conv4`` / ``ResNet12`` module AM3 builds, under the same attribute name (``conv``, so ``state_dict`` keys ``conv.*``), and
``classifier = nn.Linear(feature_dim, n_classes)``.

A training step runs on the engine's first-order encoder pair and the fused classification head (csrc/clshead.hip): the M images
of a batch are laid out as B = M / (2 R) episodes of R "support" and R "query" images, the first half of the batch on the support
side, so that the unchanged encode call normalises every R consecutive images by their own batch statistics (R =
``--pretrain_bn_group``); ``cls_head_step`` takes all M feature rows, ``encode_bwd`` the two halves of its ``dfeats``.
Validation and test are few-shot nearest-centroid classification on backbone features over the episodic batches the pixel samplers
produce: the checkpoint with the best few-shot validation loss wins.  ``--encoder_checkpoint`` (fumi_amd/utils/utils.py) loads the
``conv.*`` tensors of such a checkpoint into ``--model fumi | maml | am3``.

Born-again distillation: ``Pretrain(distill=dict(temp=, alpha=, ce_weight=))`` with ``load_teacher(state_dict)``
trains the classifier as the student of a frozen copy of an earlier generation.  Every step encodes the batch with the teacher first
(no tape), then with the student (taped), and the distillation form of the head (``cls_head_step_distill``) takes both feature sets.

The cosine classifier: ``Pretrain(head="cosine")`` (``--pretrain_head cosine``) trains the backbone in the metric a
cosine few-shot stage compares in: ``classifier = nn.Linear(feature_dim, n_classes, bias=False)`` and one scale ``cls_scale`` [1], a
parameter, or with ``head_scale_fixed`` a persistent buffer; the logits are ``cls_scale * cos(feats_m, classifier.weight_c)``.  Every
training step runs the fused cosine head (``cos_cls_head_step``, csrc/coshead.hip), whose soft form covers label smoothing and the
two-label mixes.  ``head="linear"`` is the model it was."""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import engine as _engine
from .. import lazy
from ..flatgrad import FlatGrads, ParamWatch
from ..optim import clip_log
from ..utils import utils as utils
from ..utils.average_meter import AverageMeter
from ..utils.wandb_compat import wandb
from .common import _loss_acc


class Pretrain(nn.Module):
    def __init__(self, im_encoder, image_size=84, image_channels=3, n_classes=64, bn_group=64, num_ways=None, label_smoothing=0.0,
                 metric="euclidean", metric_temp=10.0, ridge_lambda=50.0, ridge_scale=1.0, logreg=None, transductive_steps=0,
                 distill=None, svm=None, head="linear", head_scale=10.0, head_scale_fixed=False, drop=None):
        super().__init__()
        if drop is not None and im_encoder != "resnet12":
            raise NotImplementedError("DropBlock / dropout on the block outputs is built into the ResNet-12 encoder pair: drop= needs "
                                      "im_encoder resnet12")
        self.drop = None                                   # DropSchedule of the training steps, None: no drop
        self.drop_step = 0                                 # the training loop's step index: the mask seed and the annealed rate follow it
        if head not in ("linear", "cosine"):
            raise ValueError(f"the classifier head must be linear or cosine, got {head}")
        if not (math.isfinite(float(head_scale)) and float(head_scale) > 0.0):
            raise ValueError(f"the scale of the cosine classifier must be positive, got {head_scale}")
        if head != "cosine" and (head_scale_fixed or float(head_scale) != 10.0):
            raise ValueError(f"the classifier scale belongs to the cosine head, got head {head}")
        if head == "cosine" and distill is not None:
            raise NotImplementedError("the distillation head is a form of the linear head: a cosine student or teacher is not implemented")
        self.head = head                                   # the training classifier (section 41); the few-shot metric is chosen apart
        self.head_scale_fixed = bool(head_scale_fixed)
        self.svm_cfg = utils.svm_config(svm)               # fixed hyper-parameters of the SVM metric (section 39)
        self._svm = None
        self.distill = distill_config(distill)             # None, or the weights of the distillation loss (section 37)
        self.last_out = None                               # the head's output dict of the last training step
        object.__setattr__(self, "_teacher", None)         # (conv module, [W_t, b_t]) once loaded: frozen, outside parameters() / state_dict()
        self._tcache = None
        if metric not in ("euclidean", "cosine", "ridge", "logreg", "svm", "matching"):
            raise ValueError(f"the few-shot metric must be euclidean, cosine, ridge, logreg, svm or matching, got {metric}")
        if not 0 <= int(transductive_steps) <= 100:
            raise ValueError(f"the transductive refinement takes 0 to 100 steps, got {transductive_steps}")
        if int(transductive_steps) > 0 and metric in ("ridge", "logreg", "svm", "matching"):
            raise ValueError(f"the transductive refinement moves class prototypes: it goes with the euclidean and the cosine metric, got {metric}")
        self.transductive_steps = int(transductive_steps)   # soft k-means steps of the few-shot evaluation (section 36; 0: inductive)
        self._one = None
        self.logreg = utils.logreg_config(logreg)          # fixed hyper-parameters of the logistic-regression metric (section 34)
        if not (float(ridge_lambda) > 0.0 and float(ridge_scale) > 0.0):
            raise ValueError(f"the ridge weight and the logit scale of the ridge metric must be positive, got {ridge_lambda}, {ridge_scale}")
        self.ridge_lambda, self.ridge_scale = float(ridge_lambda), float(ridge_scale)   # fixed values of the ridge metric (section 33)
        self._ridge = None
        if not float(metric_temp) > 0.0:
            raise ValueError(f"the temperature of the cosine metric must be positive, got {metric_temp}")
        self.metric, self.metric_temp = metric, float(metric_temp)   # few-shot validation / test metric
        self._tau = None
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError(f"label_smoothing must lie in [0, 1), got {label_smoothing}")
        self.label_smoothing = float(label_smoothing)     # eps of the training target; evaluation has none
        self.backbone = im_encoder
        if im_encoder == "conv4":
            from .conv4 import Conv4
            self.conv = Conv4(image_channels, 64, 4, image_size)
        elif im_encoder == "resnet12":
            from .resnet12 import CHANNELS, ResNet12
            self.conv = ResNet12(image_channels, CHANNELS, image_size)
        else:
            raise NameError(f"{im_encoder} not allowed as image encoder of --model pretrain (conv4, resnet12)")
        if drop is not None:
            from .resnet12 import DropSchedule
            self.drop = DropSchedule(n_blocks=self.conv.n_blocks, **drop)
        self.n_classes = int(n_classes)
        self.bn_group = int(bn_group)          # R: images per batch-statistics group of a training step
        self.num_ways = num_ways               # N of the validation / test episodes (None: read from the labels)
        self.classifier = nn.Linear(self.conv.feature_dim, self.n_classes, bias=head == "linear")
        if head == "cosine" and self.head_scale_fixed:
            self.register_buffer("cls_scale", torch.tensor([float(head_scale)]))
        elif head == "cosine":
            self.cls_scale = nn.Parameter(torch.tensor([float(head_scale)]))
        self._dscale = None
        self._image = (int(image_channels), int(image_size))
        self._flat = None
        self._pcache = None

    def backbone_module(self):
        return self.conv

    def _head_params(self):
        """The classifier's own parameters, in the order of the flat gradient buffer: weight and bias of the linear head; weight and
        ``cls_scale`` of the cosine head, the weight alone where that scale is fixed (a buffer)."""
        if self.head == "linear":
            return [self.classifier.weight, self.classifier.bias]
        return [self.classifier.weight] + ([] if self.head_scale_fixed else [self.cls_scale])

    def _step_params(self, need_grad):
        """(detached classifier weight and bias | weight and scale, detached backbone tensors, flat gradient buffer | None), the same
        objects from step to step; rebuilt when a parameter object was replaced or moved (``_apply``)."""
        c = self._pcache
        fixed = self.head == "cosine" and self.head_scale_fixed
        if c is None or not c[0].valid() or (fixed and c[1][1] is not self._buffers["cls_scale"]):
            w, th = self._head_params(), self.conv.theta()
            c = self._pcache = (ParamWatch(self, w + th), [p.detach() for p in w] + ([self._buffers["cls_scale"]] if fixed else []),
                                [p.detach() for p in th])
            self._flat = None
        fg = None
        if need_grad:
            fg = self._flat
            if fg is None:
                fg = self._flat = FlatGrads(self._head_params() + self.conv.theta(), extra=2)
                # the fixed scale has no slot in the flat buffer: its gradient is written beside it and read by nobody
                self._dscale = torch.empty(1, device=fg.flat.device, dtype=torch.float32) if fixed else None
        return c[1], c[2], fg

    def _apply(self, fn, recurse=True):
        self._pcache = None
        self._tcache = None
        if self._teacher is not None:                      # the teacher moves with the model
            conv_t, w_t = self._teacher
            conv_t._apply(fn)
            object.__setattr__(self, "_teacher", (conv_t, [fn(t) for t in w_t]))
        return super()._apply(fn, recurse)

    def _new_backbone(self):
        if self.backbone == "conv4":
            from .conv4 import Conv4
            return Conv4(self._image[0], 64, 4, self._image[1])
        from .resnet12 import CHANNELS, ResNet12
        return ResNet12(self._image[0], CHANNELS, self._image[1])

    def load_teacher(self, state_dict):
        """The frozen teacher of the distillation loss from a ``--model pretrain`` state_dict: a second backbone of this model's class
        (``conv.*``) and its classifier (``classifier.weight``, ``classifier.bias``), on the device of the model.  A tensor that is
        missing or of another shape is a ValueError naming it.  The teacher is no submodule: it appears in neither ``parameters()``,
        ``state_dict()``, the flat gradient buffer nor the optimizer."""
        if self.distill is None:
            raise ValueError("load_teacher needs a model built with distill=dict(temp=, alpha=, ce_weight=)")
        if "cls_scale" in state_dict:
            raise ValueError("the teacher's state_dict holds cls_scale: it was trained with the cosine classifier, which the "
                             "distillation head (a form of the linear head) cannot take as a teacher")
        conv_t = self._new_backbone()
        own = {"conv." + k: v for k, v in conv_t.state_dict().items()}
        own["classifier.weight"], own["classifier.bias"] = self.classifier.weight, self.classifier.bias
        for name, dst in own.items():
            src = state_dict.get(name)
            if src is None:
                raise ValueError(f"the teacher's state_dict has no tensor {name}")
            if tuple(src.shape) != tuple(dst.shape):
                raise ValueError(f"the teacher's tensor {name} is {tuple(src.shape)}, the student's is {tuple(dst.shape)}")
        dev = self.classifier.weight.device
        conv_t.load_state_dict({k[5:]: state_dict[k] for k in own if k.startswith("conv.")})
        conv_t.to(dev).requires_grad_(False)
        w_t = [state_dict[k].detach().to(device=dev, dtype=torch.float32).clone().contiguous() for k in ("classifier.weight", "classifier.bias")]
        object.__setattr__(self, "_teacher", (conv_t, w_t))
        self._tcache = None
        return self

    def _teacher_params(self):
        """(detached teacher classifier [W_t, b_t], detached teacher backbone tensors), cached until the model moves."""
        if self._tcache is None:
            conv_t, w_t = self._teacher
            self._tcache = (w_t, [p.detach() for p in conv_t.theta()])
        return self._tcache

    def _encoders(self, eng):
        return ((eng.conv4_encode, eng.conv4_encode_bwd) if self.backbone == "conv4" else
                (eng.resnet12_encode, eng.resnet12_encode_bwd))

    def train_step(self, x, y, optimizer=None, scheduler=None, y_b=None, lam=1.0):
        """One supervised step on x [M, C, H, W] fp32, y [M] int64; returns the head's output dict (loss, correct, preds, gradients).
        The gradients are left attached to the parameters; with an optimizer its fused step follows.  y_b [M] int64 and lam: the second
        label of every row and the weight of the first (a mixup / CutMix batch); with them, or with label_smoothing > 0, the head runs
        in its soft-target form, and ``correct`` counts against y."""
        eng = _engine.get_engine()
        M, R = int(x.shape[0]), self.bn_group
        if M % (2 * R) != 0:
            raise ValueError(f"a batch of {M} images does not split into groups of 2 * {R} (--pretrain_batch must be a multiple of "
                             f"2 * --pretrain_bn_group)")
        B, half = M // (2 * R), M // 2
        w, theta, fg = self._step_params(True)
        encode, encode_bwd = self._encoders(eng)
        x = x.contiguous()
        x_s, x_q = x[:half].view(B, R, *x.shape[1:]), x[half:].view(B, R, *x.shape[1:])
        feats_t = None
        if self.distill is not None:
            if self._teacher is None:
                raise RuntimeError("Pretrain(distill=...) has no teacher: call load_teacher(state_dict) (--distill_checkpoint) before "
                                   "the first training step")
            # the teacher first: its untaped encode uses the encoder's workspace, which must stay untouched between the student's taped
            # encode and its backward.  The same x as the student's (mixed images included), the same batch-statistics groups.
            w_t, theta_t = self._teacher_params()
            t_s, t_q = encode(x_s, x_q, theta_t, keep_tape=False)
            feats_t = torch.cat((t_s.view(half, -1), t_q.view(half, -1)))
        # the student's training encode alone drops (the teacher above, validation, test and few_shot never do)
        drop = self.drop.args(self.drop_step) if self.drop is not None and self.drop.rate_at(self.drop_step) > 0.0 else None
        if drop is not None:
            f_s, f_q = eng.resnet12_encode_drop(x_s, x_q, theta, *drop, keep_tape=True)
        else:
            f_s, f_q = encode(x_s, x_q, theta, keep_tape=True)
        feats = torch.cat((f_s.view(half, -1), f_q.view(half, -1)))                 # [M, F], the images' order
        g_w, g_theta = fg.split(len(w) - 1 if self.head == "cosine" and self.head_scale_fixed else len(w))
        if self.head == "cosine":
            out = eng.cos_cls_head_step(feats, y, w[0], w[1], y_b=y_b, lam=float(lam), smoothing=self.label_smoothing, need_grad=True,
                                        grad_scale=1.0, gW=g_w[0], dtau=self._dscale if self.head_scale_fixed else g_w[1])
        elif feats_t is not None:
            out = eng.cls_head_step_distill(feats, y, w[0], w[1], feats_t, w_t[0], w_t[1], temp=self.distill["temp"],
                                            alpha=self.distill["alpha"], ce_weight=self.distill["ce_weight"], y_b=y_b,
                                            lam=float(lam), smoothing=self.label_smoothing, need_grad=True, grad_scale=1.0,
                                            gW=g_w[0], gb=g_w[1])
        elif self.label_smoothing > 0 or y_b is not None:
            out = eng.cls_head_step_soft(feats, y, w[0], w[1], y_b=y_b, lam=float(lam), smoothing=self.label_smoothing, need_grad=True,
                                         grad_scale=1.0, gW=g_w[0], gb=g_w[1])
        else:
            out = eng.cls_head_step(feats, y, w[0], w[1], need_grad=True, grad_scale=1.0, gW=g_w[0], gb=g_w[1])
        df = out["dfeats"]
        if drop is not None:
            eng.resnet12_encode_bwd_drop(x_s, x_q, df[:half].view(B, R, -1), df[half:].view(B, R, -1), theta, *drop, scale=1.0,
                                         g_theta=g_theta)
        else:
            encode_bwd(x_s, x_q, df[:half].view(B, R, -1), df[half:].view(B, R, -1), theta, scale=1.0, g_theta=g_theta)
        torch.cat((out["loss"], out["correct"] / M), out=fg.tail)
        if optimizer is not None:
            optimizer.zero_grad()
        fg.attach()
        if optimizer is not None:
            getattr(optimizer, "step_fused", optimizer.step)()
            if scheduler:
                scheduler.step()
        self.last_out = out
        return out

    def few_shot(self, batch, device):
        """(loss, acc) of nearest-centroid classification on backbone features over one episodic meta-batch: class means of the support
        features (proto_reduce), squared Euclidean distances, softmax cross-entropy on their negatives (prototypical_loss), arg-min.
        With ``metric == "cosine"``: one forward call of the fused cosine head (cos_proto_step) at the fixed temperature; with
        ``metric == "ridge"``: one forward call of the ridge-regression head (ridge_head_step) at the fixed ridge weight and scale; with
        ``metric == "logreg"``: one forward call of the logistic-regression head (logreg_head_step) at the fixed hyper-parameters; with
        ``metric == "svm"``: one forward call of the MetaOptNet-SVM head (svm_head_step) at the fixed C, eps, scale and step count; with
        ``metric == "matching"``: one forward call of the Matching Networks head (match_head_step) at the fixed temperature.
        With ``transductive_steps > 0``: one call of the transductive head (trans_proto_step), cosine at the fixed temperature or
        squared Euclidean at scale 1."""
        eng = _engine.get_engine()
        (_, _, s_im), s_y = batch['train']
        (_, _, q_im), q_y = batch['test']
        to = lambda t: t.to(device).contiguous()
        x_s, x_q, y_s, y_q = to(s_im).float(), to(q_im).float(), to(s_y), to(q_y)
        _, theta, _ = self._step_params(False)
        f_s, f_q = self._encoders(eng)[0](x_s, x_q, theta, keep_tape=False)
        N = int(self.num_ways) if self.num_ways else int(y_s.max().item()) + 1
        if self.transductive_steps > 0:
            if self.metric == "cosine":
                if self._tau is None or self._tau.device != f_s.device:
                    self._tau = torch.tensor([self.metric_temp], device=f_s.device, dtype=torch.float32)
                scale, trans_metric = self._tau, "cosine"
            else:
                if self._one is None or self._one.device != f_s.device:
                    self._one = torch.ones(1, device=f_s.device, dtype=torch.float32)
                scale, trans_metric = self._one, "euclid"
            out = eng.trans_proto_step(f_s, y_s, f_q, y_q, scale, metric=trans_metric, steps=self.transductive_steps, n_way=N)
            return _loss_acc(out, y_q)
        if self.metric in ("cosine", "matching"):
            if self._tau is None or self._tau.device != f_s.device:
                self._tau = torch.tensor([self.metric_temp], device=f_s.device, dtype=torch.float32)
            step = eng.match_head_step if self.metric == "matching" else eng.cos_proto_step
            out = step(f_s, y_s, f_q, y_q, self._tau, need_grad=False, n_way=N)
            return _loss_acc(out, y_q)
        if self.metric == "ridge":
            if self._ridge is None or self._ridge.device != f_s.device:
                self._ridge = torch.tensor([math.log(self.ridge_lambda), self.ridge_scale], device=f_s.device, dtype=torch.float32)
            out = eng.ridge_head_step(f_s, y_s, f_q, y_q, self._ridge, need_grad=False, n_way=N)
            return _loss_acc(out, y_q)
        if self.metric == "logreg":
            out = eng.logreg_head_step(f_s, y_s, f_q, y_q, n_way=N, **self.logreg)
            return _loss_acc(out, y_q)
        if self.metric == "svm":
            if self._svm is None or self._svm.device != f_s.device:
                self._svm = torch.tensor([self.svm_cfg["scale"]], device=f_s.device, dtype=torch.float32)
            c = self.svm_cfg
            out = eng.svm_head_step(f_s, y_s, f_q, y_q, self._svm, C=c["C"], eps=c["eps"], steps=c["steps"], need_grad=False, n_way=N)
            return _loss_acc(out, y_q)
        protos = eng.proto_reduce(f_s, y_s, N)                                       # [B, N, F]
        d2 = ((f_q[:, :, None, :] - protos[:, None, :, :]) ** 2).sum(-1)              # [B, Qn, N]
        loss = F.cross_entropy(-d2.reshape(-1, N), y_q.reshape(-1))
        acc = (d2.argmin(-1) == y_q).float().mean()
        return torch.stack((loss, acc))

    def evaluate(self, batch, optimizer, scheduler, device, task="train"):
        """``train``: one supervised step on batch = (x, y) or, from a mixing batch source, (x, y_a, y_b, lam); returns (loss, acc) of
        the batch (acc against y_a); ``val`` / ``test``: few-shot nearest-centroid (loss, acc) of one episodic meta-batch."""
        device = torch.device(device) if not isinstance(device, torch.device) else device
        if task == "train" and torch.is_grad_enabled():
            if not self.training:
                self.train()
            if len(batch) == 4:
                x, y, y_b, lam = batch
                self.train_step(x.to(device).float(), y.to(device), optimizer, scheduler, y_b=y_b.to(device), lam=lam)
            else:
                x, y = batch
                self.train_step(x.to(device).float(), y.to(device), optimizer, scheduler)
            return lazy.scalars(self._flat.tail, 2)
        if self.training:
            self.eval()
        with torch.no_grad():
            loss, acc = self.few_shot(batch, device).cpu().numpy()
        return loss, acc


def distill_config(cfg):
    """None, or dict(temp, alpha, ce_weight) of the distillation loss as floats, checked: temp positive, the weights not negative."""
    if cfg is None:
        return None
    c = dict(temp=float(cfg.get("temp", 4.0)), alpha=float(cfg.get("alpha", 0.5)), ce_weight=float(cfg.get("ce_weight", 0.5)))
    if not (math.isfinite(c["temp"]) and c["temp"] > 0.0):
        raise ValueError(f"the distillation temperature must be positive, got {c['temp']}")
    if not (math.isfinite(c["alpha"]) and c["alpha"] >= 0.0 and math.isfinite(c["ce_weight"]) and c["ce_weight"] >= 0.0):
        raise ValueError(f"the distillation weights must not be negative, got alpha {c['alpha']}, ce_weight {c['ce_weight']}")
    return c


def head_log(model):
    """cls_scale of the cosine classifier, else nothing."""
    if getattr(model, "head", "linear") != "cosine":
        return {}
    return {"cls_scale": float(model.cls_scale.detach()[0])}


def distill_log(model):
    """train/loss_ce, train/loss_kd and train/teacher_agree (a fraction of the batch) of the last distillation step, else nothing."""
    out = getattr(model, "last_out", None)
    if not out or "loss_kd" not in out:
        return {}
    return {"train/loss_ce": float(out["loss_ce"]), "train/loss_kd": float(out["loss_kd"]),
            "train/teacher_agree": float(out["agree"]) / max(int(out["preds"].numel()), 1)}


def training_run(args, model, optimizer, train_loader, val_loader, max_test_batches):
    """The structure of am3.training_run: validation at batch 0 and every --eval_freq, the usual checkpoint dictionary, patience,
    reload of the best checkpoint (best few-shot validation loss) at the end."""
    best_loss, best_acc = test_loop(args, model, val_loader, max_test_batches)
    print(f"\ninitial loss: {best_loss}, acc: {best_acc}")
    best_batch_idx = 0
    opt, scheduler = optimizer if type(optimizer) == tuple else (optimizer, None)
    try:
        for batch_idx, batch in enumerate(train_loader):
            model.drop_step = batch_idx                    # (--drop_rate: the step's mask seed and annealed rate)
            tl, ta = model.evaluate(batch=batch, optimizer=opt, scheduler=scheduler, device=args.device, task="train")
            wandb.log({"train/acc": ta, "train/loss": tl, "num_images": (batch_idx + 1) * args.pretrain_batch}, step=batch_idx)
            if batch_idx % args.eval_freq == 0:
                val_loss, val_acc = test_loop(args, model, val_loader, max_test_batches)
                is_best = val_loss < best_loss
                if is_best:
                    best_loss, best_batch_idx = val_loss, batch_idx
                trans = {"transductive_steps": model.transductive_steps} if getattr(model, "transductive_steps", 0) > 0 else {}
                wandb.log({"val/acc": val_acc, "val/loss": val_loss, **trans, **clip_log(opt), **distill_log(model), **head_log(model)}, step=batch_idx)
                utils.save_checkpoint({"batch_idx": batch_idx, "state_dict": model.state_dict(), "best_loss": best_loss,
                                       "optimizer": opt.state_dict(), "args": vars(args)}, is_best)
                print(f"\nBatch {batch_idx + 1}/{args.epochs}: \ntrain/loss: {tl}, train/acc: {ta}"
                      f"\nval/loss: {val_loss}, val/acc: {val_acc}")
            if (batch_idx > args.epochs - 1) or (args.patience > 0 and batch_idx - best_batch_idx > args.patience):
                break
    except KeyboardInterrupt:
        pass
    best_file = os.path.join(wandb.run.dir, "best.pth.tar")
    if os.path.exists(best_file):
        model, _ = utils.load_checkpoint(model, opt, args.device, best_file)
    return model


def test_loop(args, model, test_dataloader, max_num_batches):
    """(mean loss, mean acc) of the few-shot evaluation over max_num_batches + 1 episodic meta-batches."""
    m_loss, m_acc = AverageMeter(), AverageMeter()
    for batch_idx, batch in enumerate(test_dataloader):
        loss, acc = model.evaluate(batch=batch, optimizer=None, scheduler=None, device=args.device, task="test")
        m_loss.update(loss); m_acc.update(acc)
        if batch_idx > max_num_batches - 1:
            break
    _engine.check_status(args.device)
    return m_loss.avg, m_acc.avg
