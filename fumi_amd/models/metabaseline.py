"""Meta-Baseline (``--model metabaseline``): the episodic stage that follows a classifier pre-training (Chen et
al. 2021), and the image-only few-shot baseline on its own.

The model is the backbone of ``Pretrain`` and AM3 under the same attribute name (``conv``, so ``state_dict`` keys ``conv.*`` and
``--encoder_checkpoint`` / ``load_backbone_state`` work unchanged) and one scalar, the temperature ``temp``.  An episode is classified
by the cosine between a query's features and the class means of the support features, scaled by ``temp``; the loss is the softmax
cross-entropy over all query rows of the meta-batch.  A training step is three engine calls: ``encode`` (tape kept),
``cos_proto_step`` (csrc/cosproto.hip: loss, predictions, the gradients for both feature sets and ``temp``) and ``encode_bwd``; the
gradients land in one flat buffer and the fused optimizer step follows.  Validation and test run the head's forward form.

``head="ridge"`` (``--fewshot_head ridge``) puts the closed-form ridge-regression base learner in the head's
place: ``ridge_head_step`` (csrc/ridgehead.hip) and one parameter ``ridge = [log lambda, logit scale]`` instead of ``temp``.

``head="proto"`` (``--fewshot_head proto``) is Prototypical Networks: ``euclid_proto_step`` (csrc/euclidproto.hip),
logits ``-proto_scale * |query - class mean|^2``.  ``proto_scale`` [1] is a parameter in ``temp``'s place (TADAM's metric scaling, the
Euclidean variant of the Meta-Baseline stage) or, with ``proto_scale_fixed``, a persistent buffer that no optimizer sees: plain ProtoNet
at the default 1.0.  ``state_dict`` holds it under the same name either way.

``head="svm"`` (``--fewshot_head svm``) is MetaOptNet's multi-class SVM base learner: ``svm_head_step``
(csrc/svmhead.hip) fits the Crammer-Singer dual of each episode by FISTA and differentiates it implicitly at the fitted point.  One
parameter ``svm = [logit scale]`` in ``temp``'s place; ``C``, ``eps`` and the two step counts are fixed and always given (``svm`` dict,
as ``utils.svm_config`` returns it: the head has no silent defaults).  The largest KKT
residual and conjugate-gradient residual of the last training step are kept on the device (``svm_stats``) and logged at each validation.

``head="matching"`` (``--fewshot_head matching``) is Matching Networks (Vinyals et al. 2016, without the
full-context embeddings): ``match_head_step`` (csrc/matchhead.hip).  A query attends over the individual support rows at
``temp * cos(query, support row)`` and a class's logit is the log of the attention mass on it.  It owns ``temp`` exactly as the cosine
head does (same parameter, initial value and ``state_dict`` key) and coincides with it at one shot per class.  There are no class
prototypes, so it takes neither ``adapt="feat"`` nor ``transductive_steps > 0``.

``head="relation"`` (``--fewshot_head relation``) is the Relation Network (Sung et al. 2018) in its feature-vector
form: ``relation_head_step`` (csrc/relationhead.hip) scores every (class mean, query) pair with the learned module Linear(2F, H) -> ReLU
-> Linear(H, 1).  The model owns the submodule ``relation`` with ``w1 [2,H,F]``, ``b1``, ``w2 [H]``, ``b2 [1]`` (``state_dict`` keys
``relation.*``) and no ``temp``; the four tensors join the flat gradient buffer in front of the backbone, as ``feat.*`` do.
``relation=dict(hidden, loss)`` chooses H and the loss (``mse``, the paper's, or ``ce``).  It takes neither ``adapt="feat"`` nor
``transductive_steps > 0``.

``eval_head="logreg"`` (``--eval_head logreg``) classifies validation and test episodes with the logistic-regression
head fitted on the backbone features (``logreg_head_step``, csrc/logreghead.hip); training keeps the model's own head.  It is a choice,
not a parameter: ``state_dict`` is the same either way.

``transductive_steps > 0`` (``--transductive_steps``) classifies validation and test episodes transductively:
``trans_proto_step`` (csrc/transproto.hip) refines the class prototypes by that many soft k-means steps on the episode's queries, in the
cosine metric at ``temp`` or the Euclidean one at ``proto_scale``.  Training and ``state_dict`` are the same either way.

``adapt="feat"`` (``--fewshot_adapt feat``) is FEAT (Ye et al. 2020): the class prototypes of an episode are made
task-specific by one self-attention block over the set of prototypes, a residual and a LayerNorm (``feat_adapt_fwd`` /
``feat_adapt_bwd``, csrc/featadapt.hip), and the cosine or the prototypical head classifies against the adapted prototypes as an
N-way 1-shot support set with labels 0..N-1.  The model then owns the submodule ``feat`` (``wqkv``, ``wo``, ``bo``, ``ln_weight``,
``ln_bias``), whose gradients join the flat buffer.  A training step is five engine calls: ``encode``, ``feat_adapt_fwd``, the head,
``feat_adapt_bwd`` and ``encode_bwd``.  With ``adapt="none"`` nothing changes: same ``state_dict`` keys, engine calls and bits."""
import math
import os

import torch
import torch.nn as nn

from .. import engine as _engine
from .. import lazy
from ..flatgrad import FlatGrads, ParamWatch
from ..optim import clip_log
from ..utils import utils as utils
from ..utils.average_meter import AverageMeter
from ..utils.wandb_compat import wandb
from .common import _loss_acc


class FeatAdapt(nn.Module):
    """The parameters of the set-to-set adaptation at feature width F: the Q, K and V projections as one [3F,F] tensor (each block
    normal with std sqrt(2 / (F + F)), as FEAT initialises them), the output projection (Xavier-normal, zero bias) and the LayerNorm."""

    def __init__(self, F):
        super().__init__()
        if F % 32 != 0 or not 32 <= F <= 2048:
            raise ValueError(f"the prototype adaptation takes feature widths in multiples of 32 from 32 to 2048, got {F}")
        self.wqkv = nn.Parameter(torch.empty(3 * F, F).normal_(0.0, math.sqrt(2.0 / (F + F))))
        self.wo = nn.Parameter(nn.init.xavier_normal_(torch.empty(F, F)))
        self.bo = nn.Parameter(torch.zeros(F))
        self.ln_weight = nn.Parameter(torch.ones(F))
        self.ln_bias = nn.Parameter(torch.zeros(F))

    def tensors(self):
        """In the order of the engine's arguments (hip.FEAT_PARAMS)."""
        return [self.wqkv, self.wo, self.bo, self.ln_weight, self.ln_bias]


class RelationModule(nn.Module):
    """The parameters of the relation module at feature width F and hidden width H, in torch's [out, in] layout with nn.Linear's default
    initialisation of the two layers: ``w1 [2,H,F]`` (block 0 applied to the class mean, block 1 to the query) and ``b1 [H]`` uniform in
    +-1/sqrt(2F), ``w2 [H]`` and ``b2 [1]`` uniform in +-1/sqrt(H)."""

    def __init__(self, F, H):
        super().__init__()
        if F % 32 != 0 or not 32 <= F <= 2048:
            raise ValueError(f"the relation head takes feature widths in multiples of 32 from 32 to 2048, got {F}")
        if H % 32 != 0 or not 32 <= H <= 1024:
            raise ValueError(f"the relation head takes hidden widths in multiples of 32 from 32 to 1024, got {H}")
        k1, k2 = 1.0 / math.sqrt(2.0 * F), 1.0 / math.sqrt(float(H))
        self.w1 = nn.Parameter(torch.empty(2, H, F).uniform_(-k1, k1))
        self.b1 = nn.Parameter(torch.empty(H).uniform_(-k1, k1))
        self.w2 = nn.Parameter(torch.empty(H).uniform_(-k2, k2))
        self.b2 = nn.Parameter(torch.empty(1).uniform_(-k2, k2))

    def tensors(self):
        """In the order of the engine's arguments (hip.RELATION_PARAMS)."""
        return [self.w1, self.b1, self.w2, self.b2]


class MetaBaseline(nn.Module):
    def __init__(self, im_encoder, image_size=84, image_channels=3, num_ways=None, init_temp=10.0, head="cosine", ridge_lambda=50.0,
                 ridge_scale=1.0, eval_head="train", logreg=None, proto_scale=1.0, proto_scale_fixed=False, transductive_steps=0,
                 svm=None, adapt="none", drop=None, relation=None):
        super().__init__()
        if drop is not None and im_encoder != "resnet12":
            raise NotImplementedError("DropBlock / dropout on the block outputs is built into the ResNet-12 encoder pair: drop= needs "
                                      "im_encoder resnet12")
        self.drop = None                       # DropSchedule of the training steps, None: no drop
        self.drop_step = 0                     # the training loop's step index: the mask seed and the annealed rate follow it
        if adapt not in ("none", "feat"):
            raise ValueError(f"the prototype adaptation must be none or feat, got {adapt}")
        if adapt == "feat" and head == "matching":
            raise ValueError("the prototype adaptation (adapt=feat) moves class prototypes: the matching head attends over the support "
                             "rows and has none")
        if adapt == "feat" and head == "relation":
            raise ValueError("the prototype adaptation (adapt=feat) goes with the cosine and the prototypical head: the relation head "
                             "does not take adapted prototypes")
        if adapt == "feat" and (head not in ("cosine", "proto") or eval_head == "logreg" or int(transductive_steps) > 0):
            raise ValueError("the prototype adaptation goes with the cosine and the prototypical head, the training head at evaluation "
                             f"and no transductive refinement, got head {head}, evaluation head {eval_head}, {transductive_steps} "
                             "transductive steps")
        self.adapt = adapt
        if head not in ("cosine", "ridge", "proto", "svm", "matching", "relation"):
            raise ValueError(f"the few-shot head must be cosine, ridge, proto, svm, matching or relation, got {head}")
        if relation is not None and head != "relation":
            raise ValueError(f"relation= sets the relation head, got head {head}")
        rel = dict(hidden=256, loss="mse")
        rel.update(relation or {})
        if set(rel) != {"hidden", "loss"} or rel["loss"] not in ("mse", "ce"):
            raise ValueError(f"relation=dict(hidden, loss) with loss mse or ce expected, got {relation}")
        self.relation_loss = rel["loss"]
        if head == "svm" and svm is None:
            raise ValueError("the SVM head takes its hyper-parameters explicitly: svm=dict(C, eps, scale, steps, bwd_steps) "
                             "(utils.svm_config fills in the defaults of the flags)")
        self.svm_cfg = utils.svm_config(svm)   # C, eps, scale (initial) and the step counts of the SVM head (section 39)
        self.svm_stats = None                  # [2] on the device: max KKT residual, max CG residual of the last training step
        if eval_head not in ("train", "logreg"):
            raise ValueError(f"the evaluation head must be train or logreg, got {eval_head}")
        self.eval_head = eval_head             # validation / test classifier: the training head, or the logistic-regression head
        self.logreg = utils.logreg_config(logreg)
        if not float(init_temp) > 0.0:
            raise ValueError(f"the temperature must be positive, got {init_temp}")
        if not (float(ridge_lambda) > 0.0 and float(ridge_scale) > 0.0):
            raise ValueError(f"the ridge weight and the logit scale must be positive, got {ridge_lambda}, {ridge_scale}")
        if not float(proto_scale) > 0.0:
            raise ValueError(f"the scale of the prototypical head must be positive, got {proto_scale}")
        if proto_scale_fixed and head != "proto":
            raise ValueError(f"a fixed scale belongs to the prototypical head, got head {head}")
        if not 0 <= int(transductive_steps) <= 100:
            raise ValueError(f"the transductive refinement takes 0 to 100 steps, got {transductive_steps}")
        if int(transductive_steps) > 0 and head == "matching":
            raise ValueError("the transductive refinement (transductive_steps > 0) moves class prototypes: the matching head attends "
                             "over the support rows and has none")
        if int(transductive_steps) > 0 and head == "relation":
            raise ValueError("the transductive refinement (transductive_steps > 0) moves class prototypes in a metric: the relation "
                             "head's comparison is learned and has none")
        if int(transductive_steps) > 0 and (head in ("ridge", "svm") or eval_head == "logreg"):
            raise ValueError("the transductive refinement moves class prototypes: it goes with the cosine and the prototypical head, "
                             f"got head {head}, evaluation head {eval_head}")
        self.transductive_steps = int(transductive_steps)   # soft k-means steps of validation / test episodes (0: inductive)
        self.head = head
        self.proto_scale_fixed = bool(proto_scale_fixed)
        self.backbone = im_encoder
        if im_encoder == "conv4":
            from .conv4 import Conv4
            self.conv = Conv4(image_channels, 64, 4, image_size)
        elif im_encoder == "resnet12":
            from .resnet12 import CHANNELS, ResNet12
            self.conv = ResNet12(image_channels, CHANNELS, image_size)
        else:
            raise NameError(f"{im_encoder} not allowed as image encoder of --model metabaseline (conv4, resnet12)")
        if drop is not None:
            from .resnet12 import DropSchedule
            self.drop = DropSchedule(n_blocks=self.conv.n_blocks, **drop)
        self.num_ways = num_ways               # N of the episodes (None: read from the support labels, which synchronises)
        if head == "ridge":
            self.ridge = nn.Parameter(torch.tensor([math.log(float(ridge_lambda)), float(ridge_scale)]))
        elif head == "svm":
            self.svm = nn.Parameter(torch.tensor([self.svm_cfg["scale"]]))
        elif head == "relation":
            self.relation = RelationModule(self.conv.feature_dim, int(rel["hidden"]))
        elif head == "proto" and self.proto_scale_fixed:
            self.register_buffer("proto_scale", torch.tensor([float(proto_scale)]))
        elif head == "proto":
            self.proto_scale = nn.Parameter(torch.tensor([float(proto_scale)]))
        else:
            self.temp = nn.Parameter(torch.tensor([float(init_temp)]))
        if adapt == "feat":
            self.feat = FeatAdapt(self.conv.feature_dim)
        self._flat = None
        self._pcache = None
        self._dscale = None
        self._arange = None

    def _feat_tensors(self):
        """The tensors the model owns beside the head's scalar and the backbone: ``feat.*`` or ``relation.*`` (never both)."""
        if self.head == "relation":
            return self.relation.tensors()
        return self.feat.tensors() if self.adapt == "feat" else []

    def _class_labels(self, B, N, device):
        """y [B,N] = 0..N-1 per episode: the labels of the adapted prototypes as a 1-shot support set"""
        a = self._arange
        if a is None or a.shape != (B, N) or a.device != device:
            a = self._arange = torch.arange(N, device=device, dtype=torch.int64).repeat(B, 1).contiguous()
        return a

    def backbone_module(self):
        return self.conv

    def head_param(self):
        """The head's own parameter: ``temp`` [1] of the cosine head, ``ridge`` [2] of the ridge head, ``svm`` [1] of the SVM head,
        ``proto_scale`` [1] of the prototypical head -- None where that scale is fixed (a buffer: the head has no parameter then)."""
        if self.head == "proto":
            return None if self.proto_scale_fixed else self.proto_scale
        if self.head == "relation":
            return None
        if self.head == "svm":
            return self.svm
        return self.ridge if self.head == "ridge" else self.temp

    def _step_params(self, need_grad):
        """(detached temperature | ridge parameters | scale, detached backbone tensors, flat gradient buffer | None), the same objects
        from step to step; rebuilt when a parameter object was replaced or moved (``_apply``)."""
        c = self._pcache
        if c is None or not c[0].valid() or (self.proto_scale_fixed and c[1] is not self._buffers["proto_scale"]):
            th, hp = self.conv.theta(), self.head_param()
            own = ([] if hp is None else [hp]) + self._feat_tensors()
            scale = hp.detach() if hp is not None else None if self.head == "relation" else self._buffers["proto_scale"]
            c = self._pcache = (ParamWatch(self, own + th), scale,
                                [p.detach() for p in th], [p.detach() for p in self._feat_tensors()])
            self._flat = None
        fg = None
        if need_grad:
            fg = self._flat
            if fg is None:
                hp = self.head_param()
                fg = self._flat = FlatGrads(([] if hp is None else [hp]) + self._feat_tensors() + self.conv.theta(), extra=2)
                # the fixed scale has no slot in the flat buffer: its gradient is written beside it and read by nobody
                self._dscale = torch.empty(1, device=fg.flat.device, dtype=torch.float32) if self.proto_scale_fixed else None
        return c[1], c[2], fg

    def _apply(self, fn, recurse=True):
        self._pcache = None
        return super()._apply(fn, recurse)

    def _svm_kw(self):
        return {k: self.svm_cfg[k] for k in ("C", "eps", "steps", "bwd_steps")}

    def _encoders(self, eng):
        return ((eng.conv4_encode, eng.conv4_encode_bwd) if self.backbone == "conv4" else
                (eng.resnet12_encode, eng.resnet12_encode_bwd))

    def _episode(self, batch, device):
        (_, _, s_im), s_y = batch['train']
        (_, _, q_im), q_y = batch['test']
        to = lambda t: t.to(device).contiguous()
        x_s, x_q, y_s, y_q = to(s_im).float(), to(q_im).float(), to(s_y), to(q_y)
        N = int(self.num_ways) if self.num_ways else int(y_s.max().item()) + 1
        return x_s, x_q, y_s, y_q, N

    def train_step(self, batch, device, optimizer=None, scheduler=None):
        """One episodic step on a meta-batch of the pixel samplers; returns the head's output dict.  The gradients are left attached
        to the parameters; with an optimizer its fused step follows."""
        eng = _engine.get_engine()
        x_s, x_q, y_s, y_q, N = self._episode(batch, device)
        temp, theta, fg = self._step_params(True)
        encode, encode_bwd = self._encoders(eng)
        # the training encode alone drops (validation, test and few_shot never do)
        drop = self.drop.args(self.drop_step) if self.drop is not None and self.drop.rate_at(self.drop_step) > 0.0 else None
        if drop is not None:
            f_s, f_q = eng.resnet12_encode_drop(x_s, x_q, theta, *drop, keep_tape=True)
        else:
            f_s, f_q = encode(x_s, x_q, theta, keep_tape=True)
        featw = self._pcache[3]                 # [] without the adaptation
        g_t, g_theta = fg.split((0 if self.head_param() is None else 1) + len(featw))   # g_t: [head parameter | feat.* or relation.*]
        h_s, h_y, tape = f_s, y_s, None         # what the head takes for its support set
        if self.adapt == "feat":                # the adapted prototypes, an N-way 1-shot support set with labels 0..N-1
            h_s, tape = eng.feat_adapt_fwd(f_s, y_s, featw, n_way=N, keep_tape=True)
            h_y = self._class_labels(h_s.shape[0], N, h_s.device)
        if self.head == "relation":
            out = eng.relation_head_step(h_s, h_y, f_q, y_q, featw, loss=self.relation_loss, need_grad=True, grad_scale=1.0, g_w=g_t,
                                         n_way=N)
        elif self.head == "proto":
            out = eng.euclid_proto_step(h_s, h_y, f_q, y_q, temp, need_grad=True, grad_scale=1.0,
                                        dalpha=self._dscale if self.proto_scale_fixed else g_t[0], n_way=N)
        elif self.head == "ridge":
            out = eng.ridge_head_step(h_s, h_y, f_q, y_q, temp, need_grad=True, grad_scale=1.0, dparams=g_t[0], n_way=N)
        elif self.head == "svm":
            out = eng.svm_head_step(h_s, h_y, f_q, y_q, temp, need_grad=True, grad_scale=1.0, dscale=g_t[0], n_way=N, **self._svm_kw())
            self.svm_stats = out["stats"].amax(dim=0)
        elif self.head == "matching":
            out = eng.match_head_step(h_s, h_y, f_q, y_q, temp, need_grad=True, grad_scale=1.0, dtau=g_t[0], n_way=N)
        else:
            out = eng.cos_proto_step(h_s, h_y, f_q, y_q, temp, need_grad=True, grad_scale=1.0, dtau=g_t[0], n_way=N)
        dfeats_s = out["dfeats_s"]
        if self.adapt == "feat":                # the head's gradient for the prototypes, back to the support features
            dfeats_s, _ = eng.feat_adapt_bwd(f_s, y_s, featw, tape, dfeats_s, n_way=N, g_w=g_t[len(g_t) - len(featw):])
        if drop is not None:
            eng.resnet12_encode_bwd_drop(x_s, x_q, dfeats_s, out["dfeats_q"], theta, *drop, scale=1.0, g_theta=g_theta)
        else:
            encode_bwd(x_s, x_q, dfeats_s, out["dfeats_q"], theta, scale=1.0, g_theta=g_theta)
        _loss_acc(out, y_q, into=fg.tail)
        if optimizer is not None:
            optimizer.zero_grad()
        fg.attach()
        if optimizer is not None:
            getattr(optimizer, "step_fused", optimizer.step)()
            if scheduler:
                scheduler.step()
        return out

    def few_shot(self, batch, device):
        """[loss, acc] of one episodic meta-batch from the head's forward form (a GPU tensor of two floats)."""
        eng = _engine.get_engine()
        x_s, x_q, y_s, y_q, N = self._episode(batch, device)
        temp, theta, _ = self._step_params(False)
        f_s, f_q = self._encoders(eng)[0](x_s, x_q, theta, keep_tape=False)
        if self.adapt == "feat":                # the forward forms: the head classifies against the adapted prototypes
            f_s, _ = eng.feat_adapt_fwd(f_s, y_s, self._pcache[3], n_way=N, keep_tape=False)
            y_s = self._class_labels(f_s.shape[0], N, f_s.device)
        if self.eval_head == "logreg":
            out = eng.logreg_head_step(f_s, y_s, f_q, y_q, n_way=N, **self.logreg)
            return _loss_acc(out, y_q)
        if self.transductive_steps > 0:
            out = eng.trans_proto_step(f_s, y_s, f_q, y_q, temp, metric="euclid" if self.head == "proto" else "cosine",
                                       steps=self.transductive_steps, n_way=N)
            return _loss_acc(out, y_q)
        if self.head == "svm":
            out = eng.svm_head_step(f_s, y_s, f_q, y_q, temp, need_grad=False, n_way=N, **self._svm_kw())
            return _loss_acc(out, y_q)
        if self.head == "relation":
            out = eng.relation_head_step(f_s, y_s, f_q, y_q, self._pcache[3], loss=self.relation_loss, need_grad=False, n_way=N)
            return _loss_acc(out, y_q)
        step = getattr(eng, {"ridge": "ridge_head_step", "proto": "euclid_proto_step",
                             "matching": "match_head_step"}.get(self.head, "cos_proto_step"))
        out = step(f_s, y_s, f_q, y_q, temp, need_grad=False, n_way=N)
        return _loss_acc(out, y_q)

    def evaluate(self, batch, optimizer, scheduler, device, task="train"):
        """(loss, acc) of one episodic meta-batch: ``train`` runs a training step, ``val`` / ``test`` the forward form."""
        device = torch.device(device) if not isinstance(device, torch.device) else device
        if task == "train" and torch.is_grad_enabled():
            if not self.training:
                self.train()
            self.train_step(batch, device, optimizer, scheduler)
            return lazy.scalars(self._flat.tail, 2)
        if self.training:
            self.eval()
        with torch.no_grad():
            loss, acc = self.few_shot(batch, device).cpu().numpy()
        return loss, acc


def head_log(model):
    """What a validation logs of the head's own parameter: ``temp``, ``ridge_lambda`` and ``ridge_scale``, ``proto_scale`` or
    ``svm_scale``; with a transductive evaluation also its number of steps; for the SVM head also ``train/svm_kkt`` and
    ``train/svm_cg_res``, the largest KKT residual of the fit and the largest relative residual of the backward's conjugate gradients
    over the meta-batch of the last training step (the implicit gradient is only as good as the fit)."""
    trans = {"transductive_steps": model.transductive_steps} if getattr(model, "transductive_steps", 0) > 0 else {}
    if model.head == "proto":
        return {"proto_scale": float(model.proto_scale.detach()), **trans}
    if model.head == "relation":
        return {"relation_w2_norm": float(model.relation.w2.detach().norm())}
    if model.head == "svm":
        log = {"svm_scale": float(model.svm.detach())}
        if model.svm_stats is not None:
            kkt, cg = model.svm_stats.tolist()
            log.update({"train/svm_kkt": kkt, "train/svm_cg_res": cg})
        return log
    if model.head == "ridge":
        rho, scale = model.ridge.detach().tolist()
        return {"ridge_lambda": math.exp(rho), "ridge_scale": scale}
    return {"temp": float(model.temp.detach()), **trans}


def training_run(args, model, optimizer, train_loader, val_loader, max_test_batches):
    """The structure of pretrain.training_run: validation at batch 0 and every --eval_freq, the usual checkpoint dictionary, patience,
    reload of the best checkpoint (best validation loss) at the end."""
    best_loss, best_acc = test_loop(args, model, val_loader, max_test_batches)
    print(f"\ninitial loss: {best_loss}, acc: {best_acc}")
    best_batch_idx = 0
    opt, scheduler = optimizer if type(optimizer) == tuple else (optimizer, None)
    try:
        for batch_idx, batch in enumerate(train_loader):
            model.drop_step = batch_idx            # (--drop_rate: the step's mask seed and annealed rate)
            tl, ta = model.evaluate(batch=batch, optimizer=opt, scheduler=scheduler, device=args.device, task="train")
            wandb.log({"train/acc": ta, "train/loss": tl, "num_episodes": (batch_idx + 1) * args.batch_size}, step=batch_idx)
            if batch_idx % args.eval_freq == 0:
                val_loss, val_acc = test_loop(args, model, val_loader, max_test_batches)
                is_best = val_loss < best_loss
                if is_best:
                    best_loss, best_batch_idx = val_loss, batch_idx
                wandb.log({"val/acc": val_acc, "val/loss": val_loss, **head_log(model), **clip_log(opt)}, step=batch_idx)
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
    """(mean loss, mean acc) of the head's forward form over max_num_batches + 1 episodic meta-batches."""
    m_loss, m_acc = AverageMeter(), AverageMeter()
    for batch_idx, batch in enumerate(test_dataloader):
        loss, acc = model.evaluate(batch=batch, optimizer=None, scheduler=None, device=args.device, task="test")
        m_loss.update(loss); m_acc.update(acc)
        if batch_idx > max_num_batches - 1:
            break
    _engine.check_status(args.device)
    return m_loss.avg, m_acc.avg
