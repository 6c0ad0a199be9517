"""The compute engine behind the model classes.  There is exactly one implementation, the HIP library
(``fumi_amd/hip.py`` -> ``lib/libfumi_hip.so``); it raises when the library is missing or a tensor is not on a GPU.
The indirection exists so host-side plumbing (loops, flags, checkpoints, sharding) can be unit-tested: tests may
install a checker engine with ``set_engine`` -- product code never does."""
import torch

from . import hip

_ENGINE = None


class HipEngine:
    name = "hip-gfx950"
    folds_optimizer_step = True        # fumi_step consumes a deferred Adam step / publication (fumi_hip_adam_step_deferred)
    am3_rand_native = True             # am3_step_tx: AM3's text_encoder='rand' as a form of the step (no g, rows drawn on the device)

    def _ws(self, t):
        return hip.Workspace.get(t.device if isinstance(t, torch.Tensor) and t.is_cuda else hip._dev(t))

    def fumi_step(self, n_way, x_s, y_s, x_q, y_q, text_s, theta, phi, T, alpha, tanh_head, need_grad, grad_scale,
                  g_theta=None, g_phi=None, cls_text=None, stats=None, dropout_p=0.0, seed=0, g_cls_text=None):
        """text_s [B,S,Dt] (class rows selected on the device) or cls_text [B,N,Dt] (already selected).
        stats [2] (optional) receives grad_scale * (sum loss_b, sum acc_b); g_cls_text [B,N,Dt] (optional, need_grad) receives
        d loss / d class text rows."""
        if cls_text is not None:
            return hip.fumi_step(self._ws(x_s), x_s, y_s, x_q, y_q, theta, phi, T, alpha, tanh_head, cls_text=cls_text,
                                 need_grad=need_grad, grad_scale=grad_scale, g_theta=g_theta, g_phi=g_phi, stats=stats,
                                 dropout_p=dropout_p, seed=seed, g_cls_text=g_cls_text)
        return hip.fumi_step_select(self._ws(x_s), n_way, x_s, y_s, x_q, y_q, text_s, theta, phi, T, alpha, tanh_head,
                                    need_grad=need_grad, grad_scale=grad_scale, g_theta=g_theta, g_phi=g_phi, stats=stats,
                                    dropout_p=dropout_p, seed=seed, g_cls_text=g_cls_text)

    def glove_bag_select(self, tokens_s, y_s, n_way, table, pad_id, mode, defer=False):
        """defer: the bag rides in the first launch of the ``fumi_step`` that must follow with the result as ``cls_text``"""
        return hip.glove_bag_select(self._ws(tokens_s), tokens_s, y_s, n_way, table, pad_id, mode, defer=defer)

    def maml_step(self, x_s, y_s, x_q, y_q, params, T, alpha, first_order, need_grad, grad_scale, g_params=None,
                  stats=None):
        return hip.maml_step(self._ws(x_s), x_s, y_s, x_q, y_q, params, T, alpha, first_order, need_grad=need_grad,
                             grad_scale=grad_scale, g_params=g_params, stats=stats)

    def am3_step(self, x_s, y_s, x_q, y_q, text_s, w, n_way, lamda_fixed, need_grad, grad_scale, g_w=None,
                 dropout_p=0.0, seed=0, stats=None, want_dx=False, g_text=None):
        """g_text [B,S,Dt] (optional, need_grad) receives d loss / d text_s."""
        return hip.am3_step(self._ws(x_s), x_s, y_s, x_q, y_q, text_s, w, n_way, lamda_fixed, need_grad=need_grad,
                            grad_scale=grad_scale, g_w=g_w, dropout_p=dropout_p, seed=seed, stats=stats, want_dx=want_dx,
                            g_text=g_text)

    def am3_step_tx(self, x_s, y_s, x_q, y_q, text_rows, w, n_way, lamda_fixed, need_grad, grad_scale, g_w=None,
                    dropout_p=0.0, seed=0, stats=None, want_dx=False):
        """The AM3 step on prototype-space text rows [B,S,P] (None: drawn on the device from ``seed``); w[2:6] / g_w[2:6] may be None."""
        return hip.am3_step_tx(self._ws(x_s), x_s, y_s, x_q, y_q, text_rows, w, n_way, lamda_fixed, need_grad=need_grad,
                               grad_scale=grad_scale, g_w=g_w, dropout_p=dropout_p, seed=seed, stats=stats, want_dx=want_dx)

    def conv4_encode(self, x_s, x_q, theta, keep_tape=False):
        """Conv4 in front of a step with its own workspace (AM3): the tape lives in the device's "encoder" workspace."""
        return hip.conv4_encode(hip.Workspace.get(x_s.device, "encoder"), x_s, x_q, theta, keep_tape=keep_tape)

    def conv4_encode_bwd(self, x_s, x_q, dfeats_s, dfeats_q, theta_like, scale=1.0, g_theta=None):
        return hip.conv4_encode_bwd(hip.Workspace.get(x_s.device, "encoder"), x_s, x_q, dfeats_s, dfeats_q, theta_like,
                                    scale=scale, g_theta=g_theta)

    def resnet12_encode(self, x_s, x_q, theta, keep_tape=False):
        """ResNet-12 in front of a step with its own workspace (AM3): the tape lives in the device's "encoder" workspace."""
        return hip.resnet12_encode(hip.Workspace.get(x_s.device, "encoder"), x_s, x_q, theta, keep_tape=keep_tape)

    def resnet12_encode_bwd(self, x_s, x_q, dfeats_s, dfeats_q, theta_like, scale=1.0, g_theta=None):
        return hip.resnet12_encode_bwd(hip.Workspace.get(x_s.device, "encoder"), x_s, x_q, dfeats_s, dfeats_q, theta_like,
                                       scale=scale, g_theta=g_theta)

    def resnet12_encode_drop(self, x_s, x_q, theta, drop_rate, drop_block, drop_seed, keep_tape=False):
        """``resnet12_encode`` with DropBlock / dropout on the block outputs (training steps only; per-block rates and block sizes)."""
        return hip.resnet12_encode_drop(hip.Workspace.get(x_s.device, "encoder"), x_s, x_q, theta, drop_rate, drop_block, drop_seed,
                                        keep_tape=keep_tape)

    def resnet12_encode_bwd_drop(self, x_s, x_q, dfeats_s, dfeats_q, theta_like, drop_rate, drop_block, drop_seed, scale=1.0,
                                 g_theta=None):
        return hip.resnet12_encode_bwd_drop(hip.Workspace.get(x_s.device, "encoder"), x_s, x_q, dfeats_s, dfeats_q, theta_like,
                                            drop_rate, drop_block, drop_seed, scale=scale, g_theta=g_theta)

    def fumi_conv4_step(self, n_way, x_s, y_s, x_q, y_q, text_s, theta, phi, T, alpha, tanh_head, need_grad, grad_scale,
                        g_theta=None, g_phi=None, cls_text=None, stats=None, g_cls_text=None):
        """FuMI with the Conv4 encoder at the im_net seam: x_s [B,S,C,H,W], x_q [B,Qn,C,H,W]."""
        return hip.fumi_conv4_step(self._ws(x_s), n_way, x_s, y_s, x_q, y_q, theta, phi, T, alpha, tanh_head, cls_text=cls_text,
                                   text_s=text_s, need_grad=need_grad, grad_scale=grad_scale, g_theta=g_theta, g_phi=g_phi,
                                   stats=stats, g_cls_text=g_cls_text)

    def maml_conv4_step(self, x_s, y_s, x_q, y_q, params, T, alpha, first_order, need_grad, grad_scale, g_params=None,
                        stats=None):
        return hip.maml_conv4_step(self._ws(x_s), x_s, y_s, x_q, y_q, params, T, alpha, first_order, need_grad=need_grad,
                                   grad_scale=grad_scale, g_params=g_params, stats=stats)

    def fumi_resnet12_step(self, n_way, x_s, y_s, x_q, y_q, text_s, theta, phi, T, alpha, tanh_head, need_grad, grad_scale,
                           g_theta=None, g_phi=None, cls_text=None, stats=None, g_cls_text=None):
        """FuMI with the bf16 ResNet-12 encoder at the im_net seam (BASELINE.json configs[4])."""
        return hip.fumi_resnet12_step(self._ws(x_s), n_way, x_s, y_s, x_q, y_q, theta, phi, T, alpha, tanh_head, cls_text=cls_text,
                                      text_s=text_s, need_grad=need_grad, grad_scale=grad_scale, g_theta=g_theta, g_phi=g_phi,
                                      stats=stats, g_cls_text=g_cls_text)

    def maml_resnet12_step(self, x_s, y_s, x_q, y_q, params, T, alpha, first_order, need_grad, grad_scale, g_params=None,
                           stats=None):
        return hip.maml_resnet12_step(self._ws(x_s), x_s, y_s, x_q, y_q, params, T, alpha, first_order, need_grad=need_grad,
                                      grad_scale=grad_scale, g_params=g_params, stats=stats)

    def resnet12_features(self, x, theta):
        return hip.resnet12_features(self._ws(x), x, theta)

    def conv4_features(self, x, theta):
        return hip.conv4_features(self._ws(x), x, theta)

    def clip_step(self, text, image, w, need_loss=True, need_grad=True, g_w=None):
        return hip.clip_step(self._ws(text), text, image, w, need_loss=need_loss, need_grad=need_grad, g_w=g_w)

    def lstm_bidir(self, tokens, table, lstm_w, pad_id, use_cell):
        return hip.lstm_bidir(self._ws(tokens), tokens, table, lstm_w, pad_id, use_cell)

    def lstm_bidir_train(self, tokens, table, lstm_w, pad_id, use_cell):
        """(out, tape): the forward of a trainable bi-LSTM encoder (--fine_tune with RNN / RNNhid, fumi/models/fumi.py:65-67)."""
        return hip.lstm_bidir_train(self._ws(tokens), tokens, table, lstm_w, pad_id, use_cell)

    def lstm_bidir_bwd(self, tokens, table, lstm_w, pad_id, use_cell, tape, d_out):
        return hip.lstm_bidir_bwd(self._ws(tokens), tokens, table, lstm_w, pad_id, use_cell, tape, d_out)

    def class_rows_select(self, rows_s, y_s, n_way):
        """[B,N,...] the first support row of every class (fumi.py:207-210) of float32 OR int64 rows [B,S,W]: a pure row copy, so
        token rows go through the float kernel as pairs of 32-bit words."""
        if rows_s.dtype == torch.int64:
            out = hip.class_text_select(self._ws(rows_s), rows_s.contiguous().view(torch.float32), y_s, n_way)
            return out.view(torch.int64)
        return hip.class_text_select(self._ws(rows_s), rows_s.contiguous(), y_s, n_way)

    def am3_metrics(self, n_way, stats):
        return hip.am3_metrics(self._ws(stats), n_way, stats)

    def glove_bag(self, tokens, table, pad_id, mode):
        return hip.glove_bag(self._ws(tokens), tokens, table, pad_id, mode)

    def linear(self, x, W, b=None, act=0):
        return hip.linear_fwd(self._ws(x), x.contiguous(), W.contiguous(), b, act)

    def cls_head_step(self, feats, y, W, b, need_grad=True, grad_scale=1.0, dfeats=None, gW=None, gb=None):
        """Fused classification head of supervised pre-training: mean cross-entropy of feats @ W.T + b, its predictions and gradients."""
        return hip.cls_head_step(self._ws(feats), feats, y, W, b, need_grad=need_grad, grad_scale=grad_scale, dfeats=dfeats, gW=gW,
                                 gb=gb)

    def cls_head_step_soft(self, feats, y_a, W, b, y_b=None, lam=1.0, smoothing=0.0, need_grad=True, grad_scale=1.0, dfeats=None,
                           gW=None, gb=None):
        """The same head against the soft target of label smoothing and a two-label mix (mixup / CutMix)."""
        return hip.cls_head_step_soft(self._ws(feats), feats, y_a, W, b, y_b=y_b, lam=lam, smoothing=smoothing, need_grad=need_grad,
                                      grad_scale=grad_scale, dfeats=dfeats, gW=gW, gb=gb)

    def cls_head_step_distill(self, feats, y_a, W, b, feats_t, W_t, b_t, temp, alpha, ce_weight, y_b=None, lam=1.0, smoothing=0.0,
                              need_grad=True, grad_scale=1.0, dfeats=None, gW=None, gb=None):
        """The same head as the student of a frozen teacher: ce_weight * CE + alpha * T^2 KL(teacher || student)
        at temperature ``temp``, with loss_ce, loss_kd and the count of rows that agree with the teacher."""
        return hip.cls_head_step_distill(self._ws(feats), feats, y_a, W, b, feats_t, W_t, b_t, temp=temp, alpha=alpha,
                                         ce_weight=ce_weight, y_b=y_b, lam=lam, smoothing=smoothing, need_grad=need_grad,
                                         grad_scale=grad_scale, dfeats=dfeats, gW=gW, gb=gb)

    def cos_cls_head_step(self, feats, y_a, W, tau, y_b=None, lam=1.0, smoothing=0.0, need_grad=True, grad_scale=1.0, dfeats=None,
                          gW=None, dtau=None):
        """Fused cosine classifier head of supervised pre-training: mean cross-entropy of tau * cos(feats_m,
        W_c) against the soft target, with tau [1] on the device; its predictions and the gradients for feats, W and tau."""
        return hip.cos_cls_head_step(self._ws(feats), feats, y_a, W, tau, y_b=y_b, lam=lam, smoothing=smoothing, need_grad=need_grad,
                                     grad_scale=grad_scale, dfeats=dfeats, gW=gW, dtau=dtau)

    def cos_proto_step(self, feats_s, y_s, feats_q, y_q, tau, need_grad=True, grad_scale=1.0, want_logits=False, dfeats_s=None,
                       dfeats_q=None, dtau=None, n_way=None):
        """Fused cosine nearest-centroid head with the temperature tau [1] on the device: mean cross-entropy of
        tau * cos(query, class mean) over all query rows, its predictions and the gradients for both feature sets and tau."""
        return hip.cos_proto_step(self._ws(feats_s), feats_s, y_s, feats_q, y_q, tau, need_grad=need_grad, grad_scale=grad_scale,
                                  want_logits=want_logits, dfeats_s=dfeats_s, dfeats_q=dfeats_q, dtau=dtau, n_way=n_way)

    def euclid_proto_step(self, feats_s, y_s, feats_q, y_q, alpha, need_grad=True, grad_scale=1.0, want_logits=False, dfeats_s=None,
                          dfeats_q=None, dalpha=None, n_way=None):
        """Fused prototypical-network head with the metric scale alpha [1] on the device: mean cross-entropy of
        -alpha * |query - class mean|^2 over all query rows, its predictions and the gradients for both feature sets and alpha."""
        return hip.euclid_proto_step(self._ws(feats_s), feats_s, y_s, feats_q, y_q, alpha, need_grad=need_grad, grad_scale=grad_scale,
                                     want_logits=want_logits, dfeats_s=dfeats_s, dfeats_q=dfeats_q, dalpha=dalpha, n_way=n_way)

    def match_head_step(self, feats_s, y_s, feats_q, y_q, tau, need_grad=True, grad_scale=1.0, want_logits=False, dfeats_s=None,
                        dfeats_q=None, dtau=None, n_way=None):
        """Fused Matching Networks head with the temperature tau [1] on the device: mean cross-entropy of the
        per-class log attention mass of tau * cos(query, support row) over all query rows, its predictions and the gradients for both
        feature sets and tau."""
        return hip.match_head_step(self._ws(feats_s), feats_s, y_s, feats_q, y_q, tau, need_grad=need_grad, grad_scale=grad_scale,
                                   want_logits=want_logits, dfeats_s=dfeats_s, dfeats_q=dfeats_q, dtau=dtau, n_way=n_way)

    def relation_head_step(self, feats_s, y_s, feats_q, y_q, params, loss="mse", need_grad=True, grad_scale=1.0, want_logits=False,
                           want_hidden=False, dfeats_s=None, dfeats_q=None, g_w=None, n_way=None):
        """Fused Relation Network head with the relation module's tensors params = (w1 [2,H,F], b1, w2 [H], b2 [1]) on the device
        (DESIGN.md section 51): the ``mse`` or ``ce`` loss of z[q,n] = w2 . relu(W1s mean_n + b1 + W1q query) + b2 over all query rows,
        its predictions and the gradients for both feature sets and the four tensors (into ``g_w`` where given)."""
        return hip.relation_head_step(self._ws(feats_s), feats_s, y_s, feats_q, y_q, params, loss=loss, need_grad=need_grad,
                                      grad_scale=grad_scale, want_logits=want_logits, want_hidden=want_hidden, dfeats_s=dfeats_s,
                                      dfeats_q=dfeats_q, g_w=g_w, n_way=n_way)

    def feat_adapt_fwd(self, feats_s, y_s, w, n_way=None, keep_tape=False):
        """Set-to-set prototype adaptation (FEAT): (adapted prototypes [B,N,F], tape | None) of the class means
        of feats_s through one self-attention block, a residual and a LayerNorm; w = (wqkv, wo, bo, ln_weight, ln_bias)."""
        return hip.feat_adapt_fwd(self._ws(feats_s), feats_s, y_s, w, n_way=n_way, keep_tape=keep_tape)

    def feat_adapt_bwd(self, feats_s, y_s, w, tape, dprotos, n_way=None, dfeats_s=None, g_w=None):
        """(dfeats_s [B,S,F], g_w) for dprotos [B,N,F], the head's gradient for the adapted prototypes."""
        return hip.feat_adapt_bwd(self._ws(feats_s), feats_s, y_s, w, tape, dprotos, n_way=n_way, dfeats_s=dfeats_s, g_w=g_w)

    def ridge_head_step(self, feats_s, y_s, feats_q, y_q, params, need_grad=True, grad_scale=1.0, want_logits=False, dfeats_s=None,
                        dfeats_q=None, dparams=None, n_way=None):
        """Fused ridge-regression head with params [2] = (log lambda, logit scale) on the device: mean
        cross-entropy of scale * query . W with W the closed-form ridge solution on the support rows, its predictions and the gradients
        for both feature sets and params, through the solve."""
        return hip.ridge_head_step(self._ws(feats_s), feats_s, y_s, feats_q, y_q, params, need_grad=need_grad, grad_scale=grad_scale,
                                   want_logits=want_logits, dfeats_s=dfeats_s, dfeats_q=dfeats_q, dparams=dparams, n_way=n_way)

    def svm_head_step(self, feats_s, y_s, feats_q, y_q, scale, C=0.1, eps=1.0, steps=120, bwd_steps=40, need_grad=True, grad_scale=1.0,
                      want_logits=False, dfeats_s=None, dfeats_q=None, dscale=None, n_way=None):
        """Fused MetaOptNet-SVM head with the logit scale [1] on the device: mean cross-entropy of scale *
        query . W with W the multi-class SVM fitted on the support rows by ``steps`` steps of FISTA on its dual, its predictions and the
        implicit gradients for both feature sets and the scale (``bwd_steps`` steps of conjugate gradients); ``stats`` [B,2] holds the
        fit's KKT residual and the conjugate gradients' relative residual per episode."""
        return hip.svm_head_step(self._ws(feats_s), feats_s, y_s, feats_q, y_q, scale, C=C, eps=eps, steps=steps, bwd_steps=bwd_steps,
                                 need_grad=need_grad, grad_scale=grad_scale, want_logits=want_logits, dfeats_s=dfeats_s,
                                 dfeats_q=dfeats_q, dscale=dscale, n_way=n_way)

    def logreg_head_step(self, feats_s, y_s, feats_q, y_q, steps=100, lr=1.0, momentum=0.9, C=1.0, normalize=True, want_logits=False,
                         n_way=None):
        """Fused logistic-regression head, forward only: ``steps`` steps of heavy-ball descent from zero on the
        multinomial logistic regression of each episode's support rows, fitted in LDS; mean cross-entropy and predictions of the
        query rows."""
        return hip.logreg_head_step(self._ws(feats_s), feats_s, y_s, feats_q, y_q, steps=steps, lr=lr, momentum=momentum, C=C,
                                    normalize=normalize, want_logits=want_logits, n_way=n_way)

    def trans_proto_step(self, feats_s, y_s, feats_q, y_q, scale, metric, steps, want_logits=False, n_way=None):
        """Transductive prototype refinement, forward only: ``steps`` steps of soft k-means of the class
        prototypes on each episode's query rows, then the mean cross-entropy and predictions of the cosine (``metric="cosine"``) or
        squared-Euclidean (``"euclid"``) logits at ``scale`` [1] on the device."""
        return hip.trans_proto_step(self._ws(feats_s), feats_s, y_s, feats_q, y_q, scale, metric=metric, steps=steps,
                                    want_logits=want_logits, n_way=n_way)

    def mix_images(self, x, partner, mode, lam=1.0, box=(0, 0, 0, 0)):
        """mixup (mode 0) / CutMix (mode 1) of a gathered image batch with its rows ``partner``."""
        return hip.mix_images(self._ws(x), x, partner, mode=mode, lam=lam, box=box)

    def proto_reduce(self, x, y, n_way):
        return hip.proto_reduce(self._ws(x), x, y, n_way)

    def sgd_axpy(self, p, step_size, g):
        return hip.sgd_axpy(self._ws(p), p, step_size, g)

    def check(self, device):
        """Synchronising validity check of the last calls (labels in range, every class has a support sample, every pivot of the
        ridge head positive)."""
        device = torch.device(device)
        if device.type == "cuda":
            hip.raise_on_status(hip.Workspace.get(device).read_status())


def check_status(device):
    """Raise what the reference raises for an invalid episode.  The kernels record a label outside [0, N) or a class without
    a support sample in the workspace's status word instead of faulting; the reference's per-class loop raises IndexError there
    (fumi/models/fumi.py:209).  Reading the word synchronises the stream, so the loops call this where they wait for the
    device anyway: at the end of every validation / test loop (which also covers the training steps before it) and before a
    run ends."""
    eng = get_engine()
    if hasattr(eng, "check"):
        eng.check(device)


def get_engine():
    global _ENGINE
    if _ENGINE is None:
        hip.lib()                      # fail loudly here if the shared object has not been built
        _ENGINE = HipEngine()
    return _ENGINE


def set_engine(engine):
    """Test hook (tests/ only)."""
    global _ENGINE
    old, _ENGINE = _ENGINE, engine
    return old
