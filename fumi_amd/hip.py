"""ctypes binding of ``include/fumi_hip.h`` (the gfx950 engine, ``fumi_amd/lib/libfumi_hip.so``).

PyTorch is plumbing here: it owns device memory and the HIP stream; every tensor is handed to the
library as a raw device pointer.  There is NO CPU fallback: if the library is missing, or a tensor
is not on a GPU, these functions raise.
"""
import collections
import ctypes
import os
import threading
from ctypes import c_int, c_int64, c_float, c_void_p, c_size_t, c_char_p, POINTER

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfumi_hip.so")

# every symbol include/fumi_hip.h declares (tests/test_abi.py checks the shared object exports them all)
SYMBOLS = [
    "fumi_hip_version", "fumi_hip_strerror", "fumi_hip_last_hip_error",
    "fumi_hip_workspace_create", "fumi_hip_workspace_destroy", "fumi_hip_workspace_bytes", "fumi_hip_read_status",
    "fumi_hip_set_spin_limit", "fumi_hip_set_trace_buffer",
    "fumi_hip_set_profiling", "fumi_hip_set_profiling_every", "fumi_hip_get_profile", "fumi_hip_phase_name",
    "fumi_hip_fumi_step", "fumi_hip_fumi_step_indexed", "fumi_hip_maml_step", "fumi_hip_am3_step",
    "fumi_hip_glove_bag", "fumi_hip_glove_bag_select", "fumi_hip_glove_bag_select_deferred", "fumi_hip_glove_flush", "fumi_hip_class_text_select", "fumi_hip_xpanel_fwd", "fumi_hip_xpanel_bwd", "fumi_hip_xpanel_plan", "fumi_hip_xpanel_planes_bytes", "fumi_hip_xpanel_fwd_rows",
    "fumi_hip_epi_plan", "fumi_hip_epi_plan_query", "fumi_hip_hyper_plan", "fumi_hip_hyper_plan_query",
    "fumi_hip_reduce_segments",
    "fumi_hip_adam_step", "fumi_hip_adam_step_deferred", "fumi_hip_adam_flush",
    "fumi_hip_adamw_step", "fumi_hip_adamw_step_deferred", "fumi_hip_sgd_step", "fumi_hip_sgd_step_deferred",
    "fumi_hip_grad_norm", "fumi_hip_adam_step_clipped", "fumi_hip_adamw_step_clipped", "fumi_hip_sgd_step_clipped",
    "fumi_hip_linear_fwd", "fumi_hip_linear_bwd_data", "fumi_hip_linear_bwd_weight",
    "fumi_hip_sample_episodes", "fumi_hip_sample_episodes_tm", "fumi_hip_gather_rows", "fumi_hip_gather_images", "fumi_hip_gather_images_resized", "fumi_hip_publish_scalars",
    "fumi_hip_publish_scalars_deferred", "fumi_hip_publish_flush", "fumi_hip_am3_metrics", "fumi_hip_am3_step_plan",
    "fumi_hip_conv4_feature_dim", "fumi_hip_fumi_conv4_step", "fumi_hip_maml_conv4_step", "fumi_hip_conv4_probe", "fumi_hip_conv4_features", "fumi_hip_conv4_set_option",
    "fumi_hip_conv4_encode", "fumi_hip_conv4_encode_bwd", "fumi_hip_am3_step_dx",
    "fumi_hip_resnet12_set_budget", "fumi_hip_fumi_resnet12_step", "fumi_hip_maml_resnet12_step", "fumi_hip_resnet12_features",
    "fumi_hip_resnet12_encode", "fumi_hip_resnet12_encode_bwd", "fumi_hip_resnet12_encode_plan",
    "fumi_hip_rn12_conv", "fumi_hip_rn12_wgrad", "fumi_hip_rn12_conv_multi", "fumi_hip_rn12_wgrad_multi",
    "fumi_hip_rn12_conv_plan", "fumi_hip_rn12_conv_query", "fumi_hip_rn12_wgrad_query", 
    "fumi_hip_rn12_ew_act", "fumi_hip_rn12_ew_bwd", "fumi_hip_rn12_ew_join", "fumi_hip_rn12_ew_coef", "fumi_hip_rn12_ew_avgpool",
    "fumi_hip_rn12_ew_img_prep", "fumi_hip_rn12_ew_query", "fumi_hip_rn12_ew_plan", "fumi_hip_rn12_coef_query",
    "fumi_hip_resnet12_set_option", "fumi_hip_rn12_probe",
    "fumi_hip_conv3x3_fwd", "fumi_hip_conv3x3_bwd_data", "fumi_hip_conv3x3_bwd_weight",
    "fumi_hip_sgd_axpy", "fumi_hip_ce_fwd_bwd", "fumi_hip_proto_reduce", "fumi_hip_clip_step", "fumi_hip_lstm_bidir", "fumi_hip_lstm_tape_floats", "fumi_hip_lstm_bidir_train", "fumi_hip_lstm_bidir_bwd",
    "fumi_hip_am3_step_tx", "fumi_hip_am3_step_tx_dx",
    "fumi_hip_cls_head_step",
    "fumi_hip_cls_head_step_soft", "fumi_hip_mix_images",
    "fumi_hip_cos_proto_step", "fumi_hip_ridge_head_step", "fumi_hip_logreg_head_step", "fumi_hip_logreg_set_form",
    "fumi_hip_euclid_proto_step", "fumi_hip_trans_proto_step",
    "fumi_hip_cls_head_step_distill",
    "fumi_hip_svm_head_step", "fumi_hip_svm_set_form", "fumi_hip_svm_get_fit",
    "fumi_hip_cos_cls_head_step",
    "fumi_hip_feat_adapt_tape_floats", "fumi_hip_feat_adapt_fwd", "fumi_hip_feat_adapt_bwd",
    "fumi_hip_resnet12_encode_drop", "fumi_hip_resnet12_encode_bwd_drop", "fumi_hip_rn12_drop_apply",
    "fumi_hip_match_head_step",
    "fumi_hip_relation_head_step",
]

ST_LABEL_RANGE, ST_CLASS_MISSING, ST_SYNC_TIMEOUT, ST_NOT_POSDEF = 1, 2, 4, 8
N_PHASES = 18

_lib = None
_lock = threading.Lock()


class FumiHipError(RuntimeError):
    pass

class RowRef:
    """Zero-copy stand-in for an image tensor x[B, rows, D]: x[b, r] = table[idx[b, r]] with ``table`` [n_rows, D] fp32 resident
    on the device (fumi_hip_fumi_step_indexed).  Quacks like the tensor where FUMI.evaluate touches it."""
    __slots__ = ("table", "idx")

    def __init__(self, table, idx):
        if table.dim() != 2 or idx.dim() != 2 or idx.dtype != torch.int64 or table.dtype != torch.float32:
            raise FumiHipError("RowRef: table must be [n_rows, D] fp32 and idx [B, rows] int64")
        self.table, self.idx = table, idx

    shape = property(lambda self: (self.idx.shape[0], self.idx.shape[1], self.table.shape[1]))
    device = property(lambda self: self.table.device)
    is_cuda = property(lambda self: self.table.is_cuda)

    def __getitem__(self, sl):
        return RowRef(self.table, self.idx[sl])

    def to(self, *a, **k):
        return self

    def contiguous(self):
        return RowRef(self.table, self.idx.contiguous())

    def float(self):
        return self

    dtype = torch.float32

    def is_contiguous(self):
        return self.idx.is_contiguous()

    def materialize(self):
        return self.table[self.idx]



def lib():
    """Load the shared object once.  Fails loudly when it has not been built (``python __graft_entry__.py``)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise FumiHipError(
                f"{LIB_PATH} is missing: the MI355X engine has no CPU fallback. Build it with "
                f"`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950).")
        L = ctypes.CDLL(LIB_PATH)
        L.fumi_hip_version.restype = c_int
        L.fumi_hip_strerror.restype = c_char_p
        L.fumi_hip_strerror.argtypes = [c_int]
        L.fumi_hip_last_hip_error.restype = c_char_p
        L.fumi_hip_workspace_create.argtypes = [c_int, c_size_t, POINTER(c_void_p)]
        L.fumi_hip_workspace_destroy.argtypes = [c_void_p]
        L.fumi_hip_workspace_destroy.restype = None
        L.fumi_hip_workspace_bytes.argtypes = [c_void_p]
        L.fumi_hip_workspace_bytes.restype = c_size_t
        L.fumi_hip_read_status.argtypes = [c_void_p, c_void_p, POINTER(c_int)]
        L.fumi_hip_set_spin_limit.argtypes = [c_int]
        L.fumi_hip_set_trace_buffer.argtypes = [c_int, c_void_p]
        L.fumi_hip_set_profiling.argtypes = [c_void_p, c_int]
        L.fumi_hip_set_profiling_every.argtypes = [c_void_p, c_int]
        L.fumi_hip_get_profile.argtypes = [c_void_p, c_int, POINTER(ctypes.c_double), POINTER(c_int)]
        L.fumi_hip_phase_name.argtypes = [c_int]
        L.fumi_hip_phase_name.restype = c_char_p
        PP, PI = POINTER(c_void_p), POINTER(c_int)
        # the step entry points' argument lists, from the pieces include/fumi_hip.h writes them in (tests/test_abi.py holds every list
        # to the header, argument by argument)
        front = [c_void_p, c_void_p]                                   # ws, stream
        mlp = [c_int] * 6 + [PI]                                       # B, N, S, Qn, D, n_hidden, hid
        img = [c_int] * 8                                              # B, N, S, Qn, Cin, H, W, nblk
        text_dims = [c_int, c_int]                                     # Dt, Ht
        inner = [c_int, c_float, c_int, c_int, c_float]                # T, alpha, tanh_head | first_order, need_grad, grad_scale
        drop = [c_float, ctypes.c_uint64]                              # dropout_p, seed
        episodes = [c_void_p] * 4                                      # x_s | idx_s, y_s, x_q | idx_q, y_q
        text_in = [c_void_p] * 2                                       # cls_text, text_s
        outs = [c_void_p] * 6                                          # logits_q, preds_q, preds_q_f32, loss_b, acc_b + stats
        fumi_io = episodes + text_in + [PP, PP] + outs + [PP, PP, c_void_p]   # ... theta, phi ... g_theta, g_phi, g_cls_text
        maml_io = episodes + [PP] + outs + [PP]                        # ... params ... g_params
        L.fumi_hip_fumi_step.argtypes = front + mlp + text_dims + inner + drop + fumi_io
        L.fumi_hip_fumi_step_indexed.argtypes = front + mlp + text_dims + inner + drop + [c_void_p, c_int64] + fumi_io    # table, n_rows
        L.fumi_hip_maml_step.argtypes = front + mlp + inner + maml_io
        am3_io = (front + [c_int] * 10 + [c_float] + drop                              # B, N, S, Qn, D, Dt, Ht, P, lamda_fixed, need_grad
                  + episodes + [c_void_p, PP] + [c_void_p] * 4 + [PP, c_void_p])       # text_s, w | 4 outputs | g_w, stats
        dx = [c_void_p, c_void_p]                                      # dx_s, dx_q
        L.fumi_hip_am3_step.argtypes = am3_io + [c_void_p]             # g_text
        L.fumi_hip_am3_step_dx.argtypes = am3_io + dx + [c_void_p]
        L.fumi_hip_am3_step_tx.argtypes = am3_io + [c_void_p]          # tx_out
        L.fumi_hip_am3_step_tx_dx.argtypes = am3_io + [c_void_p] + dx
        L.fumi_hip_am3_metrics.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
        L.fumi_hip_glove_bag.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64, c_void_p, c_int, c_int,
                                         c_int, c_void_p]
        L.fumi_hip_glove_bag_select.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64,
                                                c_void_p, c_int, c_int, c_int, c_void_p]
        L.fumi_hip_glove_bag_select_deferred.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int64,
                                                         c_void_p, c_int, c_int, c_int, c_void_p]
        L.fumi_hip_glove_flush.argtypes = [c_void_p, c_void_p]
        L.fumi_hip_class_text_select.argtypes = [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p] * 3
        L.fumi_hip_xpanel_fwd.argtypes = [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p] * 5
        L.fumi_hip_xpanel_bwd.argtypes = [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p] * 3 + [c_float, c_void_p]
        L.fumi_hip_xpanel_plan.argtypes = [POINTER(c_int), c_int]
        L.fumi_hip_xpanel_fwd_rows.argtypes = [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p, c_int64] + [c_void_p] * 5
        L.fumi_hip_xpanel_planes_bytes.argtypes = []
        L.fumi_hip_xpanel_planes_bytes.restype = c_size_t
        L.fumi_hip_epi_plan.argtypes = [POINTER(c_int), c_int]
        L.fumi_hip_epi_plan_query.argtypes = [c_int] * 6 + [POINTER(c_int)] + [c_int] * 5 + [POINTER(c_int), c_int]
        L.fumi_hip_hyper_plan.argtypes = [POINTER(c_int), c_int]
        L.fumi_hip_hyper_plan_query.argtypes = [c_int] * 6 + [POINTER(c_int)] + [c_int] * 5 + [POINTER(c_int), c_int]
        L.fumi_hip_reduce_segments.argtypes = [c_void_p, c_void_p, c_int, PP, POINTER(c_int), POINTER(ctypes.c_long),
                                               POINTER(ctypes.c_long), PP, c_float]
        L.fumi_hip_adam_step.argtypes = [c_void_p, c_void_p, c_int, PP, PP, PP, PP, POINTER(ctypes.c_long)] + [c_float] * 5 + [c_int]
        L.fumi_hip_adam_step_deferred.argtypes = [c_void_p, c_int, PP, PP, PP, PP, POINTER(ctypes.c_long)] + [c_float] * 5 + [c_int]
        L.fumi_hip_adam_flush.argtypes = [c_void_p, c_void_p, POINTER(c_int)]
        betas = [c_float, ctypes.c_double, ctypes.c_double, c_float, c_float, c_int]       # lr, beta1, beta2 (doubles), eps, wd, step
        L.fumi_hip_adamw_step.argtypes = [c_void_p, c_void_p, c_int, PP, PP, PP, PP, POINTER(ctypes.c_long)] + betas
        L.fumi_hip_adamw_step_deferred.argtypes = [c_void_p, c_int, PP, PP, PP, PP, POINTER(ctypes.c_long)] + betas
        L.fumi_hip_sgd_step.argtypes = [c_void_p, c_void_p, c_int, PP, PP, PP, POINTER(ctypes.c_long)] + [c_float] * 3 + [c_int]
        L.fumi_hip_sgd_step_deferred.argtypes = [c_void_p, c_int, PP, PP, PP, POINTER(ctypes.c_long)] + [c_float] * 3 + [c_int]
        clip = [c_float, c_void_p]                                                         # max_norm, clip_out (device {norm, coef})
        L.fumi_hip_grad_norm.argtypes = [c_void_p, c_void_p, c_int, PP, POINTER(ctypes.c_long), c_void_p]
        L.fumi_hip_adam_step_clipped.argtypes = L.fumi_hip_adam_step.argtypes + clip
        L.fumi_hip_adamw_step_clipped.argtypes = L.fumi_hip_adamw_step.argtypes + clip
        L.fumi_hip_sgd_step_clipped.argtypes = L.fumi_hip_sgd_step.argtypes + clip
        L.fumi_hip_linear_fwd.argtypes = [c_void_p, c_void_p] + [c_int] * 3 + [c_void_p] * 3 + [c_int, c_void_p]
        L.fumi_hip_linear_bwd_data.argtypes = [c_void_p, c_void_p] + [c_int] * 3 + [c_void_p] * 3
        L.fumi_hip_linear_bwd_weight.argtypes = [c_void_p, c_void_p] + [c_int] * 3 + [c_void_p] * 4
        L.fumi_hip_sample_episodes.argtypes = [c_void_p, c_void_p, ctypes.c_uint64, ctypes.c_uint64] + [c_int] * 5 + [c_void_p] * 5
        L.fumi_hip_sample_episodes_tm.argtypes = ([c_void_p, c_void_p, ctypes.c_uint64, ctypes.c_uint64] + [c_int] * 5 + [c_void_p] * 2
                                                  + [c_int] + [c_void_p] * 4)
        L.fumi_hip_gather_rows.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]
        L.fumi_hip_gather_images.argtypes = ([c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_int64,
                                              POINTER(c_float), POINTER(c_float), ctypes.c_uint64, ctypes.c_uint64, c_int, c_int, c_int]
                                             + [c_float] * 3 + [c_void_p])
        L.fumi_hip_gather_images_resized.argtypes = ([c_void_p, c_void_p, c_void_p, c_int64] + [c_int] * 5 + [c_void_p, c_int64,
                                                      POINTER(c_float), POINTER(c_float), ctypes.c_uint64, ctypes.c_uint64]
                                                     + [c_int] * 6 + [c_float] * 3 + [c_int] + [c_float] * 3 + [c_void_p])
        L.fumi_hip_publish_scalars.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, ctypes.c_uint64]
        L.fumi_hip_publish_scalars_deferred.argtypes = [c_void_p, c_void_p, c_int, c_void_p, ctypes.c_uint64]
        L.fumi_hip_publish_flush.argtypes = [c_void_p, c_void_p]
        L.fumi_hip_conv4_feature_dim.argtypes = [c_int] * 3
        L.fumi_hip_fumi_conv4_step.argtypes = front + img + text_dims + inner + fumi_io
        L.fumi_hip_maml_conv4_step.argtypes = front + img + inner + maml_io
        L.fumi_hip_conv4_set_option.argtypes = [c_int, c_int]
        L.fumi_hip_resnet12_set_budget.argtypes = [ctypes.c_double]
        L.fumi_hip_fumi_resnet12_step.argtypes = front + img + [PI] + text_dims + inner + [c_int] + fumi_io       # channels | chunk
        L.fumi_hip_maml_resnet12_step.argtypes = front + img + [PI] + inner + [c_int] + maml_io
        L.fumi_hip_resnet12_features.argtypes = [c_void_p, c_void_p] + [c_int] * 6 + [PI, c_void_p, PP, c_void_p]
        L.fumi_hip_resnet12_encode.argtypes = ([c_void_p, c_void_p] + [c_int] * 7 + [PI, c_void_p, c_void_p, PP, c_void_p, c_void_p,
                                                                                  c_int])
        L.fumi_hip_resnet12_encode_bwd.argtypes = [c_void_p, c_void_p] + [c_int] * 7 + [PI] + [c_void_p] * 4 + [c_float, PP]
        L.fumi_hip_resnet12_encode_plan.argtypes = [POINTER(c_int)] * 3
        rn_drop = [POINTER(c_float), PI, ctypes.c_uint64]                                     # drop_rate, drop_block, drop_seed
        L.fumi_hip_resnet12_encode_drop.argtypes = L.fumi_hip_resnet12_encode.argtypes + rn_drop
        L.fumi_hip_resnet12_encode_bwd_drop.argtypes = L.fumi_hip_resnet12_encode_bwd.argtypes + rn_drop
        L.fumi_hip_rn12_drop_apply.argtypes = ([c_void_p, c_void_p] + [c_int] * 5 + [c_float, c_int, ctypes.c_uint64] + [c_int] * 3 +
                                               [c_void_p] * 3)
        L.fumi_hip_am3_step_plan.argtypes = [POINTER(c_int), c_int]
        L.fumi_hip_rn12_conv.argtypes = [c_void_p, c_void_p] + [c_int] * 8 + [c_void_p] * 4
        L.fumi_hip_rn12_wgrad.argtypes = [c_void_p, c_void_p] + [c_int] * 7 + [c_void_p] * 3
        LL = ctypes.c_longlong
        L.fumi_hip_rn12_conv_multi.argtypes = ([c_void_p, c_void_p] + [c_int] * 6 + [POINTER(c_int), POINTER(c_int), POINTER(c_void_p),
                                               POINTER(LL), POINTER(c_void_p), POINTER(LL), c_int, c_void_p, LL, c_void_p, LL, c_void_p])
        L.fumi_hip_rn12_wgrad_multi.argtypes = [c_void_p, c_void_p] + [c_int] * 10 + [c_void_p] * 4 + [LL, LL, c_void_p, LL]
        L.fumi_hip_rn12_conv_plan.argtypes = [POINTER(c_int), c_int]
        L.fumi_hip_rn12_conv_query.argtypes = [c_int] * 6 + [POINTER(c_int), POINTER(c_int), c_int]
        L.fumi_hip_rn12_wgrad_query.argtypes = [c_int] * 9 + [POINTER(c_int), c_int]
        L.fumi_hip_rn12_ew_act.argtypes = [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p] * 4
        L.fumi_hip_rn12_ew_bwd.argtypes = [c_void_p, c_void_p] + [c_int] * 7 + [c_void_p] * 6
        L.fumi_hip_rn12_ew_join.argtypes = [c_void_p, c_void_p] + [c_int] * 8 + [c_void_p] * 10
        L.fumi_hip_rn12_ew_coef.argtypes = ([c_void_p, c_void_p] + [c_int] * 8 + [c_float] + [c_void_p] * 4 + [LL] + [c_void_p] * 2 + [LL]
                                            + [c_void_p] * 2 + [LL, c_void_p])
        L.fumi_hip_rn12_ew_avgpool.argtypes = [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p] * 2
        L.fumi_hip_rn12_ew_img_prep.argtypes = [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p] * 2
        L.fumi_hip_rn12_ew_query.argtypes = [c_int] * 8 + [POINTER(c_int), c_int]
        L.fumi_hip_rn12_ew_plan.argtypes = [POINTER(c_int), c_int]
        L.fumi_hip_rn12_coef_query.argtypes = [c_int] * 5 + [POINTER(c_int), c_int]
        L.fumi_hip_resnet12_set_option.argtypes = [c_int, c_int]
        L.fumi_hip_rn12_probe.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_size_t, POINTER(c_size_t),
                                          POINTER(c_int)]
        L.fumi_hip_conv4_features.argtypes = [c_void_p, c_void_p] + [c_int] * 6 + [c_void_p, PP, c_void_p]
        L.fumi_hip_conv4_encode.argtypes = [c_void_p, c_void_p] + [c_int] * 7 + [c_void_p, c_void_p, PP, c_void_p, c_void_p, c_int]
        L.fumi_hip_conv4_encode_bwd.argtypes = [c_void_p, c_void_p] + [c_int] * 7 + [c_void_p] * 4 + [c_float, PP]
        L.fumi_hip_conv4_probe.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_size_t, POINTER(c_size_t)]
        for fn in (L.fumi_hip_conv3x3_fwd, L.fumi_hip_conv3x3_bwd_data, L.fumi_hip_conv3x3_bwd_weight):
            fn.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
        L.fumi_hip_sgd_axpy.argtypes = [c_void_p, c_void_p, ctypes.c_long, c_void_p, c_float, c_void_p, c_void_p]
        L.fumi_hip_ce_fwd_bwd.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        L.fumi_hip_clip_step.argtypes = [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, PP, c_int, c_void_p, c_void_p, PP]
        L.fumi_hip_lstm_bidir.argtypes = [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, c_int64, c_void_p, c_int64, PP, c_int, c_void_p]
        L.fumi_hip_lstm_tape_floats.argtypes = [c_int] * 4
        L.fumi_hip_lstm_tape_floats.restype = c_int64
        L.fumi_hip_lstm_bidir_train.argtypes = [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, c_int64, c_void_p, c_int64, PP, c_int,
                                                c_void_p, c_void_p]
        L.fumi_hip_lstm_bidir_bwd.argtypes = [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, c_int64, PP, c_int, c_void_p, c_void_p, PP]
        L.fumi_hip_proto_reduce.argtypes = [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p] * 3
        cls_lead = [c_void_p, c_void_p] + [c_int] * 3 + [c_void_p] * 2       # ws, stream, M, F, C, feats, y_a
        cls_soft = [c_void_p] + [c_float] * 2                               # y_b, lam, smoothing
        cls_tail = [c_void_p] * 3 + [c_void_p] * 3                          # loss, correct, preds, the three gradients
        L.fumi_hip_cls_head_step.argtypes = cls_lead + [c_void_p] * 2 + [c_float] + cls_tail
        for fn in (L.fumi_hip_cls_head_step_soft, L.fumi_hip_cos_cls_head_step):
            fn.argtypes = cls_lead + cls_soft + [c_void_p] * 2 + [c_float] + cls_tail
        # the teacher and the KD scalars before grad_scale; loss_parts after loss and agree after correct
        L.fumi_hip_cls_head_step_distill.argtypes = (cls_lead + cls_soft + [c_void_p] * 5 + [c_float] * 4 + [c_void_p] * 2
                                                     + cls_tail[1:2] + [c_void_p] + cls_tail[2:])
        L.fumi_hip_mix_images.argtypes = ([c_void_p, c_void_p] + [c_int] * 4 + [c_void_p, c_void_p, c_int, c_float] + [c_int] * 4
                                          + [c_void_p])
        L.fumi_hip_cos_proto_step.argtypes = [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p] * 5 + [c_float] + [c_void_p] * 7
        L.fumi_hip_ridge_head_step.argtypes = [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p] * 5 + [c_float] + [c_void_p] * 7
        L.fumi_hip_euclid_proto_step.argtypes = [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p] * 5 + [c_float] + [c_void_p] * 7
        L.fumi_hip_match_head_step.argtypes = [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p] * 5 + [c_float] + [c_void_p] * 7
        L.fumi_hip_relation_head_step.argtypes = ([c_void_p, c_void_p] + [c_int] * 6 + [c_void_p] * 8 + [c_int, c_float]
                                                  + [c_void_p] * 12)
        L.fumi_hip_feat_adapt_tape_floats.argtypes = [c_int] * 3
        L.fumi_hip_feat_adapt_tape_floats.restype = c_int64
        L.fumi_hip_feat_adapt_fwd.argtypes = [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p] * 9
        L.fumi_hip_feat_adapt_bwd.argtypes = [c_void_p, c_void_p] + [c_int] * 4 + [c_void_p] * 15
        L.fumi_hip_logreg_head_step.argtypes = ([c_void_p, c_void_p] + [c_int] * 5 + [c_void_p] * 4 + [c_int] + [c_float] * 3 + [c_int]
                                                + [c_void_p] * 4)
        L.fumi_hip_logreg_set_form.argtypes = [c_int]
        L.fumi_hip_trans_proto_step.argtypes = [c_void_p, c_void_p] + [c_int] * 5 + [c_void_p] * 5 + [c_int] * 2 + [c_void_p] * 4
        L.fumi_hip_svm_head_step.argtypes = ([c_void_p, c_void_p] + [c_int] * 5 + [c_void_p] * 5 + [c_float] * 2 + [c_int] * 2 + [c_float]
                                             + [c_void_p] * 8)
        L.fumi_hip_svm_set_form.argtypes = [c_int]
        L.fumi_hip_svm_get_fit.argtypes = [c_void_p, c_void_p] + [c_int] * 3 + [c_void_p] * 2
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        L = lib()
        msg = L.fumi_hip_strerror(rc).decode()
        if rc == -3:
            msg += ": " + L.fumi_hip_last_hip_error().decode()
        raise FumiHipError(f"{what} failed: {msg} ({rc})")


def _dev(t):
    if isinstance(t, RowRef):
        t = t.table
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise FumiHipError("the MI355X engine needs GPU tensors (there is no CPU path); got "
                           f"{getattr(t, 'device', type(t))}")
    return t.device


def _f32(t, name):
    _dev(t)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise FumiHipError(f"{name}: expected a contiguous float32 tensor, got {t.dtype} contiguous={t.is_contiguous()}")
    return c_void_p(t.data_ptr())


def _i64(t, name):
    _dev(t)
    if t.dtype != torch.int64 or not t.is_contiguous():
        raise FumiHipError(f"{name}: expected a contiguous int64 tensor, got {t.dtype}")
    return c_void_p(t.data_ptr())


def _shape(t, shape, name):
    """The kernels index raw pointers with the sizes they are told: a tensor of another shape would be read out of bounds (the
    reference raises a matmul shape error there, e.g. an embedding file whose width differs from --im_emb_dim)."""
    got = tuple(t.shape)
    if got != tuple(shape):
        raise FumiHipError(f"{name}: expected shape {tuple(shape)}, got {got}")


def _text_grad(g, dev, B, rows, Dt, name):
    """The optional text-gradient buffer of a step (include/fumi_hip.h, "The text gradient"): float32 [B, rows, Dt] or
    [B * rows, Dt] on the step's device.  None -> NULL."""
    if g is None:
        return None
    if tuple(g.shape) not in ((B, rows, Dt), (B * rows, Dt)):
        raise FumiHipError(f"{name}: expected shape {(B, rows, Dt)} or {(B * rows, Dt)}, got {tuple(g.shape)}")
    if g.device != dev:
        raise FumiHipError(f"{name}: on {g.device}, the step runs on {dev}")
    return _f32(g, name)


def _mlp_shapes(params, D, name, n_layers):
    d = D
    for i in range(n_layers):
        h = int(params[2 * i].shape[0])
        _shape(params[2 * i], (h, d), f"{name}[{2 * i}] (weight of layer {i})")
        _shape(params[2 * i + 1], (h,), f"{name}[{2 * i + 1}] (bias of layer {i})")
        d = h
    return d


_PARR_CACHE = {}


def _parr(tensors, name):
    """Pointer table of a parameter / gradient list.  The lists are the same tensors step after step, so a validated table is
    kept per (name, data pointers) -- rebuilding it costs more host time than the launch it feeds."""
    key = (name,) + tuple(t.data_ptr() for t in tensors)
    arr = _PARR_CACHE.get(key)
    if arr is not None:
        for t in tensors:                         # an address can be reused by a different tensor: keep the type check
            if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                arr = None
                break
    if arr is None:
        arr = (c_void_p * len(tensors))()
        for i, t in enumerate(tensors):
            arr[i] = _f32(t, f"{name}[{i}]").value
        if len(_PARR_CACHE) > 256:
            _PARR_CACHE.clear()
        _PARR_CACHE[key] = arr
    return arr


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device):
    """The caller's current stream on `device` (torch.cuda.current_stream builds a Stream object: ~1.4 us a call, and a step
    asks several times)."""
    if _RAW_STREAM is not None:
        idx = device.index
        return c_void_p(_RAW_STREAM(idx if idx is not None else torch.cuda.current_device()))
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Workspace:
    """One per (process, device).  Owns the engine's scratch slab; not re-entrant."""

    _per_device = {}

    def __init__(self, device, bytes_hint=0):
        device = torch.device(device)
        if device.type != "cuda":
            raise FumiHipError("the MI355X engine has no CPU path")
        self.device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        h = c_void_p()
        with torch.cuda.device(self.device):
            _check(lib().fumi_hip_workspace_create(self.device.index, bytes_hint, ctypes.byref(h)), "workspace_create")
        self._h = h

    @classmethod
    def get(cls, device, role=None):
        """The device's workspace; ``role`` names a further one (the Conv4 encoder's tape lives in its own slab, so that the
        step it feeds can lay out the main one)."""
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = idx if role is None else (idx, role)
        ws = cls._per_device.get(key)
        if ws is None:
            ws = cls._per_device[key] = Workspace(torch.device("cuda", idx))
        return ws

    @property
    def handle(self):
        return self._h

    def bytes(self):
        return int(lib().fumi_hip_workspace_bytes(self._h))

    def read_status(self):
        """Synchronises the current stream; returns and clears the device status bits."""
        st = c_int(0)
        _check(lib().fumi_hip_read_status(self._h, _stream(self.device), ctypes.byref(st)), "read_status")
        return st.value

    def set_profiling(self, on, phases=None, every=1):
        """HIP-event timing of the library's phases (bench.py); switching it clears the records.  ``phases``: names
        (fumi_hip_phase_name) to time -- an event pair costs stream time (two ~6 us bubbles), so the bench times only the
        kernel its roofline is about and only at every ``every``-th step; None = every phase."""
        _check(lib().fumi_hip_set_profiling_every(self._h, max(1, int(every))), "set_profiling_every")
        mask = 0
        if on:
            if phases is None:
                mask = -1
            else:
                names = {lib().fumi_hip_phase_name(i).decode(): i for i in range(32)}
                for p in phases:
                    mask |= 1 << names[p]
        _check(lib().fumi_hip_set_profiling(self._h, mask), "set_profiling")

    def profile(self):
        """{phase name: (total ms, launches)} since profiling was switched on (synchronises the device)."""
        out = {}
        L = lib()
        for ph in range(N_PHASES):
            ms, n = ctypes.c_double(0), c_int(0)
            _check(L.fumi_hip_get_profile(self._h, ph, ctypes.byref(ms), ctypes.byref(n)), "get_profile")
            if n.value:
                out[L.fumi_hip_phase_name(ph).decode()] = (ms.value, n.value)
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().fumi_hip_workspace_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def raise_on_status(status):
    if status & ST_SYNC_TIMEOUT:
        raise RuntimeError("a workgroup timed out waiting for the sibling workgroups of its episode "
                           "(FUMI_ST_SYNC_TIMEOUT): the results of that step are invalid")
    if status & ST_NOT_POSDEF:
        raise FloatingPointError("a pivot of the ridge head's Cholesky factorisation was not positive (FUMI_ST_NOT_POSDEF): "
                                 "non-finite features or a ridge weight that underflowed")
    if status & ST_CLASS_MISSING:
        raise IndexError("a class has no support sample (the reference raises IndexError at fumi/models/fumi.py:209)")
    if status & ST_LABEL_RANGE:
        raise IndexError("label / token id out of range")


# ----------------------------------------------------------------------------------------------------------------
def fumi_step(ws, x_s, y_s, x_q, y_q, theta, phi, T, alpha, tanh_head, *, cls_text=None, text_s=None,
              need_grad=True, grad_scale=None, g_theta=None, g_phi=None, stats=None, dropout_p=0.0, seed=0, g_cls_text=None):
    """One FuMI meta-step over B episodes (fumi/models/fumi.py:146-192).  Returns a dict of GPU tensors.  ``g_cls_text``: optional
    fp32 [B, N, Dt] buffer that a step with ``need_grad`` fills with the adjoint of the class text rows."""
    dev = _dev(x_s)
    B, S, D = x_s.shape
    Qn = x_q.shape[1]
    n_hidden = len(theta) // 2
    hid = [int(theta[2 * i].shape[0]) for i in range(n_hidden)]
    Ht, Dt = int(phi[0].shape[0]), int(phi[0].shape[1])
    N = int((cls_text.shape[1]) if cls_text is not None else 0) or None
    if N is None:
        raise FumiHipError("fumi_step: pass n_way through cls_text=[B,N,Dt] or use fumi_step_select")
    return _fumi_step(ws, dev, B, N, S, Qn, D, hid, Dt, Ht, x_s, y_s, x_q, y_q, theta, phi, T, alpha, tanh_head,
                      cls_text, text_s, need_grad, grad_scale, g_theta, g_phi, stats, dropout_p, seed, g_cls_text)


def fumi_step_select(ws, n_way, x_s, y_s, x_q, y_q, text_s, theta, phi, T, alpha, tanh_head, *,
                     need_grad=True, grad_scale=None, g_theta=None, g_phi=None, stats=None, dropout_p=0.0, seed=0,
                     g_cls_text=None):
    """Same, selecting the per-class text rows from text_s [B,S,Dt] on the device (fumi.py:207-210)."""
    dev = _dev(x_s)
    B, S, D = x_s.shape
    Qn = x_q.shape[1]
    n_hidden = len(theta) // 2
    hid = [int(theta[2 * i].shape[0]) for i in range(n_hidden)]
    Ht, Dt = int(phi[0].shape[0]), int(phi[0].shape[1])
    return _fumi_step(ws, dev, B, n_way, S, Qn, D, hid, Dt, Ht, x_s, y_s, x_q, y_q, theta, phi, T, alpha, tanh_head,
                      None, text_s, need_grad, grad_scale, g_theta, g_phi, stats, dropout_p, seed, g_cls_text)


# Parameter / gradient LISTS that a model hands over unchanged step after step (the same list objects: fumi_amd/models cache
# them) are validated once: shapes, dtypes, contiguity and the pointer tables are remembered per tuple of list identities
# (the lists are held here, so an id cannot be recycled) and re-checked only through the first tensor's address.  Callers that
# build fresh lists every call take the full checks every call.
_PARAMSETS = {}


def _paramset(key_lists, dims, build):
    key = tuple(id(x) for x in key_lists) + dims
    ent = _PARAMSETS.get(key)
    if ent is not None and all(a is b for a, b in zip(ent[0], key_lists)) and ent[1] == key_lists[0][0].data_ptr():
        return ent[2]
    val = build()
    if len(_PARAMSETS) > 64:
        _PARAMSETS.clear()
    _PARAMSETS[key] = (tuple(key_lists), key_lists[0][0].data_ptr(), val)
    return val


def _step_outputs(dev, B, Qn, N):
    """logits, preds, preds_f (the reference's float test_preds, same launch), loss_b, acc_b of a meta-step."""
    return (torch.empty(B, Qn, N, device=dev, dtype=torch.float32), torch.empty(B, Qn, device=dev, dtype=torch.int64),
            torch.empty(B, Qn, device=dev, dtype=torch.float32), torch.empty(B, device=dev, dtype=torch.float32),
            torch.empty(B, device=dev, dtype=torch.float32))


def _fumi_step(ws, dev, B, N, S, Qn, D, hid, Dt, Ht, x_s, y_s, x_q, y_q, theta, phi, T, alpha, tanh_head,
               cls_text, text_s, need_grad, grad_scale, g_theta, g_phi, stats=None, dropout_p=0.0, seed=0, g_cls_text=None):
    L = lib()

    def check_params():
        if len(theta) != 2 * len(hid) or len(phi) != 4 or not hid:
            raise FumiHipError("fumi_step: theta must hold (weight, bias) per hidden layer and phi the 4 hypernetwork tensors")
        H = _mlp_shapes(theta, D, "theta", len(hid))
        _shape(phi[0], (Ht, Dt), "phi[0]"); _shape(phi[1], (Ht,), "phi[1]"); _shape(phi[2], (H + 1, Ht), "phi[2]")
        _shape(phi[3], (H + 1,), "phi[3]")
        if need_grad and g_theta is not None:
            for i, (g, t) in enumerate(zip(list(g_theta) + list(g_phi or []), list(theta) + list(phi))):
                _shape(g, t.shape, f"gradient buffer {i}")
        return (_parr(theta, "theta"), _parr(phi, "phi"),
                _parr(g_theta, "g_theta") if (need_grad and g_theta is not None) else None,
                _parr(g_phi, "g_phi") if (need_grad and g_phi is not None) else None)

    if need_grad and g_theta is not None and g_phi is not None:
        arrs = _paramset((theta, phi, g_theta, g_phi), (D, Dt, Ht, tuple(hid)), check_params)
    else:
        arrs = check_params()
    _shape(x_q, (B, Qn, D), "x_q"); _shape(y_s, (B, S), "y_s"); _shape(y_q, (B, Qn), "y_q")
    if cls_text is not None:
        _shape(cls_text, (B, N, Dt), "cls_text")
    else:
        _shape(text_s, (B, S, Dt), "text_s")
    g_ct = _text_grad(g_cls_text, dev, B, N, Dt, "g_cls_text")
    logits, preds, preds_f, loss_b, acc_b = _step_outputs(dev, B, Qn, N)
    if need_grad:
        if g_theta is None:
            g_theta = [torch.empty_like(t) for t in theta]
        if g_phi is None:
            g_phi = [torch.empty_like(t) for t in phi]
    if grad_scale is None:
        grad_scale = 1.0 / B
    hid_arr = (c_int * len(hid))(*hid)
    head = (ws.handle, _stream(dev), B, N, S, Qn, D, len(hid), hid_arr, Dt, Ht, int(T), float(alpha), int(bool(tanh_head)),
            int(bool(need_grad)), float(grad_scale), float(dropout_p), int(seed) & 0xFFFFFFFFFFFFFFFF)
    if isinstance(x_s, RowRef) or isinstance(x_q, RowRef):             # zero-copy episodes: rows stay in the table
        if not (isinstance(x_s, RowRef) and isinstance(x_q, RowRef)) or x_s.table.data_ptr() != x_q.table.data_ptr():
            raise FumiHipError("zero-copy episodes: support and query rows must be RowRefs into the same table")
        fn, rows = L.fumi_hip_fumi_step_indexed, (_f32(x_s.table, "table"), int(x_s.table.shape[0]), _i64(x_s.idx, "idx_s"),
                                                  _i64(y_s, "y_s"), _i64(x_q.idx, "idx_q"), _i64(y_q, "y_q"))
    else:
        fn, rows = L.fumi_hip_fumi_step, (_f32(x_s, "x_s"), _i64(y_s, "y_s"), _f32(x_q, "x_q"), _i64(y_q, "y_q"))
    rc = fn(
        *head, *rows,
        _f32(cls_text, "cls_text") if cls_text is not None else None,
        _f32(text_s, "text_s") if text_s is not None else None,
        arrs[0], arrs[1],
        c_void_p(logits.data_ptr()), c_void_p(preds.data_ptr()), c_void_p(preds_f.data_ptr()), c_void_p(loss_b.data_ptr()),
        c_void_p(acc_b.data_ptr()),
        _f32(stats, "stats") if stats is not None else None,
        (arrs[2] if arrs[2] is not None else _parr(g_theta, "g_theta")) if need_grad else None,
        (arrs[3] if arrs[3] is not None else _parr(g_phi, "g_phi")) if need_grad else None,
        g_ct)
    _check(rc, "fumi_hip_fumi_step")
    return dict(logits=logits, preds=preds, preds_f=preds_f, loss_b=loss_b, acc_b=acc_b, g_theta=g_theta, g_phi=g_phi, stats=stats)


def maml_step(ws, x_s, y_s, x_q, y_q, params, T, alpha, first_order=False, *, need_grad=True, grad_scale=None,
              g_params=None, stats=None):
    """One MAML meta-step (fumi/models/maml.py:156-191).  params = hidden (W,b)* then lin_final W [N,H], b [N]."""
    dev = _dev(x_s)
    L = lib()
    B, S, D = x_s.shape
    Qn = x_q.shape[1]
    n_hidden = len(params) // 2 - 1
    if n_hidden < 0 or len(params) != 2 * n_hidden + 2:
        raise FumiHipError("maml_step: params must hold (weight, bias) per hidden layer, then lin_final's")
    hid = [int(params[2 * i].shape[0]) for i in range(n_hidden)]
    N = int(params[-2].shape[0])
    H = _mlp_shapes(params, D, "params", n_hidden)
    _shape(params[-2], (N, H), "params[-2] (lin_final.weight)"); _shape(params[-1], (N,), "params[-1] (lin_final.bias)")
    _shape(x_q, (B, Qn, D), "x_q"); _shape(y_s, (B, S), "y_s"); _shape(y_q, (B, Qn), "y_q")
    if need_grad and g_params is not None:
        for i, (g, t) in enumerate(zip(g_params, params)):
            _shape(g, t.shape, f"g_params[{i}]")
    logits, preds, preds_f, loss_b, acc_b = _step_outputs(dev, B, Qn, N)
    if need_grad and g_params is None:
        g_params = [torch.empty_like(t) for t in params]
    if grad_scale is None:
        grad_scale = 1.0 / B
    hid_arr = (c_int * max(1, len(hid)))(*hid)
    rc = L.fumi_hip_maml_step(
        ws.handle, _stream(dev), B, N, S, Qn, D, n_hidden, hid_arr, int(T), float(alpha), int(bool(first_order)),
        int(bool(need_grad)), float(grad_scale),
        _f32(x_s, "x_s"), _i64(y_s, "y_s"), _f32(x_q, "x_q"), _i64(y_q, "y_q"), _parr(params, "params"),
        _f32(logits, "logits"), _i64(preds, "preds"), _f32(preds_f, "preds_f"), _f32(loss_b, "loss_b"), _f32(acc_b, "acc_b"),
        _f32(stats, "stats") if stats is not None else None,
        _parr(g_params, "g_params") if need_grad else None)
    _check(rc, "fumi_hip_maml_step")
    return dict(logits=logits, preds=preds, preds_f=preds_f, loss_b=loss_b, acc_b=acc_b, g_params=g_params, stats=stats)


# the plan of the episode chain (csrc/episode.hip: plan_episodes), in the order fumi_hip_epi_plan writes it.  An entry of a form the
# plan did not take is 0.
EPI_PLAN_KEYS = ("adapt", "AP", "query", "reverse", "P", "two_part", "nsq", "nss", "drop", "fixed_last",
                 "ql_total", "al_total", "rl_total", "nu_adapt", "nu_query", "nu_fused", "nu_rev_init", "nu_rev_step")
EPI_ADAPT_FORMS = {0: "none", 1: "lds", 2: "global"}
EPI_QUERY_FORMS = {0: "fused_fixed", 1: "fused", 2: "lds", 3: "global"}
EPI_REVERSE_FORMS = {0: "lds_fixed", 1: "lds", 2: "global"}
# flags of fumi_hip_epi_plan_query (include/fumi_hip.h: FUMI_EPI_Q_*)
EPI_Q_HEAD, EPI_Q_SIDE, EPI_Q_PROFILING, EPI_Q_AFTER_REVERSE, EPI_Q_W_OFF_SHIFT, EPI_Q_B_OFF_SHIFT = 1, 2, 4, 8, 8, 16


def epi_plan():
    """dict over EPI_PLAN_KEYS: the forms the episode chain of the last FuMI / MAML step of this process took (fumi_hip_epi_plan;
    the form ids are named by EPI_ADAPT_FORMS / EPI_QUERY_FORMS / EPI_REVERSE_FORMS)."""
    v = (c_int * len(EPI_PLAN_KEYS))()
    _check(lib().fumi_hip_epi_plan(v, len(EPI_PLAN_KEYS)), "fumi_hip_epi_plan")
    return {k: int(x) for k, x in zip(EPI_PLAN_KEYS, v)}


def epi_plan_query(B, N, S, Qn, D, hid, T, *, need_grad=True, second_order=True, dropout=False, head=True, side=True,
                   profiling=False, after_reverse=False, w_off=(), b_off=()):
    """The same dict for a shape (fumi_hip_epi_plan_query): host arithmetic only, runs without a GPU.  ``w_off`` / ``b_off``: the
    hidden layers whose weight / bias starts one float past a 16-byte boundary.  The environment knobs are the process's own."""
    flags = ((EPI_Q_HEAD if head else 0) | (EPI_Q_SIDE if side else 0) | (EPI_Q_PROFILING if profiling else 0)
             | (EPI_Q_AFTER_REVERSE if after_reverse else 0))
    for i in w_off:
        flags |= 1 << (EPI_Q_W_OFF_SHIFT + int(i))
    for i in b_off:
        flags |= 1 << (EPI_Q_B_OFF_SHIFT + int(i))
    hid_arr = (c_int * len(hid))(*[int(x) for x in hid])
    v = (c_int * len(EPI_PLAN_KEYS))()
    _check(lib().fumi_hip_epi_plan_query(B, N, S, Qn, D, len(hid), hid_arr, int(T), int(bool(need_grad)), int(bool(second_order)),
                                         int(bool(dropout)), flags, v, len(EPI_PLAN_KEYS)), "fumi_hip_epi_plan_query")
    return {k: int(x) for k, x in zip(EPI_PLAN_KEYS, v)}


# what the hypernetwork of the last FuMI step took (csrc/hyper.hip, the rider branches of csrc/xpanel.hip), in the order
# fumi_hip_hyper_plan writes it
HYPER_PLAN_KEYS = ("fwd_form", "fwd_inst", "nrb", "nch", "bwd_form", "bwd_dpasses", "text_grad")
HYPER_FWD_FORMS = {0: "gemm", 1: "per_layer", 2: "fused", 3: "split", 4: "rode_split", 5: "rode_presplit"}
HYPER_BWD_FORMS = {0: "none", 1: "gemm", 2: "two_launch", 3: "fused", 4: "rode"}
HYPER_TEXT_GRAD = {0: "none", 1: "gemm_after", 2: "in_fallback"}
# flags of fumi_hip_hyper_plan_query (include/fumi_hip.h: FUMI_HYPER_Q_*)
HYPER_Q_SIDE, HYPER_Q_TEXT_GRAD, HYPER_Q_CLS_TEXT_OFF, HYPER_Q_PHI_OFF_SHIFT = 1, 2, 4, 8


def hyper_plan():
    """dict over HYPER_PLAN_KEYS: the forms the hypernetwork of the last FuMI step of this process took (fumi_hip_hyper_plan)."""
    v = (c_int * len(HYPER_PLAN_KEYS))()
    _check(lib().fumi_hip_hyper_plan(v, len(HYPER_PLAN_KEYS)), "fumi_hip_hyper_plan")
    return {k: int(x) for k, x in zip(HYPER_PLAN_KEYS, v)}


def hyper_plan_query(B, N, S, Qn, D, hid, Dt, Ht, T, *, need_grad=True, want_text_grad=False, side=True, cls_text_off=False,
                     phi_off=()):
    """The same dict for a shape (fumi_hip_hyper_plan_query): host arithmetic only, runs without a GPU.  ``cls_text_off`` /
    ``phi_off``: the class text rows / the hypernetwork tensors (indices into phi) that start one float past a 16-byte boundary.
    The environment knobs are the process's own."""
    flags = (HYPER_Q_SIDE if side else 0) | (HYPER_Q_TEXT_GRAD if want_text_grad else 0) | (HYPER_Q_CLS_TEXT_OFF if cls_text_off else 0)
    for i in phi_off:
        flags |= 1 << (HYPER_Q_PHI_OFF_SHIFT + int(i))
    hid_arr = (c_int * len(hid))(*[int(x) for x in hid])
    v = (c_int * len(HYPER_PLAN_KEYS))()
    _check(lib().fumi_hip_hyper_plan_query(B, N, S, Qn, D, len(hid), hid_arr, int(Dt), int(Ht), int(T), int(bool(need_grad)), flags,
                                           v, len(HYPER_PLAN_KEYS)), "fumi_hip_hyper_plan_query")
    return {k: int(x) for k, x in zip(HYPER_PLAN_KEYS, v)}


AM3_KEYS = ["Wi", "bi", "G0", "g0", "G1", "g1", "H0", "h0", "H1", "h1"]


def am3_step(ws, x_s, y_s, x_q, y_q, text_s, w, n_way, lamda_fixed=None, *, need_grad=True, grad_scale=None, g_w=None,
             dropout_p=0.0, seed=0, stats=None, want_dx=False, g_text=None):
    """One AM3 step (fumi/models/am3.py:160-200).  w: list of the 10 tensors in AM3_KEYS order.  ``stats``: optional fp32
    [3 + n_way**2] device tensor receiving [loss, correct count, grad_scale * sum of the episodes' mean lamda, confusion
    counts] (the input of ``am3_metrics``).  ``g_text``: optional fp32 [B, S, Dt] buffer that a step with ``need_grad`` fills with
    the adjoint of ``text_s``."""
    dev = _dev(x_s)
    L = lib()
    B, S, D = x_s.shape
    Qn = x_q.shape[1]
    if len(w) != 10:
        raise FumiHipError("am3_step: w must hold the 10 tensors of AM3_KEYS")
    P, Ht, Dt = int(w[0].shape[0]), int(w[2].shape[0]), int(w[2].shape[1])

    def check_params():
        for t, shp, k in zip(w, [(P, D), (P,), (Ht, Dt), (Ht,), (P, Ht), (P,), (Ht, P), (Ht,), (1, Ht), (1,)], AM3_KEYS):
            _shape(t, shp, f"w[{k}]")
        if need_grad and g_w is not None:
            for g, t, k in zip(g_w, w, AM3_KEYS):
                _shape(g, t.shape, f"g_w[{k}]")
        return (_parr(w, "w"), _parr(g_w, "g_w") if (need_grad and g_w is not None) else None)

    arrs = _paramset((w, g_w), (D,), check_params) if (need_grad and g_w is not None) else check_params()
    _shape(x_q, (B, Qn, D), "x_q"); _shape(y_s, (B, S), "y_s"); _shape(y_q, (B, Qn), "y_q"); _shape(text_s, (B, S, Dt), "text_s")
    g_t = _text_grad(g_text, dev, B, S, Dt, "g_text")
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    correct = torch.empty(1, device=dev, dtype=torch.float32)
    preds = torch.empty(B, Qn, device=dev, dtype=torch.int64)
    lam = torch.empty(B, S, device=dev, dtype=torch.float32)
    if need_grad and g_w is None:
        g_w = [torch.empty_like(t) for t in w]
    lf = -1 if lamda_fixed is None else int(lamda_fixed)
    if grad_scale is None:
        grad_scale = 1.0 / B
    args = [ws.handle, _stream(dev), B, n_way, S, Qn, D, Dt, Ht, P, lf, int(bool(need_grad)), float(grad_scale),
            float(dropout_p), int(seed) & 0xFFFFFFFFFFFFFFFF,
            _f32(x_s, "x_s"), _i64(y_s, "y_s"), _f32(x_q, "x_q"), _i64(y_q, "y_q"), _f32(text_s, "text_s"),
            arrs[0], c_void_p(loss.data_ptr()), c_void_p(preds.data_ptr()), c_void_p(lam.data_ptr()), c_void_p(correct.data_ptr()),
            (arrs[1] if arrs[1] is not None else _parr(g_w, "g_w")) if need_grad else None,
            _f32(stats, "stats") if stats is not None else None]
    dx_s = dx_q = None
    if want_dx and need_grad:               # adjoints of the image rows (an encoder in front of the step continues from them)
        dx_s, dx_q = torch.empty_like(x_s), torch.empty_like(x_q)
        _check(L.fumi_hip_am3_step_dx(*args, _f32(dx_s, "dx_s"), _f32(dx_q, "dx_q"), g_t), "fumi_hip_am3_step_dx")
    else:
        _check(L.fumi_hip_am3_step(*args, g_t), "fumi_hip_am3_step")
    return dict(loss=loss, preds=preds, lamda_s=lam, correct=correct, grads=g_w, stats=stats, dx_s=dx_s, dx_q=dx_q)


def _parr_opt(tensors, name):
    """``_parr`` for a list with ``None`` entries (NULL in the table): the text-rows form of the AM3 step never touches g's slots."""
    key = (name,) + tuple(0 if t is None else t.data_ptr() for t in tensors)
    arr = _PARR_CACHE.get(key)
    if arr is not None:
        for t in tensors:
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
                arr = None
                break
    if arr is None:
        arr = (c_void_p * len(tensors))()
        for i, t in enumerate(tensors):
            arr[i] = None if t is None else _f32(t, f"{name}[{i}]").value
        if len(_PARR_CACHE) > 256:
            _PARR_CACHE.clear()
        _PARR_CACHE[key] = arr
    return arr


def am3_step_tx(ws, x_s, y_s, x_q, y_q, text_rows, w, n_way, lamda_fixed=None, *, need_grad=True, grad_scale=None, g_w=None,
                dropout_p=0.0, seed=0, stats=None, want_dx=False, g_text=None):
    """The text-rows form of the AM3 step (fumi/models/am3.py:118-126 then :160-200, ``text_encoder='rand'``): the text prototypes are
    rows of the prototype space, g is not applied and dropout acts in h only.  ``text_rows``: fp32 [B, S, P], or ``None`` -- then the
    step draws them uniformly on [-1, 1) from ``seed`` on the device.  ``w`` / ``g_w`` keep the AM3_KEYS layout; entries 2..5 (g) may
    be ``None`` and are never read or written.  Returns what ``am3_step`` returns plus ``"tx"``, the rows the step used.  No text
    adjoint exists in this form: a ``g_text`` other than ``None`` is refused before anything is launched."""
    if g_text is not None:
        raise FumiHipError("am3_step_tx: invalid argument: the text-rows form has no text adjoint, g_text must be None")
    dev = _dev(x_s)
    L = lib()
    B, S, D = x_s.shape
    Qn = x_q.shape[1]
    if len(w) != 10:
        raise FumiHipError("am3_step_tx: w must hold the 10 entries of AM3_KEYS (entries 2..5 may be None)")
    for i, k in enumerate(AM3_KEYS):
        if w[i] is None and not 2 <= i < 6:
            raise FumiHipError(f"am3_step_tx: w[{k}] is None (only the g entries 2..5 may be)")
    P, Ht = int(w[0].shape[0]), int(w[6].shape[0])
    shapes = [(P, D), (P,), None, None, None, None, (Ht, P), (Ht,), (1, Ht), (1,)]
    for t, shp, k in zip(w, shapes, AM3_KEYS):
        if shp is None:
            if t is not None:
                _f32(t, f"w[{k}]")
        else:
            _shape(t, shp, f"w[{k}]")
    _shape(x_q, (B, Qn, D), "x_q"); _shape(y_s, (B, S), "y_s"); _shape(y_q, (B, Qn), "y_q")
    if text_rows is not None:
        _shape(text_rows, (B, S, P), "text_rows")
        tx = torch.empty_like(text_rows)
    else:
        tx = torch.empty(B, S, P, device=dev, dtype=torch.float32)
    if need_grad:
        if g_w is None:
            g_w = [None if (t is None or 2 <= i < 6) else torch.empty_like(t) for i, t in enumerate(w)]
        elif len(g_w) != 10:
            raise FumiHipError("am3_step_tx: g_w must hold 10 entries (entries 2..5 may be None)")
        for g, t, shp, k in zip(g_w, w, shapes, AM3_KEYS):
            if shp is not None:
                if g is None:
                    raise FumiHipError(f"am3_step_tx: g_w[{k}] is None (only the g entries 2..5 may be)")
                _shape(g, shp, f"g_w[{k}]")
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    correct = torch.empty(1, device=dev, dtype=torch.float32)
    preds = torch.empty(B, Qn, device=dev, dtype=torch.int64)
    lam = torch.empty(B, S, device=dev, dtype=torch.float32)
    lf = -1 if lamda_fixed is None else int(lamda_fixed)
    if grad_scale is None:
        grad_scale = 1.0 / B
    args = [ws.handle, _stream(dev), B, n_way, S, Qn, D, P, Ht, P, lf, int(bool(need_grad)), float(grad_scale),
            float(dropout_p), int(seed) & 0xFFFFFFFFFFFFFFFF,
            _f32(x_s, "x_s"), _i64(y_s, "y_s"), _f32(x_q, "x_q"), _i64(y_q, "y_q"),
            _f32(text_rows, "text_rows") if text_rows is not None else None,
            _parr_opt(w, "w_tx"), c_void_p(loss.data_ptr()), c_void_p(preds.data_ptr()), c_void_p(lam.data_ptr()),
            c_void_p(correct.data_ptr()), _parr_opt(g_w, "g_w_tx") if need_grad else None,
            _f32(stats, "stats") if stats is not None else None, c_void_p(tx.data_ptr())]
    dx_s = dx_q = None
    if want_dx and need_grad:
        dx_s, dx_q = torch.empty_like(x_s), torch.empty_like(x_q)
        _check(L.fumi_hip_am3_step_tx_dx(*args, _f32(dx_s, "dx_s"), _f32(dx_q, "dx_q")), "fumi_hip_am3_step_tx_dx")
    else:
        _check(L.fumi_hip_am3_step_tx(*args), "fumi_hip_am3_step_tx")
    return dict(loss=loss, preds=preds, lamda_s=lam, correct=correct, grads=g_w, stats=stats, dx_s=dx_s, dx_q=dx_q, tx=tx)


AM3_PLAN_KEYS = ["fast_head", "nwaves", "hgq", "imparts", "xks", "g_fwd_split", "g_fwd_rode", "h_fwd_split", "h_bwd_fused",
                 "g_bwd_fused", "tx_nparts", "text_form"]


def am3_step_plan():
    """dict over AM3_PLAN_KEYS: the form the last ``am3_step`` / ``am3_step_tx`` of this process took (fumi_hip_am3_step_plan);
    ``text_form``: 0 = g applied, 1 = prototype-space rows given, 2 = rows drawn on the device."""
    v = (c_int * len(AM3_PLAN_KEYS))()
    _check(lib().fumi_hip_am3_step_plan(v, len(AM3_PLAN_KEYS)), "fumi_hip_am3_step_plan")
    return {k: int(x) for k, x in zip(AM3_PLAN_KEYS, v)}


def am3_metrics(ws, n_way, stats):
    """[loss, acc, macro F1, macro precision, macro recall, mean lamda] (fp32 [6] on the device) from an ``am3_step`` stats
    tensor (summed over ranks first when sharded)."""
    dev = _dev(stats)
    out = torch.empty(6, device=dev, dtype=torch.float32)
    _check(lib().fumi_hip_am3_metrics(ws.handle, _stream(dev), int(n_way), _f32(stats, "stats"), _f32(out, "out6")),
           "fumi_hip_am3_metrics")
    return out


def glove_bag(ws, tokens, table, pad_id, mode="mean"):
    """WordEmbedding.forward (fumi/models/common.py:23-41): tokens [..., L] int64 -> [..., E]."""
    if mode not in ("mean", "max"):
        raise NameError(f"{mode} pooling strat not defined")           # common.py:41
    dev = _dev(tokens)
    Lseq = tokens.shape[-1]
    R = tokens.numel() // Lseq
    V, E = table.shape
    out = torch.empty(*tokens.shape[:-1], E, device=dev, dtype=torch.float32)
    rc = lib().fumi_hip_glove_bag(ws.handle, _stream(dev), _i64(tokens, "tokens"), R, Lseq, int(pad_id),
                                  _f32(table, "table"), V, E, 0 if mode == "mean" else 1, _f32(out, "out"))
    _check(rc, "fumi_hip_glove_bag")
    return out


def glove_bag_select(ws, tokens_s, y_s, n_way, table, pad_id, mode="mean", defer=False):
    """[B,N,E] pooled text of the first support row of each class (fumi.py:207-210 + common.py:23-41 in one kernel).
    defer: nothing is launched; the request rides in the first launch of the FuMI step that MUST follow on ``ws`` with the
    returned tensor as its ``cls_text`` (fumi_hip_glove_bag_select_deferred)."""
    if mode not in ("mean", "max"):
        raise NameError(f"{mode} pooling strat not defined")
    dev = _dev(tokens_s)
    B, S, Lseq = tokens_s.shape
    V, E = table.shape
    out = torch.empty(B, n_way, E, device=dev, dtype=torch.float32)
    if defer:
        rc = lib().fumi_hip_glove_bag_select_deferred(ws.handle, _i64(tokens_s, "tokens"), _i64(y_s, "y_s"), B, n_way, S, Lseq,
                                                      int(pad_id), _f32(table, "table"), V, E, 0 if mode == "mean" else 1,
                                                      _f32(out, "out"))
        _check(rc, "fumi_hip_glove_bag_select_deferred")
        ws._glove_keep = (tokens_s, y_s, table, out)  # (the request holds raw pointers until the step has launched it)
        return out
    rc = lib().fumi_hip_glove_bag_select(ws.handle, _stream(dev), _i64(tokens_s, "tokens"), _i64(y_s, "y_s"), B, n_way, S,
                                         Lseq, int(pad_id), _f32(table, "table"), V, E, 0 if mode == "mean" else 1,
                                         _f32(out, "out"))
    _check(rc, "fumi_hip_glove_bag_select")
    return out


def glove_flush(ws, device):
    """Launches a deferred embedding bag that no step has carried."""
    _check(lib().fumi_hip_glove_flush(ws.handle, _stream(device)), "fumi_hip_glove_flush")


def class_text_select(ws, text_s, y_s, n_way):
    dev = _dev(text_s)
    B, S, Dt = text_s.shape
    out = torch.empty(B, n_way, Dt, device=dev, dtype=torch.float32)
    rc = lib().fumi_hip_class_text_select(ws.handle, _stream(dev), B, n_way, S, Dt, _f32(text_s, "text_s"),
                                          _i64(y_s, "y_s"), _f32(out, "out"))
    _check(rc, "fumi_hip_class_text_select")
    return out


def _out(out, shape, dev, name):
    """A caller-supplied output tensor (tests place it inside a guarded buffer), or a fresh one."""
    if out is None:
        return torch.empty(*shape, device=dev, dtype=torch.float32)
    if tuple(out.shape) != tuple(shape) or out.device != dev:
        raise FumiHipError(f"{name}: expected shape {tuple(shape)} on {dev}, got {tuple(out.shape)} on {out.device}")
    return out


def xpanel_fwd(ws, x_s, x_q, W0, out=None):
    """A0 [B,S+Qn,h0], G [B,S+Qn,S] (support rows first).  ``out``: (A0, G) tensors to write instead of fresh ones."""
    dev = _dev(x_s)
    B, S, D = x_s.shape
    Qn, h0 = x_q.shape[1], W0.shape[0]
    A0 = _out(out[0] if out is not None else None, (B, S + Qn, h0), dev, "A0")
    G = _out(out[1] if out is not None else None, (B, S + Qn, S), dev, "G")
    _check(lib().fumi_hip_xpanel_fwd(ws.handle, _stream(dev), B, S, Qn, D, h0, _f32(x_s, "x_s"), _f32(x_q, "x_q"),
                                     _f32(W0, "W0"), _f32(A0, "A0"), _f32(G, "G")), "fumi_hip_xpanel_fwd")
    return A0, G


def xpanel_fwd_rows(ws, table, idx_s, idx_q, W0, gram=True, out=None):
    """xpanel_fwd over rows of ``table`` [n_rows, D]: row r of episode b is table[idx_s[b, r]] (r < S) or table[idx_q[b, r - S]]
    (int64 indices).  ``gram=False``: A0 only (G is None; no Gram tile runs).  ``out``: (A0, G) tensors to write."""
    dev = _dev(table)
    (B, S), Qn, h0, D = idx_s.shape, idx_q.shape[1], W0.shape[0], table.shape[1]
    for t, name in ((idx_s, "idx_s"), (idx_q, "idx_q")):
        if t.dtype != torch.int64 or not t.is_contiguous() or t.device != table.device:
            raise FumiHipError(f"xpanel_fwd_rows: {name} must be a contiguous int64 tensor on the table's device")
    A0 = _out(out[0] if out is not None else None, (B, S + Qn, h0), dev, "A0")
    G = _out(out[1] if out is not None else None, (B, S + Qn, S), dev, "G") if gram else None
    _check(lib().fumi_hip_xpanel_fwd_rows(ws.handle, _stream(dev), B, S, Qn, D, h0, _f32(table, "table"), table.shape[0],
                                          c_void_p(idx_s.data_ptr()), c_void_p(idx_q.data_ptr()), _f32(W0, "W0"), _f32(A0, "A0"),
                                          _f32(G, "G") if gram else c_void_p(None)), "fumi_hip_xpanel_fwd_rows")
    return A0, G


def xpanel_bwd(ws, x_s, x_q, Abar, scale=1.0, out=None):
    """gW0 [h0, D].  ``x_s`` or ``x_q`` (not both) may be None: a one-sided panel over the rows of the other (Abar [B, rows, h0]).
    ``out``: the tensor to write instead of a fresh one."""
    if x_s is None and x_q is None:
        raise FumiHipError("xpanel_bwd: x_s and x_q are both None")
    dev = _dev(x_s if x_s is not None else x_q)
    B, D = (x_s if x_s is not None else x_q).shape[0::2]
    S = x_s.shape[1] if x_s is not None else 0
    Qn = x_q.shape[1] if x_q is not None else 0
    h0 = Abar.shape[2]
    gW0 = _out(out, (h0, D), dev, "gW0")
    ps = _f32(x_s, "x_s") if x_s is not None else c_void_p(None)
    pq = _f32(x_q, "x_q") if x_q is not None else c_void_p(None)
    _check(lib().fumi_hip_xpanel_bwd(ws.handle, _stream(dev), B, S, Qn, D, h0, ps, pq,
                                     _f32(Abar, "Abar"), float(scale), _f32(gW0, "gW0")), "fumi_hip_xpanel_bwd")
    return gW0


def reduce_segments(ws, segs, scale=1.0):
    """The plain multi-segment slab reduction of a step's last launch, on its own (fumi_hip_reduce_segments).  ``segs``: up to 24
    tuples (src, nslab, stride, count, dst) of flat float32 tensors: dst[i] = scale * (even slabs' sum + odd slabs' sum) of
    src[t * stride + i], i < count.  A source or destination that starts off a 16-byte boundary (a view ``x[1:]``) takes the
    one-float-per-thread path.  Writes ``dst`` in place."""
    n = len(segs)
    if n > 24:
        raise FumiHipError(f"reduce_segments: {n} segments, at most 24")
    if n == 0:
        return
    dev = _dev(segs[0][0])
    src, dst = (c_void_p * n)(), (c_void_p * n)()
    ns, st, cnt = (c_int * n)(), (ctypes.c_long * n)(), (ctypes.c_long * n)()
    for k, (s, nslab, stride, count, d) in enumerate(segs):
        src[k], dst[k] = _f32(s, "src").value, _f32(d, "dst").value
        if nslab < 1 or count < 0 or stride < 0 or (nslab - 1) * stride + count > s.numel() or count > d.numel():
            raise FumiHipError(f"reduce_segments: segment {k} reads or writes past its tensors")
        ns[k], st[k], cnt[k] = nslab, stride, count
    _check(lib().fumi_hip_reduce_segments(ws.handle, _stream(dev), n, src, ns, st, cnt, dst,
                                          float(scale)), "fumi_hip_reduce_segments")


XPANEL_PLAN_KEYS = ("fwd_kernel", "fwd_ring", "fwd_ksplit", "fwd_gram_blocks", "fwd_rode",
                    "bwd_kernel", "bwd_nb", "bwd_sk", "bwd_nsplit", "bwd_kchunk", "bwd_rode", "fwd_gram_split")
XPANEL_FWD_KERNELS = {1: "generic", 2: "generic_fast", 3: "fp32", 4: "split", 5: "presplit"}
XPANEL_GRAM_SPLIT = {0: "none", 1: "planes", 2: "tile"}      # where the pre-split forward splits the support rows of its Gram tiles
XPANEL_BWD_KERNELS = {1: "guarded64", 2: "fast64", 3: "wide_fp32", 4: "wide_split", 5: "narrow_split"}


def xpanel_plan():
    """dict over XPANEL_PLAN_KEYS: the kernel form the last forward and the last backward X-panel launch of this process took
    (fumi_hip_xpanel_plan; the kernel ids are named by XPANEL_FWD_KERNELS / XPANEL_BWD_KERNELS)."""
    v = (c_int * len(XPANEL_PLAN_KEYS))()
    _check(lib().fumi_hip_xpanel_plan(v, len(XPANEL_PLAN_KEYS)), "fumi_hip_xpanel_plan")
    return {k: int(x) for k, x in zip(XPANEL_PLAN_KEYS, v)}


def xpanel_planes_bytes():
    """Bytes of bf16 operand planes the last forward X-panel launch of this process wrote and read (fumi_hip_xpanel_planes_bytes):
    3 * h0 * D * 2 for W0, plus the padded support rows of every episode under FUMI_XP_GSPLIT=0."""
    return int(lib().fumi_hip_xpanel_planes_bytes())


class AdamArgs:
    """Cached pointer tables of one fused Adam call (rebuilt only when a tensor is reallocated).  Any number of tensors: the
    unclipped entry points take up to 32, the clipped ones up to 256 (``MAX_CLIPPED_TENSORS``)."""

    def __init__(self, params, grads, exp_avg, exp_avg_sq):
        self.key = tuple(t.data_ptr() for t in params + grads + exp_avg + exp_avg_sq)
        self.n = len(params)
        self.p, self.g = _parr(params, "params"), _parr(grads, "grads")
        self.m, self.v = _parr(exp_avg, "exp_avg"), _parr(exp_avg_sq, "exp_avg_sq")
        self.numel = (ctypes.c_long * self.n)(*[t.numel() for t in params])


def adam_step(ws, args, lr, beta1, beta2, eps, weight_decay, step, device):
    rc = lib().fumi_hip_adam_step(ws.handle, _stream(device), args.n, args.p, args.g, args.m, args.v, args.numel,
                                  float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step))
    _check(rc, "fumi_hip_adam_step")


def adam_step_deferred(ws, args, lr, beta1, beta2, eps, weight_decay, step):
    """The same update, folded into the last launch of the next training meta-step of ``ws`` (fumi_hip_adam_step_deferred)."""
    rc = lib().fumi_hip_adam_step_deferred(ws.handle, args.n, args.p, args.g, args.m, args.v, args.numel,
                                           float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step))
    _check(rc, "fumi_hip_adam_step_deferred")


def adam_flush(ws, device):
    """Launches a deferred optimizer step (any rule) no meta-step has folded; True when it had to."""
    launched = c_int(0)
    _check(lib().fumi_hip_adam_flush(ws.handle, _stream(device), ctypes.byref(launched)), "fumi_hip_adam_flush")
    return bool(launched.value)


def adamw_step(ws, args, lr, beta1, beta2, eps, weight_decay, step, device):
    """torch.optim.AdamW's update (decoupled weight decay) on the same fused launch; ``args``: an ``AdamArgs``."""
    rc = lib().fumi_hip_adamw_step(ws.handle, _stream(device), args.n, args.p, args.g, args.m, args.v, args.numel,
                                   float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step))
    _check(rc, "fumi_hip_adamw_step")


def adamw_step_deferred(ws, args, lr, beta1, beta2, eps, weight_decay, step):
    rc = lib().fumi_hip_adamw_step_deferred(ws.handle, args.n, args.p, args.g, args.m, args.v, args.numel,
                                            float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step))
    _check(rc, "fumi_hip_adamw_step_deferred")


class SgdArgs:
    """Cached pointer tables of one fused SGD call; ``bufs``: the momentum buffers, or None when momentum == 0."""

    def __init__(self, params, grads, bufs):
        self.n = len(params)
        self.p, self.g = _parr(params, "params"), _parr(grads, "grads")
        self.buf = _parr(bufs, "momentum_buffer") if bufs is not None else None
        self.numel = (ctypes.c_long * self.n)(*[t.numel() for t in params])


def sgd_step(ws, args, lr, momentum, weight_decay, first, device):
    """torch.optim.SGD's update (dampening 0, no Nesterov) as one fused launch; ``first``: this step creates the momentum buffers."""
    if (args.buf is None) != (momentum == 0):
        raise FumiHipError("sgd_step: momentum buffers are needed exactly when momentum != 0")
    rc = lib().fumi_hip_sgd_step(ws.handle, _stream(device), args.n, args.p, args.g, args.buf, args.numel,
                                 float(lr), float(momentum), float(weight_decay), int(bool(first)))
    _check(rc, "fumi_hip_sgd_step")


def sgd_step_deferred(ws, args, lr, momentum, weight_decay, first):
    if (args.buf is None) != (momentum == 0):
        raise FumiHipError("sgd_step_deferred: momentum buffers are needed exactly when momentum != 0")
    rc = lib().fumi_hip_sgd_step_deferred(ws.handle, args.n, args.p, args.g, args.buf, args.numel,
                                          float(lr), float(momentum), float(weight_decay), int(bool(first)))
    _check(rc, "fumi_hip_sgd_step_deferred")


MAX_CLIPPED_TENSORS = 256        # csrc/adam.hip: CLIP_MAX_TENSORS


def grad_norm(ws, grads, out=None):
    """Global L2 norm of the fp32 GPU tensors ``grads`` (up to 256) as a one-element device tensor; nothing is read back
    (fumi_hip_grad_norm)."""
    grads = list(grads)
    dev = _dev(grads[0])
    if out is None:
        out = torch.empty(1, device=dev, dtype=torch.float32)
    numel = (ctypes.c_long * len(grads))(*[t.numel() for t in grads])
    rc = lib().fumi_hip_grad_norm(ws.handle, _stream(dev), len(grads), _parr(grads, "grads"), numel, _f32(out, "out"))
    _check(rc, "fumi_hip_grad_norm")
    return out


def _clip_out(t):
    if t.numel() != 2:
        raise FumiHipError("clip_out: expected two floats (norm, coef)")
    return _f32(t, "clip_out")


def adam_step_clipped(ws, args, lr, beta1, beta2, eps, weight_decay, step, max_norm, clip_out, device):
    """clip_grad_norm_(max_norm) and ``adam_step`` without leaving the device; ``clip_out`` receives (norm, coef), the gradients
    are left as they are.  ``args``: an ``AdamArgs`` of up to 256 tensors."""
    rc = lib().fumi_hip_adam_step_clipped(ws.handle, _stream(device), args.n, args.p, args.g, args.m, args.v, args.numel,
                                          float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                                          float(max_norm), _clip_out(clip_out))
    _check(rc, "fumi_hip_adam_step_clipped")


def adamw_step_clipped(ws, args, lr, beta1, beta2, eps, weight_decay, step, max_norm, clip_out, device):
    rc = lib().fumi_hip_adamw_step_clipped(ws.handle, _stream(device), args.n, args.p, args.g, args.m, args.v, args.numel,
                                           float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step),
                                           float(max_norm), _clip_out(clip_out))
    _check(rc, "fumi_hip_adamw_step_clipped")


def sgd_step_clipped(ws, args, lr, momentum, weight_decay, first, max_norm, clip_out, device):
    if (args.buf is None) != (momentum == 0):
        raise FumiHipError("sgd_step_clipped: momentum buffers are needed exactly when momentum != 0")
    rc = lib().fumi_hip_sgd_step_clipped(ws.handle, _stream(device), args.n, args.p, args.g, args.buf, args.numel,
                                         float(lr), float(momentum), float(weight_decay), int(bool(first)),
                                         float(max_norm), _clip_out(clip_out))
    _check(rc, "fumi_hip_sgd_step_clipped")


def linear_fwd(ws, x, W, b=None, act=0):
    dev = _dev(x)
    M, K = x.shape
    N = W.shape[0]
    y = torch.empty(M, N, device=dev, dtype=torch.float32)
    rc = lib().fumi_hip_linear_fwd(ws.handle, _stream(dev), M, N, K, _f32(x, "x"), _f32(W, "W"),
                                   _f32(b, "b") if b is not None else None, int(act), _f32(y, "y"))
    _check(rc, "fumi_hip_linear_fwd")
    return y


def linear_bwd_data(ws, dy, W):
    dev = _dev(dy)
    M, N = dy.shape
    K = W.shape[1]
    dx = torch.empty(M, K, device=dev, dtype=torch.float32)
    _check(lib().fumi_hip_linear_bwd_data(ws.handle, _stream(dev), M, N, K, _f32(dy, "dy"), _f32(W, "W"), _f32(dx, "dx")),
           "fumi_hip_linear_bwd_data")
    return dx


def linear_bwd_weight(ws, dy, x):
    dev = _dev(dy)
    M, N = dy.shape
    K = x.shape[1]
    dW = torch.empty(N, K, device=dev, dtype=torch.float32)
    db = torch.empty(N, device=dev, dtype=torch.float32)
    _check(lib().fumi_hip_linear_bwd_weight(ws.handle, _stream(dev), M, N, K, _f32(dy, "dy"), _f32(x, "x"),
                                            _f32(dW, "dW"), _f32(db, "db")), "fumi_hip_linear_bwd_weight")
    return dW, db


def sample_episodes(ws, seed, step, B, N, K, Q, class_ptr, class_items):
    """Episode indices on the device (csrc/sampler.hip): classes [B,N], items_s [B,N,K], items_q [B,N,Q] (int64)."""
    dev = _dev(class_ptr)
    C = int(class_ptr.numel()) - 1
    cls = torch.empty(B, N, device=dev, dtype=torch.int64)
    it_s = torch.empty(B, N, K, device=dev, dtype=torch.int64)
    it_q = torch.empty(B, N, Q, device=dev, dtype=torch.int64)
    _check(lib().fumi_hip_sample_episodes(ws.handle, _stream(dev), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF,
                                          B, N, K, Q, C, _i64(class_ptr, "class_ptr"), _i64(class_items, "class_items"),
                                          _i64(cls, "classes"), _i64(it_s, "items_s"), _i64(it_q, "items_q")),
           "fumi_hip_sample_episodes")
    return cls, it_s, it_q


def sample_episodes_tm(ws, seed, step, B, N, K, Q, class_ptr, class_items, fixed_split=True):
    """Episode indices with torchmeta's task semantics: classes [B,N], labels [B,N] (a permutation of 0..N-1 per task), items_s
    [B,N,K], items_q [B,N,Q]; fixed_split: a class tuple always yields the same support / query members."""
    dev = _dev(class_ptr)
    C = int(class_ptr.numel()) - 1
    cls = torch.empty(B, N, device=dev, dtype=torch.int64)
    lab = torch.empty(B, N, device=dev, dtype=torch.int64)
    it_s = torch.empty(B, N, K, device=dev, dtype=torch.int64)
    it_q = torch.empty(B, N, Q, device=dev, dtype=torch.int64)
    _check(lib().fumi_hip_sample_episodes_tm(ws.handle, _stream(dev), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF,
                                             B, N, K, Q, C, _i64(class_ptr, "class_ptr"), _i64(class_items, "class_items"),
                                             int(bool(fixed_split)), _i64(cls, "classes"), _i64(lab, "labels"), _i64(it_s, "items_s"),
                                             _i64(it_q, "items_q")), "fumi_hip_sample_episodes_tm")
    return cls, lab, it_s, it_q


def gather_rows(ws, table, idx):
    """out[i, :] = table[idx[i], :] for a 2-d fp32 / int64 / int32 table on the device (byte copy of whole rows)."""
    dev = _dev(table)
    if table.dim() != 2 or not table.is_contiguous() or table.device != idx.device or idx.dtype != torch.int64:
        raise FumiHipError("gather_rows: table must be a contiguous 2-d device tensor and idx an int64 tensor on the same device")
    row_bytes = table.shape[1] * table.element_size()
    if row_bytes % 4:
        raise FumiHipError("gather_rows: row size must be a multiple of 4 bytes")
    idx = idx.contiguous()
    out = torch.empty(idx.numel(), table.shape[1], device=dev, dtype=table.dtype)
    _check(lib().fumi_hip_gather_rows(ws.handle, _stream(dev), ctypes.c_void_p(table.data_ptr()), table.shape[0], row_bytes,
                                      _i64(idx, "idx"), idx.numel(), ctypes.c_void_p(out.data_ptr())), "fumi_hip_gather_rows")
    return out


def gather_images(ws, table, idx, mean, std, *, seed=0, step=0, stream_id=0, pad=0, flip=False, jitter=(0, 0, 0)):
    """out[i] = normalise(jitter(flip(crop(table[idx[i]])))) (csrc/imgather.hip): ``table`` uint8 [n_images, C, H, W] on the device,
    ``idx`` int64 (any shape, read flat), ``mean`` / ``std`` C floats of the [0, 1] pixel scale -> float32 [n_idx, C, H, W].
    ``pad`` > 0: random crop out of the zero-padded image; ``flip``: random horizontal flip; ``jitter``: one amplitude or
    (brightness, contrast, saturation) in [0, 1] (C == 3).  The draws are a function of (seed, step, stream_id, position in idx)."""
    dev = _dev(table)
    if (table.dim() != 4 or table.dtype != torch.uint8 or not table.is_contiguous() or not isinstance(idx, torch.Tensor)
            or table.device != idx.device or idx.dtype != torch.int64):
        raise FumiHipError("gather_images: table must be a contiguous uint8 [n_images, C, H, W] device tensor and idx an int64 "
                           f"tensor on the same device; got {table.dtype} {tuple(table.shape)}")
    n_images, C, H, W = (int(s) for s in table.shape)
    if n_images < 1:
        raise FumiHipError("gather_images: the table is empty")
    jit = (jitter,) * 3 if isinstance(jitter, (int, float)) else tuple(jitter)
    mean, std = [float(m) for m in mean], [float(s) for s in std]
    if len(mean) != C or len(std) != C or len(jit) != 3:
        raise FumiHipError(f"gather_images: mean and std need {C} entries each and jitter three")
    import numpy as np
    inv = np.float32(1.0) / np.asarray(std, dtype=np.float32)               # the kernel multiplies: 1 / std rounded once, in fp32
    idx = idx.contiguous()
    out = torch.empty(idx.numel(), C, H, W, device=dev, dtype=torch.float32)
    if idx.numel() == 0:
        return out
    _check(lib().fumi_hip_gather_images(ws.handle, _stream(dev), c_void_p(table.data_ptr()), n_images, C, H, W, _i64(idx, "idx"),
                                        idx.numel(), (c_float * C)(*mean), (c_float * C)(*[float(v) for v in inv]),
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, int(stream_id), int(pad),
                                        int(bool(flip)), float(jit[0]), float(jit[1]), float(jit[2]), _f32(out, "out")),
           "fumi_hip_gather_images")
    return out


RESIZE_FIXED, RESIZE_RANDOM = 0, 1


def gather_images_resized(ws, table, idx, mean, std, out_size, *, seed=0, step=0, stream_id=0, rect=None, scale=None, ratio=1.0,
                          flip=False, jitter=(0, 0, 0)):
    """out[i] = normalise(jitter(flip(resample(rect_i of table[idx[i]])))) (csrc/imresize.hip): ``table`` uint8 [n_images, C, Hs, Ws]
    on the device, ``out_size`` = (Ho, Wo) -> float32 [n_idx, C, Ho, Wo].  Exactly one of ``rect`` = (x0, y0, w, h), the source
    rectangle of every image (resize + centre crop), and ``scale`` = (lo, hi) with ``ratio`` = rmax >= 1, a random-resized crop per
    image (area fraction in [lo, hi], aspect ratio in [1 / rmax, rmax]).  The rectangle is resampled with a separable triangle
    filter (antialiased bilinear).  ``idx``, ``mean`` / ``std``, ``flip``, ``jitter`` and the draws as in ``gather_images``."""
    dev = _dev(table)
    if (table.dim() != 4 or table.dtype != torch.uint8 or not table.is_contiguous() or not isinstance(idx, torch.Tensor)
            or table.device != idx.device or idx.dtype != torch.int64):
        raise FumiHipError("gather_images_resized: table must be a contiguous uint8 [n_images, C, Hs, Ws] device tensor and idx an "
                           f"int64 tensor on the same device; got {table.dtype} {tuple(table.shape)}")
    n_images, C, Hs, Ws = (int(s) for s in table.shape)
    if n_images < 1:
        raise FumiHipError("gather_images_resized: the table is empty")
    if (rect is None) == (scale is None):
        raise FumiHipError("gather_images_resized: give either rect=(x0, y0, w, h) or scale=(lo, hi)")
    Ho, Wo = (int(s) for s in out_size)
    if Ho < 1 or Wo < 1:
        raise FumiHipError(f"gather_images_resized: out_size must be positive, got {(Ho, Wo)}")
    jit = (jitter,) * 3 if isinstance(jitter, (int, float)) else tuple(jitter)
    mean, std = [float(m) for m in mean], [float(s) for s in std]
    if len(mean) != C or len(std) != C or len(jit) != 3:
        raise FumiHipError(f"gather_images_resized: mean and std need {C} entries each and jitter three")
    import numpy as np
    inv = np.float32(1.0) / np.asarray(std, dtype=np.float32)               # the kernel multiplies: 1 / std rounded once, in fp32
    idx = idx.contiguous()
    out = torch.empty(idx.numel(), C, Ho, Wo, device=dev, dtype=torch.float32)
    x0, y0, w, h = (int(v) for v in rect) if rect is not None else (0, 0, Ws, Hs)
    lo, hi = (float(v) for v in scale) if scale is not None else (1.0, 1.0)
    if idx.numel() == 0:
        return out
    _check(lib().fumi_hip_gather_images_resized(ws.handle, _stream(dev), c_void_p(table.data_ptr()), n_images, C, Hs, Ws, Ho, Wo,
                                                _i64(idx, "idx"), idx.numel(), (c_float * C)(*mean),
                                                (c_float * C)(*[float(v) for v in inv]), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                int(step) & 0xFFFFFFFFFFFFFFFF, int(stream_id),
                                                RESIZE_FIXED if rect is not None else RESIZE_RANDOM, x0, y0, w, h, lo, hi, float(ratio),
                                                int(bool(flip)), float(jit[0]), float(jit[1]), float(jit[2]), _f32(out, "out")),
           "fumi_hip_gather_images_resized")
    return out


def publish_scalars(ws, src, n, host_pinned, seq, defer=False):
    """One tiny launch on the current stream writes src[:n] and then the 64-bit word ``seq`` (byte offset 56) into the pinned
    host tensor ``host_pinned`` (>= 64 bytes) with system-scope stores: the host polls the word, no copy, no event.
    ``defer``: the stores ride on the next optimizer launch (``adam_step`` / ``adamw_step`` / ``sgd_step``) of the workspace instead (``publish_flush`` issues them if
    none comes)."""
    dev = _dev(src)
    if src.dtype != torch.float32 or not src.is_contiguous() or not host_pinned.is_pinned() or host_pinned.numel() * host_pinned.element_size() < 64:
        raise FumiHipError("publish_scalars: src must be contiguous fp32 on the device, host_pinned a pinned tensor of >= 64 bytes")
    if defer:
        _check(lib().fumi_hip_publish_scalars_deferred(ws.handle, ctypes.c_void_p(src.data_ptr()), int(n),
                                                       ctypes.c_void_p(host_pinned.data_ptr()), int(seq)),
               "fumi_hip_publish_scalars_deferred")
        return
    _check(lib().fumi_hip_publish_scalars(ws.handle, _stream(dev), ctypes.c_void_p(src.data_ptr()), int(n),
                                          ctypes.c_void_p(host_pinned.data_ptr()), int(seq)), "fumi_hip_publish_scalars")


def publish_flush(ws, device):
    _check(lib().fumi_hip_publish_flush(ws.handle, _stream(device)), "fumi_hip_publish_flush")



# ---- Conv4 image encoder at the im_net seam (include/fumi_hip.h; csrc/conv4.hip) -------------------------------------------
def conv4_feature_dim(nblk, H, W):
    return int(lib().fumi_hip_conv4_feature_dim(int(nblk), int(H), int(W)))


CONV4_MAX_TAPED_STEPS = 32


def _conv4_tape_limit(T, need_grad, second_order):
    """A second-order Conv4 step keeps the tape of every inner step resident: at most 32 (csrc/conv4.hip CV_MAXTAPE); evaluation
    (no gradient) and first-order steps reuse one tape and take any T (the reference's test default is 100 steps)."""
    if need_grad and second_order and int(T) > CONV4_MAX_TAPED_STEPS:
        raise FumiHipError(f"conv4: {T} taped inner steps requested, at most {CONV4_MAX_TAPED_STEPS} are supported for a second-order "
                           f"meta-gradient (first-order steps and evaluation take any number)")


def _ci(v):
    return (c_int * len(v))(*[int(x) for x in v])


def _image_dims(name, per_block, layout, x_s, y_s, x_q, y_q, theta):
    if x_s.dim() != 5 or x_q.dim() != 5:
        raise FumiHipError(f"{name}: images must be [B, rows, Cin, H, W]")
    B, S, Cin, H, W = x_s.shape
    Qn = x_q.shape[1]
    if len(theta) % per_block or not theta:
        raise FumiHipError(f"{name}: theta must hold {layout} per block")
    _shape(x_q, (B, Qn, Cin, H, W), "x_q")
    if y_s is not None or y_q is not None:         # (the encoder pair and the feature call have no labels)
        _shape(y_s, (B, S), "y_s"); _shape(y_q, (B, Qn), "y_q")
    return B, S, Qn, Cin, H, W, len(theta) // per_block


def _conv4_shapes(x_s, y_s, x_q, y_q, theta):
    dims = _image_dims("conv4", 3, "(conv weight, BN weight, BN bias)", x_s, y_s, x_q, y_q, theta)
    Cin, H, W, nblk = dims[3:]
    for l in range(nblk):
        _shape(theta[3 * l], (64, Cin if l == 0 else 64, 3, 3), f"theta[{3 * l}] (conv weight of block {l})")
        _shape(theta[3 * l + 1], (64,), f"theta[{3 * l + 1}]"); _shape(theta[3 * l + 2], (64,), f"theta[{3 * l + 2}]")
    F = conv4_feature_dim(nblk, H, W)
    if F < 64:
        raise FumiHipError(f"conv4: {H}x{W} images are too small for {nblk} blocks")
    return dims, F, ()


def _resnet12_shapes(x_s, y_s, x_q, y_q, theta):
    dims = _image_dims("resnet12", 12, "12 tensors (W1,g1,b1, W2,g2,b2, W3,g3,b3, Ws,gs,bs)", x_s, y_s, x_q, y_q, theta)
    Cin, H, W, nblk = dims[3:]
    channels, ci = [], Cin
    for l in range(nblk):
        c = int(theta[12 * l].shape[0])
        if c % 32:
            raise FumiHipError("resnet12: channel counts must be multiples of 32")
        for k, (cin, ks) in enumerate(((ci, 3), (c, 3), (c, 3), (ci, 1))):
            _shape(theta[12 * l + 3 * k], (c, cin, ks, ks), f"theta[{12 * l + 3 * k}]")
            _shape(theta[12 * l + 3 * k + 1], (c,), f"theta[{12 * l + 3 * k + 1}]")
            _shape(theta[12 * l + 3 * k + 2], (c,), f"theta[{12 * l + 3 * k + 2}]")
        channels.append(c); ci = c
    if min(H, W) >> nblk < 1:
        raise FumiHipError(f"resnet12: {H}x{W} images are too small for {nblk} blocks")
    return dims, channels[-1], (_ci(channels),)


# What differs between the two encoders' wrappers.  shapes(x_s, y_s, x_q, y_q, theta) checks every shape (the kernels index raw
# pointers with the sizes they are told) and returns ((B, S, Qn, Cin, H, W, nblk), feature width F, the integer arguments the entry
# points take after nblk).  Symbols: fumi_hip_{fumi,maml}_<name>_step, fumi_hip_<name>_{encode,encode_bwd,features}.
_Encoder = collections.namedtuple("_Encoder", "name per_block shapes")
_CONV4 = _Encoder("conv4", 3, _conv4_shapes)
_RESNET12 = _Encoder("resnet12", 12, _resnet12_shapes)


def _inner_args(B, T, alpha, flag, need_grad, grad_scale, tail):
    """T, alpha, tanh_head | first_order, need_grad, grad_scale [, chunk] as the step entry points take them."""
    return (int(T), float(alpha), int(bool(flag)), int(bool(need_grad)), float(1.0 / B if grad_scale is None else grad_scale), *tail)


def _enc_step(enc, kind, ws, N, x_s, y_s, x_q, y_q, dims, scalars, inputs, stats, grads):
    """The call both step kinds share: image dims, the scalars after nblk, the episodes, inputs, the five outputs + stats, gradients."""
    dev, (B, S, Qn) = _dev(x_s), dims[:3]
    outs = _step_outputs(dev, B, Qn, N)
    sym = f"fumi_hip_{kind}_{enc.name}_step"
    rc = getattr(lib(), sym)(
        ws.handle, _stream(dev), B, N, *dims[1:], *scalars,
        _f32(x_s, "x_s"), _i64(y_s, "y_s"), _f32(x_q, "x_q"), _i64(y_q, "y_q"), *inputs,
        _f32(outs[0], "logits"), _i64(outs[1], "preds"), _f32(outs[2], "preds_f"), _f32(outs[3], "loss_b"), _f32(outs[4], "acc_b"),
        _f32(stats, "stats") if stats is not None else None, *grads)
    _check(rc, sym)
    return dict(logits=outs[0], preds=outs[1], preds_f=outs[2], loss_b=outs[3], acc_b=outs[4], stats=stats)


def _enc_fumi_step(enc, ws, n_way, x_s, y_s, x_q, y_q, theta, phi, T, alpha, tanh_head, cls_text, text_s, need_grad, grad_scale,
                   g_theta, g_phi, stats, g_cls_text, tail=()):
    dims, F, extra = enc.shapes(x_s, y_s, x_q, y_q, theta)
    B, S, N = dims[0], dims[1], int(n_way)
    Ht, Dt = int(phi[0].shape[0]), int(phi[0].shape[1])
    _shape(phi[1], (Ht,), "phi[1]"); _shape(phi[2], (F + 1, Ht), "phi[2]"); _shape(phi[3], (F + 1,), "phi[3]")
    if cls_text is not None:
        _shape(cls_text, (B, N, Dt), "cls_text")
    else:
        _shape(text_s, (B, S, Dt), "text_s")
    g_ct = _text_grad(g_cls_text, _dev(x_s), B, N, Dt, "g_cls_text")
    if need_grad:
        g_theta = [torch.empty_like(t) for t in theta] if g_theta is None else g_theta
        g_phi = [torch.empty_like(t) for t in phi] if g_phi is None else g_phi
    out = _enc_step(enc, "fumi", ws, N, x_s, y_s, x_q, y_q, dims,
                    (*extra, Dt, Ht, *_inner_args(B, T, alpha, tanh_head, need_grad, grad_scale, tail)),
                    (_f32(cls_text, "cls_text") if cls_text is not None else None,
                     _f32(text_s, "text_s") if text_s is not None else None, _parr(theta, "theta"), _parr(phi, "phi")), stats,
                    (_parr(g_theta, "g_theta") if need_grad else None, _parr(g_phi, "g_phi") if need_grad else None, g_ct))
    out.update(g_theta=g_theta, g_phi=g_phi)
    return out


def _enc_maml_step(enc, ws, x_s, y_s, x_q, y_q, params, T, alpha, first_order, need_grad, grad_scale, g_params, stats, tail=()):
    dims, F, extra = enc.shapes(x_s, y_s, x_q, y_q, params[:-2])
    N = int(params[-2].shape[0])
    _shape(params[-2], (N, F), "lin_final.weight"); _shape(params[-1], (N,), "lin_final.bias")
    if need_grad and g_params is None:
        g_params = [torch.empty_like(t) for t in params]
    out = _enc_step(enc, "maml", ws, N, x_s, y_s, x_q, y_q, dims,
                    (*extra, *_inner_args(dims[0], T, alpha, first_order, need_grad, grad_scale, tail)),
                    (_parr(params, "params"),), stats, (_parr(g_params, "g_params") if need_grad else None,))
    out.update(g_params=g_params)
    return out


def _enc_features(enc, ws, x, theta):
    dev = _dev(x)
    dims, F, extra = enc.shapes(x, None, x, None, theta)
    G, M = dims[:2]
    feats = torch.empty(G, M, F, device=dev, dtype=torch.float32)
    sym = f"fumi_hip_{enc.name}_features"
    _check(getattr(lib(), sym)(ws.handle, _stream(dev), G, M, *dims[3:], *extra, _f32(x, "x"), _parr(theta, "theta"),
                               _f32(feats, "feats")), sym)
    return feats


def _drop_args(nblk, drop_rate, drop_block, drop_seed):
    """(rate [nblk] fp32, block [nblk] int, seed uint64) as the ``_drop`` entry points take them (host values)."""
    if len(drop_rate) != nblk or len(drop_block) != nblk:
        raise FumiHipError("drop_rate / drop_block must hold one value per block")
    return ((c_float * nblk)(*[float(r) for r in drop_rate]), _ci(drop_block), ctypes.c_uint64(int(drop_seed) & 0xFFFFFFFFFFFFFFFF))


def _enc_encode(enc, ws, x_s, x_q, theta, keep_tape, drop=None):
    dev = _dev(x_s)
    dims, F, extra = enc.shapes(x_s, None, x_q, None, theta)
    B, S, Qn = dims[:3]
    fs = torch.empty(B, S, F, device=dev, dtype=torch.float32)
    fq = torch.empty(B, Qn, F, device=dev, dtype=torch.float32)
    sym = f"fumi_hip_{enc.name}_encode" + ("_drop" if drop is not None else "")
    tail = _drop_args(dims[-1], *drop) if drop is not None else ()
    _check(getattr(lib(), sym)(ws.handle, _stream(dev), *dims, *extra, _f32(x_s, "x_s"), _f32(x_q, "x_q"), _parr(theta, "theta"),
                               _f32(fs, "feats_s"), _f32(fq, "feats_q"), int(bool(keep_tape)), *tail), sym)
    return fs, fq


def _enc_encode_bwd(enc, ws, x_s, x_q, dfeats_s, dfeats_q, theta_like, scale, g_theta, drop=None):
    dev = _dev(x_s)
    dims, F, extra = enc.shapes(x_s, None, x_q, None, theta_like)
    B, S, Qn = dims[:3]
    _shape(dfeats_s, (B, S, F), "dfeats_s"); _shape(dfeats_q, (B, Qn, F), "dfeats_q")
    if g_theta is None:
        g_theta = [torch.empty_like(t) for t in theta_like]
    elif len(g_theta) != len(theta_like):
        raise FumiHipError(f"{enc.name}_encode_bwd: g_theta must hold one tensor per theta tensor")
    else:
        for i, (g, t) in enumerate(zip(g_theta, theta_like)):
            _shape(g, tuple(t.shape), f"g_theta[{i}]")
    sym = f"fumi_hip_{enc.name}_encode_bwd" + ("_drop" if drop is not None else "")
    tail = _drop_args(dims[-1], *drop) if drop is not None else ()
    _check(getattr(lib(), sym)(ws.handle, _stream(dev), *dims, *extra, _f32(x_s, "x_s"), _f32(x_q, "x_q"), _f32(dfeats_s, "dfeats_s"),
                               _f32(dfeats_q, "dfeats_q"), float(scale), _parr(g_theta, "g_theta"), *tail), sym)
    return g_theta


def fumi_conv4_step(ws, n_way, x_s, y_s, x_q, y_q, theta, phi, T, alpha, tanh_head, *, cls_text=None, text_s=None,
                    need_grad=True, grad_scale=None, g_theta=None, g_phi=None, stats=None, g_cls_text=None):
    """FuMI meta-step with the Conv4 encoder (fumi/models/fumi.py:146-192 with im_net = Conv4).  ``g_cls_text`` as in ``fumi_step``."""
    _conv4_tape_limit(T, need_grad, True)
    return _enc_fumi_step(_CONV4, ws, n_way, x_s, y_s, x_q, y_q, theta, phi, T, alpha, tanh_head, cls_text, text_s, need_grad,
                          grad_scale, g_theta, g_phi, stats, g_cls_text)


def maml_conv4_step(ws, x_s, y_s, x_q, y_q, params, T, alpha, first_order=False, *, need_grad=True, grad_scale=None,
                    g_params=None, stats=None):
    """MAML meta-step with the Conv4 encoder: params = theta (3 per block) + [lin_final W [N,F], b [N]]."""
    _conv4_tape_limit(T, need_grad, not first_order)
    return _enc_maml_step(_CONV4, ws, x_s, y_s, x_q, y_q, params, T, alpha, first_order, need_grad, grad_scale, g_params, stats)


def conv4_features(ws, x, theta):
    """[G, M, F] = Conv4(x [G, M, Cin, H, W]) with the batch statistics of each group of M images (forward only)."""
    return _enc_features(_CONV4, ws, x, theta)


def conv4_encode(ws, x_s, x_q, theta, keep_tape=False):
    """(feats_s [B,S,F], feats_q [B,Qn,F]) = Conv4 of every episode's support / query images (one batch-statistics group each).
    keep_tape: the activations stay laid out in ``ws`` for ``conv4_encode_bwd`` -- no other call may use ``ws`` in between."""
    return _enc_encode(_CONV4, ws, x_s, x_q, theta, keep_tape)


def conv4_encode_bwd(ws, x_s, x_q, dfeats_s, dfeats_q, theta_like, scale=1.0, g_theta=None):
    """Gradient of sum <dfeats, Conv4(x)> w.r.t. the encoder's parameters (summed over episodes, times ``scale``) from the tape the
    last ``conv4_encode(..., keep_tape=True)`` left in ``ws``."""
    return _enc_encode_bwd(_CONV4, ws, x_s, x_q, dfeats_s, dfeats_q, theta_like, scale, g_theta)


def fumi_resnet12_step(ws, n_way, x_s, y_s, x_q, y_q, theta, phi, T, alpha, tanh_head, *, cls_text=None, text_s=None,
                       need_grad=True, grad_scale=None, g_theta=None, g_phi=None, stats=None, chunk=0, g_cls_text=None):
    """FuMI meta-step with the bf16 ResNet-12 encoder (fumi/models/fumi.py:146-192 with im_net = ResNet-12).  ``g_cls_text`` as in
    ``fumi_step``."""
    return _enc_fumi_step(_RESNET12, ws, n_way, x_s, y_s, x_q, y_q, theta, phi, T, alpha, tanh_head, cls_text, text_s, need_grad,
                          grad_scale, g_theta, g_phi, stats, g_cls_text, (int(chunk),))


def maml_resnet12_step(ws, x_s, y_s, x_q, y_q, params, T, alpha, first_order=False, *, need_grad=True, grad_scale=None,
                       g_params=None, stats=None, chunk=0):
    """MAML meta-step with the bf16 ResNet-12 encoder: params = theta (12 per block) + [lin_final W [N,F], b [N]]."""
    return _enc_maml_step(_RESNET12, ws, x_s, y_s, x_q, y_q, params, T, alpha, first_order, need_grad, grad_scale, g_params, stats,
                          (int(chunk),))


def resnet12_features(ws, x, theta):
    """feats [G, M, F] = ResNet12(x [G, M, Cin, H, W]); batch statistics per group of M images."""
    return _enc_features(_RESNET12, ws, x, theta)


def resnet12_encode(ws, x_s, x_q, theta, keep_tape=False):
    """(feats_s [B,S,F], feats_q [B,Qn,F]) = ResNet-12 of every episode's support / query images (one batch-statistics group each).
    keep_tape: what the backward needs stays in ``ws`` for ``resnet12_encode_bwd`` -- no other call may use ``ws`` in between."""
    return _enc_encode(_RESNET12, ws, x_s, x_q, theta, keep_tape)


def resnet12_encode_bwd(ws, x_s, x_q, dfeats_s, dfeats_q, theta_like, scale=1.0, g_theta=None):
    """Gradient of sum <dfeats, ResNet12(x)> w.r.t. the encoder's parameters (summed over episodes, times ``scale``) from what the
    last ``resnet12_encode(..., keep_tape=True)`` left in ``ws``."""
    return _enc_encode_bwd(_RESNET12, ws, x_s, x_q, dfeats_s, dfeats_q, theta_like, scale, g_theta)


def resnet12_encode_drop(ws, x_s, x_q, theta, drop_rate, drop_block, drop_seed, keep_tape=False):
    """``resnet12_encode`` with DropBlock / dropout on every block's pooled output: ``drop_rate`` / ``drop_block`` hold one value per
    block (block size 1: element-wise dropout, 2..8: DropBlock; rate 0: nothing at that block), ``drop_seed`` is the step's 64-bit
    seed.  The mask is regenerated from (seed, block, set, global episode, image, channel, position) wherever it is needed."""
    return _enc_encode(_RESNET12, ws, x_s, x_q, theta, keep_tape, (drop_rate, drop_block, drop_seed))


def resnet12_encode_bwd_drop(ws, x_s, x_q, dfeats_s, dfeats_q, theta_like, drop_rate, drop_block, drop_seed, scale=1.0, g_theta=None):
    """``resnet12_encode_bwd`` for a tape ``resnet12_encode_drop`` left: the three drop arguments must be the tape's (FUMI_EINVAL)."""
    return _enc_encode_bwd(_RESNET12, ws, x_s, x_q, dfeats_s, dfeats_q, theta_like, scale, g_theta, (drop_rate, drop_block, drop_seed))


def rn12_drop_apply(ws, x, H, W, rate, block, seed, block_index=0, set_index=0, b0=0):
    """Unit op: x [B, M*(H+2)*(W+2), C] bf16 padded channels-last is scaled IN PLACE by keep * total / kept; returns (kept [B] int64,
    scale [B] fp32)."""
    dev = _dev(x)
    B, npix, C = x.shape
    M = npix // ((H + 2) * (W + 2))
    kept = torch.empty(B, device=dev, dtype=torch.int64)
    scale = torch.empty(B, device=dev, dtype=torch.float32)
    _check(lib().fumi_hip_rn12_drop_apply(ws.handle, _stream(dev), B, M, H, W, C, float(rate), int(block),
                                          ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(block_index), int(set_index), int(b0),
                                          _bf16ptr(x, "x"), _i64(kept, "kept"), _f32(scale, "scale")), "fumi_hip_rn12_drop_apply")
    return kept, scale


def resnet12_set_budget(gigabytes):
    """Workspace budget (GB) from which the episode chunk of the ResNet-12 steps is derived (0: default 200)."""
    _check(lib().fumi_hip_resnet12_set_budget(float(gigabytes)), "fumi_hip_resnet12_set_budget")


def resnet12_encode_plan():
    """(taped, chunk, lanes) of the last ``resnet12_encode``: taped = True for the taped form, False for the recompute form."""
    t, c, l = c_int(0), c_int(0), c_int(0)
    _check(lib().fumi_hip_resnet12_encode_plan(ctypes.byref(t), ctypes.byref(c), ctypes.byref(l)), "fumi_hip_resnet12_encode_plan")
    return bool(t.value), int(c.value), int(l.value)


def _bf16ptr(t, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()):
        raise FumiHipError(f"{name}: expected a contiguous bfloat16 GPU tensor")
    return c_void_p(t.data_ptr())


def rn12_conv(ws, x, Wt, H, W, transpose=False, want_stats=False):
    """Unit op: x [B, M*(H+2)*(W+2), Cx] bf16 padded channels-last, Wt [B, Cout, Cin, k, k] fp32 -> y bf16 (and [B,2,Cy] stats)."""
    dev = _dev(x)
    B, npix, Cx = x.shape
    Cout, Cin, k = int(Wt.shape[1]), int(Wt.shape[2]), int(Wt.shape[3])
    M = npix // ((H + 2) * (W + 2))
    Cy = Cin if transpose else Cout
    y = torch.empty(B, npix, Cy, device=dev, dtype=torch.bfloat16)
    st = torch.empty(B, 2, Cy, device=dev, dtype=torch.float32) if want_stats else None
    _check(lib().fumi_hip_rn12_conv(ws.handle, _stream(dev), B, M, H, W, Cin, Cout, k * k, int(bool(transpose)), _bf16ptr(x, "x"),
                                    _f32(Wt, "Wt"), _bf16ptr(y, "y"), _f32(st, "stats") if st is not None else None), "fumi_hip_rn12_conv")
    return (y, st) if want_stats else y


def rn12_wgrad(ws, x, dy, H, W, k):
    dev = _dev(x)
    B, npix, Cin = x.shape
    Cout = int(dy.shape[2])
    M = npix // ((H + 2) * (W + 2))
    dW = torch.empty(B, Cout, Cin, k, k, device=dev, dtype=torch.float32)
    _check(lib().fumi_hip_rn12_wgrad(ws.handle, _stream(dev), B, M, H, W, Cin, Cout, k * k, _bf16ptr(x, "x"), _bf16ptr(dy, "dy"),
                                     _f32(dW, "dW")), "fumi_hip_rn12_wgrad")
    return dW


RN12_CONV_KEYS = ("nf", "mw", "bks", "s16", "tiles", "tpi", "ncg", "xcd", "glds", "slab_rows", "lds")
RN12_WGRAD_KEYS = ("ntap", "nsplit", "ci_tiles", "co_tiles", "xcd", "reduce")
RN12_REDUCE_KERNELS = {1: "rn_wgrad_reduce_kernel<false>", 2: "rn_wgrad_reduce_kernel<true>", 3: "rn_wgrad_reduce9_kernel"}


def rn12_conv_multi(ws, B, M, H, W, Cout, srcs, y, y_stride, transpose=False, dot=None, dot_stride=0, stats=None):
    """fumi_hip_rn12_conv_multi on raw buffers.  srcs: 1..4 of (x, x_stride, Cin, Wt, w_stride, ntaps) with x a flat bf16 tensor that
    starts at episode 0 and Wt fp32 (w_stride 0: shared); y a flat bf16 tensor (NOT cleared), stats [B, 2, Cout] fp32 or None."""
    n = len(srcs)
    dev = _dev(y)
    LL = ctypes.c_longlong
    cin = (c_int * max(n, 1))(*[int(s[2]) for s in srcs])
    taps = (c_int * max(n, 1))(*[int(s[5]) for s in srcs])
    xs = (c_void_p * max(n, 1))(*[_bf16ptr(s[0], "x").value for s in srcs])
    xst = (LL * max(n, 1))(*[int(s[1]) for s in srcs])
    wp = (c_void_p * max(n, 1))(*[_f32(s[3], "Wt").value for s in srcs])
    wst = (LL * max(n, 1))(*[int(s[4]) for s in srcs])
    _check(lib().fumi_hip_rn12_conv_multi(ws.handle, _stream(dev), B, M, H, W, Cout, n, cin, taps, xs, xst, wp, wst, int(bool(transpose)),
                                          _bf16ptr(dot, "dot") if dot is not None else None, int(dot_stride), _bf16ptr(y, "y"),
                                          int(y_stride), _f32(stats, "stats") if stats is not None else None),
           "fumi_hip_rn12_conv_multi")


def rn12_wgrad_multi(ws, B, M, H, W, Cin, Cin_real, Cout, ntaps, pairs, x_stride, dy_stride, dW, dw_stride, nsplit=0):
    """fumi_hip_rn12_wgrad_multi on raw buffers.  pairs: 1..2 of (x, dy) flat bf16 tensors that start at episode 0; dW flat fp32."""
    dev = _dev(dW)
    p = [(_bf16ptr(x, "x"), _bf16ptr(dy, "dy")) for x, dy in pairs[:2]] + [(None, None)] * (2 - min(len(pairs), 2))
    _check(lib().fumi_hip_rn12_wgrad_multi(ws.handle, _stream(dev), B, M, H, W, Cin, Cin_real, Cout, ntaps, len(pairs), int(nsplit),
                                           p[0][0], p[0][1], p[1][0], p[1][1], int(x_stride), int(dy_stride), _f32(dW, "dW"),
                                           int(dw_stride)), "fumi_hip_rn12_wgrad_multi")


def rn12_conv_plan():
    """(conv, wgrad): what the last convolution launch and the last weight-gradient launch of this process decided
    (fumi_hip_rn12_conv_plan; keys RN12_CONV_KEYS / RN12_WGRAD_KEYS)."""
    v = (c_int * 17)()
    _check(lib().fumi_hip_rn12_conv_plan(v, 17), "fumi_hip_rn12_conv_plan")
    return dict(zip(RN12_CONV_KEYS, v[:11])), dict(zip(RN12_WGRAD_KEYS, v[11:]))


def rn12_conv_query(B, M, H, W, Cout, Cins):
    """The decisions launch_rn_conv takes for a shape (under this process's knobs): host arithmetic only, no GPU."""
    v = (c_int * 11)()
    cin = (c_int * max(len(Cins), 1))(*[int(c) for c in Cins])
    _check(lib().fumi_hip_rn12_conv_query(B, M, H, W, Cout, len(Cins), cin, v, 11), "fumi_hip_rn12_conv_query")
    return dict(zip(RN12_CONV_KEYS, v[:]))


def rn12_wgrad_query(B, M, H, W, Cin, Cout, ntaps, npair=1, nsplit=0):
    """The decisions launch_rn_wgrad and launch_rn_wgrad_reduce take for a shape: host arithmetic only, no GPU."""
    v = (c_int * 6)()
    _check(lib().fumi_hip_rn12_wgrad_query(B, M, H, W, Cin, Cout, ntaps, npair, nsplit, v, 6), "fumi_hip_rn12_wgrad_query")
    return dict(zip(RN12_WGRAD_KEYS, v[:]))


RN12_EW_KINDS = ("act", "bwd_reduce", "bwd_apply", "join_fwd", "join_reduce", "join_apply", "avgpool", "avgpool_bwd", "img_prep")
RN12_EW_KEYS = ("nch", "nrg", "active", "unit", "rb", "nt", "map_rb", "wb", "ncy", "ncx", "cb", "cell", "first", "nt2", "lds", "gx", "gy")
RN12_COEF_KEYS = ("first", "nt2", "gx1", "gy1", "gx", "gy", "scratch")
RN12_COEF_MODES = {"fwd": 0, "bwd": 1, "tfwd": 2, "tbwd": 3}
RN12_COEF_FIELDS = ("mu", "r", "a", "c0", "d1", "d2", "tb", "tc", "m1", "m2", "k0", "dd1", "e12")


def rn12_ew_query(B, M, H, W, C, kind, tangent=False, form=0):
    """The decisions an element-wise launcher of csrc/rn12_ew.hip takes for a shape: host arithmetic only, no GPU.  kind: a name of
    RN12_EW_KINDS (avgpool / avgpool_bwd / img_prep: B * M images; img_prep: C is the image's channel count)."""
    v = (c_int * 17)()
    _check(lib().fumi_hip_rn12_ew_query(B, M, H, W, C, RN12_EW_KINDS.index(kind), int(bool(tangent)), int(form), v, 17), "fumi_hip_rn12_ew_query")
    return dict(zip(RN12_EW_KEYS, v[:]))


def rn12_ew_plan():
    """What the last element-wise launch of this process decided (keys RN12_EW_KEYS; a coefficient launch updates first / nt2)."""
    v = (c_int * 17)()
    _check(lib().fumi_hip_rn12_ew_plan(v, 17), "fumi_hip_rn12_ew_plan")
    return dict(zip(RN12_EW_KEYS, v[:]))


def rn12_coef_query(B, nt, K, C, has_scratch=True):
    v = (c_int * 7)()
    _check(lib().fumi_hip_rn12_coef_query(B, nt, K, C, int(bool(has_scratch)), v, 7), "fumi_hip_rn12_coef_query")
    return dict(zip(RN12_COEF_KEYS, v[:]))


def _rawptr(t, name, dtype):
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise FumiHipError(f"{name}: expected a contiguous {dtype} GPU tensor")
    return c_void_p(t.data_ptr())


def rn12_ew_act(ws, B, M, H, W, C, u, ud, coef, out):
    """fumi_hip_rn12_ew_act on raw buffers (flat bf16 maps, fp32 table [B, 13, C]); ud None: the plain form."""
    bf, f4 = torch.bfloat16, torch.float32
    _check(lib().fumi_hip_rn12_ew_act(ws.handle, _stream(_dev(out)), B, M, H, W, C, _rawptr(u, "u", bf), _rawptr(ud, "ud", bf),
                                      _rawptr(coef, "coef", f4), _rawptr(out, "out", bf)), "fumi_hip_rn12_ew_act")


def rn12_ew_bwd(ws, B, M, H, W, C, apply, u, ud, da, dad, coef, out):
    """fumi_hip_rn12_ew_bwd: apply False -> out fp32 partial sums [B, nt, 2 | 3, C]; True -> out bf16 du.  ud / dad None: plain."""
    bf, f4 = torch.bfloat16, torch.float32
    _check(lib().fumi_hip_rn12_ew_bwd(ws.handle, _stream(_dev(out)), B, M, H, W, C, int(bool(apply)), int(ud is not None),
                                      _rawptr(u, "u", bf), _rawptr(ud, "ud", bf), _rawptr(da, "da", bf), _rawptr(dad, "dad", bf),
                                      _rawptr(coef, "coef", f4), _rawptr(out, "out", bf if apply else f4)), "fumi_hip_rn12_ew_bwd")


def rn12_ew_join(ws, B, M, H, W, C, pass_, u3, us, u3d, usd, coef3, coefs, dout, doutd, out0, out1=None, form=0):
    """fumi_hip_rn12_ew_join: pass_ 0 forward (out0 the pooled map), 1 reduce (out0 fp32 [B, nt, 3 | 5, C]), 2 apply (out0 du3, out1
    dus).  u3d / usd (and doutd) None: plain.  form 1: the plain apply on the cell kernel."""
    bf, f4 = torch.bfloat16, torch.float32
    _check(lib().fumi_hip_rn12_ew_join(ws.handle, _stream(_dev(out0)), B, M, H, W, C, int(pass_), int(u3d is not None), int(form),
                                       _rawptr(u3, "u3", bf), _rawptr(us, "us", bf), _rawptr(u3d, "u3d", bf), _rawptr(usd, "usd", bf),
                                       _rawptr(coef3, "coef3", f4), _rawptr(coefs, "coefs", f4), _rawptr(dout, "dout", bf),
                                       _rawptr(doutd, "doutd", bf), _rawptr(out0, "out0", f4 if pass_ == 1 else bf),
                                       _rawptr(out1, "out1", bf)), "fumi_hip_rn12_ew_join")


def rn12_ew_coef(ws, B, C, mode, nt, K, ks, n, part, coef, g=None, beta=None, pstride=0, gd=None, betad=None, dstride=0, dg=None,
                 dbeta=None, gstride=0, scratch=None):
    """fumi_hip_rn12_ew_coef: mode a name of RN12_COEF_MODES, ks = (k0, k1, k2) slices of the K partial sums, all buffers flat fp32."""
    f4 = torch.float32
    P = lambda t, name: _rawptr(t, name, f4)
    _check(lib().fumi_hip_rn12_ew_coef(ws.handle, _stream(_dev(coef)), B, C, RN12_COEF_MODES[mode], nt, K, int(ks[0]), int(ks[1]), int(ks[2]),
                                       float(n), P(part, "part"), P(coef, "coef"), P(g, "g"), P(beta, "beta"), int(pstride), P(gd, "gd"),
                                       P(betad, "betad"), int(dstride), P(dg, "dg"), P(dbeta, "dbeta"), int(gstride), P(scratch, "scratch")),
           "fumi_hip_rn12_ew_coef")


def rn12_ew_avgpool(ws, BM, H, W, C, adjoint, src, out):
    """fumi_hip_rn12_ew_avgpool: adjoint False src bf16 map -> out fp32 [BM, C]; True src fp32 [BM, C] -> out bf16 map."""
    bf, f4 = torch.bfloat16, torch.float32
    _check(lib().fumi_hip_rn12_ew_avgpool(ws.handle, _stream(_dev(out)), BM, H, W, C, int(bool(adjoint)), _rawptr(src, "in", f4 if adjoint else bf),
                                          _rawptr(out, "out", bf if adjoint else f4)), "fumi_hip_rn12_ew_avgpool")


def rn12_ew_img_prep(ws, BM, Cin, H, W, img, out):
    _check(lib().fumi_hip_rn12_ew_img_prep(ws.handle, _stream(_dev(out)), BM, Cin, H, W, _rawptr(img, "img", torch.float32),
                                           _rawptr(out, "out", torch.bfloat16)), "fumi_hip_rn12_ew_img_prep")


def resnet12_set_option(key, value):
    """fumi_hip_resnet12_set_option: key 0 = probe mode (test hook), key 1 = the reverse sweep stops after inner step `value`."""
    _check(lib().fumi_hip_resnet12_set_option(int(key), int(value)), "fumi_hip_resnet12_set_option")


def rn12_probe(ws, device, pass_, kind, block=0, idx=0):
    """Test hook: one stored intermediate of the last single-chunk ResNet-12 step run in probe mode, flat (bf16 maps as
    torch.bfloat16, everything else fp32) -- fumi_hip_rn12_probe."""
    n, bf = c_size_t(0), c_int(0)
    dummy = torch.empty(4, device=device, dtype=torch.float32)
    args = (ws.handle, _stream(device), int(pass_), int(kind), int(block), int(idx))
    _check(lib().fumi_hip_rn12_probe(*args, c_void_p(dummy.data_ptr()), 0, ctypes.byref(n), ctypes.byref(bf)), "fumi_hip_rn12_probe")
    out = torch.empty(n.value // (2 if bf.value else 4), device=device, dtype=torch.bfloat16 if bf.value else torch.float32)
    _check(lib().fumi_hip_rn12_probe(*args, c_void_p(out.data_ptr()), n.value, ctypes.byref(n), ctypes.byref(bf)), "fumi_hip_rn12_probe")
    return out


def conv4_set_option(key, value):
    """fumi_hip_conv4_set_option: key 0 = fused block 1 (default 1)."""
    _check(lib().fumi_hip_conv4_set_option(int(key), int(value)), "fumi_hip_conv4_set_option")


def conv4_probe(ws, device, pass_, kind, block=0):
    """Test hook: one intermediate tensor of the last conv4 step as a flat fp32 tensor (fumi_hip_conv4_probe)."""
    n = c_size_t(0)
    dummy = torch.empty(1, device=device, dtype=torch.float32)
    _check(lib().fumi_hip_conv4_probe(ws.handle, _stream(device), int(pass_), int(kind), int(block), _f32(dummy, "out"), 0,
                                      ctypes.byref(n)), "fumi_hip_conv4_probe")
    out = torch.empty(n.value, device=device, dtype=torch.float32)
    _check(lib().fumi_hip_conv4_probe(ws.handle, _stream(device), int(pass_), int(kind), int(block), _f32(out, "out"), n.value,
                                      ctypes.byref(n)), "fumi_hip_conv4_probe")
    return out


def _conv3x3(fn, name, ws, a, b, out_shape):
    dev = _dev(a)
    M, H, W, C = a.shape
    if C != 64:
        raise FumiHipError(f"{name}: channels-last tensors with 64 channels expected")
    out = torch.empty(out_shape, device=dev, dtype=torch.float32)
    _check(fn(ws.handle, _stream(dev), M, H, W, _f32(a, "a"), _f32(b, "b"), _f32(out, "out")), name)
    return out


def conv3x3_fwd(ws, x, Wt):
    """y [M,H,W,64] = conv3x3(x [M,H,W,64], Wt [64,64,3,3]), pad 1 (channels-last)."""
    _shape(Wt, (64, 64, 3, 3), "Wt")
    return _conv3x3(lib().fumi_hip_conv3x3_fwd, "fumi_hip_conv3x3_fwd", ws, x, Wt, x.shape)


def conv3x3_bwd_data(ws, dy, Wt):
    _shape(Wt, (64, 64, 3, 3), "Wt")
    return _conv3x3(lib().fumi_hip_conv3x3_bwd_data, "fumi_hip_conv3x3_bwd_data", ws, dy, Wt, dy.shape)


def conv3x3_bwd_weight(ws, x, dy):
    _shape(dy, x.shape, "dy")
    return _conv3x3(lib().fumi_hip_conv3x3_bwd_weight, "fumi_hip_conv3x3_bwd_weight", ws, x, dy, (64, 64, 3, 3))


def sgd_axpy(ws, p, step_size, g, out=None):
    dev = _dev(p)
    out = torch.empty_like(p) if out is None else out
    _check(lib().fumi_hip_sgd_axpy(ws.handle, _stream(dev), p.numel(), _f32(p, "p"), float(step_size), _f32(g, "g"), _f32(out, "out")),
           "fumi_hip_sgd_axpy")
    return out


def ce_fwd_bwd(ws, z, y):
    """(mean cross-entropy [1], dz [M,N], first arg-max [M]) of logits z [M,N] and labels y [M]."""
    dev = _dev(z)
    M, N = z.shape
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    dz = torch.empty_like(z)
    preds = torch.empty(M, device=dev, dtype=torch.int64)
    _check(lib().fumi_hip_ce_fwd_bwd(ws.handle, _stream(dev), M, N, _f32(z, "z"), _i64(y, "y"), _f32(loss, "loss"), _f32(dz, "dz"),
                                     _i64(preds, "preds")), "fumi_hip_ce_fwd_bwd")
    return loss, dz, preds


def proto_reduce(ws, x, y, n_way):
    """Per-class means [B,N,P] of x [B,S,P] (fumi/utils/utils.py:331-376, counts clamped to >= 1)."""
    dev = _dev(x)
    B, S, P = x.shape
    out = torch.empty(B, n_way, P, device=dev, dtype=torch.float32)
    _check(lib().fumi_hip_proto_reduce(ws.handle, _stream(dev), B, S, int(n_way), P, _f32(x, "x"), _i64(y, "y"), _f32(out, "out")),
           "fumi_hip_proto_reduce")
    return out


def cls_head_step(ws, feats, y, W, b, *, need_grad=True, grad_scale=1.0, dfeats=None, gW=None, gb=None, want_preds=True):
    """The fused classification head (csrc/clshead.hip): F.cross_entropy(feats @ W.T + b, y), mean over the M rows.  Returns a dict
    of GPU tensors: loss [1], correct [1] (count, float), preds [M] (first arg-max; None without want_preds) and, with need_grad,
    dfeats [M,F], gW [C,F], gb [C] = gradients of grad_scale * loss (written into the tensors given, else into new ones)."""
    dev, (M, F, C), out = _cls_head_io("cls_head_step", feats, W, (b, "b"), (y, "y"), None, want_preds)
    grads = _head_grads(dev, need_grad, out, dfeats=((M, F), dfeats), gW=((C, F), gW), gb=((C,), gb))
    _check(lib().fumi_hip_cls_head_step(ws.handle, _stream(dev), M, F, C, _f32(feats, "feats"), _i64(y, "y"), _f32(W, "W"), _f32(b, "b"),
                                        float(grad_scale), *_cls_head_outs(out), *grads), "fumi_hip_cls_head_step")
    return out


def _cls_head_io(name, feats, W, param, y_a, y_b, want_preds, teacher=None):
    """What the classification heads share before their call: the checks of feats [M,F] and W [C,F], of the head's second parameter
    ``param`` = (b [C] or tau [1], its name), of the labels ``y_a`` = (tensor [M], its name) and ``y_b`` (tensor [M] or None) and of
    the distillation head's ``teacher`` = (feats_t [M,F], W_t [C,F], b_t [C]), and the outputs.  Returns (dev, (M, F, C),
    dict(loss, correct, preds))."""
    dev = _dev(feats)
    if feats.dim() != 2 or W.dim() != 2:
        raise FumiHipError(f"{name}: feats [M,F] and W [C,F] expected")
    M, F = (int(v) for v in feats.shape)
    C = int(W.shape[0])
    _shape(W, (C, F), "W"); _shape(param[0], (1,) if param[1] == "tau" else (C,), param[1]); _shape(y_a[0], (M,), y_a[1])
    if teacher is not None:
        _shape(teacher[0], (M, F), "feats_t"); _shape(teacher[1], (C, F), "W_t"); _shape(teacher[2], (C,), "b_t")
    if y_b is not None:
        _shape(y_b, (M,), "y_b")
    out = dict(loss=torch.empty(1, device=dev, dtype=torch.float32), correct=torch.empty(1, device=dev, dtype=torch.float32),
               preds=torch.empty(M, device=dev, dtype=torch.int64) if want_preds else None)
    return dev, (M, F, C), out


def _cls_head_outs(out):
    """The trailing (loss, correct, preds) ctypes arguments of a classification head's entry, with their dtype checks."""
    return (_f32(out["loss"], "loss"), _f32(out["correct"], "correct"),
            _i64(out["preds"], "preds") if out["preds"] is not None else None)


def _soft_args(y_b, lam, smoothing):
    """The (y_b, lam, smoothing) ctypes arguments of the soft target; y_b None -> NULL."""
    return _i64(y_b, "y_b") if y_b is not None else None, float(lam), float(smoothing)


def _episode_head_io(name, feats_s, y_s, feats_q, y_q, n_way, want_logits, param=None, metric=None):
    """What the episode heads share before their call: the checks of feats_s [B,S,F], y_s [B,S], feats_q [B,Qn,F], y_q [B,Qn], the
    ``n_way`` default and the outputs.  ``param`` = (tensor, shape, name) is the head's device parameter, checked with the shapes;
    ``metric`` the transductive head's, checked after the dimensions.  Returns (dev, (B, S, Qn, N, F), dict(loss, correct, preds,
    logits))."""
    dev = _dev(feats_s)
    if feats_s.dim() != 3 or feats_q.dim() != 3:
        raise FumiHipError(f"{name}: feats_s [B,S,F] and feats_q [B,Qn,F] expected")
    if metric is not None and metric not in TRANS_METRICS:
        raise FumiHipError(f"{name}: metric must be cosine or euclid, got {metric}")
    B, S, F = (int(v) for v in feats_s.shape)
    Qn = int(feats_q.shape[1])
    N = int(n_way) if n_way is not None else int(y_s.max().item()) + 1
    _shape(feats_q, (B, Qn, F), "feats_q"); _shape(y_s, (B, S), "y_s"); _shape(y_q, (B, Qn), "y_q")
    if param is not None:
        _shape(*param)
    out = dict(loss=torch.empty(1, device=dev, dtype=torch.float32), correct=torch.empty(1, device=dev, dtype=torch.float32),
               preds=torch.empty(B, Qn, device=dev, dtype=torch.int64),
               logits=torch.empty(B, Qn, N, device=dev, dtype=torch.float32) if want_logits else None)
    return dev, (B, S, Qn, N, F), out


def _episode_head_args(dims, feats_s, y_s, feats_q, y_q, out):
    """The leading (dims, features, labels) and the trailing (loss, correct, preds, logits) ctypes arguments of an episode head's
    entry, with their dtype checks; called after the gradients' shapes are checked, as the order of errors always was."""
    lead = (*dims, _f32(feats_s, "feats_s"), _i64(y_s, "y_s"), _f32(feats_q, "feats_q"), _i64(y_q, "y_q"))
    tail = (_f32(out["loss"], "loss"), _f32(out["correct"], "correct"), _i64(out["preds"], "preds"),
            _f32(out["logits"], "logits") if out["logits"] is not None else None)
    return lead, tail


def _head_grads(dev, need_grad, out, **given):
    """The three gradients of a head, name=(shape, tensor given or None): into ``out`` the tensors given, else new ones, None without
    need_grad; returns their ctypes arguments."""
    args = []
    for name, (shape, t) in given.items():
        if need_grad:
            t = torch.empty(*shape, device=dev, dtype=torch.float32) if t is None else t
            _shape(t, shape, name)
        out[name] = t if need_grad else None
        args.append(_f32(t, name) if need_grad else None)
    return args


def cos_proto_step(ws, feats_s, y_s, feats_q, y_q, tau, *, need_grad=True, grad_scale=1.0, want_logits=False, dfeats_s=None,
                   dfeats_q=None, dtau=None, n_way=None):
    """The fused cosine nearest-centroid head (csrc/cosproto.hip): per episode the class means of feats_s [B,S,F] by y_s [B,S], logits
    tau * cos(feats_q [B,Qn,F], mean), mean softmax cross-entropy against y_q [B,Qn] over all B * Qn rows.  ``tau`` is a GPU tensor [1]
    (the kernels read it on the device); ``n_way`` defaults to int(y_s.max()) + 1, which synchronises -- callers that know N pass it.
    Returns a dict of GPU tensors: loss [1], correct [1] (count, float), preds [B,Qn] (first arg-max), logits [B,Qn,N] (None without
    want_logits) and, with need_grad, dfeats_s [B,S,F], dfeats_q [B,Qn,F], dtau [1] = gradients of grad_scale * loss (written into the
    tensors given, else into new ones)."""
    dev, dims, out = _episode_head_io("cos_proto_step", feats_s, y_s, feats_q, y_q, n_way, want_logits,
                                                              param=(tau, (1,), "tau"))
    B, S, Qn, N, F = dims
    grads = _head_grads(dev, need_grad, out, dfeats_s=((B, S, F), dfeats_s), dfeats_q=((B, Qn, F), dfeats_q), dtau=((1,), dtau))
    lead, tail = _episode_head_args(dims, feats_s, y_s, feats_q, y_q, out)
    _check(lib().fumi_hip_cos_proto_step(ws.handle, _stream(dev), *lead, _f32(tau, "tau"), float(grad_scale), *tail, *grads),
           "fumi_hip_cos_proto_step")
    return out


def euclid_proto_step(ws, feats_s, y_s, feats_q, y_q, alpha, *, need_grad=True, grad_scale=1.0, want_logits=False, dfeats_s=None,
                      dfeats_q=None, dalpha=None, n_way=None):
    """The fused prototypical-network head (csrc/euclidproto.hip): per episode the class means of feats_s [B,S,F] by y_s [B,S], logits
    -alpha * |feats_q [B,Qn,F] - mean|^2, mean softmax cross-entropy against y_q [B,Qn] over all B * Qn rows.  ``alpha`` is a GPU tensor
    [1] (the kernels read it on the device); ``n_way`` defaults to int(y_s.max()) + 1, which synchronises -- callers that know N pass
    it.  Returns a dict of GPU tensors: loss [1], correct [1] (count, float), preds [B,Qn] (first arg-max), logits [B,Qn,N] (None
    without want_logits) and, with need_grad, dfeats_s [B,S,F], dfeats_q [B,Qn,F], dalpha [1] = gradients of grad_scale * loss (written
    into the tensors given, else into new ones)."""
    dev, dims, out = _episode_head_io("euclid_proto_step", feats_s, y_s, feats_q, y_q, n_way, want_logits,
                                                              param=(alpha, (1,), "alpha"))
    B, S, Qn, N, F = dims
    grads = _head_grads(dev, need_grad, out, dfeats_s=((B, S, F), dfeats_s), dfeats_q=((B, Qn, F), dfeats_q), dalpha=((1,), dalpha))
    lead, tail = _episode_head_args(dims, feats_s, y_s, feats_q, y_q, out)
    _check(lib().fumi_hip_euclid_proto_step(ws.handle, _stream(dev), *lead, _f32(alpha, "alpha"), float(grad_scale), *tail, *grads),
           "fumi_hip_euclid_proto_step")
    return out


def match_head_step(ws, feats_s, y_s, feats_q, y_q, tau, *, need_grad=True, grad_scale=1.0, want_logits=False, dfeats_s=None,
                    dfeats_q=None, dtau=None, n_way=None):
    """The fused Matching Networks head (csrc/matchhead.hip): per episode a query row of feats_q [B,Qn,F] attends over the individual
    rows of feats_s [B,S,F] at tau * cos(query, support row); the logit of class n is the log-sum-exp of those scores over the support
    rows with y_s == n (the log of the attention mass on the class, up to the row's normaliser), mean softmax cross-entropy against y_q
    [B,Qn] over all B * Qn rows.  ``tau`` is a GPU tensor [1] (the kernels read it on the device); ``n_way`` defaults to
    int(y_s.max()) + 1, which synchronises -- callers that know N pass it.  A class without a support row has the logit -inf and a
    query row labelled with it is left out (FUMI_ST_CLASS_MISSING).  Returns a dict of GPU tensors: loss [1], correct [1] (count, float),
    preds [B,Qn] (first arg-max), logits [B,Qn,N] (None without want_logits) and, with need_grad, dfeats_s [B,S,F], dfeats_q [B,Qn,F],
    dtau [1] = gradients of grad_scale * loss (written into the tensors given, else into new ones)."""
    dev, dims, out = _episode_head_io("match_head_step", feats_s, y_s, feats_q, y_q, n_way, want_logits,
                                                               param=(tau, (1,), "tau"))
    B, S, Qn, N, F = dims
    grads = _head_grads(dev, need_grad, out, dfeats_s=((B, S, F), dfeats_s), dfeats_q=((B, Qn, F), dfeats_q), dtau=((1,), dtau))
    lead, tail = _episode_head_args(dims, feats_s, y_s, feats_q, y_q, out)
    _check(lib().fumi_hip_match_head_step(ws.handle, _stream(dev), *lead, _f32(tau, "tau"), float(grad_scale), *tail, *grads),
           "fumi_hip_match_head_step")
    return out


RELATION_PARAMS = ("w1", "b1", "w2", "b2")      # the relation module's tensors, in the order of the entry's arguments
RELATION_LOSSES = {"ce": 0, "mse": 1}


def relation_head_step(ws, feats_s, y_s, feats_q, y_q, params, *, loss="mse", need_grad=True, grad_scale=1.0, want_logits=False,
                       want_hidden=False, dfeats_s=None, dfeats_q=None, g_w=None, n_way=None):
    """The fused Relation Network head (csrc/relationhead.hip): per episode the class means c_n of feats_s
    [B,S,F] by y_s [B,S], U = W1s c_n + b1, V = W1q feats_q [B,Qn,F], logits z[q,n] = w2 . relu(U[n] + V[q]) + b2 -- the relation
    module Linear(2F,H) -> ReLU -> Linear(H,1) on (class mean, query) without the concatenation.  ``params`` = (w1 [2,H,F], b1 [H],
    w2 [H], b2 [1]) on the device; ``loss`` is ``mse`` (the paper's: mean over B * Qn * N of (sigmoid(z) - onehot)^2) or ``ce`` (softmax
    cross-entropy over the classes, mean over B * Qn); ``n_way`` defaults to int(y_s.max()) + 1, which synchronises.  Returns a dict of
    GPU tensors: loss [1], correct [1] (count, float), preds [B,Qn] (first arg-max), logits [B,Qn,N] (None without want_logits), with
    want_hidden hid_s [B,N,H] = U and hid_q [B,Qn,H] = V (the mask of the backward is hid_s + hid_q > 0 in fp32), and, with need_grad,
    dfeats_s [B,S,F], dfeats_q [B,Qn,F], dw1, db1, dw2, db2 = gradients of grad_scale * loss.  ``g_w`` = four caller-owned tensors
    (slices of a flat buffer) that receive dw1, db1, dw2, db2 in place."""
    if loss not in RELATION_LOSSES:
        raise FumiHipError(f"relation_head_step: loss must be mse or ce, got {loss}")
    if len(params) != len(RELATION_PARAMS):
        raise FumiHipError(f"relation_head_step: params = ({', '.join(RELATION_PARAMS)}) expected, got {len(params)} tensors")
    if params[0].dim() != 3:
        raise FumiHipError("relation_head_step: w1 [2,H,F] expected")
    dev, dims, out = _episode_head_io("relation_head_step", feats_s, y_s, feats_q, y_q, n_way, want_logits)
    B, S, Qn, N, F = dims
    H = int(params[0].shape[1])
    shapes = ((2, H, F), (H,), (H,), (1,))
    for t, shape, nm in zip(params, shapes, RELATION_PARAMS):
        _shape(t, shape, nm)
    out["hid_s"] = torch.empty(B, N, H, device=dev, dtype=torch.float32) if want_hidden else None
    out["hid_q"] = torch.empty(B, Qn, H, device=dev, dtype=torch.float32) if want_hidden else None
    if g_w is not None and len(g_w) != len(RELATION_PARAMS):
        raise FumiHipError(f"relation_head_step: g_w: {len(RELATION_PARAMS)} tensors expected, got {len(g_w)}")
    given = dict(dfeats_s=((B, S, F), dfeats_s), dfeats_q=((B, Qn, F), dfeats_q))
    for i, (shape, nm) in enumerate(zip(shapes, RELATION_PARAMS)):
        given["d" + nm] = (shape, g_w[i] if g_w is not None else None)
    grads = _head_grads(dev, need_grad, out, **given)
    lead, tail = _episode_head_args(dims, feats_s, y_s, feats_q, y_q, out)
    hid = tuple(_f32(out[k], k) if want_hidden else None for k in ("hid_s", "hid_q"))
    _check(lib().fumi_hip_relation_head_step(ws.handle, _stream(dev), *lead[:5], H, *lead[5:],
                                             *(_f32(t, nm) for t, nm in zip(params, RELATION_PARAMS)), RELATION_LOSSES[loss],
                                             float(grad_scale), *tail, *hid, *grads), "fumi_hip_relation_head_step")
    return out


FEAT_PARAMS = ("wqkv", "wo", "bo", "ln_weight", "ln_bias")      # the adaptation's tensors, in the order of the entries' arguments


def _feat_adapt_io(name, feats_s, y_s, w, n_way):
    """The checks the two adaptation entries share: feats_s [B,S,F], y_s [B,S], w = (wqkv [3F,F], wo [F,F], bo, ln_weight, ln_bias
    [F]).  Returns (dev, (B, S, N, F), the ctypes arguments from feats_s to ln_bias)."""
    dev = _dev(feats_s)
    if feats_s.dim() != 3:
        raise FumiHipError(f"{name}: feats_s [B,S,F] expected")
    if len(w) != len(FEAT_PARAMS):
        raise FumiHipError(f"{name}: w = ({', '.join(FEAT_PARAMS)}) expected, got {len(w)} tensors")
    B, S, F = (int(v) for v in feats_s.shape)
    N = int(n_way) if n_way is not None else int(y_s.max().item()) + 1
    _shape(y_s, (B, S), "y_s")
    for t, shape, nm in zip(w, ((3 * F, F), (F, F), (F,), (F,), (F,)), FEAT_PARAMS):
        _shape(t, shape, nm)
    args = (_f32(feats_s, "feats_s"), _i64(y_s, "y_s"), *(_f32(t, nm) for t, nm in zip(w, FEAT_PARAMS)))
    return dev, (B, S, N, F), args


def feat_adapt_fwd(ws, feats_s, y_s, w, *, n_way=None, keep_tape=False):
    """The set-to-set prototype adaptation (csrc/featadapt.hip): the class means of feats_s [B,S,F] by y_s [B,S]
    through one self-attention block over the N prototypes of each episode, a residual and a LayerNorm.  ``w`` = (wqkv [3F,F], wo
    [F,F], bo [F], ln_weight [F], ln_bias [F]); ``n_way`` defaults to int(y_s.max()) + 1, which synchronises.  Returns (protos
    [B,N,F], tape): the adapted prototypes -- an N-way 1-shot support set with labels 0..N-1 for cos_proto_step / euclid_proto_step --
    and, with keep_tape, what feat_adapt_bwd needs (None otherwise: the forward form, same bits)."""
    dev, (B, S, N, F), args = _feat_adapt_io("feat_adapt_fwd", feats_s, y_s, w, n_way)
    protos = torch.empty(B, N, F, device=dev, dtype=torch.float32)
    tape = torch.empty(int(lib().fumi_hip_feat_adapt_tape_floats(B, N, F)), device=dev, dtype=torch.float32) if keep_tape else None
    _check(lib().fumi_hip_feat_adapt_fwd(ws.handle, _stream(dev), B, S, N, F, *args, _f32(protos, "protos"),
                                         _f32(tape, "tape") if keep_tape else None), "fumi_hip_feat_adapt_fwd")
    return protos, tape


def feat_adapt_bwd(ws, feats_s, y_s, w, tape, dprotos, *, n_way=None, dfeats_s=None, g_w=None):
    """The backward of feat_adapt_fwd for dprotos [B,N,F] (the head's dfeats_s): returns (dfeats_s [B,S,F], g_w) with g_w the
    gradients of ``w`` in its order, written into the tensors given (``g_w`` may be slices of one flat buffer), else into new ones."""
    dev, (B, S, N, F), args = _feat_adapt_io("feat_adapt_bwd", feats_s, y_s, w, n_way)
    if tape is None or tape.numel() != int(lib().fumi_hip_feat_adapt_tape_floats(B, N, F)):
        raise FumiHipError("feat_adapt_bwd: tape: not the tape of a feat_adapt_fwd call of these shapes")
    _shape(dprotos, (B, N, F), "dprotos")
    if dfeats_s is None:
        dfeats_s = torch.empty(B, S, F, device=dev, dtype=torch.float32)
    _shape(dfeats_s, (B, S, F), "dfeats_s")
    if g_w is None:
        g_w = [torch.empty_like(t) for t in w]
    if len(g_w) != len(FEAT_PARAMS):
        raise FumiHipError(f"feat_adapt_bwd: g_w: {len(FEAT_PARAMS)} tensors expected, got {len(g_w)}")
    for g, t, nm in zip(g_w, w, FEAT_PARAMS):
        _shape(g, tuple(t.shape), "d" + nm)
    _check(lib().fumi_hip_feat_adapt_bwd(ws.handle, _stream(dev), B, S, N, F, *args, _f32(tape, "tape"), _f32(dprotos, "dprotos"),
                                         _f32(dfeats_s, "dfeats_s"), *(_f32(g, "d" + nm) for g, nm in zip(g_w, FEAT_PARAMS))),
           "fumi_hip_feat_adapt_bwd")
    return dfeats_s, g_w


def ridge_head_step(ws, feats_s, y_s, feats_q, y_q, params, *, need_grad=True, grad_scale=1.0, want_logits=False, dfeats_s=None,
                    dfeats_q=None, dparams=None, n_way=None):
    """The fused ridge-regression head (csrc/ridgehead.hip): per episode A = (X X^T + exp(rho) I)^-1 onehot(y_s) on the support rows
    X = feats_s [B,S,F], logits alpha * feats_q [B,Qn,F] X^T A, mean softmax cross-entropy against y_q [B,Qn] over all B * Qn rows.
    ``params`` is a GPU tensor [2] = (rho, alpha) (the kernels read it on the device); ``n_way`` defaults to int(y_s.max()) + 1, which
    synchronises -- callers that know N pass it.  Returns a dict of GPU tensors: loss [1], correct [1] (count, float), preds [B,Qn]
    (first arg-max), logits [B,Qn,N] (None without want_logits) and, with need_grad, dfeats_s [B,S,F], dfeats_q [B,Qn,F], dparams [2] =
    gradients of grad_scale * loss through both solves (written into the tensors given, else into new ones)."""
    dev, dims, out = _episode_head_io("ridge_head_step", feats_s, y_s, feats_q, y_q, n_way, want_logits,
                                                              param=(params, (2,), "params"))
    B, S, Qn, N, F = dims
    grads = _head_grads(dev, need_grad, out, dfeats_s=((B, S, F), dfeats_s), dfeats_q=((B, Qn, F), dfeats_q), dparams=((2,), dparams))
    lead, tail = _episode_head_args(dims, feats_s, y_s, feats_q, y_q, out)
    _check(lib().fumi_hip_ridge_head_step(ws.handle, _stream(dev), *lead, _f32(params, "params"), float(grad_scale), *tail, *grads),
           "fumi_hip_ridge_head_step")
    return out


def logreg_set_form(form):
    """The form of the logistic-regression fit's K~ A product in the calls that follow: "valu", "mfma" or None (chosen per shape)."""
    _check(lib().fumi_hip_logreg_set_form({None: -1, "valu": 0, "mfma": 1}[form]), "fumi_hip_logreg_set_form")


def logreg_head_step(ws, feats_s, y_s, feats_q, y_q, *, steps=100, lr=1.0, momentum=0.9, C=1.0, normalize=True, want_logits=False,
                     n_way=None):
    """The fused logistic-regression head, forward only (csrc/logreghead.hip): per episode ``steps`` steps of heavy-ball descent (``lr``,
    ``momentum``) from zero on the multinomial logistic regression of the support rows feats_s [B,S,F] (L2-normalised when
    ``normalize``) with weight decay 1 / (C n), fitted in LDS in the dual; logits of feats_q [B,Qn,F] (normalised alike), mean softmax
    cross-entropy against y_q [B,Qn] over all B * Qn rows.  ``n_way`` defaults to int(y_s.max()) + 1, which synchronises -- callers
    that know N pass it.  Returns a dict of GPU tensors: loss [1], correct [1] (count, float), preds [B,Qn] (first arg-max), logits
    [B,Qn,N] (None without want_logits).  The fit is not differentiated: there are no gradients."""
    dev, dims, out = _episode_head_io("logreg_head_step", feats_s, y_s, feats_q, y_q, n_way, want_logits)
    lead, tail = _episode_head_args(dims, feats_s, y_s, feats_q, y_q, out)
    _check(lib().fumi_hip_logreg_head_step(ws.handle, _stream(dev), *lead, int(steps), float(lr), float(momentum), float(C),
                                           1 if normalize else 0, *tail), "fumi_hip_logreg_head_step")
    return out


def svm_set_form(form):
    """The form of the SVM head's K' alpha products in the calls that follow: "valu", "mfma" or None (chosen per shape)."""
    _check(lib().fumi_hip_svm_set_form({None: -1, "valu": 0, "mfma": 1}[form]), "fumi_hip_svm_set_form")


def svm_head_step(ws, feats_s, y_s, feats_q, y_q, scale, *, C=0.1, eps=1.0, steps=120, bwd_steps=40, need_grad=True, grad_scale=1.0,
                  want_logits=False, dfeats_s=None, dfeats_q=None, dscale=None, n_way=None):
    """The fused MetaOptNet-SVM head (csrc/svmhead.hip): per episode the Crammer-Singer dual on K' = X X^T + eps I of the support rows
    X = feats_s [B,S,F] (alpha <= C onehot(y_s), rows summing to zero) fitted by ``steps`` steps of FISTA in LDS, logits
    scale * feats_q [B,Qn,F] X^T alpha, mean softmax cross-entropy against y_q [B,Qn] over all B * Qn rows.  ``scale`` is a GPU tensor
    [1] (the kernels read it on the device); ``n_way`` defaults to int(y_s.max()) + 1, which synchronises -- callers that know N pass
    it.  Returns a dict of GPU tensors: loss [1], correct [1] (count, float), preds [B,Qn] (first arg-max), logits [B,Qn,N] (None
    without want_logits), stats [B,2] (the fit's KKT residual and the relative residual of the backward's conjugate gradients, 0
    without need_grad) and, with need_grad, dfeats_s [B,S,F], dfeats_q [B,Qn,F], dscale [1] = the implicit gradients of grad_scale *
    loss at the fitted point, ``bwd_steps`` steps of conjugate gradients (written into the tensors given, else into new ones)."""
    dev, dims, out = _episode_head_io("svm_head_step", feats_s, y_s, feats_q, y_q, n_way, want_logits,
                                                              param=(scale, (1,), "scale"))
    B, S, Qn, N, F = dims
    grads = _head_grads(dev, need_grad, out, dfeats_s=((B, S, F), dfeats_s), dfeats_q=((B, Qn, F), dfeats_q), dscale=((1,), dscale))
    lead, tail = _episode_head_args(dims, feats_s, y_s, feats_q, y_q, out)
    out["stats"] = torch.empty(B, 2, device=dev, dtype=torch.float32)
    _check(lib().fumi_hip_svm_head_step(ws.handle, _stream(dev), *lead, _f32(scale, "scale"), float(C), float(eps), int(steps),
                                        int(bwd_steps), float(grad_scale), *tail, *grads, _f32(out["stats"], "stats")),
           "fumi_hip_svm_head_step")
    return out


def svm_get_fit(ws, B, S, N):
    """(alpha [B,S,N] float32, bound mask [B,S,N] bool) of the ``svm_head_step`` call that was the last call on ``ws``.  For tests."""
    dev = ws.device
    alpha = torch.empty(B, S, N, device=dev, dtype=torch.float32)
    mask = torch.empty(B, S, N, device=dev, dtype=torch.int32)
    _check(lib().fumi_hip_svm_get_fit(ws.handle, _stream(dev), int(B), int(S), int(N), ctypes.c_void_p(alpha.data_ptr()),
                                      ctypes.c_void_p(mask.data_ptr())), "fumi_hip_svm_get_fit")
    return alpha, mask != 0


TRANS_METRICS = {"cosine": 0, "euclid": 1}


def trans_proto_step(ws, feats_s, y_s, feats_q, y_q, scale, *, metric, steps, want_logits=False, n_way=None):
    """Transductive prototype refinement, forward only (csrc/transproto.hip): per episode ``steps`` steps of soft k-means on the query
    rows feats_q [B,Qn,F] from the class means of feats_s [B,S,F] by y_s [B,S], c_n <- (s_n + sum_q w[q,n] f_q) / (k_n + sum_q w[q,n])
    with w = softmax_n(z); z = scale * cos(query, c_n) for ``metric="cosine"``, -scale * |query - c_n|^2 for ``metric="euclid"``; mean
    softmax cross-entropy of the refined logits against y_q [B,Qn] over all B * Qn rows.  ``scale`` is a GPU tensor [1] (the kernel
    reads it on the device); ``n_way`` defaults to int(y_s.max()) + 1, which synchronises -- callers that know N pass it.  ``steps=0``
    is the forward form of ``cos_proto_step`` / ``euclid_proto_step``.  Returns a dict of GPU tensors: loss [1], correct [1] (count,
    float), preds [B,Qn] (first arg-max), logits [B,Qn,N] (None without want_logits).  There are no gradients."""
    dev, dims, out = _episode_head_io("trans_proto_step", feats_s, y_s, feats_q, y_q, n_way, want_logits,
                                               param=(scale, (1,), "scale"), metric=metric)
    lead, tail = _episode_head_args(dims, feats_s, y_s, feats_q, y_q, out)
    _check(lib().fumi_hip_trans_proto_step(ws.handle, _stream(dev), *lead, _f32(scale, "scale"), TRANS_METRICS[metric], int(steps),
                                           *tail), "fumi_hip_trans_proto_step")
    return out


def cls_head_step_soft(ws, feats, y_a, W, b, *, y_b=None, lam=1.0, smoothing=0.0, need_grad=True, grad_scale=1.0, dfeats=None,
                       gW=None, gb=None, want_preds=True):
    """``cls_head_step`` against the soft target t = (1 - smoothing) (lam onehot(y_a) + (1 - lam) onehot(y_b)) + smoothing / C
    (fumi_hip_cls_head_step_soft: label smoothing, mixup / CutMix labels).  ``y_b`` None: y_b = y_a, and lam must be 1.  ``correct``
    counts against y_a.  The same dict as ``cls_head_step``."""
    dev, (M, F, C), out = _cls_head_io("cls_head_step_soft", feats, W, (b, "b"), (y_a, "y_a"), y_b, want_preds)
    grads = _head_grads(dev, need_grad, out, dfeats=((M, F), dfeats), gW=((C, F), gW), gb=((C,), gb))
    _check(lib().fumi_hip_cls_head_step_soft(ws.handle, _stream(dev), M, F, C, _f32(feats, "feats"), _i64(y_a, "y_a"),
                                             *_soft_args(y_b, lam, smoothing), _f32(W, "W"), _f32(b, "b"), float(grad_scale),
                                             *_cls_head_outs(out), *grads), "fumi_hip_cls_head_step_soft")
    return out


def cos_cls_head_step(ws, feats, y_a, W, tau, *, y_b=None, lam=1.0, smoothing=0.0, need_grad=True, grad_scale=1.0, dfeats=None,
                      gW=None, dtau=None, want_preds=True):
    """The fused cosine classifier head (csrc/coshead.hip): mean cross-entropy of tau * cos(feats_m, W_c) against
    the soft target of ``cls_head_step_soft`` (``y_b`` None: y_b = y_a, and lam must be 1), with ``tau`` [1] on the device.  Returns a
    dict of GPU tensors: loss [1], correct [1] (count against y_a, float), preds [M] (first arg-max; None without want_preds) and, with
    need_grad, dfeats [M,F], gW [C,F], dtau [1] = gradients of grad_scale * loss (written into the tensors given, else into new ones)."""
    dev, (M, F, C), out = _cls_head_io("cos_cls_head_step", feats, W, (tau, "tau"), (y_a, "y_a"), y_b, want_preds)
    grads = _head_grads(dev, need_grad, out, dfeats=((M, F), dfeats), gW=((C, F), gW), dtau=((1,), dtau))
    _check(lib().fumi_hip_cos_cls_head_step(ws.handle, _stream(dev), M, F, C, _f32(feats, "feats"), _i64(y_a, "y_a"),
                                            *_soft_args(y_b, lam, smoothing), _f32(W, "W"), _f32(tau, "tau"), float(grad_scale),
                                            *_cls_head_outs(out), *grads), "fumi_hip_cos_cls_head_step")
    return out


def cls_head_step_distill(ws, feats, y_a, W, b, feats_t, W_t, b_t, *, temp, alpha, ce_weight, y_b=None, lam=1.0, smoothing=0.0,
                          need_grad=True, grad_scale=1.0, dfeats=None, gW=None, gb=None, want_preds=True):
    """``cls_head_step_soft`` as the student of a frozen teacher (fumi_hip_cls_head_step_distill): with
    z_t = feats_t @ W_t.T + b_t and T = ``temp``, loss = ce_weight * loss_ce + alpha * loss_kd, loss_kd = T^2 KL(softmax(z_t / T) ||
    softmax(z / T)) (batch mean).  The dict of ``cls_head_step_soft`` plus loss_ce [1], loss_kd [1] (views of loss_parts [2]) and
    agree [1] (rows whose arg-max equals the teacher's, float)."""
    dev, (M, F, C), out = _cls_head_io("cls_head_step_distill", feats, W, (b, "b"), (y_a, "y_a"), y_b, want_preds,
                                       teacher=(feats_t, W_t, b_t))
    loss_parts = torch.empty(2, device=dev, dtype=torch.float32)
    agree = torch.empty(1, device=dev, dtype=torch.float32)
    grads = _head_grads(dev, need_grad, out, dfeats=((M, F), dfeats), gW=((C, F), gW), gb=((C,), gb))
    loss, correct, preds = _cls_head_outs(out)
    _check(lib().fumi_hip_cls_head_step_distill(ws.handle, _stream(dev), M, F, C, _f32(feats, "feats"), _i64(y_a, "y_a"),
                                                *_soft_args(y_b, lam, smoothing), _f32(W, "W"), _f32(b, "b"),
                                                _f32(feats_t, "feats_t"), _f32(W_t, "W_t"), _f32(b_t, "b_t"), float(temp), float(alpha),
                                                float(ce_weight), float(grad_scale), loss, _f32(loss_parts, "loss_parts"), correct,
                                                _f32(agree, "agree"), preds, *grads), "fumi_hip_cls_head_step_distill")
    out.update(loss_parts=loss_parts, loss_ce=loss_parts[0:1], loss_kd=loss_parts[1:2], agree=agree)
    return out


MIX_MIXUP, MIX_CUTMIX = 0, 1


def mix_images(ws, x, partner, *, mode, lam=1.0, box=(0, 0, 0, 0)):
    """The blend of a gathered batch ``x`` float32 [M, C, H, W] with its rows ``partner`` int64 [M] (csrc/immix.hip), a new tensor:
    ``mode`` MIX_MIXUP: lam x[i] + (1 - lam) x[partner[i]];  MIX_CUTMIX: x[partner[i]] inside ``box`` = (bx0, by0, bx1, by1) (columns
    bx0..bx1-1 of rows by0..by1-1), x[i] elsewhere.  A partner outside [0, M) sets ST_LABEL_RANGE and leaves its row unmixed."""
    dev = _dev(x)
    if (x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous() or not isinstance(partner, torch.Tensor)
            or partner.device != x.device or partner.dtype != torch.int64):
        raise FumiHipError("mix_images: x must be a contiguous float32 [M, C, H, W] device tensor and partner an int64 tensor on the "
                           f"same device; got {x.dtype} {tuple(x.shape)}")
    M, C, H, W = (int(s) for s in x.shape)
    _shape(partner, (M,), "partner")
    if len(box) != 4:
        raise FumiHipError("mix_images: box is (bx0, by0, bx1, by1)")
    partner = partner.contiguous()
    out = torch.empty_like(x)
    _check(lib().fumi_hip_mix_images(ws.handle, _stream(dev), M, C, H, W, _f32(x, "x"), _i64(partner, "partner"),
                                     int(mode), float(lam), *(int(v) for v in box), _f32(out, "out")), "fumi_hip_mix_images")
    return out


CLIP_KEYS = ["text_fc.weight", "text_fc.bias", "text_fc2.weight", "text_fc2.bias",
             "image_fc.weight", "image_fc.bias", "image_fc2.weight", "image_fc2.bias"]


def clip_step(ws, text, image, w, *, need_loss=True, need_grad=True, g_w=None):
    """CLIP baseline (fumi/models/clip.py): sim [nt, ni]; with need_loss the symmetric cross-entropy [1] and, with need_grad, its
    gradients w.r.t. the eight tensors of CLIP_KEYS order."""
    dev = _dev(text)
    nt, Dt = text.shape
    ni, D = image.shape
    P = int(w[0].shape[0])
    for t, shp, k in zip(w, [(P, Dt), (P,), (P, P), (P,), (P, D), (P,), (P, P), (P,)], CLIP_KEYS):
        _shape(t, shp, k)
    sim = torch.empty(nt, ni, device=dev, dtype=torch.float32)
    loss = torch.empty(1, device=dev, dtype=torch.float32) if need_loss else None
    if need_grad and g_w is None:
        g_w = [torch.empty_like(t) for t in w]
    _check(lib().fumi_hip_clip_step(ws.handle, _stream(dev), nt, ni, Dt, D, P, _f32(text, "text"), _f32(image, "image"), _parr(w, "w"),
                                    int(bool(need_grad)), _f32(sim, "sim"), _f32(loss, "loss") if need_loss else None,
                                    _parr(g_w, "g_w") if need_grad else None), "fumi_hip_clip_step")
    return dict(sim=sim, loss=loss, grads=g_w if need_grad else None)


def lstm_bidir(ws, tokens, table, lstm_w, pad_id, use_cell):
    """[..., 2H] final states of a bidirectional LSTM over the non-PAD prefix of token rows [..., L] (common.py:44-161)."""
    dev = _dev(tokens)
    L = tokens.shape[-1]
    R = tokens.numel() // L
    V, E = table.shape
    H = int(lstm_w[1].shape[1])
    for d in range(2):
        _shape(lstm_w[4 * d], (4 * H, E), "weight_ih"); _shape(lstm_w[4 * d + 1], (4 * H, H), "weight_hh")
        _shape(lstm_w[4 * d + 2], (4 * H,), "bias_ih"); _shape(lstm_w[4 * d + 3], (4 * H,), "bias_hh")
    out = torch.empty(*tokens.shape[:-1], 2 * H, device=dev, dtype=torch.float32)
    _check(lib().fumi_hip_lstm_bidir(ws.handle, _stream(dev), R, L, E, H, _i64(tokens, "tokens"), int(pad_id), _f32(table, "table"), V,
                                     _parr(lstm_w, "lstm_w"), int(bool(use_cell)), _f32(out, "out")), "fumi_hip_lstm_bidir")
    return out


def _lstm_dims(tokens, table, lstm_w):
    L = tokens.shape[-1]
    R = tokens.numel() // L
    V, E = table.shape
    H = int(lstm_w[1].shape[1])
    for d in range(2):
        _shape(lstm_w[4 * d], (4 * H, E), "weight_ih"); _shape(lstm_w[4 * d + 1], (4 * H, H), "weight_hh")
        _shape(lstm_w[4 * d + 2], (4 * H,), "bias_ih"); _shape(lstm_w[4 * d + 3], (4 * H,), "bias_hh")
    return R, L, V, E, H


def lstm_bidir_train(ws, tokens, table, lstm_w, pad_id, use_cell):
    """(out [..., 2H], tape): lstm_bidir keeping what lstm_bidir_bwd needs (--fine_tune with RNN / RNNhid, fumi.py:65-67)."""
    dev = _dev(tokens)
    R, L, V, E, H = _lstm_dims(tokens, table, lstm_w)
    out = torch.empty(*tokens.shape[:-1], 2 * H, device=dev, dtype=torch.float32)
    tape = torch.empty(int(lib().fumi_hip_lstm_tape_floats(R, L, E, H)), device=dev, dtype=torch.float32)
    _check(lib().fumi_hip_lstm_bidir_train(ws.handle, _stream(dev), R, L, E, H, _i64(tokens, "tokens"), int(pad_id), _f32(table, "table"),
                                           V, _parr(lstm_w, "lstm_w"), int(bool(use_cell)), _f32(out, "out"), _f32(tape, "tape")),
           "fumi_hip_lstm_bidir_train")
    return out, tape


def lstm_bidir_bwd(ws, tokens, table, lstm_w, pad_id, use_cell, tape, d_out):
    """Gradients of the 8 LSTM tensors for the output adjoint d_out [..., 2H] of the lstm_bidir_train call that wrote `tape`."""
    dev = _dev(tokens)
    R, L, V, E, H = _lstm_dims(tokens, table, lstm_w)
    if tape.numel() != int(lib().fumi_hip_lstm_tape_floats(R, L, E, H)):
        raise ValueError("tape: not the tape of a lstm_bidir_train call of these shapes")
    if d_out.numel() != R * 2 * H:
        raise ValueError(f"d_out: expected {R * 2 * H} elements, got {d_out.numel()}")
    g_w = [torch.empty_like(t) for t in lstm_w]
    _check(lib().fumi_hip_lstm_bidir_bwd(ws.handle, _stream(dev), R, L, E, H, _i64(tokens, "tokens"), int(pad_id), _parr(lstm_w, "lstm_w"),
                                         int(bool(use_cell)), _f32(tape, "tape"), _f32(d_out, "d_out"), _parr(g_w, "g_w")),
           "fumi_hip_lstm_bidir_bwd")
    return g_w
