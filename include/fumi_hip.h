/*
 * fumi_hip.h -- C ABI of the MI355X (gfx950) episodic meta-training engine.
 *
 * The reference (s-a-malik/fumi) has no FFI: its seam is a Python API.  This ABI is what replaces the
 * arithmetic the reference obtains from torch autograd + torchmeta *inside* these Python entry points
 * (citations into /root/reference):
 *
 *   fumi_hip_fumi_step   <- FUMI.evaluate                 fumi/models/fumi.py:115-196
 *                           (+ get_hyper_params :198-212, im_forward :214-218, hyper_net :70-86,104-113)
 *   fumi_hip_maml_step   <- maml.evaluate                 fumi/models/maml.py:134-193 (PureImageNetwork :15-33)
 *   fumi_hip_am3_step    <- AM3.evaluate / forward        fumi/models/am3.py:90-126,128-212
 *                           (+ get_prototypes / prototypical_loss / get_preds  fumi/utils/utils.py:302-402)
 *   fumi_hip_glove_bag   <- WordEmbedding.forward         fumi/models/common.py:23-41
 *   fumi_hip_class_text_select <- the per-class "first support row" loop  fumi/models/fumi.py:207-210
 *   fumi_hip_linear_*    <- torchmeta MetaLinear.forward / autograd AddmmBackward (requirements.txt:10)
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer borrowed for the call (owned by the caller, e.g. a torch tensor);
 *     row-major, contiguous; fp32 values, int64 labels/tokens (the dtypes the reference's tensors have).
 *   - `theta`, `phi`, `g_theta`, `g_phi`, `hid` are HOST arrays (of device pointers / ints).
 *   - `stream` is a hipStream_t (NULL = the null stream).  All work is enqueued asynchronously on it; no call
 *     synchronises the device except workspace growth and fumi_hip_read_status.
 *   - return value: 0 on success, a negative FUMI_E* code otherwise; fumi_hip_strerror() names it.
 *   - one workspace per (process, device); a workspace is not re-entrant.
 *   - gradients are written (not accumulated) as  grad_scale * SUM over the call's episodes of d(loss_b)/d(param);
 *     pass grad_scale = 1/B for the reference's mean loss on one GPU, 1/B_global before an all-reduce(sum).
 */
#ifndef FUMI_HIP_H
#define FUMI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fumi_ws fumi_ws_t;
typedef void* fumi_stream_t;          /* hipStream_t */

#define FUMI_OK            0
#define FUMI_EINVAL      (-1)         /* bad argument (shape, NULL pointer, unsupported size) */
#define FUMI_ENOMEM      (-2)         /* workspace allocation failed */
#define FUMI_EHIP        (-3)         /* a HIP runtime call or kernel launch failed (see fumi_hip_last_hip_error) */
#define FUMI_ENOTSUP     (-4)         /* valid request this build does not implement */

/* device-side status bits (fumi_hip_read_status) -- the reference raises IndexError in both situations */
#define FUMI_ST_LABEL_RANGE   1       /* a label outside [0, N) */
#define FUMI_ST_CLASS_MISSING 2       /* a class without a support sample (fumi.py:209 would raise) */
#define FUMI_ST_SYNC_TIMEOUT  4       /* a workgroup gave up waiting for the sibling workgroups of its episode (split inner loop /
                                       * split reverse sweep): the step's results are not to be trusted; the host raises RuntimeError */
#define FUMI_ST_NOT_POSDEF    8       /* a pivot of the ridge head's Cholesky factorisation was not > 0 (a NaN counts) and was replaced
                                       * by lambda: the episode's results are not to be trusted; the host raises FloatingPointError */

#define FUMI_MAX_HIDDEN 8

int          fumi_hip_version(void);
const char*  fumi_hip_strerror(int code);
const char*  fumi_hip_last_hip_error(void);

/* A workspace owns all device memory the library allocates for its device: the scratch slab (grown on demand, bump-allocated per
 * call), a few small counters / the status word, and -- since round 2 -- the bf16 planes of the forward pass's column operand
 * (W0 and the support rows split once per step, ~16 MB at the reference sizes; rebuilt by every step, nothing to keep coherent). */
int   fumi_hip_workspace_create(int device, size_t bytes_hint, fumi_ws_t** out);
void  fumi_hip_workspace_destroy(fumi_ws_t* ws);
size_t fumi_hip_workspace_bytes(const fumi_ws_t* ws);
/* Copies the device status word to the host (synchronises `stream`) and clears it. */
int   fumi_hip_read_status(fumi_ws_t* ws, fumi_stream_t stream, int* status_out);
/* Polls a workgroup spends waiting for the sibling workgroups of its episode before it sets FUMI_ST_SYNC_TIMEOUT (process-wide;
 * default 1 << 22, about a second).  Tests set 0 to see the bit; returns the previous value. */
int   fumi_hip_set_spin_limit(int polls);
/* Development hooks: a device buffer of uint64 wall-clock stamps written by block 0 of the per-episode kernels (which = 0) or by
 * every workgroup of the forward X-panel kernel (which = 1), or cycle stamps of wave 0 of the middle workgroup of a ResNet-12
 * convolution launch (which = 2); NULL switches the stamps off (the default). */
int   fumi_hip_set_trace_buffer(int which, void* device_u64);

/* ---- in-library phase timing (HIP events recorded on the caller's stream around each phase) ---------------------
 * Used by bench.py to time the dominant kernel live inside the timed region.  Off by default (no events recorded). */
#define FUMI_PH_SELECT     0   /* class text select                                   */
#define FUMI_PH_HYPER_FWD  1   /* hypernetwork forward (2 GEMMs)                       */
#define FUMI_PH_GEMM_A0S   2   /* AM3: image encoder on the support rows               */
#define FUMI_PH_GEMM_A0Q   3   /* AM3: image encoder on the query rows                 */
#define FUMI_PH_XPANEL_FWD 4   /* [A0|G] = [Xs;Xq][W0;Xs]^T  <- dominant kernel of the FuMI/MAML step */
#define FUMI_PH_ADAPT      5   /* inner loop                                           */
#define FUMI_PH_QUERY      6   /* query forward/backward                               */
#define FUMI_PH_REVERSE    7   /* second-order reverse sweep                           */
#define FUMI_PH_REDUCE     8   /* sums over episodes                                   */
#define FUMI_PH_XPANEL_BWD 9   /* gW0 = Abar0^T X (split-K slabs + slab reduce)        */
#define FUMI_PH_HYPER_BWD 10   /* hypernetwork backward                                */
#define FUMI_PH_AM3       11   /* AM3 fused head kernels                               */
#define FUMI_PH_CONV_GEMM 12   /* Conv4: the 64 -> 64 channel products (forward, input-gradient, weight-gradient) on the MFMA */
#define FUMI_PH_CONV_FIRST 13  /* Conv4: block 1 (Cin <= 3 -> 64: K = 27, bound by writing / reading its 84x84x64 maps)   */
#define FUMI_PH_CONV_EW   14   /* Conv4: batch-norm / ReLU / max-pool passes, head, updates                               */
#define FUMI_PH_RN_CONV   15   /* ResNet-12 (bf16): forward / input-gradient convolutions on v_mfma_f32_32x32x16_bf16       */
#define FUMI_PH_RN_WGRAD  16   /* ResNet-12: weight-gradient products                                                     */
#define FUMI_PH_RN_EW     17   /* ResNet-12: batch-norm / LeakyReLU / residual join / pooling passes, head, updates       */
#define FUMI_PH_COUNT     18
/* phase_mask: bit p set = record a HIP event pair around phase p (FUMI_PH_*) on the caller's stream; -1 = every phase,
 * 0 = off.  An event pair costs a few microseconds of stream time, so time only what is needed.  Also clears the records. */
int          fumi_hip_set_profiling(fumi_ws_t* ws, int phase_mask);
/* Time only every `every`-th occurrence of a selected phase (default 1): an event record is a ~6 us bubble on the stream. */
int          fumi_hip_set_profiling_every(fumi_ws_t* ws, int every);
/* Synchronises the device; total elapsed ms and number of records of `phase` since profiling was switched on. */
int          fumi_hip_get_profile(fumi_ws_t* ws, int phase, double* total_ms, int* count);
const char*  fumi_hip_phase_name(int phase);

/* ---- FuMI meta-step (replaces fumi/models/fumi.py:146-192 for B episodes) ------------------------------------
 * theta   : 2*n_hidden pointers  W_i [hid[i], hid[i-1]] (hid[-1] = D), b_i [hid[i]]   (im_net.linear{i}.*)
 * phi     : 4 pointers           A0 [Ht,Dt], a0 [Ht], A1 [H+1,Ht], a1 [H+1]           (hyper_net.0.*, hyper_net.2.*)
 * cls_text: [B,N,Dt] per-class text encodings, or NULL to select them from text_s [B,S,Dt] (first support row of
 *           each class, fumi.py:207-210)
 * outputs : logits_q [B,Qn,N], preds_q [B,Qn] (first arg-max), preds_q_f32 [B,Qn] or NULL (the same indices as floats:
 *           what the reference's float `test_preds` tensor holds, fumi.py:180-183), loss_b [B] (query CE), acc_b [B];
 *           stats [2] (optional, may be NULL) = grad_scale * (sum_b loss_b, sum_b acc_b): with grad_scale = 1/B the
 *           meta-batch mean loss / accuracy that fumi.py:187-188 computes, ready for the same all-reduce as the gradients;
 *           g_theta/g_phi (same shapes as theta/phi) only when need_grad != 0;
 *           g_cls_text [B*N,Dt] or NULL: the text gradient (contract: "The text gradient" below, before fumi_hip_fumi_step_indexed).
 * second-order outer gradient always (fumi.py:176 hard-codes first_order=False).
 * dropout_p > 0 applies the reference's train-mode Dropout after every ReLU of im_net (fumi.py:93-99) with a fresh mask per
 * forward call (each inner step and the query pass), drawn from a counter-based hash of (seed, episode, call, layer,
 * element): statistically the reference's nn.Dropout, not its RNG stream.  Pass 0 for task != "train". */
int fumi_hip_fumi_step(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int D, int n_hidden, const int* hid, int Dt, int Ht,
        int T, float alpha, int tanh_head, int need_grad, float grad_scale, float dropout_p, uint64_t seed,
        const float* x_s, const int64_t* y_s, const float* x_q, const int64_t* y_q,
        const float* cls_text, const float* text_s,
        const float* const* theta, const float* const* phi,
        float* logits_q, int64_t* preds_q, float* preds_q_f32, float* loss_b, float* acc_b, float* stats,
        float* const* g_theta, float* const* g_phi, float* g_cls_text);

/* ---- MAML meta-step (replaces fumi/models/maml.py:156-191) ---------------------------------------------------
 * params: 2*n_hidden + 2 pointers: hidden layers as above, then lin_final W [N,H], b [N].  n_hidden = 0 is the reference's
 * hidden_dims=None: lin_final W [N,D] alone (hid may be NULL). */
int fumi_hip_maml_step(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int D, int n_hidden, const int* hid,
        int T, float alpha, int first_order, int need_grad, float grad_scale,
        const float* x_s, const int64_t* y_s, const float* x_q, const int64_t* y_q,
        const float* const* params,
        float* logits_q, int64_t* preds_q, float* preds_q_f32, float* loss_b, float* acc_b, float* stats,
        float* const* g_params);

/* ---- AM3 step (replaces am3.py:160-200 + utils.py:302-402, dropout 0) -----------------------------------------
 * w: 10 pointers  Wi [P,D], bi [P], G0 [Ht,Dt], g0 [Ht], G1 [P,Ht], g1 [P], H0 [Ht,P], h0 [Ht], H1 [1,Ht], h1 [1]
 * lamda_fixed: -1 = learned, 0 or 1 = fixed (am3.py:174-179).
 * dropout_p > 0: train-mode Dropout after the ReLU of g and of h (am3.py:82,88), counter-based masks from `seed`.
 * outputs: loss [1] (mean over B*Qn), preds_q [B,Qn] (first arg-min of the distances), lamda_s [B,S],
 *          correct [1] (number of correct query predictions, float); g_w (10 pointers) when need_grad;
 *          stats [3 + N*N] or NULL: [loss, correct count, grad_scale * sum_b mean_s lamda, confusion counts (rows = target
 *          class, columns = predicted class)] -- with grad_scale = 1 / global meta-batch a sum over ranks gives the global
 *          mean loss / lamda and the global counts, and fumi_hip_am3_metrics turns those into the reference's metrics. */
int fumi_hip_am3_step(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int D, int Dt, int Ht, int P, int lamda_fixed, int need_grad, float grad_scale,
        float dropout_p, uint64_t seed,
        const float* x_s, const int64_t* y_s, const float* x_q, const int64_t* y_q, const float* text_s,
        const float* const* w,
        float* loss, int64_t* preds_q, float* lamda_s, float* correct,
        float* const* g_w, float* stats, float* g_text);
/* The same step with the adjoints of the image rows as extra outputs (need_grad): dx_s [B,S,D], dx_q [B,Qn,D] = imbar Wi.  An
 * image encoder in front of the step (the Conv4 backbone at the image_encoder seam, am3.py:41-46) continues from them. */
int fumi_hip_am3_step_dx(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int D, int Dt, int Ht, int P, int lamda_fixed, int need_grad, float grad_scale,
        float dropout_p, uint64_t seed,
        const float* x_s, const int64_t* y_s, const float* x_q, const int64_t* y_q, const float* text_s,
        const float* const* w,
        float* loss, int64_t* preds_q, float* lamda_s, float* correct,
        float* const* g_w, float* stats, float* dx_s, float* dx_q, float* g_text);
/* ---- AM3 step on text rows (am3.py:118-126 with text_encoder = 'rand', then :160-200) ---------------------------------------
 * The same step with the text prototypes handed over as rows of the prototype space: tx = text rows, g is not applied,
 * l1 = dropout(relu(tx H0^T + h0)), lamda = sigmoid(l1 H1^T + h1); prototypes, loss, predictions, stats, dx and lamda_fixed as above.
 * Arguments as fumi_hip_am3_step / _dx except:
 *   text_s   [B*S, P] the rows themselves, or NULL: the step draws them, element e = row * P + col is
 *            (float)(mix(key3 ^ (uint32)e) >> 8) * 2^-23 - 1 with mix the 32-bit hash of the dropout masks and key3 the step's key of
 *            tag 3 for `seed` -- uniform on the 2^24-point grid of [-1, 1), exact in fp32, the same bits on every call;
 *   tx_out   [B*S, P] receives the rows the step used (optional when text_s is given, required when it is NULL);
 *   w / g_w  keep the 10-entry layout; entries 2..5 (G0, g0, G1, g1) may be NULL and are never read or written.  Dt is not used.
 * dropout_p > 0 acts in h only, with the mask fumi_hip_am3_step draws for h at the same seed (tag 2, element row * Ht + col).
 * The backward forms gWi, gbi, gH0, gh0, gH1, gh1 (h's as zeros under a fixed lamda) and nothing of g or of the text rows: these
 * forms have no text adjoint and take no g_text. */
int fumi_hip_am3_step_tx(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int D, int Dt, int Ht, int P, int lamda_fixed, int need_grad, float grad_scale,
        float dropout_p, uint64_t seed,
        const float* x_s, const int64_t* y_s, const float* x_q, const int64_t* y_q, const float* text_s,
        const float* const* w,
        float* loss, int64_t* preds_q, float* lamda_s, float* correct,
        float* const* g_w, float* stats, float* tx_out);
int fumi_hip_am3_step_tx_dx(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int D, int Dt, int Ht, int P, int lamda_fixed, int need_grad, float grad_scale,
        float dropout_p, uint64_t seed,
        const float* x_s, const int64_t* y_s, const float* x_q, const int64_t* y_q, const float* text_s,
        const float* const* w,
        float* loss, int64_t* preds_q, float* lamda_s, float* correct,
        float* const* g_w, float* stats, float* tx_out, float* dx_s, float* dx_q);
/* out6 = [loss, accuracy, macro F1, macro precision, macro recall, mean lamda] from `stats` (fumi_hip_am3_step): what
 * AM3.evaluate returns per meta-batch (am3.py:203-212 via sklearn on the host, utils.py:319-326), without leaving the device.
 * N <= 64. */
int fumi_hip_am3_metrics(fumi_ws_t* ws, fumi_stream_t stream, int N, const float* stats, float* out6);
/* Which form the last fumi_hip_am3_step / _dx / _tx / _tx_dx of this process took (csrc/am3.hip, am3_step_impl; DESIGN.md "AM3 form
 * tree"): the first min(n, 12) of  [fast head (1) or generic head (0), waves of the head workgroup, query shares per episode, image-encoder parts the
 * head adds where it reads (1 = none), contraction parts of the image-encoder pass, g forward in the split form, g forward inside
 * the X-panel launch, h forward in the split form, h backward fused, g backward fused, partials of txbar += l1bar H0 handed from h's
 * backward to g's (0 = the GEMM), text form (0 = g applied, 1 = prototype-space rows given, 2 = rows drawn; in forms 1 and 2 the four g
 * entries are 0)].  The backward entries are 0 after a call with need_grad = 0.  Recording changes no launch. */
int fumi_hip_am3_step_plan(int* plan, int n);

/* ---- finer-grained ops (unit parity tests; building blocks of the steps) --------------------------------------- */
/* out[r,:] = mean (mode 0: sum / #non-PAD tokens) or max (mode 1: over ALL L positions) of table[tok[r,l],:]. */
int fumi_hip_glove_bag(fumi_ws_t* ws, fumi_stream_t stream, const int64_t* tok, int R, int L, int64_t pad_id,
        const float* table, int V, int E, int mode, float* out);
/* Fused form for FuMI: out[b,n,:] = bag(tok_s[b, first s with y_s[b,s]==n, :])  -> [B,N,E]  (common.py:23-41 applied to
 * the N class rows that fumi.py:207-210 selects). */
int fumi_hip_glove_bag_select(fumi_ws_t* ws, fumi_stream_t stream, const int64_t* tok_s, const int64_t* y_s,
        int B, int N, int S, int L, int64_t pad_id, const float* table, int V, int E, int mode, float* out);
/* Deferred form: nothing is launched -- the request rides as extra workgroups of the first launch of the next fumi_hip_fumi_step /
 * _indexed of this workspace (or is launched at its start when that step's shapes take another path); `out` [B,N,E] must be the
 * cls_text handed to that step.  fumi_hip_glove_flush launches a pending request on its own. */
int fumi_hip_glove_bag_select_deferred(fumi_ws_t* ws, const int64_t* tok_s, const int64_t* y_s,
        int B, int N, int S, int L, int64_t pad_id, const float* table, int V, int E, int mode, float* out);
int fumi_hip_glove_flush(fumi_ws_t* ws, fumi_stream_t stream);
/* out[b,n,:] = text_s[b, first s with y_s[b,s]==n, :] */
int fumi_hip_class_text_select(fumi_ws_t* ws, fumi_stream_t stream, int B, int N, int S, int Dt,
        const float* text_s, const int64_t* y_s, float* out);
/* The two shared passes over the wide inputs (csrc/xpanel.hip), exported for unit parity tests and tuning:
 *   fwd: A0[B,S+Qn,h0] = [Xs;Xq] W0^T, G[B,S+Qn,S] = [Xs;Xq] Xs^T per episode (support rows first)
 *   bwd: gW0[h0,D] = scale * sum_b Abar[b]^T [Xs_b;Xq_b]   (Abar [B,S+Qn,h0]) */
int fumi_hip_xpanel_fwd(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int D, int h0,
        const float* x_s, const float* x_q, const float* W0, float* A0, float* G);
int fumi_hip_xpanel_bwd(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int D, int h0,
        const float* x_s, const float* x_q, const float* Abar, float scale, float* gW0);
/* The plain multi-segment slab reduction of a step's last launch (csrc/gemm.hip: reduce_multi_kernel), exported for bit-exactness
 * tests: n <= 24 segments, segment k: dst[k][i] = scale * (sum of the even slabs + sum of the odd slabs), slab t = src[k] + t *
 * stride[k], i < count[k], nslab[k] >= 1, each chain in increasing slab index. */
int fumi_hip_reduce_segments(fumi_ws_t* ws, fumi_stream_t stream, int n, const float* const* src, const int* nslab,
        const long* stride, const long* count, float* const* dst, float scale);
/* bwd also takes a one-sided panel: S == 0 (x_s may be NULL) or Qn == 0 (x_q may be NULL), not both.
 * Which kernel form the last fwd / bwd X-panel launch of this process took, up to 12 ints:
 *   [fwd kernel (1 generic guarded, 2 generic fast, 3 fp32 MFMA, 4 per-tile split, 5 pre-split), ring depth, ksplit, Gram column
 *    blocks, rider rode, bwd kernel (1 64x64 guarded, 2 64x64 fast, 3 wide fp32, 4 wide split, 5 narrow swapped split), NB, SK,
 *    nsplit, kchunk, rider rode, where the pre-split fwd form splits its Gram operand (0 another form, 1 planes written by the
 *    pre-split launch, 2 inside the Gram tiles: DESIGN.md section 45)].  Host-side record only: no launch reads it. */
int fumi_hip_xpanel_plan(int* plan, int n);
/* The forward X-panel pass over rows of a table [n_rows, D]: row r of episode b is table[idx_s[b, r]] (r < S) or table[idx_q[b, r - S]]
 * (what the zero-copy sampler passes).  G may be NULL: A0 only, and no Gram tile runs (AM3's image encoder).  An index outside
 * [0, n_rows) sets the workspace status and reads row 0. */
int fumi_hip_xpanel_fwd_rows(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int D, int h0,
        const float* table, int64_t n_rows, const int64_t* idx_s, const int64_t* idx_q, const float* W0, float* A0, float* G);
/* Bytes of bf16 operand planes the last fwd X-panel launch of this process wrote and read (0: a form without planes). */
size_t fumi_hip_xpanel_planes_bytes(void);
/* The plan of the episode chain (csrc/episode.hip: plan_episodes; DESIGN.md sections 29 and 40) of the last FuMI / MAML step of this
 * process that ran the chain, up to 18 ints:
 *   [adapt form (0 none: the inner step runs inside the fused query kernel, 1 LDS-resident, 2 generic), adapt column parts AP,
 *    query form (0 fused fixed-shape, 1 fused, 2 LDS-resident, 3 generic), reverse form (0 LDS-resident fixed-shape, 1 LDS-resident,
 *    2 generic), reverse column parts P, backward X-panel pass in two launches (0 / 1), slabs of its query-row part, slabs of its
 *    support-row part, inner-loop dropout (0 / 1), what fumi_hip_epi_fixed_last reports, floats of LDS of the query layout, of the
 *    adapt layout, of the reverse layout, staging units of the adapt table, the query table, the fused query table, the reverse
 *    sweep's first table, its per-step table].
 * An entry that belongs to a form the plan did not take is 0.  Host-side record only: no launch reads it. */
int fumi_hip_epi_plan(int* plan, int n);
/* The same entries for a shape: host arithmetic only -- no workspace, no HIP call, runs without a GPU.  `dropout`: inner-loop
 * dropout on (1) or off (0).  `flags` states what the shape cannot: FUMI_EPI_Q_HEAD the caller passes an initial head (every entry
 * point of this header does), _SIDE the workspace has its second stream and fork / join events, _PROFILING phase timing is on,
 * _AFTER_REVERSE the caller asks for an event after the reverse sweep (FUMI_OVERLAP bit 1); bit _W_OFF_SHIFT + i (_B_OFF_SHIFT + i):
 * the weight (bias) of hidden layer i starts one float past a 16-byte boundary.  The environment knobs are the process's own. */
#define FUMI_EPI_Q_HEAD 1
#define FUMI_EPI_Q_SIDE 2
#define FUMI_EPI_Q_PROFILING 4
#define FUMI_EPI_Q_AFTER_REVERSE 8
#define FUMI_EPI_Q_W_OFF_SHIFT 8
#define FUMI_EPI_Q_B_OFF_SHIFT 16
int fumi_hip_epi_plan_query(int B, int N, int S, int Qn, int D, int n_hidden, const int* hid, int T, int need_grad,
        int second_order, int dropout, int flags, int* plan, int n);
/* What the hypernetwork (hyper_net = Linear -> ReLU -> Linear [-> Tanh], csrc/hyper.hip) of the last
 * fumi_hip_fumi_step* of this process took, up to 7 ints:
 *   [forward form (0 plain GEMMs, 1 one launch per layer, 2 one launch with a workgroup per row block, 3 one launch with layer 0's
 *    columns split over workgroups, 4 that split form riding in the per-tile split forward X-panel launch, 5 riding in the pre-split
 *    one), instance of the form (register steps KS 20 / 48 / 24 for 3, 4, 5; 10 NT + NCH for 2; the column chunk of layer 0 for 1;
 *    else 0), 16-row blocks, 64-column hidden chunks (0: the hidden width is no multiple of 64), backward form (0 none: no gradients
 *    asked for, 1 plain GEMMs, 2 two launches, 3 one launch, 4 that launch riding in the backward X-panel launch), passes over the
 *    text width of the layer-0 weight slab (forms 3, 4; else 0), text gradient (0 none, 1 a GEMM after the backward's own launches,
 *    2 inside the plain-GEMM backward)].
 * Host-side record only: no launch reads it. */
int fumi_hip_hyper_plan(int* plan, int n);
/* The same entries for a shape: host arithmetic only -- no workspace, no HIP call, runs without a GPU; it asks the predicates the
 * launch path asks.  `flags`: FUMI_HYPER_Q_SIDE the workspace has its second stream (FUMI_OVERLAP then moves the hypernetwork
 * there), _TEXT_GRAD the caller passes g_cls_text, _CLS_TEXT_OFF the class text rows start one float past a 16-byte boundary,
 * bit _PHI_OFF_SHIFT + i: phi[i] does.  The X-panel operands and every workspace array count as aligned; the environment knobs
 * are the process's own. */
#define FUMI_HYPER_Q_SIDE 1
#define FUMI_HYPER_Q_TEXT_GRAD 2
#define FUMI_HYPER_Q_CLS_TEXT_OFF 4
#define FUMI_HYPER_Q_PHI_OFF_SHIFT 8
int fumi_hip_hyper_plan_query(int B, int N, int S, int Qn, int D, int n_hidden, const int* hid, int Dt, int Ht, int T, int need_grad,
        int flags, int* plan, int n);
/* One fused launch of torch.optim.Adam's update (coupled L2 weight decay, bias correction; fumi/utils/utils.py:280-283) for
 * up to 32 tensors.  Pointer/size arrays are HOST arrays; `step` is the 1-based step count. */
int fumi_hip_adam_step(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, float* const* params,
        const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const long* numel,
        float lr, float beta1, float beta2, float eps, float weight_decay, int step);
/* Deferred form: nothing is launched -- the update (same arithmetic, same order: bit-identical parameters) is folded into the
 * LAST launch of the next fumi_hip_fumi_step / _indexed of this workspace, whose final reduction produces every gradient element:
 * `optimizer.step()` (fumi/models/fumi.py:193) costs no launch of its own.  Single GPU only (with several ranks the all-reduce
 * lies between gradient and update).  fumi_hip_adam_flush launches a still pending step as the ordinary kernel (*launched = 1)
 * or reports that a meta-step had folded it (*launched = 0). */
int fumi_hip_adam_step_deferred(fumi_ws_t* ws, int n_tensors, float* const* params,
        const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const long* numel,
        float lr, float beta1, float beta2, float eps, float weight_decay, int step);
int fumi_hip_adam_flush(fumi_ws_t* ws, fumi_stream_t stream, int* launched);
/* The reference's other outer optimizers (fumi/utils/utils.py:284-299) on the same fused launch, each in the operation order of
 * torch's single-tensor implementation.  AdamW = torch.optim.AdamW: every parameter shrinks by 1 - lr * weight_decay first, then
 * Adam's moments and update on the raw gradient (no coupled L2 term); arguments as fumi_hip_adam_step, except that the betas are
 * doubles: torch folds 1 - beta in Python floats, and 1 - 0.999f is off by 1.3e-5 of 0.001.  `lr` is a per-call scalar: a schedule
 * may change it on every step, also in the deferred form. */
int fumi_hip_adamw_step(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, float* const* params,
        const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const long* numel,
        float lr, double beta1, double beta2, float eps, float weight_decay, int step);
/* SGD = torch.optim.SGD(lr, momentum, weight_decay) with dampening 0 and no Nesterov: g += wd * p; buf = g when first_step != 0
 * (the step that creates the momentum buffers: they are written, not read), else buf = momentum * buf + g; p -= lr * buf.
 * momentum == 0: there is no buffer, momentum_buf may be NULL and p -= lr * g.  Up to 32 tensors, HOST pointer/size arrays. */
int fumi_hip_sgd_step(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, float* const* params,
        const float* const* grads, float* const* momentum_buf, const long* numel,
        float lr, float momentum, float weight_decay, int first_step);
/* Their deferred forms, as fumi_hip_adam_step_deferred: folded into the last launch of the next meta-step of this workspace
 * (bit-identical to the immediate form), or launched by fumi_hip_adam_flush, which flushes a pending step of ANY rule.  One step
 * may be pending per workspace; a later registration replaces an earlier one that was never launched. */
int fumi_hip_adamw_step_deferred(fumi_ws_t* ws, int n_tensors, float* const* params,
        const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const long* numel,
        float lr, double beta1, double beta2, float eps, float weight_decay, int step);
int fumi_hip_sgd_step_deferred(fumi_ws_t* ws, int n_tensors, float* const* params,
        const float* const* grads, float* const* momentum_buf, const long* numel,
        float lr, float momentum, float weight_decay, int first_step);
/* The global L2 norm of up to 256 gradient tensors, as torch.nn.utils.clip_grad_norm_ forms it (norm_type 2): squares summed in
 * double in a fixed order (one partial per workgroup in a buffer the workspace owns, added in index order by a second launch; no
 * floating-point atomics: equal inputs give equal bits), *norm_out = (float)sqrt(sum).  norm_out is a DEVICE float; grads / numel
 * are HOST arrays.  A tensor of no elements may have a NULL pointer. */
int fumi_hip_grad_norm(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, const float* const* grads, const long* numel,
        float* norm_out);
/* Clipped forms of the three steps: clip_grad_norm_(params, max_norm) followed by the rule, without leaving the device and
 * without writing the gradients -- the norm as above, coef = min(1, max_norm / (norm + 1e-6)) in fp32 (a NaN norm gives a NaN
 * coef, an infinite one 0), then the rule on g * coef (one rounded fp32 multiply per element: the parameters and state are bit
 * for bit those of the unclipped entry point on gradients scaled by coef).  Arguments as the unclipped sibling, then max_norm
 * (finite and > 0, else FUMI_EINVAL) and clip_out, a DEVICE buffer of two floats that receives {norm, coef} (required).  Up to
 * 256 tensors (FUMI_ENOTSUP beyond), walked in chunks of 32: separate launches ordered by the stream alone.  There is no deferred
 * form: the norm needs every gradient element before the first update. */
int fumi_hip_adam_step_clipped(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, float* const* params,
        const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const long* numel,
        float lr, float beta1, float beta2, float eps, float weight_decay, int step, float max_norm, float* clip_out);
int fumi_hip_adamw_step_clipped(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, float* const* params,
        const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const long* numel,
        float lr, double beta1, double beta2, float eps, float weight_decay, int step, float max_norm, float* clip_out);
int fumi_hip_sgd_step_clipped(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, float* const* params,
        const float* const* grads, float* const* momentum_buf, const long* numel,
        float lr, float momentum, float weight_decay, int first_step, float max_norm, float* clip_out);
/* y[M,N] = act(x[M,K] W[N,K]^T + b[N]);  act: 0 none, 1 relu, 2 tanh.  b may be NULL. */
int fumi_hip_linear_fwd(fumi_ws_t* ws, fumi_stream_t stream, int M, int N, int K,
        const float* x, const float* W, const float* b, int act, float* y);
/* dx[M,K] = dy[M,N] W[N,K] */
int fumi_hip_linear_bwd_data(fumi_ws_t* ws, fumi_stream_t stream, int M, int N, int K,
        const float* dy, const float* W, float* dx);
/* dW[N,K] = dy[M,N]^T x[M,K];  db[N] = colsum(dy) (db may be NULL) */
int fumi_hip_linear_bwd_weight(fumi_ws_t* ws, fumi_stream_t stream, int M, int N, int K,
        const float* dy, const float* x, float* dW, float* db);


/* ---- Conv4 image encoder at the im_net seam ---------------------------------------------------------------------------
 * The reference adapts an MLP over pre-computed embeddings; `im_net` is "any module with forward(x, params) and
 * meta_named_parameters()" (fumi/models/fumi.py:89-100, `--im_encoder resnet` is a TODO at fumi/models/am3.py:41-46).
 * BASELINE.json words its configurations with a Conv4 encoder on 84x84 images: nblk blocks of conv3x3(64, pad 1, no bias) .
 * BatchNorm2d with BATCH statistics (training and evaluation alike) . ReLU . MaxPool2d(2), flattened like PyTorch's
 * x.view(M, -1) of NCHW.  PARITY UNPINNED for the convolutional part (nothing to import); oracle = oracle/conv4_ref.py.
 * Everything after the feature vector is the reference's algorithm (fumi.py:146-192 / maml.py:156-191).
 *   x_s [B,S,Cin,H,W], x_q [B,Qn,Cin,H,W] fp32 NCHW (Cin <= 3);  theta: 3*nblk pointers  W_l [64,Cin|64,3,3], BN weight [64],
 *   BN bias [64];  F = fumi_hip_conv4_feature_dim(nblk, H, W) = 64 * (H >> nblk) * (W >> nblk).
 *   fumi: phi = A0 [Ht,Dt], a0, A1 [F+1,Ht], a1 [F+1];  maml: params = theta then lin_final W [N,F], b [N].
 * Outputs / gradient conventions as fumi_hip_fumi_step / fumi_hip_maml_step.  Second order needs T <= 8 taped inner steps. */
int fumi_hip_conv4_feature_dim(int nblk, int H, int W);
/* Process-wide switches of the Conv4 path.  key 0: 1 (default) = block 1 recomputed band by band from the image, its 64-channel
 * full-resolution maps never stored (csrc/conv_first.hip); 0 = every block through the plain passes (what the probe tests read).
 * key 1: lanes -- parts of the meta-batch on concurrent streams of the workspace -- of the Conv4 meta-steps and encoder calls:
 * 0 (default) = the library's choice (up to 3 from 8 episodes; 2 for the encoder calls), 1 = one stream, n <= 4 = at most n. */
int fumi_hip_conv4_set_option(int key, int value);
int fumi_hip_fumi_conv4_step(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int Cin, int H, int W, int nblk, int Dt, int Ht,
        int T, float alpha, int tanh_head, int need_grad, float grad_scale,
        const float* x_s, const int64_t* y_s, const float* x_q, const int64_t* y_q,
        const float* cls_text, const float* text_s,
        const float* const* theta, const float* const* phi,
        float* logits_q, int64_t* preds_q, float* preds_q_f32, float* loss_b, float* acc_b, float* stats,
        float* const* g_theta, float* const* g_phi, float* g_cls_text);
int fumi_hip_maml_conv4_step(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int Cin, int H, int W, int nblk,
        int T, float alpha, int first_order, int need_grad, float grad_scale,
        const float* x_s, const int64_t* y_s, const float* x_q, const int64_t* y_q,
        const float* const* params,
        float* logits_q, int64_t* preds_q, float* preds_q_f32, float* loss_b, float* acc_b, float* stats,
        float* const* g_params);
/* Forward only: feats [G*M, F] = Conv4(x [G,M,Cin,H,W]); batch statistics per group of M images (one support or query set). */
int fumi_hip_conv4_features(fumi_ws_t* ws, fumi_stream_t stream, int G, int M, int Cin, int H, int W, int nblk,
        const float* x, const float* const* theta, float* feats);
/* Conv4 as the image encoder in front of a step that lays out its own workspace (AM3 at the seam am3.py:41-46; "parity
 * unpinned" like the rest of the Conv4 rows).  encode: feats_s [B,S,F], feats_q [B,Qn,F]; every episode's support set and query
 * set is one batch-statistics group.  keep_tape = 1 leaves the activations laid out in `ws`; encode_bwd (same shapes, same `ws`,
 * no other call on `ws` in between -- give the encoder its own workspace) walks them backwards from the feature adjoints:
 * g_theta (3 nblk pointers, torch layouts) = scale * sum over episodes of d<dfeats, feats>/dtheta.  FUMI_EINVAL without a tape. */
int fumi_hip_conv4_encode(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int Cin, int H, int W, int nblk,
        const float* x_s, const float* x_q, const float* const* theta, float* feats_s, float* feats_q, int keep_tape);
int fumi_hip_conv4_encode_bwd(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int Cin, int H, int W, int nblk,
        const float* x_s, const float* x_q, const float* dfeats_s, const float* dfeats_q, float scale, float* const* g_theta);
/* Test hook: copies one intermediate tensor of the LAST conv4 step of this process out of the workspace (layouts:
 * fumi_amd/csrc/conv4.hip, fumi_hip_conv4_probe).  *n_out = its size in floats; at most max_floats are copied. */
int fumi_hip_conv4_probe(fumi_ws_t* ws, fumi_stream_t stream, int pass, int kind, int block, float* out, size_t max_floats,
        size_t* n_out);
/* ---- ResNet-12 image encoder in bf16 at the im_net seam (fumi/models/fumi.py:89-100; BASELINE.json configs[4]) ----------------------
 * Four residual blocks  a1 = lrelu(BN(conv3x3(x))), a2 = lrelu(BN(conv3x3(a1))), out = maxpool2(lrelu(BN(conv3x3(a2)) + BN(conv1x1(x))))
 * with `channels[l]` output channels (multiples of 32), LeakyReLU slope 0.1, batch statistics, no conv bias; features = global
 * average pool of the last block ([rows, channels[nblk-1]]).  Images x_s [B,S,Cin,H,W], x_q [B,Qn,Cin,H,W] fp32; theta = 12 tensors
 * per block: W1 [C,Cin|C_prev,3,3], g1, b1, W2 [C,C,3,3], g2, b2, W3, g3, b3, Ws [C,Cin|C_prev,1,1], gs, bs (fp32 masters; every
 * matrix product runs in bf16 with fp32 accumulation, maps are stored in bf16).  Second-order outer gradient (fumi.py:176);
 * the reference has no such encoder: "parity unpinned", oracle = oracle/resnet12_manual.py / resnet12_ref.py.
 * `chunk`: episodes processed per pass over the tape (0 = derived from the workspace budget, fumi_hip_resnet12_set_budget /
 * FUMI_RN12_BUDGET_GB, default 200 GB): the meta-gradient is the sum over chunks. */
int fumi_hip_resnet12_set_budget(double gigabytes);
/* Test hooks of the ResNet-12 steps (no reference counterpart: the reference keeps every intermediate in autograd's graph).
 * set_option key 0: probe mode on / off -- one lane; a step whose meta-batch is a single chunk keeps its buffer table, the gradient
 * of every inner step and the direction of the last Hessian-vector product;  key 1: the reverse sweep stops after inner step `value`
 * (0 = whole sweep), so that the tangent maps of that step can be read.
 * fumi_hip_rn12_probe copies one stored intermediate of the last such step (tests/test_resnet12_probe.py compares every stage of the
 * sweep with oracle/resnet12_manual.py on the engine's own upstream maps).  pass 0..T-1: tape of support step `pass`; T: query pass;
 * T+1: tangent maps of the last Hessian-vector product; -1: parameter space.  kind, pass >= 0: 0 u[block][idx], 1 a[block][idx],
 * 2 out[block], 3 du[block][idx], 4 da[block][idx], 5 dout[block] (bf16 padded channels-last [B][M (H+2)(W+2)][C]), 6 coef[block][idx]
 * fp32 [B][13][C] (mu, r, A, C0, D1, D2, TB, TC, M1, M2, K0, DD1, E12), 7 f, 8 df [B][M][F], 9 z, 10 p, 11 dz [B][M][N] fp32.
 * kind, pass -1: 0 parameter slot idx [B][PSZ], 1 head slot idx, 2 G / 3 dh of inner step idx, 4 bar, 5 bar_h, 6 HV, 7 HV_h, 8 V, 9 V_h,
 * 10 / 11 prepared support / query images (bf16, 16 channels).  *n_bytes: size; *is_bf16: element type; copies min(size, max_bytes). */
int fumi_hip_resnet12_set_option(int key, int value);
int fumi_hip_rn12_probe(fumi_ws_t* ws, fumi_stream_t stream, int pass, int kind, int block, int idx, void* out, size_t max_bytes,
        size_t* n_bytes, int* is_bf16);
int fumi_hip_fumi_resnet12_step(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int Cin, int H, int W, int nblk, const int* channels, int Dt, int Ht,
        int T, float alpha, int tanh_head, int need_grad, float grad_scale, int chunk,
        const float* x_s, const int64_t* y_s, const float* x_q, const int64_t* y_q,
        const float* cls_text, const float* text_s,
        const float* const* theta, const float* const* phi,
        float* logits_q, int64_t* preds_q, float* preds_q_f32, float* loss_b, float* acc_b, float* stats,
        float* const* g_theta, float* const* g_phi, float* g_cls_text);
int fumi_hip_maml_resnet12_step(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int Cin, int H, int W, int nblk, const int* channels,
        int T, float alpha, int first_order, int need_grad, float grad_scale, int chunk,
        const float* x_s, const int64_t* y_s, const float* x_q, const int64_t* y_q,
        const float* const* params,
        float* logits_q, int64_t* preds_q, float* preds_q_f32, float* loss_b, float* acc_b, float* stats,
        float* const* g_params);
/* Forward only: feats [G*M, channels[nblk-1]] fp32; batch statistics per group of M images. */
int fumi_hip_resnet12_features(fumi_ws_t* ws, fumi_stream_t stream, int G, int M, int Cin, int H, int W, int nblk, const int* channels,
        const float* x, const float* const* theta, float* feats);
/* ResNet-12 as the image encoder in front of a step that lays out its own workspace (AM3 at the seam am3.py:41-46; "parity
 * unpinned" like the other ResNet-12 rows).  encode: feats_s [B,S,F], feats_q [B,Qn,F] with F = channels[nblk-1]; every episode's
 * support set and query set is one batch-statistics group; theta in the order above.  keep_tape = 1 leaves in `ws` what the
 * backward needs, theta's parameter / fragment slab included; encode_bwd (same shapes, same `ws`, no other call on `ws` in between
 * -- give the encoder its own workspace) consumes it: g_theta (12 nblk pointers, torch layouts) = scale * sum over episodes of
 * d(<dfeats_s, feats_s> + <dfeats_q, feats_q>)/dtheta.  FUMI_EINVAL without a tape of these shapes.  Two forms, chosen from the
 * workspace budget (fumi_hip_resnet12_set_budget): TAPED (the forward maps of the whole meta-batch stay resident, encode_bwd runs
 * the backward only) when they fit, else RECOMPUTE (encode_bwd runs each chunk's forward again); both give bit-identical results. */
int fumi_hip_resnet12_encode(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int Cin, int H, int W,
        int nblk, const int* channels, const float* x_s, const float* x_q, const float* const* theta,
        float* feats_s, float* feats_q, int keep_tape);
int fumi_hip_resnet12_encode_bwd(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int Cin, int H, int W,
        int nblk, const int* channels, const float* x_s, const float* x_q, const float* dfeats_s,
        const float* dfeats_q, float scale, float* const* g_theta);
/* The pair with DropBlock / dropout on every block's pooled output (the MetaOptNet / RFS ResNet-12; fumi_amd/csrc/rn12_drop.hip).
 * Arguments as above, then drop_rate [nblk] (each in [0, 1); 0: the block launches nothing), drop_block [nblk] (1: element-wise
 * dropout; 2..8: DropBlock with block size min(drop_block, H_l, W_l) on the block's pooled H_l x W_l map, which must then be at most
 * 64 x 64) and the step's 64-bit seed (host pointers / values; nothing is armed on the workspace).  The mask is a pure function of
 * (seed, block, support / query, GLOBAL episode, image, channel, position), regenerated wherever it is needed and never stored; the
 * kept cells are rescaled by total / kept counted per batch-statistics group (one episode's support or query set).  Both forms and
 * every chunking give the same bits.  The tape records the three arguments: encode_bwd_drop returns FUMI_EINVAL when its own differ
 * (the tape stays).  With every rate 0 the launches and bits are those of the pair above. */
int fumi_hip_resnet12_encode_drop(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int Cin, int H, int W,
        int nblk, const int* channels, const float* x_s, const float* x_q, const float* const* theta,
        float* feats_s, float* feats_q, int keep_tape, const float* drop_rate, const int* drop_block, uint64_t drop_seed);
int fumi_hip_resnet12_encode_bwd_drop(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int Cin, int H, int W,
        int nblk, const int* channels, const float* x_s, const float* x_q, const float* dfeats_s,
        const float* dfeats_q, float scale, float* const* g_theta, const float* drop_rate, const int* drop_block, uint64_t drop_seed);
/* The two drop launches on one raw map (unit parity): map [B][M (H+2)(W+2)][C] bf16 is scaled in place, kept_out [B] int64 and
 * scale_out [B] fp32 (device) receive each group's kept count and total / kept (0 when nothing is kept).  block_index, set (0 | 1)
 * and b0 (global index of the map's first episode) enter the mask as in the pair above.  FUMI_EINVAL (nothing launched): rate
 * outside [0, 1), block outside 1..8, block > 1 with H or W beyond 64. */
int fumi_hip_rn12_drop_apply(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int C, float rate, int block,
        uint64_t seed, int block_index, int set, int b0, void* map_in_out, int64_t* kept_out, float* scale_out);
/* Plan of the last fumi_hip_resnet12_encode: *taped = 1 (taped form) or 0 (recompute form), *chunk = episodes per chunk,
 * *lanes = streams the chunks were spread over. */
int fumi_hip_resnet12_encode_plan(int* taped, int* chunk, int* lanes);
/* The matrix kernels on raw maps (unit parity tests): x, y, dy are bf16 "padded channels-last" [B][M (H+2)(W+2)][C] with zero
 * borders, Wt / dW fp32 [B][Cout][Cin][k][k] (k = 3: ntaps 9, pad 1; k = 1: ntaps 1).  transpose != 0: the input-gradient
 * product (x has Cout channels, y has Cin).  stats (optional) [B][2][C_y]: per-channel sum and sum of squares of the stored y. */
int fumi_hip_rn12_conv(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int Cin, int Cout, int ntaps, int transpose,
        const void* x, const float* Wt, void* y, float* stats);
int fumi_hip_rn12_wgrad(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int Cin, int Cout, int ntaps,
        const void* x, const void* dy, float* dW);
/* The general forms (every launch the engine issues; tests/rn12_conv_forms.py).  conv_multi: y = sum over nsrc (1..4) sources of
 * conv_{ntaps[s]}(x[s], Wt[s]); source s has Cin[s] channels and x_stride[s] elements between episodes (>= the map: the gap is never
 * read); Wt[s] fp32 OIHW [Cout][Cin[s]][k][k], with transpose != 0 the forward layer's [Cin[s]][Cout][k][k]; w_stride[s] = 0 shares
 * one weight set over the episodes.  dot (optional): the second statistic is sum(y * dot).  y is NOT cleared (interior pixels are
 * written).  wgrad_multi: npair = 1 | 2 (x, dy) pairs are added; the maps have Cin >= Cin_real channels, dW is
 * [B][Cout][Cin_real][k][k] with dw_stride elements between episodes; nsplit = 0: the launcher's own split of the pixel axis.
 * FUMI_EINVAL (nothing launched): Cout % 32, Cin % 16, nsrc outside 1..4, ntaps not 1 | 9, npair outside 1..2, a stride shorter
 * than its map. */
int fumi_hip_rn12_conv_multi(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int Cout, int nsrc, const int* Cin,
        const int* ntaps, const void* const* x, const long long* x_stride, const float* const* Wt, const long long* w_stride,
        int transpose, const void* dot, long long dot_stride, void* y, long long y_stride, float* stats);
int fumi_hip_rn12_wgrad_multi(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int Cin, int Cin_real, int Cout, int ntaps,
        int npair, int nsplit, const void* x0, const void* dy0, const void* x1, const void* dy1, long long x_stride, long long dy_stride,
        float* dW, long long dw_stride);
/* What the last convolution launch and the last weight-gradient launch (+ reduce) of this process decided -- a host-side record
 * written beside the launches, never read by one: plan[0..10] = NF, MW, BKS, S16, tiles per episode, tiles per image (0: flat tiles),
 * column groups, XCD-grouped ids, LDS-direct slab loads, slab rows, LDS bytes; plan[11..16] = NTAP, nsplit, ci tiles, co tiles,
 * XCD-grouped ids, reduce kernel (1 rows, 2 four-way split, 3 nine-tap).  The two queries return the same decisions for a shape
 * without any HIP call (conv: plan[0..10]; wgrad: plan[0..5] = entries 11..16; nsplit = 0: the launcher's own split). */
int fumi_hip_rn12_conv_plan(int* plan, int n);
int fumi_hip_rn12_conv_query(int B, int M, int H, int W, int Cout, int nsrc, const int* Cin, int* plan, int n);
int fumi_hip_rn12_wgrad_query(int B, int M, int H, int W, int Cin, int Cout, int ntaps, int npair, int nsplit, int* plan, int n);
/* The element-wise passes between the convolutions on raw buffers (unit parity; tests/rn12_ew_forms.py): every
 * launcher as the engine calls it.  Maps are bf16 [B][M (H+2)(W+2)][C] padded channels-last, C a multiple of 8 up to 2048; a
 * coefficient table is fp32 [B][13][C] (fields MU, R, A, C0, D1, D2, TB, TC, M1, M2, K0, DD1, E12); partial sums are fp32
 * [B][nt][K][C] with nt of the query below.  act: out = lrelu(A u + C0), with ud its tangent.  bwd: apply = 0 the partial sums
 * (K = 2, tangent 3), apply = 1 du.  join: pass_ 0 the pooled map out0 [B][M (H/2+2)(W/2+2)][C], 1 the partial sums (K = 3, tangent 5),
 * 2 du3 -> out0 and dus -> out1; form = 1 runs the plain pass 2 on the one-cell-per-thread kernel the tangent pass takes.  coef: the
 * coefficient pass in mode 0 FWD (part slices k0 = sum, k1 = sum of squares; g, beta with pstride floats between episodes), 1 BWD
 * (D1, D2; dbeta = slice k0, dg = slice k1, gstride), 2 TFWD (gd, betad, dstride), 3 TBWD (slices k0, k1 + k2; gd, dg, dbeta); n =
 * interior pixels per channel; scratch (optional, B ceil(nt / 64) K C floats): lists beyond 128 slabs are first added in groups of 64.
 * avgpool: adjoint = 0 out fp32 [BM][C] = interior mean of in; 1 out bf16 map = in fp32 [BM][C] / (H W).  img_prep: img fp32
 * [BM][Cin][H][W] -> out bf16 [BM][(H+2)(W+2)][16].  Refusals, before anything is launched: FUMI_EINVAL for a missing buffer, C % 8,
 * a join of a map below 2 x 2, Cin outside 1..8, a slice outside K, a stride below C; FUMI_ENOTSUP for C above 2048 and for index
 * ranges beyond 32 bits. */
int fumi_hip_rn12_ew_act(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int C, const void* u, const void* ud,
        const float* coef, void* out);
int fumi_hip_rn12_ew_bwd(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int C, int apply, int tangent, const void* u,
        const void* ud, const void* da, const void* dad, const float* coef, void* out);
int fumi_hip_rn12_ew_join(fumi_ws_t* ws, fumi_stream_t stream, int B, int M, int H, int W, int C, int pass_, int tangent, int form,
        const void* u3, const void* us, const void* u3d, const void* usd, const float* coef3, const float* coefs, const void* dout,
        const void* doutd, void* out0, void* out1);
int fumi_hip_rn12_ew_coef(fumi_ws_t* ws, fumi_stream_t stream, int B, int C, int mode, int nt, int K, int k0, int k1, int k2, float n,
        const float* part, float* coef, const float* g, const float* beta, long long pstride, const float* gd, const float* betad,
        long long dstride, float* dg, float* dbeta, long long gstride, float* scratch);
int fumi_hip_rn12_ew_avgpool(fumi_ws_t* ws, fumi_stream_t stream, int BM, int H, int W, int C, int adjoint, const void* in, void* out);
int fumi_hip_rn12_ew_img_prep(fumi_ws_t* ws, fumi_stream_t stream, int BM, int Cin, int H, int W, const float* img, void* out);
/* What an element-wise launch decides from its shape -- host arithmetic only, no HIP call (the launchers launch what it returns).
 * kind: 0 act, 1 bwd reduce, 2 bwd apply, 3 join fwd, 4 join reduce, 5 join apply, 6 avgpool, 7 its adjoint, 8 image prep (6..8: B M
 * images; 8: C is the image's channel count).  plan[0..16] = 8-channel chunks nch, pixel groups nrg, active threads, unit (1: one unit
 * of work per thread), pixels per reduction workgroup rb, slabs per episode nt, pixels per workgroup of a walking map pass, join
 * windows per workgroup, cells per image ncy, ncx, cells per workgroup, cell (1: one cell per thread), first (1: the coefficient
 * pass behind the reduction adds groups of 64 slabs first), slabs nt2 that reach the coefficient kernel, dynamic LDS bytes, grid x, y.
 * ew_plan: the same record of the last launch of this process (the coefficient launcher updates first and nt2 only).  coef_query:
 * plan[0..6] = first, nt2, the first stage's grid x, y (0: none), the coefficient kernel's grid x, y, floats of scratch. */
int fumi_hip_rn12_ew_query(int B, int M, int H, int W, int C, int kind, int tangent, int form, int* plan, int n);
int fumi_hip_rn12_ew_plan(int* plan, int n);
int fumi_hip_rn12_coef_query(int B, int nt, int K, int C, int has_scratch, int* plan, int n);
/* The three 3x3 / pad 1 / stride 1 convolution products on 64 -> 64 channels (the set is closed under differentiation: the
 * second-order sweep uses nothing else).  Dense channels-last tensors x, y, dy [M,H,W,64]; weights W, dW [64,64,3,3] (OIHW). */
int fumi_hip_conv3x3_fwd(fumi_ws_t* ws, fumi_stream_t stream, int M, int H, int W, const float* x, const float* Wt, float* y);
int fumi_hip_conv3x3_bwd_data(fumi_ws_t* ws, fumi_stream_t stream, int M, int H, int W, const float* dy, const float* Wt, float* dx);
int fumi_hip_conv3x3_bwd_weight(fumi_ws_t* ws, fumi_stream_t stream, int M, int H, int W, const float* x, const float* dy, float* dW);
/* torchmeta gradient_update_parameters / the reference's in-place `hyper_params -= step_size * grad` (fumi.py:165-176):
 * out[i] = p[i] - step_size * g[i], n floats (out may alias p). */
int fumi_hip_sgd_axpy(fumi_ws_t* ws, fumi_stream_t stream, long n, const float* p, float step_size, const float* g, float* out);
/* F.cross_entropy forward + backward of M rows of N logits (fumi.py:162,182): loss [1] = mean NLL, dz [M,N] = (softmax - onehot)/M,
 * preds [M] = first arg-max (fumi.py:180).  A label outside [0,N) sets FUMI_ST_LABEL_RANGE. */
int fumi_hip_ce_fwd_bwd(fumi_ws_t* ws, fumi_stream_t stream, int M, int N, const float* z, const int64_t* y, float* loss, float* dz,
        int64_t* preds);
/* get_prototypes (fumi/utils/utils.py:331-376): out[b,n,:] = sum_{s: y[b,s]==n} x[b,s,:] / max(count, 1)  -> [B,N,P] */
int fumi_hip_proto_reduce(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int N, int P, const float* x, const int64_t* y, float* out);
/* ---- The classification heads of --model pretrain (fumi_hip_cls_head_step ... fumi_hip_cos_cls_head_step; shared code in
 * csrc/cls_head.h) ----
 * PREDICTIONS, for all four: preds is the first arg-max, as torch.max gives it; a row of NaNs predicts class 0.
 * LABELS, for all four: a label outside [0,C), in y_a or y_b, sets FUMI_ST_LABEL_RANGE; that row adds nothing to any loss, count or
 * gradient while the divisor stays M.
 * ORDER, for all four: every sum has a fixed order and there are no floating-point atomics, so two calls on the same inputs give the
 * same bits.
 * SHAPES, for all four: 1 <= M <= 4096, F % 32 == 0, 32 <= F <= 2048, 2 <= C <= 1024: FUMI_ENOTSUP / FUMI_EINVAL otherwise, before any
 * launch.  Each entry says below only what is its own. */
/* The classification head of supervised pre-training (csrc/clshead.hip), fused: F.cross_entropy(feats W^T + b, y)
 * with mean reduction over the M rows and its backward, in two launches.  feats [M,F], y [M], W [C,F], b [C];  loss [1] = mean NLL,
 * correct [1] = number of rows whose first arg-max equals the label (float), preds [M] = first arg-max (may be NULL);
 * dfeats [M,F], gW [C,F], gb [C] = gradients of grad_scale * loss (written, not accumulated) -- all three given (training form) or all
 * three NULL (forward form: loss, correct and preds are bit-identical to the training form's).  fp32 with fp32 accumulation on
 * v_mfma_f32_16x16x4_f32; the logits of a 16-row tile stay in LDS from the product through the softmax to dlogits and dfeats =
 * dlogits W, only dlogits goes to memory (workspace) for gW = dlogits^T feats and gb = colsum(dlogits).  Predictions,
 * labels, order and shapes: the common contract above. */
int fumi_hip_cls_head_step(fumi_ws_t* ws, fumi_stream_t stream, int M, int F, int C,
        const float* feats, const int64_t* y, const float* W, const float* b, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* dfeats, float* gW, float* gb);
/* The same head against a soft target: label smoothing `smoothing` = eps and a mix of two labels per row, what
 * mixup and CutMix train on.  With u = 1 - lam computed in fp32,
 *     t[m,c] = (1 - eps) * (lam * [c == y_a[m]] + u * [c == y_b[m]]) + eps / C
 *     loss = mean_m (lse_m - sum_c t[m,c] z[m,c]),   dlogits = grad_scale / M * (softmax - t);
 * dfeats, gW, gb follow from dlogits as above, correct counts the rows whose first arg-max equals y_a, preds is unchanged.
 * y_b == NULL means y_b = y_a (label smoothing alone; lam must be 1).  The same two launches, LDS image, shapes, fixed summation
 * orders and forward form as fumi_hip_cls_head_step; sum_c z[m,c] (needed for eps > 0) is formed by the strided loop and butterfly of
 * the log-sum-exp.  With y_b == NULL, lam = 1, smoothing = 0 all six outputs are bit-identical to fumi_hip_cls_head_step.
 * Labels: the common contract above, for y_a and y_b.
 * FUMI_EINVAL before any launch: smoothing outside [0, 1), lam outside [0, 1], y_b == NULL with lam != 1. */
int fumi_hip_cls_head_step_soft(fumi_ws_t* ws, fumi_stream_t stream, int M, int F, int C,
        const float* feats, const int64_t* y_a, const int64_t* y_b, float lam, float smoothing,
        const float* W, const float* b, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* dfeats, float* gW, float* gb);
/* The same head as the student of a frozen teacher: knowledge distillation beside the soft target of the entry
 * above.  feats_t [M,F], W_t [C,F], b_t [C] are the teacher's features and classifier; with T = kd_temp, z_t = feats_t W_t^T + b_t,
 * p = softmax(z_t / T), q = softmax(z / T) and t the soft target,
 *     loss_ce = mean_m (lse(z_m) - sum_c t z),   loss_kd = T^2 mean_m KL(p || q),
 *     loss = ce_weight * loss_ce + kd_alpha * loss_kd,
 *     dlogits = grad_scale / M * (ce_weight (softmax(z) - t) + kd_alpha T (q - p));
 * KL is formed as sum_c p (z_t / T) - lse(z_t / T) - sum_c p (z / T) + lse(z / T), no logarithm of a probability is taken.  dfeats, gW,
 * gb follow from dlogits as above (the teacher receives no gradient), correct and preds are those of the soft entry,
 * loss_parts [2] = (loss_ce, loss_kd), agree [1] = number of rows whose first arg-max of z equals the first arg-max of z_t (float).
 * The same two launches, LDS image, shapes, fixed summation orders and forward form: the teacher's logits of a 16-row tile are formed in
 * the LDS image first, p goes to the workspace ([M,C] floats, the teacher's only trace in memory), then the student's logits overwrite
 * the image.  With kd_alpha = 0, ce_weight = 1 loss, correct, preds, dfeats, gW and gb are bit-identical to fumi_hip_cls_head_step_soft.
 * Labels: the common contract above; a row left out adds nothing to either loss, correct, agree or the gradients.
 * FUMI_EINVAL before any launch: a NULL teacher pointer, loss_parts or agree; kd_temp, kd_alpha or ce_weight not finite; kd_temp <= 0;
 * a negative kd_alpha or ce_weight; the refusals of the soft entry. */
int fumi_hip_cls_head_step_distill(fumi_ws_t* ws, fumi_stream_t stream, int M, int F, int C,
        const float* feats, const int64_t* y_a, const int64_t* y_b, float lam, float smoothing,
        const float* W, const float* b, const float* feats_t, const float* W_t, const float* b_t,
        float kd_temp, float kd_alpha, float ce_weight, float grad_scale,
        float* loss, float* loss_parts, float* correct, float* agree, int64_t* preds, float* dfeats, float* gW, float* gb);
/* The cosine classifier head of supervised pre-training (csrc/coshead.hip): the linear head above on unit
 * vectors with a learned scale and no bias.  feats [M,F], y_a, y_b [M], W [C,F], tau [1] on the device.  With
 * u_m = feats_m / max(|feats_m|, 1e-12), v_c = W_c / max(|W_c|, 1e-12) (norms in fp32), k[m,c] = u_m . v_c and t the soft target of
 * fumi_hip_cls_head_step_soft (y_b == NULL means y_b = y_a, and lam must be 1; the hard target is y_b == NULL, lam = 1, smoothing = 0),
 *     z = tau k,   loss = mean_m (lse(z_m) - sum_c t z),   dz = grad_scale / M * (softmax(z) - t),
 *     dtau     = sum_{m,c} dz k,
 *     dfeats_m = tau / |feats_m| * (sum_c dz[m,c] v_c - (sum_c dz[m,c] k[m,c]) u_m),
 *     gW_c     = tau / |W_c|     * (sum_m dz[m,c] u_m - (sum_m dz[m,c] k[m,c]) v_c).
 * loss [1], correct [1] = number of rows whose first arg-max equals y_a (float), preds [M] = first arg-max (may be NULL);
 * dfeats [M,F], gW [C,F], dtau [1] = gradients of grad_scale * loss (written, not accumulated) -- all three given (training form) or
 * all three NULL (forward form: loss, correct and preds are bit-identical to the training form's).  Three launches: the reciprocal
 * norms of the C + M rows, then the two launches of the linear head; k of a 16-row tile stays in LDS from the product through the
 * softmax to dz and dfeats, dz / |feats_m| and dz k go to memory (workspace, 2 [M,C] floats) for gW.
 * A row of feats or W whose norm is below 1e-12 is the zero direction: k = 0 along it and its gradient row is zero; nothing else is
 * affected.  Predictions, labels, order and shapes: the common contract above.  FUMI_EINVAL before any launch
 * also for smoothing outside [0, 1), lam outside [0, 1], y_b == NULL with lam != 1, a NULL tau. */
int fumi_hip_cos_cls_head_step(fumi_ws_t* ws, fumi_stream_t stream, int M, int F, int C,
        const float* feats, const int64_t* y_a, const int64_t* y_b, float lam, float smoothing,
        const float* W, const float* tau, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* dfeats, float* gW, float* dtau);
/* ---- The episode heads (fumi_hip_cos_proto_step ... fumi_hip_trans_proto_step; shared code in csrc/fewshot_head.h) ----
 * LABELS, for all five: a label outside [0,N) sets FUMI_ST_LABEL_RANGE.  Such a query row adds nothing to the loss, the count or any
 * gradient while the divisor stays B * Qn; such a support row is left out exactly (of every mean, count, sum and fit) and gets a zero
 * gradient.  A class without a support row sets FUMI_ST_CLASS_MISSING.  Each entry says below only what is its own.
 * ORDER, for all five: every sum has a fixed order and there are no floating-point atomics, so two calls on the same inputs give the
 * same bits; preds is the first arg-max, as torch.max gives it. */
/* The cosine nearest-centroid head with a learned temperature (csrc/cosproto.hip): the few-shot metric of a
 * pre-trained backbone and the episodic loss of the Meta-Baseline stage, fused.  Per episode b, with norm(x) = x / max(|x|_2, 1e-12)
 * (F.normalize):
 *     c_n = mean of the rows of feats_s[b] with y_s == n (count clamped to >= 1, as fumi_hip_proto_reduce),
 *     z[q,n] = tau * <norm(feats_q[b,q]), norm(c_n)>,
 * loss [1] = mean over all B * Qn query rows of the softmax cross-entropy of z against y_q, preds [B,Qn] = first arg-max of z (may be
 * NULL), correct [1] = number of rows with preds == y_q (float), logits [B,Qn,N] = z (may be NULL).  tau [1] is read from DEVICE memory:
 * it is a parameter the optimizer updates, no host synchronisation is needed.
 * dfeats_s [B,S,F], dfeats_q [B,Qn,F], dtau [1] = gradients of grad_scale * loss (written, not accumulated) -- all three given (training
 * form) or all three NULL (forward form: loss, correct, preds and logits are bit-identical to the training form's).  dfeats_q goes
 * through the row normalisation, dfeats_s through the prototype normalisation and the class mean (every support row of class n receives
 * dc_n / count_n), dtau = sum dz[q,n] cos[q,n].  Where a norm is below the clamp the gradient is the plain d / 1e-12, as autograd gives
 * it; the projection onto the tangent space applies only where the norm is at or above the clamp.
 * fp32 with fp32 accumulation on v_mfma_f32_16x16x4_f32, three launches (class means; 16-row query tiles; [16 classes x 128 features]
 * blocks of the support gradient plus the final sums).  ORDER as above.
 * LABELS as above; a class without a support row has a zero prototype.
 * B >= 1, 1 <= S <= 1024, Qn >= 1, B * Qn <= 65536, 2 <= N <= 64, F % 32 == 0, 32 <= F <= 2048: FUMI_ENOTSUP otherwise; FUMI_EINVAL for
 * a NULL required pointer or for one or two of the three gradient pointers; both before any launch. */
int fumi_hip_cos_proto_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* tau, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* logits, float* dfeats_s, float* dfeats_q, float* dtau);
/* The prototypical-network head with a metric scale (csrc/euclidproto.hip): Snell et al. 2017, and the Euclidean
 * variant of the Meta-Baseline stage with TADAM's learned scale, in the slot of fumi_hip_cos_proto_step.  Per episode b:
 *     c_n = mean of the rows of feats_s[b] with y_s == n (count clamped to >= 1, as fumi_hip_proto_reduce),
 *     d2[q,n] = sum_f (feats_q[b,q,f] - c_n[f])^2,   z[q,n] = -alpha * d2[q,n],
 * loss [1] = mean over all B * Qn query rows of the softmax cross-entropy of z against y_q, preds [B,Qn] = first arg-max of z (may be
 * NULL), correct [1] = number of rows with preds == y_q (float), logits [B,Qn,N] = z (may be NULL).  alpha [1] is read from DEVICE
 * memory: it may be a parameter the optimizer updates, no host synchronisation is needed.
 * dfeats_s [B,S,F], dfeats_q [B,Qn,F], dalpha [1] = gradients of grad_scale * loss (written, not accumulated) -- all three given
 * (training form) or all three NULL (forward form: loss, correct, preds and logits are bit-identical to the training form's).  With
 * dz = grad_scale / (B Qn) (softmax(z) - onehot(y_q)):
 *     dfeats_q = 2 alpha dz C,   dc_n = 2 alpha ((dz^T F_q)_n - c_n sum_q dz[q,n]),   dalpha = -sum dz * d2,
 * every support row of class n receives dc_n / count_n.  The term -2 alpha f_q sum_n dz[q,n] of dfeats_q is left out: the sum is zero
 * in exact arithmetic.
 * The [B,Qn,N,F] differences are never formed.  The distances come from one product per tile of 16 query rows, taken relative to the
 * episode's mean prototype m = (1/N) sum_n c_n:  d2 = |f_q - m|^2 - 2 (f_q . c'_n - m . c'_n) + |c'_n|^2 with c'_n = c_n - m, so an
 * offset common to all features of an episode (post-ReLU features have one) does not cost the distance its digits.
 * fp32 with fp32 accumulation on v_mfma_f32_16x16x4_f32, three launches (class means, centred; 16-row query tiles; [16 classes x 128
 * features] blocks of the support gradient plus the final sums).  ORDER as above.
 * LABELS as above; a class without a support row has a zero prototype: its logits are -alpha |f_q|^2.
 * B >= 1, 1 <= S <= 1024, Qn >= 1, B * Qn <= 65536, 2 <= N <= 64, F % 32 == 0, 32 <= F <= 2048: FUMI_ENOTSUP otherwise; FUMI_EINVAL for
 * a NULL required pointer or for one or two of the three gradient pointers; both before any launch. */
int fumi_hip_euclid_proto_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* alpha, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* logits, float* dfeats_s, float* dfeats_q, float* dalpha);
/* The Matching Networks head with a learned temperature (csrc/matchhead.hip): Vinyals et al. 2016 without the
 * full-context embeddings, in the slot of fumi_hip_cos_proto_step.  A query attends over the individual support rows, not over class
 * means.  Per episode b, with norm(x) = x / max(|x|_2, 1e-12) (F.normalize) and a support row valid when its label is in [0,N):
 *     cos[q,i] = <norm(feats_q[b,q]), norm(feats_s[b,i])>,   a[q,i] = tau * cos[q,i],
 *     z[q,n] = logsumexp over the valid rows i with y_s == n of a[q,i]     (the class maximum is subtracted before exp),
 * loss [1] = mean over all B * Qn query rows of the softmax cross-entropy of z against y_q, which is the Matching Networks negative
 * log-likelihood -log sum_{i: y_i = y_q} softmax_i(a[q,:]); preds [B,Qn] = first arg-max of z (may be NULL), correct [1] = number of
 * rows with preds == y_q (float), logits [B,Qn,N] = z (may be NULL).  z is formed per class from the class's own maximum, never as the
 * log of a sum of globally normalised probabilities: a class far below the row's best keeps a finite, accurate logit.  tau [1] is read
 * from DEVICE memory: it is a parameter the optimizer updates, no host synchronisation is needed.
 * dfeats_s [B,S,F], dfeats_q [B,Qn,F], dtau [1] = gradients of grad_scale * loss (written, not accumulated) -- all three given (training
 * form) or all three NULL (forward form: loss, correct, preds and logits are bit-identical to the training form's).  With gs =
 * grad_scale / (B Qn), p[q,i] the softmax of a over all valid rows and r[q,i] the softmax within the class y_q (zero outside it):
 *     da[q,i] = gs (p[q,i] - r[q,i])        (each row of da sums to zero),        dtau = sum da * cos,
 *     dfeats_q = rq (G_q - norm(f_q) <norm(f_q), G_q>),   G_q = tau sum_i da[q,i] norm(x_i),
 *     dfeats_s = rs (G_i - norm(x_i) <norm(x_i), G_i>),   G_i = tau sum_q da[q,i] norm(f_q),
 * rq, rs the reciprocal clamped norms.  Where a norm is below the clamp the gradient is the plain d / 1e-12, as autograd gives it; the
 * projection onto the tangent space applies only where the norm is at or above the clamp.
 * fp32 with fp32 accumulation on v_mfma_f32_16x16x4_f32, three launches (support norms, class counts and status; 16-row query tiles with
 * the [16,S] scores in LDS; [16 support rows x 128 features] blocks of the support gradient plus the final sums).  ORDER as above.
 * LABELS as above, with one difference the method forces: a class without a valid support row has no zero prototype -- there is no row
 * to attend to -- so z = -inf for it (it carries no mass and is never predicted unless the whole row is NaN), and a query row
 * labelled with such a class is left out exactly like a query label outside [0,N).  A row of NaNs predicts class 0.
 * B >= 1, 1 <= S <= 512, Qn >= 1, B * Qn <= 65536, 2 <= N <= 64, F % 32 == 0, 32 <= F <= 2048: FUMI_ENOTSUP otherwise; FUMI_EINVAL for
 * a NULL required pointer or for one or two of the three gradient pointers; both before any launch. */
int fumi_hip_match_head_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* tau, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* logits, float* dfeats_s, float* dfeats_q, float* dtau);
/* The Relation Network head (csrc/relationhead.hip): Sung et al. 2018 in the feature-vector form of the relation
 * module, Linear(2F,H) -> ReLU -> Linear(H,1) on the concatenation (class mean, query), which is never formed.  It is the one episode
 * head that owns weight TENSORS, all read from device memory in torch's [out, in] layout: w1 [2,H,F] (block 0 = W1s, applied to the class
 * mean; block 1 = W1q, applied to the query), b1 [H], w2 [H], b2 [1].  Per episode b, with c_n the mean of the valid support rows of
 * class n (count clamped to >= 1, the sums in the order of fumi_hip_proto_reduce):
 *     U[n,:] = W1s c_n + b1,   V[q,:] = W1q feats_q[b,q],   z[q,n] = w2 . relu(U[n,:] + V[q,:]) + b2.
 * loss_kind 1 (mse, the paper's loss): loss [1] = 1 / (B Qn N) * sum over the valid query rows and the N classes of
 * (sigmoid(z[q,n]) - onehot(y_q)[n])^2, and with s = sigmoid(z), t the one-hot target, dz = grad_scale * 2 / (B Qn N) * (s - t) s (1 - s).
 * loss_kind 0 (ce, Chen et al. 2019): loss [1] = mean over all B * Qn rows of the softmax cross-entropy of z over the N classes,
 * dz = grad_scale / (B Qn) * (softmax - onehot).  In both, preds [B,Qn] = first arg-max of z (may be NULL), correct [1] = number of rows
 * with preds == y_q (float), logits [B,Qn,N] = z (may be NULL); hid_s [B,N,H] = U and hid_q [B,Qn,H] = V (either may be NULL).
 * dfeats_s [B,S,F], dfeats_q [B,Qn,F], dw1 [2,H,F], db1 [H], dw2 [H], db2 [1] = gradients of grad_scale * loss (written, not
 * accumulated) -- all six given (training form) or all six NULL (forward form: loss, correct, preds, logits, hid_s and hid_q are
 * bit-identical to the training form's).  With the mask m[q,n,h] = (U[n,h] + V[q,h] > 0):
 *     dV[q,h] = w2[h] sum_n dz[q,n] m,   dU[n,h] = w2[h] sum_q dz[q,n] m,   dw2[h] = sum_{b,q,n} dz relu(U + V),   db2 = sum dz,
 *     db1 = column sum of dU over all B N rows,   dW1q = dV^T F_q over all B Qn rows,   dW1s = dU^T C over all B N rows,
 *     dfeats_q = dV W1q,   dc = dU W1s,   every valid support row of class n receives dc_n / count_n.
 * THE MASK is part of the interface, the ReLU's kink being the one place where fp32 and a float64 restatement may legitimately
 * disagree: it is fl32(U[n,h] + V[q,h]) > 0, ONE fp32 addition of the stored fp32 U and V, in the forward and in the backward.  A
 * correctly rounded sum keeps the sign of the exact sum, so the mask can be rebuilt exactly from hid_s and hid_q.
 * fp32 throughout; U, V and the five products of the backward on the dense GEMM (v_mfma_f32_32x32x2_f32), the pair terms on the VALU.
 * Launches: class means, counts and status; U; V; 16-row query tiles that walk H in chunks of 128 with the episode's U chunk [N,128]
 * and the tile's V chunk [16,128] in LDS (z, the loss, and in the training form dz and dV); training form only: one workgroup per
 * (group of episodes, 128 hidden units) for dU, dw2 and db1 over all Qn rows (three fixed levels: 8 rows, 64 rows, the blocks) with the
 * mask rebuilt from U and V, then
 * dfeats_q, dc, dW1q, dW1s (the last two split over their rows into at most 8 slabs and summed in slab order where the rows are
 * many); last, the scatter of dc to the support rows and the final sums.  5 launches in the forward form, 10 to 12 in the training form.
 * Workspace, in floats, M = B Qn: B N F + B N + 3 ceil-tiles + (B N H without hid_s) + (M H without hid_q); training form in addition
 * M N + M H + B N H + B N F + 2 min(B,256) H + the slabs, at most 4 M floats each.  No mask and no per-tile [N,H] image is stored: at
 * M = 65536, N = 64, H = 1024 the terms in M are 0.54 GB against the 1 GB such an image would take, and 17 MB at H = 32.
 * ORDER as above, the sums across query tiles (dU) and across episodes (dw1, db1, dw2, db2) included.  LABELS as above: a support row
 * left out is written as a zero row of dfeats_s; a class without a support row has a zero prototype, so U[n,:] = b1.  A row of NaNs
 * predicts class 0.
 * B >= 1, 1 <= S <= 1024, Qn >= 1, B * Qn <= 65536, 2 <= N <= 64, F % 32 == 0, 32 <= F <= 2048, H % 32 == 0, 32 <= H <= 1024,
 * loss_kind 0 or 1: FUMI_ENOTSUP otherwise; FUMI_EINVAL for a NULL required pointer or for one to five of the six gradient pointers;
 * both before any launch, nothing is written. */
int fumi_hip_relation_head_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F, int H,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* w1, const float* b1,
        const float* w2, const float* b2, int loss_kind, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* logits, float* hid_s, float* hid_q,
        float* dfeats_s, float* dfeats_q, float* dw1, float* db1, float* dw2, float* db2);
/* The ridge-regression few-shot head with a backward (csrc/ridgehead.hip): the closed-form base learner of R2-D2
 * and of MetaOptNet's ridge head, in the slot of fumi_hip_cos_proto_step.  params [2] = (rho, alpha) is read from DEVICE memory (both
 * are parameters the optimizer updates); lam = exp(rho) is the ridge weight, alpha the logit scale.  Per episode b, with X = feats_s[b]
 * [S,F], Y = onehot(y_s[b]) [S,N], Fq = feats_q[b] [Qn,F]:
 *     M = X X^T + lam I,   A = M^-1 Y,   W = X^T A [F,N],   z = alpha Fq W,
 * loss [1] = mean over all B * Qn query rows of the softmax cross-entropy of z against y_q, preds [B,Qn] = first arg-max of z (may be
 * NULL), correct [1] = number of rows with preds == y_q (float), logits [B,Qn,N] = z (may be NULL).
 * dfeats_s [B,S,F], dfeats_q [B,Qn,F], dparams [2] = gradients of grad_scale * loss (written, not accumulated) -- all three given
 * (training form) or all three NULL (forward form: loss, correct, preds and logits are bit-identical to the training form's):
 *     dz = grad_scale / (B Qn) (softmax(z) - onehot(y_q)),   dfeats_q = alpha dz W^T,   dW = alpha Fq^T dz,   G = M^-1 (X dW),
 *     dfeats_s = A (dW - X^T G)^T - G W^T,   dparams = (-lam sum G * A,  sum dz * (Fq W)).
 * fp32 with fp32 accumulation on v_mfma_f32_16x16x4_f32; M is factored once per episode (Cholesky in LDS) and the factor serves both
 * solves.  Four launches in the forward form, six in the training form.  ORDER as above.
 * LABELS as above; a support row left out counts as a zero feature row, its rows of Y, A and dfeats_s are zero; a class without a
 * support row has logits 0.  A pivot of the factorisation
 * that is not > 0 (a NaN counts) sets FUMI_ST_NOT_POSDEF and is replaced by lam; the call returns and the other episodes are untouched.
 * B >= 1, 1 <= S <= 128, Qn >= 1, B * Qn <= 65536, 2 <= N <= 64, F % 32 == 0, 32 <= F <= 2048: FUMI_ENOTSUP otherwise; FUMI_EINVAL for
 * a NULL required pointer or for one or two of the three gradient pointers; both before any launch. */
int fumi_hip_ridge_head_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* params, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* logits, float* dfeats_s, float* dfeats_q, float* dparams);
/* The logistic-regression few-shot head, forward only (csrc/logreghead.hip): the frozen-backbone protocol of Tian
 * et al. 2020.  Per episode b, with X = feats_s[b] [S,F], x~_i = x_i / max(|x_i|, 1e-12) when `normalize` (the query rows alike), n the
 * number of support rows with a label in [0,N) (at least 1), wd = 1 / (C n):
 *     f(W, b) = (1/n) sum_i CE(W^T x~_i + b, y_i) + (wd/2) |W|^2      (scikit-learn's LogisticRegression(C) divided by n),
 * `steps` steps of heavy-ball descent V <- momentum V + grad, (W, b) <- (W, b) - lr V from W = 0, b = 0, V = 0, iterated in the dual
 * (W_t = X~^T A_t, on K~ = X~ X~^T in LDS; exactly the primal iteration), then z = Fq~ W + b.
 * loss [1] = mean over all B * Qn query rows of the softmax cross-entropy of z against y_q, preds [B,Qn] = first arg-max of z (may be
 * NULL), correct [1] = number of rows with preds == y_q (float), logits [B,Qn,N] = z (may be NULL).  There are no gradient outputs.
 * fp32; four launches (fit, one workgroup per episode; W^T; 16-row query tiles; the final sums).  ORDER as above, with or
 * without preds and logits.
 * LABELS as above; a support row left out has a zero row and column of K~ and zero rows of Y and R and does not count in n; a class
 * without a support row is fitted like any class.  The fit
 * runs `steps` steps whatever the values are; non-finite features stay inside their episode.
 * B >= 1, 1 <= S <= 128, Qn >= 1, B * Qn <= 65536, 2 <= N <= 64, F % 32 == 0, 32 <= F <= 2048, 1 <= steps <= 10000, lr > 0,
 * 0 <= momentum < 1, C > 0: FUMI_ENOTSUP otherwise; FUMI_EINVAL for a NULL required pointer; both before any launch. */
int fumi_hip_logreg_head_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, int steps, float lr, float momentum, float C,
        int normalize, float* loss, float* correct, int64_t* preds, float* logits);
/* The form of the fit's product K~ A [S,S] x [S,NP] in the calls that follow, process-wide: 0 the VALU loop, 1 the f32 MFMA
 * (v_mfma_f32_16x16x4_f32), -1 (the default) the faster of the two as measured for the shape.  Both forms are held to the same
 * float64 definition; each gives the same bits from call to call, the two need not agree in the last bits.  FUMI_EINVAL for any
 * other value.  For tests and tools/bench_logreg_head.py. */
int fumi_hip_logreg_set_form(int form);
/* The MetaOptNet-SVM few-shot head with an implicit backward (csrc/svmhead.hip): the multi-class SVM base
 * learner of Lee et al. 2019, in the slot of fumi_hip_ridge_head_step.  scale [1] is read from DEVICE memory (a parameter the
 * optimizer updates); C and eps are fixed.  Per episode b, with X = feats_s[b] [S,F], Y = onehot(y_s[b]) [S,N], Fq = feats_q[b]
 * [Qn,F], K' = X X^T + eps I:
 *     alpha = argmin 1/2 tr(alpha^T K' alpha) - <alpha, Y>   subject to   alpha_ik <= C Y_ik,   sum_k alpha_ik = 0 for every i,
 *     W = X^T alpha [F,N],   z = scale Fq W,
 * fitted by `steps` steps of FISTA from zero at the step 1 / max_i sum_j |K'_ij| with the momentum sequence
 * t' = (1 + sqrt(1 + 4 t^2)) / 2; the projection on the constraints is exact (from the breakpoints of each row, no tolerance).
 * loss [1] = mean over all B * Qn query rows of the softmax cross-entropy of z against y_q, preds [B,Qn] = first arg-max of z (may be
 * NULL), correct [1] = number of rows with preds == y_q (float), logits [B,Qn,N] = z (may be NULL).
 * dfeats_s [B,S,F], dfeats_q [B,Qn,F], dscale [1] = gradients of grad_scale * loss (written, not accumulated) -- all three given
 * (training form) or all three NULL (forward form: loss, correct, preds and logits are bit-identical to the training form's).  The
 * gradient is the implicit one at the fitted point, not an unrolled one: with `bound` the entries the last projection clamped
 * (v_k - tau >= C Y_ik in the kernel's arithmetic), P the map that zeroes the bound entries and takes from every row the mean of its
 * free entries (a row with fewer than two free entries becomes zero), dz = grad_scale / (B Qn) (softmax(z) - onehot(y_q)):
 *     dW = scale Fq^T dz,   p: P K' P p = P (X dW)   (`bwd_steps` steps of conjugate gradients from zero, ended early when r.r <= 1e-12 r0.r0),
 *     dfeats_s = alpha (dW - X^T p)^T - p W^T,   dfeats_q = scale dz W^T,   dscale = sum dz * (Fq W).
 * stats [B,2] (may be NULL) = per episode the KKT residual max |alpha - proj(alpha - (K' alpha - Y))| of the fit and the relative
 * residual sqrt(r.r / r0.r0) the conjugate gradients ended at (0 in the forward form): the gradient is only as good as the fit.
 * fp32; K' alpha on v_mfma_f32_16x16x4_f32 or in a VALU loop (fumi_hip_svm_set_form), K' and the iterates in LDS, one workgroup per
 * episode for the fit and for the conjugate gradients.  Four launches in the forward form, six in the training form.  ORDER as above.
 * LABELS as above; a support row left out counts as a zero feature row, has alpha_i = 0 and a zero row of dfeats_s; a class without
 * a support row is fitted like any class.  The fit runs `steps` steps whatever the values are.
 * B >= 1, 1 <= S <= 128, Qn >= 1, B * Qn <= 65536, 2 <= N <= 64, F % 4 == 0, 4 <= F <= 2048, 1 <= steps <= 10000,
 * 1 <= bwd_steps <= 1000, C > 0, eps > 0, no NULL required pointer, all or none of the three gradient pointers: FUMI_EINVAL
 * otherwise, before any launch. */
int fumi_hip_svm_head_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* scale, float C, float eps,
        int steps, int bwd_steps, float grad_scale, float* loss, float* correct, int64_t* preds, float* logits, float* dfeats_s,
        float* dfeats_q, float* dscale, float* stats);
/* The form of the products K' Zt and K' d [S,S] x [S,N] of the fit and of the conjugate gradients in the calls that follow,
 * process-wide: 0 the VALU loop, 1 the f32 MFMA, -1 (the default) the faster of the two as measured for the shape.  Both forms are
 * held to the same float64 definition; each gives the same bits from call to call, the two need not agree in the last bits.
 * FUMI_EINVAL for any other value.  For tests and tools/bench_svm_head.py. */
int fumi_hip_svm_set_form(int form);
/* alpha [B,S,N] (float) and the bound mask [B,S,N] (int32, 1 = bound) of the fumi_hip_svm_head_step call that was the last call on
 * this workspace, copied from the workspace on `stream` into device memory.  B, S, N are that call's.  For tests. */
int fumi_hip_svm_get_fit(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int N, float* alpha, int32_t* mask);
/* Transductive prototype refinement, forward only (csrc/transproto.hip): per episode, from the class sums s_n and
 * counts k_n of feats_s [B,S,F] by y_s [B,S] and c^0_n = s_n / max(k_n, 1), `steps` steps of soft k-means on the query rows feats_q
 * [B,Qn,F],
 *     w = softmax_n(z(c^t)),   c^{t+1}_n = (s_n + sum_q w[q,n] f_q) / (k_n + sum_q w[q,n]),
 * with z(c)[q,n] = scale[0] cos(f_q, c_n) (metric 0; both norms clamped at 1e-12) or -scale[0] |f_q - c_n|^2 (metric 1).  loss [1] is
 * the mean softmax cross-entropy of z(c^steps) against y_q [B,Qn] over all B * Qn rows, correct [1] the number of rows whose first
 * arg-max is the label, preds [B,Qn] that arg-max (optional), logits [B,Qn,N] z(c^steps) (optional).  steps = 0 is the forward form
 * of fumi_hip_cos_proto_step / fumi_hip_euclid_proto_step.  scale is a device pointer.  The iteration runs in the dual on X_all S^T
 * and X_all X_q^T (the f32 MFMA; metric 1 takes the rows relative to the mean step-0 prototype first), one workgroup per episode, two
 * barriers per step.  ORDER as above.
 * LABELS as above; a query row whose label is out of range still takes part in the refinement; a class without a support row starts
 * from a zero prototype and is refined like any class.
 * B >= 1, S >= 1, Qn >= 1, S + Qn <= 512, Qn * N <= 8192, B * Qn <= 65536, 2 <= N <= 64, F % 32 == 0, 32 <= F <= 2048,
 * 0 <= steps <= 100: FUMI_ENOTSUP otherwise; FUMI_EINVAL for a NULL required pointer or a metric other than 0 or 1; both before any
 * launch. */
int fumi_hip_trans_proto_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* scale, int metric, int steps,
        float* loss, float* correct, int64_t* preds, float* logits);
/* Set-to-set prototype adaptation in front of the prototype heads (csrc/featadapt.hip): FEAT (Ye et al., CVPR
 * 2020), one self-attention block over the set of an episode's class prototypes, one head with d_k = d_v = F.  Per episode b:
 *     P  = mean of the rows of feats_s[b] with y_s == n (count clamped to >= 1, as fumi_hip_proto_reduce)      [N,F]
 *     Q  = P Wq^T,  K = P Wk^T,  V = P Wv^T          (Wqkv [3F,F] = the rows of Wq, Wk, Wv in this order; no bias)
 *     A  = softmax_rows(Q K^T / sqrt(F))             [N,N]   (the row maximum is subtracted before exp)
 *     O  = A V,   U = O Wo^T + bo,   R = P + U       (Wo [F,F], bo [F])
 *     P' = gamma * (R - mean_f R) / sqrt(var_f R + 1e-5) + beta                  (LayerNorm over F, biased variance; gamma, beta [F])
 * protos_out [B,N,F] = P'.  It is an N-way 1-shot support set with the labels 0..N-1 of every episode: fumi_hip_cos_proto_step and
 * fumi_hip_euclid_proto_step classify against it unchanged, and their dfeats_s is dprotos of the backward.
 * K and V are formed from P - m, m the episode's mean prototype, and O = A V + m Wv^T: the same numbers in exact arithmetic, without the
 * round-off that an offset common to all features (post-ReLU features have one) costs the softmax and its backward.
 * tape: caller memory of fumi_hip_feat_adapt_tape_floats(B, N, F) floats that receives what the backward needs (P, Q|K|V, A, O, R, the
 * mean and 1 / std of every row, the class counts), or NULL (forward form: protos_out is bit-identical to the taped form's).
 * fumi_hip_feat_adapt_bwd, given the tape of the forward call on the same inputs and dprotos [B,N,F] = d(grad_scale * loss) / dP',
 * writes (never accumulates) dfeats_s [B,S,F], dWqkv [3F,F], dWo [F,F], dbo [F], dgamma [F], dbeta [F]: through the LayerNorm (dR,
 * dgamma = sum_rows dP' xhat, dbeta = sum_rows dP'), the output projection, the attention (dV = A^T dO, dA = dO V^T,
 * dS = A (dA - sum_n dA A) / sqrt(F), dQ = dS K, dK = dS^T Q), the three projections and the residual; every support row of class n
 * receives dP_n / count_n.  The gradient outputs need no alignment beyond a float's (they may be slices of one flat buffer).
 * fp32 with fp32 accumulation on the f32 MFMA.  Forward: eight launches (class means; three products for Q, K | V and m Wv^T; scores and softmax, one workgroup per
 * episode, the contraction over F streamed through LDS; A V per 128 features; O Wo^T + bo; residual and LayerNorm, one wave per row).
 * Backward: ten launches.  The four F x F projections and their gradients run on the dense GEMM behind fumi_hip_linear_*.  ORDER as
 * for the episode heads: fixed summation orders, no floating-point atomics, equal inputs give equal bits.
 * LABELS: a support label outside [0,N) sets FUMI_ST_LABEL_RANGE; that row is left out of the mean and gets a zero gradient.  A class
 * without a support row sets FUMI_ST_CLASS_MISSING, has P_n = 0 and still takes part in the attention.  The forward raises the flags.
 * B >= 1, 1 <= S <= 1024, 2 <= N <= 64, B * N <= 65536, F % 32 == 0, 32 <= F <= 2048: FUMI_ENOTSUP otherwise (the tape size is 0
 * there); FUMI_EINVAL for a NULL required pointer (every pointer but the forward's tape); both before any launch. */
int64_t fumi_hip_feat_adapt_tape_floats(int B, int N, int F);
int fumi_hip_feat_adapt_fwd(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int N, int F, const float* feats_s,
        const int64_t* y_s, const float* Wqkv, const float* Wo, const float* bo, const float* gamma, const float* beta,
        float* protos_out, float* tape);
int fumi_hip_feat_adapt_bwd(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int N, int F, const float* feats_s,
        const int64_t* y_s, const float* Wqkv, const float* Wo, const float* bo, const float* gamma, const float* beta,
        const float* tape, const float* dprotos, float* dfeats_s, float* dWqkv, float* dWo, float* dbo, float* dgamma,
        float* dbeta);
/* mix_images (csrc/immix.hip): the blend of a gathered batch x float [M,C,H,W] with the rows partner [M]
 * (device int64) names, into out (same shape; must not overlap x, row i reads row partner[i]: FUMI_EINVAL).
 *   mode 0, mixup:   out[i] = lam * x[i] + (1.0f - lam) * x[partner[i]], each operation rounded on its own; the box is ignored.
 *   mode 1, CutMix:  out[i][:, r, c] = x[partner[i]][:, r, c] for by0 <= r < by1, bx0 <= c < bx1 and x[i] elsewhere (a copy);
 *                    lam is ignored.
 * A row that is its own partner is copied.  A partner outside [0, M) sets FUMI_ST_LABEL_RANGE and its row is copied unmixed; no
 * read leaves x.  128-bit loads and stores when C H W % 4 == 0 and both pointers are 16-byte aligned, single floats otherwise.
 * FUMI_EINVAL: M, C, H or W < 1, mode not 0 or 1, lam outside [0, 1], a box outside the image or with bx1 < bx0 or by1 < by0 (mode 1). */
int fumi_hip_mix_images(fumi_ws_t* ws, fumi_stream_t stream, int M, int C, int H, int W, const float* x, const int64_t* partner,
        int mode, float lam, int bx0, int by0, int bx1, int by1, float* out);


/* ---- beside the episodic path -------------------------------------------------------------------------------
 * CLIP baseline, fumi/models/clip.py.  w: 8 pointers text_fc W [P,Dt], b [P], text_fc2 W [P,P], b, image_fc W [P,D], b,
 * image_fc2 W [P,P], b.  sim [nt,ni] = cosine similarity of every (text row, image row) pair (clip.py:27-41).  loss != NULL
 * (needs nt == ni): the symmetric cross-entropy against the diagonal, (CE(sim) + CE(sim^T)) / 2 (clip.py:101-105); need_grad:
 * its gradient w.r.t. the 8 tensors (written, not accumulated). */
int fumi_hip_clip_step(fumi_ws_t* ws, fumi_stream_t stream, int nt, int ni, int Dt, int D, int P,
        const float* text, const float* image, const float* const* w, int need_grad,
        float* sim, float* loss, float* const* g_w);
/* bi-LSTM text encoders RNN / RnnHid (fumi/models/common.py:44-161), forward only: tokens [R,L] int64 -> embedding rows of
 * table [V,E] -> single-layer bidirectional LSTM over the non-PAD prefix of every row (pack_padded_sequence semantics) ->
 * out [R,2H] = each direction's final hidden state (use_cell = 0: RNN) or cell state (use_cell = 1: RnnHid).
 * w: 8 pointers in nn.LSTM's layout (gate order i,f,g,o): weight_ih_l0 [4H,E], weight_hh_l0 [4H,H], bias_ih_l0, bias_hh_l0, then
 * the four *_reverse tensors. */
int fumi_hip_lstm_bidir(fumi_ws_t* ws, fumi_stream_t stream, int R, int L, int E, int H,
        const int64_t* tokens, int64_t pad_id, const float* table, int64_t V, const float* const* w, int use_cell, float* out);
/* The same encoders under --fine_tune (fumi/models/fumi.py:65-67 leaves text_encoder.parameters() trainable; the word table is
 * nn.Embedding.from_pretrained, frozen either way, common.py:60-63).  The training-mode forward writes, besides out, the tape the
 * backward needs into caller memory of fumi_hip_lstm_tape_floats(R, L, E, H) floats; the backward is back-propagation through time
 * over the same packed prefixes: d_out [R,2H] (adjoint of out) -> g_w, 8 tensors shaped like w (written, not accumulated;
 * bias_ih and bias_hh receive the same sums).  Rows whose d_out is zero contribute nothing. */
int64_t fumi_hip_lstm_tape_floats(int R, int L, int E, int H);
int fumi_hip_lstm_bidir_train(fumi_ws_t* ws, fumi_stream_t stream, int R, int L, int E, int H,
        const int64_t* tokens, int64_t pad_id, const float* table, int64_t V, const float* const* w, int use_cell, float* out,
        float* tape);
int fumi_hip_lstm_bidir_bwd(fumi_ws_t* ws, fumi_stream_t stream, int R, int L, int E, int H,
        const int64_t* tokens, int64_t pad_id, const float* const* w, int use_cell, const float* tape, const float* d_out,
        float* const* g_w);
/* The text gradient, what autograd hands a trainable text encoder in the reference, is the last argument of every step that has
 * one: fumi_hip_fumi_step / _indexed / fumi_hip_fumi_conv4_step / fumi_hip_fumi_resnet12_step write g_cls_text [B*N, Dt] =
 * d(grad_scale * sum_b loss_b) / d(class text rows) (get_hyper_params, fumi.py:196-215), whether the rows came as cls_text or were
 * selected from text_s; fumi_hip_am3_step / _dx write g_text [B*S, Dt] = d loss / d text_s (every support row feeds its class
 * prototype, am3.py:113-126).  NULL = not wanted.  Written only when need_grad != 0; with need_grad == 0 a given buffer is ignored
 * and left untouched.  Never retained past the call. */

/* FuMI meta-step on ZERO-COPY episodes: identical to fumi_hip_fumi_step except that the image rows are not handed over as
 * x_s [B,S,D] / x_q [B,Qn,D] but addressed in an HBM-resident table [n_rows, D] through idx_s [B,S] / idx_q [B,Qn] (what
 * fumi_hip_sample_episodes produces): the two X-panel kernels read the rows where they lie, the 2*B*(S+Qn)*D*4 bytes of a
 * gathered meta-batch are never written or re-read.  Bit-identical results to the gathered call.  An index outside
 * [0, n_rows) sets FUMI_ST_LABEL_RANGE and is read as row 0. */
int fumi_hip_fumi_step_indexed(fumi_ws_t* ws, fumi_stream_t stream,
        int B, int N, int S, int Qn, int D, int n_hidden, const int* hid, int Dt, int Ht,
        int T, float alpha, int tanh_head, int need_grad, float grad_scale, float dropout_p, uint64_t seed,
        const float* table, int64_t n_rows, const int64_t* idx_s, const int64_t* y_s, const int64_t* idx_q, const int64_t* y_q,
        const float* cls_text, const float* text_s,
        const float* const* theta, const float* const* phi,
        float* logits_q, int64_t* preds_q, float* preds_q_f32, float* loss_b, float* acc_b, float* stats,
        float* const* g_theta, float* const* g_phi, float* g_cls_text);

/* ---- GPU-resident episode sampler (replaces fumi/dataset/data.py:294-581 + the torchmeta loader for
 * precomputed embeddings held in HBM) ---------------------------------------------------------------------------------
 * sample_episodes: for every episode b < B: N distinct classes of [0, C) and, per class, K + Q distinct members of its
 *   item list class_items[class_ptr[c] .. class_ptr[c+1]) (CSR, device arrays), all uniformly at random from the
 *   counter-based stream (seed, step) -- reproducible, restated in oracle/sampler_ref.py.  Outputs (device, int64):
 *   classes [B,N], items_s [B,N,K], items_q [B,N,Q] (class-major like torchmeta's ConcatTask: label of slot n is n).
 *   A class with fewer than K + Q items sets FUMI_ST_CLASS_MISSING (torchmeta's ClassSplitter raises) and wraps around.
 * gather_rows: out[i, :] = table[idx[i], :] for rows of row_bytes bytes (a multiple of 4): the image rows of a meta-batch,
 *   or the per-class text rows / token rows.  An index outside [0, n_rows) sets FUMI_ST_LABEL_RANGE and reads row 0. */
int fumi_hip_sample_episodes(fumi_ws_t* ws, fumi_stream_t stream, uint64_t seed, uint64_t step, int B, int N, int K, int Q,
        int C, const int64_t* class_ptr, const int64_t* class_items, int64_t* classes, int64_t* items_s, int64_t* items_q);
/* The same with torchmeta's task semantics: labels [B,N] = a random permutation of 0..N-1 per task
 * (torchmeta.transforms.Categorical relabels the class slots); fixed_split != 0: the K + Q members of every class are a
 * function of (seed, the task's class tuple) only -- ClassSplitter(shuffle=True) seeds its permutation with hash(task) + seed, so
 * a class tuple drawn again has the same support / query split.  Same (seed, step) stream for the class draw as above. */
int fumi_hip_sample_episodes_tm(fumi_ws_t* ws, fumi_stream_t stream, uint64_t seed, uint64_t step, int B, int N, int K, int Q,
        int C, const int64_t* class_ptr, const int64_t* class_items, int fixed_split, int64_t* classes, int64_t* labels,
        int64_t* items_s, int64_t* items_q);
int fumi_hip_gather_rows(fumi_ws_t* ws, fumi_stream_t stream, const void* table, int64_t n_rows, int64_t row_bytes,
        const int64_t* idx, int64_t n_idx, void* out);
/* gather_images (csrc/imgather.hip): out[i] = normalise(jitter(flip(crop(zero_pad(table[idx[i]]))))) -- n_idx images of a device
 *   table uint8 [n_images, C, H, W] (planar) into float [n_idx, C, H, W], one launch, nothing on the host.  mean / inv_std are
 *   HOST arrays of C floats.  All draws come from the stream of fumi_hip_sample_episodes: key = its 32-bit (seed, step) key,
 *   r(c, n) = rand_below(key, i, 0xFF00 + stream_id, c, n) with i the flat output index (stream_id: 0 support, 1 query, < 254).
 *     crop    ox = r(0, 2 pad + 1), oy = r(1, 2 pad + 1) for pad > 0, else both pad;   flip  fl = flip ? r(2, 2) : 0
 *     source  sx = (fl ? W - 1 - x : x) + ox - pad, sy = y + oy - pad; byte 0 outside the image (pad, crop, flip: torchvision's order)
 *     float   v = (float)u * k, k the fp32 nearest to 1 / 255
 *     jitter  (any amplitude > 0; brightness, contrast, saturation in this order; an amplitude of 0 skips its step)
 *             f_j = 1 + a_j (2 u_j - 1), u_j = r(3 + j, 1 << 24) 2^-24;  v = clamp01(v f_0);  v = clamp01(m + f_1 (v - m)) with m the
 *             mean over the H x W output window of g = 0.299 R + 0.587 G + 0.114 B;  v = clamp01(g + f_2 (v - g)), g recomputed
 *     out     (v - mean[c]) * inv_std[c]
 *   No FMA contraction: with the jitter off the result is bit-reproducible in float32 (tests/image_gather_ref.py); with it on
 *   only the order of the gray-mean sum is free, and it is fixed (two calls give the same bits).
 *   An index outside [0, n_images) sets FUMI_ST_LABEL_RANGE and reads image 0.  C in 1..8, H, W >= 1, 0 <= pad <= 64, amplitudes
 *   in [0, 1] (FUMI_EINVAL otherwise); jitter with C != 3, or an image of more than ~64 KB, is FUMI_ENOTSUP. */
int fumi_hip_gather_images(fumi_ws_t* ws, fumi_stream_t stream, const uint8_t* table, int64_t n_images, int C, int H, int W,
        const int64_t* idx, int64_t n_idx, const float* mean, const float* inv_std, uint64_t seed, uint64_t step, int stream_id,
        int pad, int flip, float jit_brightness, float jit_contrast, float jit_saturation, float* out);
/* gather_images_resized (csrc/imresize.hip): the same for a table whose images are not of the size the encoder takes --
 *   out[i] = normalise(jitter(flip(resample(rect_i of table[idx[i]])))), table uint8 [n_images, C, Hs, Ws], out float [n_idx, C, Ho, Wo].
 *   rect_i = (x0, y0, w, h) in whole source pixels, 1 <= w <= Ws, 1 <= h <= Hs, inside the image, is resampled to Ho x Wo with a
 *   separable triangle filter (antialiased bilinear: plain bilinear with clamped edges when the rectangle is not larger than the
 *   output, an exact copy when it is of the same size).  Every operation below is ONE float32 operation rounded on its own (no FMA
 *   contraction, no fast-math, correctly rounded / and sqrt), restated in tests/image_resize_ref.py.
 *   Per axis (x shown: n_in = w, n_out = Wo; y the same with h, Ho):
 *     scale = (float)n_in / (float)n_out;  s = max(scale, 1);  inv = 1 / s
 *     output x:  c = scale * ((float)x + 0.5f);  k0 = max(0, (int)(c - s + 0.5f)),  k1 = min(n_in, (int)(c + s + 0.5f))  (truncating)
 *                w_k = max(0, 1 - |((float)k - c + 0.5f) * inv|) for k = k0 .. k1 - 1;  tot = sum of w_k in ascending k from 0.f
 *     horizontal t[y'][x] = (sum in ascending k of w_k * (float)u[y0 + y'][x0 + k], accumulated as acc = acc + w_k * v) / tot, for every
 *     row y' of the rectangle, pixel values as floats in 0..255;  vertical: the same over t, giving r[y][x].
 *     (The kernel recomputes the horizontal sums of the rows an output pixel needs and drops end taps of weight 0: the same bits.)
 *   After resampling:  flip  output column x takes r[y][fl ? Wo - 1 - x : x], fl = flip ? r(2, 2) : 0;  v = r * k, k the fp32 nearest
 *     to 1 / 255;  jitter (counters 3..5) and (v - mean[c]) * inv_std[c] exactly as fumi_hip_gather_images: same formulas, order and
 *     clamp; the gray mean is taken over the Ho x Wo output, in double, in a fixed order (two calls give the same bits).
 *   mode FUMI_RESIZE_FIXED: (rect_x0, rect_y0, rect_w, rect_h) for every image; FUMI_EINVAL if it leaves the image.
 *   mode FUMI_RESIZE_RANDOM: a random-resized crop per image, 0 < scale_min <= scale_max <= 1, ratio_max >= 1 (FUMI_EINVAL
 *     otherwise), from the same hash r(c, n) = rand_below(key, i, 0xFF00 + stream_id, c, n); counters 0..5 keep their meaning.
 *     With U(c) = (float)r(c, 1 << 24) * 0x1p-24f:
 *       a = scale_min + (scale_max - scale_min) * U(6);  q = 1 + (ratio_max - 1) * U(7);  ratio = r(8, 2) ? q : 1 / q
 *       A = (float)(Hs * Ws);  wf = sqrt(a * A * ratio),  hf = sqrt(a * A / ratio)
 *       w = clamp((int)rintf(wf), 1, Ws),  h = clamp((int)rintf(hf), 1, Hs)  (ties to even);  x0 = r(9, Ws - w + 1),  y0 = r(10, Hs - h + 1)
 *     One pass with clamping: torchvision's RandomResizedCrop draws again (up to ten times, then falls back to a centre crop) where
 *     this clamps, so rectangles near the limits of scale and ratio are a little more frequent here.
 *   Status and refusals as fumi_hip_gather_images: an index outside [0, n_images) sets FUMI_ST_LABEL_RANGE and reads image 0; C in
 *   1..8, sizes >= 1, amplitudes in [0, 1] (FUMI_EINVAL otherwise); jitter with C != 3 is FUMI_ENOTSUP.  Size limit (FUMI_ENOTSUP
 *   beyond it): Hs, Ws, Ho, Wo <= 4096, C Ho Wo max(Ho, Wo) < 2^32, and one workgroup's LDS <= 160 KiB:
 *     C * (round_up_16(rows * Ws) + 16) + 112 + 4 * (Wo * mx + Ho * my + 4 * (Wo + Ho)) bytes,  rows = rect_h (fixed) | Hs (random),
 *     mx = floor(2 max(wmax / Wo, 1)) + 2 with wmax = rect_w | Ws, my likewise from rows and Ho.
 *   A 3 x 160 x 160 rectangle into 3 x 84 x 84 takes 83,008 bytes, a 3 x 224 x 224 one into 84 x 84 takes 158,080. */
#define FUMI_RESIZE_FIXED 0
#define FUMI_RESIZE_RANDOM 1
int fumi_hip_gather_images_resized(fumi_ws_t* ws, fumi_stream_t stream, const uint8_t* table, int64_t n_images, int C,
        int Hs, int Ws, int Ho, int Wo, const int64_t* idx, int64_t n_idx, const float* mean, const float* inv_std, uint64_t seed,
        uint64_t step, int stream_id, int mode, int rect_x0, int rect_y0, int rect_w, int rect_h, float scale_min, float scale_max,
        float ratio_max, int flip, float jit_brightness, float jit_contrast, float jit_saturation, float* out);

/* ---- event-free read-back of a step's scalars (replaces outer_loss.detach().cpu().numpy(), fumi/models/fumi.py:195) ----
 * One single-wave launch on `stream` stores src[0..n) (device, fp32, n <= 14) into host_pinned[0..n) and then `seq` into the
 * 64-bit word at byte offset 56 of host_pinned, all with system-scope stores: the host polls that word instead of waiting on
 * an event (an async copy + event record idles the stream for ~10 us per step).  host_pinned: 64 bytes of page-locked,
 * device-accessible host memory (hipHostMalloc / a pinned torch tensor), 8-byte aligned. */
int fumi_hip_publish_scalars(fumi_ws_t* ws, fumi_stream_t stream, const float* src, int n, void* host_pinned, uint64_t seq);
/* Deferred form: the same stores ride on the next fumi_hip_adam_step / _adamw_step / _sgd_step launch of this workspace (the optimizer
 * step that follows a training meta-step: one launch less); fumi_hip_publish_flush issues them on their own if none came.  At most
 * one publication may be pending per workspace; src must stay valid and unchanged until it has been issued. */
int fumi_hip_publish_scalars_deferred(fumi_ws_t* ws, const float* src, int n, void* host_pinned, uint64_t seq);
int fumi_hip_publish_flush(fumi_ws_t* ws, fumi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FUMI_HIP_H */
