// Host code shared by the entry points of the meta-steps (api.hip, conv4.hip, rn12.hip): the hypernetwork head as plain GEMMs, the
// problem front of the two image-encoder steps and the statistics tail.  No kernels: everything launches through common.h.
#pragma once
#include "common.h"
#include <string.h>

// ---- the hypernetwork head (fumi.py:70-86,104-113): rows are (episode, class) pairs ---------------------------------------------
//     u = relu(ctext A0^T + b0),  h = [tanh](u A1^T + b1),  phi = {A0 [Ht,Dt], b0 [Ht], A1 [H1,Ht], b1 [H1]}
struct HyperHead {
    int R, Dt, Ht, H1, tanh_head;             // R = B * N rows, H1 = feature width + 1
    const float* const* phi;
    float *c, *u, *ub, *h, *hbar, *hpb;       // class text rows [R,Dt] | u, ubar [R,Ht] | h, hbar, tanh'(h) hbar [R,H1]
    const float* ctext;                       // the rows the head reads: the caller's cls_text, or c once it has been selected into
};
// Buffer layout: c, u, ub, h, hbar, hpb one after the other, each rounded up to 64 floats -- the 256 bytes of ws_align, so a carve
// from the workspace slab and one from a float allocation (ResNet-12: ws->side_buf) are the same layout.
constexpr size_t head_al(size_t n) { return (n + 63) / 64 * 64; }
static_assert(ws_align(sizeof(float)) == head_al(1) * sizeof(float), "the head's carve rounds as ws_align does");
static inline size_t hyper_head_floats(int R, int Dt, int Ht, int H1) {
    return head_al((size_t)R * Dt) + 2 * head_al((size_t)R * Ht) + 3 * head_al((size_t)R * H1);
}
static inline HyperHead hyper_head_carve(float* base, int R, int Dt, int Ht, int H1, int tanh_head, const float* const* phi,
                                         const float* cls_text) {
    HyperHead hd = {R, Dt, Ht, H1, tanh_head, phi, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, cls_text};
    auto take = [&](size_t n) { float* q = base; base += head_al(n); return q; };
    hd.c = take((size_t)R * Dt); hd.u = take((size_t)R * Ht); hd.ub = take((size_t)R * Ht);
    hd.h = take((size_t)R * H1); hd.hbar = take((size_t)R * H1); hd.hpb = take((size_t)R * H1);
    return hd;
}
static inline bool hyper_head_args_ok(const float* const* phi, float* const* g_phi, int need_grad) {
    if (!phi || (need_grad && !g_phi)) return false;
    for (int i = 0; i < 4; ++i) if (!phi[i] || (need_grad && !g_phi[i])) return false;
    return true;
}
static inline int hyper_head_fwd_gemm(hipStream_t st, const HyperHead& hd) {
    GemmArgs g = gemm_args(hd.R, hd.Ht, hd.Dt, hd.ctext, hd.Dt, hd.phi[0], hd.Dt, hd.u, hd.Ht);
    g.bias = hd.phi[1]; g.act = 1;
    if (int rc = launch_gemm(st, g, 0, 0)) return rc;
    g = gemm_args(hd.R, hd.H1, hd.Ht, hd.u, hd.Ht, hd.phi[2], hd.Ht, hd.h, hd.H1);
    g.bias = hd.phi[3]; g.act = hd.tanh_head ? 2 : 0;
    return launch_gemm(st, g, 0, 0);
}
// d(scale * sum_b loss_b) / d ctext = scale * ubar A0  [R,Dt]   (needs ubar in hd.ub: every form of the backward leaves it there)
static inline int hyper_head_text_grad_gemm(hipStream_t st, const HyperHead& hd, float grad_scale, float* text_grad) {
    GemmArgs g = gemm_args(hd.R, hd.Dt, hd.Ht, hd.ub, hd.Ht, hd.phi[0], hd.Dt, text_grad, hd.Dt);
    g.alpha = grad_scale;
    return launch_gemm(st, g, 0, 1);
}
// From hd.hbar = d loss_b / d h (unscaled), in ONE launch order at every site:
//     tanh' -> gA1 -> colsum g_b1 -> ubar (ReLU mask in the epilogue) -> gA0 -> text gradient (when wanted) -> colsum g_b0.
// text_grad (may be NULL) is the step's g_cls_text buffer [R,Dt].
static inline int hyper_head_bwd_gemm(hipStream_t st, const HyperHead& hd, float grad_scale, float* const* g_phi, float* text_grad) {
    const float* hp = hd.hbar;
    int rc;
    if (hd.tanh_head) { if ((rc = launch_tanh_bwd(st, (long)hd.R * hd.H1, hd.h, hd.hbar, hd.hpb))) return rc; hp = hd.hpb; }
    GemmArgs g = gemm_args(hd.H1, hd.Ht, hd.R, hp, hd.H1, hd.u, hd.Ht, g_phi[2], hd.Ht);      // gA1 = hp^T u
    g.alpha = grad_scale;
    if ((rc = launch_gemm(st, g, 1, 1))) return rc;
    if ((rc = launch_colsum(st, hp, hd.R, hd.H1, hd.H1, grad_scale, g_phi[3]))) return rc;
    g = gemm_args(hd.R, hd.Ht, hd.H1, hp, hd.H1, hd.phi[2], hd.Ht, hd.ub, hd.Ht);             // ubar = (hp A1) * relu'(u)
    g.mask = hd.u;
    if ((rc = launch_gemm(st, g, 0, 1))) return rc;
    g = gemm_args(hd.Ht, hd.Dt, hd.R, hd.ub, hd.Ht, hd.ctext, hd.Dt, g_phi[0], hd.Dt);        // gA0 = ubar^T c
    g.alpha = grad_scale;
    if ((rc = launch_gemm(st, g, 1, 1))) return rc;
    if (text_grad && (rc = hyper_head_text_grad_gemm(st, hd, grad_scale, text_grad))) return rc;
    return launch_colsum(st, hd.ub, hd.R, hd.Ht, hd.Ht, grad_scale, g_phi[1]);
}

// ---- problem front of the image-encoder meta-steps --------------------------------------------------------------------------------
constexpr int ENC_MAXTHETA = 48;              // ResNet-12: 12 tensors x 4 blocks (Conv4: 3 x 4)
struct EncProblem {
    int B, N, S, Qn, Cin, H, W, nblk, T;
    float alpha, grad_scale;
    int need_grad, second_order;
    const float* x_s; const int64_t* y_s; const float* x_q; const int64_t* y_q;
    const float* theta[ENC_MAXTHETA];         // per_block tensors per block, torch layouts
    float* g_theta[ENC_MAXTHETA];
    const float* head;                        // [B][N][F+1]
    float* head_bar;                          // [B][N][F+1] d loss_b / d head_b (unscaled)
    float* logits_q; int64_t* preds_q; float* preds_f; float* loss_b; float* acc_b; float* stats;
};
static inline int enc_fill_problem(EncProblem& p, int per_block, int max_blk, int B, int N, int S, int Qn, int Cin, int H, int W,
                                   int nblk, int T, float alpha, int need_grad, int second_order, float grad_scale, const float* x_s,
                                   const int64_t* y_s, const float* x_q, const int64_t* y_q, const float* const* theta, float* logits_q,
                                   int64_t* preds_q, float* preds_f, float* loss_b, float* acc_b, float* stats, float* const* g_theta) {
    memset(&p, 0, sizeof(EncProblem));
    if (!x_s || !y_s || !x_q || !y_q || !theta || !logits_q || !preds_q || !loss_b || !acc_b) return FUMI_EINVAL;
    if (nblk < 1 || nblk > max_blk || per_block * nblk > ENC_MAXTHETA || (need_grad && !g_theta)) return FUMI_EINVAL;
    p.B = B; p.N = N; p.S = S; p.Qn = Qn; p.Cin = Cin; p.H = H; p.W = W; p.nblk = nblk; p.T = T; p.alpha = alpha;
    p.grad_scale = grad_scale; p.need_grad = need_grad ? 1 : 0; p.second_order = second_order ? 1 : 0;
    p.x_s = x_s; p.y_s = y_s; p.x_q = x_q; p.y_q = y_q;
    for (int i = 0; i < per_block * nblk; ++i) {
        if (!theta[i] || (need_grad && !g_theta[i])) return FUMI_EINVAL;
        p.theta[i] = theta[i]; p.g_theta[i] = need_grad ? g_theta[i] : nullptr;
    }
    p.logits_q = logits_q; p.preds_q = preds_q; p.preds_f = preds_f; p.loss_b = loss_b; p.acc_b = acc_b; p.stats = stats;
    return FUMI_OK;
}

// ---- statistics tail: stats[0] = scale * sum_b loss_b, stats[1] = scale * sum_b acc_b (nothing when stats is NULL) ------------------
static inline int launch_episode_stats(hipStream_t st, int B, const float* loss_b, const float* acc_b, float scale, float* stats) {
    if (!stats) return FUMI_OK;
    ReduceSegs sg; sg.n = 0; sg.scale = scale;
    sg.add(loss_b, B, 1, 1, stats); sg.add(acc_b, B, 1, 1, stats + 1);
    return launch_reduce_multi(st, sg);
}
