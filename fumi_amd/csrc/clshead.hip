// Classification head of the supervised pre-training step: F.cross_entropy(feats W^T + b, y), mean over the
// M rows, with its backward, for a head over hundreds of classes.
//
//   launch 1, one workgroup per tile of 16 rows:
//       Z = feats_tile W^T + b          [16, C] on the f32 MFMA (wg_mm), kept in LDS
//       per row: first arg-max, log-sum-exp, NLL; the tile's loss / correct sums go to part[tile]
//       training form: Z <- dlogits = grad_scale / M * (softmax(Z) - onehot) in place, also written to memory for launch 2,
//                      dfeats_tile = dlogits W      (wg_mm, A read from LDS)
//   launch 2, one workgroup per [16 classes x 128 features] block of gW, each over ALL M rows (no sum across workgroups):
//       gW = dlogits^T feats,  gb = colsum(dlogits) (the workgroups of the first feature block);
//       one further workgroup adds part[0..ntile) in index order: loss = sum / M, correct = count.
//   The forward form (no gradient pointers) is launch 1 without its backward half and launch 2 with that last workgroup alone: the
//   same instructions produce loss, correct and preds in both forms.
// The heads' common contract (fixed order of every sum, first arg-max, the label rule, no floating-point atomics) is stated in
// cls_head.h, which also holds what this file shares with coshead.hip: the tile constants, ClsHead and ClsSoft, the host's checks,
// the soft-target builder and launch geometry, and the tile sums.  Still copies, here and on z = tau k in coshead.hip, each marked
// "(cls_head.h: a copy)": the row arg-max (twice here: teacher and student), the row sums, the label rule, the soft target, the
// final sum over the tiles and the column sum -- through a helper each changed an instruction stream.
//
// Soft-target form (fumi_hip_cls_head_step_soft): label smoothing eps and a two-label mix (mixup / CutMix),
//   t[m,c] = (1 - eps) (lam [c == y_a[m]] + u [c == y_b[m]]) + eps / C,  u = 1 - lam in fp32,
//   loss = mean_m (lse_m - sum_c t[m,c] z[m,c]),  dlogits = grad_scale / M * (softmax - t).
// The rows kernel is a template on SOFT: the per-row part reads z[y_b] too and, for eps > 0, forms sum_c z[c] by the strided loop and
// butterfly of the log-sum-exp; everything else, launch 2 included, is the hard form's code.  With y_b = y_a, lam = 1, eps = 0 every
// extra operation is exact (a product by 1, a sum with 0), so that call returns the hard form's bits.
//
// Distillation form (fumi_hip_cls_head_step_distill): a frozen teacher (feats_t, W_t, b_t) beside the soft target,
//   p = softmax(z_t / T), q = softmax(z / T),  kl_m = sum_c p (z_t / T) - lse(z_t / T) - sum_c p (z / T) + lse(z / T),
//   loss = ce_weight * loss_ce + alpha * T^2 mean_m kl_m,  dlogits = grad_scale / M * (ce_weight (softmax(z) - t) + alpha T (q - p)).
// The rows kernel is also a template on KD: that instance first forms the teacher's logits in the same LDS image, takes their first
// arg-max, lse(z_t / T) and sum_c p z_t / T per row and writes p to the workspace array pt [M, C], every lane the columns c = l + 16 k it
// reads back itself later; after a barrier the student's logits overwrite the image and the per-row part runs as before with two more
// strided sums.  The tile's loss_kd and agree sums take part[2 * CL_MAXTILE + tile] and part[3 * CL_MAXTILE + tile]; launch 2 is a
// template on KD only in its last workgroup.  The instances with KD = false are the code they were.  With alpha = 0, ce_weight = 1 every
// extra operation is exact, so that call returns the soft form's bits.
#include <type_traits>
#include "cls_head.h"

namespace {

struct ClsKD {                     // the teacher of the distillation form and its weights
    const float* ft; const float* Wt; const float* bt;
    float* pt;                     // [M, C] softmax(z_t / T), workspace
    float invT, aT, cw;            // 1 / T, alpha T, ce_weight
    float T2, alpha;               // T^2, alpha (launch 2)
    float* parts; float* agree;    // loss_parts [2], agree [1] (launch 2)
};
struct ClsNoKD {};

template <bool SOFT, bool KD>
__global__ __launch_bounds__(256) void cls_head_rows_kernel(ClsHead d, ClsSoft sf, const float* __restrict__ feats, const int64_t* __restrict__ y,
                                                            const float* __restrict__ W, const float* __restrict__ bias,
                                                            int64_t* __restrict__ preds, float* __restrict__ part,
                                                            float* __restrict__ dlog, float* __restrict__ dfeats, int* status,
                                                            typename std::conditional<KD, ClsKD, ClsNoKD>::type kd) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int M = d.M, F = d.F, C = d.C, ldz = d.ldz;
    const int m0 = blockIdx.x * CL_TM, rows = min(CL_TM, M - m0);
    float* Z = sm;                               // [16, ldz]
    float* rl = Z + CL_TM * ldz;                 // [16] row losses, [16] row hits (KD: [16] row KL terms, [16] rows agreeing with the teacher)
    float* mm = rl + 64;
    const float* ft = feats + (long)m0 * F;

    float kt = 0.f; int argt = 0;                // the teacher's row scalars: sum_c p (z_t - max) / T - log sum exp, first arg-max
    if constexpr (KD) {
        const float* ftt = kd.ft + (long)m0 * F;
        for (int c0 = 0; c0 < C; c0 += CL_NB) {
            const int nb = min(CL_NB, C - c0);
            wg_mm(mm, CL_MM, rows, nb, F, ftt, F, 1, kd.Wt + (long)c0 * F, 1, F,
                  [&](int m, int n, float acc) { Z[m * ldz + c0 + n] = acc + kd.bt[c0 + n]; });
        }
        __syncthreads();
        const int row = tid >> 4, l = tid & 15;
        if (row < rows) {
            const float* z = Z + row * ldz;
            float mx = -INFINITY; int arg = C;                                           // (cls_head.h: a copy, like the row sums below)
            for (int c = l; c < C; c += 16) { const float v = z[c]; if (v > mx) { mx = v; arg = c; } }
            for (int o = 8; o > 0; o >>= 1) {
                const float v2 = __shfl_xor(mx, o, 64); const int a2 = __shfl_xor(arg, o, 64);
                if (v2 > mx || (v2 == mx && a2 < arg)) { mx = v2; arg = a2; }
            }
            if (arg >= C) arg = 0;
            float s = 0.f;
            for (int c = l; c < C; c += 16) s += expf((z[c] - mx) * kd.invT);
            for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            const float inv = 1.f / s;
            float* pr = kd.pt + (long)(m0 + row) * C;
            float pz = 0.f;
            for (int c = l; c < C; c += 16) {
                const float u = (z[c] - mx) * kd.invT, p = expf(u) * inv;
                pz += p * u; pr[c] = p;                                                  // read back by this lane only
            }
            for (int o = 8; o > 0; o >>= 1) pz += __shfl_xor(pz, o, 64);
            kt = pz - logf(s); argt = arg;
        }
        __syncthreads();                         // the student's logits overwrite the image
    }

    for (int c0 = 0; c0 < C; c0 += CL_NB) {
        const int nb = min(CL_NB, C - c0);
        wg_mm(mm, CL_MM, rows, nb, F, ft, F, 1, W + (long)c0 * F, 1, F,
              [&](int m, int n, float acc) { Z[m * ldz + c0 + n] = acc + bias[c0 + n]; });
    }
    __syncthreads();

    {   // 16 lanes per row
        const int row = tid >> 4, l = tid & 15;
        float loss = 0.f, hit = 0.f;
        [[maybe_unused]] float lkd = 0.f, agr = 0.f;
        if (row < rows) {
            float* z = Z + row * ldz;
            float mx = -INFINITY; int arg = C;                                           // (cls_head.h: a copy, like the row sums, the label rule and t below)
            for (int c = l; c < C; c += 16) { const float v = z[c]; if (v > mx) { mx = v; arg = c; } }
            for (int o = 8; o > 0; o >>= 1) {
                const float v2 = __shfl_xor(mx, o, 64); const int a2 = __shfl_xor(arg, o, 64);
                if (v2 > mx || (v2 == mx && a2 < arg)) { mx = v2; arg = a2; }
            }
            if (arg >= C) arg = 0;
            float s = 0.f;
            for (int c = l; c < C; c += 16) s += expf(z[c] - mx);
            for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            long yv = y[m0 + row], yw = SOFT ? sf.yb[m0 + row] : 0;
            const bool ok = yv >= 0 && yv < C && yw >= 0 && yw < C;
            if (!ok) { if (l == 0) atomicOr(status, FUMI_ST_LABEL_RANGE); yv = 0; yw = 0; }
            if (SOFT) {
                float tz = sf.wa * z[yv] + sf.wb * z[yw];                                // sum_c t[c] z[c]
                if (sf.base > 0.f) {
                    float sz = 0.f;
                    for (int c = l; c < C; c += 16) sz += z[c];
                    for (int o = 8; o > 0; o >>= 1) sz += __shfl_xor(sz, o, 64);
                    tz += sf.base * sz;
                }
                loss = ok ? mx + logf(s) - tz : 0.f;
            } else {
                loss = ok ? mx + logf(s) - z[yv] : 0.f;
            }
            hit = (ok && arg == (int)yv) ? 1.f : 0.f;
            if (l == 0 && preds) preds[m0 + row] = arg;
            [[maybe_unused]] float invq = 0.f;
            [[maybe_unused]] const float* pr = nullptr;
            if constexpr (KD) {                                                          // the same sums at z / T, against the teacher's p
                pr = kd.pt + (long)(m0 + row) * C;
                float sq = 0.f, pz = 0.f;
                for (int c = l; c < C; c += 16) { const float u = (z[c] - mx) * kd.invT; sq += expf(u); pz += pr[c] * u; }
                for (int o = 8; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
                for (int o = 8; o > 0; o >>= 1) pz += __shfl_xor(pz, o, 64);
                lkd = ok ? kt - (pz - logf(sq)) : 0.f;
                agr = (ok && arg == argt) ? 1.f : 0.f;
                invq = 1.f / sq;
            }
            if (d.train) {
                const float inv = 1.f / s, gs = ok ? d.gs : 0.f;
                float* dl = dlog + (long)(m0 + row) * C;
                for (int c = l; c < C; c += 16) {
                    const float t = SOFT ? sf.base + (c == (int)yv ? sf.wa : 0.f) + (c == (int)yw ? sf.wb : 0.f)
                                         : (c == (int)yv ? 1.f : 0.f);
                    float g;
                    if constexpr (KD) {
                        const float q = expf((z[c] - mx) * kd.invT) * invq;
                        g = gs * (kd.cw * (expf(z[c] - mx) * inv - t) + kd.aT * (q - pr[c]));
                    } else {
                        g = gs * (expf(z[c] - mx) * inv - t);
                    }
                    z[c] = g; dl[c] = g;
                }
            }
        }
        if (l == 0) {
            rl[row] = loss; rl[16 + row] = hit;
            if constexpr (KD) { rl[32 + row] = lkd; rl[48 + row] = agr; }
        }
    }
    __syncthreads();
    cl_tile_part<2>(rl, part);                                                       // loss, correct
    if constexpr (KD) cl_tile_part<2>(rl, part, 2);                                    // KL, agree
    if (!d.train) return;
    // dfeats_tile [rows, F] = dlogits_tile [rows, C] W [C, F]
    for (int f0 = 0; f0 < F; f0 += CL_NB) {
        const int nb = min(CL_NB, F - f0);
        wg_mm(mm, CL_MM, rows, nb, C, Z, ldz, 1, W + f0, F, 1,
              [&](int m, int n, float acc) { dfeats[(long)(m0 + m) * F + f0 + n] = acc; });
    }
}

template <bool KD>
__global__ __launch_bounds__(256) void cls_head_wgrad_kernel(ClsHead d, int nfb, const float* __restrict__ feats,
                                                             const float* __restrict__ dlog, const float* __restrict__ part,
                                                             float* __restrict__ loss, float* __restrict__ correct,
                                                             float* __restrict__ gW, float* __restrict__ gb,
                                                             typename std::conditional<KD, ClsKD, ClsNoKD>::type kd) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int M = d.M, F = d.F, C = d.C;
    if (blockIdx.x == gridDim.x - 1) {           // the sums over the row tiles, in index order
        if (tid == 0) {                          // (cls_head.h: a copy)
            float a = 0.f, c = 0.f;
            for (int t = 0; t < d.ntile; ++t) { a += part[t]; c += part[CL_MAXTILE + t]; }
            if constexpr (KD) {
                float k = 0.f, g = 0.f;
                for (int t = 0; t < d.ntile; ++t) { k += part[2 * CL_MAXTILE + t]; g += part[3 * CL_MAXTILE + t]; }
                const float lce = a / (float)M, lkl = k / (float)M;
                const float lkd = kd.T2 * lkl;
                kd.parts[0] = lce; kd.parts[1] = lkd;
                loss[0] = kd.cw * lce + kd.alpha * lkd; correct[0] = c; kd.agree[0] = g;
            } else {
                loss[0] = a / (float)M; correct[0] = c;
            }
        }
        return;
    }
    const int cb = blockIdx.x / nfb, fb = blockIdx.x - cb * nfb;
    const int c0 = cb * CL_TM, f0 = fb * CL_NB;
    const int nc = min(CL_TM, C - c0), nf = min(CL_NB, F - f0);
    // gW[c0 + m, f0 + n] = sum_k dlog[k, c0 + m] feats[k, f0 + n]
    wg_mm(sm, CL_MM, nc, nf, M, dlog + c0, 1, C, feats + f0, F, 1,
          [&](int m, int n, float acc) { gW[(long)(c0 + m) * F + f0 + n] = acc; });
    if (fb != 0) return;
    __syncthreads();
    {   // gb[c0 + c] = sum_k dlog[k, c0 + c]: 16 strided partial sums per class, added in index order (cls_head.h: a copy)
        const int c = tid & 15, j = tid >> 4;
        float s = 0.f;
        if (c < nc) for (int k = j; k < M; k += 16) s += dlog[(long)k * C + c0 + c];
        sm[j * 16 + c] = s;
        __syncthreads();
        if (j == 0 && c < nc) {
            float a = 0.f;
            for (int i = 0; i < 16; ++i) a += sm[i * 16 + c];
            gb[c0 + c] = a;
        }
    }
}

}  // namespace

// all entries: soft == nullptr is the hard form, kdp != nullptr (with soft) the distillation form
static int cls_head_launch(fumi_ws_t* ws, fumi_stream_t stream, int M, int F, int C, const float* feats, const int64_t* y,
        const ClsSoft* soft, const float* W, const float* b, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* dfeats, float* gW, float* gb, const ClsKD* kdp = nullptr) {
    const int train = cl_grad_form(dfeats, gW, gb);
    if (int rc = cl_args_check(ws, M, F, C, train, {feats, y, W, b, loss, correct})) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    ClsHead d;
    cl_dims_fill(d, M, F, C, train, grad_scale);
    const int nslot = kdp ? 4 : 2;                                                   // index-ordered sums per tile
    int rc = ws_reserve(ws, ws_align((size_t)nslot * CL_MAXTILE * 4) + (train ? ws_align((size_t)M * C * 4) : 0) +
                            (kdp ? ws_align((size_t)M * C * 4) : 0));
    if (rc) return rc;
    float* part = ws_f(ws, nslot * CL_MAXTILE);
    float* dlog = train ? ws_f(ws, (size_t)M * C) : nullptr;
    const size_t lds1 = ((size_t)CL_TM * d.ldz + 64 + CL_MM) * 4, lds2 = train ? (size_t)CL_MM * 4 : 0;   // the forward form's one workgroup only adds the tile sums
    const int nfb = cl_feature_blocks(F);
    if (kdp) {
        ClsKD kd = *kdp;
        kd.pt = ws_f(ws, (size_t)M * C);
        FUMI_SET_DYN_LDS((cls_head_rows_kernel<true, true>), lds1);
        hipLaunchKernelGGL((cls_head_rows_kernel<true, true>), dim3(d.ntile), dim3(256), lds1, st, d, *soft, feats, y, W, b, preds, part,
                           dlog, dfeats, ws->status, kd);
        LAUNCH_CHECK();
        FUMI_SET_DYN_LDS(cls_head_wgrad_kernel<true>, lds2);
        hipLaunchKernelGGL(cls_head_wgrad_kernel<true>, dim3(cl_wgrad_grid(d)), dim3(256), lds2, st, d, nfb, feats, dlog, part,
                           loss, correct, gW, gb, kd);
        LAUNCH_CHECK();
        return FUMI_OK;
    }
    if (soft) {
        FUMI_SET_DYN_LDS((cls_head_rows_kernel<true, false>), lds1);
        hipLaunchKernelGGL((cls_head_rows_kernel<true, false>), dim3(d.ntile), dim3(256), lds1, st, d, *soft, feats, y, W, b, preds, part,
                           dlog, dfeats, ws->status, ClsNoKD{});
    } else {
        FUMI_SET_DYN_LDS((cls_head_rows_kernel<false, false>), lds1);
        hipLaunchKernelGGL((cls_head_rows_kernel<false, false>), dim3(d.ntile), dim3(256), lds1, st, d, ClsSoft{nullptr, 1.f, 0.f, 0.f},
                           feats, y, W, b, preds, part, dlog, dfeats, ws->status, ClsNoKD{});
    }
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(cls_head_wgrad_kernel<false>, lds2);
    hipLaunchKernelGGL(cls_head_wgrad_kernel<false>, dim3(cl_wgrad_grid(d)), dim3(256), lds2, st, d, nfb, feats, dlog, part, loss,
                       correct, gW, gb, ClsNoKD{});
    LAUNCH_CHECK();
    return FUMI_OK;
}

extern "C" int fumi_hip_cls_head_step(fumi_ws_t* ws, fumi_stream_t stream, int M, int F, int C,
        const float* feats, const int64_t* y, const float* W, const float* b, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* dfeats, float* gW, float* gb) {
    return cls_head_launch(ws, stream, M, F, C, feats, y, nullptr, W, b, grad_scale, loss, correct, preds, dfeats, gW, gb);
}

extern "C" int fumi_hip_cls_head_step_soft(fumi_ws_t* ws, fumi_stream_t stream, int M, int F, int C,
        const float* feats, const int64_t* y_a, const int64_t* y_b, float lam, float smoothing,
        const float* W, const float* b, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* dfeats, float* gW, float* gb) {
    ClsSoft soft;
    if (int rc = cl_soft_fill(soft, y_a, y_b, lam, smoothing, C)) return rc;
    return cls_head_launch(ws, stream, M, F, C, feats, y_a, &soft, W, b, grad_scale, loss, correct, preds, dfeats, gW, gb);
}

extern "C" int fumi_hip_cls_head_step_distill(fumi_ws_t* ws, fumi_stream_t stream, int M, int F, int C,
        const float* feats, const int64_t* y_a, const int64_t* y_b, float lam, float smoothing,
        const float* W, const float* b, const float* feats_t, const float* W_t, const float* b_t,
        float kd_temp, float kd_alpha, float ce_weight, float grad_scale,
        float* loss, float* loss_parts, float* correct, float* agree, int64_t* preds, float* dfeats, float* gW, float* gb) {
    if (!feats_t || !W_t || !b_t || !loss_parts || !agree) return FUMI_EINVAL;
    auto finite = [](float v) { return v - v == 0.f; };                             // neither NaN nor an infinity
    if (!finite(kd_temp) || !finite(kd_alpha) || !finite(ce_weight) || !(kd_temp > 0.f) || kd_alpha < 0.f || ce_weight < 0.f ||
        !finite(1.f / kd_temp) || !finite(kd_alpha * kd_temp * kd_temp))
        return FUMI_EINVAL;
    ClsSoft soft;
    if (int rc = cl_soft_fill(soft, y_a, y_b, lam, smoothing, C)) return rc;
    ClsKD kd;
    kd.ft = feats_t; kd.Wt = W_t; kd.bt = b_t; kd.pt = nullptr;
    kd.invT = 1.f / kd_temp; kd.aT = kd_alpha * kd_temp; kd.cw = ce_weight; kd.T2 = kd_temp * kd_temp; kd.alpha = kd_alpha;
    kd.parts = loss_parts; kd.agree = agree;
    return cls_head_launch(ws, stream, M, F, C, feats, y_a, &soft, W, b, grad_scale, loss, correct, preds, dfeats, gW, gb, &kd);
}
