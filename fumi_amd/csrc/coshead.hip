// Cosine classifier head of the supervised pre-training step (--pretrain_head cosine): the classifier the
// backbone is trained with when the few-shot stage that follows compares directions (Gidaris & Komodakis 2018, Baseline++).  With
//   u_m = feats_m / max(|feats_m|, eps),  v_c = W_c / max(|W_c|, eps),  eps = 1e-12 (norms in fp32),  k[m,c] = u_m . v_c,
//   z = tau k (no bias),  t = the soft target of fumi_hip_cls_head_step_soft,
//   loss = mean_m (lse(z_m) - sum_c t z),  dz = grad_scale / M * (softmax(z) - t),
//   dtau     = sum_{m,c} dz k,
//   dfeats_m = tau / |feats_m| * (sum_c dz[m,c] v_c - r_m u_m),   r_m = sum_c dz[m,c] k[m,c],
//   gW_c     = tau / |W_c|     * (sum_m dz[m,c] u_m - q_c v_c),   q_c = sum_m dz[m,c] k[m,c].
//
//   launch 0, one wave per row of W (C rows) and of feats (M rows): rn = 1 / |row|, the squares added in a fixed order (a lane's
//       float4s in index order, then a butterfly over the 64 lanes).  A row whose norm is below eps gets rn = 0: it is the zero
//       direction, k = 0 along it and its gradient row is exactly zero, and no 1 / eps ever multiplies anything.
//   launch 1, one workgroup per tile of 16 rows (the linear head's, csrc/clshead.hip):
//       K = (feats_tile W^T) rf[m] rw[c]     [16, C] on the f32 MFMA (wg_mm), kept in LDS; z = tau K is formed where it is read
//       per row: first arg-max, log-sum-exp, soft target; the tile's loss / correct sums go to part[tile]
//       training form: per row r_m = sum_c dz k (the strided loop and butterfly of the log-sum-exp); dz rf[m] and dz k go to memory
//                      for launch 2; the image becomes dz rw[c], dfeats_tile = tau rf[m] (image . W - r_m u_m) (wg_mm2: the
//                      feats element of the epilogue is loaded before the product); the tile's sum of r_m goes to part[2, tile]
//   launch 2, one workgroup per [16 classes x 128 features] block of gW, each over ALL M rows:
//       q_c = colsum(dz k) of its 16 classes (16 strided partial sums per class, added in index order), then
//       gW = tau rw[c] ((dz rf)^T feats - q_c v_c), the W element of the epilogue loaded before the product;
//       one further workgroup adds part[0..ntile) in index order: loss, correct, dtau.
//   The forward form (no gradient pointers) is launches 0 and 1 without the backward half and that last workgroup alone.
// The heads' common contract (fixed order of every sum, first arg-max, the label rule, no floating-point atomics) is stated in
// cls_head.h; the launches hand over through memory.
//
// Shared with the linear heads, in cls_head.h: the tile constants, the dims and soft-target fields of CosHead, the host's checks, the
// soft-target builder and launch geometry, and the tile sums.  Still copies of the linear head's lines, on z = tau k, each marked
// "(cls_head.h: a copy)": the row arg-max, the log-sum-exp and sum_c z, the label rule, the soft target, the final sum over the tiles
// and the column sum q_c -- through a helper each changed this file's or clshead.hip's instruction streams.
// Departures from the plan of the issue:
//   * q_c comes from a second workspace array (dz k), not from a stored k: either way launch 1 writes and launch 2 reads one more
//     [M, C] array, and the stored product saves launch 2 the multiplication and the second read of dz.
//   * there is one instance of the rows kernel, the soft one: with y_b = y_a, lam = 1, smoothing = 0 its extra operations are exact
//     (a product by 1, a sum with 0), which csrc/clshead.hip already relies on.
#include "cls_head.h"

namespace {

constexpr float KH_EPS = 1e-12f;

struct CosHead : ClsHead { ClsSoft sf; };   // the kernels' one argument: the layout it always had

// rn[0, C) = 1 / |W_c|, rn[C, C + M) = 1 / |feats_m|; 0 where the norm is below eps
__global__ __launch_bounds__(256) void cos_head_norm_kernel(int M, int F, int C, const float* __restrict__ feats,
                                                            const float* __restrict__ W, float* __restrict__ rn) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= C + M) return;                                                        // wave-uniform
    const float* src = row < C ? W + (long)row * F : feats + (long)(row - C) * F;
    float s = 0.f;
    if ((((uintptr_t)src) & 15) == 0) {
        const f32x4* p = (const f32x4*)src;
        for (int i = lane; i < (F >> 2); i += 64) { const f32x4 v = p[i]; s += v[0] * v[0]; s += v[1] * v[1]; s += v[2] * v[2]; s += v[3] * v[3]; }
    } else {                                                                         // (a view that starts off a 16-byte boundary)
        for (int i = lane; i < F; i += 64) s += src[i] * src[i];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float n = sqrtf(s);
    if (lane == 0) rn[row] = n >= KH_EPS ? 1.f / n : 0.f;
}

__global__ __launch_bounds__(256) void cos_head_rows_kernel(CosHead d, const float* __restrict__ feats, const int64_t* __restrict__ y,
                                                            const float* __restrict__ W, const float* __restrict__ taup,
                                                            const float* __restrict__ rn, int64_t* __restrict__ preds,
                                                            float* __restrict__ part, float* __restrict__ da, float* __restrict__ dk,
                                                            float* __restrict__ dfeats, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int M = d.M, F = d.F, C = d.C, ldz = d.ldz;
    const int m0 = blockIdx.x * CL_TM, rows = min(CL_TM, M - m0);
    float* Z = sm;                               // [16, ldz]: k, then dz rw[c]
    float* rl = Z + CL_TM * ldz;                 // [16] row losses, [16] row hits, [16] r_m, [16] rf
    float* rws = rl + 64;                        // [ldz] rw
    float* mm = rws + ldz;
    const float* ft = feats + (long)m0 * F;
    const float tau = taup[0];

    for (int c = tid; c < C; c += 256) rws[c] = rn[c];
    if (tid < CL_TM) rl[48 + tid] = tid < rows ? rn[C + m0 + tid] : 0.f;
    __syncthreads();

    for (int c0 = 0; c0 < C; c0 += CL_NB) {
        const int nb = min(CL_NB, C - c0);
        wg_mm(mm, CL_MM, rows, nb, F, ft, F, 1, W + (long)c0 * F, 1, F,
              [&](int m, int n, float acc) { Z[m * ldz + c0 + n] = acc * rl[48 + m] * rws[c0 + n]; });
    }
    __syncthreads();

    {   // 16 lanes per row
        const int row = tid >> 4, l = tid & 15;
        float loss = 0.f, hit = 0.f, rsum = 0.f;
        if (row < rows) {
            float* z = Z + row * ldz;
            float mx = -INFINITY; int arg = C;                                           // (cls_head.h: a copy, like the row sums, the label rule and t below)
            for (int c = l; c < C; c += 16) { const float v = tau * z[c]; if (v > mx) { mx = v; arg = c; } }
            for (int o = 8; o > 0; o >>= 1) {
                const float v2 = __shfl_xor(mx, o, 64); const int a2 = __shfl_xor(arg, o, 64);
                if (v2 > mx || (v2 == mx && a2 < arg)) { mx = v2; arg = a2; }           // first arg-max (torch.max)
            }
            if (arg >= C) arg = 0;                                                       // (a row of NaNs)
            float s = 0.f;
            for (int c = l; c < C; c += 16) s += expf(tau * z[c] - mx);
            for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            long yv = y[m0 + row], yw = d.sf.yb[m0 + row];
            const bool ok = yv >= 0 && yv < C && yw >= 0 && yw < C;
            if (!ok) { if (l == 0) atomicOr(status, FUMI_ST_LABEL_RANGE); yv = 0; yw = 0; }
            float tz = d.sf.wa * (tau * z[yv]) + d.sf.wb * (tau * z[yw]);                      // sum_c t[c] z[c]
            if (d.sf.base > 0.f) {
                float sz = 0.f;
                for (int c = l; c < C; c += 16) sz += tau * z[c];
                for (int o = 8; o > 0; o >>= 1) sz += __shfl_xor(sz, o, 64);
                tz += d.sf.base * sz;
            }
            loss = ok ? mx + logf(s) - tz : 0.f;
            hit = (ok && arg == (int)yv) ? 1.f : 0.f;
            if (l == 0 && preds) preds[m0 + row] = arg;
            if (d.train) {
                const float inv = 1.f / s, gs = ok ? d.gs : 0.f, rfm = rl[48 + row];
                float* ar = da + (long)(m0 + row) * C;
                float* kr = dk + (long)(m0 + row) * C;
                for (int c = l; c < C; c += 16) {
                    const float k = z[c];
                    const float t = d.sf.base + (c == (int)yv ? d.sf.wa : 0.f) + (c == (int)yw ? d.sf.wb : 0.f);
                    const float g = gs * (expf(tau * k - mx) * inv - t), gk = g * k;
                    rsum += gk;
                    z[c] = g * rws[c]; ar[c] = g * rfm; kr[c] = gk;
                }
                for (int o = 8; o > 0; o >>= 1) rsum += __shfl_xor(rsum, o, 64);
            }
        }
        if (l == 0) { rl[row] = loss; rl[16 + row] = hit; rl[32 + row] = rsum; }
    }
    __syncthreads();
    cl_tile_part<3>(rl, part);                                                       // loss, correct, r_m
    if (!d.train) return;
    // dfeats_tile [rows, F] = tau rf[m] ((dz rw) [rows, C] W [C, F] - r_m u_m)
    for (int f0 = 0; f0 < F; f0 += CL_NB) {
        const int nb = min(CL_NB, F - f0);
        wg_mm2(mm, CL_MM, rows, nb, C, Z, ldz, 1, W + f0, F, 1,
               [&](int m, int n) { return ft[(long)m * F + f0 + n]; },
               [&](int m, int n, float acc, float x) {
                   const float rfm = rl[48 + m];
                   dfeats[(long)(m0 + m) * F + f0 + n] = (tau * rfm) * (acc - rl[32 + m] * (x * rfm));
               });
    }
}

__global__ __launch_bounds__(256) void cos_head_wgrad_kernel(CosHead d, int nfb, const float* __restrict__ feats, const float* __restrict__ W,
                                                             const float* __restrict__ taup, const float* __restrict__ rn,
                                                             const float* __restrict__ da, const float* __restrict__ dk,
                                                             const float* __restrict__ part, float* __restrict__ loss,
                                                             float* __restrict__ correct, float* __restrict__ gW, float* __restrict__ dtau) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int M = d.M, F = d.F, C = d.C;
    if (blockIdx.x == gridDim.x - 1) {           // the sums over the row tiles, in index order
        if (tid == 0) {                          // (cls_head.h: a copy)
            float a = 0.f, c = 0.f, r = 0.f;
            for (int t = 0; t < d.ntile; ++t) { a += part[t]; c += part[CL_MAXTILE + t]; r += part[2 * CL_MAXTILE + t]; }
            loss[0] = a / (float)M; correct[0] = c;
            if (d.train) dtau[0] = r;
        }
        return;
    }
    const int cb = blockIdx.x / nfb, fb = blockIdx.x - cb * nfb;
    const int c0 = cb * CL_TM, f0 = fb * CL_NB;
    const int nc = min(CL_TM, C - c0), nf = min(CL_NB, F - f0);
    float* ql = sm + CL_MM;                      // [16, 16] partial sums, [16] q_c, [16] rw
    const float tau = taup[0];
    {   // q[c] = sum_k dk[k, c0 + c]: 16 strided partial sums per class, added in index order (cls_head.h: a copy)
        const int c = tid & 15, j = tid >> 4;
        float s = 0.f;
        if (c < nc) for (int k = j; k < M; k += 16) s += dk[(long)k * C + c0 + c];
        ql[j * 16 + c] = s;
        __syncthreads();
        if (j == 0) {
            float a = 0.f;
            for (int i = 0; i < 16; ++i) a += ql[i * 16 + c];
            ql[256 + c] = a; ql[272 + c] = c < nc ? rn[c0 + c] : 0.f;
        }
        __syncthreads();
    }
    // gW[c0 + m, f0 + n] = tau rw[c] (sum_k da[k, c0 + m] feats[k, f0 + n] - q_c v_c)
    wg_mm2(sm, CL_MM, nc, nf, M, da + c0, 1, C, feats + f0, F, 1,
           [&](int m, int n) { return W[(long)(c0 + m) * F + f0 + n]; },
           [&](int m, int n, float acc, float w) {
               const float rwc = ql[272 + m];
               gW[(long)(c0 + m) * F + f0 + n] = (tau * rwc) * (acc - ql[256 + m] * (w * rwc));
           });
}

}  // namespace

extern "C" int fumi_hip_cos_cls_head_step(fumi_ws_t* ws, fumi_stream_t stream, int M, int F, int C,
        const float* feats, const int64_t* y_a, const int64_t* y_b, float lam, float smoothing,
        const float* W, const float* tau, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* dfeats, float* gW, float* dtau) {
    CosHead d;
    if (int rc = cl_soft_fill(d.sf, y_a, y_b, lam, smoothing, C)) return rc;
    const int train = cl_grad_form(dfeats, gW, dtau);
    if (int rc = cl_args_check(ws, M, F, C, train, {feats, y_a, W, tau, loss, correct})) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    cl_dims_fill(d, M, F, C, train, grad_scale);
    int rc = ws_reserve(ws, ws_align((size_t)3 * CL_MAXTILE * 4) + ws_align((size_t)(C + M) * 4) +
                            (train ? 2 * ws_align((size_t)M * C * 4) : 0));
    if (rc) return rc;
    float* part = ws_f(ws, 3 * CL_MAXTILE);
    float* rn = ws_f(ws, (size_t)C + M);
    float* da = train ? ws_f(ws, (size_t)M * C) : nullptr;
    float* dk = train ? ws_f(ws, (size_t)M * C) : nullptr;
    const size_t lds1 = ((size_t)CL_TM * d.ldz + 64 + d.ldz + CL_MM) * 4;
    const size_t lds2 = train ? (size_t)(CL_MM + 288) * 4 : 0;                      // the forward form's one workgroup only adds the tile sums
    hipLaunchKernelGGL(cos_head_norm_kernel, dim3((C + M + 3) / 4), dim3(256), 0, st, M, F, C, feats, W, rn);
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(cos_head_rows_kernel, lds1);
    hipLaunchKernelGGL(cos_head_rows_kernel, dim3(d.ntile), dim3(256), lds1, st, d, feats, y_a, W, tau, rn, preds, part, da, dk, dfeats,
                       ws->status);
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(cos_head_wgrad_kernel, lds2);
    hipLaunchKernelGGL(cos_head_wgrad_kernel, dim3(cl_wgrad_grid(d)), dim3(256), lds2, st, d, cl_feature_blocks(F), feats, W, tau, rn, da, dk,
                       part, loss, correct, gW, dtau);
    LAUNCH_CHECK();
    return FUMI_OK;
}
