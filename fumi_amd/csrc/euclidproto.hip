// Prototypical-network head with a metric scale (Snell et al. 2017; --fewshot_head proto): per episode
//     c_n = mean of the support rows of class n,   d2[q,n] = |f_q - c_n|^2,   z = -alpha d2,
// mean softmax cross-entropy of z over all B * Qn query rows, first arg-max predictions, and the gradients of grad_scale * loss with
// respect to the query rows, the support rows and alpha.  The [B,Qn,N,F] difference tensor is never formed: the distances come from
// one product per row tile.  A plain |f|^2 - 2 f.c + |c|^2 expansion loses the distance under the squares when the features share an
// offset (post-ReLU features do), so every vector is taken relative to the episode's mean prototype m = (1/N) sum_n c_n first:
//     c'_n = c_n - m,   f'_q = f_q - m,   d2 = |f'_q|^2 - 2 (f_q . c'_n - m . c'_n) + |c'_n|^2,
// which is the same number in exact arithmetic for any m, and whose three terms are of the size of d2 itself for this one.
//
//   launch 1, one workgroup per (episode, block of 256 features): class sums in LDS, one column per thread, support rows added in
//       index order (the order of fumi_hip_proto_reduce); every class of a column is then in LDS, so the thread takes their mean m,
//       writes c'_n and m, and the block writes its sums of c'_n[f]^2 and m[f] c'_n[f], and the class counts.
//   launch 2, one workgroup per (episode, tile of 16 query rows): |f_q - m|^2 formed from the differences (16 lanes per row), |c'_n|^2
//       and m . c'_n from the block sums in index order, f_tile C'^T on the f32 MFMA (wg_mm), d2 kept in LDS; per row first arg-max,
//       log-sum-exp, NLL; the tile's loss / correct / dalpha sums go to part[tile].  Training form: with
//       dz = grad_scale / (B Qn) (softmax - onehot),
//           dfeats_q = 2 alpha dz C'                                  (wg_mm, A read from LDS)
//       -- sum_n dz[q,n] (c_n - f_q) with the term f'_q sum_n dz[q,n] left out: the sum is zero but for round-off -- and dz goes to
//       memory for launch 3.  dalpha = -sum dz (d2 - min_n d2), the same sum for the same reason, without the common part of the row.
//   launch 3, one workgroup per (episode, 16 classes, 128 features), each over ALL Qn rows (no sum across workgroups):
//           dc_n = 2 alpha ((dz^T F_q)_n - (c'_n + m) sum_q dz[q,n])  (wg_mm2)
//       scattered to the support rows of class n as dc_n / count_n; one further workgroup adds part[0..ntile): loss, correct, dalpha.
//   The forward form (no gradient pointers) is launch 1, launch 2 without its backward half and the last workgroup of launch 3: the
//   same instructions produce loss, correct, preds and logits in both forms.
// Fixed summation orders, the first arg-max, the label-range and missing-class rules and the absence of floating-point atomics are
// those of fewshot_head.h.  A support row left out gets a zero gradient, a class without a support row a zero prototype (it counts
// as such in m).  alpha is read from device memory by the kernels.
#include "fewshot_head.h"

namespace {

__global__ __launch_bounds__(256) void euclid_proto_means_kernel(HeadDims d, const float* __restrict__ xs,
                                                                 const int64_t* __restrict__ ys, float* __restrict__ protos,
                                                                 float* __restrict__ mvec, float* __restrict__ psq,
                                                                 float* __restrict__ cntf, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, N = d.N, F = d.F;
    const int b = blockIdx.x / d.nfb1, fb = blockIdx.x - b * d.nfb1;
    float* acc = sm;                             // [N, 256] class sums, then means, then c'
    float* mcol = acc + N * FH_PF;               // [256] the mean prototype of each column
    int* lab = (int*)(mcol + FH_PF);             // [S] labels, -1 where out of range
    int* cnt = lab + S;                          // [N]
    const bool bad = fh_stage_labels(ys + (long)b * S, S, N, lab);
    if (bad && fb == 0) atomicOr(status, FUMI_ST_LABEL_RANGE);
    for (int i = tid; i < N * FH_PF; i += 256) acc[i] = 0.f;
    __syncthreads();
    fh_proto_counts(lab, S, N, cnt, cntf, b, fb == 0, status);
    const int f = fb * FH_PF + tid;
    if (f < F) fh_class_sums(acc, lab, xs + (long)b * S * F + f, S, F);
    __syncthreads();
    float m = 0.f;
    if (f < F) {
        for (int n = 0; n < N; ++n) {            // the means, and their mean over the classes in index order
            const float c = acc[n * FH_PF + tid] / (float)cnt[n];
            acc[n * FH_PF + tid] = c;
            m += c;
        }
        m /= (float)N;
        for (int n = 0; n < N; ++n) {
            const float c = acc[n * FH_PF + tid] - m;
            acc[n * FH_PF + tid] = c;
            protos[((long)b * N + n) * F + f] = c;
        }
        mvec[(long)b * F + f] = m;
    }
    mcol[tid] = m;
    __syncthreads();
    {   // sum_f c'_n[f]^2 and sum_f m[f] c'_n[f] over this block's columns (columns past F hold 0): one wave per class
        const int wave = tid >> 6, lane = tid & 63;
        for (int n = wave; n < N; n += 4) {
            float s = 0.f, t = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float v = acc[n * FH_PF + lane + 64 * j]; s += v * v; t += v * mcol[lane + 64 * j]; }
            for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); t += __shfl_xor(t, o, 64); }
            if (lane == 0) {
                psq[(((long)b * d.nfb1 + fb) * 2) * N + n] = s;
                psq[(((long)b * d.nfb1 + fb) * 2 + 1) * N + n] = t;
            }
        }
    }
}

__global__ __launch_bounds__(256) void euclid_proto_rows_kernel(HeadDims d, const float* __restrict__ fq,
                                                                const int64_t* __restrict__ yq, const float* __restrict__ protos,
                                                                const float* __restrict__ mvec, const float* __restrict__ psq,
                                                                const float* __restrict__ alpha_p, int64_t* __restrict__ preds,
                                                                float* __restrict__ logits, float* __restrict__ part,
                                                                float* __restrict__ Wd, float* __restrict__ dfq, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int Qn = d.Qn, N = d.N, F = d.F, ldz = d.ldz;
    const int b = blockIdx.x / d.tpe, q0 = (blockIdx.x - b * d.tpe) * FH_TM, rows = min(FH_TM, Qn - q0);
    const long r0 = (long)b * Qn + q0;           // the tile's first row among all B * Qn
    float* Z = sm;                               // [16, ldz] d2, then dz
    float* qs = Z + FH_TM * ldz;                 // [16] |f_q - m|^2
    float* rl = qs + 16;                         // [16] row losses, [16] row hits, [16] row dalpha
    float* cn = rl + 48;                         // [64] |c'_n|^2
    float* mc = cn + 64;                         // [64] m . c'_n
    float* mm = mc + 64;
    const float* ft = fq + r0 * F;
    const float* pc = protos + (long)b * N * F;
    const float* mv = mvec + (long)b * F;
    const float alpha = alpha_p[0];
    const int row = tid >> 4, l = tid & 15;      // 16 lanes per row

    {
        float s = 0.f;
        if (row < rows) {
            const float* x = ft + (long)row * F;
            if ((((uintptr_t)x) & 15) == 0 && (((uintptr_t)mv) & 15) == 0) {
                const f32x4* x4 = (const f32x4*)x;
                const f32x4* m4 = (const f32x4*)mv;
                for (int k = l; k < (F >> 2); k += 16) {
                    const f32x4 v = x4[k] - m4[k];
                    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
                }
            } else {
                for (int k = l; k < F; k += 16) { const float v = x[k] - mv[k]; s += v * v; }
            }
        }
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (l == 0) qs[row] = s;
    }
    if (tid < N) {
        float s = 0.f, t = 0.f;
        for (int k = 0; k < d.nfb1; ++k) {
            s += psq[(((long)b * d.nfb1 + k) * 2) * N + tid];
            t += psq[(((long)b * d.nfb1 + k) * 2 + 1) * N + tid];
        }
        cn[tid] = s; mc[tid] = t;
    }
    __syncthreads();
    wg_mm(mm, FH_MM, rows, N, F, ft, F, 1, pc, 1, F,
          [&](int m, int n, float acc) { Z[m * ldz + n] = (qs[m] + cn[n]) - 2.f * (acc - mc[n]); });
    __syncthreads();

    {
        float loss = 0.f, hit = 0.f, da = 0.f;
        if (row < rows) {
            float* c = Z + row * ldz;
            float ds[4], z[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; ds[j] = n < N ? c[n] : 0.f; z[j] = -alpha * ds[j]; }
            // The row's softmax cross-entropy, the same block in the four rows kernels.  It stays a copy: through helper functions (a
            // softmax helper alone included) the compiler allocates this kernel's registers differently and the training heads measured
            // 0.2 - 0.7 % slower.  A change to the arg-max, the label rule or the NLL is made in all four.
            float mx = -INFINITY; int arg = N;
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; if (n < N && z[j] > mx) { mx = z[j]; arg = n; } }
            for (int o = 8; o > 0; o >>= 1) {
                const float v2 = __shfl_xor(mx, o, 64); const int a2 = __shfl_xor(arg, o, 64);
                if (v2 > mx || (v2 == mx && a2 < arg)) { mx = v2; arg = a2; }           // first arg-max (torch.max)
            }
            if (arg >= N) arg = 0;                                                       // (a row of NaNs)
            float e[4], s = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) { e[j] = l + 16 * j < N ? expf(z[j] - mx) : 0.f; s += e[j]; }
            for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            long yv = yq[r0 + row];
            const bool ok = yv >= 0 && yv < N;
            if (!ok) { if (l == 0) atomicOr(status, FUMI_ST_LABEL_RANGE); yv = 0; }
            loss = ok ? mx + logf(s) + alpha * c[yv] : 0.f;
            hit = (ok && arg == (int)yv) ? 1.f : 0.f;
            if (l == 0 && preds) preds[r0 + row] = arg;
            if (logits) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; if (n < N) logits[(r0 + row) * N + n] = z[j]; }
            }
            if (d.train) {
                float dm = INFINITY;                                                     // the row's smallest d2
#pragma unroll
                for (int j = 0; j < 4; ++j) if (l + 16 * j < N) dm = fminf(dm, ds[j]);
                for (int o = 8; o > 0; o >>= 1) dm = fminf(dm, __shfl_xor(dm, o, 64));
                const float inv = 1.f / s, gs = ok ? d.gs : 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = l + 16 * j;
                    if (n < N) {
                        const float g = gs * (e[j] * inv - (n == (int)yv ? 1.f : 0.f));   // dz
                        da -= g * (ds[j] - dm);
                        Wd[(r0 + row) * N + n] = g;
                        c[n] = g;
                    }
                }
                for (int o = 8; o > 0; o >>= 1) da += __shfl_xor(da, o, 64);
            }
        }
        if (l == 0) { rl[row] = loss; rl[16 + row] = hit; rl[32 + row] = da; }
    }
    __syncthreads();
    fh_tile_part<3>(rl, part, d.ntile);
    if (!d.train) return;
    // dfeats_tile [rows, F] = 2 alpha dz [rows, N] C' [N, F]
    const float a2 = 2.f * alpha;
    for (int f0 = 0; f0 < F; f0 += FH_NB) {
        const int nb = min(FH_NB, F - f0);
        wg_mm(mm, FH_MM, rows, nb, N, Z, ldz, 1, pc + f0, F, 1,
              [&](int m, int n, float acc) { dfq[(r0 + m) * F + f0 + n] = a2 * acc; });
    }
}

__global__ __launch_bounds__(256) void euclid_proto_sgrad_kernel(HeadDims d, int nfb, int ncb, const float* __restrict__ fq,
                                                                 const int64_t* __restrict__ ys, const float* __restrict__ protos,
                                                                 const float* __restrict__ mvec, const float* __restrict__ cntf,
                                                                 const float* __restrict__ Wd, const float* __restrict__ alpha_p,
                                                                 const float* __restrict__ part, float* __restrict__ loss,
                                                                 float* __restrict__ correct, float* __restrict__ dalpha,
                                                                 float* __restrict__ dfs) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, Qn = d.Qn, N = d.N, F = d.F;
    if (blockIdx.x == gridDim.x - 1) {           // the sums over the row tiles
        fh_sum_parts<3>(part, d.ntile, sm, [&](const float (&t)[3]) {
            loss[0] = t[0] / (float)((long)d.B * Qn); correct[0] = t[1];
            if (dalpha) dalpha[0] = t[2];
        });
        return;
    }
    const int per = ncb * nfb;
    const int b = blockIdx.x / per, r = blockIdx.x - b * per, cb = r / nfb, fb = r - cb * nfb;
    const int c0 = cb * FH_TM, f0 = fb * FH_NB;
    const int nc = min(FH_TM, N - c0), nf = min(FH_NB, F - f0);
    float* dc = sm + FH_MM;                      // [16, FH_LDC]
    float* ts = dc + FH_TM * FH_LDC;             // [16, 16] strided column sums of dz
    float* tc = ts + 256;                        // [16] sum_q dz[q, n]
    const float a2 = 2.f * alpha_p[0];
    {   // sum_q dz[q, n]: 16 strided partial sums per class, added in index order
        const int c = tid & 15, j = tid >> 4;
        float s = 0.f;
        if (c < nc) for (int k = j; k < Qn; k += 16) s += Wd[((long)b * Qn + k) * N + c0 + c];
        ts[j * 16 + c] = s;
        __syncthreads();
        if (j == 0) {
            float a = 0.f;
            for (int i = 0; i < 16; ++i) a += ts[i * 16 + c];
            tc[c] = a;
        }
    }
    __syncthreads();
    // dc[m, n] = 2 alpha (sum_k dz[k, c0 + m] f_q[k, f0 + n] - (c'[c0 + m, f0 + n] + m[f0 + n]) tc_m)
    wg_mm2(sm, FH_MM, nc, nf, Qn, Wd + (long)b * Qn * N + c0, 1, N, fq + (long)b * Qn * F + f0, F, 1,
           [&](int m, int n) { return f32pair{protos[((long)b * N + c0 + m) * F + f0 + n], mvec[(long)b * F + f0 + n]}; },
           [&](int m, int n, float acc, f32pair c) { dc[m * FH_LDC + n] = a2 * (acc - (c.x + c.y) * tc[m]); });
    __syncthreads();
    fh_scatter_class_grad(dc, ys, cntf, dfs, b, S, N, F, c0, nc, f0, nf, cb == 0);
}

}  // namespace

extern "C" int fumi_hip_euclid_proto_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* alpha, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* logits, float* dfeats_s, float* dfeats_q, float* dalpha) {
    if (int rc = head_args_check(ws, B, S, Qn, N, F, S <= 1024, {feats_s, y_s, feats_q, y_q, alpha, loss, correct})) return rc;
    const int train = head_grad_form(dfeats_s, dfeats_q, dalpha);
    if (train < 0) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    const HeadDims d = head_dims_fill(B, S, Qn, N, F, train, grad_scale);
    const size_t n_pro = (size_t)B * N * F, n_m = (size_t)B * F, n_psq = (size_t)B * d.nfb1 * 2 * N, n_cnt = (size_t)B * N,
                 n_part = (size_t)3 * d.ntile, n_dz = (size_t)B * Qn * N;
    int rc = ws_reserve(ws, ws_align(n_pro * 4) + ws_align(n_m * 4) + ws_align(n_psq * 4) + ws_align(n_cnt * 4) + ws_align(n_part * 4)
                            + (train ? ws_align(n_dz * 4) : 0));
    if (rc) return rc;
    float* protos = ws_f(ws, n_pro); float* mvec = ws_f(ws, n_m); float* psq = ws_f(ws, n_psq); float* cntf = ws_f(ws, n_cnt);
    float* part = ws_f(ws, n_part);
    float* Wd = train ? ws_f(ws, n_dz) : nullptr;
    const size_t lds1 = ((size_t)N * FH_PF + FH_PF + S + N) * 4;
    const size_t lds2 = ((size_t)FH_TM * d.ldz + 192 + FH_MM) * 4;
    const size_t lds3 = train ? ((size_t)FH_MM + FH_TM * FH_LDC + 256 + 16) * 4 : (size_t)768 * 4;   // the forward form's one workgroup only adds the tile sums
    FUMI_SET_DYN_LDS(euclid_proto_means_kernel, lds1);
    hipLaunchKernelGGL(euclid_proto_means_kernel, dim3(B * d.nfb1), dim3(256), lds1, st, d, feats_s, y_s, protos, mvec, psq, cntf,
                       ws->status);
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(euclid_proto_rows_kernel, lds2);
    hipLaunchKernelGGL(euclid_proto_rows_kernel, dim3(d.ntile), dim3(256), lds2, st, d, feats_q, y_q, protos, mvec, psq, alpha, preds,
                       logits, part, Wd, dfeats_q, ws->status);
    LAUNCH_CHECK();
    const int nfb = (F + FH_NB - 1) / FH_NB, ncb = (N + FH_TM - 1) / FH_TM;
    FUMI_SET_DYN_LDS(euclid_proto_sgrad_kernel, lds3);
    hipLaunchKernelGGL(euclid_proto_sgrad_kernel, dim3((train ? B * ncb * nfb : 0) + 1), dim3(256), lds3, st, d, nfb, ncb, feats_q, y_s,
                       protos, mvec, cntf, Wd, alpha, part, loss, correct, dalpha, dfeats_s);
    LAUNCH_CHECK();
    return FUMI_OK;
}
