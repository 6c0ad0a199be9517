// Cosine nearest-centroid head with a learned temperature (Meta-Baseline stage): per episode
//     c_n = mean of the support rows of class n,   cos[q,n] = <f_q, c_n> / (max(|f_q|, eps) max(|c_n|, eps)),   z = tau cos,
// mean softmax cross-entropy of z over all B * Qn query rows, first arg-max predictions, and the gradients of grad_scale * loss with
// respect to the query rows, the support rows and tau.  The normalised vectors are never formed: q^ = rq f_q and c^_n = rp_n c_n with
// rq = 1 / max(|f_q|, eps), rp_n = 1 / max(|c_n|, eps), so both scales move into the epilogues of the products.
//
//   launch 1, one workgroup per (episode, block of 256 features): class sums in LDS, one column per thread, support rows added in
//       index order (the order of fumi_hip_proto_reduce); writes the means, sum_f c_n[f]^2 of its feature block and the class counts.
//   launch 2, one workgroup per (episode, tile of 16 query rows): |f_q| (16 lanes per row), |c_n| from the block sums in index order,
//       cos = (f_tile C^T) rq rp on the f32 MFMA (wg_mm), kept in LDS; per row first arg-max, log-sum-exp, NLL; the tile's loss /
//       correct / dtau sums go to part[tile].  Training form: with dcos = tau dz, dz = grad_scale / (B Qn) (softmax - onehot),
//           dfeats_q = rq ((dcos rp) C - f_q rq sum_n dcos cos)        (wg_mm2, A read from LDS; the second term only where |f_q| >= eps)
//       and dcos rq, dcos cos go to memory for launch 3.
//   launch 3, one workgroup per (episode, 16 classes, 128 features), each over ALL Qn rows (no sum across workgroups):
//           dc_n = rp_n ((dcos rq)^T F_q - c_n rp_n sum_q dcos cos)    (the second term only where |c_n| >= eps)
//       scattered to the support rows of class n as dc_n / count_n; one further workgroup adds part[0..ntile): loss, correct, dtau.
//   The forward form (no gradient pointers) is launch 1, launch 2 without its backward half and the last workgroup of launch 3: the
//   same instructions produce loss, correct, preds and logits in both forms.
// Fixed summation orders, the first arg-max, the label-range and missing-class rules and the absence of floating-point atomics are
// those of fewshot_head.h.  A support row left out gets a zero gradient, a class without a support row a zero prototype.  tau is
// read from device memory by the kernels.
#include "fewshot_head.h"

namespace {

constexpr float CP_EPS = 1e-12f;   // F.normalize's clamp

__global__ __launch_bounds__(256) void cos_proto_means_kernel(HeadDims d, const float* __restrict__ xs, const int64_t* __restrict__ ys,
                                                              float* __restrict__ protos, float* __restrict__ psq,
                                                              float* __restrict__ cntf, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, N = d.N, F = d.F;
    const int b = blockIdx.x / d.nfb1, fb = blockIdx.x - b * d.nfb1;
    float* acc = sm;                             // [N, 256] class sums, then means
    int* lab = (int*)(acc + N * FH_PF);          // [S] labels, -1 where out of range
    int* cnt = lab + S;                          // [N]
    const bool bad = fh_stage_labels(ys + (long)b * S, S, N, lab);
    if (bad && fb == 0) atomicOr(status, FUMI_ST_LABEL_RANGE);
    for (int i = tid; i < N * FH_PF; i += 256) acc[i] = 0.f;
    __syncthreads();
    fh_proto_counts(lab, S, N, cnt, cntf, b, fb == 0, status);
    const int f = fb * FH_PF + tid;
    if (f < F) fh_class_sums(acc, lab, xs + (long)b * S * F + f, S, F);
    __syncthreads();
    if (f < F) {
        for (int n = 0; n < N; ++n) {
            const float m = acc[n * FH_PF + tid] / (float)cnt[n];
            acc[n * FH_PF + tid] = m;
            protos[((long)b * N + n) * F + f] = m;
        }
    }
    __syncthreads();
    {   // sum_f c_n[f]^2 over this block's columns (columns past F hold 0): one wave per class
        const int wave = tid >> 6, lane = tid & 63;
        for (int n = wave; n < N; n += 4) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float v = acc[n * FH_PF + lane + 64 * j]; s += v * v; }
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) psq[((long)b * d.nfb1 + fb) * N + n] = s;
        }
    }
}

__global__ __launch_bounds__(256) void cos_proto_rows_kernel(HeadDims d, const float* __restrict__ fq, const int64_t* __restrict__ yq,
                                                             const float* __restrict__ protos, const float* __restrict__ psq,
                                                             const float* __restrict__ tau_p, int64_t* __restrict__ preds,
                                                             float* __restrict__ logits, float* __restrict__ part,
                                                             float* __restrict__ Wd, float* __restrict__ U, float* __restrict__ dfq,
                                                             int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int Qn = d.Qn, N = d.N, F = d.F, ldz = d.ldz;
    const int b = blockIdx.x / d.tpe, q0 = (blockIdx.x - b * d.tpe) * FH_TM, rows = min(FH_TM, Qn - q0);
    const long r0 = (long)b * Qn + q0;           // the tile's first row among all B * Qn
    float* Z = sm;                               // [16, ldz] cos, then dcos rp
    float* rq = Z + FH_TM * ldz;                 // [16] 1 / max(|f_q|, eps)
    float* se = rq + 16;                         // [16] |f_q| >= eps, then rq sum_n dcos cos where it is
    float* rl = se + 16;                         // [16] row losses, [16] row hits, [16] row dtau
    float* rp = rl + 48;                         // [64] 1 / max(|c_n|, eps)
    float* mm = rp + 64;
    const float* ft = fq + r0 * F;
    const float* pc = protos + (long)b * N * F;
    const float tau = tau_p[0];
    const int row = tid >> 4, l = tid & 15;      // 16 lanes per row

    {
        float s = 0.f;
        if (row < rows) {
            const float* x = ft + (long)row * F;
            if ((((uintptr_t)x) & 15) == 0) {
                const f32x4* x4 = (const f32x4*)x;
                for (int k = l; k < (F >> 2); k += 16) { const f32x4 v = x4[k]; s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }
            } else {
                for (int k = l; k < F; k += 16) s += x[k] * x[k];
            }
        }
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (l == 0) { const float nq = sqrtf(s); rq[row] = 1.f / fmaxf(nq, CP_EPS); se[row] = nq >= CP_EPS ? 1.f : 0.f; }
    }
    if (tid < N) {
        float s = 0.f;
        for (int k = 0; k < d.nfb1; ++k) s += psq[((long)b * d.nfb1 + k) * N + tid];
        rp[tid] = 1.f / fmaxf(sqrtf(s), CP_EPS);
    }
    __syncthreads();
    wg_mm(mm, FH_MM, rows, N, F, ft, F, 1, pc, 1, F, [&](int m, int n, float acc) { Z[m * ldz + n] = acc * rq[m] * rp[n]; });
    __syncthreads();

    {
        float loss = 0.f, hit = 0.f, dt = 0.f;
        if (row < rows) {
            float* c = Z + row * ldz;
            float cs[4], z[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; cs[j] = n < N ? c[n] : 0.f; z[j] = tau * cs[j]; }
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
            loss = ok ? mx + logf(s) - tau * c[yv] : 0.f;
            hit = (ok && arg == (int)yv) ? 1.f : 0.f;
            if (l == 0 && preds) preds[r0 + row] = arg;
            if (logits) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; if (n < N) logits[(r0 + row) * N + n] = z[j]; }
            }
            if (d.train) {
                const float inv = 1.f / s, gs = ok ? d.gs : 0.f, rqm = rq[row];
                float sd = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = l + 16 * j;
                    if (n < N) {
                        const float g = gs * (e[j] * inv - (n == (int)yv ? 1.f : 0.f));   // dz
                        const float dc = tau * g;                                          // dcos
                        dt += g * cs[j]; sd += dc * cs[j];
                        Wd[(r0 + row) * N + n] = dc * rqm; U[(r0 + row) * N + n] = dc * cs[j];
                        c[n] = dc * rp[n];
                    }
                }
                for (int o = 8; o > 0; o >>= 1) { dt += __shfl_xor(dt, o, 64); sd += __shfl_xor(sd, o, 64); }
                if (l == 0) se[row] = se[row] * sd * rqm;
            }
        }
        if (l == 0) { rl[row] = loss; rl[16 + row] = hit; rl[32 + row] = dt; }
    }
    __syncthreads();
    fh_tile_part<3>(rl, part, d.ntile);
    if (!d.train) return;
    // dfeats_tile [rows, F] = rq ((dcos rp) [rows, N] C [N, F] - f_tile se)
    for (int f0 = 0; f0 < F; f0 += FH_NB) {
        const int nb = min(FH_NB, F - f0);
        wg_mm2(mm, FH_MM, rows, nb, N, Z, ldz, 1, pc + f0, F, 1,
               [&](int m, int n) { return ft[(long)m * F + f0 + n]; },
               [&](int m, int n, float acc, float x) { dfq[(r0 + m) * F + f0 + n] = rq[m] * (acc - x * se[m]); });
    }
}

__global__ __launch_bounds__(256) void cos_proto_sgrad_kernel(HeadDims d, int nfb, int ncb, const float* __restrict__ fq,
                                                              const int64_t* __restrict__ ys, const float* __restrict__ protos,
                                                              const float* __restrict__ psq, const float* __restrict__ cntf,
                                                              const float* __restrict__ Wd, const float* __restrict__ U,
                                                              const float* __restrict__ part, float* __restrict__ loss,
                                                              float* __restrict__ correct, float* __restrict__ dtau,
                                                              float* __restrict__ dfs) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, Qn = d.Qn, N = d.N, F = d.F;
    if (blockIdx.x == gridDim.x - 1) {           // the sums over the row tiles
        fh_sum_parts<3>(part, d.ntile, sm, [&](const float (&t)[3]) {
            loss[0] = t[0] / (float)((long)d.B * Qn); correct[0] = t[1];
            if (dtau) dtau[0] = t[2];
        });
        return;
    }
    const int per = ncb * nfb;
    const int b = blockIdx.x / per, r = blockIdx.x - b * per, cb = r / nfb, fb = r - cb * nfb;
    const int c0 = cb * FH_TM, f0 = fb * FH_NB;
    const int nc = min(FH_TM, N - c0), nf = min(FH_NB, F - f0);
    float* dc = sm + FH_MM;                      // [16, FH_LDC]
    float* ts = dc + FH_TM * FH_LDC;             // [16, 16] strided column sums of dcos cos
    float* rps = ts + 256;                       // [16] 1 / max(|c_n|, eps)
    float* tc = rps + 16;                        // [16] rp_n sum_q dcos cos where |c_n| >= eps, else 0
    {   // sum_q dcos[q, n] cos[q, n]: 16 strided partial sums per class, added in index order
        const int c = tid & 15, j = tid >> 4;
        float s = 0.f;
        if (c < nc) for (int k = j; k < Qn; k += 16) s += U[((long)b * Qn + k) * N + c0 + c];
        ts[j * 16 + c] = s;
        __syncthreads();
        if (j == 0 && c < nc) {
            float a = 0.f, p2 = 0.f;
            for (int i = 0; i < 16; ++i) a += ts[i * 16 + c];
            for (int k = 0; k < d.nfb1; ++k) p2 += psq[((long)b * d.nfb1 + k) * N + c0 + c];
            const float pn = sqrtf(p2), rpn = 1.f / fmaxf(pn, CP_EPS);
            rps[c] = rpn; tc[c] = pn >= CP_EPS ? a * rpn : 0.f;
        }
    }
    __syncthreads();
    // dc[m, n] = rp_m (sum_k (dcos rq)[k, c0 + m] f_q[k, f0 + n] - c[c0 + m, f0 + n] tc_m)
    wg_mm2(sm, FH_MM, nc, nf, Qn, Wd + (long)b * Qn * N + c0, 1, N, fq + (long)b * Qn * F + f0, F, 1,
           [&](int m, int n) { return protos[((long)b * N + c0 + m) * F + f0 + n]; },
           [&](int m, int n, float acc, float c) { dc[m * FH_LDC + n] = rps[m] * (acc - c * tc[m]); });
    __syncthreads();
    fh_scatter_class_grad(dc, ys, cntf, dfs, b, S, N, F, c0, nc, f0, nf, cb == 0);
}

}  // namespace

extern "C" int fumi_hip_cos_proto_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* tau, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* logits, float* dfeats_s, float* dfeats_q, float* dtau) {
    if (int rc = head_args_check(ws, B, S, Qn, N, F, S <= 1024, {feats_s, y_s, feats_q, y_q, tau, loss, correct})) return rc;
    const int train = head_grad_form(dfeats_s, dfeats_q, dtau);
    if (train < 0) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    const HeadDims d = head_dims_fill(B, S, Qn, N, F, train, grad_scale);
    const size_t n_pro = (size_t)B * N * F, n_psq = (size_t)B * d.nfb1 * N, n_cnt = (size_t)B * N, n_part = (size_t)3 * d.ntile,
                 n_dz = (size_t)B * Qn * N;
    int rc = ws_reserve(ws, ws_align(n_pro * 4) + ws_align(n_psq * 4) + ws_align(n_cnt * 4) + ws_align(n_part * 4)
                            + (train ? 2 * ws_align(n_dz * 4) : 0));
    if (rc) return rc;
    float* protos = ws_f(ws, n_pro); float* psq = ws_f(ws, n_psq); float* cntf = ws_f(ws, n_cnt); float* part = ws_f(ws, n_part);
    float* Wd = train ? ws_f(ws, n_dz) : nullptr; float* U = train ? ws_f(ws, n_dz) : nullptr;
    const size_t lds1 = ((size_t)N * FH_PF + S + N) * 4;
    const size_t lds2 = ((size_t)FH_TM * d.ldz + 144 + FH_MM) * 4;
    const size_t lds3 = train ? ((size_t)FH_MM + FH_TM * FH_LDC + 256 + 32) * 4 : (size_t)768 * 4;   // the forward form's one workgroup only adds the tile sums
    FUMI_SET_DYN_LDS(cos_proto_means_kernel, lds1);
    hipLaunchKernelGGL(cos_proto_means_kernel, dim3(B * d.nfb1), dim3(256), lds1, st, d, feats_s, y_s, protos, psq, cntf, ws->status);
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(cos_proto_rows_kernel, lds2);
    hipLaunchKernelGGL(cos_proto_rows_kernel, dim3(d.ntile), dim3(256), lds2, st, d, feats_q, y_q, protos, psq, tau, preds, logits, part,
                       Wd, U, dfeats_q, ws->status);
    LAUNCH_CHECK();
    const int nfb = (F + FH_NB - 1) / FH_NB, ncb = (N + FH_TM - 1) / FH_TM;
    FUMI_SET_DYN_LDS(cos_proto_sgrad_kernel, lds3);
    hipLaunchKernelGGL(cos_proto_sgrad_kernel, dim3((train ? B * ncb * nfb : 0) + 1), dim3(256), lds3, st, d, nfb, ncb, feats_q, y_s,
                       protos, psq, cntf, Wd, U, part, loss, correct, dtau, dfeats_s);
    LAUNCH_CHECK();
    return FUMI_OK;
}
