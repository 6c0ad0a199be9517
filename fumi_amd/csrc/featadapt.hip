// Set-to-set prototype adaptation in front of the prototype heads (FEAT: Ye et al., CVPR 2020; --fewshot_adapt feat; DESIGN.md
// section 43).  Per episode, with F the feature width:
//     P  = class means of feats_s by y_s                      [N,F]   (counts clamped to >= 1, as fumi_hip_proto_reduce)
//     Q  = P Wq^T,  K = P Wk^T,  V = P Wv^T                   [N,F]   (one product against Wqkv [3F,F])
//     A  = softmax_rows(Q K^T / sqrt(F))                      [N,N]   (row maximum subtracted before exp)
//     O  = A V,   U = O Wo^T + bo,   R = P + U
//     P' = gamma (R - mean_f R) / sqrt(var_f R + 1e-5) + beta         (biased variance)
// Post-ReLU features share a large offset, and so do their prototypes.  Evaluated as written, that offset sits in every score and in
// every dO V^T as a term common to the row, which the softmax and its backward then cancel at the cost of the digits.  So K and V are
// formed from the prototypes relative to the episode's mean prototype m = (1/N) sum_n P_n (as euclidproto.hip centres its distances):
//     K~ = (P - m) Wk^T,  V~ = (P - m) Wv^T,  A = softmax(Q K~^T / sqrt(F)),  O = A V~ + m Wv^T,
// the same numbers in exact arithmetic (a term common to a row of the scores does not reach the softmax; the rows of A sum to 1), and
// the backward reads K~ and V~ where the formulas read K and V: dA = dO V~^T differs from dO V^T by a term common to the row, which
// dS = A (dA - sum_n dA A) removes, and dQ = dS K~ = dS K because the rows of dS sum to 0.
// P' is an N-way 1-shot support set with labels 0..N-1 for fumi_hip_cos_proto_step / fumi_hip_euclid_proto_step, whose dfeats_s comes
// back here as dP'.
//
//   forward, eight launches:
//     1  fa_means_kernel, one workgroup per (episode, block of 256 features): the class sums of the heads (fewshot_head.h) -> P, P - m,
//        m, counts; the only place where the two label flags are raised.
//     2, 3, 4  Q = P Wq^T, K~ | V~ = (P - m) [Wk; Wv]^T into one [B N, 3F] image, m Wv^T [B, F], on the dense GEMM (gemm.hip).
//     5  fa_scores_kernel, one workgroup per episode: Q K^T on the f32 MFMA with the contraction over F streamed through LDS in slabs
//        (wg_mm: [N,F] does not fit, the [N,N] scores do), the scaled softmax in LDS, 16 lanes per row -> A.
//     6  fa_av_kernel, one workgroup per (episode, 128 features): O = A V~ + m Wv^T.
//     7  U = O Wo^T + bo on the dense GEMM, written where R will stand.
//     8  fa_ln_fwd_kernel, one wave per row of the B N: R = P + U, mean, variance about the mean, P'; keeps R, mean and 1 / std.
//   backward, ten launches:
//     1  fa_ln_bwd_kernel, one wave per row: dR, and dP' * xhat for the dgamma sum.
//     2, 3  dgamma, dbeta, dbo as column sums over all B N rows: partial sums of 128-row chunks, then those in index order
//        (launch_colsum_multi).
//     4, 5  dWo = dR^T O and dO = dR Wo on the dense GEMM.
//     6  fa_dscores_kernel, one workgroup per episode: dA = dO V^T (streamed over F as the scores of the forward), the softmax backward
//        dS = A (dA - sum_n dA A) / sqrt(F) in LDS.
//     7  fa_dqkv_kernel, one workgroup per (episode, 128 features): dV = A^T dO, dQ = dS K, dK = dS^T Q -> dQKV [B N, 3F].
//     8, 9  dP (projection paths) = dQKV Wqkv and dWqkv = dQKV^T P on the dense GEMM.
//     10 fa_scatter_kernel, one workgroup per support row: (dR + dP)_n / count_n to every row of class n, zero to a row left out.
// Everything is fp32 with fp32 accumulation; every sum has a fixed order (butterflies, index-ordered loops, the MFMA's k order) and
// there is no floating-point atomic, so equal inputs give equal bits.  The forward form (no tape) runs the same eight launches on
// workspace memory: protos_out is bit-identical.
#include "fewshot_head.h"
#include <math.h>

namespace {

constexpr int FA_RPW = 4;                        // rows per workgroup of the LayerNorm kernels: one wave each

// the tape, in floats; every part starts on a multiple of 4 floats
struct FaTape { size_t P, QKV, A, O, R, stat, cnt, total; };
static inline size_t fa_r4(size_t n) { return (n + 3) & ~(size_t)3; }
static inline FaTape fa_tape(int B, int N, int F) {
    const size_t M = (size_t)B * N;
    FaTape t;
    size_t o = 0;
    t.P = o; o += fa_r4(M * F);
    t.QKV = o; o += fa_r4(M * 3 * F);
    t.A = o; o += fa_r4(M * N);
    t.O = o; o += fa_r4(M * F);
    t.R = o; o += fa_r4(M * F);
    t.stat = o; o += fa_r4(M * 2);
    t.cnt = o; o += fa_r4(M);
    t.total = o;
    return t;
}
static inline bool fa_limits(int B, int S, int N, int F) {
    return B >= 1 && S >= 1 && S <= 1024 && N >= 2 && N <= 64 && (long)B * N <= 65536 && F % 32 == 0 && F >= 32 && F <= 2048;
}

__global__ __launch_bounds__(256) void fa_means_kernel(int S, int N, int F, int nfb1, const float* __restrict__ xs,
                                                       const int64_t* __restrict__ ys, float* __restrict__ P,
                                                       float* __restrict__ Pc, float* __restrict__ mvec,
                                                       float* __restrict__ cntf, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / nfb1, fb = blockIdx.x - b * nfb1;
    float* acc = sm;                             // [N, 256] class sums
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
        float m = 0.f;
        for (int n = 0; n < N; ++n) {            // the means, and their mean over the classes in index order
            const float c = acc[n * FH_PF + tid] / (float)cnt[n];
            acc[n * FH_PF + tid] = c;
            P[((long)b * N + n) * F + f] = c;
            m += c;
        }
        m /= (float)N;
        for (int n = 0; n < N; ++n) Pc[((long)b * N + n) * F + f] = acc[n * FH_PF + tid] - m;
        mvec[(long)b * F + f] = m;
    }
}

// Z [N, ldz] in LDS holds the scores: A = softmax of its rows -> Aout [N, N]; 16 lanes per row, 16 rows per pass
__device__ __forceinline__ void fa_softmax_rows(const float* Z, int ldz, int N, float* __restrict__ Aout) {
    const int tid = threadIdx.x, l = tid & 15;
    for (int r0 = 0; r0 < N; r0 += 16) {
        const int row = r0 + (tid >> 4);
        const bool live = row < N;
        const float* z = Z + (live ? row : 0) * ldz;
        float v[4], mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; v[j] = n < N ? z[n] : -INFINITY; mx = fmaxf(mx, v[j]); }
        for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float e[4], s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { e[j] = l + 16 * j < N ? expf(v[j] - mx) : 0.f; s += e[j]; }
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float inv = 1.f / s;
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; if (n < N) Aout[(long)row * N + n] = e[j] * inv; }
        }
    }
}

__global__ __launch_bounds__(256) void fa_scores_kernel(int N, int F, int ldz, float scale, const float* __restrict__ QKV,
                                                        float* __restrict__ A) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.x;
    float* Z = sm;                               // [N, ldz]
    float* mm = Z + N * ldz;
    const float* q = QKV + (long)b * N * 3 * F;
    wg_mm(mm, FH_MM, N, N, F, q, 3L * F, 1, q + F, 1, 3L * F, [&](int m, int n, float acc) { Z[m * ldz + n] = acc * scale; });
    __syncthreads();
    fa_softmax_rows(Z, ldz, N, A + (long)b * N * N);
}

__global__ __launch_bounds__(256) void fa_av_kernel(int N, int F, int nfb, const float* __restrict__ A, const float* __restrict__ QKV,
                                                    const float* __restrict__ Vbar, float* __restrict__ O) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.x / nfb, f0 = (blockIdx.x - b * nfb) * FH_NB, nf = min(FH_NB, F - f0);
    const float* v = QKV + (long)b * N * 3 * F + 2 * F + f0;
    wg_mm(sm, FH_MM, N, nf, N, A + (long)b * N * N, N, 1, v, 3L * F, 1,
          [&](int m, int n, float acc) { O[((long)b * N + m) * F + f0 + n] = acc + Vbar[(long)b * F + f0 + n]; });
}

// butterfly sum over the 64 lanes of a wave: every lane holds the total
__device__ __forceinline__ float fa_wave_sum(float s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

__global__ __launch_bounds__(256) void fa_ln_fwd_kernel(int M, int F, const float* __restrict__ P, float* __restrict__ R,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float* __restrict__ out, float* __restrict__ stat) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * FA_RPW + (threadIdx.x >> 6);
    if (row >= M) return;                        // wave-uniform, and the kernel has no barrier
    const float* p = P + (long)row * F;
    float* u = R + (long)row * F;                // U on entry, R on exit
    float s = 0.f;
    for (int f = lane; f < F; f += 64) s += p[f] + u[f];
    const float mean = fa_wave_sum(s) / (float)F;
    float v = 0.f;
    for (int f = lane; f < F; f += 64) { const float d = (p[f] + u[f]) - mean; v += d * d; }
    const float rstd = 1.f / sqrtf(fa_wave_sum(v) / (float)F + 1e-5f);
    for (int f = lane; f < F; f += 64) {
        const float r = p[f] + u[f];
        u[f] = r;
        out[(long)row * F + f] = gamma[f] * ((r - mean) * rstd) + beta[f];
    }
    if (lane == 0) { stat[2 * (long)row] = mean; stat[2 * (long)row + 1] = rstd; }
}

__global__ __launch_bounds__(256) void fa_ln_bwd_kernel(int M, int F, const float* __restrict__ R, const float* __restrict__ stat,
                                                        const float* __restrict__ gamma, const float* __restrict__ dy,
                                                        float* __restrict__ dR, float* __restrict__ dgx) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * FA_RPW + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* r = R + (long)row * F;
    const float* g = dy + (long)row * F;
    const float mean = stat[2 * (long)row], rstd = stat[2 * (long)row + 1];
    float s1 = 0.f, s2 = 0.f;
    for (int f = lane; f < F; f += 64) {
        const float xh = (r[f] - mean) * rstd, t = g[f] * gamma[f];
        s1 += t; s2 += t * xh;
    }
    const float m1 = fa_wave_sum(s1) / (float)F, m2 = fa_wave_sum(s2) / (float)F;
    for (int f = lane; f < F; f += 64) {
        const float xh = (r[f] - mean) * rstd, t = g[f] * gamma[f];
        dR[(long)row * F + f] = rstd * ((t - m1) - xh * m2);
        dgx[(long)row * F + f] = g[f] * xh;
    }
}

__global__ __launch_bounds__(256) void fa_dscores_kernel(int N, int F, int ldz, float scale, const float* __restrict__ dO,
                                                         const float* __restrict__ QKV, const float* __restrict__ A,
                                                         float* __restrict__ dS) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, l = tid & 15, b = blockIdx.x;
    float* Z = sm;                               // [N, ldz] dA
    float* mm = Z + N * ldz;
    const float* v = QKV + (long)b * N * 3 * F + 2 * F;
    wg_mm(mm, FH_MM, N, N, F, dO + (long)b * N * F, F, 1, v, 1, 3L * F, [&](int m, int n, float acc) { Z[m * ldz + n] = acc; });
    __syncthreads();
    const float* Ab = A + (long)b * N * N;
    float* dSb = dS + (long)b * N * N;
    for (int r0 = 0; r0 < N; r0 += 16) {         // 16 lanes per row, as the forward softmax
        const int row = r0 + (tid >> 4);
        const bool live = row < N;
        const float* z = Z + (live ? row : 0) * ldz;
        const float* a = Ab + (long)(live ? row : 0) * N;
        float av[4], dv[4], t = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = l + 16 * j;
            av[j] = n < N ? a[n] : 0.f; dv[j] = n < N ? z[n] : 0.f;
            t += av[j] * dv[j];
        }
        for (int o = 8; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; if (n < N) dSb[(long)row * N + n] = av[j] * (dv[j] - t) * scale; }
        }
    }
}

__global__ __launch_bounds__(256) void fa_dqkv_kernel(int N, int F, int nfb, const float* __restrict__ A, const float* __restrict__ dS,
                                                      const float* __restrict__ dO, const float* __restrict__ QKV,
                                                      float* __restrict__ dQKV) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.x / nfb, f0 = (blockIdx.x - b * nfb) * FH_NB, nf = min(FH_NB, F - f0);
    const float* Ab = A + (long)b * N * N;
    const float* dSb = dS + (long)b * N * N;
    const float* q = QKV + (long)b * N * 3 * F + f0;
    float* d = dQKV + (long)b * N * 3 * F + f0;
    // dQ = dS K,  dK = dS^T Q,  dV = A^T dO
    wg_mm(sm, FH_MM, N, nf, N, dSb, N, 1, q + F, 3L * F, 1, [&](int m, int n, float acc) { d[(long)m * 3 * F + n] = acc; });
    wg_mm(sm, FH_MM, N, nf, N, dSb, 1, N, q, 3L * F, 1, [&](int m, int n, float acc) { d[(long)m * 3 * F + F + n] = acc; });
    wg_mm(sm, FH_MM, N, nf, N, Ab, 1, N, dO + (long)b * N * F + f0, F, 1,
          [&](int m, int n, float acc) { d[(long)m * 3 * F + 2 * F + n] = acc; });
}

__global__ __launch_bounds__(256) void fa_scatter_kernel(int S, int N, int F, const int64_t* __restrict__ ys,
                                                         const float* __restrict__ cntf, const float* __restrict__ dR,
                                                         const float* __restrict__ dPp, float* __restrict__ dfs) {
    const long i = blockIdx.x;                   // support row among all B * S
    const long b = i / S, t = ys[i];
    float* o = dfs + i * F;
    if (t < 0 || t >= N) {                       // a row left out of the mean
        for (int f = threadIdx.x; f < F; f += 256) o[f] = 0.f;
        return;
    }
    const long pr = b * N + t;
    const float c = cntf[pr];
    for (int f = threadIdx.x; f < F; f += 256) o[f] = (dR[pr * F + f] + dPp[pr * F + f]) / c;
}

}  // namespace

extern "C" int64_t fumi_hip_feat_adapt_tape_floats(int B, int N, int F) {
    if (!fa_limits(B, 1, N, F)) return 0;
    return (int64_t)fa_tape(B, N, F).total;
}

extern "C" int fumi_hip_feat_adapt_fwd(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int N, int F, const float* feats_s,
        const int64_t* y_s, const float* Wqkv, const float* Wo, const float* bo, const float* gamma, const float* beta,
        float* protos_out, float* tape) {
    if (!ws) return FUMI_EINVAL;
    if (!fa_limits(B, S, N, F)) return FUMI_ENOTSUP;
    for (const void* p : {(const void*)feats_s, (const void*)y_s, (const void*)Wqkv, (const void*)Wo, (const void*)bo,
                          (const void*)gamma, (const void*)beta, (const void*)protos_out})
        if (!p) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    const FaTape t = fa_tape(B, N, F);
    const size_t MF = (size_t)B * N * F, BF = (size_t)B * F;
    int rc = ws_reserve(ws, ws_align(MF * 4) + 2 * ws_align(BF * 4) + (tape ? 0 : ws_align(t.total * 4)));
    if (rc) return rc;
    float* Pc = ws_f(ws, MF); float* mvec = ws_f(ws, BF); float* Vbar = ws_f(ws, BF);
    float* tp = tape ? tape : ws_f(ws, t.total);
    const int M = B * N, nfb1 = (F + FH_PF - 1) / FH_PF, nfb = (F + FH_NB - 1) / FH_NB, ldz = ((N + 15) & ~15) + 4;
    const float scale = (float)(1.0 / sqrt((double)F));

    const size_t lds1 = ((size_t)N * FH_PF + S + N) * 4;
    FUMI_SET_DYN_LDS(fa_means_kernel, lds1);
    hipLaunchKernelGGL(fa_means_kernel, dim3(B * nfb1), dim3(256), lds1, st, S, N, F, nfb1, feats_s, y_s, tp + t.P, Pc, mvec,
                       tp + t.cnt, ws->status);
    LAUNCH_CHECK();
    const float* Wkv = Wqkv + (size_t)F * F;
    if ((rc = launch_gemm(st, gemm_args(M, F, F, tp + t.P, F, Wqkv, F, tp + t.QKV, 3L * F), 0, 0))) return rc;           // Q
    if ((rc = launch_gemm(st, gemm_args(M, 2 * F, F, Pc, F, Wkv, F, tp + t.QKV + F, 3L * F), 0, 0))) return rc;          // K~ | V~
    if ((rc = launch_gemm(st, gemm_args(B, F, F, mvec, F, Wkv + (size_t)F * F, F, Vbar, F), 0, 0))) return rc;           // m Wv^T
    const size_t lds3 = ((size_t)N * ldz + FH_MM) * 4;
    FUMI_SET_DYN_LDS(fa_scores_kernel, lds3);
    hipLaunchKernelGGL(fa_scores_kernel, dim3(B), dim3(256), lds3, st, N, F, ldz, scale, tp + t.QKV, tp + t.A);
    LAUNCH_CHECK();
    const size_t lds4 = (size_t)FH_MM * 4;
    FUMI_SET_DYN_LDS(fa_av_kernel, lds4);
    hipLaunchKernelGGL(fa_av_kernel, dim3(B * nfb), dim3(256), lds4, st, N, F, nfb, tp + t.A, tp + t.QKV, Vbar, tp + t.O);
    LAUNCH_CHECK();
    GemmArgs g = gemm_args(M, F, F, tp + t.O, F, Wo, F, tp + t.R, F);
    g.bias = bo;
    if ((rc = launch_gemm(st, g, 0, 0))) return rc;
    hipLaunchKernelGGL(fa_ln_fwd_kernel, dim3((M + FA_RPW - 1) / FA_RPW), dim3(256), 0, st, M, F, tp + t.P, tp + t.R, gamma, beta,
                       protos_out, tp + t.stat);
    LAUNCH_CHECK();
    return FUMI_OK;
}

extern "C" int fumi_hip_feat_adapt_bwd(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int N, int F, const float* feats_s,
        const int64_t* y_s, const float* Wqkv, const float* Wo, const float* bo, const float* gamma, const float* beta,
        const float* tape, const float* dprotos, float* dfeats_s, float* dWqkv, float* dWo, float* dbo, float* dgamma,
        float* dbeta) {
    if (!ws) return FUMI_EINVAL;
    if (!fa_limits(B, S, N, F)) return FUMI_ENOTSUP;
    for (const void* p : {(const void*)feats_s, (const void*)y_s, (const void*)Wqkv, (const void*)Wo, (const void*)bo,
                          (const void*)gamma, (const void*)beta, (const void*)tape, (const void*)dprotos, (const void*)dfeats_s,
                          (const void*)dWqkv, (const void*)dWo, (const void*)dbo, (const void*)dgamma, (const void*)dbeta})
        if (!p) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    const FaTape t = fa_tape(B, N, F);
    const int M = B * N, nfb = (F + FH_NB - 1) / FH_NB, ldz = ((N + 15) & ~15) + 4;
    const size_t MF = (size_t)M * F, NN = (size_t)M * N;
    const float scale = (float)(1.0 / sqrt((double)F));
    ColsumJobs jobs; jobs.n = 0; jobs.part_total = 0;
    float* const none = nullptr;
    jobs.add(none, M, F, F, dgamma); jobs.add(none, M, F, F, dbeta); jobs.add(none, M, F, F, dbo);
    int rc = ws_reserve(ws, 4 * ws_align(MF * 4) + ws_align(NN * 4) + ws_align(3 * MF * 4) + ws_align((size_t)jobs.part_total * 4));
    if (rc) return rc;
    float* dR = ws_f(ws, MF); float* dgx = ws_f(ws, MF); float* dO = ws_f(ws, MF); float* dPp = ws_f(ws, MF);
    float* dS = ws_f(ws, NN); float* dQKV = ws_f(ws, 3 * MF); float* part = ws_f(ws, (size_t)jobs.part_total);
    jobs.X[0] = dgx; jobs.X[1] = dprotos; jobs.X[2] = dR;

    hipLaunchKernelGGL(fa_ln_bwd_kernel, dim3((M + FA_RPW - 1) / FA_RPW), dim3(256), 0, st, M, F, tape + t.R, tape + t.stat, gamma,
                       dprotos, dR, dgx);
    LAUNCH_CHECK();
    if ((rc = launch_colsum_multi(st, jobs, part))) return rc;
    if ((rc = launch_gemm(st, gemm_args(F, F, M, dR, F, tape + t.O, F, dWo, F), 1, 1))) return rc;             // dWo = dR^T O
    if ((rc = launch_gemm(st, gemm_args(M, F, F, dR, F, Wo, F, dO, F), 0, 1))) return rc;                      // dO = dR Wo
    const size_t lds6 = ((size_t)N * ldz + FH_MM) * 4;
    FUMI_SET_DYN_LDS(fa_dscores_kernel, lds6);
    hipLaunchKernelGGL(fa_dscores_kernel, dim3(B), dim3(256), lds6, st, N, F, ldz, scale, dO, tape + t.QKV, tape + t.A, dS);
    LAUNCH_CHECK();
    const size_t lds7 = (size_t)FH_MM * 4;
    FUMI_SET_DYN_LDS(fa_dqkv_kernel, lds7);
    hipLaunchKernelGGL(fa_dqkv_kernel, dim3(B * nfb), dim3(256), lds7, st, N, F, nfb, tape + t.A, dS, dO, tape + t.QKV, dQKV);
    LAUNCH_CHECK();
    if ((rc = launch_gemm(st, gemm_args(M, F, 3 * F, dQKV, 3L * F, Wqkv, F, dPp, F), 0, 1))) return rc;        // dP = dQKV Wqkv
    if ((rc = launch_gemm(st, gemm_args(3 * F, F, M, dQKV, 3L * F, tape + t.P, F, dWqkv, F), 1, 1))) return rc;   // dWqkv = dQKV^T P
    hipLaunchKernelGGL(fa_scatter_kernel, dim3(B * S), dim3(256), 0, st, S, N, F, y_s, tape + t.cnt, dR, dPp, dfeats_s);
    LAUNCH_CHECK();
    return FUMI_OK;
}
