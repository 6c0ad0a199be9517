// What the episode heads share (cosproto.hip, euclidproto.hip, ridgehead.hip, logreghead.hip, transproto.hip):
// the tile constants, the host's limit checks and launch dimensions, and the blocks of the kernels that are the same in every head --
// label staging and class counts, the class sums, the tile sums and the gradient scatter.  Device functions only, inlined into the
// kernels of each file; where the heads differ they pass a lambda, as wg_mm's epilogues do.
// NOT here: the per-row softmax cross-entropy of the rows kernels and of the transductive loop, and the label block of the kernels
// that run one workgroup per episode (ridge factor, logreg fits).  Those stay copies in their kernels, each with a comment: routed
// through helpers the compiler allocated those kernels' registers differently and they measured 0.2 - 1 % slower.
//
// What every head promises, in these blocks and in the copies:
//   - every sum has a fixed order (butterflies, index-ordered loops, strided sums added in index order): equal inputs give equal bits;
//   - the prediction is the FIRST arg-max, as torch.max returns it; a row of NaNs predicts class 0;
//   - a label outside [0, N) sets FUMI_ST_LABEL_RANGE: such a query row adds nothing to the loss, the count or any gradient while the
//     divisor stays B * Qn; such a support row is staged as -1 and left out of every count and sum;
//   - a class without a support row sets FUMI_ST_CLASS_MISSING;
//   - no floating-point atomics: the only atomic is the OR into the status word.
#pragma once
#include "common.h"
#include <initializer_list>

constexpr int FH_TM = 16;          // query rows per workgroup of the rows kernel, classes per workgroup of the support-gradient kernel
constexpr int FH_NB = 128;         // output columns of one wg_mm call; features per workgroup of the [N, 128] launches
constexpr int FH_MM = 16384;       // floats of LDS the products stage their operands in
constexpr int FH_PF = 256;         // features per workgroup of the means kernel: one column per thread
constexpr int FH_LDC = FH_NB + 4;  // row stride of the [16, 128] and [N, 128] LDS images

// ---- host side ---------------------------------------------------------------------------------------------------------------------
struct HeadDims {
    int B, S, Qn, N, F, ldz, tpe, ntile, nfb1, train;   // tpe: row tiles per episode, nfb1: feature blocks of the means kernel
    float gs;                                           // grad_scale / (B Qn)
};
// the shape and row-tile fields, for HeadDims and for the structs that carry them beside fields of their own (Ridge, Logreg: those
// keep their layouts, an embedded HeadDims would only add kernel arguments they do not read)
template <class D>
static inline void head_rows_fill(D& d, int B, int S, int Qn, int N, int F) {
    d.B = B; d.S = S; d.Qn = Qn; d.N = N; d.F = F;
    d.ldz = ((N + 15) & ~15) + 4; d.tpe = (Qn + FH_TM - 1) / FH_TM; d.ntile = B * d.tpe;
}
static inline float head_grad_scale(float grad_scale, int B, int Qn) { return grad_scale / (float)((long)B * Qn); }
static inline HeadDims head_dims_fill(int B, int S, int Qn, int N, int F, int train, float grad_scale) {
    HeadDims d;
    head_rows_fill(d, B, S, Qn, N, F);
    d.nfb1 = (F + FH_PF - 1) / FH_PF; d.train = train; d.gs = head_grad_scale(grad_scale, B, Qn);
    return d;
}
// The refusals of every entry in their fixed order: FUMI_EINVAL without a workspace, FUMI_ENOTSUP outside the common limits or the
// entry's own (`own_limits`), FUMI_EINVAL for a null among `need`.
static inline int head_args_check(const fumi_ws_t* ws, int B, int S, int Qn, int N, int F, bool own_limits,
                                  std::initializer_list<const void*> need) {
    if (!ws) return FUMI_EINVAL;
    if (B < 1 || S < 1 || Qn < 1 || N < 2 || N > 64 || F % 32 != 0 || F < 32 || F > 2048 || (long)B * Qn > 65536 || !own_limits)
        return FUMI_ENOTSUP;
    for (const void* p : need) if (!p) return FUMI_EINVAL;
    return FUMI_OK;
}
// the three gradient pointers come together or not at all: 1 training form, 0 forward form, -1 neither
static inline int head_grad_form(const void* dfeats_s, const void* dfeats_q, const void* dparam) {
    const int ngrad = (dfeats_s ? 1 : 0) + (dfeats_q ? 1 : 0) + (dparam ? 1 : 0);
    return ngrad == 3 ? 1 : ngrad == 0 ? 0 : -1;
}

// ---- labels and class counts -------------------------------------------------------------------------------------------------------
// y [S] -> lab [S] in LDS, -1 where the label is outside [0, N); whether this thread met such a label.  Which workgroups OR the status
// bit is the caller's rule (the heads with feature blocks report from block 0 only).
__device__ __forceinline__ bool fh_stage_labels(const int64_t* y, int S, int N, int* lab) {
    bool bad = false;
    for (int i = threadIdx.x; i < S; i += 256) {
        const long t = y[i];
        const bool ok = t >= 0 && t < N;
        lab[i] = ok ? (int)t : -1;
        bad |= !ok;
    }
    return bad;
}
// the support rows of class n, after the barrier that follows the staging; clamping and the status bit are the caller's
__device__ __forceinline__ int fh_class_count(const int* lab, int S, int n) {
    int c = 0;
    for (int i = 0; i < S; ++i) c += lab[i] == n ? 1 : 0;
    return c;
}
// The prototype heads' convention (cosine, Euclidean): cnt [N] in LDS holds the counts clamped to >= 1, the divisor of the means; the
// first feature block (`first`) writes them as floats to cntf [B, N] and reports a class without a support row.
__device__ __forceinline__ void fh_proto_counts(const int* lab, int S, int N, int* cnt, float* cntf, int b, bool first,
                                                int* status) {
    const int tid = threadIdx.x;
    if (tid >= N) return;
    const int c = fh_class_count(lab, S, tid);
    cnt[tid] = c > 0 ? c : 1;
    if (first) {
        cntf[(long)b * N + tid] = (float)(c > 0 ? c : 1);
        if (c == 0) atomicOr(status, FUMI_ST_CLASS_MISSING);
    }
}

// ---- class sums, one column per thread ---------------------------------------------------------------------------------------------
// acc [N, 256] in LDS += the support rows of this thread's column x (row stride F), in index order: the order of fumi_hip_proto_reduce
__device__ __forceinline__ void fh_class_sums(float* acc, const int* lab, const float* x, int S, int F) {
    const int tid = threadIdx.x;
    int i = 0;
    for (; i + 4 <= S; i += 4) {                 // four loads in flight, added in index order
        float v[4]; int l[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { v[u] = x[(long)(i + u) * F]; l[u] = lab[i + u]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) if (l[u] >= 0) acc[l[u] * FH_PF + tid] += v[u];
    }
    for (; i < S; ++i) { const int l = lab[i]; if (l >= 0) acc[l * FH_PF + tid] += x[(long)i * F]; }
}

// ---- tile sums ---------------------------------------------------------------------------------------------------------------------
// rl [K][16] (row scalars of this workgroup's tile, after a barrier) -> part[k * ntile + tile], rows in index order, by thread 0
template <int K>
__device__ __forceinline__ void fh_tile_part(const float* rl, float* part, int ntile) {
    if (threadIdx.x != 0) return;
    float a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = 0.f;
    for (int r = 0; r < FH_TM; ++r) {
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] += rl[16 * k + r];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) part[k * ntile + blockIdx.x] = a[k];
}
// done(t) in thread 0 with t[k] = sum of part[k * n .. k * n + n): 256 strided sums, then those in index order.  One whole
// workgroup calls it, with sm [K * 256] floats of LDS.
template <int K, class Done>
__device__ __forceinline__ void fh_sum_parts(const float* part, int n, float* sm, Done&& done) {
    const int tid = threadIdx.x;
    float t[K];
#pragma unroll
    for (int k = 0; k < K; ++k) t[k] = 0.f;
    for (int i = tid; i < n; i += 256) {
#pragma unroll
        for (int k = 0; k < K; ++k) t[k] += part[k * n + i];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) sm[256 * k + tid] = t[k];
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) t[k] = 0.f;
        for (int i = 0; i < 256; ++i) {
#pragma unroll
            for (int k = 0; k < K; ++k) t[k] += sm[256 * k + i];
        }
        done(t);
    }
}

// ---- the prototype gradients back to the support rows ------------------------------------------------------------------------------
// Workgroup (episode b, classes c0 .. c0 + nc, features f0 .. f0 + nf) holds dc [16, FH_LDC] in LDS: every support row of class n
// receives dc_n / count_n; the first class block (`zero_left_out`) zeroes the rows whose label is out of range.
__device__ __forceinline__ void fh_scatter_class_grad(const float* dc, const int64_t* ys, const float* cntf,
                                                      float* dfs, int b, int S, int N, int F, int c0, int nc, int f0,
                                                      int nf, bool zero_left_out) {
    const int tid = threadIdx.x, n = tid & (FH_NB - 1);
    if (n >= nf) return;
    for (int i = tid >> 7; i < S; i += 2) {
        const long t = ys[(long)b * S + i];
        float* o = dfs + ((long)b * S + i) * F + f0 + n;
        if (t >= 0 && t < N) {
            const int m = (int)t - c0;
            if (m >= 0 && m < nc) *o = dc[m * FH_LDC + n] / cntf[(long)b * N + t];
        } else if (zero_left_out) {
            *o = 0.f;
        }
    }
}
