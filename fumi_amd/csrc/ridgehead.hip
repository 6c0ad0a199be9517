// Ridge-regression few-shot head with a backward (R2-D2 / the ridge head of MetaOptNet).  Per episode, with X the
// support rows [S,F], Y their one-hot labels [S,N], Fq the query rows [Qn,F], lam = exp(rho), params = (rho, alpha) in device memory:
//     M = X X^T + lam I,   A = M^-1 Y,   W = X^T A,   u = Fq W,   z = alpha u,
// mean softmax cross-entropy of z over all B * Qn query rows, first arg-max predictions, and the gradients of grad_scale * loss:
//     dz = grad_scale / (B Qn) (softmax(z) - onehot),   dFq = alpha dz W^T,   dW = alpha Fq^T dz,   G = M^-1 (X dW),
//     dX = A (dW - X^T G)^T - G W^T,   dalpha = sum dz u,   drho = -lam sum G A.
// M is symmetric positive definite, so one Cholesky factor L (M = L L^T) serves both solves.
//
//   launch 1, one workgroup per episode: Gram matrix through wg_mm into LDS (rows and columns of a support row whose label is out of
//       range are zeroed: the row is left out exactly), lam on the diagonal, right-looking Cholesky in LDS, forward and back
//       substitution for the N right-hand sides; A, L and 1 / diag(L) go to the workspace.
//   launch 2, one workgroup per (episode, 128 features): W^T = A^T X [N,F].
//   launch 3, one workgroup per (episode, tile of 16 query rows): u = f_tile W on the f32 MFMA, kept in LDS; per row first arg-max,
//       log-sum-exp, NLL; the tile's loss / correct / dalpha sums go to part[tile].  Training form: dFq = (alpha dz) W^T, dz to memory.
//   launch 4, one workgroup per (episode, 128 features) over ALL Qn rows: dW^T block = alpha dz^T Fq, then this block's share of X dW
//       as a partial [S,N].
//   launch 5, one workgroup per episode: the partials added in block order, G = M^-1 (X dW) from the stored L, the episode's
//       -lam sum G A.
//   launch 6, one workgroup per (episode, 128 features): D = dW^T - G^T X in LDS, dX = A D - G W^T; one further workgroup adds the
//       tile and episode partials in index order into loss, correct and dparams.
//   The forward form (no gradient pointers) is launches 1 to 3 without the backward half of launch 3, and the last workgroup of
//   launch 6: the same instructions produce loss, correct, preds and logits in both forms.
// Fixed summation orders, the first arg-max, the label-range and missing-class rules and the absence of floating-point atomics are
// those of fewshot_head.h.  A class without a support row has logits 0; a pivot that is not > 0 (a NaN counts) sets
// FUMI_ST_NOT_POSDEF and is replaced by lam.  rho and alpha are read from device memory by the kernels.
#include "fewshot_head.h"

namespace {

struct Ridge {                     // (HeadDims' fields without nfb1, filled by head_rows_fill)
    int B, S, Qn, N, F, ldz, tpe, ntile, ldl, NP, lg, nfb, train;   // ldl: odd row stride of L; NP = 1 << lg: N rounded up to a power of two
    float gs;                                                       // grad_scale / (B Qn)
};

// R [S, NP] in LDS <- (L L^T)^-1 R with the strict lower triangle of L [S, ldl] and dinv = 1 / diag(L), both in LDS.  Column-oriented
// substitution: at step j every row past j takes its update from row j, lanes run along the right-hand sides (contiguous in R, L read
// as a broadcast), one barrier per step.  Rows are scaled by dinv after each sweep, so nothing is written where another thread reads.
__device__ __forceinline__ void ridge_solve(const float* L, int ldl, const float* dinv, float* R, int S, int NP, int lg) {
    const int tid = threadIdx.x, n = tid & (NP - 1), r = tid >> lg, rs = 256 >> lg;
    for (int j = 0; j < S; ++j) {                // L y = R
        __syncthreads();
        const float yj = R[j * NP + n] * dinv[j];
        for (int i = j + 1 + r; i < S; i += rs) R[i * NP + n] -= L[i * ldl + j] * yj;
    }
    __syncthreads();
    for (int i = r; i < S; i += rs) R[i * NP + n] *= dinv[i];
    for (int j = S - 1; j >= 0; --j) {           // L^T a = y
        __syncthreads();
        const float aj = R[j * NP + n] * dinv[j];
        for (int i = r; i < j; i += rs) R[i * NP + n] -= L[j * ldl + i] * aj;
    }
    __syncthreads();
    for (int i = r; i < S; i += rs) R[i * NP + n] *= dinv[i];
    __syncthreads();
}

__global__ __launch_bounds__(256) void ridge_factor_kernel(Ridge d, const float* __restrict__ xs, const int64_t* __restrict__ ys,
                                                           const float* __restrict__ params, float* __restrict__ Lw,
                                                           float* __restrict__ dinvw, float* __restrict__ Aw, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, N = d.N, F = d.F, ldl = d.ldl, NP = d.NP;
    const int b = blockIdx.x;
    float* mm = sm;                              // wg_mm's staging area, then Y / A [S, NP]
    float* Lm = mm + FH_MM;                      // [S, ldl]
    float* dinv = Lm + S * ldl;                  // [S]
    int* lab = (int*)(dinv + S);                 // [S] labels, -1 where out of range
    const float lam = expf(params[0]);
    // (the label block of fewshot_head.h, kept inline: through the helpers this kernel's long loops below measured 0.5 - 1 % slower)
    bool bad = false;
    for (int i = tid; i < S; i += 256) {
        const long t = ys[(long)b * S + i];
        const bool ok = t >= 0 && t < N;
        lab[i] = ok ? (int)t : -1;
        bad |= !ok;
    }
    if (bad) atomicOr(status, FUMI_ST_LABEL_RANGE);
    __syncthreads();
    if (tid < N) {
        int c = 0;
        for (int i = 0; i < S; ++i) c += lab[i] == tid ? 1 : 0;
        if (c == 0) atomicOr(status, FUMI_ST_CLASS_MISSING);
    }
    const float* X = xs + (long)b * S * F;
    wg_mm(mm, FH_MM, S, S, F, X, F, 1, X, 1, F, [&](int m, int n, float acc) {
        const float v = (lab[m] >= 0 && lab[n] >= 0) ? acc : 0.f;
        Lm[m * ldl + n] = m == n ? v + lam : v;
    });
    // right-looking Cholesky of the lower triangle.  Column j stays unscaled while the sweep runs (its scale 1 / sqrt(pivot) is applied
    // where it is read), so a step writes only columns past j and one barrier per column is enough.  Each half-wave updates 32
    // consecutive columns of one row: the row read is contiguous, L[i][j] a broadcast, L[k][j] runs down a column at the odd stride.
    for (int j = 0; j < S; ++j) {
        __syncthreads();
        float p = Lm[j * ldl + j];
        if (!(p > 0.f)) { p = lam; if (tid == 0) atomicOr(status, FUMI_ST_NOT_POSDEF); }
        const float inv = 1.f / sqrtf(p);
        if (tid == 0) dinv[j] = inv;
        for (int i = j + 1 + (tid >> 5); i < S; i += 8) {
            const float lij = Lm[i * ldl + j] * inv;
            for (int k = j + 1 + (tid & 31); k <= i; k += 32) Lm[i * ldl + k] -= lij * (Lm[k * ldl + j] * inv);
        }
    }
    __syncthreads();
    for (int i = tid >> 5; i < S; i += 8)
        for (int j = tid & 31; j < i; j += 32) Lm[i * ldl + j] *= dinv[j];
    float* Y = mm;
    for (int t = tid; t < S * NP; t += 256) { const int i = t >> d.lg, n = t & (NP - 1); Y[t] = lab[i] == n ? 1.f : 0.f; }
    ridge_solve(Lm, ldl, dinv, Y, S, NP, d.lg);
    for (int t = tid; t < S * NP; t += 256) { const int i = t >> d.lg, n = t & (NP - 1); if (n < N) Aw[((long)b * S + i) * N + n] = Y[t]; }
    for (int t = tid; t < S * ldl; t += 256) Lw[(long)b * S * ldl + t] = Lm[t];
    for (int i = tid; i < S; i += 256) dinvw[(long)b * S + i] = dinv[i];
}

__global__ __launch_bounds__(256) void ridge_w_kernel(Ridge d, const float* __restrict__ xs, const float* __restrict__ Aw,
                                                      float* __restrict__ Wt) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int S = d.S, N = d.N, F = d.F;
    const int b = blockIdx.x / d.nfb, f0 = (blockIdx.x - b * d.nfb) * FH_NB, nf = min(FH_NB, F - f0);
    // W^T[m, f0 + n] = sum_k A[k, m] X[k, f0 + n]
    wg_mm(sm, FH_MM, N, nf, S, Aw + (long)b * S * N, 1, N, xs + (long)b * S * F + f0, F, 1,
          [&](int m, int n, float acc) { Wt[((long)b * N + m) * F + f0 + n] = acc; });
}

__global__ __launch_bounds__(256) void ridge_rows_kernel(Ridge d, const float* __restrict__ fq, const int64_t* __restrict__ yq,
                                                         const float* __restrict__ Wt, const float* __restrict__ params,
                                                         int64_t* __restrict__ preds, float* __restrict__ logits,
                                                         float* __restrict__ part, float* __restrict__ dzw, float* __restrict__ dfq,
                                                         int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int Qn = d.Qn, N = d.N, F = d.F, ldz = d.ldz;
    const int b = blockIdx.x / d.tpe, q0 = (blockIdx.x - b * d.tpe) * FH_TM, rows = min(FH_TM, Qn - q0);
    const long r0 = (long)b * Qn + q0;           // the tile's first row among all B * Qn
    float* Z = sm;                               // [16, ldz] u, then alpha dz
    float* rl = Z + FH_TM * ldz;                 // [16] row losses, [16] row hits, [16] row dalpha
    float* mm = rl + 48;
    const float* ft = fq + r0 * F;
    const float* wt = Wt + (long)b * N * F;
    const float alpha = params[1];
    const int row = tid >> 4, l = tid & 15;      // 16 lanes per row

    wg_mm(mm, FH_MM, rows, N, F, ft, F, 1, wt, 1, F, [&](int m, int n, float acc) { Z[m * ldz + n] = acc; });
    __syncthreads();

    {
        float loss = 0.f, hit = 0.f, da = 0.f;
        if (row < rows) {
            float* c = Z + row * ldz;
            float us[4], z[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; us[j] = n < N ? c[n] : 0.f; z[j] = alpha * us[j]; }
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
            loss = ok ? mx + logf(s) - alpha * c[yv] : 0.f;
            hit = (ok && arg == (int)yv) ? 1.f : 0.f;
            if (l == 0 && preds) preds[r0 + row] = arg;
            if (logits) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; if (n < N) logits[(r0 + row) * N + n] = z[j]; }
            }
            if (d.train) {
                const float inv = 1.f / s, gs = ok ? d.gs : 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = l + 16 * j;
                    if (n < N) {
                        const float g = gs * (e[j] * inv - (n == (int)yv ? 1.f : 0.f));   // dz
                        da += g * us[j];
                        dzw[(r0 + row) * N + n] = g;
                        c[n] = alpha * g;
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
    // dfeats_tile [rows, F] = (alpha dz) [rows, N] W^T [N, F]
    for (int f0 = 0; f0 < F; f0 += FH_NB) {
        const int nb = min(FH_NB, F - f0);
        wg_mm(mm, FH_MM, rows, nb, N, Z, ldz, 1, wt + f0, F, 1,
              [&](int m, int n, float acc) { dfq[(r0 + m) * F + f0 + n] = acc; });
    }
}

__global__ __launch_bounds__(256) void ridge_dw_kernel(Ridge d, const float* __restrict__ xs, const float* __restrict__ fq,
                                                       const float* __restrict__ dzw, const float* __restrict__ params,
                                                       float* __restrict__ dWt, float* __restrict__ P) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int S = d.S, Qn = d.Qn, N = d.N, F = d.F;
    const int b = blockIdx.x / d.nfb, fb = blockIdx.x - b * d.nfb, f0 = fb * FH_NB, nf = min(FH_NB, F - f0);
    float* dWl = sm + FH_MM;                     // [N, FH_LDC] this block of dW^T
    const float alpha = params[1];
    // dW^T[m, f0 + n] = alpha sum_q dz[q, m] Fq[q, f0 + n]
    wg_mm(sm, FH_MM, N, nf, Qn, dzw + (long)b * Qn * N, 1, N, fq + (long)b * Qn * F + f0, F, 1, [&](int m, int n, float acc) {
        const float v = alpha * acc;
        dWl[m * FH_LDC + n] = v;
        dWt[((long)b * N + m) * F + f0 + n] = v;
    });
    __syncthreads();
    // this block's share of (X dW)[m, n] = sum_k X[m, f0 + k] dW^T[n, f0 + k]
    float* p = P + ((long)b * d.nfb + fb) * S * N;
    wg_mm(sm, FH_MM, S, N, nf, xs + (long)b * S * F + f0, F, 1, dWl, 1, FH_LDC, [&](int m, int n, float acc) { p[m * N + n] = acc; });
}

__global__ __launch_bounds__(256) void ridge_g_kernel(Ridge d, const int64_t* __restrict__ ys, const float* __restrict__ params,
                                                      const float* __restrict__ Lw, const float* __restrict__ dinvw,
                                                      const float* __restrict__ Aw, const float* __restrict__ P,
                                                      float* __restrict__ Gw, float* __restrict__ partd) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, N = d.N, ldl = d.ldl, NP = d.NP;
    const int b = blockIdx.x;
    float* Lm = sm;                              // [S, ldl]
    float* dinv = Lm + S * ldl;                  // [S]
    float* R = dinv + S;                         // [S, NP] X dW, then G
    float* red = R + S * NP;                     // [256]
    for (int t = tid; t < S * ldl; t += 256) Lm[t] = Lw[(long)b * S * ldl + t];
    for (int i = tid; i < S; i += 256) dinv[i] = dinvw[(long)b * S + i];
    for (int t = tid; t < S * NP; t += 256) {
        const int i = t >> d.lg, n = t & (NP - 1);
        const long y = ys[(long)b * S + i];
        float s = 0.f;
        if (n < N && y >= 0 && y < N)            // (a support row left out has a zero row of X)
            for (int k = 0; k < d.nfb; ++k) s += P[(((long)b * d.nfb + k) * S + i) * N + n];
        R[t] = s;
    }
    ridge_solve(Lm, ldl, dinv, R, S, NP, d.lg);
    float s = 0.f;
    for (int t = tid; t < S * NP; t += 256) {
        const int i = t >> d.lg, n = t & (NP - 1);
        if (n < N) { const float g = R[t]; Gw[((long)b * S + i) * N + n] = g; s += g * Aw[((long)b * S + i) * N + n]; }
    }
    red[tid] = s;
    __syncthreads();
    if (tid == 0) {
        float a = 0.f;
        for (int i = 0; i < 256; ++i) a += red[i];
        partd[b] = -expf(params[0]) * a;
    }
}

__global__ __launch_bounds__(256) void ridge_dx_kernel(Ridge d, const float* __restrict__ xs, const float* __restrict__ Aw,
                                                       const float* __restrict__ Gw, const float* __restrict__ Wt,
                                                       const float* __restrict__ dWt, const float* __restrict__ part,
                                                       const float* __restrict__ partd, float* __restrict__ loss,
                                                       float* __restrict__ correct, float* __restrict__ dparams, float* dfs) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, N = d.N, F = d.F;
    if (blockIdx.x == gridDim.x - 1) {           // the sums over the row tiles, and the episodes' drho in index order
        fh_sum_parts<3>(part, d.ntile, sm, [&](const float (&t)[3]) {
            loss[0] = t[0] / (float)((long)d.B * d.Qn); correct[0] = t[1];
            if (dparams) {
                float r = 0.f;
                for (int i = 0; i < d.B; ++i) r += partd[i];
                dparams[0] = r; dparams[1] = t[2];
            }
        });
        return;
    }
    const int b = blockIdx.x / d.nfb, f0 = (blockIdx.x - b * d.nfb) * FH_NB, nf = min(FH_NB, F - f0);
    float* Dl = sm + FH_MM;                      // [N, FH_LDC] dW^T - G^T X of this feature block
    const float* X = xs + (long)b * S * F + f0;
    const float* A = Aw + (long)b * S * N;
    const float* G = Gw + (long)b * S * N;
    float* o = dfs + (long)b * S * F + f0;
    wg_mm2(sm, FH_MM, N, nf, S, G, 1, N, X, F, 1,
           [&](int m, int n) { return dWt[((long)b * N + m) * F + f0 + n]; },
           [&](int m, int n, float acc, float w) { Dl[m * FH_LDC + n] = w - acc; });
    __syncthreads();
    // dX = A D - G W^T: the second product first, the first one added to what it left
    wg_mm(sm, FH_MM, S, nf, N, G, N, 1, Wt + (long)b * N * F + f0, F, 1, [&](int m, int n, float acc) { o[(long)m * F + n] = -acc; });
    __syncthreads();
    wg_mm2(sm, FH_MM, S, nf, N, A, N, 1, Dl, FH_LDC, 1,
           [&](int m, int n) { return o[(long)m * F + n]; },
           [&](int m, int n, float acc, float x) { o[(long)m * F + n] = x + acc; });
}

}  // namespace

extern "C" int fumi_hip_ridge_head_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* params, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* logits, float* dfeats_s, float* dfeats_q, float* dparams) {
    if (int rc = head_args_check(ws, B, S, Qn, N, F, S <= 128, {feats_s, y_s, feats_q, y_q, params, loss, correct})) return rc;
    const int train = head_grad_form(dfeats_s, dfeats_q, dparams);
    if (train < 0) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    Ridge d;
    head_rows_fill(d, B, S, Qn, N, F);
    d.ldl = S | 1; d.lg = 1; while ((1 << d.lg) < N) ++d.lg;
    d.NP = 1 << d.lg; d.nfb = (F + FH_NB - 1) / FH_NB; d.train = train;
    d.gs = head_grad_scale(grad_scale, B, Qn);
    const size_t n_L = (size_t)B * S * d.ldl, n_di = (size_t)B * S, n_A = (size_t)B * S * N, n_W = (size_t)B * N * F,
                 n_part = (size_t)3 * d.ntile, n_dz = (size_t)B * Qn * N, n_P = (size_t)B * d.nfb * S * N;
    int rc = ws_reserve(ws, ws_align(n_L * 4) + ws_align(n_di * 4) + ws_align(n_A * 4) + ws_align(n_W * 4) + ws_align(n_part * 4)
                            + (train ? ws_align(n_dz * 4) + ws_align(n_W * 4) + ws_align(n_P * 4) + ws_align(n_A * 4)
                                       + ws_align((size_t)B * 4) : 0));
    if (rc) return rc;
    float* Lw = ws_f(ws, n_L); float* dinvw = ws_f(ws, n_di); float* Aw = ws_f(ws, n_A); float* Wt = ws_f(ws, n_W);
    float* part = ws_f(ws, n_part);
    float* dzw = train ? ws_f(ws, n_dz) : nullptr; float* dWt = train ? ws_f(ws, n_W) : nullptr;
    float* P = train ? ws_f(ws, n_P) : nullptr; float* Gw = train ? ws_f(ws, n_A) : nullptr;
    float* partd = train ? ws_f(ws, (size_t)B) : nullptr;
    const size_t lds1 = ((size_t)FH_MM + S * d.ldl + 2 * S) * 4;
    const size_t lds2 = (size_t)FH_MM * 4;
    const size_t lds3 = ((size_t)FH_TM * d.ldz + 48 + FH_MM) * 4;
    const size_t lds4 = ((size_t)FH_MM + 64 * FH_LDC) * 4;
    const size_t lds5 = ((size_t)S * d.ldl + S + S * d.NP + 256) * 4;
    const size_t lds6 = train ? lds4 : (size_t)768 * 4;   // the forward form's one workgroup only adds the tile sums
    FUMI_SET_DYN_LDS(ridge_factor_kernel, lds1);
    hipLaunchKernelGGL(ridge_factor_kernel, dim3(B), dim3(256), lds1, st, d, feats_s, y_s, params, Lw, dinvw, Aw, ws->status);
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(ridge_w_kernel, lds2);
    hipLaunchKernelGGL(ridge_w_kernel, dim3(B * d.nfb), dim3(256), lds2, st, d, feats_s, Aw, Wt);
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(ridge_rows_kernel, lds3);
    hipLaunchKernelGGL(ridge_rows_kernel, dim3(d.ntile), dim3(256), lds3, st, d, feats_q, y_q, Wt, params, preds, logits, part, dzw,
                       dfeats_q, ws->status);
    LAUNCH_CHECK();
    if (train) {
        FUMI_SET_DYN_LDS(ridge_dw_kernel, lds4);
        hipLaunchKernelGGL(ridge_dw_kernel, dim3(B * d.nfb), dim3(256), lds4, st, d, feats_s, feats_q, dzw, params, dWt, P);
        LAUNCH_CHECK();
        FUMI_SET_DYN_LDS(ridge_g_kernel, lds5);
        hipLaunchKernelGGL(ridge_g_kernel, dim3(B), dim3(256), lds5, st, d, y_s, params, Lw, dinvw, Aw, P, Gw, partd);
        LAUNCH_CHECK();
    }
    FUMI_SET_DYN_LDS(ridge_dx_kernel, lds6);
    hipLaunchKernelGGL(ridge_dx_kernel, dim3((train ? B * d.nfb : 0) + 1), dim3(256), lds6, st, d, feats_s, Aw, Gw, Wt, dWt, part, partd,
                       loss, correct, dparams, dfeats_s);
    LAUNCH_CHECK();
    return FUMI_OK;
}
