// Logistic-regression few-shot head fitted in LDS (the frozen-backbone protocol of Tian et al. 2020).  Forward only.
// Per episode, with X the support rows [S,F], x~_i = x_i / max(|x_i|, 1e-12) when `normalize` (the query rows alike), n the number of
// support rows with a label in [0, N) (at least 1), wd = 1 / (C n):
//     f(W, b) = (1/n) sum_i CE(W^T x~_i + b, y_i) + (wd/2) |W|^2,
// T steps of heavy-ball descent V <- beta V + grad, (W, b) <- (W, b) - eta V from zero.  Every iterate is W_t = X~^T A_t with A_t [S,N],
// so the fit iterates on K~ = X~ X~^T alone (K~_ij = K_ij / (|x_i| |x_j|), the norms from the diagonal of K = X X^T):
//     Z = K~ A + 1 b^T,  P = softmax_rows(Z),  R = (P - Y) / n,  VA <- beta VA + R + wd A,  Vb <- beta Vb + colsum(R),
//     A <- A - eta VA,  b <- b - eta Vb,
// and the query logits are z = Fq~ W_T + b_T.
//
//   launch 1, one workgroup per episode: Gram matrix through wg_mm into LDS at an odd row stride, rows and columns of left-out rows
//       zeroed, inverse norms from the diagonal, then the T steps with K~, A, VA, b, Vb and the labels in LDS or registers; no global
//       access between the Gram product and the store of A' (A'_i = A_i / |x_i|, so W = X^T A') and b.  A thread owns the elements
//       (i, n) of A and VA with n = tid % NP and i = tid / NP + p * (256 / NP), NP = N rounded up to a power of two: a row of Z is NP
//       adjacent lanes of one wave and its softmax two fixed-order butterflies, Z itself never leaves registers.  b and Vb are kept by
//       every thread for its own column (the same operations in the same order everywhere).
//       BARRIERS: ONE per solver step.  A is double-buffered (a step reads all of A_t and each thread writes its own elements of
//       A_t+1), the per-wave column sums of R alternate between two slots, so the only hazard left is "every A_t+1 and column sum
//       written before the next step reads them".  When the 64 KB staging area (both copies of A live there after the Gram product),
//       K~ and VA do not fit the 160 KB of a CU (only S >= 126 with N > 32) VA takes the place of the second copy, A is updated in
//       place after the step's reads and a step has TWO barriers.  LDS request at S = 128, N = 64: 134656 bytes (131.5 KB).
//       K~ A [S,S] x [S,NP] exists in two forms, chosen per shape by the host (fumi_hip_logreg_set_form overrides the choice):
//       the VALU loop above, and the f32 MFMA (v_mfma_f32_16x16x4_f32, logreg_fit_mfma_kernel): K~ zero-padded to [Sp, Sp + 4]
//       (Sp = S rounded up to 16; one ds_read_b128 gives a lane its 4 k values), A at the row stride max(NP, 16) + 4 (= 4 mod 8:
//       the 4 ds_read_b32 of a lane are conflict-free), a wave owns row tiles wave, wave + 4 with all column tiles of a row tile
//       in its accumulators, so a row of Z is 16 lanes x CT registers and its softmax stays in registers as well; the same
//       double-buffering and barrier count (two barriers when S > 112 with N > 32).
//   launch 2, one workgroup per (episode, 128 features): W^T = A'^T X [N,F].
//   launch 3, one workgroup per (episode, tile of 16 query rows): the tile's inverse row norms, u = f_tile W on the f32 MFMA into LDS,
//       z = u / |f| + b; per row first arg-max, log-sum-exp, NLL; the tile's loss and correct sums go to part[tile].
//   launch 4, one workgroup: the tile partials added in index order into loss and correct.
// Fixed summation orders, the first arg-max, the label-range and missing-class rules and the absence of floating-point atomics are
// those of fewshot_head.h.  The fit runs a fixed number of steps whatever the values are.  A support row left out is a zero row and
// column of K~ and zero rows of Y and R, and is not counted in n; a class without a support row is fitted like any class.
// After the Gram product the fit keeps A (and A' or VA) in the FH_MM floats of the products' staging area.
#include "fewshot_head.h"

namespace {

constexpr size_t LR_LDS_MAX = 160 * 1024;
// the form of K~ A the host picks when none is forced (measured, profiles/logreg_head/): the MFMA from S * NP elements of Z on
#define LOGREG_AUTO_MFMA(S, NP) ((S) * (NP) >= 1024)

struct Logreg {
    int B, S, Qn, N, F, ldz, tpe, ntile, ldl, NP, lg, nfb, steps, normalize, db, Sp, lda, body;   // Sp, lda, body: the MFMA form's
    float lr, beta, C;
};

__global__ __launch_bounds__(256) void logreg_fit_kernel(Logreg d, const float* __restrict__ xs, const int64_t* __restrict__ ys,
                                                         float* __restrict__ Aw, float* __restrict__ bw, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = d.S, N = d.N, F = d.F, ldl = d.ldl, NP = d.NP, SN = S * NP;
    const int b = blockIdx.x;
    float* mm = sm;                              // wg_mm's staging area, then A [S, NP] twice (or A and VA)
    float* Km = mm + FH_MM;                      // [S, ldl]
    float* A0 = mm;
    float* A1 = mm + SN;                         // the second copy of A when double-buffered
    float* VA = d.db ? Km + S * ldl : mm + SN;   // [S, NP]
    float* inv = Km + S * ldl + (d.db ? SN : 0); // [S] 1 / |x_i|, 0 for a row left out
    int* lab = (int*)(inv + S);                  // [S] labels, -1 where out of range
    float* red = (float*)(lab + S);              // [2][4][64] per-wave column sums of R, two slots
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
    int cnt = 0;
    for (int i = 0; i < S; ++i) cnt += lab[i] >= 0 ? 1 : 0;
    const float nf = (float)max(cnt, 1), invn = 1.f / nf, wd = 1.f / (d.C * nf), eta = d.lr, beta = d.beta;
    const float* X = xs + (long)b * S * F;
    wg_mm(mm, FH_MM, S, S, F, X, F, 1, X, 1, F, [&](int m, int n, float acc) { Km[m * ldl + n] = acc; });
    __syncthreads();
    for (int i = tid; i < S; i += 256)
        inv[i] = lab[i] < 0 ? 0.f : (d.normalize ? 1.f / fmaxf(sqrtf(Km[i * ldl + i]), 1e-12f) : 1.f);
    for (int t = tid; t < SN; t += 256) { A0[t] = 0.f; VA[t] = 0.f; }
    __syncthreads();
    for (int i = tid >> 5; i < S; i += 8)
        for (int j = tid & 31; j < S; j += 32) {
            const float si = inv[i], sj = inv[j];
            Km[i * ldl + j] = (si != 0.f && sj != 0.f) ? Km[i * ldl + j] * si * sj : 0.f;
        }
    __syncthreads();

    const int n = tid & (NP - 1), r = tid >> d.lg, rs = 256 >> d.lg;
    const bool col = n < N;
    float bn = 0.f, vbn = 0.f;                   // b[n] and Vb[n], in every thread of column n
    for (int t = 0; t < d.steps; ++t) {
        const float* Ac = (d.db && (t & 1)) ? A1 : A0;
        float* An = (d.db && !(t & 1)) ? A1 : A0;
        float cs = 0.f;
        for (int i0 = 0; i0 < S; i0 += rs) {     // every lane runs every pass: the butterflies need the whole wave
            const bool act = i0 + r < S;
            const int i = act ? i0 + r : S - 1;
            const float* kr = Km + i * ldl;
            const float* ac = Ac + n;
            float z = 0.f;
#pragma unroll 16
            for (int j = 0; j < S; ++j) z = fmaf(kr[j], ac[j * NP], z);   // (one chain in index order; the unroll only batches the LDS reads)
            z += bn;
            float mx = col ? z : -INFINITY;
            for (int o = NP >> 1; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            const float e = col ? expf(z - mx) : 0.f;
            float s = e;
            for (int o = NP >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            const int li = lab[i];
            const float rr = (act && col && li >= 0) ? (e / s - (li == n ? 1.f : 0.f)) * invn : 0.f;
            if (act) {
                const int k = i * NP + n;
                const float a = Ac[k], va = beta * VA[k] + rr + wd * a;
                VA[k] = va;
                if (d.db) An[k] = a - eta * va;
            }
            cs += rr;
        }
        for (int o = NP; o < 64; o <<= 1) cs += __shfl_xor(cs, o, 64);   // the lanes of this wave that hold column n
        float* rd = red + (t & 1) * 256;
        if (lane < NP) rd[wave * 64 + n] = cs;
        __syncthreads();
        if (!d.db)
            for (int i = r; i < S; i += rs) A0[i * NP + n] -= eta * VA[i * NP + n];
        vbn = beta * vbn + (((rd[n] + rd[64 + n]) + rd[128 + n]) + rd[192 + n]);
        bn -= eta * vbn;
        if (!d.db) __syncthreads();
    }
    const float* Af = (d.db && (d.steps & 1)) ? A1 : A0;
    if (col)
        for (int i = r; i < S; i += rs) Aw[((long)b * S + i) * N + n] = Af[i * NP + n] * inv[i];   // a thread's own elements
    if (r == 0 && col) bw[(long)b * N + n] = bn;
}

// The fit with K~ A on the f32 MFMA.  LDS: K~ [Sp, Sp + 4] | body: wg_mm's staging area, then A [Sp, lda], VA and (double-buffered)
// the second A | 1 / |x_i| [S] | labels [S] | column sums [2][4][64].  CT = column tiles of 16 (NP <= 16: 1, 32: 2, 64: 4).
template <int CT>
__global__ __launch_bounds__(256) void logreg_fit_mfma_kernel(Logreg d, const float* __restrict__ xs, const int64_t* __restrict__ ys,
                                                              float* __restrict__ Aw, float* __restrict__ bw, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int S = d.S, N = d.N, F = d.F, Sp = d.Sp, ldk = Sp + 4, lda = d.lda, SA = Sp * lda;
    const int b = blockIdx.x;
    float* Km = sm;                              // [Sp, ldk], zero past S
    float* mm = Km + Sp * ldk;
    float* A0 = mm;                              // [Sp, lda], zero past S and past N
    float* VA = mm + SA;
    float* A1 = mm + 2 * SA;                     // (double-buffered only)
    float* inv = mm + d.body;                    // [S] 1 / |x_i|, 0 for a row left out
    int* lab = (int*)(inv + S);                  // [S] labels, -1 where out of range
    float* red = (float*)(lab + S);              // [2][4][64] per-wave column sums of R, two slots
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
    int cnt = 0;
    for (int i = 0; i < S; ++i) cnt += lab[i] >= 0 ? 1 : 0;
    const float nf = (float)max(cnt, 1), invn = 1.f / nf, wd = 1.f / (d.C * nf), eta = d.lr, beta = d.beta;
    const float* X = xs + (long)b * S * F;
    wg_mm(mm, FH_MM, S, S, F, X, F, 1, X, 1, F, [&](int m, int n, float acc) { Km[m * ldk + n] = acc; });
    __syncthreads();
    for (int i = tid; i < S; i += 256)
        inv[i] = lab[i] < 0 ? 0.f : (d.normalize ? 1.f / fmaxf(sqrtf(Km[i * ldk + i]), 1e-12f) : 1.f);
    for (int t = tid; t < (d.db ? 3 : 2) * SA; t += 256) A0[t] = 0.f;
    __syncthreads();
    for (int i = tid >> 5; i < Sp; i += 8)
        for (int j = tid & 31; j < ldk; j += 32) {
            float v = 0.f;
            if (i < S && j < S) { const float si = inv[i], sj = inv[j]; if (si != 0.f && sj != 0.f) v = Km[i * ldk + j] * si * sj; }
            Km[i * ldk + j] = v;
        }
    __syncthreads();

    float bn[CT], vbn[CT];                       // b and Vb of columns r + 16 c, in every lane that holds them
#pragma unroll
    for (int c = 0; c < CT; ++c) { bn[c] = 0.f; vbn[c] = 0.f; }
    const int ntile = Sp >> 4;
    for (int t = 0; t < d.steps; ++t) {
        const float* Ac = (d.db && (t & 1)) ? A1 : A0;
        float* An = (d.db && !(t & 1)) ? A1 : A0;
        float cs[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) cs[c] = 0.f;
        for (int rt = wave; rt < ntile; rt += 4) {       // wave-uniform
            const int m0 = rt << 4;
            f32x4 acc[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* kp = Km + (m0 + r) * ldk + 4 * q;
            const float* ap = Ac + 4 * q * lda + r;
            for (int kk = 0; kk < Sp; kk += 16) {        // lane (r, q) feeds k = kk + 4 q + e on the e-th MFMA, for both operands
                const f32x4 av = *(const f32x4*)(kp + kk);
                f32x4 bv[CT];
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const float* p = ap + kk * lda + 16 * c;
                    bv[c][0] = p[0]; bv[c][1] = p[lda]; bv[c][2] = p[2 * lda]; bv[c][3] = p[3 * lda];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int c = 0; c < CT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[c][e], acc[c], 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {                // register e of lane (r, q): row m0 + 4 q + e, columns r + 16 c
                const int i = m0 + 4 * q + e;
                const bool act = i < S;
                float z[CT], ex[CT];
                float mx = -INFINITY;
#pragma unroll
                for (int c = 0; c < CT; ++c) { z[c] = acc[c][e] + bn[c]; if (r + 16 * c < N) mx = fmaxf(mx, z[c]); }
                for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < CT; ++c) { ex[c] = r + 16 * c < N ? expf(z[c] - mx) : 0.f; s += ex[c]; }
                for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                const int li = lab[act ? i : S - 1];
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const int n = r + 16 * c;
                    const float rr = (act && n < N && li >= 0) ? (ex[c] / s - (li == n ? 1.f : 0.f)) * invn : 0.f;
                    if (act) {
                        const int k = i * lda + n;
                        const float a = Ac[k], va = beta * VA[k] + rr + wd * a;
                        VA[k] = va;
                        if (d.db) An[k] = a - eta * va;
                    }
                    cs[c] += rr;
                }
            }
        }
        float* rd = red + (t & 1) * 256;
#pragma unroll
        for (int c = 0; c < CT; ++c) {                   // the four lanes of this wave that hold column r + 16 c
            cs[c] += __shfl_xor(cs[c], 16, 64);
            cs[c] += __shfl_xor(cs[c], 32, 64);
            if (lane < 16) rd[wave * 64 + 16 * c + r] = cs[c];
        }
        __syncthreads();
        if (!d.db)
            for (int rt = wave; rt < ntile; rt += 4)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = (rt << 4) + 4 * q + e;
                    if (i < S)
#pragma unroll
                        for (int c = 0; c < CT; ++c) { const int k = i * lda + r + 16 * c; A0[k] -= eta * VA[k]; }
                }
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int n = r + 16 * c;
            vbn[c] = beta * vbn[c] + (((rd[n] + rd[64 + n]) + rd[128 + n]) + rd[192 + n]);
            bn[c] -= eta * vbn[c];
        }
        if (!d.db) __syncthreads();
    }
    const float* Af = (d.db && (d.steps & 1)) ? A1 : A0;
    for (int t = tid; t < S * N; t += 256) { const int i = t / N, n = t - i * N; Aw[((long)b * S + i) * N + n] = Af[i * lda + n] * inv[i]; }
    if (tid < 16)
#pragma unroll
        for (int c = 0; c < CT; ++c) if (r + 16 * c < N) bw[(long)b * N + r + 16 * c] = bn[c];
}

__global__ __launch_bounds__(256) void logreg_w_kernel(Logreg d, const float* __restrict__ xs, const float* __restrict__ Aw,
                                                       float* __restrict__ Wt) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int S = d.S, N = d.N, F = d.F;
    const int b = blockIdx.x / d.nfb, f0 = (blockIdx.x - b * d.nfb) * FH_NB, nf = min(FH_NB, F - f0);
    // W^T[m, f0 + n] = sum_k A'[k, m] X[k, f0 + n]
    wg_mm(sm, FH_MM, N, nf, S, Aw + (long)b * S * N, 1, N, xs + (long)b * S * F + f0, F, 1,
          [&](int m, int n, float acc) { Wt[((long)b * N + m) * F + f0 + n] = acc; });
}

__global__ __launch_bounds__(256) void logreg_rows_kernel(Logreg d, const float* __restrict__ fq, const int64_t* __restrict__ yq,
                                                          const float* __restrict__ Wt, const float* __restrict__ bw,
                                                          int64_t* __restrict__ preds, float* __restrict__ logits,
                                                          float* __restrict__ part, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int Qn = d.Qn, N = d.N, F = d.F, ldz = d.ldz;
    const int b = blockIdx.x / d.tpe, q0 = (blockIdx.x - b * d.tpe) * FH_TM, rows = min(FH_TM, Qn - q0);
    const long r0 = (long)b * Qn + q0;           // the tile's first row among all B * Qn
    float* Z = sm;                               // [16, ldz] u, then z
    float* rl = Z + FH_TM * ldz;                 // [16] row losses, [16] row hits
    float* iq = rl + 32;                         // [16] 1 / |f_row|
    float* mm = iq + 16;
    const float* ft = fq + r0 * F;
    const float* wt = Wt + (long)b * N * F;
    const float* bb = bw + (long)b * N;
    const int row = tid >> 4, l = tid & 15;      // 16 lanes per row

    {   // the tile's inverse row norms: 16 lanes stride over the row, a fixed-order butterfly
        float s = 0.f;
        if (d.normalize && row < rows) {
            const float* f = ft + (long)row * F;
            for (int k = 4 * l; k < F; k += 64) { const f32x4 v = *(const f32x4*)(f + k); s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }
        }
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (l == 0) iq[row] = d.normalize ? 1.f / fmaxf(sqrtf(s), 1e-12f) : 1.f;
    }
    wg_mm(mm, FH_MM, rows, N, F, ft, F, 1, wt, 1, F, [&](int m, int n, float acc) { Z[m * ldz + n] = acc; });
    __syncthreads();
    for (int t = tid; t < rows * N; t += 256) { const int m = t / N, n = t - m * N; Z[m * ldz + n] = Z[m * ldz + n] * iq[m] + bb[n]; }
    __syncthreads();

    {
        float loss = 0.f, hit = 0.f;
        if (row < rows) {
            const float* c = Z + row * ldz;
            float z[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; z[j] = n < N ? c[n] : 0.f; }
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
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) s += l + 16 * j < N ? expf(z[j] - mx) : 0.f;
            for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            long yv = yq[r0 + row];
            const bool ok = yv >= 0 && yv < N;
            if (!ok) { if (l == 0) atomicOr(status, FUMI_ST_LABEL_RANGE); yv = 0; }
            loss = ok ? mx + logf(s) - c[yv] : 0.f;
            hit = (ok && arg == (int)yv) ? 1.f : 0.f;
            if (l == 0 && preds) preds[r0 + row] = arg;
            if (logits) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; if (n < N) logits[(r0 + row) * N + n] = z[j]; }
            }
        }
        if (l == 0) { rl[row] = loss; rl[16 + row] = hit; }
    }
    __syncthreads();
    fh_tile_part<2>(rl, part, d.ntile);
}

__global__ __launch_bounds__(256) void logreg_sum_kernel(Logreg d, const float* __restrict__ part, float* __restrict__ loss,
                                                         float* __restrict__ correct) {
    __shared__ float sm[512];
    fh_sum_parts<2>(part, d.ntile, sm, [&](const float (&t)[2]) {      // the sums over the row tiles
        loss[0] = t[0] / (float)((long)d.B * d.Qn); correct[0] = t[1];
    });
}

int g_logreg_form = -1;           // -1: chosen per shape, 0: VALU loop, 1: f32 MFMA

}  // namespace

extern "C" int fumi_hip_logreg_set_form(int form) {
    if (form < -1 || form > 1) return FUMI_EINVAL;
    g_logreg_form = form;
    return FUMI_OK;
}

extern "C" int fumi_hip_logreg_head_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, int steps, float lr, float momentum, float C,
        int normalize, float* loss, float* correct, int64_t* preds, float* logits) {
    const bool own = S <= 128 && steps >= 1 && steps <= 10000 && lr > 0.f && momentum >= 0.f && momentum < 1.f && C > 0.f;
    if (int rc = head_args_check(ws, B, S, Qn, N, F, own, {feats_s, y_s, feats_q, y_q, loss, correct})) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    Logreg d;
    head_rows_fill(d, B, S, Qn, N, F);
    d.ldl = S | 1; d.lg = 1; while ((1 << d.lg) < N) ++d.lg;
    d.NP = 1 << d.lg; d.nfb = (F + FH_NB - 1) / FH_NB;
    d.steps = steps; d.normalize = normalize ? 1 : 0; d.lr = lr; d.beta = momentum; d.C = C;
    const size_t fit_small = ((size_t)2 * S + 512) * 4;   // 1 / |x|, labels, two slots of per-wave column sums
    const bool mfma = g_logreg_form == 1 || (g_logreg_form < 0 && LOGREG_AUTO_MFMA(S, d.NP));
    size_t lds1;
    d.Sp = (S + 15) & ~15; d.lda = (d.NP < 16 ? 16 : d.NP) + 4; d.body = 0;
    if (mfma) {                                 // K~ [Sp, Sp + 4] | max(staging, A, VA [, A]) | small
        const size_t SA = (size_t)d.Sp * d.lda, km = (size_t)d.Sp * (d.Sp + 4);
        auto body = [&](size_t nbuf) { return nbuf * SA > (size_t)FH_MM ? nbuf * SA : (size_t)FH_MM; };
        d.db = (km + body(3)) * 4 + fit_small <= LR_LDS_MAX ? 1 : 0;
        d.body = (int)body(d.db ? 3 : 2);
        lds1 = (km + d.body) * 4 + fit_small;
    } else {                                    // staging / A twice (S NP <= 8192 floats each) | K~ [S, S | 1] | [VA] | small
        const size_t lds_db = ((size_t)FH_MM + S * d.ldl + S * d.NP) * 4 + fit_small;
        d.db = lds_db <= LR_LDS_MAX ? 1 : 0;
        lds1 = d.db ? lds_db : ((size_t)FH_MM + S * d.ldl) * 4 + fit_small;
    }
    const size_t lds2 = (size_t)FH_MM * 4;
    const size_t lds3 = ((size_t)FH_TM * d.ldz + 48 + FH_MM) * 4;
    const size_t n_A = (size_t)B * S * N, n_b = (size_t)B * N, n_W = (size_t)B * N * F, n_part = (size_t)2 * d.ntile;
    int rc = ws_reserve(ws, ws_align(n_A * 4) + ws_align(n_b * 4) + ws_align(n_W * 4) + ws_align(n_part * 4));
    if (rc) return rc;
    float* Aw = ws_f(ws, n_A); float* bw = ws_f(ws, n_b); float* Wt = ws_f(ws, n_W); float* part = ws_f(ws, n_part);
    if (mfma && d.NP <= 16) {
        FUMI_SET_DYN_LDS(logreg_fit_mfma_kernel<1>, lds1);
        hipLaunchKernelGGL(logreg_fit_mfma_kernel<1>, dim3(B), dim3(256), lds1, st, d, feats_s, y_s, Aw, bw, ws->status);
    } else if (mfma && d.NP == 32) {
        FUMI_SET_DYN_LDS(logreg_fit_mfma_kernel<2>, lds1);
        hipLaunchKernelGGL(logreg_fit_mfma_kernel<2>, dim3(B), dim3(256), lds1, st, d, feats_s, y_s, Aw, bw, ws->status);
    } else if (mfma) {
        FUMI_SET_DYN_LDS(logreg_fit_mfma_kernel<4>, lds1);
        hipLaunchKernelGGL(logreg_fit_mfma_kernel<4>, dim3(B), dim3(256), lds1, st, d, feats_s, y_s, Aw, bw, ws->status);
    } else {
        FUMI_SET_DYN_LDS(logreg_fit_kernel, lds1);
        hipLaunchKernelGGL(logreg_fit_kernel, dim3(B), dim3(256), lds1, st, d, feats_s, y_s, Aw, bw, ws->status);
    }
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(logreg_w_kernel, lds2);
    hipLaunchKernelGGL(logreg_w_kernel, dim3(B * d.nfb), dim3(256), lds2, st, d, feats_s, Aw, Wt);
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(logreg_rows_kernel, lds3);
    hipLaunchKernelGGL(logreg_rows_kernel, dim3(d.ntile), dim3(256), lds3, st, d, feats_q, y_q, Wt, bw, preds, logits, part, ws->status);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(logreg_sum_kernel, dim3(1), dim3(256), 0, st, d, part, loss, correct);
    LAUNCH_CHECK();
    return FUMI_OK;
}
