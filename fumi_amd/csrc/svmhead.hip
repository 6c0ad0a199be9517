// MetaOptNet-SVM few-shot head with an implicit backward (Lee et al. 2019).  Per episode, with X the support rows
// [S,F], Y their one-hot labels [S,N], Fq the query rows [Qn,F], K' = X X^T + eps I, scale a learned scalar in device memory:
//     alpha* = argmin 1/2 tr(alpha^T K' alpha) - <alpha, Y>   s.t.  alpha_ik <= C Y_ik,  sum_k alpha_ik = 0     (Crammer-Singer dual)
//     W = X^T alpha*,   u = Fq W,   z = scale u,
// mean softmax cross-entropy of z over all B * Qn query rows, first arg-max predictions.
// FIT: T steps of FISTA from zero at the step 1 / L, L = max_i sum_j |K'_ij| (Gershgorin), t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2:
//     G = K' Zt - Y,   alpha+ = proj(Zt - G / L),   Zt <- alpha+ + (t_k - 1) / t_{k+1} (alpha+ - alpha).
// proj acts per row (v the row, u = C Y_i): a = min(v - tau, u), tau the root of sum_k min(v_k - tau, u_k) = 0, computed exactly from
// the breakpoints b_k = v_k - u_k (svm_proj below).  The entries with v_k - tau >= u_k of the LAST projection are the bound mask.
// BACKWARD: the implicit gradient at the fitted point.  free = not bound; P zeroes the bound entries and takes from every row the mean
// over its free entries (a row with fewer than two free entries becomes zero); dz = grad_scale / (B Qn) (softmax(z) - onehot):
//     dW = scale Fq^T dz,   g = X dW,   p: P K' P p = P g (Tb steps of conjugate gradients from zero, stopped when r.r <= 1e-12 r0.r0),
//     dX = alpha (dW - X^T p)^T - p W^T,   dFq = scale dz W^T,   dscale = sum dz u.
//
//   launch 1, one workgroup per episode (svm_fit_kernel): Gram matrix through wg_mm into LDS, zero-padded to [Sp, Sp + 4] (Sp = S
//       rounded up to 16), rows and columns of left-out rows zeroed, eps on the diagonal, L, then the T steps with K', Zt (twice) and
//       alpha in LDS: a step reads all of Zt_k and each thread writes its own elements of alpha and Zt_k+1, ONE barrier per step.
//       Where K', both Zt and alpha do not fit the 160 KB of a CU (S > 112 with N > 32) alpha, which only its owner touches, lives in
//       a scratch image in device memory instead; the barrier count stays.  LDS request at S = 128, N = 64: 138752 bytes.  Then
//       one more product for the KKT residual max |alpha - proj(alpha - (K' alpha - Y))|; alpha, the mask and K' go to the workspace.
//       K' Zt [S,S] x [S,N] exists in two forms (fumi_hip_svm_set_form overrides the host's choice): a VALU loop, a row of the result
//       being NP adjacent lanes (NP = N rounded up to a power of two), and the f32 MFMA (v_mfma_f32_16x16x4_f32), a row being 16
//       lanes x CT registers as in logreg_fit_mfma_kernel.  Both share the images (rows at the stride max(NP, 16) + 4 = 4 mod 8) and
//       the projection, which runs on the product's registers: G never exists in memory.
//   launch 2, one workgroup per (episode, 128 features): W^T = alpha^T X [N,F].
//   launch 3, one workgroup per (episode, tile of 16 query rows): u = f_tile W on the f32 MFMA, kept in LDS; per row first arg-max,
//       log-sum-exp, NLL; the tile's loss / correct / dscale sums go to part[tile].  Training form: dFq = (scale dz) W^T, dz to memory.
//   launch 4, one workgroup per (episode, 128 features) over ALL Qn rows: dW^T block = scale dz^T Fq, then this block's share of X dW
//       as a partial [S,N].
//   launch 5, one workgroup per episode (svm_cg_kernel): the partials added in block order, the conjugate gradients with K' and the
//       search direction in LDS (one K' d product per step, three barriers), q, r and p in LDS as far as they fit and else in scratch
//       images only their owners touch; p and the final relative residual sqrt(r.r / r0.r0) go to the workspace and to stats.
//   launch 6, one workgroup per (episode, 128 features): D = dW^T - p^T X in LDS, dX = alpha D - p W^T; one further workgroup adds the
//       tile partials in index order into loss, correct and dscale.
//   The forward form (no gradient pointers) is launches 1 to 3 without the backward half of launch 3, and the last workgroup of
//   launch 6: the same instructions produce loss, correct, preds and logits in both forms.
// Fixed summation orders, the first arg-max, the label-range and missing-class rules and the absence of floating-point atomics are
// those of fewshot_head.h.  The fit runs T steps whatever the values are; the CG's early exit is the same for every thread of an
// episode.  A support row left out has alpha_i = 0 and every entry bound, so p_i = 0 and its gradient row is zero.
#include "fewshot_head.h"

namespace {

constexpr size_t SVM_LDS_MAX = 160 * 1024;
constexpr float SVM_CG_FLOOR = 1e-12f;     // of r0.r0: past a relative residual of 1e-6 fp32 conjugate gradients only add noise
// the form of K' Zt the host picks when none is forced (measured, profiles/svm_head/): the MFMA from S * NP elements on
#define SVM_AUTO_MFMA(S, NP) ((S) * (NP) >= 1024)

struct Svm {                       // (HeadDims' fields without nfb1, filled by head_rows_fill)
    int B, S, Qn, N, F, ldz, tpe, ntile, NP, lg, nfb, train, T, Tb, Sp, ldk, lda, SA, body, nlds;   // SA = Sp * lda, one image;
    float C, eps, gs;                                                   // nlds: owner-only images kept in LDS (fit: 0 | 1, CG: 0 .. 3)
};

// The elements a thread owns and, with PROD, their products z = sum_j Km[i, j] Zc[j, n]: visit(i, act, z) once per row pass, by whole
// waves (visit may exchange lanes).  VALU form (MF false, CT 1): row i = i0 + tid / NP, column tid % NP; rows past S are visited
// with act false and i = S - 1.  MFMA form: a wave owns the row tiles wave, wave + 4, ..; register e of lane (r, q) is row
// m0 + 4 q + e, columns r + 16 c; act is i < S.
template <bool MF, int CT, bool PROD, class Visit>
__device__ __forceinline__ void svm_rows(const Svm& d, const float* Km, const float* Zc, Visit&& visit) {
    const int tid = threadIdx.x, S = d.S, ldk = d.ldk, lda = d.lda;
    if constexpr (MF) {
        const int lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4, Sp = d.Sp;
        for (int rt = wave; rt < (Sp >> 4); rt += 4) {   // wave-uniform
            const int m0 = rt << 4;
            f32x4 acc[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if constexpr (PROD) {
                const float* kp = Km + (m0 + r) * ldk + 4 * q;
                const float* ap = Zc + 4 * q * lda + r;
                for (int kk = 0; kk < Sp; kk += 16) {    // lane (r, q) feeds k = kk + 4 q + e on the e-th MFMA, for both operands
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
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = m0 + 4 * q + e;
                float z[CT];
#pragma unroll
                for (int c = 0; c < CT; ++c) z[c] = acc[c][e];
                visit(i, i < S, z);
            }
        }
    } else {
        const int n = tid & (d.NP - 1), r = tid >> d.lg, rs = 256 >> d.lg;
        for (int i0 = 0; i0 < S; i0 += rs) {             // every lane runs every pass: the exchanges need the whole wave
            const bool act = i0 + r < S;
            const int i = act ? i0 + r : S - 1;
            float z[CT] = {0.f};
            if constexpr (PROD) {
                const float* kr = Km + i * ldk;
                const float* ac = Zc + n;
                float s = 0.f;
#pragma unroll 16
                for (int j = 0; j < S; ++j) s = fmaf(kr[j], ac[j * lda], s);   // (one chain in index order)
                z[0] = s;
            }
            visit(i, act, z);
        }
    }
}

// The projection of one row on {a <= u, sum a = 0}, u_n = C at n = li and 0 elsewhere.  The row is W adjacent lanes x CT registers,
// element c of lane l being column l + W c; columns >= N do not exist.  Ordered by (b_k, k) with b_k = v_k - u_k, the candidate of
// an entry frees every entry up to itself: tau = (sum_free v + sum_bound u) / #free, from W CT lane exchanges.  It is consistent on
// its lower side when tau > b_k, which holds up to the root's rank and fails past it; the candidate kept is the one of the largest such
// rank (rank 1 always counts) -- in exact arithmetic the one consistent candidate.  a = min(v - tau, u), bd = v - tau >= u.  li < 0
// (a row left out): a = 0, every entry bound.  No index and no trip count depends on a float.
template <int CT>
__device__ __forceinline__ void svm_proj(const float (&v)[CT], int W, int l, int N, int li, float C, float (&a)[CT], bool (&bd)[CT]) {
    float bk[CT], s[CT];
    int cnt[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int n = l + W * c;
        bk[c] = n < N ? v[c] - (n == li ? C : 0.f) : INFINITY; s[c] = 0.f; cnt[c] = 0;
    }
#pragma unroll 2
    for (int o = 0; o < W; ++o) {
        const int lj = l ^ o;
#pragma unroll
        for (int c2 = 0; c2 < CT; ++c2) {
            const float vj = __shfl_xor(v[c2], o, 64);
            const int j = lj + W * c2;
            const bool in = j < N;
            const float uj = j == li ? C : 0.f, bj = vj - uj;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const bool fr = in && (bj < bk[c] || (bj == bk[c] && j <= l + W * c));
                cnt[c] += fr ? 1 : 0;
                s[c] += in ? (fr ? vj : uj) : 0.f;
            }
        }
    }
    float tau[CT];
    int key = 0;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        tau[c] = s[c] / (float)cnt[c];
        const bool ok = l + W * c < N && (tau[c] > bk[c] || cnt[c] == 1);
        key = max(key, ok ? cnt[c] : 0);
    }
    for (int o = W >> 1; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o, 64));
    float ts = -INFINITY;                        // (the ranks of a row are a permutation: one entry has rank `key`)
#pragma unroll
    for (int c = 0; c < CT; ++c) if (l + W * c < N && cnt[c] == key) ts = tau[c];
    for (int o = W >> 1; o > 0; o >>= 1) ts = fmaxf(ts, __shfl_xor(ts, o, 64));
    if (key == 0) ts = NAN;                      // (a row of NaNs)
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int n = l + W * c;
        const float u = n == li ? C : 0.f, dl = v[c] - ts;
        bd[c] = li < 0 || dl >= u;
        a[c] = (li < 0 || n >= N) ? 0.f : (dl >= u ? u : dl);
    }
}

// the sum of one float per thread over the workgroup, the same bits in every thread: a fixed butterfly per wave, the four waves in
// index order through red[4 slot ..]; one barrier.  A slot is free again two barriers later.
__device__ __forceinline__ float svm_block_sum(float s, float* red, int slot) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[4 * slot + (threadIdx.x >> 6)] = s;
    __syncthreads();
    const float* r = red + 4 * slot;
    return ((r[0] + r[1]) + r[2]) + r[3];
}

template <bool MF, int CT>
__global__ __launch_bounds__(256) void svm_fit_kernel(Svm d, const float* __restrict__ xs, const int64_t* __restrict__ ys,
                                                      float* __restrict__ Aw, int* __restrict__ maskw, float* __restrict__ Kw,
                                                      float* Ascr, float* __restrict__ stats, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, N = d.N, F = d.F, Sp = d.Sp, ldk = d.ldk, lda = d.lda, SA = d.SA;
    const int b = blockIdx.x;
    const int W = MF ? 16 : d.NP, l = MF ? (tid & 15) : (tid & (d.NP - 1));
    float* Km = sm;                              // [Sp, ldk], zero past S
    float* body = Km + Sp * ldk;                 // wg_mm's staging area, then Zt twice and (nlds) alpha, each [Sp, lda], zero past S, N
    float* Z0 = body;
    float* Z1 = body + SA;
    float* Al = d.nlds ? body + 2 * SA : Ascr + (long)b * SA;
    int* lab = (int*)(body + d.body);            // [S] labels, -1 where out of range
    float* red = (float*)(lab + S);              // [256]
    if (fh_stage_labels(ys + (long)b * S, S, N, lab)) atomicOr(status, FUMI_ST_LABEL_RANGE);
    __syncthreads();
    if (tid < N && fh_class_count(lab, S, tid) == 0) atomicOr(status, FUMI_ST_CLASS_MISSING);
    const float* X = xs + (long)b * S * F;
    wg_mm(body, FH_MM, S, S, F, X, F, 1, X, 1, F, [&](int m, int n, float acc) { Km[m * ldk + n] = acc; });
    __syncthreads();
    for (int t = tid; t < Sp * ldk; t += 256) {
        const int i = t / ldk, j = t - i * ldk;
        float v = 0.f;
        if (i < S && j < S) { if (lab[i] >= 0 && lab[j] >= 0) v = Km[t]; if (i == j) v += d.eps; }
        Km[t] = v;
    }
    for (int t = tid; t < (d.nlds ? 3 : 2) * SA; t += 256) body[t] = 0.f;
    __syncthreads();
    if (tid < S) {
        float s = 0.f;
        for (int j = 0; j < S; ++j) s += fabsf(Km[tid * ldk + j]);
        red[tid] = s;
    }
    __syncthreads();
    float L = 0.f;
    for (int i = 0; i < S; ++i) L = fmaxf(L, red[i]);
    const float invL = 1.f / L, C = d.C;
    __syncthreads();

    float tk = 1.f;
    for (int t = 0; t < d.T; ++t) {
        const float tn = (1.f + sqrtf(1.f + 4.f * tk * tk)) * 0.5f, mom = (tk - 1.f) / tn;
        tk = tn;
        const float* Zc = (t & 1) ? Z1 : Z0;
        float* Zn = (t & 1) ? Z0 : Z1;
        const bool last = t == d.T - 1;
        svm_rows<MF, CT, true>(d, Km, Zc, [&](int i, bool act, const float (&z)[CT]) {
            const int li = act ? lab[i] : -1;
            float v[CT], ao[CT], a[CT];
            bool bd[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const int n = l + W * c, k = i * lda + n;
                ao[c] = (t > 0 && act && n < N) ? Al[k] : 0.f;
                v[c] = Zc[k] - (z[c] - (n == li ? 1.f : 0.f)) * invL;
            }
            svm_proj<CT>(v, W, l, N, li, C, a, bd);
            if (act) {
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const int n = l + W * c, k = i * lda + n;
                    if (n < N) {
                        Al[k] = a[c];
                        Zn[k] = (last && !d.nlds) ? a[c] : a[c] + mom * (a[c] - ao[c]);   // (alpha itself for the KKT product)
                        if (last) { const long o = ((long)b * S + i) * N + n; Aw[o] = a[c]; maskw[o] = bd[c] ? 1 : 0; }
                    }
                }
            }
        });
        __syncthreads();
    }
    // the KKT residual: alpha against one unit projected-gradient step from it
    const float* Af = d.nlds ? Al : (((d.T - 1) & 1) ? Z0 : Z1);
    float res = 0.f;
    svm_rows<MF, CT, true>(d, Km, Af, [&](int i, bool act, const float (&z)[CT]) {
        const int li = act ? lab[i] : -1;
        float v[CT], al[CT], a[CT];
        bool bd[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int n = l + W * c;
            al[c] = Af[i * lda + n];
            v[c] = al[c] - (z[c] - (n == li ? 1.f : 0.f));
        }
        svm_proj<CT>(v, W, l, N, li, C, a, bd);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const float x = fabsf(al[c] - a[c]);
            if (act && l + W * c < N && (x > res || x != x)) res = x;                     // (a NaN stays)
        }
    });
    for (int o = 32; o > 0; o >>= 1) { const float x = __shfl_xor(res, o, 64); if (x > res || x != x) res = x; }
    if ((tid & 63) == 0) red[tid >> 6] = res;
    __syncthreads();
    if (tid == 0 && stats) {
        for (int w = 1; w < 4; ++w) { const float x = red[w]; if (x > res || x != x) res = x; }
        stats[2 * b] = res; stats[2 * b + 1] = 0.f;
    }
    if (d.train)
        for (int t = tid; t < Sp * ldk; t += 256) Kw[(long)b * Sp * ldk + t] = Km[t];
}

__global__ __launch_bounds__(256) void svm_w_kernel(Svm d, const float* __restrict__ xs, const float* __restrict__ Aw,
                                                    float* __restrict__ Wt) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int S = d.S, N = d.N, F = d.F;
    const int b = blockIdx.x / d.nfb, f0 = (blockIdx.x - b * d.nfb) * FH_NB, nf = min(FH_NB, F - f0);
    // W^T[m, f0 + n] = sum_k alpha[k, m] X[k, f0 + n]
    wg_mm(sm, FH_MM, N, nf, S, Aw + (long)b * S * N, 1, N, xs + (long)b * S * F + f0, F, 1,
          [&](int m, int n, float acc) { Wt[((long)b * N + m) * F + f0 + n] = acc; });
}

__global__ __launch_bounds__(256) void svm_rows_kernel(Svm d, const float* __restrict__ fq, const int64_t* __restrict__ yq,
                                                       const float* __restrict__ Wt, const float* __restrict__ scalep,
                                                       int64_t* __restrict__ preds, float* __restrict__ logits,
                                                       float* __restrict__ part, float* __restrict__ dzw, float* __restrict__ dfq,
                                                       int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int Qn = d.Qn, N = d.N, F = d.F, ldz = d.ldz;
    const int b = blockIdx.x / d.tpe, q0 = (blockIdx.x - b * d.tpe) * FH_TM, rows = min(FH_TM, Qn - q0);
    const long r0 = (long)b * Qn + q0;           // the tile's first row among all B * Qn
    float* Z = sm;                               // [16, ldz] u, then scale dz
    float* rl = Z + FH_TM * ldz;                 // [16] row losses, [16] row hits, [16] row dscale
    float* mm = rl + 48;
    const float* ft = fq + r0 * F;
    const float* wt = Wt + (long)b * N * F;
    const float scale = scalep[0];
    const int row = tid >> 4, l = tid & 15;      // 16 lanes per row

    wg_mm(mm, FH_MM, rows, N, F, ft, F, 1, wt, 1, F, [&](int m, int n, float acc) { Z[m * ldz + n] = acc; });
    __syncthreads();

    {
        float loss = 0.f, hit = 0.f, da = 0.f;
        if (row < rows) {
            float* c = Z + row * ldz;
            float us[4], z[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; us[j] = n < N ? c[n] : 0.f; z[j] = scale * us[j]; }
            // The row's softmax cross-entropy, the same block in the rows kernels of every head (see ridgehead.hip): a change to the
            // arg-max, the label rule or the NLL is made in all of them.
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
            loss = ok ? mx + logf(s) - scale * c[yv] : 0.f;
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
                        c[n] = scale * g;
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
    // dfeats_tile [rows, F] = (scale dz) [rows, N] W^T [N, F]
    for (int f0 = 0; f0 < F; f0 += FH_NB) {
        const int nb = min(FH_NB, F - f0);
        wg_mm(mm, FH_MM, rows, nb, N, Z, ldz, 1, wt + f0, F, 1,
              [&](int m, int n, float acc) { dfq[(r0 + m) * F + f0 + n] = acc; });
    }
}

__global__ __launch_bounds__(256) void svm_dw_kernel(Svm d, const float* __restrict__ xs, const float* __restrict__ fq,
                                                     const float* __restrict__ dzw, const float* __restrict__ scalep,
                                                     float* __restrict__ dWt, float* __restrict__ Pg) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int S = d.S, Qn = d.Qn, N = d.N, F = d.F;
    const int b = blockIdx.x / d.nfb, fb = blockIdx.x - b * d.nfb, f0 = fb * FH_NB, nf = min(FH_NB, F - f0);
    float* dWl = sm + FH_MM;                     // [N, FH_LDC] this block of dW^T
    const float scale = scalep[0];
    // dW^T[m, f0 + n] = scale sum_q dz[q, m] Fq[q, f0 + n]
    wg_mm(sm, FH_MM, N, nf, Qn, dzw + (long)b * Qn * N, 1, N, fq + (long)b * Qn * F + f0, F, 1, [&](int m, int n, float acc) {
        const float v = scale * acc;
        dWl[m * FH_LDC + n] = v;
        dWt[((long)b * N + m) * F + f0 + n] = v;
    });
    __syncthreads();
    // this block's share of g[m, n] = (X dW)[m, n] = sum_k X[m, f0 + k] dW^T[n, f0 + k]
    float* p = Pg + ((long)b * d.nfb + fb) * S * N;
    wg_mm(sm, FH_MM, S, N, nf, xs + (long)b * S * F + f0, F, 1, dWl, 1, FH_LDC, [&](int m, int n, float acc) { p[m * N + n] = acc; });
}

// LDS: K' [Sp, ldk] | d [Sp, lda] | the first nlds of q, r, p, each [Sp, lda] | bound bits of the rows [S] (64 bits each) | sums [12]
template <bool MF, int CT>
__global__ __launch_bounds__(256) void svm_cg_kernel(Svm d, const float* __restrict__ Kw, const int* __restrict__ maskw,
                                                     const float* __restrict__ Pg, float* Sscr, float* __restrict__ Pw,
                                                     float* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, N = d.N, Sp = d.Sp, ldk = d.ldk, lda = d.lda, SA = d.SA;
    const int b = blockIdx.x;
    const int W = MF ? 16 : d.NP, l = MF ? (tid & 15) : (tid & (d.NP - 1));
    float* Km = sm;
    float* D = Km + Sp * ldk;
    float* img[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) img[k] = k < d.nlds ? D + (1 + k) * SA : Sscr + ((long)b * 3 + k) * SA;
    float* Q = img[0];
    float* R = img[1];
    float* P = img[2];
    unsigned long long* rowm = (unsigned long long*)(D + (1 + d.nlds) * SA);
    float* red = (float*)(rowm + S);
    for (int t = tid; t < Sp * ldk; t += 256) Km[t] = Kw[(long)b * Sp * ldk + t];
    for (int t = tid; t < SA; t += 256) D[t] = 0.f;
    if (tid < S) {
        unsigned long long m = 0;
        for (int n = 0; n < N; ++n) if (maskw[((long)b * S + tid) * N + n]) m |= 1ull << n;
        rowm[tid] = m;
    }
    __syncthreads();
    // x [CT] of row i -> P x: bound entries zero, the free ones less their mean; fr: the free entries
    auto proj = [&](int i, bool act, float (&x)[CT], bool (&fr)[CT]) {
        const unsigned long long fm = act ? ~rowm[i] : 0ull;
        float s = 0.f;
        int nf = 0;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int n = l + W * c;
            fr[c] = n < N && ((fm >> n) & 1ull);
            s += fr[c] ? x[c] : 0.f; nf += fr[c] ? 1 : 0;
        }
        for (int o = W >> 1; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); nf += __shfl_xor(nf, o, 64); }
        const float mean = s / (float)max(nf, 1);
#pragma unroll
        for (int c = 0; c < CT; ++c) x[c] = (fr[c] && nf >= 2) ? x[c] - mean : 0.f;
    };
    float part = 0.f;
    svm_rows<MF, CT, false>(d, Km, D, [&](int i, bool act, const float (&)[CT]) {       // r = d = P g, p = 0
        float g[CT];
        bool fr[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int n = l + W * c;
            float s = 0.f;
            if (act && n < N)
                for (int k = 0; k < d.nfb; ++k) s += Pg[(((long)b * d.nfb + k) * S + i) * N + n];
            g[c] = s;
        }
        proj(i, act, g, fr);
        if (act) {
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const int n = l + W * c, k = i * lda + n;
                if (n < N) { R[k] = g[c]; D[k] = g[c]; P[k] = 0.f; part += g[c] * g[c]; }
            }
        }
    });
    const float rr0 = svm_block_sum(part, red, 2);
    float rr = rr0;
    for (int it = 0; it < d.Tb; ++it) {
        if (!(rr > SVM_CG_FLOOR * rr0)) break;   // (the same value in every thread)
        part = 0.f;
        svm_rows<MF, CT, true>(d, Km, D, [&](int i, bool act, const float (&z)[CT]) {   // q = P K' d
            float q[CT];
            bool fr[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) q[c] = z[c];
            proj(i, act, q, fr);
            if (act) {
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const int n = l + W * c, k = i * lda + n;
                    if (n < N) { Q[k] = q[c]; part += D[k] * q[c]; }
                }
            }
        });
        const float a = rr / svm_block_sum(part, red, 0);
        part = 0.f;
        svm_rows<MF, CT, false>(d, Km, D, [&](int i, bool act, const float (&)[CT]) {
            if (act) {
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const int n = l + W * c, k = i * lda + n;
                    if (n < N) { P[k] += a * D[k]; const float r = R[k] - a * Q[k]; R[k] = r; part += r * r; }
                }
            }
        });
        const float rn = svm_block_sum(part, red, 1), beta = rn / rr;
        svm_rows<MF, CT, false>(d, Km, D, [&](int i, bool act, const float (&)[CT]) {
            if (act) {
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const int n = l + W * c, k = i * lda + n;
                    if (n < N) D[k] = R[k] + beta * D[k];
                }
            }
        });
        rr = rn;
        __syncthreads();
    }
    svm_rows<MF, CT, false>(d, Km, D, [&](int i, bool act, const float (&)[CT]) {
        if (act) {
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const int n = l + W * c;
                if (n < N) Pw[((long)b * S + i) * N + n] = P[i * lda + n];
            }
        }
    });
    if (tid == 0 && stats) stats[2 * b + 1] = rr0 > 0.f ? sqrtf(rr / rr0) : 0.f;
}

__global__ __launch_bounds__(256) void svm_dx_kernel(Svm d, const float* __restrict__ xs, const float* __restrict__ Aw,
                                                     const float* __restrict__ Pw, const float* __restrict__ Wt,
                                                     const float* __restrict__ dWt, const float* __restrict__ part,
                                                     float* __restrict__ loss, float* __restrict__ correct,
                                                     float* __restrict__ dscale, float* dfs) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int S = d.S, N = d.N, F = d.F;
    if (blockIdx.x == gridDim.x - 1) {           // the sums over the row tiles
        fh_sum_parts<3>(part, d.ntile, sm, [&](const float (&t)[3]) {
            loss[0] = t[0] / (float)((long)d.B * d.Qn); correct[0] = t[1];
            if (dscale) dscale[0] = t[2];
        });
        return;
    }
    const int b = blockIdx.x / d.nfb, f0 = (blockIdx.x - b * d.nfb) * FH_NB, nf = min(FH_NB, F - f0);
    float* Dl = sm + FH_MM;                      // [N, FH_LDC] dW^T - p^T X of this feature block
    const float* X = xs + (long)b * S * F + f0;
    const float* A = Aw + (long)b * S * N;
    const float* G = Pw + (long)b * S * N;
    float* o = dfs + (long)b * S * F + f0;
    wg_mm2(sm, FH_MM, N, nf, S, G, 1, N, X, F, 1,
           [&](int m, int n) { return dWt[((long)b * N + m) * F + f0 + n]; },
           [&](int m, int n, float acc, float w) { Dl[m * FH_LDC + n] = w - acc; });
    __syncthreads();
    // dX = alpha D - p W^T: the second product first, the first one added to what it left
    wg_mm(sm, FH_MM, S, nf, N, G, N, 1, Wt + (long)b * N * F + f0, F, 1, [&](int m, int n, float acc) { o[(long)m * F + n] = -acc; });
    __syncthreads();
    wg_mm2(sm, FH_MM, S, nf, N, A, N, 1, Dl, FH_LDC, 1,
           [&](int m, int n) { return o[(long)m * F + n]; },
           [&](int m, int n, float acc, float x) { o[(long)m * F + n] = x + acc; });
}

int g_svm_form = -1;              // -1: chosen per shape, 0: VALU loop, 1: f32 MFMA

template <class... A>
int svm_launch_fit(bool mfma, int NP, size_t lds, hipStream_t st, int B, A... a) {
#define SVM_FIT(MF, CT) do { FUMI_SET_DYN_LDS((svm_fit_kernel<MF, CT>), lds); \
        hipLaunchKernelGGL((svm_fit_kernel<MF, CT>), dim3(B), dim3(256), lds, st, a...); } while (0)
    if (!mfma) SVM_FIT(false, 1); else if (NP <= 16) SVM_FIT(true, 1); else if (NP == 32) SVM_FIT(true, 2); else SVM_FIT(true, 4);
#undef SVM_FIT
    return FUMI_OK;
}
template <class... A>
int svm_launch_cg(bool mfma, int NP, size_t lds, hipStream_t st, int B, A... a) {
#define SVM_CG(MF, CT) do { FUMI_SET_DYN_LDS((svm_cg_kernel<MF, CT>), lds); \
        hipLaunchKernelGGL((svm_cg_kernel<MF, CT>), dim3(B), dim3(256), lds, st, a...); } while (0)
    if (!mfma) SVM_CG(false, 1); else if (NP <= 16) SVM_CG(true, 1); else if (NP == 32) SVM_CG(true, 2); else SVM_CG(true, 4);
#undef SVM_CG
    return FUMI_OK;
}

}  // namespace

extern "C" int fumi_hip_svm_set_form(int form) {
    if (form < -1 || form > 1) return FUMI_EINVAL;
    g_svm_form = form;
    return FUMI_OK;
}

extern "C" int fumi_hip_svm_head_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* scale, float C, float eps,
        int steps, int bwd_steps, float grad_scale, float* loss, float* correct, int64_t* preds, float* logits, float* dfeats_s,
        float* dfeats_q, float* dscale, float* stats) {
    // (not head_args_check: this head takes any F % 4 == 0 -- wg_mm stages feature blocks of any length -- and refuses with one code)
    if (!ws || B < 1 || S < 1 || S > 128 || Qn < 1 || (long)B * Qn > 65536 || N < 2 || N > 64 || F < 4 || F > 2048 || F % 4 != 0
        || steps < 1 || steps > 10000 || bwd_steps < 1 || bwd_steps > 1000 || !(C > 0.f) || !(eps > 0.f))
        return FUMI_EINVAL;
    for (const void* p : {(const void*)feats_s, (const void*)y_s, (const void*)feats_q, (const void*)y_q, (const void*)scale,
                          (const void*)loss, (const void*)correct}) if (!p) return FUMI_EINVAL;
    const int train = head_grad_form(dfeats_s, dfeats_q, dscale);
    if (train < 0) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    Svm d;
    head_rows_fill(d, B, S, Qn, N, F);
    d.lg = 1; while ((1 << d.lg) < N) ++d.lg;
    d.NP = 1 << d.lg; d.nfb = (F + FH_NB - 1) / FH_NB; d.train = train; d.T = steps; d.Tb = bwd_steps;
    d.Sp = (S + 15) & ~15; d.ldk = d.Sp + 4; d.lda = (d.NP < 16 ? 16 : d.NP) + 4; d.SA = d.Sp * d.lda;
    d.C = C; d.eps = eps; d.gs = head_grad_scale(grad_scale, B, Qn);
    const bool mfma = g_svm_form == 1 || (g_svm_form < 0 && SVM_AUTO_MFMA(S, d.NP));
    const size_t km = (size_t)d.Sp * d.ldk, SA = (size_t)d.SA;
    // launch 1: K' | max(staging, Zt twice [, alpha]) | labels [S], sums [256]
    auto body = [&](size_t nbuf) { return nbuf * SA > (size_t)FH_MM ? nbuf * SA : (size_t)FH_MM; };
    const int fit_lds = (km + body(3) + S + 256) * 4 <= SVM_LDS_MAX ? 1 : 0;
    const size_t fit_body = body(fit_lds ? 3 : 2), lds1 = (km + fit_body + S + 256) * 4;
    // launch 5: K' | d | up to three of q, r, p | bound bits [S] x 8 bytes, sums [12]
    const size_t cg_base = (km + SA + 2 * (size_t)S + 12) * 4;
    int cg_lds = 0;
    while (cg_lds < 3 && cg_base + (size_t)(cg_lds + 1) * SA * 4 <= SVM_LDS_MAX) ++cg_lds;
    const size_t lds5 = cg_base + (size_t)cg_lds * SA * 4;
    if (lds1 > SVM_LDS_MAX || lds5 > SVM_LDS_MAX) return FUMI_EINVAL;   // (not reached within the limits above)
    const size_t n_A = (size_t)B * S * N, n_W = (size_t)B * N * F, n_part = (size_t)3 * d.ntile, n_dz = (size_t)B * Qn * N,
                 n_P = (size_t)B * d.nfb * S * N, n_K = (size_t)B * km, n_as = fit_lds ? 0 : (size_t)B * SA;
    int rc = ws_reserve(ws, 2 * ws_align(n_A * 4) + ws_align(n_W * 4) + ws_align(n_part * 4) + ws_align(n_as * 4)
                            + (train ? ws_align(n_K * 4) + ws_align(n_dz * 4) + ws_align(n_W * 4) + ws_align(n_P * 4)
                                       + ws_align(n_A * 4) + ws_align(B * 3 * SA * 4) : 0));
    if (rc) return rc;
    float* Aw = ws_f(ws, n_A); int* maskw = (int*)ws_f(ws, n_A);          // (first, in this order: fumi_hip_svm_get_fit reads them)
    float* Wt = ws_f(ws, n_W); float* part = ws_f(ws, n_part);
    float* Ascr = n_as ? ws_f(ws, n_as) : nullptr;
    float* Kw = train ? ws_f(ws, n_K) : nullptr; float* dzw = train ? ws_f(ws, n_dz) : nullptr;
    float* dWt = train ? ws_f(ws, n_W) : nullptr; float* Pg = train ? ws_f(ws, n_P) : nullptr;
    float* Pw = train ? ws_f(ws, n_A) : nullptr; float* Sscr = train ? ws_f(ws, (size_t)B * 3 * SA) : nullptr;
    const size_t lds2 = (size_t)FH_MM * 4;
    const size_t lds3 = ((size_t)FH_TM * d.ldz + 48 + FH_MM) * 4;
    const size_t lds4 = ((size_t)FH_MM + 64 * FH_LDC) * 4;
    const size_t lds6 = train ? lds4 : (size_t)768 * 4;   // the forward form's one workgroup only adds the tile sums
    d.body = (int)fit_body; d.nlds = fit_lds;
    if (int e = svm_launch_fit(mfma, d.NP, lds1, st, B, d, feats_s, y_s, Aw, maskw, Kw, Ascr, stats, ws->status)) return e;
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(svm_w_kernel, lds2);
    hipLaunchKernelGGL(svm_w_kernel, dim3(B * d.nfb), dim3(256), lds2, st, d, feats_s, Aw, Wt);
    LAUNCH_CHECK();
    FUMI_SET_DYN_LDS(svm_rows_kernel, lds3);
    hipLaunchKernelGGL(svm_rows_kernel, dim3(d.ntile), dim3(256), lds3, st, d, feats_q, y_q, Wt, scale, preds, logits, part, dzw,
                       dfeats_q, ws->status);
    LAUNCH_CHECK();
    if (train) {
        FUMI_SET_DYN_LDS(svm_dw_kernel, lds4);
        hipLaunchKernelGGL(svm_dw_kernel, dim3(B * d.nfb), dim3(256), lds4, st, d, feats_s, feats_q, dzw, scale, dWt, Pg);
        LAUNCH_CHECK();
        d.nlds = cg_lds;
        if (int e = svm_launch_cg(mfma, d.NP, lds5, st, B, d, Kw, maskw, Pg, Sscr, Pw, stats)) return e;
        LAUNCH_CHECK();
    }
    FUMI_SET_DYN_LDS(svm_dx_kernel, lds6);
    hipLaunchKernelGGL(svm_dx_kernel, dim3((train ? B * d.nfb : 0) + 1), dim3(256), lds6, st, d, feats_s, Aw, Pw, Wt, dWt, part, loss,
                       correct, dscale, dfeats_s);
    LAUNCH_CHECK();
    return FUMI_OK;
}

extern "C" int fumi_hip_svm_get_fit(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int N, float* alpha, int32_t* mask) {
    if (!ws || !alpha || !mask || B < 1 || S < 1 || N < 1) return FUMI_EINVAL;
    const size_t n_A = (size_t)B * S * N;
    if (!ws->base || 2 * ws_align(n_A * 4) > ws->cap) return FUMI_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    HIP_TRY(hipMemcpyAsync(alpha, ws->base, n_A * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(mask, ws->base + ws_align(n_A * 4), n_A * 4, hipMemcpyDeviceToDevice, st));
    return FUMI_OK;
}
