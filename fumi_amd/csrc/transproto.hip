// Transductive prototype refinement (soft k-means of Ren et al. 2018; --transductive_steps).  Forward only.
// Per episode, with s_n the sum and k_n the count of the support rows of class n and c^0_n = s_n / max(k_n, 1):
//     w = softmax_n(z(c^t)) over the query rows,   c^{t+1}_n = (s_n + sum_q w[q,n] f_q) / (k_n + sum_q w[q,n]),   t = 0 .. steps-1,
// z(c)[q,n] = scale cos(f_q, c_n) (metric 0, the cosine head's clamp 1e-12 on both norms) or -scale |f_q - c_n|^2 (metric 1); loss,
// predictions and logits come from z(c^steps).  steps = 0 is the forward form of the cosine / the prototypical head.
//
// The iteration runs in the dual.  Every prototype is a combination of the episode's M = S + Qn rows: with U_n = mass_n c_n,
//     U^t_n = s_n + sum_q w[q,n] f_q,   mass_n = k_n + sum_q w[q,n],
// so that with the two products over F, made once per call on the f32 MFMA,
//     P0 = X_all S^T [M, N]  (all rows against the class sums)   and   KQ = X_all X_q^T [M, Qn],
// a step needs only G = P0 + KQ w [M, N]:   <f_q, c_n> = G[q,n] / mass_n,   |c_n|^2 = (sum_s Y[s,n] G[s,n] + sum_q w[q,n] G[q,n]) / mass_n^2,
// and |f_q|^2 = KQ[q,q] is fixed.  Of the support rows of G only the column of the row's own class is used.
// Metric 1 takes every row relative to m, the mean of the step-0 prototypes (section 35's argument: d2 does not change, and every
// quantity above is then of the size of d2, so a common offset of the features costs no digits).  A weighted mean moves with its
// points, so the refinement is the same in the shifted frame.  Metric 0 is not shift-invariant and uses the raw rows (m = 0).
// A class without a support row starts from the zero prototype, which is -m in the shifted frame: its column of P0 is X' (-m) and its
// |c|^2 is |m|^2 at step 0; from step 1 on it has s_n = 0, k_n = 0 and is refined like any class.
//
//   launch 1, one workgroup per (episode, block of 256 features): class sums in LDS, one column per thread, support rows added in index
//       order; c^0, m, and the class vectors U^0_n = k_n (c^0_n - m) (the raw sums for metric 0; -m for a missing class) go to memory
//       with the block's share of |m|^2.
//   launch 2, one workgroup per (episode, 64 rows, 64 columns): P0 and KQ tiles.  The rows are staged through LDS 32 features at a
//       time, m subtracted on the way (the next chunk's loads are in flight during the MFMAs); each of the four waves holds 16 rows x 64
//       columns in four accumulators.  Rows and columns are laid out padded (support rows to Sp, query rows to Qp, multiples of 16) and
//       the padding is written as zeros, so the loop reads whole tiles with no bounds check.
//   launch 3, one workgroup per episode: the step loop.  w [Qp, ldw] and the query rows of G are held in LDS; KQ is streamed from the
//       workspace as the A operand of G = P0 + KQ w (v_mfma_f32_16x16x4_f32, a wave owns the row tiles wave, wave + 4, ...).
//       BARRIERS: TWO per step, which is what the data flow allows: |c_n|^2 needs a sum over ALL rows of G, which needs all of w;
//       the next w needs |c_n|^2.  Phase a (G tiles, per-wave column sums of a G) | barrier | phase b (mass, |c|^2, z, softmax, the
//       wave's column sums of the new w) | barrier.  After the last step phase b writes logits, predictions and the row losses, and
//       the episode's loss / correct sums go to part[b] in a fixed order.
//   launch 4, one workgroup: the episode partials added in index order into loss and correct.
// Fixed summation orders, the first arg-max, the label-range and missing-class rules and the absence of floating-point atomics are
// those of fewshot_head.h.  A query row whose label is out of range still takes part in the refinement, which reads no query label.
// scale is read from device memory by the kernel.
#include "fewshot_head.h"

namespace {

constexpr int TP_T = 64;           // rows and columns of a tile of launch 2
constexpr int TP_KC = 32;          // features per staged chunk of launch 2
constexpr int TP_LDI = TP_KC + 4;  // row stride of its LDS images (= 4 mod 32: conflict-free ds_read_b128)
constexpr size_t TP_LDS_MAX = 160 * 1024;

struct TransProto {
    int B, S, Qn, N, F, Sp, Qp, MP, CT, ldw, steps, metric, nfb1, rtm, ctq, vec;   // CT: column tiles of 16 (ldp = 16 CT); vec: 16-byte rows
};

__global__ __launch_bounds__(256) void trans_proto_means_kernel(TransProto d, const float* __restrict__ xs,
                                                                const int64_t* __restrict__ ys, float* __restrict__ U,
                                                                float* __restrict__ mvec, float* __restrict__ msqp, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, N = d.N, F = d.F;
    const int b = blockIdx.x / d.nfb1, fb = blockIdx.x - b * d.nfb1;
    float* acc = sm;                             // [N, 256] class sums
    float* mcol = acc + N * FH_PF;               // [256] m[f]^2 of each column
    int* lab = (int*)(mcol + FH_PF);             // [S] labels, -1 where out of range
    int* cnt = lab + S;                          // [N]
    const bool bad = fh_stage_labels(ys + (long)b * S, S, N, lab);
    if (bad && fb == 0) atomicOr(status, FUMI_ST_LABEL_RANGE);
    for (int i = tid; i < N * FH_PF; i += 256) acc[i] = 0.f;
    __syncthreads();
    if (tid < N) {                               // the raw counts: k_n = 0 is a case of its own here
        const int c = fh_class_count(lab, S, tid);
        cnt[tid] = c;
        if (c == 0 && fb == 0) atomicOr(status, FUMI_ST_CLASS_MISSING);
    }
    const int f = fb * FH_PF + tid;
    if (f < F) fh_class_sums(acc, lab, xs + (long)b * S * F + f, S, F);
    __syncthreads();
    float m = 0.f;
    if (f < F) {
        if (d.metric) {                          // the mean of the step-0 prototypes, classes in index order
            for (int n = 0; n < N; ++n) m += acc[n * FH_PF + tid] / (float)max(cnt[n], 1);
            m /= (float)N;
            for (int n = 0; n < N; ++n) {
                const float k = (float)max(cnt[n], 1);
                U[((long)b * N + n) * F + f] = (acc[n * FH_PF + tid] / k - m) * k;
            }
        } else {
            for (int n = 0; n < N; ++n) U[((long)b * N + n) * F + f] = acc[n * FH_PF + tid];
        }
        mvec[(long)b * F + f] = m;
    }
    mcol[tid] = m * m;
    __syncthreads();
    if (tid < 64) {                              // |m|^2 over this block's columns (columns past F hold 0)
        float s = ((mcol[tid] + mcol[tid + 64]) + mcol[tid + 128]) + mcol[tid + 192];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (tid == 0) msqp[(long)b * d.nfb1 + fb] = s;
    }
}

// four floats of a row, or zeros: the load is unconditional from a clamped address (a guarded load is a basic block with a full wait)
__device__ __forceinline__ f32x4 tp_load4(const float* p, bool vec) {
    if (vec) return *(const f32x4*)p;
    return (f32x4){p[0], p[1], p[2], p[3]};
}

__global__ __launch_bounds__(256) void trans_proto_gram_kernel(TransProto d, const float* __restrict__ xs, const float* __restrict__ xq,
                                                               const float* __restrict__ U, const float* __restrict__ mvec,
                                                               float* __restrict__ P0, float* __restrict__ KQ) {
    __shared__ __attribute__((aligned(16))) float Ai[TP_T * TP_LDI];
    __shared__ __attribute__((aligned(16))) float Bi[TP_T * TP_LDI];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int S = d.S, Qn = d.Qn, N = d.N, F = d.F, Sp = d.Sp, Qp = d.Qp, MP = d.MP;
    const int per = d.rtm * (1 + d.ctq);
    const int b = blockIdx.x / per, rr = blockIdx.x - b * per, rt = rr / (1 + d.ctq), ct = rr - rt * (1 + d.ctq);
    const int row0 = rt * TP_T, col0 = ct == 0 ? 0 : (ct - 1) * TP_T;
    const float* xsb = xs + (long)b * S * F;
    const float* xqb = xq + (long)b * Qn * F;
    const float* mv = mvec + (long)b * F;
    const bool centre = d.metric != 0, vec = d.vec != 0;
    // a thread stages two 16-byte pieces of each operand per chunk: rows (tid >> 3) and (tid >> 3) + 32, features 4 (tid & 7) ..
    const int c4 = (tid & 7) << 2;
    const float* pa[2]; const float* pb[2]; bool va[2], vb[2], cb;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int row = (tid >> 3) + 32 * u;
        const int ip = row0 + row;               // a padded row: support rows [0, Sp), query rows [Sp, Sp + Qp)
        if (ip < Sp) { va[u] = ip < S; pa[u] = xsb + (long)(va[u] ? ip : 0) * F; }
        else { const int qi = ip - Sp; va[u] = qi < Qn; pa[u] = xqb + (long)(va[u] ? qi : 0) * F; }
        if (ct == 0) { vb[u] = row < N; pb[u] = U + ((long)b * N + (vb[u] ? row : 0)) * F; }
        else { const int j = col0 + row; vb[u] = j < Qn; pb[u] = xqb + (long)(vb[u] ? j : 0) * F; }
    }
    cb = centre && ct != 0;                      // the class vectors are already relative to m
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 ra[2], rb[2];
    auto fetch = [&](int k0) {
        const f32x4 m4 = centre ? *(const f32x4*)(mv + k0 + c4) : z4;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f32x4 a = tp_load4(pa[u] + k0 + c4, vec), bb = tp_load4(pb[u] + k0 + c4, vec);
            ra[u] = va[u] ? a - m4 : z4;
            rb[u] = vb[u] ? (cb ? bb - m4 : bb) : z4;
        }
    };
    const int nct = ct == 0 ? d.CT : min(4, (Qp - col0) >> 4);     // column tiles of 16 that exist
    const bool rowact = row0 + 16 * wave < MP;                     // (wave-uniform; MP is a multiple of 16)
    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = z4;
    fetch(0);
    for (int k0 = 0; k0 < F; k0 += TP_KC) {
        __syncthreads();                         // the previous chunk's fragment reads are done
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int row = (tid >> 3) + 32 * u;
            *(f32x4*)(Ai + row * TP_LDI + c4) = ra[u];
            *(f32x4*)(Bi + row * TP_LDI + c4) = rb[u];
        }
        __syncthreads();
        if (k0 + TP_KC < F) fetch(k0 + TP_KC);
        if (rowact) {
#pragma unroll
            for (int kk = 0; kk < TP_KC; kk += 16) {   // lane (r, q) feeds k = kk + 4 q + e on the e-th MFMA, for both operands
                const f32x4 av = *(const f32x4*)(Ai + (16 * wave + r) * TP_LDI + kk + 4 * q);
                f32x4 bv[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) bv[c] = *(const f32x4*)(Bi + (16 * c + r) * TP_LDI + kk + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (c < nct) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[c][e], acc[c], 0, 0, 0);
            }
        }
    }
    if (!rowact) return;
    const int ldo = ct == 0 ? 16 * d.CT : Qp;
    float* out = (ct == 0 ? P0 : KQ) + (long)b * MP * ldo + col0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < nct)
#pragma unroll
            for (int e = 0; e < 4; ++e) out[(long)(row0 + 16 * wave + 4 * q + e) * ldo + 16 * c + r] = acc[c][e];
}

template <int CT>
__global__ __launch_bounds__(256) void trans_proto_loop_kernel(TransProto d, const float* __restrict__ P0, const float* __restrict__ KQ,
                                                               const float* __restrict__ msqp, const int64_t* __restrict__ ys,
                                                               const int64_t* __restrict__ yq, const float* __restrict__ scale_p,
                                                               int64_t* __restrict__ preds, float* __restrict__ logits,
                                                               float* __restrict__ part, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int S = d.S, Qn = d.Qn, N = d.N, Sp = d.Sp, Qp = d.Qp, MP = d.MP, ldw = d.ldw;
    constexpr int ldp = 16 * CT;
    const int b = blockIdx.x;
    float* W = sm;                               // [Qp, ldw] the soft assignments, zero past Qn and past N
    float* G = W + Qp * ldw;                     // [Qp, ldw] the query rows of G
    float* fq2 = G + Qp * ldw;                   // [Qp] |f_q|^2 (metric 1: relative to m)
    float* rl = fq2 + Qp;                        // [Qp] row losses, [Qp] row hits
    float* redq = rl + 2 * Qp;                   // [4][64] per-wave column sums of a G
    float* redm = redq + 256;                    // [2][4][64] per-wave column sums of w, two slots
    int* lab = (int*)(redm + 512);               // [Sp] support labels, -1 where out of range or past S
    int* kcnt = lab + Sp;                        // [64] class counts
    const float* P0b = P0 + (long)b * MP * ldp;
    const float* KQb = KQ + (long)b * MP * Qp;
    for (int i = tid; i < Sp; i += 256) {        // (not fh_stage_labels: padded to Sp, and launch 1 has reported the status)
        long t = -1;
        if (i < S) t = ys[(long)b * S + i];
        lab[i] = (t >= 0 && t < N) ? (int)t : -1;
    }
    for (int i = tid; i < Qp * ldw; i += 256) W[i] = 0.f;
    for (int i = tid; i < Qp; i += 256) {
        fq2[i] = i < Qn ? KQb[(long)(Sp + i) * Qp + i] : 0.f;
        rl[i] = 0.f; rl[Qp + i] = 0.f;
    }
    __syncthreads();
    if (tid < 64) {
        int c = 0;
        for (int i = 0; i < S; ++i) c += lab[i] == tid ? 1 : 0;
        kcnt[tid] = c;
    }
    __syncthreads();
    float kf[CT];                                // k_n of the columns r + 16 c, in every lane that holds them
#pragma unroll
    for (int c = 0; c < CT; ++c) kf[c] = (float)kcnt[r + 16 * c];
    const float scale = scale_p[0];
    float msq = 0.f;                             // |m|^2: the step-0 |c|^2 of a class without a support row
    if (d.metric) for (int k = 0; k < d.nfb1; ++k) msq += msqp[(long)b * d.nfb1 + k];
    const int ntile = MP >> 4, stile = Sp >> 4;

    for (int t = 0; t <= d.steps; ++t) {
        // ---- phase a: G = P0 + KQ w^t on this wave's row tiles; the wave's share of sum_i a[i,n] G[i,n] ----
        float cs[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) cs[c] = 0.f;
        for (int rt = wave; rt < ntile; rt += 4) {       // wave-uniform
            const int m0 = rt << 4;
            float p0[CT][4];
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) p0[c][e] = P0b[(long)(m0 + 4 * q + e) * ldp + 16 * c + r];
            f32x4 acc[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (t > 0) {
                const float* kp = KQb + (long)(m0 + r) * Qp + 4 * q;
                const float* wp = W + 4 * q * ldw + r;
                f32x4 an = *(const f32x4*)kp;
                for (int kk = 0; kk < Qp; kk += 16) {    // lane (r, q) feeds k = kk + 4 q + e on the e-th MFMA, for both operands
                    const f32x4 av = an;                 // (the next step's piece of KQ is in flight during this step's MFMAs)
                    an = *(const f32x4*)(kp + min(kk + 16, Qp - 16));
                    f32x4 bv[CT];
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        const float* p = wp + kk * ldw + 16 * c;
                        bv[c][0] = p[0]; bv[c][1] = p[ldw]; bv[c][2] = p[2 * ldw]; bv[c][3] = p[3 * ldw];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int c = 0; c < CT; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[c][e], acc[c], 0, 0, 0);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {                // register e of lane (r, q): row m0 + 4 q + e, columns r + 16 c
                const int i = m0 + 4 * q + e;
                if (rt < stile) {
                    const int li = lab[i];
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        const float g = acc[c][e] + ((t == 0 || kf[c] > 0.f) ? p0[c][e] : 0.f);
                        cs[c] += li == r + 16 * c ? g : 0.f;
                    }
                } else {
                    const int k = (i - Sp) * ldw + r;
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        const float g = acc[c][e] + ((t == 0 || kf[c] > 0.f) ? p0[c][e] : 0.f);
                        G[k + 16 * c] = g;
                        if (t > 0) cs[c] += W[k + 16 * c] * g;
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CT; ++c) {                   // the four lanes of this wave that hold column r + 16 c
            cs[c] += __shfl_xor(cs[c], 16, 64);
            cs[c] += __shfl_xor(cs[c], 32, 64);
            if (lane < 16) redq[wave * 64 + 16 * c + r] = cs[c];
        }
        __syncthreads();
        // ---- phase b: mass, |c|^2, z, and the next w or the outputs; 16 lanes per row, columns r + 16 c ----
        const float* rm = redm + ((t + 1) & 1) * 256;    // written by step t - 1
        float* rn = redm + (t & 1) * 256;
        float inv[CT], cn[CT], ws[CT];                   // 1 / mass_n; metric 0: 1 / max(|c_n|, eps), metric 1: |c_n|^2
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int n = r + 16 * c;
            float Q = ((redq[n] + redq[64 + n]) + redq[128 + n]) + redq[192 + n];
            if (t == 0 && d.metric && kf[c] == 0.f) Q += msq;
            const float mass = t == 0 ? fmaxf(kf[c], 1.f) : kf[c] + (((rm[n] + rm[64 + n]) + rm[128 + n]) + rm[192 + n]);
            inv[c] = n < N ? 1.f / mass : 0.f;
            cn[c] = d.metric ? Q * inv[c] * inv[c] : 1.f / fmaxf(sqrtf(fmaxf(Q, 0.f)) * inv[c], 1e-12f);
            ws[c] = 0.f;
        }
        const bool last = t == d.steps;
        for (int rt = stile + wave; rt < ntile; rt += 4) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int qi = ((rt - stile) << 4) + 4 * p + q;
                const bool act = qi < Qn;
                const float* g = G + qi * ldw + r;
                const float f2 = fq2[qi];
                const float fi = d.metric ? 0.f : scale / fmaxf(sqrtf(f2), 1e-12f);
                // (fh_row_softmax's block over CT columns, kept inline with the arg-max fused into the loop that forms z: through the
                // helper the compiler reorders this step loop and the head measured 0.2 - 0.4 % slower)
                float z[CT];
                float mx = -INFINITY; int arg = N;
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const int n = r + 16 * c;
                    const float dot = g[16 * c] * inv[c];
                    z[c] = d.metric ? -scale * ((f2 + cn[c]) - 2.f * dot) : fi * dot * cn[c];
                    if (n < N && z[c] > mx) { mx = z[c]; arg = n; }
                }
                for (int o = 8; o > 0; o >>= 1) {
                    const float v2 = __shfl_xor(mx, o, 64); const int a2 = __shfl_xor(arg, o, 64);
                    if (v2 > mx || (v2 == mx && a2 < arg)) { mx = v2; arg = a2; }           // first arg-max (torch.max)
                }
                if (arg >= N) arg = 0;                                                       // (a row of NaNs)
                float ex[CT], s = 0.f;
#pragma unroll
                for (int c = 0; c < CT; ++c) { ex[c] = r + 16 * c < N ? expf(z[c] - mx) : 0.f; s += ex[c]; }
                for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                if (!last) {
                    const float is = 1.f / s;
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        const float wv = act ? ex[c] * is : 0.f;
                        if (act && r + 16 * c < N) W[qi * ldw + r + 16 * c] = wv;
                        ws[c] += wv;
                    }
                } else if (act) {
                    const long row = (long)b * Qn + qi;
                    long yv = yq[row];
                    const bool ok = yv >= 0 && yv < N;
                    if (!ok) { if (r == 0) atomicOr(status, FUMI_ST_LABEL_RANGE); yv = 0; }
                    // z of the label's column: the lane that holds it hands it to the row's first lane
                    float zy = 0.f;
#pragma unroll
                    for (int c = 0; c < CT; ++c) if (r + 16 * c == (int)yv) zy = z[c];
                    for (int o = 8; o > 0; o >>= 1) zy += __shfl_xor(zy, o, 64);
                    if (r == 0) {
                        rl[qi] = ok ? mx + logf(s) - zy : 0.f;
                        rl[Qp + qi] = (ok && arg == (int)yv) ? 1.f : 0.f;
                        if (preds) preds[row] = arg;
                    }
                    if (logits) {
#pragma unroll
                        for (int c = 0; c < CT; ++c) if (r + 16 * c < N) logits[row * N + r + 16 * c] = z[c];
                    }
                }
            }
        }
        if (!last) {
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                ws[c] += __shfl_xor(ws[c], 16, 64);
                ws[c] += __shfl_xor(ws[c], 32, 64);
                if (lane < 16) rn[wave * 64 + 16 * c + r] = ws[c];
            }
        }
        __syncthreads();
    }
    {   // the episode's sums: strided partials, a butterfly per wave, the four waves in index order
        float a = 0.f, h = 0.f;
        for (int i = tid; i < Qp; i += 256) { a += rl[i]; h += rl[Qp + i]; }
        for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); h += __shfl_xor(h, o, 64); }
        if (lane == 0) { redq[wave] = a; redq[4 + wave] = h; }
        __syncthreads();
        if (tid == 0) {
            part[b] = ((redq[0] + redq[1]) + redq[2]) + redq[3];
            part[d.B + b] = ((redq[4] + redq[5]) + redq[6]) + redq[7];
        }
    }
}

__global__ __launch_bounds__(256) void trans_proto_sum_kernel(TransProto d, const float* __restrict__ part, float* __restrict__ loss,
                                                              float* __restrict__ correct) {
    __shared__ float sm[512];
    fh_sum_parts<2>(part, d.B, sm, [&](const float (&t)[2]) {          // the sums over the episodes
        loss[0] = t[0] / (float)((long)d.B * d.Qn); correct[0] = t[1];
    });
}

}  // namespace

extern "C" int fumi_hip_trans_proto_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* scale, int metric, int steps,
        float* loss, float* correct, int64_t* preds, float* logits) {
    const bool own = S + Qn <= 512 && (long)Qn * N <= 8192 && steps >= 0 && steps <= 100;
    if (int rc = head_args_check(ws, B, S, Qn, N, F, own, {feats_s, y_s, feats_q, y_q, scale, loss, correct})) return rc;
    if (metric != 0 && metric != 1) return FUMI_EINVAL;
    TransProto d;
    d.B = B; d.S = S; d.Qn = Qn; d.N = N; d.F = F; d.Sp = (S + 15) & ~15; d.Qp = (Qn + 15) & ~15; d.MP = d.Sp + d.Qp;
    d.CT = (N + 15) >> 4; d.ldw = 16 * d.CT + 4; d.steps = steps; d.metric = metric; d.nfb1 = (F + FH_PF - 1) / FH_PF;
    d.rtm = (d.MP + TP_T - 1) / TP_T; d.ctq = (d.Qp + TP_T - 1) / TP_T;
    d.vec = ((((uintptr_t)feats_s) | ((uintptr_t)feats_q)) & 15) == 0 ? 1 : 0;
    const size_t lds1 = ((size_t)N * FH_PF + FH_PF + S + N) * 4;
    const size_t lds3 = ((size_t)2 * d.Qp * d.ldw + 3 * d.Qp + 256 + 512 + d.Sp + 64) * 4;
    if (lds3 > TP_LDS_MAX) return FUMI_ENOTSUP;  // (not reached inside the limits above: at most 152256 bytes, at Qn = 481, N = 17)
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    const size_t n_U = (size_t)B * N * F, n_m = (size_t)B * F, n_msq = (size_t)B * d.nfb1, n_P0 = (size_t)B * d.MP * 16 * d.CT,
                 n_KQ = (size_t)B * d.MP * d.Qp, n_part = (size_t)2 * B;
    int rc = ws_reserve(ws, ws_align(n_U * 4) + ws_align(n_m * 4) + ws_align(n_msq * 4) + ws_align(n_P0 * 4) + ws_align(n_KQ * 4) +
                            ws_align(n_part * 4));
    if (rc) return rc;
    float* U = ws_f(ws, n_U); float* mvec = ws_f(ws, n_m); float* msqp = ws_f(ws, n_msq); float* P0 = ws_f(ws, n_P0);
    float* KQ = ws_f(ws, n_KQ); float* part = ws_f(ws, n_part);
    FUMI_SET_DYN_LDS(trans_proto_means_kernel, lds1);
    hipLaunchKernelGGL(trans_proto_means_kernel, dim3(B * d.nfb1), dim3(256), lds1, st, d, feats_s, y_s, U, mvec, msqp, ws->status);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(trans_proto_gram_kernel, dim3(B * d.rtm * (1 + d.ctq)), dim3(256), 0, st, d, feats_s, feats_q, U, mvec, P0, KQ);
    LAUNCH_CHECK();
#define TP_LOOP(CTV)                                                                                                              \
    do {                                                                                                                          \
        FUMI_SET_DYN_LDS(trans_proto_loop_kernel<CTV>, lds3);                                                                     \
        hipLaunchKernelGGL(trans_proto_loop_kernel<CTV>, dim3(B), dim3(256), lds3, st, d, P0, KQ, msqp, y_s, y_q, scale, preds,    \
                           logits, part, ws->status);                                                                             \
    } while (0)
    if (d.CT == 1) TP_LOOP(1); else if (d.CT == 2) TP_LOOP(2); else if (d.CT == 3) TP_LOOP(3); else TP_LOOP(4);
#undef TP_LOOP
    LAUNCH_CHECK();
    hipLaunchKernelGGL(trans_proto_sum_kernel, dim3(1), dim3(256), 0, st, d, part, loss, correct);
    LAUNCH_CHECK();
    return FUMI_OK;
}
