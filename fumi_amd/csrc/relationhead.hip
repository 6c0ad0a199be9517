// Relation Network head (Sung et al. 2018; --fewshot_head relation): the few-shot head whose comparison function is
// learned.  The feature-vector form of the paper's relation module, Linear(2F, H) -> ReLU -> Linear(H, 1) on the concatenation (class
// mean, query), with the first weight split into its halves w1 [2, H, F] = (W1s, W1q) so that no concatenation is ever formed.  Per
// episode, with c_n the mean of the valid support rows of class n (count clamped to >= 1):
//     U[n,:] = W1s c_n + b1  [N, H],   V[q,:] = W1q f_q  [Qn, H],   z[q,n] = w2 . relu(U[n,:] + V[q,:]) + b2,
// loss kind 1 (mse, the paper's): 1 / (B Qn N) sum over the valid rows and the N classes of (sigmoid(z) - onehot(y_q))^2,
//     dz = grad_scale 2 / (B Qn N) (s - t) s (1 - s);
// loss kind 0 (ce, Chen et al. 2019): the softmax cross-entropy of z over the N classes, mean over B Qn rows,
//     dz = grad_scale / (B Qn) (softmax - onehot).
// preds is the first arg-max of z, correct and logits = z mean what they mean in every other head.  Backward, with the mask
// m[q,n,h] = (U[n,h] + V[q,h] > 0):
//     dV[q,h] = w2[h] sum_n dz[q,n] m,   dU[n,h] = w2[h] sum_q dz[q,n] m,   dw2[h] = sum dz relu(U + V),   db2 = sum dz,
//     db1 = column sum of dU,   dW1q = dV^T F_q,   dW1s = dU^T C,   dfeats_q = dV W1q,   dc = dU W1s,
// and every valid support row of class n receives dc_n / count_n.
// THE MASK is fl32(U[n,h] + V[q,h]) > 0: ONE fp32 addition of the stored fp32 U and V (hid_s, hid_q), in every kernel that needs it.  A
// correctly rounded sum keeps the sign of the exact sum, so a float64 reference rebuilds the kernels' mask from those two outputs.
//
//   launch 1, one workgroup per (episode, 256 features): class sums in LDS, one column per thread, rows in index order; the means, the
//       class counts and the status bits.
//   launches 2, 3: U = C W1s^T + b1 and V = F_q W1q^T on the dense GEMM (gemm.hip), into hid_s / hid_q where the caller gave them.
//   launch 4, one workgroup per (episode, tile of 16 query rows), 16 lanes per row: H is walked in chunks of 128 with the episode's U
//       chunk [N, 128] and the tile's V chunk [16, 128] in LDS; lane l holds 8 hidden units of its row, a class's chunk sum is a
//       16-lane butterfly, the chunks are added in index order; then the loss block.  Training form: dz goes to memory and stays in
//       LDS, and a second walk over the chunks forms dV (classes in index order).  The tile's loss / correct / db2 sums go to part.
//   launch 5 (training), one workgroup per (group of episodes, chunk of 128 hidden units): dU and the episode's share of dw2 over ALL Qn
//       rows, 64 rows of V and dz staged at a time and summed in three fixed levels (8 rows, the block, the blocks), the mask rebuilt
//       from U and V -- no mask and no per-tile [N, H] image is ever stored; a workgroup walks its episodes in index order and leaves
//       one partial row of dw2 and db1.
//   launches 6 - 9 (training): dfeats_q, dc, dW1q, dW1s on the dense GEMM; the weight gradients' contraction over all B Qn (B N) rows is
//       split into slabs that a fixed-order reduction adds (launch_reduce_slabs) where it is long.
//   last launch: (training) one workgroup per (episode, 16 classes, 128 features) scatters dc to the support rows, one per 256 hidden
//       units adds the partial rows of dw2 and db1 in index order; one workgroup adds part[0..ntile): loss, correct, db2.
//   The forward form is launches 1 - 4 without the backward half of 4 and the last workgroup: the same instructions produce loss,
//   correct, preds, logits, hid_s and hid_q in both forms.
// Fixed summation orders, the first arg-max, the label-range and missing-class rules and the absence of floating-point atomics are
// those of fewshot_head.h.  A support row left out gets a zero gradient, a class without a support row a zero prototype (U = b1).
#include "fewshot_head.h"

namespace {

constexpr int RH_HC = 128;             // hidden units per chunk
constexpr int RH_LDH = RH_HC + 4;      // row stride of the [N, 128] and [16, 128] chunk images of the pair kernel
constexpr int RH_QB = 64;              // query rows staged at a time by the dU kernel
constexpr int RH_LDQ = RH_QB + 4;      // row stride of its transposed dz image [N, 64]
constexpr int RH_MAXG = 256;           // groups of episodes of the dU kernel: rows of the dw2 / db1 partial sums
constexpr int RH_SMAX = 1024, RH_HMAX = 1024;

struct RelDims { int H, mse; float gz, linv; };   // gz: dz's factor; linv: 1 / the loss's divisor

// rows [nr, hc] of src (row stride ld, from column h0) -> img [nrp, RH_LDH-like stride `ldi`], zero past nr and past hc
__device__ __forceinline__ void rh_stage(float* img, int ldi, int nrp, int nr, int hc, const float* src, long ld) {
    const int tid = threadIdx.x;
    if (((((uintptr_t)src) & 15) == 0) && (ld & 3) == 0) {
        for (int i = tid; i < nrp * (RH_HC / 4); i += 256) {
            const int r = i >> 5, c = (i & 31) << 2;
            const bool ok = r < nr && c < hc;
            const f32x4 t = *(const f32x4*)(src + (ok ? (long)r * ld + c : 0));
            *(f32x4*)(img + r * ldi + c) = ok ? t : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    } else {
        for (int i = tid; i < nrp * RH_HC; i += 256) {
            const int r = i >> 7, c = i & 127;
            img[r * ldi + c] = (r < nr && c < hc) ? src[(long)r * ld + c] : 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void rel_means_kernel(HeadDims d, const float* __restrict__ xs, const int64_t* __restrict__ ys,
                                                        float* __restrict__ cm, float* __restrict__ cntf, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, N = d.N, F = d.F;
    const int b = blockIdx.x / d.nfb1, fb = blockIdx.x - b * d.nfb1;
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
    if (f < F) for (int n = 0; n < N; ++n) cm[((long)b * N + n) * F + f] = acc[n * FH_PF + tid] / (float)cnt[n];
}

__global__ __launch_bounds__(256) void rel_pair_kernel(HeadDims d, RelDims rd, const float* __restrict__ U, const float* __restrict__ V,
                                                       const float* __restrict__ w2, const float* __restrict__ b2,
                                                       const int64_t* __restrict__ yq, int64_t* __restrict__ preds,
                                                       float* __restrict__ logits, float* __restrict__ part, float* __restrict__ dzg,
                                                       float* __restrict__ dV, int* status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int Qn = d.Qn, N = d.N, H = rd.H, ldz = d.ldz;
    const int b = blockIdx.x / d.tpe, q0 = (blockIdx.x - b * d.tpe) * FH_TM, rows = min(FH_TM, Qn - q0);
    const long r0 = (long)b * Qn + q0;           // the tile's first row among all B * Qn
    float* Uc = sm;                              // [N, RH_LDH] the episode's U chunk
    float* Vc = Uc + N * RH_LDH;                 // [16, RH_LDH] the tile's V chunk
    float* wc = Vc + FH_TM * RH_LDH;             // [128] w2 chunk
    float* DZ = wc + RH_HC;                      // [16, ldz] dz
    float* rl = DZ + FH_TM * ldz;                // [16] row losses, [16] row hits, [16] row sums of dz
    const int row = tid >> 4, l = tid & 15;      // 16 lanes per row
    const bool live = row < rows;
    const float* Ub = U + (long)b * N * H;
    const float* Vt = V + r0 * H;

    auto stage = [&](int h0, int hc) {
        __syncthreads();
        rh_stage(Uc, RH_LDH, N, N, hc, Ub + h0, H);
        rh_stage(Vc, RH_LDH, FH_TM, rows, hc, Vt + h0, H);
        if (tid < RH_HC) wc[tid] = tid < hc ? w2[h0 + tid] : 0.f;
        __syncthreads();
    };

    // z[q, n] = sum_h w2[h] relu(U[n,h] + V[q,h]): lane l owns the hidden units 4l .. 4l+3 and 64+4l .. 64+4l+3 of the chunk, the
    // classes l, l + 16, l + 32, l + 48 of its row
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int h0 = 0; h0 < H; h0 += RH_HC) {
        stage(h0, min(RH_HC, H - h0));
        const f32x4 v0 = *(const f32x4*)(Vc + row * RH_LDH + 4 * l), v1 = *(const f32x4*)(Vc + row * RH_LDH + 64 + 4 * l);
        const f32x4 w0 = *(const f32x4*)(wc + 4 * l), w1 = *(const f32x4*)(wc + 64 + 4 * l);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            for (int nn = 0; nn < 16 && 16 * j + nn < N; ++nn) {
                const float* u = Uc + (16 * j + nn) * RH_LDH + 4 * l;
                const f32x4 u0 = *(const f32x4*)u, u1 = *(const f32x4*)(u + 64);
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) { const float p = u0[k] + v0[k]; s += w0[k] * (p <= 0.f ? 0.f : p); }
#pragma unroll
                for (int k = 0; k < 4; ++k) { const float p = u1[k] + v1[k]; s += w1[k] * (p <= 0.f ? 0.f : p); }
                for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                if (l == nn) z[j] += s;
            }
        }
    }
    {
        const float bias = b2[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] += bias;
    }

    {
        float loss = 0.f, hit = 0.f, sdz = 0.f;
        // the row's first arg-max, as in the rows kernels of the other heads (cosproto.hip)
        float mx = -INFINITY; int arg = N;
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; if (n < N && z[j] > mx) { mx = z[j]; arg = n; } }
        for (int o = 8; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(mx, o, 64); const int a2 = __shfl_xor(arg, o, 64);
            if (v2 > mx || (v2 == mx && a2 < arg)) { mx = v2; arg = a2; }                   // first arg-max (torch.max)
        }
        if (arg >= N) arg = 0;                                                               // (a row of NaNs)
        long yv = live ? yq[r0 + row] : 0;
        const bool inr = yv >= 0 && yv < N;
        if (!inr) { if (l == 0) atomicOr(status, FUMI_ST_LABEL_RANGE); yv = 0; }
        const bool ok = live && inr;
        float dz[4];
        if (rd.mse) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = l + 16 * j;
                const float s = 1.f / (1.f + expf(-z[j]));
                const float e = s - (n == (int)yv ? 1.f : 0.f);
                if (n < N) loss += e * e;
                dz[j] = (ok && n < N) ? rd.gz * e * s * (1.f - s) : 0.f;
            }
            for (int o = 8; o > 0; o >>= 1) loss += __shfl_xor(loss, o, 64);
        } else {
            float e[4], s = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) { e[j] = l + 16 * j < N ? expf(z[j] - mx) : 0.f; s += e[j]; }
            for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            const int jy = (int)yv >> 4;
            const float zs = jy == 0 ? z[0] : jy == 1 ? z[1] : jy == 2 ? z[2] : z[3];
            const float zy = __shfl(zs, (tid & 48) + ((int)yv & 15), 64);
            loss = logf(s) - (zy - mx);
            const float inv = 1.f / s;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = l + 16 * j;
                dz[j] = (ok && n < N) ? rd.gz * (e[j] * inv - (n == (int)yv ? 1.f : 0.f)) : 0.f;
            }
        }
        if (!ok) loss = 0.f;
        hit = (ok && arg == (int)yv) ? 1.f : 0.f;
        if (live) {
            if (l == 0 && preds) preds[r0 + row] = arg;
            if (logits) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const int n = l + 16 * j; if (n < N) logits[(r0 + row) * N + n] = z[j]; }
            }
        }
        if (d.train) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = l + 16 * j;
                if (n < N) {
                    sdz += dz[j];
                    DZ[row * ldz + n] = dz[j];
                    if (live) dzg[(r0 + row) * N + n] = dz[j];
                }
            }
            for (int o = 8; o > 0; o >>= 1) sdz += __shfl_xor(sdz, o, 64);
        }
        if (l == 0) { rl[row] = loss; rl[16 + row] = hit; rl[32 + row] = sdz; }
    }
    __syncthreads();
    fh_tile_part<3>(rl, part, d.ntile);
    if (!d.train) return;
    // dV[q, h] = w2[h] sum_n dz[q, n] (U[n,h] + V[q,h] > 0), classes in index order
    for (int h0 = 0; h0 < H; h0 += RH_HC) {
        const int hc = min(RH_HC, H - h0);
        if (H > RH_HC) stage(h0, hc);            // (one chunk: it is still staged)
        const f32x4 v0 = *(const f32x4*)(Vc + row * RH_LDH + 4 * l), v1 = *(const f32x4*)(Vc + row * RH_LDH + 64 + 4 * l);
        const f32x4 w0 = *(const f32x4*)(wc + 4 * l), w1 = *(const f32x4*)(wc + 64 + 4 * l);
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
        for (int n = 0; n < N; ++n) {
            const float* u = Uc + n * RH_LDH + 4 * l;
            const f32x4 u0 = *(const f32x4*)u, u1 = *(const f32x4*)(u + 64);
            const float g = DZ[row * ldz + n];
#pragma unroll
            for (int k = 0; k < 4; ++k) { a0[k] += (u0[k] + v0[k] > 0.f) ? g : 0.f; a1[k] += (u1[k] + v1[k] > 0.f) ? g : 0.f; }
        }
        if (live) {
            float* o = dV + (r0 + row) * H + h0;
            if (4 * l < hc) *(f32x4*)(o + 4 * l) = w0 * a0;
            if (64 + 4 * l < hc) *(f32x4*)(o + 64 + 4 * l) = w1 * a1;
        }
    }
}

__global__ __launch_bounds__(256) void rel_du_kernel(HeadDims d, RelDims rd, int nhc, int epg, const float* __restrict__ U,
                                                     const float* __restrict__ V, const float* __restrict__ dzg,
                                                     const float* __restrict__ w2, float* __restrict__ dU, float* __restrict__ pw2,
                                                     float* __restrict__ pb1) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int B = d.B, Qn = d.Qn, N = d.N, H = rd.H;
    const int g = blockIdx.x / nhc, h0 = (blockIdx.x - g * nhc) * RH_HC, hc = min(RH_HC, H - h0);
    float* Ul = sm;                              // [N, 128] the episode's U chunk
    float* acc = Ul + N * RH_HC;                 // [N, 128] sum_q dz m over the staged block of rows
    float* tot = acc + N * RH_HC;                // [N, 128] the blocks' sums, added in block order
    float* Vb = tot + N * RH_HC;                 // [64, 128] a block of V rows; then the halves' dw2 sums
    float* dzT = Vb + RH_QB * RH_HC;             // [N, RH_LDQ] the block's dz, transposed
    const int h = tid & (RH_HC - 1), half = tid >> 7;   // this thread's hidden unit; it takes the classes half, half + 2, ...
    const bool act = h < hc;
    const float w = act ? w2[h0 + h] : 0.f;
    float sw2 = 0.f, sb1 = 0.f;
    const int b1 = min(B, (g + 1) * epg);
    for (int b = g * epg; b < b1; ++b) {
        __syncthreads();
        rh_stage(Ul, RH_HC, N, N, hc, U + (long)b * N * H + h0, H);
        for (int i = tid; i < N * RH_HC; i += 256) tot[i] = 0.f;
        // Three levels, each in index order: 8 rows in registers, the 64 rows of a staged block, the blocks.  Qn reaches 65536 and the
        // terms of a class cancel (rows of dz sum to zero with the ce loss): one running sum over all rows would lose the digits.
        float a2 = 0.f;
        for (int qb = 0; qb < Qn; qb += RH_QB) {
            const int nq = min(RH_QB, Qn - qb);
            __syncthreads();
            rh_stage(Vb, RH_HC, RH_QB, nq, hc, V + ((long)b * Qn + qb) * H + h0, H);
            for (int i = tid; i < RH_QB * N; i += 256) {
                const int r = i / N, n = i - r * N;
                dzT[n * RH_LDQ + r] = r < nq ? dzg[((long)b * Qn + qb) * N + i] : 0.f;
            }
            __syncthreads();
            float a2b = 0.f;
            for (int qs = 0; qs < nq; qs += 8) {
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = Vb[(qs + k) * RH_HC + h];
                for (int n = half; n < N; n += 2) {
                    const float u = Ul[n * RH_HC + h];
                    const f32x4 d0 = *(const f32x4*)(dzT + n * RH_LDQ + qs), d1 = *(const f32x4*)(dzT + n * RH_LDQ + qs + 4);
                    float s8 = 0.f, t8 = 0.f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const float p = u + v[k], dk = k < 4 ? d0[k & 3] : d1[k & 3];
                        s8 += p > 0.f ? dk : 0.f;
                        t8 += dk * (p <= 0.f ? 0.f : p);
                    }
                    acc[n * RH_HC + h] = qs == 0 ? s8 : acc[n * RH_HC + h] + s8;      // (this thread's own entries: no barrier)
                    a2b += t8;
                }
            }
            for (int n = half; n < N; n += 2) tot[n * RH_HC + h] += acc[n * RH_HC + h];
            a2 += a2b;
        }
        __syncthreads();
        Vb[tid] = a2;
        __syncthreads();
        if (half == 0) {
            sw2 += Vb[h] + Vb[RH_HC + h];
            float sb = 0.f;
            for (int n = 0; n < N; ++n) {
                const float du = w * tot[n * RH_HC + h];
                if (act) dU[((long)b * N + n) * H + h0 + h] = du;
                sb += du;
            }
            sb1 += sb;
        }
    }
    if (half == 0 && act) { pw2[(long)g * H + h0 + h] = sw2; pb1[(long)g * H + h0 + h] = sb1; }
}

__global__ __launch_bounds__(256) void rel_final_kernel(HeadDims d, RelDims rd, int nfb, int ncb, int nhb, int nbg,
                                                        const int64_t* __restrict__ ys, const float* __restrict__ cntf,
                                                        const float* __restrict__ dc, const float* __restrict__ pw2,
                                                        const float* __restrict__ pb1, const float* __restrict__ part,
                                                        float* __restrict__ loss, float* __restrict__ correct,
                                                        float* __restrict__ dfs, float* __restrict__ dw2, float* __restrict__ db1,
                                                        float* __restrict__ db2) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x;
    const int S = d.S, N = d.N, F = d.F, H = rd.H;
    if (blockIdx.x == gridDim.x - 1) {           // the sums over the row tiles
        fh_sum_parts<3>(part, d.ntile, sm, [&](const float (&t)[3]) {
            loss[0] = t[0] * rd.linv; correct[0] = t[1];
            if (db2) db2[0] = t[2];
        });
        return;
    }
    const int nsc = d.B * ncb * nfb;
    if ((int)blockIdx.x >= nsc) {                // dw2, db1: the groups' partial rows in index order
        const int hh = ((int)blockIdx.x - nsc) * 256 + tid;
        if (hh < H) {
            float a = 0.f, c = 0.f;
            for (int k = 0; k < nbg; ++k) { a += pw2[(long)k * H + hh]; c += pb1[(long)k * H + hh]; }
            dw2[hh] = a; db1[hh] = c;
        }
        return;
    }
    const int per = ncb * nfb;
    const int b = blockIdx.x / per, r = blockIdx.x - b * per, cb = r / nfb, fb = r - cb * nfb;
    const int c0 = cb * FH_TM, f0 = fb * FH_NB;
    const int nc = min(FH_TM, N - c0), nf = min(FH_NB, F - f0);
    float* dcl = sm;                             // [16, FH_LDC]
    for (int i = tid; i < FH_TM * FH_NB; i += 256) {
        const int m = i >> 7, n = i & (FH_NB - 1);
        dcl[m * FH_LDC + n] = (m < nc && n < nf) ? dc[((long)b * N + c0 + m) * F + f0 + n] : 0.f;
    }
    __syncthreads();
    fh_scatter_class_grad(dcl, ys, cntf, dfs, b, S, N, F, c0, nc, f0, nf, cb == 0);
}

}  // namespace

extern "C" int fumi_hip_relation_head_step(fumi_ws_t* ws, fumi_stream_t stream, int B, int S, int Qn, int N, int F, int H,
        const float* feats_s, const int64_t* y_s, const float* feats_q, const int64_t* y_q, const float* w1, const float* b1,
        const float* w2, const float* b2, int loss_kind, float grad_scale,
        float* loss, float* correct, int64_t* preds, float* logits, float* hid_s, float* hid_q,
        float* dfeats_s, float* dfeats_q, float* dw1, float* db1, float* dw2, float* db2) {
    const bool own = S <= RH_SMAX && H % 32 == 0 && H >= 32 && H <= RH_HMAX && (loss_kind == 0 || loss_kind == 1);
    if (int rc = head_args_check(ws, B, S, Qn, N, F, own, {feats_s, y_s, feats_q, y_q, w1, b1, w2, b2, loss, correct})) return rc;
    const int ngrad = (dfeats_s ? 1 : 0) + (dfeats_q ? 1 : 0) + (dw1 ? 1 : 0) + (db1 ? 1 : 0) + (dw2 ? 1 : 0) + (db2 ? 1 : 0);
    if (ngrad != 0 && ngrad != 6) return FUMI_EINVAL;
    const int train = ngrad == 6;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipSetDevice(ws->device));
    const HeadDims d = head_dims_fill(B, S, Qn, N, F, train, grad_scale);
    RelDims rd;
    rd.H = H; rd.mse = loss_kind;
    const double rowsN = (double)B * Qn * (loss_kind ? N : 1);
    rd.gz = (float)((loss_kind ? 2.0 : 1.0) * (double)grad_scale / rowsN); rd.linv = (float)(1.0 / rowsN);
    const long MQ = (long)B * Qn, MS = (long)B * N, HF = (long)H * F;
    const int nhc = (H + RH_HC - 1) / RH_HC, nhb = (H + 255) / 256;
    const int epg = (B + RH_MAXG - 1) / RH_MAXG, nbg = (B + epg - 1) / epg;
    // the weight gradients contract over all MQ (MS) rows: slabs of at least 512 rows, at most 8, at most 4 M floats of slabs
    auto nsplit_of = [&](long K) { long n = K / 512; n = n < 8 ? n : 8; const long cap = (4L << 20) / HF; n = n < cap ? n : cap; return (int)(n < 1 ? 1 : n); };
    const int nsq = nsplit_of(MQ), nss = nsplit_of(MS);
    const size_t n_cm = (size_t)MS * F, n_cnt = (size_t)MS, n_part = (size_t)3 * d.ntile, n_u = (size_t)MS * H, n_v = (size_t)MQ * H,
                 n_dz = (size_t)MQ * N, n_pg = (size_t)nbg * H, n_sq = nsq > 1 ? (size_t)nsq * HF : 0, n_ss = nss > 1 ? (size_t)nss * HF : 0;
    size_t need = ws_align(n_cm * 4) + ws_align(n_cnt * 4) + ws_align(n_part * 4) + (hid_s ? 0 : ws_align(n_u * 4))
                  + (hid_q ? 0 : ws_align(n_v * 4));
    if (train) need += ws_align(n_dz * 4) + ws_align(n_v * 4) + ws_align(n_u * 4) + ws_align(n_cm * 4) + 2 * ws_align(n_pg * 4)
                       + ws_align(n_sq * 4) + ws_align(n_ss * 4);
    int rc = ws_reserve(ws, need);
    if (rc) return rc;
    float* cm = ws_f(ws, n_cm); float* cntf = ws_f(ws, n_cnt); float* part = ws_f(ws, n_part);
    float* U = hid_s ? hid_s : ws_f(ws, n_u); float* V = hid_q ? hid_q : ws_f(ws, n_v);
    float *dzg = nullptr, *dV = nullptr, *dU = nullptr, *dc = nullptr, *pw2 = nullptr, *pb1 = nullptr, *slq = nullptr, *sls = nullptr;
    if (train) {
        dzg = ws_f(ws, n_dz); dV = ws_f(ws, n_v); dU = ws_f(ws, n_u); dc = ws_f(ws, n_cm); pw2 = ws_f(ws, n_pg); pb1 = ws_f(ws, n_pg);
        slq = ws_f(ws, n_sq); sls = ws_f(ws, n_ss);
    }
    const size_t lds1 = ((size_t)N * FH_PF + S + N) * 4;
    const size_t lds4 = ((size_t)(N + FH_TM) * RH_LDH + RH_HC + FH_TM * d.ldz + 64) * 4;
    const size_t lds5 = ((size_t)3 * N * RH_HC + RH_QB * RH_HC + N * RH_LDQ) * 4;
    const size_t lds9 = train ? (size_t)FH_TM * FH_LDC * 4 : (size_t)768 * 4;    // at least the 768 floats of the tile sums
    FUMI_SET_DYN_LDS(rel_means_kernel, lds1);
    hipLaunchKernelGGL(rel_means_kernel, dim3(B * d.nfb1), dim3(256), lds1, st, d, feats_s, y_s, cm, cntf, ws->status);
    LAUNCH_CHECK();
    {
        GemmArgs g = gemm_args((int)MS, H, F, cm, F, w1, F, U, H);                           // U = C W1s^T + b1
        g.bias = b1;
        if ((rc = launch_gemm(st, g, 0, 0))) return rc;
        if ((rc = launch_gemm(st, gemm_args((int)MQ, H, F, feats_q, F, w1 + HF, F, V, H), 0, 0))) return rc;    // V = F_q W1q^T
    }
    FUMI_SET_DYN_LDS(rel_pair_kernel, lds4);
    hipLaunchKernelGGL(rel_pair_kernel, dim3(d.ntile), dim3(256), lds4, st, d, rd, U, V, w2, b2, y_q, preds, logits, part, dzg, dV,
                       ws->status);
    LAUNCH_CHECK();
    const int nfb = (F + FH_NB - 1) / FH_NB, ncb = (N + FH_TM - 1) / FH_TM;
    if (train) {
        FUMI_SET_DYN_LDS(rel_du_kernel, lds5);
        hipLaunchKernelGGL(rel_du_kernel, dim3(nbg * nhc), dim3(256), lds5, st, d, rd, nhc, epg, U, V, dzg, w2, dU, pw2, pb1);
        LAUNCH_CHECK();
        if ((rc = launch_gemm(st, gemm_args((int)MQ, F, H, dV, H, w1 + HF, F, dfeats_q, F), 0, 1))) return rc;   // dfeats_q = dV W1q
        if ((rc = launch_gemm(st, gemm_args((int)MS, F, H, dU, H, w1, F, dc, F), 0, 1))) return rc;              // dc = dU W1s
        auto wgrad = [&](long K, const float* dy, const float* x, float* out, int ns, float* slabs) -> int {     // out = dy^T x
            GemmArgs g = gemm_args(H, F, (int)K, dy, H, x, F, out, F);
            if (ns > 1) {
                g.kchunk = (int)((((K + ns - 1) / ns) + 31) & ~31L); g.nsplit = (int)((K + g.kchunk - 1) / g.kchunk);
                g.C = slabs; g.sCsplit = HF;
            }
            if (int r = launch_gemm(st, g, 1, 1)) return r;
            return ns > 1 ? launch_reduce_slabs(st, slabs, g.nsplit, HF, HF, 1.f, out) : FUMI_OK;
        };
        if ((rc = wgrad(MQ, dV, feats_q, dw1 + HF, nsq, slq))) return rc;                                       // dW1q = dV^T F_q
        if ((rc = wgrad(MS, dU, cm, dw1, nss, sls))) return rc;                                                  // dW1s = dU^T C
    }
    FUMI_SET_DYN_LDS(rel_final_kernel, lds9);
    hipLaunchKernelGGL(rel_final_kernel, dim3((train ? B * ncb * nfb + nhb : 0) + 1), dim3(256), lds9, st, d, rd, nfb, ncb, nhb, nbg,
                       y_s, cntf, dc, pw2, pb1, part, loss, correct, dfeats_s, dw2, db1, db2);
    LAUNCH_CHECK();
    return FUMI_OK;
}
