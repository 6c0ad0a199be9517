// GloVe / word2vec embedding bag, the device body (glove.hip's kernel and the rider workgroups of xpanel.hip's pre-split launch share it).
// WordEmbedding.forward (fumi/models/common.py:23-41) + the per-class first-support-row pick of fumi/models/fumi.py:207-210.
#pragma once
#include "common.h"

// one 512-thread workgroup per output row: the row's L tokens are split over the 8 waves (8x the gathers in flight per
// row; the whole launch is only B*N = 160 rows at the bench shape, so a wave per row left most CUs idle)
constexpr int GW = 8;        // waves per output row
constexpr int GU = 16;       // row gathers in flight per wave
// one output row `r` by the 512 threads of the calling workgroup; part: [GW][Ep] partial sums / maxima, then [GW] counts (LDS)
template <bool VEC>
__device__ __forceinline__ void glove_bag_row(const GloveArgs& ga, int r, float* part) {
    const int64_t* __restrict__ tok = ga.tok; const float* __restrict__ table = ga.table; float* __restrict__ out = ga.out;
    const int L = ga.L, V = ga.V, E = ga.E, mode = ga.mode, N = ga.N, S = ga.S; const int64_t pad_id = ga.pad_id;
    const int64_t* __restrict__ y_s = ga.y_s; int* status = ga.status;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int W = VEC ? 4 : 1;
    const int nchunk = (E / W + 63) / 64;        // chunks of 64 lanes x W floats
    const int Ep = nchunk * 64 * W;
    float* cnts = part + GW * Ep;
    long src_row = r;
    if (y_s) {                                   // select form: output row r = (episode, class); source = first support row of the class
        const int b = r / N, c = r - b * N;
        const int64_t* ys = y_s + (long)b * S;
        int first = S;
        for (int s0 = 0; s0 < S && first == S; s0 += 64) {
            const int s_ = s0 + lane;
            const unsigned long long m = __ballot(s_ < S && ys[s_] == c);
            if (m) first = s0 + __ffsll((long long)m) - 1;
        }
        if (first == S) {                        // the reference raises IndexError here (fumi.py:209)
            if (threadIdx.x == 0) atomicOr(status, FUMI_ST_CLASS_MISSING);
            for (int j = threadIdx.x; j < E; j += blockDim.x) out[(long)r * E + j] = __builtin_nanf("");
            return;
        }
        src_row = (long)b * S + first;
    }
    const int64_t* t = tok + src_row * L;
    const int lw = (L + GW - 1) / GW;            // tokens per wave
    const int lbeg = wave * lw, lend = min(L, lbeg + lw);
    // CH chunks (c, .., c + CH - 1) in ONE pass over the wave's tokens: the CH * GU row gathers of a token batch are issued together.
    // Every chunk still adds (maxes) its tokens in increasing order into its own accumulator, so the pooled bits do not depend on CH.
    auto chunks = [&](auto ch, int c) {
        constexpr int CH = decltype(ch)::value;
        int jc[CH];
        f32x4 acc[CH];
#pragma unroll
        for (int h = 0; h < CH; ++h) {
            const int j = ((c + h) * 64 + lane) * W;
            jc[h] = j < E ? j : 0;
            acc[h] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (mode == 1) acc[h] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        }
        int cnt = 0;
        for (int l0 = lbeg; l0 < lend; l0 += 64) {
            const int nl = min(64, lend - l0);
            long my = lane < nl ? t[l0 + lane] : pad_id;
            cnt += __popcll(__ballot(lane < nl && my != pad_id));
            if (my < 0 || my >= V) { if (lane < nl) atomicOr(status, FUMI_ST_LABEL_RANGE); my = 0; }
            const int mylo = (int)my;
            for (int u0 = 0; u0 < nl; u0 += GU) {
                f32x4 v[CH][GU];
#pragma unroll
                for (int u = 0; u < GU; ++u) {
                    const int id = __shfl(mylo, min(u0 + u, nl - 1), 64);
#pragma unroll
                    for (int h = 0; h < CH; ++h) {
                        const float* row = table + (long)id * E + jc[h];
                        if (VEC) v[h][u] = *(const f32x4*)row; else { v[h][u] = (f32x4){0.f, 0.f, 0.f, 0.f}; v[h][u][0] = row[0]; }
                    }
                }
#pragma unroll
                for (int h = 0; h < CH; ++h) {
#pragma unroll
                    for (int u = 0; u < GU; ++u) {
                        if (u0 + u < nl) {
                            if (mode == 0) acc[h] += v[h][u];
                            else { acc[h][0] = fmaxf(acc[h][0], v[h][u][0]); acc[h][1] = fmaxf(acc[h][1], v[h][u][1]); acc[h][2] = fmaxf(acc[h][2], v[h][u][2]); acc[h][3] = fmaxf(acc[h][3], v[h][u][3]); }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int h = 0; h < CH; ++h) {
            float* pp = part + wave * Ep + ((c + h) * 64 + lane) * W;
            if (VEC) *(f32x4*)pp = acc[h]; else pp[0] = acc[h][0];
        }
        if (lane == 0 && c == 0) cnts[wave] = (float)cnt;
    };
    int c = 0;
    for (; c + 1 < nchunk; c += 2) chunks(WgInt<2>{}, c);                  // (E = 300: nchunk == 2, one pass, 32 gathers in flight)
    if (c < nchunk) chunks(WgInt<1>{}, c);
    __syncthreads();
    float dn = 0.f;
#pragma unroll
    for (int w_ = 0; w_ < GW; ++w_) dn += cnts[w_];
    for (int j = threadIdx.x; j < E; j += blockDim.x) {
        float a = part[j];
#pragma unroll
        for (int w_ = 1; w_ < GW; ++w_) a = mode == 0 ? a + part[w_ * Ep + j] : fmaxf(a, part[w_ * Ep + j]);
        out[(long)r * E + j] = mode == 0 ? a / dn : a;
    }
}

