// DropBlock / dropout on the pooled block outputs of the bf16 ResNet-12 (the MetaOptNet / RFS ResNet-12: element-wise dropout after
// the early blocks, DropBlock after the late ones).  The maps are bf16 "padded channels-last" [B][M (H+2)(W+2)][C] (rn12.h).
//
// The mask is a pure function of (64-bit seed, block, set, GLOBAL episode b0 + b, image m, channel c, seed position (i, j)): a chain
// of 32-bit counter mixes (the `mix` of the inner-loop dropout, common.h / episode.hip) keyed per dimension, so no flat index exists
// that could wrap, and nothing of the mask is stored: the count launch and the apply launch, the forward and the backward, every
// chunking and both forms of the encoder pair regenerate the same bits.
//
//   plane key (k0, k1):  k0 = mix(mix(mix(mix(seed_lo ^ G1 (2 blk + set + 1)) ^ seed_hi) + G2 e) ^ G3 m),  k1 = mix(k0 ^ G4 (c + 1))
//   seed (i, j) is set   iff  mix(mix(k0 ^ (i << 16 | j)) ^ k1) < thr          (thr = floor(gamma 2^32), computed by the host)
//
// bs == 1 (dropout): a set seed drops its own cell.  bs > 1 (DropBlock): seeds live on the (H-bs+1) x (W-bs+1) grid and seed (i, j)
// drops [i, i+bs) x [j, j+bs).  A lane owns one (image, channel) plane and walks its rows: the row's seed bits are built in one
// 64-bit word (W <= 64), dilated along the row with bs shift-ORs, and down the rows by OR-ing the last bs row words, which live in
// registers (bs <= 8) -- every seed is hashed once per plane and launch.  Consecutive lanes hold consecutive channels: coalesced.
//
// out = keep * scale * x, scale = (float)total / (float)kept over one batch-statistics group (one episode's support or query set,
// total = M H W C); kept is an INTEGER count (64-bit integer atomics: no order problem), scale is formed once by the last workgroup
// of the group in the count launch; the product is fp32, rounded to bf16 to nearest-even.  Borders are not touched.
#include "rn12.h"

namespace {

__device__ __forceinline__ unsigned dk_mix(unsigned x) {                 // = drop_mix (episode.hip)
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}

struct DropArgs {
    int M, H, W, C, bs;                       // bs: effective block size (1: dropout)
    unsigned thr, seed_lo, seed_hi;
    int blk, set, b0;
    long total;                               // M H W C
};

// key of the group's planes before the image and the channel are mixed in
__device__ __forceinline__ unsigned dk_group_key(const DropArgs& a, int b) {
    unsigned k = dk_mix(a.seed_lo ^ (0x9E3779B9U * (unsigned)(2 * a.blk + a.set + 1)));
    k = dk_mix(k ^ a.seed_hi);
    return dk_mix(k + 0x85EBCA6BU * (unsigned)(a.b0 + b));
}
__device__ __forceinline__ bool dk_seed(unsigned k0, unsigned k1, int i, int j, unsigned thr) {
    return dk_mix(dk_mix(k0 ^ (((unsigned)i << 16) | (unsigned)j)) ^ k1) < thr;
}

// One item per lane.  BLOCKS: item = plane (m, c);  else item = row (m, r, c) of an element-wise dropout (no coupling between rows).
// APPLY: x <- keep * scale * x in place;  else: count the kept cells of the group, the last workgroup of the group forms the scale.
template <bool BLOCKS, bool APPLY>
__global__ __launch_bounds__(256) void rn_drop_kernel(DropArgs a, rbf16* __restrict__ x, unsigned long long* __restrict__ kept,
                                                      unsigned* __restrict__ ticket, float* __restrict__ scale) {
    const int b = blockIdx.y;
    const long nitem = BLOCKS ? (long)a.M * a.C : (long)a.M * a.H * a.C;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    const int Wp = a.W + 2;
    const long Pp = (long)(a.H + 2) * Wp;
    unsigned cnt = 0;
    if (q < nitem) {
        const int c = (int)(q % a.C);
        const long t = q / a.C;
        const int m = BLOCKS ? (int)t : (int)(t / a.H);
        const unsigned k0 = dk_mix(dk_group_key(a, b) ^ (0xC2B2AE35U * (unsigned)m));
        const unsigned k1 = dk_mix(k0 ^ (0x27D4EB2FU * (unsigned)(c + 1)));
        const float sc = APPLY ? scale[b] : 0.f;
        rbf16* xp = APPLY ? x + (((long)b * a.M + m) * Pp) * a.C + c : nullptr;
        if (BLOCKS) {
            const int bs = a.bs, Hs = a.H - bs + 1, Ws = a.W - bs + 1;
            unsigned long long r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, r5 = 0, r6 = 0;     // the dilated seed rows r-1 .. r-7
            for (int r = 0; r < a.H; ++r) {
                unsigned long long s = 0;
                if (r < Hs) for (int j = 0; j < Ws; ++j) s |= (unsigned long long)dk_seed(k0, k1, r, j, a.thr) << j;
                unsigned long long d = s;
#pragma unroll
                for (int k = 1; k < 8; ++k) if (k < bs) d |= s << k;
                unsigned long long drop = d;
                if (bs > 1) drop |= r0;
                if (bs > 2) drop |= r1;
                if (bs > 3) drop |= r2;
                if (bs > 4) drop |= r3;
                if (bs > 5) drop |= r4;
                if (bs > 6) drop |= r5;
                if (bs > 7) drop |= r6;
                r6 = r5; r5 = r4; r4 = r3; r3 = r2; r2 = r1; r1 = r0; r0 = d;
                if (APPLY) {
                    rbf16* row = xp + ((long)(r + 1) * Wp + 1) * a.C;
                    for (int j = 0; j < a.W; ++j) {
                        rbf16* p = row + (long)j * a.C;
                        *p = (drop >> j) & 1ull ? (rbf16)0 : rn_f2bf(rn_bf2f(*p) * sc);
                    }
                } else {
                    cnt += (unsigned)(a.W - __popcll(drop));
                }
            }
        } else {
            const int r = (int)(t % a.H);
            rbf16* row = APPLY ? xp + ((long)(r + 1) * Wp + 1) * a.C : nullptr;
            for (int j = 0; j < a.W; ++j) {
                const bool drop = dk_seed(k0, k1, r, j, a.thr);
                if (APPLY) {
                    rbf16* p = row + (long)j * a.C;
                    *p = drop ? (rbf16)0 : rn_f2bf(rn_bf2f(*p) * sc);
                } else {
                    cnt += drop ? 0u : 1u;
                }
            }
        }
    }
    if (APPLY) return;
    __shared__ unsigned s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o);          // a workgroup's cells: < 2^32 (256 planes of <= 64 x 64, or rows)
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(&kept[b], (unsigned long long)s_cnt);
        __threadfence();
        if (atomicAdd(&ticket[b], 1u) == gridDim.x - 1) {                 // the last workgroup of the group: every count has landed
            __threadfence();
            const unsigned long long k = atomicAdd(&kept[b], 0ull);
            scale[b] = k ? __fdiv_rn((float)a.total, (float)k) : 0.f;
        }
    }
}

}  // namespace

// Refusals of both launches (nothing is launched): rate outside [0, 1), block outside 1..8, and for DropBlock a map beyond 64 x 64.
int rn_drop_plan(int H, int W, float rate, int block, int* bs_out, unsigned* thr_out) {
    if (H < 1 || W < 1 || !(rate >= 0.f) || !(rate < 1.f) || block < 1 || block > 8) return FUMI_EINVAL;
    if (block > 1 && (H > 64 || W > 64)) return FUMI_EINVAL;
    if (block == 1 && (H > 65535 || W > 65535)) return FUMI_EINVAL;
    int bs = block; if (bs > H) bs = H; if (bs > W) bs = W;
    const double gamma = (double)rate / ((double)bs * bs) * ((double)H * W) / ((double)(H - bs + 1) * (double)(W - bs + 1));
    double t = gamma * 4294967296.0;                                       // gamma <= rate < 1
    if (t > 4294967295.0) t = 4294967295.0;
    *bs_out = bs; *thr_out = (unsigned)t;                                  // floor
    return FUMI_OK;
}

// kept [B] (64-bit), ticket [B], scale [B]: kept and ticket are cleared here; `map` [B][M (H+2)(W+2)][C] is scaled in place.
// apply == 0: only the count launch (kept, scale);  count == 0: only the apply launch (reads scale).
int launch_rn_drop(hipStream_t st, int B, int M, const RnGeom& g, int C, float rate, int block, unsigned long long seed, int blk,
                   int set, int b0, rbf16* map, unsigned long long* kept, unsigned* ticket, float* scale, bool count, bool apply) {
    DropArgs a;
    const int rc = rn_drop_plan(g.H, g.W, rate, block, &a.bs, &a.thr);
    if (rc) return rc;
    if (B < 1 || M < 1 || C < 1 || blk < 0 || set < 0 || set > 1 || b0 < 0) return FUMI_EINVAL;
    a.M = M; a.H = g.H; a.W = g.W; a.C = C; a.seed_lo = (unsigned)(seed & 0xffffffffULL); a.seed_hi = (unsigned)(seed >> 32);
    a.blk = blk; a.set = set; a.b0 = b0; a.total = (long)M * g.H * g.W * C;
    const bool blocks = a.bs > 1;
    const long nitem = blocks ? (long)M * C : (long)M * g.H * C;
    const dim3 grid((unsigned)((nitem + 255) / 256), (unsigned)B);
    if (count) {
        if ((void*)ticket == (void*)(kept + B)) HIP_TRY(hipMemsetAsync(kept, 0, (size_t)B * 12, st));
        else {
            HIP_TRY(hipMemsetAsync(kept, 0, (size_t)B * 8, st));
            HIP_TRY(hipMemsetAsync(ticket, 0, (size_t)B * 4, st));
        }
        if (blocks) hipLaunchKernelGGL((rn_drop_kernel<true, false>), grid, dim3(256), 0, st, a, map, kept, ticket, scale);
        else hipLaunchKernelGGL((rn_drop_kernel<false, false>), grid, dim3(256), 0, st, a, map, kept, ticket, scale);
        LAUNCH_CHECK();
    }
    if (apply) {
        if (blocks) hipLaunchKernelGGL((rn_drop_kernel<true, true>), grid, dim3(256), 0, st, a, map, kept, ticket, scale);
        else hipLaunchKernelGGL((rn_drop_kernel<false, true>), grid, dim3(256), 0, st, a, map, kept, ticket, scale);
        LAUNCH_CHECK();
    }
    return FUMI_OK;
}
