// Image gather for the GPU-resident episode sampler: a meta-batch of raw images straight from a uint8 pixel table in HBM.
//   out[i] = normalise(jitter(flip(crop(zero_pad(table[idx[i]])))))        table uint8 [n_images, C, H, W] (planar),
//                                                                             out   float [n_idx,    C, H, W]
// One launch per index list (support / query); 21 KB in and 85 KB out per 3 x 84 x 84 image, nothing touches the host.  Every
// random draw comes from the sampler's counter-based hash (sampler.hip: smix / srand_below) with the second counter
// 0xFF00 + stream_id -- the episode kernels use second counters below 64 and 0xFFFE / 0xFFFF -- so a batch is reproducible from
// (seed, step) and restated bit for bit in tests/image_gather_ref.py:
//   crop    ox = r(0, 2 pad + 1), oy = r(1, 2 pad + 1)   (pad > 0; else both = pad)         r(c, n) = srand_below(key, i, 0xFF00 + stream_id, c, n)
//   flip    fl = flip ? r(2, 2) : 0
//   source  sx = (fl ? W - 1 - x : x) + ox - pad, sy = y + oy - pad; byte 0 outside the image (zero padding, crop, flip: torchvision's order)
//   float   v = (float)u * fl32(1/255)
//   jitter  f_j = 1 + a_j (2 u_j - 1), u_j = r(3 + j, 2^24) 2^-24; a step whose amplitude is 0 is skipped
//             brightness v = clamp01(v f_0); contrast v = clamp01(m + f_1 (v - m)), m = mean over the H x W window of the gray value
//             g = 0.299 R + 0.587 G + 0.114 B; saturation v = clamp01(g + f_2 (v - g)) with g recomputed
//   out     (v - mean[c]) * inv_std[c]
// FMA contraction is off for the whole file (HIP's default is -ffp-contract=fast; common.h: adam_update1): every operation rounds
// on its own, so with the jitter off the result is bit-reproducible in numpy float32.  With the jitter on the only freedom is the
// order of the gray-mean sum: it is accumulated in double, in a fixed order (thread partials, wave shuffles, four waves through
// LDS; no atomics), so two calls give the same bits.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int IG_THREADS = 256;
constexpr int IG_STAGE = 6;                  // 16-byte loads in flight per thread: 6 x 256 x 16 = 24 KB covers 3 x 84 x 84 (21,168 bytes)
constexpr int IG_MAXC = 8;
constexpr int IG_TAIL = 2 * IG_MAXC * (int)sizeof(float) + 4 * (int)sizeof(double);   // mean / inv_std, wave partials
constexpr long IG_MAX_BYTES = 64 * 1024 - IG_TAIL - 16;                              // image bytes one workgroup stages (LDS)

typedef unsigned int ig_u32x4 __attribute__((ext_vector_type(4)));

struct ImgArgs {
    const unsigned char* table; long n_images;
    const int64_t* idx; long n_idx;
    float* out; int* status;
    int C, H, W, pad, flip, stream_id;
    unsigned key;
    unsigned magic_wu, magic_h;               // ceil(2^32 / d) of the two divisors (0 for d = 1): n / d = umulhi(n, magic), n d < 2^32
    float a0, a1, a2;
    float mean[IG_MAXC], inv_std[IG_MAXC];
};

__device__ __forceinline__ unsigned ig_mix(unsigned x) {                  // = smix (sampler.hip)
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ unsigned ig_rand_below(unsigned key, unsigned a, unsigned b, unsigned c, unsigned n) {     // = srand_below
    const unsigned r = ig_mix(ig_mix(ig_mix(key ^ (a * 0x9E3779B9U)) ^ (b * 0x85EBCA6BU)) ^ (c * 0xC2B2AE35U));
    return (unsigned)(((unsigned long long)r * n) >> 32);
}
__device__ __forceinline__ int ig_div(int n, unsigned magic) { return magic ? (int)__umulhi((unsigned)n, magic) : n; }
__device__ __forceinline__ float ig_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float ig_gray(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }

// VEC: the image is staged with 16-byte loads and a thread writes four consecutive floats of a row with one 16-byte store
// (image bytes % 16 == 0, W % 4 == 0, 16-byte aligned table and output); otherwise bytes in, one float out.  JIT: colour jitter
// (C == 3): a thread owns whole pixels, all three channels.
template <bool VEC, bool JIT>
__global__ __launch_bounds__(IG_THREADS) void gather_images_kernel(const ImgArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ig_smem[];
    constexpr int PX = VEC ? 4 : 1;
    const int tid = threadIdx.x, C = p.C, H = p.H, W = p.W, pad = p.pad;
    const int HW = H * W, nbytes = C * HW, Wu = W / PX;
    const int img_room = (nbytes + 15) & ~15;
    unsigned char* img = ig_smem;
    float* s_mean = (float*)(ig_smem + img_room);
    float* s_istd = s_mean + IG_MAXC;
    double* s_red = (double*)(s_istd + IG_MAXC);
#pragma unroll
    for (int k = 0; k < IG_MAXC; ++k)
        if (tid == k) { s_mean[k] = p.mean[k]; s_istd[k] = p.inv_std[k]; }
    const float k255 = 1.0f / 255.0f;

    for (long i = blockIdx.x; i < p.n_idx; i += gridDim.x) {
        long r = p.idx[i];
        if (r < 0 || r >= p.n_images) { if (tid == 0) atomicOr(p.status, FUMI_ST_LABEL_RANGE); r = 0; }
        const unsigned char* src = p.table + r * (long)nbytes;
        __syncthreads();                                          // the previous image's readers are done (and s_mean is written)
        if (VEC) {
            const int n16 = nbytes >> 4;
            const ig_u32x4* src16 = (const ig_u32x4*)src;
            for (int c0 = 0; c0 < n16; c0 += IG_THREADS * IG_STAGE) {
                ig_u32x4 v[IG_STAGE];
#pragma unroll
                for (int u = 0; u < IG_STAGE; ++u) { const int ch = c0 + u * IG_THREADS + tid; v[u] = src16[ch < n16 ? ch : n16 - 1]; }
#pragma unroll
                for (int u = 0; u < IG_STAGE; ++u) { const int ch = c0 + u * IG_THREADS + tid; if (ch < n16) ((ig_u32x4*)img)[ch] = v[u]; }
            }
        } else {
#pragma unroll 1
            for (int b = tid; b < nbytes; b += IG_THREADS) img[b] = src[b];
        }
        const unsigned ui = (unsigned)i, sid = 0xFF00u + (unsigned)p.stream_id;
        const int ox = pad > 0 ? (int)ig_rand_below(p.key, ui, sid, 0u, 2u * pad + 1u) : pad;
        const int oy = pad > 0 ? (int)ig_rand_below(p.key, ui, sid, 1u, 2u * pad + 1u) : pad;
        const bool fl = p.flip && ig_rand_below(p.key, ui, sid, 2u, 2u) != 0u;
        const int dx = ox - pad, dy = oy - pad;
        float* dst = p.out + i * (long)nbytes;
        __syncthreads();

        if (!JIT) {
            const int nu = C * H * Wu;
#pragma unroll VEC ? 2 : 1
            for (int q = tid; q < nu; q += IG_THREADS) {
                const int row = ig_div(q, p.magic_wu), x0 = (q - row * Wu) * PX;          // row = c * H + y
                const int c = ig_div(row, p.magic_h), y = row - c * H;
                const int sy = y + dy;
                const bool yin = sy >= 0 && sy < H;
                const unsigned char* line = img + (c * H + (yin ? sy : 0)) * W;
                const float mu = s_mean[c], is = s_istd[c];
                float o[PX];
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    const int x = x0 + k, sx = (fl ? W - 1 - x : x) + dx;
                    const bool in = yin && sx >= 0 && sx < W;
                    const unsigned u = line[in ? sx : 0];                       // always a byte of the staged image
                    o[k] = ((float)(in ? u : 0u) * k255 - mu) * is;
                }
                if (VEC) *(f32x4*)(dst + row * W + x0) = f32x4{o[0], o[1 % PX], o[2 % PX], o[3 % PX]};
                else dst[row * W + x0] = o[0];
            }
        } else {
            const float a0 = p.a0, a1 = p.a1, a2 = p.a2;
            float f[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float a = j == 0 ? a0 : j == 1 ? a1 : a2;
                const float uj = (float)ig_rand_below(p.key, ui, sid, 3u + j, 1u << 24) * 0x1p-24f;
                f[j] = 1.f + a * (2.f * uj - 1.f);
            }
            const int nu = H * Wu;
            float m = 0.f;
            for (int pass = a1 > 0.f ? 0 : 1; pass < 2; ++pass) {
                double part = 0.0;
                for (int q = tid; q < nu; q += IG_THREADS) {
                    const int y = ig_div(q, p.magic_wu), x0 = (q - y * Wu) * PX;
                    const int sy = y + dy;
                    const bool yin = sy >= 0 && sy < H;
                    const unsigned char* line = img + (yin ? sy : 0) * W;
                    float o[3][PX];
#pragma unroll
                    for (int k = 0; k < PX; ++k) {
                        const int x = x0 + k, sx = (fl ? W - 1 - x : x) + dx;
                        const bool in = yin && sx >= 0 && sx < W;
                        const int so = in ? sx : 0;
                        const unsigned u0 = line[so], u1 = line[HW + so], u2 = line[2 * HW + so];
                        float v0 = (float)(in ? u0 : 0u) * k255, v1 = (float)(in ? u1 : 0u) * k255, v2 = (float)(in ? u2 : 0u) * k255;
                        if (a0 > 0.f) { v0 = ig_clamp01(v0 * f[0]); v1 = ig_clamp01(v1 * f[0]); v2 = ig_clamp01(v2 * f[0]); }
                        if (pass == 0) {
                            part += (double)ig_gray(v0, v1, v2);
                        } else {
                            if (a1 > 0.f) {
                                v0 = ig_clamp01(m + f[1] * (v0 - m)); v1 = ig_clamp01(m + f[1] * (v1 - m)); v2 = ig_clamp01(m + f[1] * (v2 - m));
                            }
                            if (a2 > 0.f) {
                                const float g = ig_gray(v0, v1, v2);
                                v0 = ig_clamp01(g + f[2] * (v0 - g)); v1 = ig_clamp01(g + f[2] * (v1 - g)); v2 = ig_clamp01(g + f[2] * (v2 - g));
                            }
                            o[0][k] = (v0 - s_mean[0]) * s_istd[0];
                            o[1][k] = (v1 - s_mean[1]) * s_istd[1];
                            o[2][k] = (v2 - s_mean[2]) * s_istd[2];
                        }
                    }
                    if (pass == 1) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            if (VEC) *(f32x4*)(dst + c * HW + y * W + x0) = f32x4{o[c][0], o[c][1 % PX], o[c][2 % PX], o[c][3 % PX]};
                            else dst[c * HW + y * W + x0] = o[c][0];
                        }
                    }
                }
                if (pass == 0) {                                   // fixed order: 64 lanes by shuffles, then the four waves in turn
#pragma unroll
                    for (int s = 32; s > 0; s >>= 1) part += __shfl_down(part, s, 64);
                    if ((tid & 63) == 0) s_red[tid >> 6] = part;
                    __syncthreads();
                    m = (float)((((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]) / (double)HW);
                }
            }
        }
    }
}

unsigned ig_magic(int d) { return d <= 1 ? 0u : (unsigned)((0x100000000ULL + (unsigned)d - 1) / (unsigned)d); }

template <bool VEC, bool JIT>
void ig_launch(hipStream_t st, unsigned blocks, size_t lds, const ImgArgs& a) {
    hipLaunchKernelGGL((gather_images_kernel<VEC, JIT>), dim3(blocks), dim3(IG_THREADS), lds, st, a);
}

}  // namespace

extern "C" int fumi_hip_gather_images(fumi_ws_t* ws, fumi_stream_t stream, const uint8_t* table, int64_t n_images, int C, int H, int W,
        const int64_t* idx, int64_t n_idx, const float* mean, const float* inv_std, uint64_t seed, uint64_t step, int stream_id,
        int pad, int flip, float jit_brightness, float jit_contrast, float jit_saturation, float* out) {
    if (!ws || !table || !idx || !mean || !inv_std || !out || n_images < 1 || n_idx < 0) return FUMI_EINVAL;
    if (C < 1 || C > IG_MAXC || H < 1 || W < 1 || pad < 0 || pad > 64 || stream_id < 0 || stream_id > 0xFD) return FUMI_EINVAL;
    const float jit[3] = {jit_brightness, jit_contrast, jit_saturation};
    bool any = false;
    for (float j : jit) {
        if (!(j >= 0.f && j <= 1.f)) return FUMI_EINVAL;
        any |= j > 0.f;
    }
    if (any && C != 3) return FUMI_ENOTSUP;
    const long nbytes = (long)C * H * W;
    if ((long)H * W > IG_MAX_BYTES || nbytes > IG_MAX_BYTES || n_idx > 0xFFFFFFFFLL) return FUMI_ENOTSUP;     // one image per workgroup, in LDS
    if (n_idx == 0) return FUMI_OK;
    HIP_TRY(hipSetDevice(ws->device));
    auto mix = [](unsigned x) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; };
    unsigned key = mix((unsigned)(seed & 0xffffffffULL));                       // the key of fumi_hip_sample_episodes
    key = mix(key ^ (unsigned)(seed >> 32));
    key = mix(key ^ (unsigned)(step & 0xffffffffULL));
    key = mix(key ^ (unsigned)(step >> 32));
    const bool vec = nbytes % 16 == 0 && W % 4 == 0 && (uintptr_t)table % 16 == 0 && (uintptr_t)out % 16 == 0;
    ImgArgs a;
    a.table = table; a.n_images = (long)n_images; a.idx = idx; a.n_idx = (long)n_idx; a.out = out; a.status = ws->status;
    a.C = C; a.H = H; a.W = W; a.pad = pad; a.flip = flip ? 1 : 0; a.stream_id = stream_id; a.key = key;
    a.magic_wu = ig_magic(vec ? W / 4 : W); a.magic_h = ig_magic(H);
    a.a0 = jit[0]; a.a1 = jit[1]; a.a2 = jit[2];
    for (int c = 0; c < IG_MAXC; ++c) { a.mean[c] = c < C ? mean[c] : 0.f; a.inv_std[c] = c < C ? inv_std[c] : 1.f; }
    const size_t lds = (size_t)((nbytes + 15) & ~15L) + IG_TAIL;
    const unsigned blocks = (unsigned)(n_idx < 4096 ? n_idx : 4096);
    if (vec) { if (any) ig_launch<true, true>((hipStream_t)stream, blocks, lds, a); else ig_launch<true, false>((hipStream_t)stream, blocks, lds, a); }
    else     { if (any) ig_launch<false, true>((hipStream_t)stream, blocks, lds, a); else ig_launch<false, false>((hipStream_t)stream, blocks, lds, a); }
    LAUNCH_CHECK();
    return FUMI_OK;
}
