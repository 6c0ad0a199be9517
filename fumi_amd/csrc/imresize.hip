// Resize and random-resized-crop for the GPU-resident episode sampler: beside imgather.hip, for a uint8 pixel table whose images are
// not of the size the encoder takes.
//   out[i] = normalise(jitter(flip(resample(rect_i of table[idx[i]]))))     table uint8 [n_images, C, Hs, Ws] (planar),
//                                                                            out   float [n_idx,    C, Ho, Wo]
// rect_i = (x0, y0, w, h) in whole source pixels: one rectangle for the launch (fixed mode: resize + centre crop) or one
// random-resized-crop draw per image (random mode); it is resampled to Ho x Wo with a separable triangle filter (antialiased
// bilinear: plain bilinear with clamped edges when the rectangle is not larger than the output, a copy when it is of the same size).
// Per axis (n_in = w | h, n_out = Wo | Ho), every operation a float32 operation rounded on its own:
//   scale = (float)n_in / (float)n_out, s = max(scale, 1), inv = 1 / s
//   output x: c = scale * ((float)x + 0.5f); k0 = max(0, (int)(c - s + 0.5f)), k1 = min(n_in, (int)(c + s + 0.5f))
//             w_k = max(0, 1 - |((float)k - c + 0.5f) * inv|) for k0 <= k < k1; tot = sum of w_k in ascending k from 0.f
//   horizontal t[y'][x] = (sum in ascending k of w_k * (float)u[y0 + y'][x0 + k], acc = acc + w_k * v) / tot for every rectangle row,
//   vertical the same over t.  Then flip (counter 2), v = r * fl32(1/255), jitter (counters 3..5) and normalisation exactly as
//   imgather.hip does them; the gray mean runs over the Ho x Wo output in double in a fixed order.
// Random mode (counters 6..10 of the same hash, second counter 0xFF00 + stream_id), U(c) = (float)r(c, 1 << 24) * 0x1p-24f:
//   a = smin + (smax - smin) U(6); q = 1 + (rmax - 1) U(7); ratio = r(8, 2) ? q : 1 / q; A = (float)(Hs Ws)
//   w = clamp(rint(sqrt(a A ratio)), 1, Ws), h = clamp(rint(sqrt(a A / ratio)), 1, Hs); x0 = r(9, Ws - w + 1), y0 = r(10, Hs - h + 1)
// The whole is restated in numpy in tests/image_resize_ref.py; with the jitter off that restatement is this kernel bit for bit.
//
// Kernel: one workgroup per output image.  Only the rectangle's rows go to LDS (full-width rows of every channel, so a channel is
// one contiguous span; 16-byte loads from clamped addresses, the span's misalignment absorbed by LDS byte reads).  The first
// Wo + Ho threads write the per-axis tap tables (first tap, count, weights, tot) to LDS -- once per workgroup in fixed mode, once
// per image in random mode; taps of weight 0 at either end of a range are dropped (they add +0 to a non-negative sum: same bits).
// A thread then produces four consecutive output floats: for every tap row it recomputes the four horizontal sums from LDS bytes
// (no intermediate image: 3 x 160 x 84 floats would not fit) and accumulates them vertically.  Under jitter a thread owns whole
// pixels: it stores the three resampled channels of its quads to the output, the workgroup reduces the gray mean, and the thread
// re-reads its OWN stores for the colour pass (program order: no fence needed; LDS stays free for a second workgroup per CU).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RZ_THREADS = 256;
constexpr int RZ_STAGE = 3;                  // 16-byte loads in flight per thread: 3 x 256 x 16 = 12 KB covers a channel of 96 x 96
constexpr int RZ_MAXC = 8;
constexpr int RZ_MAXDIM = 4096;              // Hs, Ws, Ho, Wo
constexpr long RZ_MAX_LDS = 160 * 1024;
constexpr int RZ_HEAD = 4 * (int)sizeof(double) + (2 * RZ_MAXC + 4) * (int)sizeof(float);      // wave partials, mean / inv_std, amplitudes

typedef unsigned int rz_u32x4 __attribute__((ext_vector_type(4)));

struct RzArgs {
    const unsigned char* table; int n_images;
    const int64_t* idx; long n_idx;
    float* out; int* status;
    int C, Hs, Ws, Ho, Wo, flip, stream_id;
    int rx0, ry0, rw, rh;                     // fixed mode: the rectangle
    float smin, smax, rmax;                   // random mode
    int mtx, mty;                             // weight slots per output column / row
    int chan_room;                            // LDS bytes per staged channel (a multiple of 16)
    unsigned key;
    unsigned magic_wu, magic_ho;              // ceil(2^32 / d) of the two divisors (0 for d = 1)
    float a0, a1, a2;
    float mean[RZ_MAXC], inv_std[RZ_MAXC];
};

struct RzEnt { int k0, cnt; float tot; int pad; };      // LDS: the taps of one output column / row: first tap, count, sum of weights
struct RzTabs {                                          // LDS: the tap tables of one image
    RzEnt *ex, *ey;                                      // [Wo], [Ho]
    float *wx, *wy;                                      // [Wo][mtx], [Ho][mty]
};

__device__ __forceinline__ unsigned rz_mix(unsigned x) {                  // = smix (sampler.hip)
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ unsigned rz_rand_below(unsigned key, unsigned a, unsigned b, unsigned c, unsigned n) {     // = srand_below
    const unsigned r = rz_mix(rz_mix(rz_mix(key ^ (a * 0x9E3779B9U)) ^ (b * 0x85EBCA6BU)) ^ (c * 0xC2B2AE35U));
    return (unsigned)(((unsigned long long)r * n) >> 32);
}
__device__ __forceinline__ int rz_div(int n, unsigned magic) { return magic ? (int)__umulhi((unsigned)n, magic) : n; }
__device__ __forceinline__ float rz_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float rz_gray(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }

// the taps of output x of one axis: first tap, count (at most mt), weights w[x * mt + j], tot
__device__ __forceinline__ void rz_build_axis(int x, int n_in, int n_out, int mt, float* w, RzEnt* ent) {
    const float scale = (float)n_in / (float)n_out;
    const float s = fmaxf(scale, 1.f), inv = 1.f / s;
    const float c = scale * ((float)x + 0.5f);
    const int k0 = max(0, (int)(c - s + 0.5f)), k1 = min(n_in, (int)(c + s + 0.5f));
    float t = 0.f;
    int first = k0, n = 0, last = 0;
    for (int k = k0; k < k1; ++k) {
        const float wk = fmaxf(0.f, 1.f - fabsf(((float)k - c + 0.5f) * inv));
        t = t + wk;
        if (wk == 0.f && n == 0) { first = k + 1; continue; }
        if (n < mt) w[x * mt + n] = wk;
        ++n;
        if (wk != 0.f) last = n;
    }
    ent[x] = RzEnt{first, min(last, mt), t, 0};
}

// PX consecutive output columns x0.. of output row y of one channel (chan: the staged rows of the rectangle, at its first column),
// on the 0..255 scale, flipped
template <int PX>
__device__ __forceinline__ void rz_resample(const unsigned char* chan, int Ws, const RzTabs& T, int mtx, int mty, int y, int x0, bool fl,
                                            int Wo, float (&o)[PX]) {
    int kx[PX], cx[PX];
    float tx[PX], acc[PX];
    const float* wp[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const int x = x0 + k, xs = fl ? Wo - 1 - x : x;
        const RzEnt e = T.ex[xs];
        kx[k] = e.k0; cx[k] = e.cnt; tx[k] = e.tot; wp[k] = T.wx + xs * mtx; acc[k] = 0.f;
    }
    const RzEnt ey = T.ey[y];
    const int ky = ey.k0, cy = ey.cnt;
    const float* wyp = T.wy + y * mty;
    for (int jy = 0; jy < cy; ++jy) {
        const unsigned char* line = chan + (ky + jy) * Ws;
        const float wyv = wyp[jy];
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const unsigned char* px = line + kx[k];
            float h = 0.f;
            for (int jx = 0; jx < cx[k]; ++jx) h = h + wp[k][jx] * (float)px[jx];
            acc[k] = acc[k] + wyv * (h / tx[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < PX; ++k) o[k] = acc[k] / ey.tot;
}

// VEC: 16-byte staging loads and one 16-byte store of four consecutive floats (image bytes % 16 == 0, Wo % 4 == 0, 16-byte aligned
// table and output); otherwise bytes in, one float out.  JIT: colour jitter (C == 3).  RND: a rectangle per image.
template <bool VEC, bool JIT, bool RND>
__global__ __launch_bounds__(RZ_THREADS) void gather_images_resized_kernel(const RzArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rz_smem[];
    constexpr int PX = VEC ? 4 : 1;
    const int tid = threadIdx.x, C = JIT ? 3 : p.C, Hs = p.Hs, Ws = p.Ws, Ho = p.Ho, Wo = p.Wo;
    const int HWo = Ho * Wo, Wu = Wo / PX, room = p.chan_room, mtx = p.mtx, mty = p.mty;
    const int plane = Hs * Ws;
    const int img_bytes = C * plane;                          // (< 2^28: RZ_MAXC, RZ_MAXDIM)
    unsigned char* img = rz_smem;
    double* s_red = (double*)(rz_smem + C * room);
    float* s_mean = (float*)(s_red + 4);
    float* s_istd = s_mean + RZ_MAXC;
    RzTabs T;
    float* s_amp = s_istd + RZ_MAXC;            // the jitter amplitudes: read where the colour pass starts, so that they do not occupy
    T.ex = (RzEnt*)(s_amp + 4);                 // scalar registers during staging and resampling
    T.ey = T.ex + Wo; T.wx = (float*)(T.ey + Ho); T.wy = T.wx + Wo * mtx;
#pragma unroll
    for (int k = 0; k < RZ_MAXC; ++k)
        if (tid == k) { s_mean[k] = p.mean[k]; s_istd[k] = p.inv_std[k]; }
    if (JIT && tid == 0) { s_amp[0] = p.a0; s_amp[1] = p.a1; s_amp[2] = p.a2; }
    int rx0 = p.rx0, ry0 = p.ry0, rw = p.rw, rh = p.rh;
    if (!RND) {
        for (int e = tid; e < Wo + Ho; e += RZ_THREADS) {
            if (e < Wo) rz_build_axis(e, rw, Wo, mtx, T.wx, T.ex);
            else rz_build_axis(e - Wo, rh, Ho, mty, T.wy, T.ey);
        }
    }
    const float k255 = 1.0f / 255.0f;

    const unsigned n_idx = (unsigned)p.n_idx;                 // (< 2^31)
    for (unsigned i = blockIdx.x; i < n_idx; i += gridDim.x) {
        long r = p.idx[i];
        if (r < 0 || r >= p.n_images) { if (tid == 0) atomicOr(p.status, FUMI_ST_LABEL_RANGE); r = 0; }
        const unsigned ui = i, sid = 0xFF00u + (unsigned)p.stream_id;
        if (RND) {
            const float u6 = (float)rz_rand_below(p.key, ui, sid, 6u, 1u << 24) * 0x1p-24f;
            const float u7 = (float)rz_rand_below(p.key, ui, sid, 7u, 1u << 24) * 0x1p-24f;
            const float a = p.smin + (p.smax - p.smin) * u6;
            const float q = 1.f + (p.rmax - 1.f) * u7;
            const float ratio = rz_rand_below(p.key, ui, sid, 8u, 2u) != 0u ? q : 1.f / q;
            const float A = (float)plane;
            const float wf = sqrtf(a * A * ratio), hf = sqrtf(a * A / ratio);
            rw = (int)fminf(fmaxf(rintf(wf), 1.f), (float)Ws);
            rh = (int)fminf(fmaxf(rintf(hf), 1.f), (float)Hs);
            rx0 = (int)rz_rand_below(p.key, ui, sid, 9u, (unsigned)(Ws - rw + 1));
            ry0 = (int)rz_rand_below(p.key, ui, sid, 10u, (unsigned)(Hs - rh + 1));
        }
        const bool fl = p.flip && rz_rand_below(p.key, ui, sid, 2u, 2u) != 0u;
        const int span = rh * Ws, row0 = ry0 * Ws;                // bytes of one channel's rows; their offset in the channel
        const unsigned char* src_img = p.table + r * (long)img_bytes;
        __syncthreads();                                          // the previous image's readers are done (and s_mean is written)
        if (VEC) {
            const int n16 = ((span + 15) >> 4) + 1;               // covers the span from its 16-byte-aligned start; <= room / 16
            const int last16 = (img_bytes >> 4) - 1;              // a chunk past the image holds no byte of the span: clamped into it
#pragma unroll 1
            for (int c = 0; c < C; ++c) {
                const rz_u32x4* src16 = (const rz_u32x4*)src_img + ((c * plane + row0) >> 4);
                const int room16 = last16 - ((c * plane + row0) >> 4);
                rz_u32x4* to = (rz_u32x4*)(img + c * room);
                for (int c0 = 0; c0 < n16; c0 += RZ_THREADS * RZ_STAGE) {
                    rz_u32x4 v[RZ_STAGE];
#pragma unroll
                    for (int u = 0; u < RZ_STAGE; ++u) { const int ch = min(c0 + u * RZ_THREADS + tid, n16 - 1); v[u] = src16[min(ch, room16)]; }
#pragma unroll
                    for (int u = 0; u < RZ_STAGE; ++u) { const int ch = c0 + u * RZ_THREADS + tid; if (ch < n16) to[ch] = v[u]; }
                }
            }
        } else {
            for (int c = 0; c < C; ++c) {
                const unsigned char* src = src_img + c * plane + row0;
#pragma unroll 1
                for (int b = tid; b < span; b += RZ_THREADS) img[c * room + b] = src[b];
            }
        }
        if (RND) {
            for (int e = tid; e < Wo + Ho; e += RZ_THREADS) {
                if (e < Wo) rz_build_axis(e, rw, Wo, mtx, T.wx, T.ex);
                else rz_build_axis(e - Wo, rh, Ho, mty, T.wy, T.ey);
            }
        }
        float* dst = p.out + (long)i * (C * HWo);
        __syncthreads();

        if (!JIT) {
            const int nu = C * Ho * Wu;
            for (int q = tid; q < nu; q += RZ_THREADS) {
                const int row = rz_div(q, p.magic_wu), x0 = (q - row * Wu) * PX;          // row = c * Ho + y
                const int c = rz_div(row, p.magic_ho), y = row - c * Ho;
                const int mis = VEC ? (c * plane + row0) & 15 : 0;        // (an image is a multiple of 16 bytes)
                float o[PX];
                rz_resample<PX>(img + c * room + mis + rx0, Ws, T, mtx, mty, y, x0, fl, Wo, o);
                const float mu = s_mean[c], is = s_istd[c];
#pragma unroll
                for (int k = 0; k < PX; ++k) o[k] = (o[k] * k255 - mu) * is;
                if (VEC) *(f32x4*)(dst + row * Wo + x0) = f32x4{o[0], o[1 % PX], o[2 % PX], o[3 % PX]};
                else dst[row * Wo + x0] = o[0];
            }
        } else {
            const int nu = Ho * Wu;
#pragma unroll 1
            for (int c = 0; c < 3; ++c) {                           // the resampled image, on the 0..1 scale, into the output
                const int mis = VEC ? (c * plane + row0) & 15 : 0;  // (an image is a multiple of 16 bytes)
                for (int q = tid; q < nu; q += RZ_THREADS) {        // (the same quads for every channel: the colour pass reads its own)
                    const int y = rz_div(q, p.magic_wu), x0 = (q - y * Wu) * PX;
                    float o[PX];
                    rz_resample<PX>(img + c * room + mis + rx0, Ws, T, mtx, mty, y, x0, fl, Wo, o);
#pragma unroll
                    for (int k = 0; k < PX; ++k) o[k] = o[k] * k255;
                    if (VEC) *(f32x4*)(dst + c * HWo + y * Wo + x0) = f32x4{o[0], o[1 % PX], o[2 % PX], o[3 % PX]};
                    else dst[c * HWo + y * Wo + x0] = o[0];
                }
            }
            const float a0 = s_amp[0], a1 = s_amp[1], a2 = s_amp[2];       // (in vector registers: the same value in every lane)
            const bool on0 = a0 > 0.f, on1 = a1 > 0.f, on2 = a2 > 0.f;
            float f[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float a = j == 0 ? a0 : j == 1 ? a1 : a2;
                const float uj = (float)rz_rand_below(p.key, ui, sid, 3u + j, 1u << 24) * 0x1p-24f;
                f[j] = 1.f + a * (2.f * uj - 1.f);
            }
            float m = 0.f;
            for (int pass = on1 ? 0 : 1; pass < 2; ++pass) {  // a thread reads back the quads it stored itself
                double part = 0.0;
                for (int q = tid; q < nu; q += RZ_THREADS) {
                    const int y = rz_div(q, p.magic_wu), x0 = (q - y * Wu) * PX;
                    float* at = dst + y * Wo + x0;
                    float in[3][PX], o[3][PX];
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if (VEC) { const f32x4 t = *(const f32x4*)(at + c * HWo); in[c][0] = t[0]; in[c][1 % PX] = t[1]; in[c][2 % PX] = t[2]; in[c][3 % PX] = t[3]; }
                        else in[c][0] = at[c * HWo];
                    }
#pragma unroll
                    for (int k = 0; k < PX; ++k) {
                        float v0 = in[0][k], v1 = in[1][k], v2 = in[2][k];
                        if (on0) { v0 = rz_clamp01(v0 * f[0]); v1 = rz_clamp01(v1 * f[0]); v2 = rz_clamp01(v2 * f[0]); }
                        if (pass == 0) {
                            part += (double)rz_gray(v0, v1, v2);
                        } else {
                            if (on1) {
                                v0 = rz_clamp01(m + f[1] * (v0 - m)); v1 = rz_clamp01(m + f[1] * (v1 - m)); v2 = rz_clamp01(m + f[1] * (v2 - m));
                            }
                            if (on2) {
                                const float g = rz_gray(v0, v1, v2);
                                v0 = rz_clamp01(g + f[2] * (v0 - g)); v1 = rz_clamp01(g + f[2] * (v1 - g)); v2 = rz_clamp01(g + f[2] * (v2 - g));
                            }
                            o[0][k] = (v0 - s_mean[0]) * s_istd[0];
                            o[1][k] = (v1 - s_mean[1]) * s_istd[1];
                            o[2][k] = (v2 - s_mean[2]) * s_istd[2];
                        }
                    }
                    if (pass == 1) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            if (VEC) *(f32x4*)(at + c * HWo) = f32x4{o[c][0], o[c][1 % PX], o[c][2 % PX], o[c][3 % PX]};
                            else at[c * HWo] = o[c][0];
                        }
                    }
                }
                if (pass == 0) {                                   // fixed order: 64 lanes by shuffles, then the four waves in turn
#pragma unroll
                    for (int s = 32; s > 0; s >>= 1) part += __shfl_down(part, s, 64);
                    if ((tid & 63) == 0) s_red[tid >> 6] = part;
                    __syncthreads();
                    m = (float)((((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]) / (double)HWo);
                }
            }
        }
    }
}

unsigned rz_magic(int d) { return d <= 1 ? 0u : (unsigned)((0x100000000ULL + (unsigned)d - 1) / (unsigned)d); }

// weight slots per output of an axis that resamples at most n_in pixels to n_out: k1 - k0 <= floor(2 s) + 1, one more for rounding
int rz_slots(int n_in, int n_out) {
    const double s = n_in > n_out ? (double)n_in / n_out : 1.0;
    return (int)(2.0 * s) + 2;
}

template <bool VEC, bool JIT, bool RND>
int rz_launch(hipStream_t st, unsigned blocks, size_t lds, const RzArgs& a) {
    FUMI_SET_DYN_LDS((gather_images_resized_kernel<VEC, JIT, RND>), lds);
    hipLaunchKernelGGL((gather_images_resized_kernel<VEC, JIT, RND>), dim3(blocks), dim3(RZ_THREADS), lds, st, a);
    LAUNCH_CHECK();
    return FUMI_OK;
}

template <bool VEC, bool JIT>
int rz_launch_mode(bool rnd, hipStream_t st, unsigned blocks, size_t lds, const RzArgs& a) {
    return rnd ? rz_launch<VEC, JIT, true>(st, blocks, lds, a) : rz_launch<VEC, JIT, false>(st, blocks, lds, a);
}

}  // namespace

extern "C" int fumi_hip_gather_images_resized(fumi_ws_t* ws, fumi_stream_t stream, const uint8_t* table, int64_t n_images, int C,
        int Hs, int Ws, int Ho, int Wo, const int64_t* idx, int64_t n_idx, const float* mean, const float* inv_std, uint64_t seed,
        uint64_t step, int stream_id, int mode, int rect_x0, int rect_y0, int rect_w, int rect_h, float scale_min, float scale_max,
        float ratio_max, int flip, float jit_brightness, float jit_contrast, float jit_saturation, float* out) {
    if (!ws || !table || !idx || !mean || !inv_std || !out || n_images < 1 || n_idx < 0) return FUMI_EINVAL;
    if (C < 1 || C > RZ_MAXC || Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1 || stream_id < 0 || stream_id > 0xFD) return FUMI_EINVAL;
    if (mode != FUMI_RESIZE_FIXED && mode != FUMI_RESIZE_RANDOM) return FUMI_EINVAL;
    const bool rnd = mode == FUMI_RESIZE_RANDOM;
    if (rnd) {
        if (!(scale_min > 0.f && scale_min <= scale_max && scale_max <= 1.f)) return FUMI_EINVAL;
        if (!(ratio_max >= 1.f && ratio_max <= 3.0e38f)) return FUMI_EINVAL;
    } else {
        if (rect_w < 1 || rect_h < 1 || rect_x0 < 0 || rect_y0 < 0 || rect_w > Ws || rect_h > Hs || rect_x0 > Ws - rect_w
            || rect_y0 > Hs - rect_h) return FUMI_EINVAL;
    }
    const float jit[3] = {jit_brightness, jit_contrast, jit_saturation};
    bool any = false;
    for (float j : jit) {
        if (!(j >= 0.f && j <= 1.f)) return FUMI_EINVAL;
        any |= j > 0.f;
    }
    if (any && C != 3) return FUMI_ENOTSUP;
    if (Hs > RZ_MAXDIM || Ws > RZ_MAXDIM || Ho > RZ_MAXDIM || Wo > RZ_MAXDIM || n_idx > 0x7FFFFFFFLL || n_images > 0x7FFFFFFFLL) return FUMI_ENOTSUP;
    // LDS of one workgroup: the rectangle's full-width rows of every channel (all rows in random mode) + the tap tables
    const int rows = rnd ? Hs : rect_h;
    const int mtx = rz_slots(rnd ? Ws : rect_w, Wo), mty = rz_slots(rows, Ho);
    const long room = (((long)rows * Ws + 15) & ~15L) + 16;
    const long lds = (long)C * room + RZ_HEAD + 4L * ((long)Wo * mtx + (long)Ho * mty + 4L * (Wo + Ho));
    if (lds > RZ_MAX_LDS || (long)C * Ho * Wo * (Wo > Ho ? Wo : Ho) >= (1L << 32)) return FUMI_ENOTSUP;     // (rz_div: n d < 2^32)
    if (n_idx == 0) return FUMI_OK;
    HIP_TRY(hipSetDevice(ws->device));
    auto mix = [](unsigned x) { x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x; };
    unsigned key = mix((unsigned)(seed & 0xffffffffULL));                       // the key of fumi_hip_sample_episodes
    key = mix(key ^ (unsigned)(seed >> 32));
    key = mix(key ^ (unsigned)(step & 0xffffffffULL));
    key = mix(key ^ (unsigned)(step >> 32));
    const bool vec = ((long)C * Hs * Ws) % 16 == 0 && Wo % 4 == 0 && (uintptr_t)table % 16 == 0 && (uintptr_t)out % 16 == 0;
    RzArgs a;
    a.table = table; a.n_images = (int)n_images; a.idx = idx; a.n_idx = (long)n_idx; a.out = out; a.status = ws->status;
    a.C = C; a.Hs = Hs; a.Ws = Ws; a.Ho = Ho; a.Wo = Wo; a.flip = flip ? 1 : 0; a.stream_id = stream_id; a.key = key;
    a.rx0 = rnd ? 0 : rect_x0; a.ry0 = rnd ? 0 : rect_y0; a.rw = rnd ? Ws : rect_w; a.rh = rnd ? Hs : rect_h;
    a.smin = scale_min; a.smax = scale_max; a.rmax = ratio_max;
    a.mtx = mtx; a.mty = mty; a.chan_room = (int)room;
    a.magic_wu = rz_magic(vec ? Wo / 4 : Wo); a.magic_ho = rz_magic(Ho);
    a.a0 = jit[0]; a.a1 = jit[1]; a.a2 = jit[2];
    for (int c = 0; c < RZ_MAXC; ++c) { a.mean[c] = c < C ? mean[c] : 0.f; a.inv_std[c] = c < C ? inv_std[c] : 1.f; }
    const unsigned blocks = (unsigned)(n_idx < 4096 ? n_idx : 4096);
    const hipStream_t st = (hipStream_t)stream;
    if (vec) return any ? rz_launch_mode<true, true>(rnd, st, blocks, (size_t)lds, a) : rz_launch_mode<true, false>(rnd, st, blocks, (size_t)lds, a);
    return any ? rz_launch_mode<false, true>(rnd, st, blocks, (size_t)lds, a) : rz_launch_mode<false, false>(rnd, st, blocks, (size_t)lds, a);
}
