// Blend of a gathered image batch with a permutation of itself: mixup and CutMix for supervised pre-training.
//   x, out float [M, C, H, W];  p = partner[i]
//   mode 0 (mixup)   out[i] = lam * x[i] + (1.0f - lam) * x[p]              every operation rounded on its own (no FMA contraction)
//   mode 1 (CutMix)  out[i][:, r, c] = x[p][:, r, c] for by0 <= r < by1, bx0 <= c < bx1, x[i] elsewhere: a copy, bit for bit
// A pass of its own behind either gather (imgather.hip / imresize.hip), so both images of a pair carry their own crop, flip and
// jitter draws.  A row whose partner is itself is copied; a partner outside [0, M) sets FUMI_ST_LABEL_RANGE and its row is copied
// unmixed as well: no read leaves x.  No LDS, no atomics but the OR into the status word.
// VEC: an image of a multiple of four floats (and 16-byte aligned x, out) moves as 128-bit loads and stores, one quad of four
// consecutive floats per thread and trip of the grid-stride loop; the box test is per element, so a quad may straddle rows.  Any
// other image length leaves the later images off 16-byte alignment: those tensors go one float at a time.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int MX_THREADS = 256;
constexpr int MX_BLOCKS = 256 * 8;               // 256 CUs x 8 workgroups of 4 waves: every SIMD holds 8 waves

struct MixArgs {
    const float* x; const int64_t* partner; float* out; int* status;
    long M; int n, H, W;                         // n = C * H * W floats per image
    int mode, bx0, by0, bx1, by1;
    float lam, u;
};

template <bool VEC>
__global__ __launch_bounds__(MX_THREADS) void mix_images_kernel(const MixArgs a) {
    constexpr int PX = VEC ? 4 : 1;
    const int nu = a.n / PX;                     // units (quads | floats) per image
    const long total = a.M * (long)nu, stride = (long)gridDim.x * MX_THREADS;
    for (long g = (long)blockIdx.x * MX_THREADS + threadIdx.x; g < total; g += stride) {
        const long i = g / nu;
        const int q = (int)(g - i * nu), e0 = q * PX;
        long p = a.partner[i];
        if (p < 0 || p >= a.M) { if (q == 0) atomicOr(a.status, FUMI_ST_LABEL_RANGE); p = i; }
        const float* xi = a.x + i * (long)a.n + e0;
        float* o = a.out + i * (long)a.n + e0;
        if (p == i) {                                                            // nothing to mix with: a copy
            if (VEC) *(f32x4*)o = *(const f32x4*)xi; else *o = *xi;
            continue;
        }
        const float* xp = a.x + p * (long)a.n + e0;
        float va[PX], vb[PX], r[PX];
        if (VEC) {
            const f32x4 ta = *(const f32x4*)xi, tb = *(const f32x4*)xp;
#pragma unroll
            for (int k = 0; k < PX; ++k) { va[k] = ta[k]; vb[k] = tb[k]; }
        } else { va[0] = *xi; vb[0] = *xp; }
        if (a.mode == 0) {
#pragma unroll
            for (int k = 0; k < PX; ++k) r[k] = a.lam * va[k] + a.u * vb[k];
        } else {
            const int line = e0 / a.W;                                           // c * H + row of the unit's first float
            int col = e0 - line * a.W, row = line % a.H;
#pragma unroll
            for (int k = 0; k < PX; ++k) {
                const bool in = row >= a.by0 && row < a.by1 && col >= a.bx0 && col < a.bx1;
                r[k] = in ? vb[k] : va[k];
                if (++col == a.W) { col = 0; if (++row == a.H) row = 0; }
            }
        }
        if (VEC) *(f32x4*)o = f32x4{r[0], r[1 % PX], r[2 % PX], r[3 % PX]}; else *o = r[0];
    }
}

}  // namespace

extern "C" int fumi_hip_mix_images(fumi_ws_t* ws, fumi_stream_t stream, int M, int C, int H, int W, const float* x,
        const int64_t* partner, int mode, float lam, int bx0, int by0, int bx1, int by1, float* out) {
    if (!ws || !x || !partner || !out || M < 1 || C < 1 || H < 1 || W < 1) return FUMI_EINVAL;
    if (mode != 0 && mode != 1) return FUMI_EINVAL;
    if (!(lam >= 0.f && lam <= 1.f)) return FUMI_EINVAL;
    if (mode == 1 && (bx0 < 0 || by0 < 0 || bx1 > W || by1 > H || bx1 < bx0 || by1 < by0)) return FUMI_EINVAL;
    const long n = (long)C * H * W;
    if (n > 0x7FFFFFFFL) return FUMI_ENOTSUP;
    const long bytes = (long)M * n * 4;
    const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
    if (xa < oa + (uintptr_t)bytes && oa < xa + (uintptr_t)bytes) return FUMI_EINVAL;       // row i reads row partner[i]
    HIP_TRY(hipSetDevice(ws->device));
    MixArgs a;
    a.x = x; a.partner = partner; a.out = out; a.status = ws->status;
    a.M = M; a.n = (int)n; a.H = H; a.W = W;
    a.mode = mode; a.bx0 = bx0; a.by0 = by0; a.bx1 = bx1; a.by1 = by1;
    a.lam = lam; a.u = 1.0f - lam;
    const bool vec = n % 4 == 0 && xa % 16 == 0 && oa % 16 == 0;
    const long units = (long)M * (vec ? n / 4 : n), want = (units + MX_THREADS - 1) / MX_THREADS;
    const unsigned blocks = (unsigned)(want < MX_BLOCKS ? want : MX_BLOCKS);
    if (vec) hipLaunchKernelGGL(mix_images_kernel<true>, dim3(blocks), dim3(MX_THREADS), 0, (hipStream_t)stream, a);
    else     hipLaunchKernelGGL(mix_images_kernel<false>, dim3(blocks), dim3(MX_THREADS), 0, (hipStream_t)stream, a);
    LAUNCH_CHECK();
    return FUMI_OK;
}
