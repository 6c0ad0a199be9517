// Fused multi-tensor Adam step (torch.optim.Adam semantics: coupled L2 weight decay, bias correction), one launch
// for every parameter tensor.  Replaces the optimizer.step() of fumi/models/fumi.py:193 (fumi/utils/utils.py:280-283:
// Adam(lr, weight_decay)), which torch runs as ~7 multi-tensor kernels.  Same operation order as torch's
// _single_tensor_adam so the parameters stay bit-comparable:
//   g += wd * p ; m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g g ; p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
// HBM-bound elementwise kernel: 16-byte accesses, 4 tensors' worth of traffic (p, g, m, v) per element.
// The same launch runs the reference's other outer optimizers (fumi/utils/utils.py:284-299), one template instance per rule, each
// in the operation order of torch's single-tensor implementation (element functions: common.h):
//   AdamW (torch.optim.AdamW): p *= 1 - lr wd, then Adam's moments and update on the raw gradient -- four streams as Adam;
//   SGD   (torch.optim.SGD, dampening 0, no Nesterov): g += wd p ; buf = g on a parameter's first step, else mu buf + g ;
//         p -= lr buf -- three streams (p, g, buf); two (p, g) when momentum == 0 and there is no buffer.
// Clipped form (torch.nn.utils.clip_grad_norm_, norm_type 2, ahead of any of the rules above): three kinds of
// launch that the stream alone orders -- grad_sumsq_kernel (one double partial per workgroup), clip_finish_kernel (the partials
// added in index order -> norm and coef as two device floats), optim_clipped_kernel (the rule on g * coef; g itself is only read).
#include "common.h"

namespace {

constexpr int MAXT = 32;
template <int NS> struct OptTensors {
    float* p[MAXT]; const float* g[MAXT]; float* s[NS][MAXT];   // s: the rule's state streams (Adam / AdamW: exp_avg, exp_avg_sq; SGD: buf)
    long end[MAXT];          // cumulative element counts rounded up to 4 per tensor (in float4 units)
    long numel[MAXT];        // element count per tensor (by value: no per-step host-to-device copy)
    int n;
};
template <> struct OptTensors<0> { float* p[MAXT]; const float* g[MAXT]; long end[MAXT]; long numel[MAXT]; int n; };

// g * coef of the clipped form: one fp32 multiply that rounds on its own (never the first half of an FMA with the rule's g + wd p)
__device__ __forceinline__ float clip_scale1(float g, float coef) {
#pragma clang fp contract(off)
    return g * coef;
}

// The step of both kernels below, as text: inside a device function blockDim.x compiles to the form for non-uniform workgroups and
// the plain kernel would no longer be the code it was.  CLIP: every gradient element is multiplied by COEF on its way into the rule.
// A deferred publication of the step's statistics (sampler.hip: publish_scalars_kernel) rides in the last workgroup and saves its
// own launch; a momentum buffer's first step writes it only (rd0).
#define OPTIM_STEP_BODY(CLIP, COEF) \
    constexpr int NS = opt_nstate(RULE);                                                                                            \
                                                                                                                                    \
    if (pub_dst && blockIdx.x == gridDim.x - 1 && threadIdx.x < 64) {                                                               \
        const int i = threadIdx.x;                                                                                                  \
        if (i < pub_n) __hip_atomic_store(pub_dst + i, pub_src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);                    \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                            \
        if (i == 0) __hip_atomic_store((unsigned long long*)(pub_dst + 14), pub_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  \
    }                                                                                                                               \
    const bool rd0 = NS >= 1 && !(RULE == OPT_SGD_MOMENTUM && c.first);                                                             \
    for (long i4 = blockIdx.x * (long)blockDim.x + threadIdx.x; i4 < total4; i4 += (long)gridDim.x * blockDim.x) {                  \
        int k = 0;                                                                                                                  \
        while (k + 1 < t.n && i4 >= t.end[k]) ++k;                                                                                  \
        const long base4 = k ? t.end[k - 1] : 0;                                                                                    \
        const long e0 = (i4 - base4) * 4;                                                                                           \
        const long n = t.numel[k];                                                                                                  \
        float* p = t.p[k]; const float* g = t.g[k];                                                                                 \
        float* s0 = nullptr; float* s1 = nullptr;                                                                                   \
        if constexpr (NS >= 1) s0 = t.s[0][k];                                                                                      \
        if constexpr (NS >= 2) s1 = t.s[1][k];                                                                                      \
        const bool full = e0 + 3 < n && ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)s0 | (uintptr_t)s1) & 15) == 0);                \
        if (full) {                                                                                                                 \
            f32x4 pp = *(f32x4*)(p + e0), gg = *(const f32x4*)(g + e0), aa = {0.f, 0.f, 0.f, 0.f}, bb = aa;                         \
            if (rd0) aa = *(f32x4*)(s0 + e0);                                                                                       \
            if constexpr (NS >= 2) bb = *(f32x4*)(s1 + e0);                                                                         \
_Pragma("unroll")                                                                                                                   \
            for (int e = 0; e < 4; ++e) {                                                                                           \
                float pe = pp[e], ae = aa[e], be = bb[e];                                                                           \
                opt_update1<RULE>((CLIP) ? clip_scale1(gg[e], COEF) : gg[e], pe, ae, be, c);                                        \
                pp[e] = pe; aa[e] = ae; bb[e] = be;                                                                                 \
            }                                                                                                                       \
            *(f32x4*)(p + e0) = pp;                                                                                                 \
            if constexpr (NS >= 1) *(f32x4*)(s0 + e0) = aa;                                                                         \
            if constexpr (NS >= 2) *(f32x4*)(s1 + e0) = bb;                                                                         \
        } else {                                                                                                                    \
            for (long e = e0; e < n && e < e0 + 4; ++e) {                                                                           \
                float pe = p[e], ae = 0.f, be = 0.f;                                                                                \
                if (rd0) ae = s0[e];                                                                                                \
                if constexpr (NS >= 2) be = s1[e];                                                                                  \
                opt_update1<RULE>((CLIP) ? clip_scale1(g[e], COEF) : g[e], pe, ae, be, c);                                          \
                p[e] = pe;                                                                                                          \
                if constexpr (NS >= 1) s0[e] = ae;                                                                                  \
                if constexpr (NS >= 2) s1[e] = be;                                                                                  \
            }                                                                                                                       \
        }                                                                                                                           \
    }

template <int RULE>
__global__ __launch_bounds__(256) void optim_kernel(OptTensors<opt_nstate(RULE)> t, long total4, OptCoef c,
                                                    const float* __restrict__ pub_src, int pub_n, float* pub_dst,
                                                    unsigned long long pub_seq) {
    OPTIM_STEP_BODY(false, 1.f)
}

// clipped form: `clip` = {norm, coef} as clip_finish_kernel left them, an earlier launch of the same stream; each workgroup reads coef once
template <int RULE>
__global__ __launch_bounds__(256) void optim_clipped_kernel(OptTensors<opt_nstate(RULE)> t, long total4, OptCoef c,
                                                            const float* __restrict__ clip, const float* __restrict__ pub_src,
                                                            int pub_n, float* pub_dst, unsigned long long pub_seq) {
    const float coef = clip[1];
    OPTIM_STEP_BODY(true, coef)
}

// ---- global gradient norm -----------------------------------------------------------------------------------------------------
constexpr int NORM_CAP = 1024;                // workgroups of one sum-of-squares launch (= partials it writes), at most
constexpr int CLIP_MAX_TENSORS = 256;         // tensors of a clipped step or a norm: CLIP_MAX_TENSORS / MAXT chunks of one table each
struct GradTensors { const float* g[MAXT]; long end[MAXT]; long numel[MAXT]; int n; };    // as OptTensors, the gradients alone

// parts[blockIdx.x] = sum of g^2 over the quads this workgroup's grid-stride loop visits, in double (a product of two floats is
// exact there).  Thread, lane and wave order are fixed and the grid depends on the element counts only: equal inputs, equal bits.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(GradTensors t, long total4, double* __restrict__ parts) {
    double acc = 0.0;
    for (long i4 = blockIdx.x * (long)blockDim.x + threadIdx.x; i4 < total4; i4 += (long)gridDim.x * blockDim.x) {
        int k = 0;
        while (k + 1 < t.n && i4 >= t.end[k]) ++k;
        const long base4 = k ? t.end[k - 1] : 0;
        const long e0 = (i4 - base4) * 4;
        const long n = t.numel[k];
        const float* g = t.g[k];
        const bool full = e0 + 3 < n && (((uintptr_t)g & 15) == 0);
        if (full) {
            const f32x4 gg = *(const f32x4*)(g + e0);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += (double)gg[e] * (double)gg[e];
        } else {
            for (long e = e0; e < n && e < e0 + 4; ++e) acc += (double)g[e] * (double)g[e];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_down(acc, off, 64);            // lanes: a fixed tree
    __shared__ double wsum[4];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) parts[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];    // waves: in order
}

// One workgroup: sum = parts[0] + parts[1] + ... in index order (staged through LDS by all threads, added by thread 0, so the order
// is no property of this kernel's shape); *norm_out = (float)sqrt(sum), and where coef_out is given torch's clip coefficient
// clamp(max_norm / (norm + 1e-6), max = 1) in fp32 -- the comparison that way round: a NaN norm gives a NaN coefficient.
__global__ __launch_bounds__(256) void clip_finish_kernel(const double* __restrict__ parts, int n_parts, float max_norm,
                                                          float* __restrict__ norm_out, float* __restrict__ coef_out) {
    __shared__ double tile[1024];
    double sum = 0.0;
    for (int base = 0; base < n_parts; base += 1024) {
        const int m = n_parts - base < 1024 ? n_parts - base : 1024;
        for (int i = threadIdx.x; i < m; i += 256) tile[i] = parts[base + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) sum += tile[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        const float norm = (float)sqrt(sum);
        *norm_out = norm;
        if (coef_out) {
            const float c = max_norm / (norm + 1e-6f);
            *coef_out = (c > 1.0f) ? 1.0f : c;
        }
    }
}

template <int RULE, bool CLIP = false> void optim_launch(fumi_ws* ws, hipStream_t st, const AdamPending& ap, const float* clip = nullptr) {
    constexpr int NS = opt_nstate(RULE);
    OptTensors<NS> t;
    long tot4 = 0;
    for (int k = 0; k < ap.n; ++k) {
        t.p[k] = ap.p[k]; t.g[k] = ap.g[k]; t.numel[k] = ap.numel[k];
        if constexpr (NS >= 1) t.s[0][k] = ap.s[0][k];
        if constexpr (NS >= 2) t.s[1][k] = ap.s[1][k];
        tot4 += (ap.numel[k] + 3) / 4;
        t.end[k] = tot4;
    }
    t.n = ap.n;
    int blocks = (int)((tot4 + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) return;
    if constexpr (CLIP)
        hipLaunchKernelGGL(optim_clipped_kernel<RULE>, dim3(blocks), dim3(256), 0, st, t, tot4, ap.c, clip, ws->pub_src, ws->pub_n, ws->pub_dst, ws->pub_seq);
    else
        hipLaunchKernelGGL(optim_kernel<RULE>, dim3(blocks), dim3(256), 0, st, t, tot4, ap.c, ws->pub_src, ws->pub_n, ws->pub_dst, ws->pub_seq);
    ws->pub_dst = nullptr; ws->pub_src = nullptr;                 // a pending publication rode along
}

// one fused launch of the step `ap` describes; `clip` (device {norm, coef}): its clipped form
int optim_launch_any(fumi_ws* ws, hipStream_t st, const AdamPending& ap, const float* clip = nullptr) {
    if (clip) {
        switch (ap.rule) {
            case OPT_ADAM: optim_launch<OPT_ADAM, true>(ws, st, ap, clip); break;
            case OPT_ADAMW: optim_launch<OPT_ADAMW, true>(ws, st, ap, clip); break;
            case OPT_SGD_MOMENTUM: optim_launch<OPT_SGD_MOMENTUM, true>(ws, st, ap, clip); break;
            case OPT_SGD: optim_launch<OPT_SGD, true>(ws, st, ap, clip); break;
            default: return FUMI_EINVAL;
        }
    } else {
        switch (ap.rule) {
            case OPT_ADAM: optim_launch<OPT_ADAM>(ws, st, ap); break;
            case OPT_ADAMW: optim_launch<OPT_ADAMW>(ws, st, ap); break;
            case OPT_SGD_MOMENTUM: optim_launch<OPT_SGD_MOMENTUM>(ws, st, ap); break;
            case OPT_SGD: optim_launch<OPT_SGD>(ws, st, ap); break;
            default: return FUMI_EINVAL;
        }
    }
    LAUNCH_CHECK();
    return FUMI_OK;
}

// checks the caller's host arrays and copies them into `ap` (s0 / s1: the rule's state streams, NULL where it has none)
int optim_fill(AdamPending* ap, int rule, int n_tensors, int max_tensors, float* const* params, const float* const* grads,
               float* const* s0, float* const* s1, const long* numel_host) {
    const int ns = opt_nstate(rule);
    if (!params || !grads || (ns >= 1 && !s0) || (ns >= 2 && !s1) || !numel_host || n_tensors < 1) return FUMI_EINVAL;
    if (n_tensors > max_tensors) return FUMI_ENOTSUP;
    for (int k = 0; k < n_tensors; ++k) {
        if (!params[k] || !grads[k] || (ns >= 1 && !s0[k]) || (ns >= 2 && !s1[k]) || numel_host[k] < 0) return FUMI_EINVAL;
        ap->p[k] = params[k]; ap->g[k] = grads[k]; ap->numel[k] = numel_host[k];
        ap->s[0][k] = ns >= 1 ? s0[k] : nullptr; ap->s[1][k] = ns >= 2 ? s1[k] : nullptr;
    }
    ap->n = n_tensors; ap->rule = rule;
    return FUMI_OK;
}

// Adam / AdamW: bias corrections (and AdamW's decay factor and 1 - beta) in double, as torch computes them in Python floats
OptCoef adam_coef(int rule, float lr, double beta1, double beta2, float eps, float weight_decay, int step) {
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    OptCoef c;
    c.lr = (float)(lr / bc1); c.a = (float)(1.0 / sqrt(bc2)); c.b1 = (float)beta1; c.b2 = (float)beta2; c.eps = eps;
    c.wd = rule == OPT_ADAMW ? (float)(1.0 - (double)lr * (double)weight_decay) : weight_decay;
    c.omb1 = (float)(1.0 - beta1); c.omb2 = (float)(1.0 - beta2);
    c.first = 0;
    return c;
}
OptCoef sgd_coef(float lr, float momentum, float weight_decay, int first_step) {
    OptCoef c;
    c.lr = lr; c.a = momentum; c.b1 = 0.f; c.b2 = 0.f; c.eps = 0.f; c.omb1 = 0.f; c.omb2 = 0.f; c.wd = weight_decay; c.first = first_step ? 1 : 0;
    return c;
}

constexpr int MAX_FOLD = 24;                  // segments of the final reduction (ReduceSegs, common.h)
int step_now(fumi_ws* ws, hipStream_t st, int rule, int n_tensors, float* const* params, const float* const* grads, float* const* s0,
             float* const* s1, const long* numel_host, const OptCoef& c) {
    AdamPending ap;
    const int rc = optim_fill(&ap, rule, n_tensors, MAXT, params, grads, s0, s1, numel_host);
    if (rc) return rc;
    ap.c = c;
    HIP_TRY(hipSetDevice(ws->device));
    return optim_launch_any(ws, st, ap);
}
int step_later(fumi_ws* ws, int rule, int n_tensors, float* const* params, const float* const* grads, float* const* s0,
               float* const* s1, const long* numel_host, const OptCoef& c) {
    AdamPending ap{};                             // filled aside: a refused call leaves a step that is already pending as it was
    const int rc = optim_fill(&ap, rule, n_tensors, MAX_FOLD, params, grads, s0, s1, numel_host);
    if (rc) return rc;
    ap.c = c;
    ap.on = 1;
    if (!ws->adam) ws->adam = new AdamPending();
    *ws->adam = ap;
    return FUMI_OK;
}

// The norm of up to CLIP_MAX_TENSORS gradient tensors: one sum-of-squares launch per chunk of MAXT tensors, each writing its
// partials behind the previous chunk's in the workspace's own buffer (never the slab: an AM3 encoder tape may be live there), then
// the finish launch.  coef_out NULL: the norm alone.  A tensor of no elements may have a NULL pointer (torch gives it one).
int norm_launch(fumi_ws* ws, hipStream_t st, int n_tensors, const float* const* grads, const long* numel_host, float max_norm,
                float* norm_out, float* coef_out) {
    if (!ws->clip_parts)
        if (hipMalloc((void**)&ws->clip_parts, (size_t)(CLIP_MAX_TENSORS / MAXT) * NORM_CAP * sizeof(double)) != hipSuccess) {
            ws->clip_parts = nullptr;
            return FUMI_ENOMEM;
        }
    int n_parts = 0;
    for (int k0 = 0; k0 < n_tensors; k0 += MAXT) {
        GradTensors t;
        long tot4 = 0;
        t.n = n_tensors - k0 < MAXT ? n_tensors - k0 : MAXT;
        for (int k = 0; k < t.n; ++k) {
            t.g[k] = grads[k0 + k]; t.numel[k] = numel_host[k0 + k];
            tot4 += (numel_host[k0 + k] + 3) / 4;
            t.end[k] = tot4;
        }
        long blocks = (tot4 + 255) / 256;
        if (blocks > NORM_CAP) blocks = NORM_CAP;
        if (blocks < 1) continue;
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3((int)blocks), dim3(256), 0, st, t, tot4, ws->clip_parts + n_parts);
        n_parts += (int)blocks;
    }
    hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(256), 0, st, ws->clip_parts, n_parts, max_norm, norm_out, coef_out);
    LAUNCH_CHECK();
    return FUMI_OK;
}

// NULL pointers are allowed exactly where a tensor has no elements
int clip_check(int rule, int n_tensors, float* const* params, const float* const* grads, float* const* s0, float* const* s1,
               const long* numel_host) {
    const int ns = rule >= 0 ? opt_nstate(rule) : 0;              // rule < 0: the gradients alone (fumi_hip_grad_norm)
    if ((rule >= 0 && !params) || !grads || (ns >= 1 && !s0) || (ns >= 2 && !s1) || !numel_host || n_tensors < 1) return FUMI_EINVAL;
    if (n_tensors > CLIP_MAX_TENSORS) return FUMI_ENOTSUP;
    for (int k = 0; k < n_tensors; ++k) {
        if (numel_host[k] < 0) return FUMI_EINVAL;
        if (numel_host[k] > 0 && ((rule >= 0 && !params[k]) || !grads[k] || (ns >= 1 && !s0[k]) || (ns >= 2 && !s1[k]))) return FUMI_EINVAL;
    }
    return FUMI_OK;
}

// norm launches, finish launch, then the rule's clipped launch per chunk of MAXT tensors, every chunk reading the same coef
int step_clipped(fumi_ws* ws, hipStream_t st, int rule, int n_tensors, float* const* params, const float* const* grads, float* const* s0,
                 float* const* s1, const long* numel_host, const OptCoef& c, float max_norm, float* clip_out) {
    if (!clip_out || !(max_norm > 0.f) || !(max_norm <= 3.402823466e+38f)) return FUMI_EINVAL;       // (NaN fails the first comparison)
    int rc = clip_check(rule, n_tensors, params, grads, s0, s1, numel_host);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ws->device));
    rc = norm_launch(ws, st, n_tensors, grads, numel_host, max_norm, clip_out, clip_out + 1);
    if (rc) return rc;
    const int ns = opt_nstate(rule);
    for (int k0 = 0; k0 < n_tensors; k0 += MAXT) {
        AdamPending ap;
        ap.n = n_tensors - k0 < MAXT ? n_tensors - k0 : MAXT; ap.rule = rule; ap.on = 0; ap.c = c;
        for (int k = 0; k < ap.n; ++k) {
            ap.p[k] = params[k0 + k]; ap.g[k] = grads[k0 + k]; ap.numel[k] = numel_host[k0 + k];
            ap.s[0][k] = ns >= 1 ? s0[k0 + k] : nullptr; ap.s[1][k] = ns >= 2 ? s1[k0 + k] : nullptr;
        }
        rc = optim_launch_any(ws, st, ap, clip_out);
        if (rc) return rc;
    }
    return FUMI_OK;
}

}  // namespace

int launch_adam_pending(fumi_ws* ws, hipStream_t st) {
    AdamPending* ap = ws ? ws->adam : nullptr;
    if (!ap || !ap->on) return FUMI_OK;
    ap->on = 0;
    return optim_launch_any(ws, st, *ap);
}

// Deferred forms: nothing is launched; the update is folded into the LAST launch of the next training meta-step of this workspace
// (fumi_hip_fumi_step / _indexed: the final reduction produces every gradient element, the rule's update follows element by element
// in the same thread) -- single GPU only: with several ranks the all-reduce lies between gradient and update.
// fumi_hip_adam_flush launches whatever is still pending as the ordinary kernel (a step that could not fold it, or none).
extern "C" int fumi_hip_adam_step_deferred(fumi_ws_t* ws, int n_tensors, float* const* params, const float* const* grads,
        float* const* exp_avg, float* const* exp_avg_sq, const long* numel_host,
        float lr, float beta1, float beta2, float eps, float weight_decay, int step) {
    if (!ws || step < 1) return FUMI_EINVAL;
    return step_later(ws, OPT_ADAM, n_tensors, params, grads, exp_avg, exp_avg_sq, numel_host,
                      adam_coef(OPT_ADAM, lr, beta1, beta2, eps, weight_decay, step));
}

extern "C" int fumi_hip_adamw_step_deferred(fumi_ws_t* ws, int n_tensors, float* const* params, const float* const* grads,
        float* const* exp_avg, float* const* exp_avg_sq, const long* numel_host,
        float lr, double beta1, double beta2, float eps, float weight_decay, int step) {
    if (!ws || step < 1) return FUMI_EINVAL;
    return step_later(ws, OPT_ADAMW, n_tensors, params, grads, exp_avg, exp_avg_sq, numel_host,
                      adam_coef(OPT_ADAMW, lr, beta1, beta2, eps, weight_decay, step));
}

extern "C" int fumi_hip_sgd_step_deferred(fumi_ws_t* ws, int n_tensors, float* const* params, const float* const* grads,
        float* const* momentum_buf, const long* numel_host, float lr, float momentum, float weight_decay, int first_step) {
    if (!ws || (momentum != 0.f && !momentum_buf)) return FUMI_EINVAL;
    return step_later(ws, momentum != 0.f ? OPT_SGD_MOMENTUM : OPT_SGD, n_tensors, params, grads, momentum_buf, nullptr, numel_host,
                      sgd_coef(lr, momentum, weight_decay, first_step));
}

// *launched = 1 when the pending step was still to do (it is launched now, as the plain kernel), 0 when a meta-step had folded it
extern "C" int fumi_hip_adam_flush(fumi_ws_t* ws, fumi_stream_t stream, int* launched) {
    if (!ws) return FUMI_EINVAL;
    const int pending = ws->adam && ws->adam->on;
    if (launched) *launched = pending;
    if (!pending) return FUMI_OK;
    HIP_TRY(hipSetDevice(ws->device));
    return launch_adam_pending(ws, (hipStream_t)stream);
}

extern "C" int fumi_hip_adam_step(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, float* const* params,
        const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const long* numel_host,
        float lr, float beta1, float beta2, float eps, float weight_decay, int step) {
    if (!ws || step < 1) return FUMI_EINVAL;
    return step_now(ws, (hipStream_t)stream, OPT_ADAM, n_tensors, params, grads, exp_avg, exp_avg_sq, numel_host,
                    adam_coef(OPT_ADAM, lr, beta1, beta2, eps, weight_decay, step));
}

extern "C" int fumi_hip_adamw_step(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, float* const* params,
        const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const long* numel_host,
        float lr, double beta1, double beta2, float eps, float weight_decay, int step) {
    if (!ws || step < 1) return FUMI_EINVAL;
    return step_now(ws, (hipStream_t)stream, OPT_ADAMW, n_tensors, params, grads, exp_avg, exp_avg_sq, numel_host,
                    adam_coef(OPT_ADAMW, lr, beta1, beta2, eps, weight_decay, step));
}

extern "C" int fumi_hip_sgd_step(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, float* const* params,
        const float* const* grads, float* const* momentum_buf, const long* numel_host, float lr, float momentum, float weight_decay,
        int first_step) {
    if (!ws || (momentum != 0.f && !momentum_buf)) return FUMI_EINVAL;
    return step_now(ws, (hipStream_t)stream, momentum != 0.f ? OPT_SGD_MOMENTUM : OPT_SGD, n_tensors, params, grads, momentum_buf, nullptr,
                    numel_host, sgd_coef(lr, momentum, weight_decay, first_step));
}

// The global L2 norm of the gradients alone (the first two stages of a clipped step): *norm_out, a DEVICE float.
extern "C" int fumi_hip_grad_norm(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, const float* const* grads, const long* numel_host,
        float* norm_out) {
    if (!ws || !norm_out) return FUMI_EINVAL;
    const int rc = clip_check(-1, n_tensors, nullptr, grads, nullptr, nullptr, numel_host);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ws->device));
    return norm_launch(ws, (hipStream_t)stream, n_tensors, grads, numel_host, 0.f, norm_out, nullptr);
}

// Clipped forms: clip_out[0] = norm of all gradients, clip_out[1] = coef = min(1, max_norm / (norm + 1e-6)); the rule then sees
// g * coef.  Up to 256 tensors; the gradients are read only.  No deferred form: the norm needs every gradient element first.
extern "C" int fumi_hip_adam_step_clipped(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, float* const* params,
        const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const long* numel_host,
        float lr, float beta1, float beta2, float eps, float weight_decay, int step, float max_norm, float* clip_out) {
    if (!ws || step < 1) return FUMI_EINVAL;
    return step_clipped(ws, (hipStream_t)stream, OPT_ADAM, n_tensors, params, grads, exp_avg, exp_avg_sq, numel_host,
                        adam_coef(OPT_ADAM, lr, beta1, beta2, eps, weight_decay, step), max_norm, clip_out);
}

extern "C" int fumi_hip_adamw_step_clipped(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, float* const* params,
        const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const long* numel_host,
        float lr, double beta1, double beta2, float eps, float weight_decay, int step, float max_norm, float* clip_out) {
    if (!ws || step < 1) return FUMI_EINVAL;
    return step_clipped(ws, (hipStream_t)stream, OPT_ADAMW, n_tensors, params, grads, exp_avg, exp_avg_sq, numel_host,
                        adam_coef(OPT_ADAMW, lr, beta1, beta2, eps, weight_decay, step), max_norm, clip_out);
}

extern "C" int fumi_hip_sgd_step_clipped(fumi_ws_t* ws, fumi_stream_t stream, int n_tensors, float* const* params,
        const float* const* grads, float* const* momentum_buf, const long* numel_host, float lr, float momentum, float weight_decay,
        int first_step, float max_norm, float* clip_out) {
    if (!ws || (momentum != 0.f && !momentum_buf)) return FUMI_EINVAL;
    return step_clipped(ws, (hipStream_t)stream, momentum != 0.f ? OPT_SGD_MOMENTUM : OPT_SGD, n_tensors, params, grads, momentum_buf,
                        nullptr, numel_host, sgd_coef(lr, momentum, weight_decay, first_step), max_norm, clip_out);
}
