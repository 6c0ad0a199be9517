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

template <int RULE>
__global__ __launch_bounds__(256) void optim_kernel(OptTensors<opt_nstate(RULE)> t, long total4, OptCoef c,
                                                    const float* __restrict__ pub_src, int pub_n, float* pub_dst,
                                                    unsigned long long pub_seq) {
    constexpr int NS = opt_nstate(RULE);
    // rider: a deferred publication of the step's statistics (sampler.hip: publish_scalars_kernel) saves its own launch
    if (pub_dst && blockIdx.x == gridDim.x - 1 && threadIdx.x < 64) {
        const int i = threadIdx.x;
        if (i < pub_n) __hip_atomic_store(pub_dst + i, pub_src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (i == 0) __hip_atomic_store((unsigned long long*)(pub_dst + 14), pub_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const bool rd0 = NS >= 1 && !(RULE == OPT_SGD_MOMENTUM && c.first);     // (a momentum buffer's first step writes it only)
    for (long i4 = blockIdx.x * (long)blockDim.x + threadIdx.x; i4 < total4; i4 += (long)gridDim.x * blockDim.x) {
        int k = 0;
        while (k + 1 < t.n && i4 >= t.end[k]) ++k;
        const long base4 = k ? t.end[k - 1] : 0;
        const long e0 = (i4 - base4) * 4;
        const long n = t.numel[k];
        float* p = t.p[k]; const float* g = t.g[k];
        float* s0 = nullptr; float* s1 = nullptr;
        if constexpr (NS >= 1) s0 = t.s[0][k];
        if constexpr (NS >= 2) s1 = t.s[1][k];
        const bool full = e0 + 3 < n && ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)s0 | (uintptr_t)s1) & 15) == 0);
        if (full) {
            f32x4 pp = *(f32x4*)(p + e0), gg = *(const f32x4*)(g + e0), aa = {0.f, 0.f, 0.f, 0.f}, bb = aa;
            if (rd0) aa = *(f32x4*)(s0 + e0);
            if constexpr (NS >= 2) bb = *(f32x4*)(s1 + e0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pp[e], ae = aa[e], be = bb[e];
                opt_update1<RULE>(gg[e], pe, ae, be, c);
                pp[e] = pe; aa[e] = ae; bb[e] = be;
            }
            *(f32x4*)(p + e0) = pp;
            if constexpr (NS >= 1) *(f32x4*)(s0 + e0) = aa;
            if constexpr (NS >= 2) *(f32x4*)(s1 + e0) = bb;
        } else {
            for (long e = e0; e < n && e < e0 + 4; ++e) {
                float pe = p[e], ae = 0.f, be = 0.f;
                if (rd0) ae = s0[e];
                if constexpr (NS >= 2) be = s1[e];
                opt_update1<RULE>(g[e], pe, ae, be, c);
                p[e] = pe;
                if constexpr (NS >= 1) s0[e] = ae;
                if constexpr (NS >= 2) s1[e] = be;
            }
        }
    }
}

template <int RULE> void optim_launch(fumi_ws* ws, hipStream_t st, const AdamPending& ap) {
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
    hipLaunchKernelGGL(optim_kernel<RULE>, dim3(blocks), dim3(256), 0, st, t, tot4, ap.c, ws->pub_src, ws->pub_n, ws->pub_dst, ws->pub_seq);
    ws->pub_dst = nullptr; ws->pub_src = nullptr;                 // a pending publication rode along
}

// one fused launch of the step `ap` describes
int optim_launch_any(fumi_ws* ws, hipStream_t st, const AdamPending& ap) {
    switch (ap.rule) {
        case OPT_ADAM: optim_launch<OPT_ADAM>(ws, st, ap); break;
        case OPT_ADAMW: optim_launch<OPT_ADAMW>(ws, st, ap); break;
        case OPT_SGD_MOMENTUM: optim_launch<OPT_SGD_MOMENTUM>(ws, st, ap); break;
        case OPT_SGD: optim_launch<OPT_SGD>(ws, st, ap); break;
        default: return FUMI_EINVAL;
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
    if (!ws->adam) { ws->adam = new AdamPending(); ws->adam->on = 0; }
    const int rc = optim_fill(ws->adam, rule, n_tensors, MAX_FOLD, params, grads, s0, s1, numel_host);
    if (rc) return rc;
    ws->adam->c = c;
    ws->adam->on = 1;
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
